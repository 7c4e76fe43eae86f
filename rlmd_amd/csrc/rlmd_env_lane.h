// rlmd_env_lane.h — the lane model: one step and one reset of one lane of the
// batched environments, as device functions (the part oracle/envs.py mirrors
// line by line; env.hip holds the kernels that call it).
//
// Reference semantics restated (file:line into majidsina/rlmd):
//   coin   envs/coin_flip_envs.py:150-216 (A), :290-362 (B, stop-loss = |a0| :308),
//          :436-521 (C); consts :40-93
//   dice   envs/dice_roll_envs.py:153-219, :293-365, :439-524; consts :39-96
//   gbm    envs/gbm_envs.py:147-212, :286-357, :431-515; consts :43-90
//   dice_sh envs/dice_roll_sh_envs.py:160-235 (INSURED), :290-365, :420-502, :557-645
//   market envs/market_envs.py:133-202 (D1), :611-682 (Dx) + B/C variants
//   dones  tools/env_resources.py:26-80 (any lev_max), :83-137 (all), :140-200 (market)
//   slicing tools/env_resources.py:203-291 (observed_market_state/time_slice/shuffle_data)
//
// Precision follows the reference's dtype flow under NumPy 2 for f32 actions
// (restated and pinned bit-exactly in oracle/envs.py): wealth and
// returns f64; GBM / market leverages f32 (`f32 * Python int`), coin / dice
// leverages f64 (`f32 * np.float64`); stop-loss, retention, safe-haven leverage,
// `1e4 * stop_loss`, `max(., MIN_VALUE)` and the first-step bet size f32;
// Dice_SH_INSURED leverage f32.  FP contraction is off so every rounding happens
// where NumPy's does: hence the pragma below, and include this header only from
// translation units that build.py compiles with -ffp-contract=off (a contracted
// multiply-add in a caller's lambda inlined into the step changes wealth bits).
#pragma once
#pragma clang fp contract(off)
#include <math.h>
#include "../../include/rlmd_abi.h"
#include "rlmd_common.h"

namespace {

constexpr double kInitialValue = 1e4;
constexpr double kMinValue = 100.0;  // max(MIN_VALUE_RATIO * INITIAL_VALUE, 1)
constexpr double kMaxAbsAction = 0.99;
constexpr double kMinWeight = 1e-5;

struct FamConst {
  double max_value, min_reward, min_return, max_return, lev_factor;
};

__host__ __device__ constexpr FamConst fam_const(int fam) {
  switch (fam) {
    case RLMD_COIN: return {1e18, 1e-3, -0.9, 1e10, 2.0};
    case RLMD_DICE: return {1e18, 1e-3, -0.9, 1e10, 2.0};
    case RLMD_GBM: return {1e18, 1e-3, -2.3025850929940455 /* np.log(0.1) */, 1e10, 5.0};
    case RLMD_DICE_SH: return {1e18, 1e-6, -0.99, 1e10, 2.0};
    default: return {1e34, 1e-3, -0.9, 1e10, 3.0};
  }
}

// GBM: LOG_MEAN = DRIFT - VOL**2 / 2 (envs/gbm_envs.py:43-63)
constexpr double kGbmDrift = 0.0540025395205692;
constexpr double kGbmVol = 0.1897916175617430;
// dice_sh: I_LEV_FACTOR = (-1 - 5) / (-0.5 - 5) (envs/dice_roll_sh_envs.py:70)
constexpr double kShILev = (-1.0 - 5.0) / (-0.5 - 5.0);

struct EnvParams {
  int fam, inv, n_lanes, n, obs_days, time_length, action_days, shuffle_days;
  int state_dim, action_dim, risk_dim, draw_dim, ext_len, start_range, n_days;
  int slice_groups;  // market: lanes sharing slice draws in groups (lane % G; 0 = per lane)
  // replay rows store s = s' from an episode's second step on: the reference's
  // coin / dice / GBM / market envs return one self.next_state array mutated in
  // place (e.g. gbm_envs.py:125, 184-186, 212), its loop keeps state = next_state
  // (rl_multiplicative.py:245, rl_market.py:273) and stores state after the
  // next env.step (:218-220; replay.py:164-167 copies then); reset() returns a
  // fresh array (gbm_envs.py:224-229), so an episode's first row keeps the reset
  // state.  Dice_SH builds a new array per step (dice_roll_sh_envs.py:336): 0.
  int alias_state;
  uint64_t seed;
  const double* prices;  // market [n_days, n]
  // lane state
  double* wealth;
  int32_t* time;
  int32_t* start;
  uint32_t* episode;
  // per-episode log of the fused train step (nullable): one region of ep_cap
  // rows [step, lane, final reward, length, risk...] (ep_w floats) per wave,
  // ep_cnt[wave] = rows appended since the last drain (counts past ep_cap too)
  float* ep_rows;
  uint32_t* ep_cnt;
  int ep_cap, ep_w;
};

// --- categorical outcome from a uniform: NumPy legacy choice(a, p) =
// a[searchsorted(cumsum(p)/cumsum(p)[-1], u, 'right')] (pinned by tests/golden/rng_kat.npz).
__device__ __host__ inline double coin_outcome(double u) {
  const double c0 = 0.5, c1 = 0.5 + 0.5;
  const int idx = (c0 / c1 <= u) + (c1 / c1 <= u);
  return idx == 0 ? 0.5 : -0.4;
}
__device__ __host__ inline int dice_index(double u) {
  const double p0 = 1.0 / 6.0, p1 = 1.0 / 6.0, p2 = 1.0 - (1.0 / 6.0 + 1.0 / 6.0);
  const double c0 = p0, c1 = c0 + p1, c2 = c1 + p2;
  return (c0 / c2 <= u) + (c1 / c2 <= u) + (c2 / c2 <= u);
}
__device__ __host__ inline double dice_value(int idx) {
  return idx == 0 ? 0.5 : (idx == 1 ? -0.5 : 0.05);
}

// Fisher–Yates permutation of a block of `bs` (<= 16) rows for market shuffles.
// The permutation lives in one 64-bit register as 16 four-bit entries (no
// per-thread array, hence no scratch).
__device__ inline int market_perm(uint64_t seed, uint32_t lane, uint32_t ep, uint32_t blk, int bs,
                                  int pos) {
  uint64_t p = 0xFEDCBA9876543210ull;  // entry i = i
  rlmd_u32x4 w = {0, 0, 0, 0};
  for (int i = bs - 1, k = 0; i >= 1; --i, ++k) {
    if ((k & 3) == 0) w = rlmd_philox(seed, lane, ep, RLMD_TAG_MKT_PERM, blk * 4u + (k >> 2));
    const uint32_t word = (k & 3) == 0 ? w.x : (k & 3) == 1 ? w.y : (k & 3) == 2 ? w.z : w.w;
    const int j = (int)(((uint64_t)word * (uint64_t)(i + 1)) >> 32);
    const uint64_t pi = (p >> (4 * i)) & 15u, pj = (p >> (4 * j)) & 15u;
    p &= ~((15ull << (4 * i)) | (15ull << (4 * j)));
    p |= (pj << (4 * i)) | (pi << (4 * j));
  }
  return (int)((p >> (4 * pos)) & 15u);
}

// the Philox counter of a lane's market slice draws (start row, block shuffles)
__device__ inline uint32_t slice_key(const EnvParams& P, uint32_t lane) {
  return P.slice_groups > 0 ? lane % (uint32_t)P.slice_groups : lane;
}

// source price row of extract row e (time_slice + shuffle_data)
__device__ inline int market_row(const EnvParams& P, uint32_t lane, int start, uint32_t ep, int e) {
  const int D = P.shuffle_days;
  if (D <= 1) return start + e;
  const int full = P.ext_len / D, blk = e / D, within = e % D;
  const int bs = blk < full ? D : P.ext_len - full * D;
  return start + blk * D + market_perm(P.seed, slice_key(P, lane), ep, (uint32_t)blk, bs, within);
}

// observed_market_state element k (tools/env_resources.py:203-226): D1 -> row t*ad
// asset k; Dx -> rows [t*ad, t*ad+d) flattened then reversed.
__device__ inline double market_obs(const EnvParams& P, uint32_t lane, int start, uint32_t ep,
                                    int t, int k) {
  int row, asset;
  if (P.obs_days == 1) {
    row = t * P.action_days;
    asset = k;
  } else {
    const int f = P.obs_days * P.n - 1 - k;
    row = t * P.action_days + f / P.n;
    asset = f % P.n;
  }
  return P.prices[(int64_t)market_row(P, lane, start, ep, row) * P.n + asset];
}

// np.sum / np.mean of a small array: NumPy's pairwise_sum for n <= 128
// (sequential below 8 elements, 8 accumulators otherwise).
template <typename T, typename GetF>
__device__ inline T np_sum(int n, GetF get) {
  T res;
  if (n < 8) {
    res = (T)0;
    for (int i = 0; i < n; ++i) res += get(i);
  } else {
    T r[8];
    for (int k = 0; k < 8; ++k) r[k] = get(k);
    int i = 8;
    for (; i < n - (n % 8); i += 8)
      for (int k = 0; k < 8; ++k) r[k] += get(i + k);
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += get(i);
  }
  return res;
}
template <typename T, typename GetF>
__device__ inline T np_mean(int n, GetF get) {
  return np_sum<T>(n, get) / (T)n;
}

struct StepOut {
  double W, reward;
  bool done, learn_done;
};

struct NoDoneHook {
  __device__ void operator()(const StepOut&) const {}
};

// market: the action-independent relative prices obs(t, k) / obs(0, k) - 1 of a
// step, when a caller has them precomputed (kOn); otherwise read in the step
struct NoMrel {
  static constexpr bool kOn = false;
  __device__ double operator()(int) const { return 0.0; }
};
struct MrelRow {
  static constexpr bool kOn = true;
  const double* row;
  __device__ double operator()(int k) const { return row[k]; }
};

// One env step for one lane.  `act(i)` yields action i as AT, `draw(j)` the
// j-th uniform/normal.  Writes state element k through st(k, v) and risk
// element k through rk(k, v).
// AT is the dtype of the action array the reference's env.step receives: f32
// from the policy / warm-up sampler, f64 inside the smoothing window (np.clip
// with np.float64 bounds promotes, utils.py:345-373).  Every action-derived
// quantity follows NumPy 2's promotion from it: with f32 actions, GBM/market
// leverage (x Python int) and the half-shifted stop-loss / retention / safe-haven
// weights stay f32; with f64 actions everything is f64.
//
// FAM (the env family) is a template parameter, so each family's kernel holds
// only its own code; NG > 0 fixes n_gambles / n_assets at compile time (the
// n == 1 configurations), NG == 0 reads it from P.
template <int FAM, int NG, typename AT, typename ActF, typename DrawF, typename StF, typename RkF,
          typename DoneF = NoDoneHook, typename MrelF = NoMrel>
__device__ inline StepOut env_step_lane(const EnvParams& P, uint32_t lane, double w0, int t,
                                        int start, uint32_t ep, ActF act, DrawF draw, StF st,
                                        RkF rk, DoneF on_done = DoneF{}, MrelF mrel = MrelF{}) {
  constexpr FamConst C = fam_const(FAM);
  constexpr int fam = FAM;
  const int inv = P.inv, n = NG ? NG : P.n;
  const bool use_all = (fam == RLMD_GBM || fam == RLMD_MARKET);  // lev_max: np.all (Q4)
  const bool f32lev = use_all && sizeof(AT) == 4;                // lev = f32 action * int
  const double lev_cap64 = kMaxAbsAction * C.lev_factor;
  const float lev_cap32 = (float)lev_cap64;
  auto half_shift = [](AT a) -> AT { return (a + (AT)kMaxAbsAction) / (AT)2; };

  AT sl32 = (AT)NAN, ret32 = (AT)NAN, lev_sh32 = (AT)NAN;
  double R = 0.0, lev_mean = 0.0, lev0 = 0.0, r_sh = 0.0, r_die = 0.0;
  bool lev_max_any = false, lev_max_all = true, lev_min_all = true;
  int lev_off = 0;

  if (fam == RLMD_DICE_SH) {
    const int idx = dice_index(draw(0));
    r_die = dice_value(idx);
    r_sh = idx == 2 ? -0.99 : (idx == 0 ? -0.99 : 5.0);  // MID, UP -> -0.99 ; DOWN -> 5
    double lev;
    if (inv == RLMD_INV_INSURED) {
      const AT lev32 = act(0) * (AT)kShILev;  // action * Python float
      lev = (double)lev32;
      lev_sh32 = (AT)1 - lev32;
      lev_min_all = fabs(lev32) < (AT)kMinWeight;
    } else {
      const int ai = inv == RLMD_INV_A ? 0 : (inv == RLMD_INV_B ? 1 : 2);
      if (inv != RLMD_INV_A) sl32 = half_shift(act(0));
      if (inv == RLMD_INV_C) ret32 = half_shift(act(1));
      lev = (double)act(ai) * C.lev_factor;
      lev_sh32 = half_shift(act(ai + 1)) * (AT)1;
      lev_min_all = fabs(lev) < kMinWeight;
    }
    lev_max_any = fabs(lev) == lev_cap64;
    R = lev * r_die + (double)(lev_sh32 * (AT)r_sh);
    lev_mean = lev;
    lev0 = lev;
  } else {
    if (inv == RLMD_INV_B) {
      sl32 = fam == RLMD_COIN ? (AT)fabs(act(0)) : half_shift(act(0));  // Coin_InvB: |a0| (Q1)
      lev_off = 1;
    } else if (inv == RLMD_INV_C) {
      sl32 = half_shift(act(0));
      ret32 = half_shift(act(1));
      lev_off = 2;
    }
    auto ret_of = [&](int j) -> double {
      if (fam == RLMD_COIN) return coin_outcome(draw(j));
      if (fam == RLMD_DICE) return dice_value(dice_index(draw(j)));
      if (fam == RLMD_GBM) return (kGbmDrift - kGbmVol * kGbmVol / 2) + kGbmVol * draw(j);
      if constexpr (MrelF::kOn) return mrel(j);
      return market_obs(P, lane, start, ep, t, j) / market_obs(P, lane, start, ep, 0, j) - 1.0;
    };
    auto lev_of = [&](int j) -> double {
      const AT a = act(lev_off + j);
      return f32lev ? (double)((float)a * (float)C.lev_factor) : (double)a * C.lev_factor;
    };
    R = np_sum<double>(n, [&](int j) { return lev_of(j) * ret_of(j); });  // np.sum(lev * r)
    for (int j = 0; j < n; ++j) {
      const AT a = act(lev_off + j);
      if (f32lev) {
        const float l32 = (float)a * (float)C.lev_factor;
        lev_max_all &= fabsf(l32) == lev_cap32;
        lev_min_all &= fabsf(l32) < (float)kMinWeight;
      } else {
        const double lev = (double)a * C.lev_factor;
        lev_max_all &= fabs(lev) == lev_cap64;
        lev_max_any |= fabs(lev) == lev_cap64;
        lev_min_all &= fabs(lev) < kMinWeight;
      }
    }
    lev0 = lev_of(0);
    if (f32lev)
      lev_mean = (double)np_mean<float>(n, [&](int j) { return (float)act(lev_off + j) * (float)C.lev_factor; });
    else
      lev_mean = np_mean<double>(n, [&](int j) { return (double)act(lev_off + j) * C.lev_factor; });
  }

  // one-step return and growth factor
  double g;
  if (fam == RLMD_GBM) {
    R = fmax(R, C.min_return);
    g = fmin(exp(R), 1.0 + C.max_return);
  } else {
    R = fmin(fmax(R, C.min_return), C.max_return);
    g = 1.0 + R;
  }

  double W, mw;
  bool done_active = false;
  if (inv == RLMD_INV_A || inv == RLMD_INV_INSURED) {
    mw = kMinValue;
    W = fmin(fmax(w0 * g, kMinValue), C.max_value);
  } else {
    const AT mw32 = fmax((AT)kInitialValue * sl32, (AT)kMinValue);
    if (inv == RLMD_INV_C && w0 > kInitialValue)
      mw = kInitialValue + (w0 - kInitialValue) * (double)ret32;
    else
      mw = (double)mw32;
    // episode's first step: wealth is still the Python float 1e4 -> f32 subtraction
    const double active = t == 1 ? (double)fmax((AT)kInitialValue - mw32, (AT)0) : fmax(w0 - mw, 0.0);
    W = fmin(fmax(mw + active * g, mw), C.max_value);
    done_active = active == 0.0;
  }
  const double growth = W / kInitialValue;
  const double reward = exp(log(growth) / (double)t);

  // next state / MAX_VALUE (and done_state = any(next_state >= 1))
  bool done_state = false;
  auto put = [&](int k, double v) {
    const double s = v / C.max_value;
    done_state |= s >= 1.0;
    st(k, s);
  };
  put(0, W);
  put(1, R);
  put(2, growth);
  put(3, reward);
  if (fam == RLMD_DICE_SH) {
    put(4, r_die);
    put(5, r_sh);
  } else if (fam == RLMD_MARKET) {
    const int m = P.obs_days * n;
    for (int k = 0; k < m; ++k)
      put(4 + k, MrelF::kOn ? mrel(k)
                            : market_obs(P, lane, start, ep, t, k) / market_obs(P, lane, start, ep, 0, k) - 1.0);
  } else {
    for (int j = 0; j < n; ++j) {
      double r;
      if (fam == RLMD_COIN) r = coin_outcome(draw(j));
      else if (fam == RLMD_DICE) r = dice_value(dice_index(draw(j)));
      else r = (kGbmDrift - kGbmVol * kGbmVol / 2) + kGbmVol * draw(j);
      put(4 + j, r);
    }
  }

  const bool lev_max = use_all ? lev_max_all : lev_max_any;
  const bool done_time = fam == RLMD_MARKET &&
                         t == (P.obs_days == 1 ? P.time_length : P.time_length - P.obs_days + 1);
  const bool done = done_time || W == mw || reward < C.min_reward || R == C.min_return || lev_max ||
                    lev_min_all || done_state || done_active;
  StepOut o;
  o.W = W;
  o.reward = reward;
  o.done = done;
  o.learn_done = done && !done_state && !done_time;
  on_done(o);  // the done flags are known before the risk vector is emitted

  // risk vector
  rk(0, reward);
  rk(1, W);
  rk(2, R);
  if (fam == RLMD_DICE_SH) {
    rk(3, lev0);
    rk(4, (double)sl32);
    rk(5, (double)ret32);
    rk(6, (double)lev_sh32);
  } else {
    rk(3, lev_mean);
    int k = 4;
    if (inv == RLMD_INV_B || inv == RLMD_INV_C) rk(k++, (double)sl32);
    if (inv == RLMD_INV_C) rk(k++, (double)ret32);
    if (n > 1) {
      for (int j = 0; j < n; ++j) {
        const AT a = act(lev_off + j);
        rk(k + j, f32lev ? (double)((float)a * (float)C.lev_factor) : (double)a * C.lev_factor);
      }
    }
  }
  return o;
}

// draws for gamble j: Philox(seed, lane, step, ENV_DRAW, j/2), two per block
template <int FAM>
__device__ inline double philox_draw(const EnvParams& P, uint32_t lane, uint32_t step, int j) {
  const rlmd_u32x4 v = rlmd_philox(P.seed, lane, step, RLMD_TAG_ENV_DRAW, (uint32_t)(j >> 1));
  if (FAM == RLMD_GBM) {
    double z0, z1;
    rlmd_normal2(v, z0, z1);
    return (j & 1) ? z1 : z0;
  }
  return (j & 1) ? rlmd_u01(v.z, v.w) : rlmd_u01(v.x, v.y);
}

// reset one lane: episode start (market: new slice), state element writer
// start_at >= 0 (market): the episode's first price row is given (eval_market's
// gap index) instead of drawn.
// ep_now >= 0: the lane's current episode counter, already in a register (the
// training step's epilogue loaded it with the lane state; re-reading it here put
// a dependent global load into the tail of every wave with a finished lane).
template <int FAM, typename StF>
__device__ inline void env_reset_lane(const EnvParams& P, uint32_t lane, StF st, int start_at = -1,
                                      int64_t ep_now = -1) {
  P.wealth[lane] = kInitialValue;
  P.time[lane] = 1;
  const uint32_t ep = (ep_now >= 0 ? (uint32_t)ep_now : P.episode[lane]) + 1;
  P.episode[lane] = ep;
  constexpr FamConst C = fam_const(FAM);
  st(0, kInitialValue / C.max_value);
  st(1, 0.0);
  st(2, 1.0 / C.max_value);
  st(3, 1.0 / C.max_value);
  if (FAM == RLMD_MARKET) {
    const rlmd_u32x4 v = rlmd_philox(P.seed, slice_key(P, lane), ep, RLMD_TAG_MKT_START, 0);
    const int start = start_at >= 0 ? start_at : (int)rlmd_below(v.x, v.y, (uint64_t)P.start_range);
    P.start[lane] = start;
    const int m = P.obs_days * P.n;
    for (int k = 0; k < m; ++k)
      st(4 + k, P.obs_days == 1 ? 0.0 : market_obs(P, lane, start, ep, 0, k) / C.max_value);
  } else {
    for (int k = 4; k < P.state_dim; ++k) st(k, 0.0);
  }
}

}  // namespace
