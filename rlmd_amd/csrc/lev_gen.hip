// lev_gen.hip — the leverage experiments' outcome matrices, drawn on the device (gfx950).
//
// Replaces the Bernoulli / Categorical / Normal tensors of lev/coin_flip.py:160-161,
// lev/dice_roll.py:147-148 and lev/gbm.py:123-124 (f32 / int64 / f32 [investors][horizon],
// 12 - 40 GB at the reference's sizes) with the u8 / f32 matrix the sweeps read, filled in
// place.  Element (i, j) is a pure function of its index:
//   v = Philox4x32-10(seed, (first_investor + i, stream, RLMD_TAG_LEV_OUTCOME, j >> 1))
//   categorical  u = u01(v.x, v.y) (even j) or u01(v.z, v.w) (odd j); class
//                (t0 <= u) + (t1 <= u); the element is the class's code.  u is the 53-bit
//                integer k = (a >> 5) << 26 | (b >> 6) scaled by 2^-53, so t <= u is
//                ceil(t 2^53) <= k exactly: the host turns the thresholds into integers
//                and the kernel compares integers (no f64 on the device);
//   normal       (float)(log_mean + vol * z), z the block's Box-Muller pair (z0 even j,
//                z1 odd j), in f64, rounded once.
// oracle/philox.py's uniform_draws / normal_draws regenerate the same draws.
//
// Shape: a thread owns a run of 16 consecutive steps of one investor = 8 Philox blocks,
// and stores them as one 16-byte vector (u8) or four (f32); consecutive threads own
// consecutive runs of the same row, so a wave's u8 stores cover 1 KiB of one row.  A
// workgroup takes whole rows (rows_per_block x runs slots, >= 2048 where the matrix has
// them) so a short row does not leave lanes idle.  The ragged last run and the pad
// columns horizon .. ld - 1 (written as 0) are predicated.  By count the kernel is bound
// by Philox's 32-bit multiplies (40 per block, quarter rate), not by its stores.
#include <math.h>

#include "rlmd_common.h"
#include "rlmd_internal.h"

namespace {

constexpr int kRun = 16;         // steps per thread
constexpr int kThreads = 256;    // workgroup
constexpr int kSlots = 2048;     // runs a workgroup aims to hold (8 per thread)

struct GenArgs {
  uint64_t seed;
  uint64_t t0, t1;  // categorical: ceil(threshold * 2^53)
  double log_mean, vol;
  int64_t investors, ld;
  uint32_t stream, lane0, runs, rows_per_block, codes;
  int32_t horizon;
};

__device__ __forceinline__ uint32_t cat_code(uint32_t a, uint32_t b, const GenArgs& g) {
  const uint64_t k = ((uint64_t)(a >> 5) << 26) | (uint64_t)(b >> 6);
  const uint32_t cls = (uint32_t)(k >= g.t0) + (uint32_t)(k >= g.t1);
  return (g.codes >> (8u * cls)) & 0xFFu;
}

// VEC: bytes per store (16 / 4 need the base and ld aligned to VEC; 1 takes any view)
template <int VEC>
__global__ __launch_bounds__(kThreads) void lev_gen_cat_kernel(GenArgs g, uint8_t* __restrict__ out) {
  const int64_t row0 = (int64_t)blockIdx.x * g.rows_per_block;
  const int64_t left = g.investors - row0;
  const uint32_t rows = left < (int64_t)g.rows_per_block ? (uint32_t)left : g.rows_per_block;
  const uint32_t slots = rows * g.runs;
  for (uint32_t l = threadIdx.x; l < slots; l += kThreads) {
    const uint32_t rl = l / g.runs, run = l - rl * g.runs;
    const int64_t row = row0 + rl;
    const uint32_t c0 = g.lane0 + (uint32_t)row;
    const int64_t s0 = (int64_t)run * kRun;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int b = 0; b < kRun / 2; ++b) {
      const int64_t s = s0 + 2 * b;
      if (s < g.horizon) {
        const rlmd_u32x4 v = rlmd_philox(g.seed, c0, g.stream, RLMD_TAG_LEV_OUTCOME, (uint32_t)(s >> 1));
        uint32_t pair = cat_code(v.x, v.y, g);
        if (s + 1 < g.horizon) pair |= cat_code(v.z, v.w, g) << 8;
        w[b >> 1] |= pair << (16 * (b & 1));
      }
    }
    uint8_t* p = out + row * g.ld + s0;
    if constexpr (VEC == 16) {
      *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);  // ld % 16 == 0: the run is inside the row
    } else if constexpr (VEC == 4) {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (s0 + 4 * q < g.ld) *reinterpret_cast<uint32_t*>(p + 4 * q) = w[q];  // ld % 4 == 0
    } else {
#pragma unroll
      for (int j = 0; j < kRun; ++j)
        if (s0 + j < g.ld) p[j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
    }
  }
}

// VEC: 16-byte stores (base 16-byte aligned, ld % 4 == 0) or one f32 at a time
template <bool VEC>
__global__ __launch_bounds__(kThreads) void lev_gen_normal_kernel(GenArgs g, float* __restrict__ out) {
  const int64_t row0 = (int64_t)blockIdx.x * g.rows_per_block;
  const int64_t left = g.investors - row0;
  const uint32_t rows = left < (int64_t)g.rows_per_block ? (uint32_t)left : g.rows_per_block;
  const uint32_t slots = rows * g.runs;
  for (uint32_t l = threadIdx.x; l < slots; l += kThreads) {
    const uint32_t rl = l / g.runs, run = l - rl * g.runs;
    const int64_t row = row0 + rl;
    const uint32_t c0 = g.lane0 + (uint32_t)row;
    const int64_t s0 = (int64_t)run * kRun;
    float* p = out + row * g.ld + s0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {  // four steps = two Philox blocks = one 16-byte store
      const int64_t sq = s0 + 4 * q;
      if (sq >= g.ld) break;
      float o[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const int64_t s = sq + 2 * b;
        if (s < g.horizon) {
          double z0, z1;
          rlmd_normal2(rlmd_philox(g.seed, c0, g.stream, RLMD_TAG_LEV_OUTCOME, (uint32_t)(s >> 1)), z0, z1);
          o[2 * b] = (float)(g.log_mean + g.vol * z0);
          if (s + 1 < g.horizon) o[2 * b + 1] = (float)(g.log_mean + g.vol * z1);
        }
      }
      if constexpr (VEC) {
        *reinterpret_cast<float4*>(p + 4 * q) = make_float4(o[0], o[1], o[2], o[3]);  // ld % 4 == 0
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (sq + j < g.ld) p[4 * q + j] = o[j];
      }
    }
  }
}

// ceil(t * 2^53) of a threshold in [0, inf): t <= u for u = k 2^-53 exactly when this <= k
bool threshold53(double t, uint64_t* out) {
  if (!(t >= 0.0)) return false;  // NaN included
  const double two53 = 9007199254740992.0;
  *out = t >= 1.0 ? (uint64_t)two53 + (t > 1.0) : (uint64_t)ceil(ldexp(t, 53));  // t > 1: above every k
  return true;
}

}  // namespace

extern "C" {

int rlmd_lev_outcomes(int32_t kind, uint64_t seed, uint32_t stream, int64_t first_investor, int64_t investors,
                      int32_t horizon, const double* params_host, void* out_dev, int64_t ld, void* stream_handle) {
  RLMD_CHECK(kind == 0 || kind == 1, "kind: 0 categorical (u8), 1 normal (f32)");
  RLMD_CHECK(params_host && out_dev, "null argument");
  RLMD_CHECK(investors >= 1 && horizon >= 1, "bad sizes: investors and horizon must be at least 1");
  RLMD_CHECK(ld >= horizon && ld <= (1ll << 30), "bad sizes: ld must be at least horizon (and at most 2^30)");
  RLMD_CHECK(first_investor >= 0 && investors <= (1ll << 32) && first_investor <= (1ll << 32) - investors,
             "first_investor + investors must not exceed 2^32 (the investor is one Philox counter word)");
  GenArgs g{};
  g.seed = seed;
  g.stream = stream;
  g.lane0 = (uint32_t)first_investor;
  g.investors = investors;
  g.horizon = horizon;
  g.ld = ld;
  g.runs = (uint32_t)((ld + kRun - 1) / kRun);
  g.rows_per_block = g.runs >= (uint32_t)kSlots ? 1u : (kSlots + g.runs - 1) / g.runs;
  const int64_t blocks = (investors + g.rows_per_block - 1) / g.rows_per_block;
  RLMD_CHECK(blocks <= 0x7FFFFFFFll, "bad sizes: too many rows of this length for one launch");
  hipStream_t st = (hipStream_t)stream_handle;
  const uintptr_t base = reinterpret_cast<uintptr_t>(out_dev);
  if (kind == 0) {
    RLMD_CHECK(threshold53(params_host[0], &g.t0) && threshold53(params_host[1], &g.t1) &&
                   params_host[0] <= params_host[1],
               "categorical thresholds must satisfy 0 <= t0 <= t1");
    uint32_t codes = 0;
    for (int c = 0; c < 3; ++c) {
      const double v = params_host[2 + c];
      RLMD_CHECK(v >= 0.0 && v <= 255.0 && v == floor(v), "categorical codes must be integers in 0..255");
      codes |= (uint32_t)v << (8 * c);
    }
    g.codes = codes;
    uint8_t* out = static_cast<uint8_t*>(out_dev);
    if (base % 16 == 0 && ld % 16 == 0)
      lev_gen_cat_kernel<16><<<dim3((unsigned)blocks), dim3(kThreads), 0, st>>>(g, out);
    else if (base % 4 == 0 && ld % 4 == 0)
      lev_gen_cat_kernel<4><<<dim3((unsigned)blocks), dim3(kThreads), 0, st>>>(g, out);
    else
      lev_gen_cat_kernel<1><<<dim3((unsigned)blocks), dim3(kThreads), 0, st>>>(g, out);
  } else {
    g.log_mean = params_host[0];
    g.vol = params_host[1];
    RLMD_CHECK(g.log_mean == g.log_mean && g.vol == g.vol, "normal parameters must not be NaN");
    RLMD_CHECK(base % 4 == 0, "f32 output must be 4-byte aligned");
    float* out = static_cast<float*>(out_dev);
    if (base % 16 == 0 && ld % 4 == 0)
      lev_gen_normal_kernel<true><<<dim3((unsigned)blocks), dim3(kThreads), 0, st>>>(g, out);
    else
      lev_gen_normal_kernel<false><<<dim3((unsigned)blocks), dim3(kThreads), 0, st>>>(g, out);
  }
  RLMD_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
