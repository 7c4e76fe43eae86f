// rlmd_replay_dev.h — device pieces of the replay sampler shared by replay.hip
// (replay_sample_kernel) and the learner launches that run them as roles when
// the sample launch is hoisted off the training step's chain (learn.hip
// agent_learn_k): the hash-path draw (update.hip, the call's last launch draws
// the next call's index sets) and the single-step row gather (rows.hip, update
// 0's fwd_rows gathers by index).
#pragma once
#include "rlmd_common.h"
#include "rlmd_internal.h"

namespace rlmd {

constexpr int kDrawMaxRounds = 64;
constexpr int kSortPopulation = 8192;         // M at or below: sort-based subset (replay.hip)
constexpr int kDrawHash = 2 * RLMD_MAX_BATCH;  // LDS hash table entries of the draw

// LDS of one draw (28 KB .. 32 KB): the candidates and the hash table
struct DrawLds {
  static constexpr int cand = 0;                                // int64 [RLMD_MAX_BATCH]
  static constexpr int key = cand + RLMD_MAX_BATCH * 8;         // u64 [kDrawHash]
  static constexpr int own = key + kDrawHash * 8;               // int [kDrawHash]
  static constexpr int total = own + kDrawHash * 4;
};

// The next call's draw as extra workgroups of a learner launch (n = 0: none):
// workgroup k draws mini-batch k with counter ctr + k into idx_out + k * B.
struct SampleDrawArgs {
  int64_t M;
  uint64_t seed, ctr;
  int64_t* idx_out;
  int32_t B, n;
};

// Update 0's fwd_rows of a hoisted call (rows.hip, GATHER): idx holds the K
// prepared index sets [K][B]; the row workgroups stage mini-batch 0 straight from
// the ring and publish it to slab offset 0, nk - 1 x ceil(B / 64) extra
// workgroups gather mini-batches 1 .. nk - 1 into offsets 1 .. nk - 1.
struct HoistGatherArgs {
  const int64_t* idx;
  ReplayView rb;
  int64_t* o_idx;
  float *o_s, *o_a, *o_r, *o_s2, *o_xsa;
  uint8_t* o_done;
  int32_t nk;
};
constexpr int kGatherRows = 64;  // rows per extra gather workgroup (one wave)

// M > kSortPopulation: B distinct indices in [0, M) into cand[0, B).  Rounds of:
// hash every candidate into an LDS table; the smallest slot per index owns it
// (atomicMin: order-independent); the other slots redraw.  Slot i is thread
// i % NTH's: a workgroup narrower than the batch owns several slots per thread.
// Ends with a barrier: every thread may read cand afterwards.
template <int NTH>
__device__ __forceinline__ void replay_draw_hash(int64_t M, int B, uint64_t seed, uint32_t ctr_lo, uint32_t c2,
                                                 int64_t* cand, unsigned long long* tab_key, int* tab_own) {
  constexpr int H = kDrawHash;
  constexpr int PER = (RLMD_MAX_BATCH + NTH - 1) / NTH;
  const int t = threadIdx.x;
#pragma unroll
  for (int q = 0; q < PER; ++q) {
    const int i = t + q * NTH;
    if (i < B) {
      const rlmd_u32x4 v = rlmd_philox(seed, (uint32_t)i, ctr_lo, c2, 0u);
      cand[i] = (int64_t)rlmd_below(v.x, v.y, (uint64_t)M);
    }
  }
  for (int round = 1; round <= kDrawMaxRounds; ++round) {
    for (int e = t; e < H; e += NTH) {
      tab_key[e] = ~0ull;
      tab_own[e] = 0x7fffffff;
    }
    __syncthreads();
    int h[PER];
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const int i = t + q * NTH;
      h[q] = 0;
      if (i < B) {
        const unsigned long long c = (unsigned long long)cand[i];
        int hh = (int)((c * 0x9E3779B97F4A7C15ull) >> 52) & (H - 1);
        for (int probe = 0; probe < H; ++probe) {
          const unsigned long long old = atomicCAS(&tab_key[hh], ~0ull, c);
          if (old == ~0ull || old == c) break;
          hh = (hh + 1) & (H - 1);
        }
        atomicMin(&tab_own[hh], i);
        h[q] = hh;
      }
    }
    __syncthreads();
    bool any = false;
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const int i = t + q * NTH;
      const bool dup = i < B && tab_own[h[q]] != i;
      if (dup) {
        const rlmd_u32x4 v = rlmd_philox(seed, (uint32_t)i, ctr_lo, c2, (uint32_t)round);
        cand[i] = (int64_t)rlmd_below(v.x, v.y, (uint64_t)M);
      }
      any |= dup;
    }
    if (!__syncthreads_or(any)) break;
  }
  __syncthreads();
}

// The draw role of a learner launch: workgroup k of a.n (NTH threads, DrawLds
// bytes of LDS at smem) writes mini-batch k's indices.
template <int NTH>
__device__ __forceinline__ void replay_draw_role(const SampleDrawArgs& a, int k, unsigned char* smem) {
  int64_t* cand = reinterpret_cast<int64_t*>(smem + DrawLds::cand);
  const uint64_t ctr = a.ctr + (uint64_t)k;
  const uint32_t c2 = RLMD_TAG_REPLAY_IDX | ((uint32_t)(ctr >> 32) << 8);
  replay_draw_hash<NTH>(a.M, a.B, a.seed, (uint32_t)ctr, c2, cand,
                        reinterpret_cast<unsigned long long*>(smem + DrawLds::key),
                        reinterpret_cast<int*>(smem + DrawLds::own));
  int64_t* out = a.idx_out + (int64_t)k * a.B;
  for (int i = threadIdx.x; i < a.B; i += NTH) rlmd_st_wt(out + i, cand[i]);
}

// Single-step rows (the training loop's case): every load of the row issued
// before its first store. In gather_row's element loops each store is counted
// in vmcnt and the outputs may alias the ring as far as the compiler knows, so
// every element waited on its own scattered-row round trip (S + S + A + 2 of
// them per row). Clamped indices keep the loads branch-free; the stores are
// write-through (the next kernel reads them).
__device__ __forceinline__ void gather_row1(const rlmd::ReplayView& rb, int64_t row, int i, float* s, float* a,
                                            float* r, float* s2, uint8_t* done, float* xsa, int32_t* eff) {
  constexpr int C = 8;
  const int S = rb.S, A = rb.A, X = S + A;
  const float* st = rb.state + row * S;
  const float* ns = rb.next_state + row * S;
  const float* ac = rb.action + row * A;
  float sv[C], nv[C], av[C];
#pragma unroll
  for (int q = 0; q < C; ++q) {
    sv[q] = st[q < S ? q : S - 1];
    nv[q] = ns[q < S ? q : S - 1];
    av[q] = ac[q < A ? q : A - 1];
  }
  const float rew = rb.reward[row];
  const uint8_t dn = rb.done[row];
#pragma unroll
  for (int q = 0; q < C; ++q) {
    if (q < S) {
      if (s) rlmd_st_wt(s + (int64_t)i * S + q, sv[q]);
      if (xsa) rlmd_st_wt(xsa + (int64_t)i * X + q, sv[q]);
      if (s2) rlmd_st_wt(s2 + (int64_t)i * S + q, nv[q]);
    }
    if (q < A) {
      if (a) rlmd_st_wt(a + (int64_t)i * A + q, av[q]);
      if (xsa) rlmd_st_wt(xsa + (int64_t)i * X + S + q, av[q]);
    }
  }
  if (r) rlmd_st_wt(r + i, rew);
  if (done) rlmd_st_wt(done + i, dn);
  if (eff) rlmd_st_wt(eff + i, (int32_t)1);
  // wider rows (market Dx observations, many-action investors): the rest per chunk
  for (int k0 = C; k0 < S || k0 < A; k0 += C) {
#pragma unroll
    for (int q = 0; q < C; ++q) {
      const int k = k0 + q;
      sv[q] = st[k < S ? k : S - 1];
      nv[q] = ns[k < S ? k : S - 1];
      av[q] = ac[k < A ? k : A - 1];
    }
#pragma unroll
    for (int q = 0; q < C; ++q) {
      const int k = k0 + q;
      if (k < S) {
        if (s) rlmd_st_wt(s + (int64_t)i * S + k, sv[q]);
        if (xsa) rlmd_st_wt(xsa + (int64_t)i * X + k, sv[q]);
        if (s2) rlmd_st_wt(s2 + (int64_t)i * S + k, nv[q]);
      }
      if (k < A) {
        if (a) rlmd_st_wt(a + (int64_t)i * A + k, av[q]);
        if (xsa) rlmd_st_wt(xsa + (int64_t)i * X + S + k, av[q]);
      }
    }
  }
}

}  // namespace rlmd
