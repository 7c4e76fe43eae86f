// replay.hip — on-device replay ring + fused sample/gather for gfx950.
//
// Replaces tools/replay_torch.py (ReplayBufferTorch) / tools/replay.py:
//   store_exp   :167-197 (torch) / :143-174 (numpy): ring slot mem_idx % mem_size,
//               reward stored as max(r, r_abs_zero = -inf) == r;
//   sample_exp  :360-412 (torch randperm(max_mem)[:B]) / :334-376 (numpy
//               choice(max_mem, B, replace=False)): B DISTINCT uniform indices
//               over the filled part of the ring, then row gathers.
// Distinct indices on the GPU, two regimes (both restated in oracle/replay.py,
// so a sample is reproducible on the CPU index for index):
//   M <= 8192: a uniformly random B-subset as the B smallest of M random keys
//              (one LDS bitonic sort of (philox32 << 32 | index));
//   M >  8192: draw B candidates with Philox, redraw every slot whose index
//              already appeared at a smaller slot (found through an LDS hash
//              table whose entries keep the minimum owning slot), repeat
//              (collision rate <= B/M <= 1/8 per round).
// Multi-step mode (tools/replay.py:93-332): rows carry (position, episode,
// episode start) tags and every lane its episode bookkeeping, so the reference's
// history slicing — including its one-step-ahead slices of finished episodes and
// the episode-0 fallback of in-progress ones — is O(1) per
// sampled row; the n-step return, initial (next) state and action, and eff are
// gathered in the same kernel (restated in oracle/replay.py MultiStepRing).
#include <string.h>

#include <string>
#include <vector>

#include <stddef.h>
#include "rlmd_common.h"
#include "rlmd_internal.h"
#include "rlmd_replay_dev.h"

struct rlmd_replay_s {
  rlmd::ReplayView v;
  int64_t mem_idx = 0;
};

namespace {

constexpr int kSampleThreads = RLMD_MAX_BATCH;

__device__ __forceinline__ int64_t ms_row(const rlmd::ReplayView& rb, int lane, int64_t pos) {
  return (pos * rb.lanes + lane) % rb.capacity;
}

// Gather row `row` into output slot i: single-step copies the row; multi-step
// follows MultiStepRing.gather (oracle/replay.py).
__device__ void gather_row(const rlmd::ReplayView& rb, int64_t row, int i, float* s, float* a, float* r,
                           float* s2, uint8_t* done, float* xsa, int32_t* eff) {
  const int S = rb.S, A = rb.A;
  int64_t src = row;  // row supplying the (initial) state and action
  float rew = rb.reward[row];
  int e = 1;
  if (rb.n_steps > 1) {
    const int lane = (int)(row % rb.lanes);
    const int32_t* t = rb.tag + 3 * row;
    const int32_t* ls = rb.lane + 4 * (int64_t)lane;
    const int64_t sp = t[0], j = t[1], aj = t[2], m = ls[1], d0 = ls[3];
    int64_t lo, b;
    if (j == 0) {
      lo = 0;
      b = sp;
    } else if (j < m) {
      lo = aj;
      b = rb.done[row] ? sp : sp + 1;
    } else {
      lo = 0;
      b = sp - aj + 1 < d0 ? sp - aj + 1 : d0;
    }
    e = (int)(b - lo + 1 < rb.n_steps ? b - lo + 1 : rb.n_steps);
    const int64_t f = b - e + 1;
    double acc = rb.additive ? 0.0 : 1.0;
    for (int k = 0; k < e - 1; ++k) {
      const double term = pow(rb.gamma, (double)k) * (double)rb.reward[ms_row(rb, lane, f + k)];
      acc = rb.additive ? acc + term : acc * term;
    }
    rew = (float)acc;
    src = ms_row(rb, lane, f);
    for (int k = 0; k < S; ++k) {
      const float v = rb.next_state[src * S + k];  // histories hold next states
      if (s) s[(int64_t)i * S + k] = v;
      if (xsa) xsa[(int64_t)i * (S + A) + k] = v;
    }
  } else {
    for (int k = 0; k < S; ++k) {
      const float v = rb.state[row * S + k];
      if (s) s[(int64_t)i * S + k] = v;
      if (xsa) xsa[(int64_t)i * (S + A) + k] = v;
    }
  }
  for (int k = 0; k < S; ++k)
    if (s2) s2[(int64_t)i * S + k] = rb.next_state[row * S + k];
  for (int k = 0; k < A; ++k) {
    const float v = rb.action[src * A + k];
    if (a) a[(int64_t)i * A + k] = v;
    if (xsa) xsa[(int64_t)i * (S + A) + S + k] = v;
  }
  if (r) r[i] = rew;
  if (done) done[i] = rb.done[row];
  if (eff) eff[i] = e;
}
// gather_row1 (single-step rows) and the hash-path draw: rlmd_replay_dev.h, shared
// with the learner launches that run them as roles (learn.hip agent_learn_k)
using rlmd::gather_row1;
using rlmd::kSortPopulation;  // M at or below: sort-based subset

// replay_sample_kernel's explicit arguments as laid out in the kernarg segment
// (each at its natural alignment, in order): their exact byte count bounds the
// argument prefetch
struct SampleKargs {
  rlmd::ReplayView rb;
  int64_t M;
  int B, G;
  uint64_t seed;
  uint32_t ctr_lo, ctr_hi;
  int64_t* idx_out;
  float *s, *a, *r, *s2;
  uint8_t* done;
  float* xsa;
  int32_t* eff;
};

__global__ void __launch_bounds__(kSampleThreads)
    replay_sample_kernel(rlmd::ReplayView rb, int64_t M, int B, int G, uint64_t seed, uint32_t ctr_lo,
                         uint32_t ctr_hi, int64_t* idx_out, float* s, float* a,
                         float* r, float* s2, uint8_t* done, float* xsa, int32_t* eff) {
  rlmd_kernarg_prefetch<(int)(offsetof(SampleKargs, eff) + sizeof(int32_t*))>();
  __shared__ uint64_t keys[kSortPopulation];
  __shared__ int64_t cand[kSampleThreads];
  __shared__ int any_dup;
  const int i = threadIdx.x;
  // workgroups [G k, G k + G) of a K-batch launch all draw mini-batch k with
  // counter ctr + k (the same distinct set: the draw is a function of the
  // counter) and each gathers 1 / G of its rows — the gather's scattered
  // row reads spread over G CUs — into offset k
  const int part = blockIdx.x % G;
  {
    const int k = blockIdx.x / G;
    const uint64_t ctr = ((uint64_t)ctr_hi << 32 | ctr_lo) + (uint64_t)k;
    ctr_lo = (uint32_t)ctr;
    ctr_hi = (uint32_t)(ctr >> 32);
    const int S = rb.S, A = rb.A;
    if (idx_out) idx_out += (int64_t)k * B;
    if (s) s += (int64_t)k * B * S;
    if (a) a += (int64_t)k * B * A;
    if (r) r += (int64_t)k * B;
    if (s2) s2 += (int64_t)k * B * S;
    if (done) done += (int64_t)k * B;
    if (xsa) xsa += (int64_t)k * B * (S + A);
    if (eff) eff += (int64_t)k * B;
  }
  const uint32_t c2 = RLMD_TAG_REPLAY_IDX | (ctr_hi << 8);
  if (M <= kSortPopulation) {
    int npow = 1;
    while (npow < M) npow <<= 1;
    for (int e = i; e < npow; e += kSampleThreads) {
      if (e < M) {
        const rlmd_u32x4 v = rlmd_philox(seed, (uint32_t)e, ctr_lo, c2, 0xFFFFFFFFu);
        keys[e] = ((uint64_t)v.x << 32) | (uint64_t)e;
      } else {
        keys[e] = ~0ull;
      }
    }
    __syncthreads();
    for (int k = 2; k <= npow; k <<= 1) {
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int e = i; e < npow; e += kSampleThreads) {
          const int exj = e ^ j;
          if (exj > e) {
            const uint64_t x = keys[e], y = keys[exj];
            const bool up = (e & k) == 0;
            if ((x > y) == up) {
              keys[e] = y;
              keys[exj] = x;
            }
          }
        }
        __syncthreads();
      }
    }
    if (i < B) cand[i] = (int64_t)(keys[i] & 0xFFFFFFFFu);
  } else {
    // rounds of hash-table dedupe (rlmd_replay_dev.h replay_draw_hash)
    __shared__ unsigned long long tab_key[rlmd::kDrawHash];
    __shared__ int tab_own[rlmd::kDrawHash];
    rlmd::replay_draw_hash<kSampleThreads>(M, B, seed, ctr_lo, c2, cand, tab_key, tab_own);
  }
  __syncthreads();
  const int per = (B + G - 1) / G;
  if (i >= B || i < part * per || i >= (part + 1) * per) return;
  const int64_t row = cand[i];
  if (idx_out) idx_out[i] = row;
  if (rb.n_steps > 1)
    gather_row(rb, row, i, s, a, r, s2, done, xsa, eff);
  else
    gather_row1(rb, row, i, s, a, r, s2, done, xsa, eff);
}

__global__ void replay_gather_kernel(rlmd::ReplayView rb, int n, const int64_t* rows, float* s, float* a,
                                     float* r, float* s2, uint8_t* done, int32_t* eff) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) gather_row(rb, rows[i], i, s, a, r, s2, done, nullptr, eff);
}

__global__ void replay_insert_kernel(rlmd::ReplayView rb, int64_t base, int64_t n, const float* s,
                                     const float* a, const float* r, const float* s2,
                                     const uint8_t* d) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t row = (base + i) % rb.capacity;
  for (int k = 0; k < rb.S; ++k) {
    rb.state[row * rb.S + k] = s[i * rb.S + k];
    rb.next_state[row * rb.S + k] = s2[i * rb.S + k];
  }
  for (int k = 0; k < rb.A; ++k) rb.action[row * rb.A + k] = a[i * rb.A + k];
  rb.reward[row] = r[i];
  rb.done[row] = d[i];
  if (rb.n_steps > 1) rlmd::ms_record(rb, (int)((base + i) % rb.lanes), row, d[i] != 0);
}

__global__ void replay_read_kernel(rlmd::ReplayView rb, int64_t start, int64_t n, float* s, float* a,
                                   float* r, float* s2, uint8_t* d) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t row = (start + i) % rb.capacity;
  for (int k = 0; k < rb.S; ++k) {
    if (s) s[i * rb.S + k] = rb.state[row * rb.S + k];
    if (s2) s2[i * rb.S + k] = rb.next_state[row * rb.S + k];
  }
  for (int k = 0; k < rb.A; ++k)
    if (a) a[i * rb.A + k] = rb.action[row * rb.A + k];
  if (r) r[i] = rb.reward[row];
  if (d) d[i] = rb.done[row];
}

}  // namespace

namespace rlmd {

ReplayView replay_view(rlmd_replay_t rb) { return rb->v; }
int64_t replay_mem_idx(rlmd_replay_t rb) { return rb->mem_idx; }
void replay_advance(rlmd_replay_t rb, int64_t n) { rb->mem_idx += n; }

int replay_sample_launch(const ReplayView& rb, int64_t M, int B, int K, uint64_t seed, uint64_t ctr,
                         int64_t* idx, float* s, float* a, float* r, float* s2, uint8_t* done, float* xsa,
                         int32_t* eff, hipStream_t stream) {
  RLMD_CHECK(B >= 1 && B <= RLMD_MAX_BATCH, "batch must be in [1, 1024]");
  RLMD_CHECK(K >= 1, "need at least one mini-batch");
  RLMD_CHECK(M >= B, "replay holds fewer transitions than the mini-batch");
  RLMD_CHECK(M <= (int64_t)1 << 52, "replay too large");
  const int G = B >= 256 ? 8 : 1;  // gather parts per mini-batch
  hipLaunchKernelGGL(replay_sample_kernel, dim3(K * G), dim3(kSampleThreads), 0, stream, rb, M, B, G, seed,
                     (uint32_t)ctr, (uint32_t)(ctr >> 32), idx, s, a, r, s2, done, xsa, eff);
  RLMD_LAUNCH_CHECK();
  return 0;
}

}  // namespace rlmd

extern "C" {

int rlmd_replay_create(int64_t capacity, int32_t S, int32_t A, rlmd_replay_t* out) {
  RLMD_CHECK(out && capacity > 0 && S > 0 && A > 0, "bad replay arguments");
  auto* rb = new rlmd_replay_s();
  rb->v.capacity = capacity;
  rb->v.S = S;
  rb->v.A = A;
  RLMD_HIP(hipMalloc(&rb->v.state, sizeof(float) * capacity * S));
  RLMD_HIP(hipMalloc(&rb->v.next_state, sizeof(float) * capacity * S));
  RLMD_HIP(hipMalloc(&rb->v.action, sizeof(float) * capacity * A));
  RLMD_HIP(hipMalloc(&rb->v.reward, sizeof(float) * capacity));
  RLMD_HIP(hipMalloc(&rb->v.done, capacity));
  rb->v.n_steps = 1;
  rb->v.lanes = 1;
  rb->v.additive = 1;
  rb->v.gamma = 0.99;
  *out = rb;
  return 0;
}

int rlmd_replay_set_multistep(rlmd_replay_t rb, int32_t lanes, int32_t n_steps, int32_t additive,
                              double gamma) {
  RLMD_CHECK(rb, "null replay");
  RLMD_CHECK(rb->mem_idx == 0, "multi-step mode must be set before the first insert");
  RLMD_CHECK(lanes >= 1 && rb->v.capacity % lanes == 0, "capacity must be a multiple of the lane count");
  RLMD_CHECK(n_steps >= 1, "multi_steps must be >= 1");
  rb->v.n_steps = n_steps;
  rb->v.lanes = lanes;
  rb->v.additive = additive ? 1 : 0;
  rb->v.gamma = gamma;
  if (n_steps > 1) {
    if (!rb->v.tag) RLMD_HIP(hipMalloc(&rb->v.tag, sizeof(int32_t) * 3 * rb->v.capacity));
    if (rb->v.lane) RLMD_HIP(hipFree(rb->v.lane));
    RLMD_HIP(hipMalloc(&rb->v.lane, sizeof(int32_t) * 4 * lanes));
    std::vector<int32_t> init(4 * (size_t)lanes, 0);
    for (int32_t l = 0; l < lanes; ++l) init[4 * l + 3] = -1;
    RLMD_HIP(hipMemcpy(rb->v.lane, init.data(), sizeof(int32_t) * init.size(), hipMemcpyHostToDevice));
  }
  return 0;
}

int rlmd_replay_destroy(rlmd_replay_t rb) {
  if (!rb) return 0;
  (void)hipFree(rb->v.state);
  (void)hipFree(rb->v.next_state);
  (void)hipFree(rb->v.action);
  (void)hipFree(rb->v.reward);
  (void)hipFree(rb->v.done);
  if (rb->v.tag) (void)hipFree(rb->v.tag);
  if (rb->v.lane) (void)hipFree(rb->v.lane);
  delete rb;
  return 0;
}

int rlmd_replay_insert(rlmd_replay_t rb, int64_t n, const float* s, const float* a, const float* r,
                       const float* s2, const uint8_t* d, void* stream) {
  RLMD_CHECK(rb && s && a && r && s2 && d, "null argument");
  if (n <= 0) return 0;
  RLMD_CHECK(rb->v.n_steps <= 1 || n <= rb->v.lanes, "multi-step insert: at most one transition per lane per call");
  hipLaunchKernelGGL(replay_insert_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, rb->v, rb->mem_idx, n, s, a, r, s2, d);
  RLMD_LAUNCH_CHECK();
  rb->mem_idx += n;
  return 0;
}

int rlmd_replay_read(rlmd_replay_t rb, int64_t start, int64_t n, float* s, float* a, float* r,
                     float* s2, uint8_t* d, void* stream) {
  RLMD_CHECK(rb && start >= 0, "bad argument");
  if (n <= 0) return 0;
  hipLaunchKernelGGL(replay_read_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, rb->v, start, n, s, a, r, s2, d);
  RLMD_LAUNCH_CHECK();
  return 0;
}

int rlmd_replay_mem_idx(rlmd_replay_t rb, int64_t* m) {
  RLMD_CHECK(rb && m, "null argument");
  *m = rb->mem_idx;
  return 0;
}

int rlmd_replay_sample(rlmd_replay_t rb, int32_t B, uint64_t seed, uint64_t ctr, int64_t* idx,
                       float* s, float* a, float* r, float* s2, uint8_t* done, int32_t* eff, void* stream) {
  RLMD_CHECK(rb, "null replay");
  const int64_t M = rb->mem_idx < rb->v.capacity ? rb->mem_idx : rb->v.capacity;
  return rlmd::replay_sample_launch(rb->v, M, B, 1, seed, ctr, idx, s, a, r, s2, done, nullptr, eff,
                                    (hipStream_t)stream);
}

int rlmd_replay_gather(rlmd_replay_t rb, int32_t n, const int64_t* rows, float* s, float* a, float* r,
                       float* s2, uint8_t* done, int32_t* eff, void* stream) {
  RLMD_CHECK(rb && rows, "null argument");
  if (n <= 0) return 0;
  hipLaunchKernelGGL(replay_gather_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     rb->v, n, rows, s, a, r, s2, done, eff);
  RLMD_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
