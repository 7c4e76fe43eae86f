// cvt_bf16_probe.hip — does gfx950's v_cvt_pk_bf16_f32 give the bits of
// rlmd_mfma.h's f2bf_rne (the integer convert of the acting body and, as to_bf16
// until round 9, of the row kernels) for every f32?  One kernel over all 2^32 inputs
// (NaNs, infinities, denormals and ties included), compiled with the library's
// flags, so it runs in the library's denormal mode.  Candidates per input: the
// instruction's low half, its high half, the compiler's own f32 -> __bf16 cast,
// and both halves of the library's f2bf_pk.  Prints the mismatch counts (NaN
// inputs counted apart) and the first counter-examples; exit status 0 only if
// every candidate matches everywhere.
//
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -Irlmd_amd/csrc -Iinclude \
//         tools/probe/cvt_bf16_probe.hip -o tools/_probe/cvt_bf16_probe
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "rlmd_act_rows.h"

namespace {

constexpr int kKinds = 5, kKeep = 8;

struct Result {
  unsigned long long bad[kKinds], bad_nan[kKinds];
  unsigned n_ex;
  unsigned ex[kKeep][3];  // kind, input bits, got << 16 | want
};

__device__ __forceinline__ unsigned cvt_pk(float lo, float hi) {
  unsigned r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
  return r;
}

__global__ void __launch_bounds__(256) probe(Result* res) {
  const unsigned stride = gridDim.x * blockDim.x;  // a power of two: 2^32 / stride passes
  unsigned u = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned passes = (unsigned)(0x100000000ull / stride);
  for (unsigned p = 0; p < passes; ++p, u += stride) {
    const float f = __uint_as_float(u);
    const unsigned want = rlmd::actrows::f2bf_rne(f);
    const unsigned got[kKinds] = {cvt_pk(f, 0.f) & 0xffffu, cvt_pk(0.f, f) >> 16,
                                  (unsigned)__builtin_bit_cast(unsigned short, (__bf16)f),
                                  rlmd::actrows::f2bf_pk(f, 0.f) & 0xffffu, rlmd::actrows::f2bf_pk(0.f, f) >> 16};
    const bool nan = (u & 0x7fffffffu) > 0x7f800000u;
#pragma unroll
    for (int k = 0; k < kKinds; ++k) {
      if (got[k] == want) continue;
      atomicAdd(nan ? &res->bad_nan[k] : &res->bad[k], 1ull);
      const unsigned slot = atomicAdd(&res->n_ex, 1u);
      if (slot < kKeep) {
        res->ex[slot][0] = k;
        res->ex[slot][1] = u;
        res->ex[slot][2] = got[k] << 16 | want;
      }
    }
  }
}

}  // namespace

#define CHECK(x)                                                   \
  do {                                                             \
    hipError_t e_ = (x);                                           \
    if (e_ != hipSuccess) {                                        \
      fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));      \
      return 2;                                                    \
    }                                                              \
  } while (0)

int main() {
  Result* d = nullptr;
  Result h{};
  CHECK(hipMalloc(&d, sizeof(Result)));
  CHECK(hipMemset(d, 0, sizeof(Result)));
  hipLaunchKernelGGL(probe, dim3(4096), dim3(256), 0, 0, d);
  CHECK(hipGetLastError());
  CHECK(hipDeviceSynchronize());
  CHECK(hipMemcpy(&h, d, sizeof(Result), hipMemcpyDeviceToHost));
  CHECK(hipFree(d));
  const char* names[kKinds] = {"v_cvt_pk_bf16_f32 low half", "v_cvt_pk_bf16_f32 high half", "(__bf16) cast",
                               "f2bf_pk low half", "f2bf_pk high half"};
  bool ok = true;
  for (int k = 0; k < kKinds; ++k) {
    printf("%-28s mismatches: %llu finite/inf, %llu NaN (of 2^32 inputs)\n", names[k], h.bad[k], h.bad_nan[k]);
    ok = ok && h.bad[k] == 0 && h.bad_nan[k] == 0;
  }
  for (unsigned i = 0; i < h.n_ex && i < (unsigned)kKeep; ++i)
    printf("  counter-example: %s  input 0x%08x  got 0x%04x  f2bf_rne 0x%04x\n", names[h.ex[i][0]], h.ex[i][1],
           h.ex[i][2] >> 16, h.ex[i][2] & 0xffffu);
  printf(ok ? "IDENTICAL\n" : "DIFFERENT\n");
  return ok ? 0 : 1;
}
