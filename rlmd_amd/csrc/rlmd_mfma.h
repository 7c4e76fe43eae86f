// rlmd_mfma.h — the MFMA operand types of the learner's kernels (gfx950, wave64)
// and the one-K-step multiply both compute precisions share.
#pragma once
#include "../../include/rlmd_abi.h"

namespace rlmd {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short bf16x8 __attribute__((ext_vector_type(8)));

// One K-step of a 16 x 16 output block: T the operand element, Frag a lane's 16
// bytes of it, KS the k covered by one fragment per lane.
template <int PREC>
struct Mfma;
template <>
struct Mfma<RLMD_BF16> {
  using T = unsigned short;
  using Frag = bf16x8;
  static constexpr int KS = 32;
  __device__ __forceinline__ static void mfma(const Frag& a, const Frag& b, f32x4& c) {
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  }
};
template <>
struct Mfma<RLMD_FP32> {
  using T = float;
  using Frag = f32x4;
  static constexpr int KS = 16;
  // lane group q = lane >> 4 holds k = k0 + 4q + j in element j: four 16x16x4
  // MFMAs cover k0 .. k0 + 15 (a permutation of the k order, same products)
  __device__ __forceinline__ static void mfma(const Frag& a, const Frag& b, f32x4& c) {
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0], b[0], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1], b[1], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[2], b[2], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[3], b[3], c, 0, 0, 0);
  }
};

}  // namespace rlmd
