// rlmd_mfma.h — the MFMA operand types of the learner's kernels (gfx950, wave64)
// and the one-K-step multiply both compute precisions share.
#pragma once
#include "../../include/rlmd_abi.h"

namespace rlmd {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short bf16x8 __attribute__((ext_vector_type(8)));

// RNE f32 -> bf16, NaN kept quiet; branch-free (a select, not a divergent branch).
// The integer form (about 7 VALU ops a value): the definition f2bf_pk is held to.
__device__ __forceinline__ unsigned short f2bf_rne(float f) {
  const unsigned u = __float_as_uint(f);
  const unsigned r = (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
  return (unsigned short)((u & 0x7fffffffu) > 0x7f800000u ? ((u >> 16) | 0x40u) : r);
}

// f2bf_rne(lo) | f2bf_rne(hi) << 16 in one instruction: the compiler's f32 -> bf16
// conversion is gfx950's v_cvt_pk_bf16_f32, whose bits equal f2bf_rne's for all
// 2^32 inputs in this library's denormal mode (NaNs, infinities, denormals and
// ties included: tools/probe/cvt_bf16_probe.hip).  The bf16 operand convert of
// the acting body and of the learner's row kernels.
__device__ __forceinline__ uint32_t f2bf_pk(float lo, float hi) {
  typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{lo, hi}, bf16x2));
}

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
