// The 16-lanes-per-row dot product shared by the selection kernels that score
// gathered fp32 rows against a vector held in LDS (mmr.hip, expand.hip,
// lexical.hip's fusion, fuse.hip's mean mode) and, for the fold alone, by
// crossenc.hip's head, which keeps this lane-to-dimension map over bf16 rows.
//
// Lane `part` (0 .. 15) of a group takes a FIXED share of the dimensions,
// whichever slot, group or wave the row sits in -- d4 == part (mod 16) over
// the float4 index d4 = d / 4 on the vector path, d == part (mod 16) on the
// scalar path -- in ascending order, one fma each, and the 16 partial sums are
// folded by xor shuffles 8, 4, 2, 1. One dot therefore passes through at most
//   L(D) = 4 ceil(D / 64) + 4                    (>= ceil(D / 16) + 4, the scalar path's depth)
// fp32 roundings, and two identical rows get bit-identical sums.
#pragma once
#include "lzk_common.h"

// this lane's share of <a, x> and of |x|^2 (a: LDS, zero padded to a multiple of 4; x: a row in global memory)
__device__ __forceinline__ void lzk_dot16_part(const float* a, const float* __restrict__ x, int D, int vec, int part,
                                               float& dot, float& xx) {
  dot = 0.f;
  xx = 0.f;
  if (vec) {
    const int n4 = D >> 2;
#pragma unroll 4
    for (int d4 = part; d4 < n4; d4 += 16) {
      const float4 xv = *reinterpret_cast<const float4*>(x + 4 * d4);
      const float4 av = *reinterpret_cast<const float4*>(a + 4 * d4);
      dot = fmaf(av.x, xv.x, dot); xx = fmaf(xv.x, xv.x, xx);
      dot = fmaf(av.y, xv.y, dot); xx = fmaf(xv.y, xv.y, xx);
      dot = fmaf(av.z, xv.z, dot); xx = fmaf(xv.z, xv.z, xx);
      dot = fmaf(av.w, xv.w, dot); xx = fmaf(xv.w, xv.w, xx);
    }
  } else {
    for (int d = part; d < D; d += 16) {
      const float xv = x[d];
      dot = fmaf(a[d], xv, dot);
      xx = fmaf(xv, xv, xx);
    }
  }
}

// this lane's share of |a|^2 in the same order (a: LDS, zero padded to a multiple of 4): the query's norm
__device__ __forceinline__ float lzk_sq16_part(const float* a, int D, int vec, int part) {
  float aa = 0.f;
  if (vec) {
    for (int d4 = part; d4 < (D >> 2); d4 += 16) {
      const float4 v = *reinterpret_cast<const float4*>(a + 4 * d4);
      aa = fmaf(v.x, v.x, aa); aa = fmaf(v.y, v.y, aa); aa = fmaf(v.z, v.z, aa); aa = fmaf(v.w, v.w, aa);
    }
  } else {
    for (int d = part; d < D; d += 16) aa = fmaf(a[d], a[d], aa);
  }
  return aa;
}

// the 16 partial sums of a group, in the one fixed order
__device__ __forceinline__ float lzk_fold16(float a) {
  a += __shfl_xor(a, 8, 64);
  a += __shfl_xor(a, 4, 64);
  a += __shfl_xor(a, 2, 64);
  a += __shfl_xor(a, 1, 64);
  return a;
}

// cosine from a dot and the two norms; 0 when either norm is 0
__device__ __forceinline__ float lzk_cos(float dot, float na, float nb) {
  return (na > 0.f && nb > 0.f) ? dot / (na * nb) : 0.f;
}
