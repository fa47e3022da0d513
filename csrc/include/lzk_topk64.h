// The 64-bit (score, row) key and the bitonic top-64 tournament shared by the
// kernels that keep up to 64 results per query in LDS (widek.hip, lexical.hip,
// fuse.hip, crossenc.hip): one text, so the tie order of every wide result
// cannot drift between them.
//
// Key. (score, row) -> u64, larger = better in the framework's order (score
// descending, row ascending): high word = the fp32 bits mapped monotonically
// (negative: ~bits, else bits | 0x80000000; -0 is folded into +0 and nan into
// -inf first), low word = 0xffffffff - row. Key 0 is below every real entry
// (-inf maps to 0x007fffff) and marks an empty slot. Equal keys (the same row
// listed twice) are kept as they are: max / min of two equal keys is the pair.
//
// Tournament (topk64_rounds). Every 64-entry block is sorted descending
// inside one wave (21 compare-exchange steps by __shfl_xor, no barrier). Then
// rounds with stride s = 1, 2, 4, ...: blocks a and a + s (a a multiple of
// 2 s) hold descending lists A and B; C[t] = max(A[t], B[63 - t]) is a bitonic
// sequence holding the 64 best of the 128, six more steps sort it, and it
// replaces A in place (only lane t reads A[t]; B is read only). A block
// without a partner stays. After ceil(log2(blocks)) rounds block 0 holds the
// 64 best of all, descending. One barrier per round.
#pragma once
#include "lzk_common.h"

typedef unsigned long long u64;

__device__ __forceinline__ u64 wide_key(float s, int row) {
  if (!(s == s)) s = LZK_NEG_INF;
  s += 0.0f;  // -0 -> +0: the order treats them as equal
  const unsigned u = __float_as_uint(s);
  const unsigned m = (u >> 31) ? ~u : (u | 0x80000000u);
  return ((u64)m << 32) | (u64)(0xffffffffu - (unsigned)row);
}

__device__ __forceinline__ void wide_unkey(u64 key, float& s, int& row) {
  const unsigned m = (unsigned)(key >> 32);
  const unsigned u = (m >> 31) ? (m & 0x7fffffffu) : ~m;
  s = __uint_as_float(u);
  row = (int)(0xffffffffu - (unsigned)(key & 0xffffffffu));
  if (m == 0u || s == LZK_NEG_INF) { s = LZK_NEG_INF; row = -1; }
}

__device__ __forceinline__ u64 kmax(u64 a, u64 b) { return a > b ? a : b; }
__device__ __forceinline__ u64 kmin(u64 a, u64 b) { return a < b ? a : b; }

// 64 keys, one per lane -> descending by lane.
__device__ __forceinline__ u64 wave_sort_desc(u64 v, int lane) {
#pragma unroll
  for (int k = 2; k <= 64; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
      const u64 o = __shfl_xor(v, j, 64);
      const bool low = (lane & j) == 0, desc = (lane & k) == 0;
      v = (low == desc) ? kmax(v, o) : kmin(v, o);
    }
  }
  return v;
}

// A bitonic sequence of 64 keys -> descending by lane.
__device__ __forceinline__ u64 wave_merge_desc(u64 v, int lane) {
#pragma unroll
  for (int j = 32; j > 0; j >>= 1) {
    const u64 o = __shfl_xor(v, j, 64);
    v = (lane & j) == 0 ? kmax(v, o) : kmin(v, o);
  }
  return v;
}

// keys[0 .. 64 nb): blocks b0 .. nb - 1 are unsorted, blocks below b0 already
// descending (b0 = 0: every block unsorted). On return block 0 holds the 64
// best of all nb blocks, descending. Every thread of the block calls it (nb,
// b0 block-uniform), and blockDim.x is a multiple of 64: a wave owns a block.
__device__ __forceinline__ void topk64_rounds(u64* keys, int b0, int nb) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  __syncthreads();
  for (int b = b0 + wave; b < nb; b += nw) keys[64 * b + lane] = wave_sort_desc(keys[64 * b + lane], lane);
  for (int s = 1; s < nb; s <<= 1) {
    __syncthreads();
    for (int a = wave * 2 * s; a + s < nb; a += nw * 2 * s) {
      const u64 A = keys[64 * a + lane];
      const u64 B = keys[64 * (a + s) + 63 - lane];
      keys[64 * a + lane] = wave_merge_desc(kmax(A, B), lane);
    }
  }
  __syncthreads();
}
