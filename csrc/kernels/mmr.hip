// Diversity-aware selection over a search's candidate pool: greedy
// maximal-marginal-relevance (MMR) picks, one block per query.
//
//   obj_t(c) = (1 - delta) cos(q, c) - delta max_{s in S_t} cos(c, s)      (the max is 0 while S_0 is empty)
//
// over the pool's fp32 rows; the argmax is picked k times, ties to the lower
// graph row (better(), lzk_common.h). cos is 0 when either norm is 0. Pool
// entries < 0 or >= n are empty slots and are never read.
//
// Layout. MMR_NT = 256 threads: 16 groups of 16 lanes; group g owns pool slots
// g, g + 16, g + 32, g + 48. The query sits in LDS, the row picked last beside
// it. A pass scores every owned slot against one of the two: float4 loads when
// D % 4 == 0 and X is 16-byte aligned with ldx % 4 == 0, scalar loads otherwise.
// The relevance pass also sums |x|^2, so no norm column is consulted. Then k
// rounds: wave 0 holds slot f in lane f and takes the wave argmax; the picked
// row is copied to LDS; all 16 groups fold its cosine to every remaining slot
// into maxsim[f] (not after the last pick). Pool rows are re-read through L2
// each round: (k - 1) * F * D * 4 bytes per query.
//
// Summation order (MMR_SUM_DEPTH in ops/mmr_ops.py restates it; the tests read
// it there). Lane `part` of a group takes a FIXED share of the dimensions,
// whichever slot, group or wave the row sits in -- d4 == part (mod 16) over
// the float4 index d4 = d / 4 on the vector path, d == part (mod 16) on the
// scalar path -- in ascending order, one fma each, and the 16 partial sums are
// folded by xor shuffles 8, 4, 2, 1. One dot therefore passes through at most
//   L(D) = 4 ceil(D / 64) + 4                    (>= ceil(D / 16) + 4, the scalar path's depth)
// fp32 roundings, and |cos32 - cos64| <= (2 L(D) + 8) 2^-24: L for the dot, L
// jointly for the two norms under their square roots, 8 for the two sqrt, the
// multiply, the divide and the four roundings of the objective. Two identical
// rows get bit-identical dots, norms and objectives, so the row decides
// between them. A launch takes one path for every dot it computes.
#include "lzk_common.h"
#include "lzk_dot16.h"  // lzk_dot16_part, lzk_sq16_part, lzk_fold16, lzk_cos: the layout stated above

namespace {

constexpr int MMR_NT = 256;
constexpr int MMR_MAX_F = 64;           // one pool slot per lane of the selecting wave
constexpr int MMR_NONE = 0x7fffffff;    // tie key of an empty slot: loses to every row
constexpr size_t MMR_MAX_LDS = 64 * 1024;

__global__ __launch_bounds__(MMR_NT) void mmr_select_kernel(
    const float* __restrict__ X, long ldx, int n, const float* __restrict__ Q, long ldq, int D,
    const long* __restrict__ cand, int F, int k, float delta, int* __restrict__ pick, float* __restrict__ obj,
    int vec) {
  extern __shared__ __attribute__((aligned(16))) float s_dyn[];
  __shared__ float s_rel[MMR_MAX_F];   // cos(q, slot)
  __shared__ float s_nrm[MMR_MAX_F];   // |slot's row|
  __shared__ float s_max[MMR_MAX_F];   // max cosine to the rows picked so far
  __shared__ int s_row[MMR_MAX_F];     // graph row of the slot, -1 = empty or picked
  __shared__ int s_pick;               // the slot picked this round, -1 = the pool ran out
  const int Dq = (D + 3) & ~3;
  float* s_q = s_dyn;        // [Dq] the query, zero padded
  float* s_p = s_dyn + Dq;   // [Dq] the row picked last
  const int tid = threadIdx.x, lane = tid & 63, part = lane & 15, grp = tid >> 4;
  const long m = blockIdx.x;

  for (int d = tid; d < Dq; d += MMR_NT) s_q[d] = d < D ? Q[m * ldq + d] : 0.f;
  if (tid < MMR_MAX_F) {
    long r = tid < F ? cand[m * F + tid] : -1;
    if (r < 0 || r >= n) r = -1;  // (an empty slot, or a row the graph does not have: never read)
    s_row[tid] = (int)r;
    s_max[tid] = LZK_NEG_INF;
  }
  __syncthreads();

  // ---- |q|: every group sums the same shares in the same order
  const float qn = sqrtf(lzk_fold16(lzk_sq16_part(s_q, D, vec, part)));

  // ---- relevance and norms of the owned slots
  for (int f0 = 0; f0 < F; f0 += MMR_NT / 16) {  // (block-uniform trip count: the folds run with whole waves)
    const int f = f0 + grp;
    const int r = f < F ? s_row[f] : -1;
    float dot = 0.f, xx = 0.f;
    if (r >= 0) lzk_dot16_part(s_q, X + (long)r * ldx, D, vec, part, dot, xx);
    dot = lzk_fold16(dot);
    xx = lzk_fold16(xx);
    if (part == 0 && f < F) {
      const float xn = sqrtf(xx);
      s_nrm[f] = xn;
      s_rel[f] = lzk_cos(dot, qn, xn);
    }
  }
  __syncthreads();

  const float w = 1.f - delta;
  for (int t = 0; t < k; ++t) {
    if (tid < 64) {  // wave 0: slot `lane`
      const int r = lane < F ? s_row[lane] : -1;
      const float mx = t == 0 ? 0.f : s_max[lane];
      const float o = r >= 0 ? w * s_rel[lane] - delta * mx : LZK_NEG_INF;
      float bs = o;
      int br = r >= 0 ? r : MMR_NONE;
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) {
        const float s2 = __shfl_xor(bs, off, 64);
        const int r2 = __shfl_xor(br, off, 64);
        if (better(s2, r2, bs, br)) { bs = s2; br = r2; }
      }
      // one value for the whole wave, then the lowest slot that holds it
      bs = __shfl(bs, 0, 64);
      br = __shfl(br, 0, 64);
      const unsigned long long hit = __ballot(r >= 0 && r == br && o == bs);
      const int slot = (br != MMR_NONE && hit) ? __ffsll((long long)hit) - 1 : -1;
      if (slot >= 0) {
        if (lane == 0) {
          pick[m * k + t] = slot;
          obj[m * k + t] = bs;
          s_pick = slot;
          s_row[slot] = -1;
        }
      } else {  // the pool ran out: padding from here on
        for (int j = t + lane; j < k; j += 64) {
          pick[m * k + j] = -1;
          obj[m * k + j] = LZK_NEG_INF;
        }
        if (lane == 0) s_pick = -1;
      }
    }
    __syncthreads();
    const int slot = s_pick;
    if (slot < 0 || t == k - 1) break;  // (block-uniform)
    // ---- the picked row to LDS, then its cosine to every remaining slot
    {
      const long r = cand[m * F + slot];  // (validated when s_row was filled)
      const float* xr = X + r * ldx;
      if (vec) {
        for (int d4 = tid; d4 < (D >> 2); d4 += MMR_NT)
          *reinterpret_cast<float4*>(s_p + 4 * d4) = *reinterpret_cast<const float4*>(xr + 4 * d4);
      } else {
        for (int d = tid; d < Dq; d += MMR_NT) s_p[d] = d < D ? xr[d] : 0.f;
      }
    }
    __syncthreads();
    const float pn = s_nrm[slot];
    for (int f0 = 0; f0 < F; f0 += MMR_NT / 16) {
      const int f = f0 + grp;
      const int r = f < F ? s_row[f] : -1;
      float dot = 0.f, xx = 0.f;
      if (r >= 0) lzk_dot16_part(s_p, X + (long)r * ldx, D, vec, part, dot, xx);
      dot = lzk_fold16(dot);
      if (part == 0 && r >= 0) s_max[f] = fmaxf(s_max[f], lzk_cos(dot, s_nrm[f], pn));
    }
    __syncthreads();
  }
}

}  // namespace

// MMR picks of M pools. X fp32 [n, D] with row stride ldx; Q fp32 [M, D] with
// row stride ldq; cand int64 [M, F] graph rows (< 0 or >= n: empty), F <= 64;
// 1 <= k <= F; 0 <= delta <= 1. pick int32 [M, k]: the pool slot of each pick
// in pick order, -1 once the pool ran out; obj fp32 [M, k]: the objective at
// each pick, -inf for padding.
LZK_EXPORT int lzk_mmr_select(const float* X, long ldx, long n, const float* Q, long ldq, int M, int D,
                              const long* cand, int F, int k, float delta, int* pick, float* obj, void* stream) {
  if (D <= 0 || F < 1 || F > MMR_MAX_F || k < 1 || k > F || M < 0 || n < 0 || n >= (1L << 31) || ldx < D || ldq < D)
    return (int)hipErrorInvalidValue;
  if (!(delta >= 0.f && delta <= 1.f)) return (int)hipErrorInvalidValue;
  const size_t lds = 2 * (size_t)((D + 3) & ~3) * sizeof(float);
  if (lds > MMR_MAX_LDS) return (int)hipErrorInvalidValue;  // (D > 8192: the query and the picked row do not fit)
  if (M == 0) return 0;
  if (!Q || !cand || !pick || !obj || (!X && n > 0)) return (int)hipErrorInvalidValue;
  const int vec = (D % 4 == 0) && (ldx % 4 == 0) && (((uintptr_t)X & 15) == 0);
  (void)hipFuncSetAttribute((const void*)mmr_select_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(mmr_select_kernel, dim3(M), dim3(MMR_NT), lds, (hipStream_t)stream, X, ldx, (int)n, Q, ldq, D,
                     cand, F, k, delta, pick, obj, vec);
  return (int)hipGetLastError();
}
