// Multi-query search (fuse=): the pools of a group of sub-queries are fused
// into one ranked list on the device (lazzaro_amd/ops/fuse_ops.py holds the
// contract in full). One block per group.
//
//   pools      sub-query j of the group has a pool of P slots (graph rows, < 0
//              or >= n: empty). rank_j(v) = 1 + the number of non-empty slots
//              before the FIRST occurrence of v in pool j; a later occurrence
//              is ignored for the score but counts as a slot for those after.
//   candidates the union of the group's pools, at most 16 x 64 = 1024 rows;
//              support(v) = the number of pools that hold v
//   rrf        score(v) = (float)(sum in sub-query order over the pools that
//              hold v of (double)w_j / ((double)rrf_k + rank_j(v))), fp64 with
//              nothing contracted, rounded once
//   mean       score(v) = sum_j wn_j cos(q_j, v) over ALL sub-queries of the
//              group, an fp32 fmaf chain in sub-query order from 0; cos over
//              the fp32 rows and queries, 0 when either norm is 0
//   result     the k largest by the fp32 score, ties to the lower row,
//              (-inf, -1, support 0) beyond the candidate count
//
// Layout. FUSE_NT = 256 threads. The candidate table is lzk_rowset.h's, as in
// expand.hip: an open-addressing hash of FUSE_HASH = 2048 slots (at most
// FUSE_MAX_CAND = 1024 keys, so it never fills) keyed by the row, and a dense
// list of the rows in arrival order. s_idx maps a hash slot to the row's place
// in the dense list. The ranks are a byte matrix [1024][16] over (place,
// sub-query), 0 = absent.
//
// Phases. (1) every thread inserts pool slots: the table and the list. (2)
// after a barrier thread j < G walks pool j in slot order with a rank counter
// of its own, looks each row up (never inserts) and writes cell (place, j) if
// it is still 0: one writer per cell, so the first-occurrence rule does not
// depend on the arrival order. (3) scores: rrf -- one thread per candidate
// sums its row of the matrix in j order; mean -- 16 lanes per candidate gather
// the row ONCE and dot it against every staged query. (4) 64-bit (score, row)
// keys and the bitonic tournament of 64-entry blocks (lzk_topk64.h, every
// block unsorted: b0 = 0). The order of the dense list depends on arrival;
// nothing that is returned does: keys are totally ordered and support is
// looked up by row.
//
// mean: summation order and error. The group's queries sit in LDS, zero
// padded to a multiple of 4 floats (G * ceil4(D) <= 16384 floats, 64 KiB).
// fuse_dots16 is lzk_dot16_part with one accumulator per staged query: lane
// `part` takes the same fixed share of the dimensions in the same ascending
// order, one fma each, and lzk_fold16 folds the 16 partial sums. One dot
// therefore passes through at most L(D) = 4 ceil(D / 64) + 4 fp32 roundings
// and, as derived in mmr.hip, |cos32 - cos64| <= (2 L(D) + 8) 2^-24 (L for the
// dot, L jointly for the two norms, 8 for the square roots, the product and
// the quotient). The fp64 score of the contract uses the same fp32 weights
// wn_j = (float)(w_j / sum w), so the weights carry no error of their own;
// they are >= 0 and sum to at most 1 + G 2^-25, so the cosine errors enter
// weighted and do not add beyond the largest (times 1 + G 2^-25). The chain
// rounds once per fmaf, G times, each on a partial sum of magnitude <= 1 +
// (2 L(D) + 8) 2^-24 < 2: at most one unit of 2^-24 each. With 2 units of
// slack for the second-order terms (the weights' sum above 1, a |cos32| above
// 1 by its own error inside the products):
//   |score32 - score64| <= (2 L(D) + 8 + G + 2) 2^-24            (fuse_tol in ops/fuse_ops.py)
// Identical rows get identical cosines, so equal scores give equal bits.
#include "lzk_common.h"
#include "lzk_dot16.h"
#include "lzk_rowset.h"
#include "lzk_topk64.h"

namespace {

constexpr int FUSE_NT = 256;
constexpr int FUSE_MAX_Q = 16;       // sub-queries per group
constexpr int FUSE_MAX_P = 64;       // slots per pool
constexpr int FUSE_MAX_CAND = 1024;  // FUSE_MAX_Q * FUSE_MAX_P: the union cannot exceed it
constexpr int FUSE_HASH = 2048;
constexpr int FUSE_MAX_K = 64;
constexpr int FUSE_MAX_QF = 16384;   // floats of staged queries: 64 KiB beside the 48 KiB of tables

// lzk_dot16_part's order with one accumulator per staged query: this lane's
// share of <q_j, x> for j < G and of |x|^2; the row is loaded once.
__device__ __forceinline__ void fuse_dots16(const float* s_q, int Dq, int G, const float* __restrict__ x, int D, int vec,
                                            int part, float (&dot)[FUSE_MAX_Q], float& xx) {
#pragma unroll
  for (int j = 0; j < FUSE_MAX_Q; ++j) dot[j] = 0.f;
  xx = 0.f;
  if (vec) {
    const int n4 = D >> 2;
    for (int d4 = part; d4 < n4; d4 += 16) {
      const float4 xv = *reinterpret_cast<const float4*>(x + 4 * d4);
      xx = fmaf(xv.x, xv.x, xx); xx = fmaf(xv.y, xv.y, xx); xx = fmaf(xv.z, xv.z, xx); xx = fmaf(xv.w, xv.w, xx);
#pragma unroll
      for (int j = 0; j < FUSE_MAX_Q; ++j) {
        if (j < G) {
          const float4 av = *reinterpret_cast<const float4*>(s_q + (long)j * Dq + 4 * d4);
          dot[j] = fmaf(av.x, xv.x, dot[j]); dot[j] = fmaf(av.y, xv.y, dot[j]);
          dot[j] = fmaf(av.z, xv.z, dot[j]); dot[j] = fmaf(av.w, xv.w, dot[j]);
        }
      }
    }
  } else {
    for (int d = part; d < D; d += 16) {
      const float xv = x[d];
      xx = fmaf(xv, xv, xx);
#pragma unroll
      for (int j = 0; j < FUSE_MAX_Q; ++j)
        if (j < G) dot[j] = fmaf(s_q[(long)j * Dq + d], xv, dot[j]);
    }
  }
}

// mode 0: rrf, 1: mean. gcap: the most sub-queries a group may have (the LDS
// was sized by it for mean); a group outside 1 .. gcap, or outside the M
// queries, is served as an empty one.
__global__ __launch_bounds__(FUSE_NT) void fuse_select_kernel(
    const float* __restrict__ X, long ldx, int n, const float* __restrict__ Q, long ldq, int M, int D,
    const long* __restrict__ off, const long* __restrict__ pools, int P, const float* __restrict__ w, int mode,
    float rrf_k, int gcap, int k, long* __restrict__ orow, float* __restrict__ oscore, int* __restrict__ osup,
    int* __restrict__ ncand, int vec) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) float s_q[];  // mean: [G][Dq] the group's queries, zero padded
  __shared__ u64 s_keys[FUSE_MAX_CAND];
  __shared__ int s_key[FUSE_HASH];    // row of the hash slot, -1 = free
  __shared__ int s_idx[FUSE_HASH];    // its place in the dense list
  __shared__ int s_list[FUSE_MAX_CAND];   // rows in arrival order
  __shared__ float s_score[FUSE_MAX_CAND];
  __shared__ __attribute__((aligned(16))) unsigned char s_rank[FUSE_MAX_CAND * FUSE_MAX_Q];  // [place][sub-query], 0 = absent
  __shared__ float s_qn[FUSE_MAX_Q];
  __shared__ float s_w[FUSE_MAX_Q];
  __shared__ int s_cnt;
  const int tid = threadIdx.x, part = tid & 15, grp = tid >> 4;
  const long g = blockIdx.x;
  const int Dq = (D + 3) & ~3;

  long base = off[g];
  long Gl = off[g + 1] - base;
  if (base < 0 || Gl < 1 || Gl > gcap || base + Gl > M) { base = 0; Gl = 0; }
  const int G = (int)Gl;

  for (int h = tid; h < FUSE_HASH; h += FUSE_NT) s_key[h] = -1;
  {
    unsigned* z = reinterpret_cast<unsigned*>(s_rank);
    for (int i = tid; i < FUSE_MAX_CAND * FUSE_MAX_Q / 4; i += FUSE_NT) z[i] = 0u;
  }
  if (tid < FUSE_MAX_Q) s_w[tid] = tid < G ? w[base + tid] : 0.f;
  if (tid == 0) s_cnt = 0;
  if (mode == 1)
    for (int j = 0; j < G; ++j)
      for (int d = tid; d < Dq; d += FUSE_NT) s_q[(long)j * Dq + d] = d < D ? Q[(base + j) * ldq + d] : 0.f;
  __syncthreads();

  // ---- (1) the union: the table and the dense list
  for (int t = tid; t < G * P; t += FUSE_NT) {
    const long r = pools[base * P + t];
    if (r >= 0 && r < n)  // (the list never fills: G * P <= 1024 slots are inserted)
      lzk_rowset_insert<FUSE_HASH, FUSE_MAX_CAND>((int)r, s_key, s_list, &s_cnt,
                                                  [&](unsigned h, int i) { s_idx[h] = i; });
  }
  __syncthreads();
  const int cnt = min(s_cnt, FUSE_MAX_CAND);

  // ---- (2) ranks: thread j walks pool j in slot order; cell (place, j) has this one writer
  if (tid < G) {
    const long* pj = pools + (base + tid) * P;
    int seen = 0;  // non-empty slots so far
    for (int s = 0; s < P; ++s) {
      const long r = pj[s];
      if (r < 0 || r >= n) continue;
      ++seen;
      const int i = lzk_rowset_find<FUSE_HASH>((int)r, s_key, s_idx);  // its place in the dense list
      if (i >= 0 && i < FUSE_MAX_CAND && s_rank[i * FUSE_MAX_Q + tid] == 0) s_rank[i * FUSE_MAX_Q + tid] = (unsigned char)seen;
    }
  }
  // |q_j| (mean): group j sums query j's shares in lzk_dot16_part's order
  if (mode == 1 && grp < G) {
    // (a group of 16 lanes is whole or absent: grp is uniform over it)
    const float qq = lzk_fold16(lzk_sq16_part(s_q + (long)grp * Dq, D, vec, part));
    if (part == 0) s_qn[grp] = sqrtf(qq);
  }
  __syncthreads();

  // ---- (3) scores
  if (mode == 0) {
    const double kk = (double)rrf_k;
    for (int i = tid; i < cnt; i += FUSE_NT) {
      double acc = 0.0;
      for (int j = 0; j < G; ++j) {
        const int r = s_rank[i * FUSE_MAX_Q + j];
        if (r) acc = acc + (double)s_w[j] / (kk + (double)r);
      }
      s_score[i] = (float)acc;
    }
  } else {
    for (int i0 = 0; i0 < cnt; i0 += FUSE_NT / 16) {  // (block-uniform trip count: the folds run with whole waves)
      const int i = i0 + grp;
      const int r = i < cnt ? s_list[i] : -1;
      float dot[FUSE_MAX_Q], xx = 0.f;
      if (r >= 0) {
        fuse_dots16(s_q, Dq, G, X + (long)r * ldx, D, vec, part, dot, xx);
      } else {
#pragma unroll
        for (int j = 0; j < FUSE_MAX_Q; ++j) dot[j] = 0.f;
      }
      xx = lzk_fold16(xx);
      const float xn = sqrtf(xx);
      float sc = 0.f;
#pragma unroll
      for (int j = 0; j < FUSE_MAX_Q; ++j) {
        if (j < G) {
          const float dj = lzk_fold16(dot[j]);
          sc = fmaf(s_w[j], lzk_cos(dj, s_qn[j], xn), sc);
        }
      }
      if (part == 0 && r >= 0) s_score[i] = sc;
    }
  }
  __syncthreads();

  // ---- (4) the k best by (score, row)
  const int nb = cnt > 0 ? (cnt + 63) >> 6 : 1;
  for (int i = tid; i < 64 * nb; i += FUSE_NT) s_keys[i] = i < cnt ? wide_key(s_score[i], s_list[i]) : 0ull;
  topk64_rounds(s_keys, 0, nb);
  if (tid < k) {
    float v;
    int r;
    wide_unkey(s_keys[tid], v, r);
    int sup = 0;
    if (r >= 0) {
      const int i = lzk_rowset_find<FUSE_HASH>(r, s_key, s_idx);
      if (i >= 0 && i < FUSE_MAX_CAND)
        for (int j = 0; j < G; ++j) sup += s_rank[i * FUSE_MAX_Q + j] != 0;
    }
    orow[g * k + tid] = r;
    oscore[g * k + tid] = v;
    osup[g * k + tid] = sup;
  }
  if (tid == 0) ncand[g] = cnt;
}

}  // namespace

// Fusion of the pools of NG groups of sub-queries. X fp32 [n, D] with row
// stride ldx and Q fp32 [M, D] with row stride ldq (mode 1 only; mode 0 reads
// neither); off int64 [NG + 1] on the device, ascending from 0 to M, every
// group 1 .. gmax sub-queries and gmax <= 16 (the caller validated them on
// the host: a group outside that is served as empty, never read out of
// bounds); pools int64 [M, P], P <= 64, graph rows (< 0 or >= n: empty); w
// fp32 [M]: mode 0 the weights, mode 1 the weights normalised per group.
// mode 1: gmax * ceil4(D) <= 16384. rows int64, scores fp32, support int32
// [NG, k], 1 <= k <= 64 (padding -1, -inf, 0); ncand int32 [NG].
LZK_EXPORT int lzk_fuse_select(const float* X, long ldx, long n, const float* Q, long ldq, int M, int D,
                               const long* off, int NG, int gmax, const long* pools, int P, const float* w, int mode,
                               float rrf_k, int k, long* rows, float* scores, int* support, int* ncand, void* stream) {
  if (M < 0 || NG < 0 || n < 0 || n >= (1L << 31) - 1 || P < 1 || P > FUSE_MAX_P || k < 1 || k > FUSE_MAX_K ||
      gmax < 1 || gmax > FUSE_MAX_Q || (mode != 0 && mode != 1))
    return (int)hipErrorInvalidValue;
  if (mode == 0 && !(rrf_k > 0.f && rrf_k < __builtin_huge_valf())) return (int)hipErrorInvalidValue;
  size_t lds = 0;
  int vec = 0;
  if (mode == 1) {
    if (D <= 0 || ldx < D || ldq < D) return (int)hipErrorInvalidValue;
    const long qf = (long)gmax * ((D + 3) & ~3);
    if (qf > FUSE_MAX_QF) return (int)hipErrorInvalidValue;
    lds = (size_t)qf * sizeof(float);
    vec = (D % 4 == 0) && (ldx % 4 == 0) && (((uintptr_t)X & 15) == 0);
  }
  if (NG == 0) return 0;
  if (!off || !pools || !w || !rows || !scores || !support || !ncand) return (int)hipErrorInvalidValue;
  if (mode == 1 && (!Q || (n > 0 && !X))) return (int)hipErrorInvalidValue;
  if (lds > 0) {
    const hipError_t e = hipFuncSetAttribute((const void*)fuse_select_kernel,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(fuse_select_kernel, dim3((unsigned)NG), dim3(FUSE_NT), lds, (hipStream_t)stream, X, ldx, (int)n, Q,
                     ldq, M, D, off, pools, P, w, mode, rrf_k, gmax, k, rows, scores, support, ncand, vec);
  return (int)hipGetLastError();
}
