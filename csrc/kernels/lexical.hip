// Keyword and hybrid search (lexical=): the BM25 scan over a tenant's lexical
// columns and the fusion of its pool with the dense pool
// (lazzaro_amd/ops/lex_ops.py holds the contract in full).
//
// Columns. slots u32 [n, W], W in {8, 16, 32}, rows 16-byte aligned: a slot is
// (t << 8) | tf with a 24-bit term id t and tf in 1 .. 255, the used slots
// first, ascending by t, then zeros. dl int32 [n]: the row's word count.
//
// Score of query m and row r, fp64 in exactly this order, contraction off:
//
//   K(r)    = k1 * ((1 - b) + b * (dl[r] / avgdl))
//   c(j)    = w[m, t_j] * ((tf_j * (k1 + 1)) / (tf_j + K(r)))    used slot j whose term is a query term
//   s(m, r) = (float)(sum of c(j) in ascending slot order)
//
// The weights w (the idf of every query term) and avgdl come from the host: no
// kernel computes a logarithm. A row is eligible when bias[r] is finite and
// s > 0. lex_row_scores is the one device function that computes s, for the
// scan (8 queries against their merged term table) and for the fusion (one
// query against its own table). A term the query does not hold has weight 0
// in the table and is skipped; so is a query term of weight 0: adding c = 0 to
// a sum that starts at +0 changes no bit.
//
// lex_scan_kernel. Block (x, y) serves the tile of 8 queries y and the rows
// x * 256 + tid, strided by gridDim.x * 256 (a capped grid). The tile's merged
// term table (256 sorted ids, 0xffffffff padded, duplicates allowed: every
// instance carries the weights of all 8 queries) and its weights sit in LDS;
// a thread loads its row's slots with 16-byte loads, drops the slots whose
// term is not in the tile's 8,192-bit term set (one independent LDS read per
// slot, the set built from the table when the block starts; with at most 256
// terms set about 3 % of the other slots pass) and finds each remaining term
// by a lower-bound search of 8 dependent steps. A match with s > 0 is pushed as a
// 64-bit (score, row) key -- lzk_topk64.h's -- into the query's LDS buffer
// under an LDS atomic counter. Before a step that could overflow a buffer (more than
// LX_FLUSH entries held, 256 more possible) the block reduces it to its best
// 64 by the bitonic tournament, takes the 64th as the query's threshold -- a
// later key below it is not pushed: it could never return -- and goes on. Each block writes one partial
// list of 64 per query, ps / pi [M, gridDim.x, 64], which lzk_cand_select_wide
// merges (its order is the contract's: score descending, row ascending). Keys
// are totally ordered, so the result does not depend on arrival order.
//
// lex_fuse_kernel. One block per query: the candidates are the dense pool and
// the lexical pool (a row listed twice counts once), each scored
//   (1 - alpha) * cos(q, v) + alpha * (s(m, v) / den[m])          fp32, contraction off
// with cos over the fp32 rows by the 16-lane dot of lzk_dot16.h (mmr.hip's
// summation order: at most L(D) = 4 ceil(D / 64) + 4 roundings a dot) and s by
// lex_row_scores; the `k` best by (blend descending, row ascending) come back,
// (-inf, -1) once the candidates run out.
//
// The key and the tournament are lzk_topk64.h's.
#include "lzk_common.h"
#include "lzk_dot16.h"
#include "lzk_topk64.h"

namespace {

constexpr int LX_NT = 256;
constexpr int LX_TQ = 8;                   // queries per tile
constexpr int LX_T = 32;                   // terms per query
constexpr int LX_UT = LX_TQ * LX_T;        // entries of a tile's merged table
constexpr int LX_KB = 640;                 // keys per query in LDS: the running best 64 + 576 entries
constexpr int LX_ROOM = LX_KB - 64;
constexpr int LX_FLUSH = LX_ROOM - LX_NT;  // a step pushes at most one key per thread and query
constexpr int LX_BITS = 8192;              // bits of a tile's term set (one word per thread)
constexpr int LX_MAX_C = 128;              // fused candidates per query: two pools of 64
constexpr size_t LX_MAX_LDS = 64 * 1024;

struct LexParams {
  double k1, kp1, omb, b, avgdl;  // k1, k1 + 1, 1 - b, b, avgdl
};

// s(., r) before the rounding to fp32, for the NQ queries of a term table:
// tab[TN] sorted ascending (0xffffffff padded), tw[TN][NQ] the weight of each
// entry's term for each query (0: the query does not hold it). `row`: the
// row's W slots (16-byte aligned), loaded whole before anything is tested.
// BITS (the scan): `bits` is a LX_BITS-bit set of the table's terms by their
// low bits; a slot whose bit is clear cannot match and skips the search (a set
// bit proves nothing: the search decides). Whichever instance of a term listed
// more than once the search lands on carries the same weights. The matching
// slots are added in ascending slot order either way.
template <int NQ, int TN, int W, bool BITS>
__device__ __forceinline__ void lex_row_scores(const unsigned* __restrict__ row, int dl, const unsigned* tab,
                                               const double* tw, const unsigned* bits, const LexParams& p,
                                               double (&acc)[NQ]) {
#pragma clang fp contract(off)
  unsigned sl[W];
#pragma unroll
  for (int j4 = 0; j4 < W; j4 += 4) {
    const uint4 v = *reinterpret_cast<const uint4*>(row + j4);
    sl[j4] = v.x; sl[j4 + 1] = v.y; sl[j4 + 2] = v.z; sl[j4 + 3] = v.w;
  }
  unsigned hit = 0;
#pragma unroll
  for (int j = 0; j < W; ++j) {
    const unsigned t = sl[j] >> 8;
    bool h = sl[j] != 0u;
    if (BITS) h = h && ((bits[(t >> 5) & (LX_BITS / 32 - 1)] >> (t & 31u)) & 1u);
    hit |= (h ? 1u : 0u) << j;
  }
#pragma unroll
  for (int q = 0; q < NQ; ++q) acc[q] = 0.0;
  if (hit == 0u) return;
  const double K = p.k1 * (p.omb + p.b * ((double)dl / p.avgdl));
#pragma unroll
  for (int j = 0; j < W; ++j) {
    if (!((hit >> j) & 1u)) continue;
    const unsigned t = sl[j] >> 8;
    int lo = 0;  // the number of entries below t, at most TN - 1
#pragma unroll
    for (int step = TN >> 1; step > 0; step >>= 1)
      if (tab[lo + step - 1] < t) lo += step;
    if (tab[lo] != t) continue;
    const double tf = (double)(sl[j] & 255u);
    const double x = (tf * p.kp1) / (tf + K);
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const double w = tw[lo * NQ + q];
      if (w != 0.0) acc[q] = acc[q] + w * x;
    }
  }
}

template <int W>
__global__ __launch_bounds__(LX_NT) void lex_scan_kernel(const unsigned* __restrict__ slots,
                                                         const int* __restrict__ dl, const float* __restrict__ bias,
                                                         int n, const unsigned* __restrict__ utab,
                                                         const double* __restrict__ uw, int M, LexParams p,
                                                         float* __restrict__ ps, int* __restrict__ pi) {
  __shared__ u64 s_keys[LX_TQ * LX_KB];
  __shared__ double s_w[LX_UT * LX_TQ];
  __shared__ unsigned s_tab[LX_UT];
  __shared__ unsigned s_bits[LX_BITS / 32];
  __shared__ u64 s_thr[LX_TQ];  // the query's 64th best key so far (0 until 64 are held): nothing below it is kept
  __shared__ int s_cnt[LX_TQ];
  const int tid = threadIdx.x, tile = blockIdx.y, blk = blockIdx.x, nblk = gridDim.x;

  const unsigned mine = utab[(long)tile * LX_UT + tid];  // (LX_NT == LX_UT entries)
  s_tab[tid] = mine;
  s_bits[tid] = 0u;  // (LX_BITS / 32 == LX_NT words)
  __syncthreads();
  if (mine != 0xffffffffu) atomicOr(&s_bits[(mine >> 5) & (LX_BITS / 32 - 1)], 1u << (mine & 31u));
  for (int i = tid; i < LX_UT * LX_TQ; i += LX_NT) s_w[i] = uw[(long)tile * LX_UT * LX_TQ + i];
  for (int i = tid; i < LX_TQ * 64; i += LX_NT) s_keys[(i >> 6) * LX_KB + (i & 63)] = 0;
  if (tid < LX_TQ) {
    s_cnt[tid] = 0;
    s_thr[tid] = 0;
  }

  // reduce query q's buffer of c entries into its running best 64 (block-uniform call)
  auto reduce = [&](int q, int c) {
    u64* kq = s_keys + q * LX_KB;
    const int padded = (c + 63) & ~63;
    for (int i = c + tid; i < padded; i += LX_NT) kq[64 + i] = 0;
    topk64_rounds(kq, 1, 1 + padded / 64);
    if (tid == 0) {  // (every thread read the count before the tournament's first barrier)
      s_cnt[q] = 0;
      s_thr[q] = kq[63];
    }
  };

  for (long base = (long)blk * LX_NT; base < n; base += (long)nblk * LX_NT) {
    __syncthreads();
    for (int q = 0; q < LX_TQ; ++q) {
      const int c = s_cnt[q];
      if (c > LX_FLUSH) reduce(q, c);
    }
    __syncthreads();
    const long r = base + tid;
    if (r < n) {
      const float bv = bias[r];
      if (fabsf(bv) <= 3.402823466e+38f) {  // finite
        double acc[LX_TQ];
        lex_row_scores<LX_TQ, LX_UT, W, true>(slots + r * W, dl[r], s_tab, s_w, s_bits, p, acc);
#pragma unroll
        for (int q = 0; q < LX_TQ; ++q) {
          const float s = (float)acc[q];
          if (s > 0.f) {
            const u64 key = wide_key(s, (int)r);
            if (key > s_thr[q]) {  // (a key below the 64th best so far can never return)
              const int pos = atomicAdd(&s_cnt[q], 1);  // < LX_FLUSH + 1 + LX_NT <= LX_ROOM
              s_keys[q * LX_KB + 64 + pos] = key;
            }
          }
        }
      }
    }
  }
  __syncthreads();
  for (int q = 0; q < LX_TQ; ++q) {
    const int c = s_cnt[q];
    if (c > 0) reduce(q, c);
  }
  __syncthreads();
  for (int i = tid; i < LX_TQ * 64; i += LX_NT) {
    const int q = i >> 6, t = i & 63;
    const long m = (long)tile * LX_TQ + q;
    if (m < M) {
      float v;
      int r;
      wide_unkey(s_keys[q * LX_KB + t], v, r);
      const long o = (m * nblk + blk) * 64 + t;
      ps[o] = v;
      pi[o] = r;
    }
  }
}

__device__ __forceinline__ float lex_blend(float alpha, float cosv, float s, float den) {
#pragma clang fp contract(off)
  const float lexn = den > 0.f ? s / den : 0.f;
  const float w0 = 1.f - alpha;
  return w0 * cosv + alpha * lexn;
}

__global__ __launch_bounds__(LX_NT) void lex_fuse_kernel(const float* __restrict__ X, long ldx, int n,
                                                         const float* __restrict__ Q, long ldq, int D, int vec,
                                                         const long* __restrict__ dpool,
                                                         const long* __restrict__ lpool, int P,
                                                         const unsigned* __restrict__ slots,
                                                         const int* __restrict__ dl, int W,
                                                         const unsigned* __restrict__ qt,
                                                         const double* __restrict__ qw,
                                                         const float* __restrict__ den, LexParams p, float alpha,
                                                         int k, float* __restrict__ os, long* __restrict__ oi) {
  extern __shared__ __attribute__((aligned(16))) float s_q[];  // [Dq] the query, zero padded
  __shared__ u64 s_keys[LX_MAX_C];
  __shared__ double s_tw[LX_T];
  __shared__ unsigned s_tab[LX_T];
  __shared__ int s_row[LX_MAX_C];
  const int Dq = (D + 3) & ~3;
  const int tid = threadIdx.x, lane = tid & 63, part = lane & 15, grp = tid >> 4;
  const long m = blockIdx.x;

  for (int d = tid; d < Dq; d += LX_NT) s_q[d] = d < D ? Q[m * ldq + d] : 0.f;
  if (tid < LX_T) {
    s_tab[tid] = qt[m * LX_T + tid];
    s_tw[tid] = qw[m * LX_T + tid];
  }
  long mine = -1;
  if (tid < LX_MAX_C) {
    if (dpool) {
      if (tid < P) mine = dpool[m * P + tid];
      else if (tid < 2 * P) mine = lpool[m * P + tid - P];
    } else if (tid < P) {
      mine = lpool[m * P + tid];
    }
    if (mine < 0 || mine >= n) mine = -1;  // (an empty slot, or a row the tenant does not have: never read)
    s_row[tid] = (int)mine;
  }
  __syncthreads();
  bool dup = false;
  if (tid < LX_MAX_C && mine >= 0)
    for (int j = 0; j < tid; ++j) dup |= s_row[j] == (int)mine;  // (a row of both pools counts once)
  __syncthreads();
  if (dup) s_row[tid] = -1;
  __syncthreads();

  // |q|: every group sums the same shares in the same order
  const float qn = sqrtf(lzk_fold16(lzk_sq16_part(s_q, D, vec, part)));
  const float dn = den[m];

  for (int f0 = 0; f0 < LX_MAX_C; f0 += LX_NT / 16) {  // (block-uniform trip count: the folds run with whole waves)
    const int f = f0 + grp;
    const int r = s_row[f];
    float dot = 0.f, xx = 0.f;
    if (r >= 0) lzk_dot16_part(s_q, X + (long)r * ldx, D, vec, part, dot, xx);
    dot = lzk_fold16(dot);
    xx = lzk_fold16(xx);
    if (part == 0) {
      u64 key = 0;
      if (r >= 0) {
        double acc[1];
        const unsigned* row = slots + (long)r * W;
        if (W == 8) lex_row_scores<1, LX_T, 8, false>(row, dl[r], s_tab, s_tw, nullptr, p, acc);
        else if (W == 16) lex_row_scores<1, LX_T, 16, false>(row, dl[r], s_tab, s_tw, nullptr, p, acc);
        else lex_row_scores<1, LX_T, 32, false>(row, dl[r], s_tab, s_tw, nullptr, p, acc);
        key = wide_key(lex_blend(alpha, lzk_cos(dot, qn, sqrtf(xx)), (float)acc[0], dn), r);
      }
      s_keys[f] = key;
    }
  }
  topk64_rounds(s_keys, 0, LX_MAX_C / 64);
  if (tid < k) {
    float v;
    int r;
    wide_unkey(s_keys[tid], v, r);
    os[m * k + tid] = v;
    oi[m * k + tid] = r;
  }
}

inline bool lex_w_ok(int W) { return W == 8 || W == 16 || W == 32; }

}  // namespace

// Row blocks (gridDim.x) lzk_lex_scan uses for n rows and M queries (cap <= 0:
// its own choice -- about 512 blocks over all query tiles, at least 16 row
// blocks, never more than the rows fill): ps / pi hold M * blocks * 64 entries.
LZK_EXPORT int lzk_lex_scan_blocks(long n, int M, int cap) {
  if (n <= 0 || M <= 0) return 1;
  const int tiles = (M + LX_TQ - 1) / LX_TQ;
  long nb = cap > 0 ? cap : (512 / tiles > 16 ? 512 / tiles : 16);
  const long full = (n + LX_NT - 1) / LX_NT;
  if (nb > full) nb = full;
  if (nb > 1024) nb = 1024;
  return (int)(nb < 1 ? 1 : nb);
}

// The BM25 partial pass. slots / dl / bias: the columns over rows [0, n);
// utab u32 [tiles, 256] and uw f64 [tiles, 256, 8]: the merged term table of
// every tile of 8 queries and its weights (ops/lex_ops.py tile_tables);
// ps fp32 / pi int32 [M, nblk, 64]: the partial lists, descending, (-inf, -1)
// padded. nblk: the row blocks, 1 .. 1024 -- ps / pi MUST hold M * nblk * 64
// entries, which nothing here can check: take nblk from lzk_lex_scan_blocks(n,
// M, cap) and size the lists by it. nblk <= 0: that function's own choice
// (cap = 0) is taken here, for lists sized by it.
LZK_EXPORT int lzk_lex_scan(const unsigned* slots, const int* dl, const float* bias, long n, int W,
                            const unsigned* utab, const double* uw, int M, double k1, double b, double avgdl, int nblk,
                            float* ps, int* pi, void* stream) {
  if (M <= 0 || n <= 0) return 0;
  if (nblk <= 0) nblk = lzk_lex_scan_blocks(n, M, 0);
  if (!lex_w_ok(W) || n >= (1L << 31) || nblk < 1 || nblk > 1024 || !slots || !dl || !bias || !utab || !uw || !ps || !pi)
    return (int)hipErrorInvalidValue;
  if (((uintptr_t)slots & 15) != 0 || !(avgdl > 0.0) || !(k1 >= 0.0) || !(b >= 0.0 && b <= 1.0))
    return (int)hipErrorInvalidValue;
  const int tiles = (M + LX_TQ - 1) / LX_TQ;
  if (tiles > 65535) return (int)hipErrorInvalidValue;
  const LexParams p{k1, k1 + 1.0, 1.0 - b, b, avgdl};
  const dim3 grid((unsigned)nblk, (unsigned)tiles);
  hipStream_t st = (hipStream_t)stream;
  if (W == 8)
    hipLaunchKernelGGL(lex_scan_kernel<8>, grid, dim3(LX_NT), 0, st, slots, dl, bias, (int)n, utab, uw, M, p, ps, pi);
  else if (W == 16)
    hipLaunchKernelGGL(lex_scan_kernel<16>, grid, dim3(LX_NT), 0, st, slots, dl, bias, (int)n, utab, uw, M, p, ps, pi);
  else
    hipLaunchKernelGGL(lex_scan_kernel<32>, grid, dim3(LX_NT), 0, st, slots, dl, bias, (int)n, utab, uw, M, p, ps, pi);
  return (int)hipGetLastError();
}

// The fusion. X fp32 [n, D] (row stride ldx), Q fp32 [M, D] (row stride ldq);
// dpool (or null: no dense pool) and lpool int64 [M, P], P <= 64, graph rows
// (< 0 or >= n: empty); qt u32 [M, 32] each query's terms ascending, 0xffffffff
// padded; qw f64 [M, 32] their weights; den fp32 [M]; 1 <= k <= 64. os fp32 /
// oi int64 [M, k]: the blend and the row, descending, (-inf, -1) padded.
LZK_EXPORT int lzk_lex_fuse(const float* X, long ldx, long n, const float* Q, long ldq, int M, int D,
                            const long* dpool, const long* lpool, int P, const unsigned* slots, const int* dl, int W,
                            const unsigned* qt, const double* qw, const float* den, double k1, double b, double avgdl,
                            float alpha, int k, float* os, long* oi, void* stream) {
  if (D <= 0 || P < 1 || P > 64 || k < 1 || k > 64 || M < 0 || n < 0 || n >= (1L << 31) || ldx < D || ldq < D)
    return (int)hipErrorInvalidValue;
  if (!lex_w_ok(W) || !(alpha >= 0.f && alpha <= 1.f) || !(avgdl > 0.0) || !(k1 >= 0.0) || !(b >= 0.0 && b <= 1.0))
    return (int)hipErrorInvalidValue;
  const size_t lds = (size_t)((D + 3) & ~3) * sizeof(float);
  if (lds > LX_MAX_LDS - 4096) return (int)hipErrorInvalidValue;
  if (M == 0) return 0;
  if (!Q || !lpool || !qt || !qw || !den || !os || !oi || ((!X || !slots || !dl) && n > 0) ||
      ((uintptr_t)slots & 15) != 0)
    return (int)hipErrorInvalidValue;
  const int vec = (D % 4 == 0) && (ldx % 4 == 0) && (((uintptr_t)X & 15) == 0);
  const LexParams p{k1, k1 + 1.0, 1.0 - b, b, avgdl};
  hipLaunchKernelGGL(lex_fuse_kernel, dim3((unsigned)M), dim3(LX_NT), lds, (hipStream_t)stream, X, ldx, (int)n, Q,
                     ldq, D, vec, dpool, lpool, P, slots, dl, W, qt, qw, den, p, alpha, k, os, oi);
  return (int)hipGetLastError();
}
