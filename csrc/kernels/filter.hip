// Filtered store search (TenantGraph.store_search(..., where=)): metadata
// predicates evaluated over the tenant's HBM columns, and a scan that reads
// only the rows that pass.
//
//   lzk_tg_filter_plan      the predicate over rows [0, n) -> a per-row score
//                           bias (the store bias where the row passes, -inf
//                           where it does not), the passing rows in ascending
//                           order and their count. Three launches: evaluate +
//                           per-block counts, an exclusive scan of the block
//                           counts, ordered writes (a wave ballot prefix inside
//                           the block's range). No atomic append: the row
//                           order is the tie-break of every search.
//   lzk_gather_topk_partial fp32 scores alpha * <q, emb32[row]> + bias[row] of
//                           the listed rows only; per (query, chunk of the
//                           list) the best kslot as (score, graph row), ties to
//                           the lower row. lzk_topk_merge (search.hip) reduces
//                           the chunks.
//
// Indexed scan layout. A 256-thread block takes one chunk of the row list and
// one tile of QT queries (fp32, in LDS). 16 lanes share a row: one wave
// instruction reads 4 rows x 256 contiguous bytes (float4 per lane), every
// loaded float4 is used for all QT queries of the tile, so a listed row is
// read once per query tile. The rows of a chunk are taken 256 at a time (a
// slab): their scores go through LDS, then one wave per query pops the slab's
// entries that beat the query's running list (kept sorted across lanes 0..K-1)
// -- usually none after the first slabs, so the pass costs one wave argmax.
#include "lzk_common.h"
#include "lzk_rowpred.h"

LZK_DEBUG_STATE(filter)

namespace {

constexpr int FP_NT = 256;

// LzkFilterBounds (ops/filter_ops.py FilterBounds), FilterCols and fp_pass: lzk_rowpred.h

// pass 1: bias[i] and the number of passing rows of every 256-row block
__global__ __launch_bounds__(FP_NT) void fp_eval_kernel(FilterCols c, LzkFilterBounds b, const float* __restrict__ sqn,
                                                        long n, float* __restrict__ bias, int* __restrict__ bcount) {
  __shared__ int s_w[FP_NT / 64];
  const long i = (long)blockIdx.x * FP_NT + threadIdx.x;
  bool p = false;
  if (i < n) {
    p = fp_pass(c, b, i);
    const float ok = b.l2 ? 0.0f - sqn[i] : 0.0f;  // (0 - |x|^2, not -|x|^2: +0 for a zero row, as the torch form)
    bias[i] = p ? ok : LZK_NEG_INF;
  }
  const unsigned long long m = __ballot(p);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = __popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) bcount[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// pass 2: exclusive scan of the block counts in place (one block; thread t
// owns a contiguous span), total -> *count
__global__ __launch_bounds__(FP_NT) void fp_scan_kernel(int* __restrict__ bcount, int nb, int* __restrict__ count) {
  __shared__ int s_sum[FP_NT];
  const int t = threadIdx.x;
  const int per = (nb + FP_NT - 1) / FP_NT;
  const int a = min(nb, t * per), e = min(nb, a + per);
  int s = 0;
  for (int j = a; j < e; ++j) s += bcount[j];
  s_sum[t] = s;
  __syncthreads();
  if (t == 0) {
    int run = 0;
    for (int j = 0; j < FP_NT; ++j) { const int v = s_sum[j]; s_sum[j] = run; run += v; }
    *count = run;
  }
  __syncthreads();
  int run = s_sum[t];
  for (int j = a; j < e; ++j) { const int v = bcount[j]; bcount[j] = run; run += v; }
}

// pass 3: the passing rows of block b to rows[boff[b] ...], in row order
__global__ __launch_bounds__(FP_NT) void fp_write_kernel(FilterCols c, LzkFilterBounds b, long n,
                                                         const int* __restrict__ boff, int* __restrict__ rows,
                                                         long rows_cap) {
  __shared__ int s_w[FP_NT / 64];
  const long i = (long)blockIdx.x * FP_NT + threadIdx.x;
  const bool p = i < n && fp_pass(c, b, i);
  const unsigned long long m = __ballot(p);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) s_w[w] = __popcll(m);
  __syncthreads();
  if (!p) return;
  int off = boff[blockIdx.x];
  for (int j = 0; j < w; ++j) off += s_w[j];
  off += __popcll(m & ((1ull << lane) - 1ull));
  if (off >= 0 && off < rows_cap) rows[off] = (int)i;
}

// ---------------------------------------------------------------- indexed scan

constexpr int GS_NT = 256;
constexpr int GS_SLAB = 256;       // rows scored between two selections
constexpr int GS_NONE = 0x7fffffff;

template <int QT, int K>
__global__ __launch_bounds__(GS_NT) void gather_topk_kernel(
    const float* __restrict__ X, long ldx, int nrows, const int* __restrict__ rows, int count,
    const float* __restrict__ Q, long ldq, int nq, const float* __restrict__ bias, float alpha, int D,
    int rows_per_chunk, int n_chunks, float* __restrict__ ps, int* __restrict__ pi, int vec) {
  extern __shared__ __attribute__((aligned(16))) float s_dyn[];
  const int Dq = (D + 3) & ~3;
  float* s_q = s_dyn;                                   // [QT][Dq] queries of the tile, zero padded
  float* s_sc = s_q + (long)QT * Dq;                    // [QT][GS_SLAB] scores of the slab
  int* s_row = (int*)(s_sc + QT * GS_SLAB);             // [GS_SLAB] graph rows of the slab
  float* s_ts = (float*)(s_row + GS_SLAB);              // [QT][16] running lists
  int* s_ti = (int*)(s_ts + QT * 16);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int chunk = blockIdx.x, q0 = blockIdx.y * QT;
  const int nqt = min(QT, nq - q0);

  for (int e = tid; e < QT * Dq; e += GS_NT) {
    const int q = e / Dq, d = e - q * Dq;
    s_q[e] = (q < nqt && d < D) ? Q[(long)(q0 + q) * ldq + d] : 0.f;
  }
  for (int e = tid; e < QT * 16; e += GS_NT) { s_ts[e] = LZK_NEG_INF; s_ti[e] = GS_NONE; }
  __syncthreads();

  const int c0 = chunk * rows_per_chunk;
  const int c1 = min(count, c0 + rows_per_chunk);
  const int part = lane & 15, grp = lane >> 4;
  for (int s0 = c0; s0 < c1; s0 += GS_SLAB) {
    // ---- scores of the slab's rows: wave w takes slab rows [64 w, 64 w + 64), 4 at a time
    for (int st = 0; st < 16; ++st) {
      const int sr = wave * 64 + st * 4 + grp;  // slab row of this 16-lane group
      const int li = s0 + sr;
      int r = li < c1 ? rows[li] : -1;
      if ((unsigned)r >= (unsigned)nrows) r = -1;  // (never for a plan's list; a bad list must not read out of bounds)
      float acc[QT];
#pragma unroll
      for (int q = 0; q < QT; ++q) acc[q] = 0.f;
      if (r >= 0) {
        const float* xr = X + (long)r * ldx;
        if (vec) {
          const int n4 = D >> 2;
#pragma unroll 4
          for (int d4 = part; d4 < n4; d4 += 16) {
            const float4 xv = *reinterpret_cast<const float4*>(xr + 4 * d4);
#pragma unroll
            for (int q = 0; q < QT; ++q) {
              const float4 qv = *reinterpret_cast<const float4*>(s_q + (long)q * Dq + 4 * d4);
              acc[q] = fmaf(qv.x, xv.x, acc[q]);
              acc[q] = fmaf(qv.y, xv.y, acc[q]);
              acc[q] = fmaf(qv.z, xv.z, acc[q]);
              acc[q] = fmaf(qv.w, xv.w, acc[q]);
            }
          }
        } else {
          for (int d = part; d < D; d += 16) {
            const float xv = xr[d];
#pragma unroll
            for (int q = 0; q < QT; ++q) acc[q] = fmaf(s_q[(long)q * Dq + d], xv, acc[q]);
          }
        }
      }
#pragma unroll
      for (int q = 0; q < QT; ++q) {
        float a = acc[q];
        a += __shfl_xor(a, 8, 64);
        a += __shfl_xor(a, 4, 64);
        a += __shfl_xor(a, 2, 64);
        a += __shfl_xor(a, 1, 64);
        if (part == 0) s_sc[q * GS_SLAB + sr] = r >= 0 ? fmaf(alpha, a, bias[r]) : LZK_NEG_INF;
      }
      if (part == 0) s_row[sr] = r >= 0 ? r : GS_NONE;
    }
    __syncthreads();
    // ---- selection: wave w merges the slab into the lists of queries w, w + 4, ...
    for (int q = wave; q < nqt; q += GS_NT / 64) {
      // the running list, sorted best first, entry j in lane j (j < K)
      float ls = lane < K ? s_ts[q * 16 + lane] : LZK_NEG_INF;
      int lr = lane < K ? s_ti[q * 16 + lane] : GS_NONE;
      float cs[GS_SLAB / 64];
      int cr[GS_SLAB / 64];
#pragma unroll
      for (int j = 0; j < GS_SLAB / 64; ++j) {
        cs[j] = s_sc[q * GS_SLAB + j * 64 + lane];
        cr[j] = s_row[j * 64 + lane];
      }
      for (int round = 0; round < K; ++round) {
        float hs = cs[0]; int hr = cr[0]; int hj = 0;
#pragma unroll
        for (int j = 1; j < GS_SLAB / 64; ++j)
          if (better(cs[j], cr[j], hs, hr)) { hs = cs[j]; hr = cr[j]; hj = j; }
        float bs = hs; int br = hr;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
          const float s2 = __shfl_xor(bs, o, 64);
          const int r2 = __shfl_xor(br, o, 64);
          if (better(s2, r2, bs, br)) { bs = s2; br = r2; }
        }
        const float wsc = __shfl(ls, K - 1, 64);
        const int wr = __shfl(lr, K - 1, 64);
        if (br == GS_NONE || !better(bs, br, wsc, wr)) break;  // (wave-uniform)
        // insert at pos = #entries better than the new one; the tail shifts down a lane
        const int pos = __popcll(__ballot(lane < K && better(ls, lr, bs, br)));
        const float us = __shfl_up(ls, 1, 64);
        const int ur = __shfl_up(lr, 1, 64);
        if (lane == pos) { ls = bs; lr = br; }
        else if (lane > pos && lane < K) { ls = us; lr = ur; }
        if (hr == br && hs == bs) {  // rows are unique in a list: one lane owns the winner
#pragma unroll
          for (int j = 0; j < GS_SLAB / 64; ++j)
            if (j == hj) { cs[j] = LZK_NEG_INF; cr[j] = GS_NONE; }
        }
      }
      if (lane < K) { s_ts[q * 16 + lane] = ls; s_ti[q * 16 + lane] = lr; }
    }
    __syncthreads();
  }
  for (int e = tid; e < nqt * K; e += GS_NT) {
    const int q = e / K, j = e - q * K;
    const float s = s_ts[q * 16 + j];
    const int r = s_ti[q * 16 + j];
    const long o = ((long)(q0 + q) * n_chunks + chunk) * K + j;
    ps[o] = s;
    pi[o] = (r == GS_NONE || s == LZK_NEG_INF) ? -1 : r;
  }
}

size_t gs_lds_bytes(int QT, int D) {
  const int Dq = (D + 3) & ~3;
  return ((size_t)QT * Dq + (size_t)QT * GS_SLAB + GS_SLAB + 2 * (size_t)QT * 16) * 4;
}

template <int QT, int K>
hipError_t gs_launch(const float* X, long ldx, int nrows, const int* rows, int count, const float* Q, long ldq, int nq,
                     const float* bias, float alpha, int D, int rpc, int n_chunks, float* ps, int* pi, int vec,
                     hipStream_t st) {
  const size_t lds = gs_lds_bytes(QT, D);
  (void)hipFuncSetAttribute((const void*)gather_topk_kernel<QT, K>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds);
  dim3 grid(n_chunks, (nq + QT - 1) / QT);
  hipLaunchKernelGGL((gather_topk_kernel<QT, K>), grid, dim3(GS_NT), lds, st, X, ldx, nrows, rows, count, Q, ldq, nq,
                     bias, alpha, D, rpc, n_chunks, ps, pi, vec);
  return hipGetLastError();
}

template <int QT>
hipError_t gs_launch_k(int kslot, const float* X, long ldx, int nrows, const int* rows, int count, const float* Q,
                       long ldq, int nq, const float* bias, float alpha, int D, int rpc, int n_chunks, float* ps,
                       int* pi, int vec, hipStream_t st) {
#define LZK_GS(KK) return gs_launch<QT, KK>(X, ldx, nrows, rows, count, Q, ldq, nq, bias, alpha, D, rpc, n_chunks, ps, pi, vec, st)
  switch (kslot) {
    case 1: LZK_GS(1);
    case 2: LZK_GS(2);
    case 4: LZK_GS(4);
    case 8: LZK_GS(8);
    case 10: LZK_GS(10);
    case 16: LZK_GS(16);
    default: return hipErrorInvalidValue;
  }
#undef LZK_GS
}

}  // namespace

// Workspace ints lzk_tg_filter_plan needs for n rows (the block counts).
LZK_EXPORT long lzk_tg_filter_plan_ws(long n) { return (n + FP_NT - 1) / FP_NT + 1; }

// The predicate over rows [0, n): bias[n], rows[<= rows_cap] ascending,
// *count. ws: lzk_tg_filter_plan_ws(n) ints. cols: the addresses of sal, acc,
// last, ts, shard, kind, sup, stored, type codes, shard bitmap, exclusion
// bitmap (the last three may be null when their test is off).
LZK_EXPORT int lzk_tg_filter_plan(const void* const* cols, LzkFilterBounds b, const float* sqn, long n, float* bias,
                                  int* rows, long rows_cap, int* count, int* ws, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (n < 0 || n >= (1L << 31)) return (int)hipErrorInvalidValue;
  if (n == 0) return (int)hipMemsetAsync(count, 0, sizeof(int), st);
  FilterCols c;
  c.sal = (const float*)cols[0]; c.acc = (const int*)cols[1]; c.last = (const double*)cols[2];
  c.ts = (const double*)cols[3]; c.shard = (const int*)cols[4]; c.kind = (const uint8_t*)cols[5];
  c.sup = (const uint8_t*)cols[6]; c.stored = (const uint8_t*)cols[7]; c.tcode = (const uint8_t*)cols[8];
  c.shard_bits = (const unsigned*)cols[9]; c.exclude_bits = (const unsigned*)cols[10];
  if (((b.flags & FB_TYPES) && !c.tcode) || ((b.flags & FB_SHARDS) && !c.shard_bits && b.n_shard_bits > 0) ||
      ((b.flags & FB_EXCLUDE) && !c.exclude_bits) || (b.l2 && !sqn))
    return (int)hipErrorInvalidValue;
  const int nb = (int)((n + FP_NT - 1) / FP_NT);
  hipLaunchKernelGGL(fp_eval_kernel, dim3(nb), dim3(FP_NT), 0, st, c, b, sqn, n, bias, ws);
  hipLaunchKernelGGL(fp_scan_kernel, dim3(1), dim3(FP_NT), 0, st, ws, nb, count);
  hipLaunchKernelGGL(fp_write_kernel, dim3(nb), dim3(FP_NT), 0, st, c, b, n, (const int*)ws, rows, rows_cap);
  return (int)hipGetLastError();
}

// Chunks of the row list the partial buffers must be sized for: whole
// 256-row slabs, about target_wgs blocks over all query tiles.
// (the query tile: the widest of 8, 4, 1 the batch fills whose LDS image stays within 64 KiB)
static int gather_topk_qtile(int nq, int D) {
  if (nq > 4 && gs_lds_bytes(8, D) <= 64 * 1024) return 8;
  if (nq > 1 && gs_lds_bytes(4, D) <= 64 * 1024) return 4;
  return 1;
}

LZK_EXPORT int lzk_gather_topk_chunks(int count, int nq, int D, int target_wgs) {
  const int qt = gather_topk_qtile(nq, D);
  const int n_qtiles = (nq + qt - 1) / qt;
  int n_chunks = (target_wgs + n_qtiles - 1) / n_qtiles;
  const int max_chunks = (count + GS_SLAB - 1) / GS_SLAB;
  if (n_chunks > max_chunks) n_chunks = max_chunks;
  if (n_chunks < 1) n_chunks = 1;
  const int rpc = ((count + n_chunks - 1) / n_chunks + GS_SLAB - 1) / GS_SLAB * GS_SLAB;
  return rpc > 0 ? (count + rpc - 1) / rpc : 1;
}

// Partial pass over the listed rows: ps/pi are [nq, n_chunks, kslot] with
// n_chunks = lzk_gather_topk_chunks(count, nq, D, target_wgs); pi holds graph
// rows (-1 = empty). X fp32 [nrows, D] with row stride ldx, Q fp32 [nq, D].
LZK_EXPORT int lzk_gather_topk_partial(const float* X, long ldx, int nrows, const int* rows, int count, const float* Q,
                                       long ldq, int nq, const float* bias, float alpha, int D, int kslot,
                                       int n_chunks, float* ps, int* pi, void* stream) {
  if (D <= 0 || nq <= 0 || count <= 0 || nrows <= 0 || n_chunks <= 0 || !bias || !rows) return (int)hipErrorInvalidValue;
  if (gs_lds_bytes(1, D) > 64 * 1024) return (int)hipErrorInvalidValue;  // (D > ~15,000: one query does not fit the LDS tile)
  hipStream_t st = (hipStream_t)stream;
  const int rpc = ((count + n_chunks - 1) / n_chunks + GS_SLAB - 1) / GS_SLAB * GS_SLAB;
  if ((long)rpc * n_chunks < count) return (int)hipErrorInvalidValue;
  const int vec = (D % 4 == 0) && (ldx % 4 == 0) && (((uintptr_t)X & 15) == 0);
  hipError_t rc;
  switch (gather_topk_qtile(nq, D)) {
    case 1: rc = gs_launch_k<1>(kslot, X, ldx, nrows, rows, count, Q, ldq, nq, bias, alpha, D, rpc, n_chunks, ps, pi, vec, st); break;
    case 4: rc = gs_launch_k<4>(kslot, X, ldx, nrows, rows, count, Q, ldq, nq, bias, alpha, D, rpc, n_chunks, ps, pi, vec, st); break;
    default: rc = gs_launch_k<8>(kslot, X, ldx, nrows, rows, count, Q, ldq, nq, bias, alpha, D, rpc, n_chunks, ps, pi, vec, st); break;
  }
  return (int)rc;
}
