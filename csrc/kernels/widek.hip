// Wide-k stages of the certified int8 store search (ops/search.py
// flat_topk_i8_wide, 17 <= k <= 64): a candidate-list select and an exact
// bf16 fallback that keep 64 results per query. The scan kernels are
// threshold scans and do not know k; what bakes in 16 slots is the per-lane
// register lists (TopK<K>) of the select / merge / lane kernels. Here a list
// is staged in LDS as 64-bit keys and reduced by a bitonic tournament of
// 64-entry blocks, one block per wave, so no lane holds more than one key.
// lzk_topk64.h holds the key and the tournament (topk64_rounds). Both kernels
// keep their running best 64 in block 0 of the staging and call it with
// b0 = 1 over each piece staged behind it.
#include "lzk_common.h"
#include "lzk_topk64.h"

namespace {

constexpr int WK = 64;           // results kept per query
constexpr int SEL_LB_MAX = 257;  // LDS blocks of the select: the running best + 16,384 entries (128.5 KB)

// lzk_cand_select's contract with kout <= 64, one block per query: the first
// n = min(cnt & 0x3fffffff, cap) entries of the list (cnt null: n = cap),
// ordered by (score desc, row asc); -inf entries select as (-inf, -1);
// ovf[q] = cnt > cap || (need && cnt < need[q]). A list longer than the LDS
// staging (lb - 1 blocks of 64) is walked in pieces, block 0 carrying the
// running best 64. q_active (optional): a query with q_active[q] == 0 is
// left alone -- os / oi / ovf untouched (the merge of the masked fallback).
__global__ void cand_select_wide_kernel(const int* __restrict__ cnt, const float* __restrict__ cs,
                                        const int* __restrict__ ci, int cap, int lb, int kout, long idx_offset,
                                        float* __restrict__ os, long* __restrict__ oi, int* __restrict__ ovf,
                                        const int* __restrict__ need, const int* __restrict__ q_active) {
  extern __shared__ u64 wkeys[];
  const int q = blockIdx.x;
  if (q_active && !q_active[q]) return;
  const int tid = threadIdx.x, nt = blockDim.x;
  const int c = cnt ? cnt[q] : cap;
  if (tid == 0 && ovf) ovf[q] = (c > cap || (need && c < need[q])) ? 1 : 0;
  const int n = min(c & 0x3fffffff, cap);
  const float* s = cs + (long)q * cap;
  const int* ix = ci + (long)q * cap;
  if (tid < 64) wkeys[tid] = 0;
  int pos = 0;
  do {
    const int take = min(n - pos, (lb - 1) * 64);
    const int padded = (take + 63) & ~63;
    for (int i = tid; i < padded; i += nt) wkeys[64 + i] = i < take ? wide_key(s[pos + i], ix[pos + i]) : 0;
    topk64_rounds(wkeys, 1, 1 + padded / 64);
    pos += take;
  } while (pos < n);
  if (tid < kout) {
    float v;
    int r;
    wide_unkey(wkeys[tid], v, r);
    os[(long)q * kout + tid] = v;
    oi[(long)q * kout + tid] = r < 0 ? -1 : (long)r + idx_offset;
  }
}

// Exact top-64 of alpha <Q[q], X[r]> + bias[r] over the rows of one chunk,
// bf16 rows and queries: block (c, y) serves chunk c for the queries y, y +
// gridDim.y, ... (q_active: only those flagged; an unflagged query costs one
// load) and writes the partial list ps / pi [nq, nch, 64] (descending,
// (-inf, -1) padded; a row whose score is -inf is never listed).
//
// Accumulation order of one score (the tests' bound is counted from this):
// the 8 lanes part = 0 .. 7 of a row split it into 8-element pieces; lane
// part runs ONE fp32 fma chain from 0 over its pieces part, part + 8, ... in
// ascending column order (D / 8 fmas of exact bf16 x bf16 products: at most
// D / 8 roundings on a product), then the xor-shuffle adds o = 1, 2, 4 (3
// roundings), then alpha * acc and + bias (2): at most D / 8 + 5 roundings.
constexpr int WT_ROWS = 960;  // rows per tile: 15 blocks of 64 beside the running best

__global__ __launch_bounds__(256) void flat_topk_wide_kernel(const u16* __restrict__ X, long ldx, int nrows,
                                                             const u16* __restrict__ Qm, long ldq, int nq, int D,
                                                             const float* __restrict__ bias, float alpha,
                                                             int rows_per_chunk, int nch,
                                                             const int* __restrict__ q_active,
                                                             float* __restrict__ ps, int* __restrict__ pi) {
  __shared__ u64 keys[64 + WT_ROWS];
  __shared__ float qf[2048];
  const int tid = threadIdx.x, part = tid & 7, slot = tid >> 3;
  const int c = blockIdx.x;
  const int r0 = c * rows_per_chunk;
  const int r1 = min(nrows, r0 + rows_per_chunk);
  const int pieces = D >> 3;
  for (int q = blockIdx.y; q < nq; q += gridDim.y) {
    if (q_active && !q_active[q]) continue;  // block-uniform
    for (int d = tid; d < D; d += 256) qf[d] = bf16_to_f32(Qm[(long)q * ldq + d]);
    if (tid < 64) keys[tid] = 0;
    __syncthreads();
    for (int t0 = r0; t0 < r1; t0 += WT_ROWS) {
      const int rows = min(WT_ROWS, r1 - t0);
      const int padded = (rows + 63) & ~63;
      for (int i = slot; i < padded; i += 32) {
        const int r = t0 + i;
        const bool in = i < rows;
        float acc = 0.f;
        if (in) {
          const u16* xr = X + (long)r * ldx;
          for (int p = part; p < pieces; p += 8) {
            const u16x8 v = *reinterpret_cast<const u16x8*>(xr + 8 * p);
            const float* qp = qf + 8 * p;
#pragma unroll
            for (int e = 0; e < 8; ++e) acc = fmaf(qp[e], bf16_to_f32(v[e]), acc);
          }
        }
        acc += __shfl_xor(acc, 1, 64);
        acc += __shfl_xor(acc, 2, 64);
        acc += __shfl_xor(acc, 4, 64);
        if (part == 0) {
          u64 key = 0;
          if (in) {
            const float sc = alpha * acc + (bias ? bias[r] : 0.f);
            if (sc == sc && sc != LZK_NEG_INF) key = wide_key(sc, r);
          }
          keys[64 + i] = key;
        }
      }
      topk64_rounds(keys, 1, 1 + padded / 64);
    }
    if (tid < WK) {
      float v;
      int r;
      wide_unkey(keys[tid], v, r);
      const long o = ((long)q * nch + c) * WK + tid;
      ps[o] = v;
      pi[o] = r;
    }
    __syncthreads();
  }
}

int wide_rows_per_chunk(int nrows, int n_chunks) {
  if (n_chunks <= 0) {
    n_chunks = (nrows + 8191) / 8192;
    if (n_chunks > 256) n_chunks = 256;
  }
  if (n_chunks < 1) n_chunks = 1;
  return ((nrows + n_chunks - 1) / n_chunks + 31) / 32 * 32;
}

int launch_select_wide(const int* cnt, const float* cs, const int* ci, int cap, int nq, int kout, long idx_offset,
                       float* os, long* oi, int* ovf, const int* need, const int* q_active, hipStream_t st) {
  if (nq <= 0 || cap <= 0 || kout < 1 || kout > WK || !cs || !ci || !os || !oi) return (int)hipErrorInvalidValue;
  int lb = (cap + 63) / 64 + 1;
  if (lb > SEL_LB_MAX) lb = SEL_LB_MAX;
  const size_t lds = (size_t)lb * 64 * sizeof(u64);
  const int nt = lb <= 33 ? 256 : 1024;
  hipError_t e = hipFuncSetAttribute((const void*)cand_select_wide_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)(SEL_LB_MAX * 64 * sizeof(u64)));
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(cand_select_wide_kernel, dim3((unsigned)nq), dim3(nt), lds, st, cnt, cs, ci, cap, lb, kout,
                     idx_offset, os, oi, ovf, need, q_active);
  return (int)hipGetLastError();
}

int flat_wide(const void* X, long ldx, int nrows, const void* Qm, long ldq, int nq, const float* bias, float alpha,
              int D, int n_chunks, float* ps, int* pi, int k, long idx_offset, float* os, long* oi,
              const int* q_active, hipStream_t st) {
  if (D % 8 != 0 || D <= 0 || D > 2048 || ldx % 8 != 0 || ldx < D || ldq < D || ((uintptr_t)X) % 16 != 0)
    return (int)hipErrorInvalidValue;
  if (nq <= 0 || nrows <= 0 || k < 1 || k > WK || !ps || !pi) return (int)hipErrorInvalidValue;
  const int rpc = wide_rows_per_chunk(nrows, n_chunks);
  const int nch = (nrows + rpc - 1) / rpc;
  if (nq > 0x3fffffff / (nch * WK)) return (int)hipErrorInvalidValue;
  const dim3 grid((unsigned)nch, (unsigned)(nq < 64 ? nq : 64));
  hipLaunchKernelGGL(flat_topk_wide_kernel, grid, dim3(256), 0, st, (const u16*)X, ldx, nrows, (const u16*)Qm, ldq,
                     nq, D, bias, alpha, rpc, nch, q_active, ps, pi);
  const int rc = (int)hipGetLastError();
  if (rc) return rc;
  // the merge: the select over each query's nch * 64 partial entries
  return launch_select_wide(nullptr, ps, pi, nch * WK, nq, k, idx_offset, os, oi, nullptr, nullptr, q_active, st);
}

}  // namespace

// See cand_select_wide_kernel. cnt null: every list holds cap entries.
LZK_EXPORT int lzk_cand_select_wide(const int* cnt, const float* cs, const int* ci, int cap, int nq, int kout,
                                    long idx_offset, float* os, long* oi, int* ovf, const int* need,
                                    const int* q_active, void* stream) {
  return launch_select_wide(cnt, cs, ci, cap, nq, kout, idx_offset, os, oi, ovf, need, q_active,
                            (hipStream_t)stream);
}

// Row chunks lzk_flat_topk_wide uses for a store (n_chunks <= 0: its own
// choice, 8,192 rows per chunk, at most 256 chunks): ps / pi must hold
// nq * chunks * 64 entries.
LZK_EXPORT int lzk_flat_topk_wide_chunks(int nrows, int n_chunks) {
  if (nrows <= 0) return 1;
  const int rpc = wide_rows_per_chunk(nrows, n_chunks);
  return (nrows + rpc - 1) / rpc;
}

// Exact top-k (k <= 64) of alpha <Q16[q], X16[r]> + bias[r] over all rows:
// the partial pass (flat_topk_wide_kernel) + the merge, two launches.
// X16 [nrows, ldx] bf16 (16-B aligned rows, D % 8 == 0, D <= 2048), os / oi
// [nq, k] (rows + idx_offset; (-inf, -1) past the live rows).
LZK_EXPORT int lzk_flat_topk_wide(const void* X, long ldx, int nrows, const void* Qm, long ldq, int nq,
                                  const float* bias, float alpha, int D, int n_chunks, float* ps, int* pi, int k,
                                  long idx_offset, float* os, long* oi, void* stream) {
  return flat_wide(X, ldx, nrows, Qm, ldq, nq, bias, alpha, D, n_chunks, ps, pi, k, idx_offset, os, oi, nullptr,
                   (hipStream_t)stream);
}

// The same for the queries with q_active[q] != 0 only; the others' rows of
// os / oi (and of ps / pi) are left untouched. No host read.
LZK_EXPORT int lzk_flat_topk_wide_masked(const void* X, long ldx, int nrows, const void* Qm, long ldq, int nq,
                                         const float* bias, float alpha, int D, int n_chunks, float* ps, int* pi,
                                         int k, long idx_offset, float* os, long* oi, const int* q_active,
                                         void* stream) {
  if (!q_active) return (int)hipErrorInvalidValue;
  return flat_wide(X, ldx, nrows, Qm, ldq, nq, bias, alpha, D, n_chunks, ps, pi, k, idx_offset, os, oi, q_active,
                   (hipStream_t)stream);
}
