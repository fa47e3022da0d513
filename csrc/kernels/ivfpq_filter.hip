// Filtered IVF-PQ lists (IVFPQIndex.filter_rows): the code rows whose id passes
// a filter, compacted in CSR order, so the filtered scans of ivfpq.hip
// (lzk_ivfpq_scan_f / _deep_f / _thresh_f) score passing rows only and keep
// every lane busy -- a per-row bit mask would only save a wave whose 64 rows
// all fail.
//
//   lzk_ivfpq_filter_rows  frows: the passing code rows, ascending; foff[l]:
//                          the number of passing rows below list_off[l], so
//                          list l's passing rows are frows[foff[l] .. foff[l+1])
//                          and foff[nlist] is their count.
//
// The shape of filter.hip's plan build: flag + per-block counts, an exclusive
// scan of the block counts (one block), ordered writes by a wave ballot prefix
// -- no atomic append, the row order is the tie-break of every scan -- then one
// thread per list bound takes a lower bound over frows. No host
// synchronisation; nothing is written at or past frows[max_rows], and when more
// rows pass than max_rows every foff entry stops at max_rows.
#include "lzk_common.h"

namespace {

constexpr int IF_NT = 256;

// code row r passes when its id is inside the allow column and the entry
// passes: kind 0 a uint8 that is non-zero, kind 1 an fp32 bias above -inf
template <int KIND>
__device__ __forceinline__ bool if_pass(const long* __restrict__ pos, const long* __restrict__ vids,
                                        const void* __restrict__ allow, long n_ids, long r) {
  const long id = vids[pos[r]];
  if (id < 0 || id >= n_ids) return false;
  if constexpr (KIND == 0) return ((const uint8_t*)allow)[id] != 0;
  return ((const float*)allow)[id] > LZK_NEG_INF;
}

template <int KIND>
__global__ __launch_bounds__(IF_NT) void if_eval_kernel(const long* __restrict__ pos, const long* __restrict__ vids,
                                                        const void* __restrict__ allow, long n_ids, long n,
                                                        int* __restrict__ bcount) {
  __shared__ int s_w[IF_NT / 64];
  const long i = (long)blockIdx.x * IF_NT + threadIdx.x;
  const bool p = i < n && if_pass<KIND>(pos, vids, allow, n_ids, i);
  const unsigned long long m = __ballot(p);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = __popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) bcount[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// exclusive scan of the block counts in place (one block; thread t owns a
// contiguous span), total -> bcount[nb]
__global__ __launch_bounds__(IF_NT) void if_scan_kernel(int* __restrict__ bcount, int nb) {
  __shared__ int s_sum[IF_NT];
  const int t = threadIdx.x;
  const int per = (nb + IF_NT - 1) / IF_NT;
  const int a = min(nb, t * per), e = min(nb, a + per);
  int s = 0;
  for (int j = a; j < e; ++j) s += bcount[j];
  s_sum[t] = s;
  __syncthreads();
  if (t == 0) {
    int run = 0;
    for (int j = 0; j < IF_NT; ++j) { const int v = s_sum[j]; s_sum[j] = run; run += v; }
    bcount[nb] = run;
  }
  __syncthreads();
  int run = s_sum[t];
  for (int j = a; j < e; ++j) { const int v = bcount[j]; bcount[j] = run; run += v; }
}

template <int KIND>
__global__ __launch_bounds__(IF_NT) void if_write_kernel(const long* __restrict__ pos, const long* __restrict__ vids,
                                                         const void* __restrict__ allow, long n_ids, long n,
                                                         const int* __restrict__ boff, int* __restrict__ frows,
                                                         long max_rows) {
  __shared__ int s_w[IF_NT / 64];
  const long i = (long)blockIdx.x * IF_NT + threadIdx.x;
  const bool p = i < n && if_pass<KIND>(pos, vids, allow, n_ids, i);
  const unsigned long long m = __ballot(p);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) s_w[w] = __popcll(m);
  __syncthreads();
  if (!p) return;
  long off = boff[blockIdx.x];
  for (int j = 0; j < w; ++j) off += s_w[j];
  off += __popcll(m & ((1ull << lane) - 1ull));
  if (off >= 0 && off < max_rows) frows[off] = (int)i;
}

// foff[l] = the number of listed rows below list_off[l] (a lower bound over the
// written part of frows: at most max_rows entries, so an overflow clamps)
__global__ __launch_bounds__(IF_NT) void if_off_kernel(const int* __restrict__ frows, const int* __restrict__ total,
                                                       long max_rows, const long* __restrict__ list_off, int nlist,
                                                       long* __restrict__ foff) {
  const int l = blockIdx.x * IF_NT + threadIdx.x;
  if (l > nlist) return;
  const long cnt = min((long)*total, max_rows);
  const long x = list_off[l];
  long lo = 0, hi = cnt;
  while (lo < hi) {
    const long mid = (lo + hi) >> 1;
    if ((long)frows[mid] < x) lo = mid + 1; else hi = mid;
  }
  foff[l] = lo;
}

}  // namespace

// Workspace ints lzk_ivfpq_filter_rows needs for n_codes rows.
LZK_EXPORT long lzk_ivfpq_filter_rows_ws(long n_codes) { return (n_codes + IF_NT - 1) / IF_NT + 1; }

// pos [n_codes] int64 (vector row of a code row), vids int64 (id of a vector
// row), allow [n_ids] (allow_kind 0: uint8, 1: fp32 bias), list_off [nlist + 1]
// int64 -> frows [max_rows] int32, foff [nlist + 1] int64.
LZK_EXPORT int lzk_ivfpq_filter_rows(const long* pos, const long* vids, long n_codes, const void* allow,
                                     int allow_kind, long n_ids, const long* list_off, int nlist, long max_rows,
                                     int* frows, long* foff, int* ws, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (n_codes < 0 || n_codes >= (1L << 31) || nlist < 0 || max_rows < 0 || n_ids < 0 || !foff || !list_off ||
      (allow_kind != 0 && allow_kind != 1))
    return (int)hipErrorInvalidValue;
  if (n_codes == 0 || max_rows == 0 || n_ids == 0)
    return (int)hipMemsetAsync(foff, 0, (size_t)(nlist + 1) * sizeof(long), st);
  if (!pos || !vids || !allow || !frows || !ws) return (int)hipErrorInvalidValue;
  const int nb = (int)((n_codes + IF_NT - 1) / IF_NT);
  if (allow_kind == 0) {
    hipLaunchKernelGGL(if_eval_kernel<0>, dim3(nb), dim3(IF_NT), 0, st, pos, vids, allow, n_ids, n_codes, ws);
    hipLaunchKernelGGL(if_scan_kernel, dim3(1), dim3(IF_NT), 0, st, ws, nb);
    hipLaunchKernelGGL(if_write_kernel<0>, dim3(nb), dim3(IF_NT), 0, st, pos, vids, allow, n_ids, n_codes,
                       (const int*)ws, frows, max_rows);
  } else {
    hipLaunchKernelGGL(if_eval_kernel<1>, dim3(nb), dim3(IF_NT), 0, st, pos, vids, allow, n_ids, n_codes, ws);
    hipLaunchKernelGGL(if_scan_kernel, dim3(1), dim3(IF_NT), 0, st, ws, nb);
    hipLaunchKernelGGL(if_write_kernel<1>, dim3(nb), dim3(IF_NT), 0, st, pos, vids, allow, n_ids, n_codes,
                       (const int*)ws, frows, max_rows);
  }
  hipLaunchKernelGGL(if_off_kernel, dim3((nlist + 1 + IF_NT - 1) / IF_NT), dim3(IF_NT), 0, st, (const int*)frows,
                     (const int*)(ws + nb), max_rows, list_off, nlist, foff);
  return (int)hipGetLastError();
}
