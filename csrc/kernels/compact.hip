// Row reclamation (TenantGraph.compact): stable in-place compaction of a
// tenant's HBM columns. Evicted / pruned nodes stay behind as GHOST rows; the
// rows that nothing refers to any more are squeezed out and the live rows
// slide down in their order, so every tie-break by row stays what it was.
//
//   rc_mark_*           keep[r] from (kind, stored, dirty), then the edges'
//                       endpoints, then the parents of kept rows
//   (host)              remap = exclusive prefix sum of keep, n + 1 entries
//   rc_move_rows_kernel the kept rows of one chunk [c0, c1) to their new place
//   rc_move_scalars_kernel  the narrow columns, gathered out of place
//   rc_remap_*          edge endpoints and parent values through remap
//
// In-place schedule of the wide columns (lzk_rc_move_rows). remap[r] <= r for
// every row, so a row only ever moves down. Chunks of chunk_rows rows run in
// ascending order on one stream, starting at the first dead row (the rows
// before it do not move).
//   * A chunk with remap[c1] <= c0 is written directly: the launch reads rows
//     of [c0, c1) only and writes rows of [remap[c0], remap[c1]) only, and
//     that range ends at or before c0 -- no block can overwrite a row another
//     block of the same launch still has to read.
//   * Any other chunk overlaps its own source, so it is gathered into a bounce
//     buffer of chunk_rows * row_bytes first and copied down afterwards; the
//     copy is ordered behind the gather on the stream.
//   * Either way a chunk writes below c1 only, and every later chunk reads
//     rows at or above c1 only, so nothing a later chunk needs is overwritten.
// Once chunk_rows rows have been reclaimed every chunk is direct.
#include "lzk_common.h"

LZK_DEBUG_STATE(compact)

namespace {

constexpr int RC_NT = 256;
constexpr int RC_MAX_BLOCKS = 2048;
constexpr int RC_MAX_COLS = 16;

__global__ void rc_mark_kernel(const uint8_t* __restrict__ kind, const uint8_t* __restrict__ stored,
                               const uint8_t* __restrict__ dirty, long n, uint8_t* __restrict__ keep) {
  for (long r = (long)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (long)gridDim.x * blockDim.x)
    keep[r] = (kind[r] == 1 || stored[r] != 0 || dirty[r] != 0) ? 1 : 0;
}

// plain byte stores of the same value: no atomics needed
__global__ void rc_mark_edges_kernel(const int* __restrict__ src, const int* __restrict__ dst, long ne, long n,
                                     uint8_t* __restrict__ keep) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < ne; i += (long)gridDim.x * blockDim.x) {
    const int s = src[i], d = dst[i];
    if (s >= 0 && s < n) keep[s] = 1;
    if (d >= 0 && d < n) keep[d] = 1;
  }
}

// Parents of kept rows are kept, and so are theirs: the thread of a kept row
// walks up while it finds rows not yet marked. Whoever turns a flag from 0 to
// 1 goes on to that row's parent, so the chain is complete whichever thread
// gets there first; a marked row ends the walk, so a parent cycle ends it too.
__global__ void rc_mark_parents_kernel(const int* __restrict__ parent, long n, uint8_t* keep) {
  for (long r = (long)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (long)gridDim.x * blockDim.x) {
    if (!keep[r]) continue;
    int p = parent[r];
    while (p >= 0 && p < n && !keep[p]) {
      keep[p] = 1;
      p = parent[p];
    }
  }
}

// The kept rows of [c0, c1) to dst + (remap[r] - remap[c0]) * row_bytes, VT
// bytes per lane. LPR lanes share a row (a power of two <= 64), so a wave
// takes 64 / LPR whole rows at a time and a dead row costs one flag read.
template <typename VT>
__global__ void rc_move_rows_kernel(const uint8_t* __restrict__ base, long row_bytes, const uint8_t* __restrict__ keep,
                                    const int* __restrict__ remap, long c0, long c1, uint8_t* __restrict__ dst,
                                    int lpr) {
  const long nvec = row_bytes / (long)sizeof(VT);
  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long nthr = (long)gridDim.x * blockDim.x;
  const int sub = (int)(tid % lpr);
  const long d0 = remap[c0];
  for (long r = c0 + tid / lpr; r < c1; r += nthr / lpr) {
    if (!keep[r]) continue;
    const long o = (long)remap[r] - d0;
    LZK_DCHECK(o >= 0 && o <= r - c0);
    const VT* s = reinterpret_cast<const VT*>(base + (size_t)r * (size_t)row_bytes);
    VT* d = reinterpret_cast<VT*>(dst + (size_t)o * (size_t)row_bytes);
    for (long v = sub; v < nvec; v += lpr) d[v] = s[v];
  }
}

struct RcCol {
  const void* src;
  void* dst;
  int size;  // 1, 4 or 8 bytes
  int pad;
};
struct RcCols {
  RcCol c[RC_MAX_COLS];
  int n;
};

// dst_col[remap[r]] = src_col[r] for every kept row, every narrow column in one launch
__global__ void rc_move_scalars_kernel(RcCols cols, const uint8_t* __restrict__ keep, const int* __restrict__ remap,
                                       long n) {
  for (long r = (long)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (long)gridDim.x * blockDim.x) {
    if (!keep[r]) continue;
    const long o = remap[r];
    LZK_DCHECK(o >= 0 && o <= r);
    for (int j = 0; j < cols.n; ++j) {
      const RcCol c = cols.c[j];
      if (c.size == 4)
        static_cast<uint32_t*>(c.dst)[o] = static_cast<const uint32_t*>(c.src)[r];
      else if (c.size == 8)
        static_cast<uint64_t*>(c.dst)[o] = static_cast<const uint64_t*>(c.src)[r];
      else
        static_cast<uint8_t*>(c.dst)[o] = static_cast<const uint8_t*>(c.src)[r];
    }
  }
}

__global__ void rc_remap_edges_kernel(int* __restrict__ src, int* __restrict__ dst, long ne,
                                      const int* __restrict__ remap, long n_old) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < ne; i += (long)gridDim.x * blockDim.x) {
    const int s = src[i], d = dst[i];
    if (s >= 0 && s < n_old) src[i] = remap[s];
    if (d >= 0 && d < n_old) dst[i] = remap[d];
  }
}

__global__ void rc_remap_parent_kernel(int* __restrict__ parent, long n_new, const int* __restrict__ remap,
                                       long n_old) {
  for (long r = (long)blockIdx.x * blockDim.x + threadIdx.x; r < n_new; r += (long)gridDim.x * blockDim.x) {
    const int p = parent[r];
    if (p >= 0 && p < n_old) parent[r] = remap[p];
  }
}

inline unsigned rc_grid(long work) {
  long b = (work + RC_NT - 1) / RC_NT;
  return (unsigned)(b < 1 ? 1 : (b > RC_MAX_BLOCKS ? RC_MAX_BLOCKS : b));
}

template <typename VT>
void rc_launch_move(const uint8_t* base, long row_bytes, const uint8_t* keep, const int* remap, long c0, long c1,
                    uint8_t* dst, hipStream_t st) {
  const long nvec = row_bytes / (long)sizeof(VT);
  int lpr = 1;
  while (lpr < 64 && lpr < nvec) lpr <<= 1;
  hipLaunchKernelGGL(rc_move_rows_kernel<VT>, dim3(rc_grid((c1 - c0) * lpr)), dim3(RC_NT), 0, st, base, row_bytes,
                     keep, remap, c0, c1, dst, lpr);
}

}  // namespace

LZK_EXPORT int lzk_rc_mark(const uint8_t* kind, const uint8_t* stored, const uint8_t* dirty, const int* parent,
                           long n, const int* src, const int* dst, long ne, uint8_t* keep, void* stream) {
  if (n <= 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(rc_mark_kernel, dim3(rc_grid(n)), dim3(RC_NT), 0, st, kind, stored, dirty, n, keep);
  if (ne > 0) hipLaunchKernelGGL(rc_mark_edges_kernel, dim3(rc_grid(ne)), dim3(RC_NT), 0, st, src, dst, ne, n, keep);
  hipLaunchKernelGGL(rc_mark_parents_kernel, dim3(rc_grid(n)), dim3(RC_NT), 0, st, parent, n, keep);
  return (int)hipGetLastError();
}

// One column, in place. ``bounds`` (host): remap at first, first + chunk_rows,
// ..., n -- nchunks + 1 values. ``bounce``: chunk_rows * row_bytes bytes.
// ``stats`` (host, may be null): bytes moved, direct chunks, bounced chunks.
LZK_EXPORT int lzk_rc_move_rows(void* base_, long row_bytes, const uint8_t* keep, const int* remap, long n, long first,
                                long chunk_rows, const int* bounds, void* bounce_, long bounce_bytes, long* stats,
                                void* stream) {
  if (stats) stats[0] = stats[1] = stats[2] = 0;
  if (n <= 0 || first >= n || row_bytes <= 0) return 0;
  if (chunk_rows <= 0 || first < 0) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  uint8_t* base = static_cast<uint8_t*>(base_);
  uint8_t* bounce = static_cast<uint8_t*>(bounce_);
  const uintptr_t al = (uintptr_t)base | (uintptr_t)bounce | (uintptr_t)row_bytes;
  const int vec = (al % 16 == 0) ? 16 : (al % 4 == 0) ? 4 : 1;
  long ci = 0;
  for (long c0 = first; c0 < n; c0 += chunk_rows, ++ci) {
    const long c1 = c0 + chunk_rows < n ? c0 + chunk_rows : n;
    const long d0 = bounds[ci], d1 = bounds[ci + 1];
    const long m = d1 - d0;
    if (m <= 0) continue;  // nothing kept in this chunk
    if (d0 > c0 || m > c1 - c0) return (int)hipErrorInvalidValue;  // remap must not move a row up
    const bool direct = d1 <= c0;
    if (!direct && (bounce == nullptr || m * row_bytes > bounce_bytes)) return (int)hipErrorInvalidValue;
    uint8_t* dst = direct ? base + (size_t)d0 * (size_t)row_bytes : bounce;
    if (vec == 16)
      rc_launch_move<uint4>(base, row_bytes, keep, remap, c0, c1, dst, st);
    else if (vec == 4)
      rc_launch_move<uint32_t>(base, row_bytes, keep, remap, c0, c1, dst, st);
    else
      rc_launch_move<uint8_t>(base, row_bytes, keep, remap, c0, c1, dst, st);
    if (!direct) {
      hipError_t e = hipMemcpyAsync(base + (size_t)d0 * (size_t)row_bytes, bounce, (size_t)m * (size_t)row_bytes,
                                    hipMemcpyDeviceToDevice, st);
      if (e != hipSuccess) return (int)e;
    }
    if (stats) {
      stats[0] += m * row_bytes;
      stats[direct ? 1 : 2] += 1;
    }
  }
  return (int)hipGetLastError();
}

// ``tab`` (host): ncols x (src pointer, dst pointer, element size) as int64 triples
LZK_EXPORT int lzk_rc_move_scalars(const long* tab, int ncols, const uint8_t* keep, const int* remap, long n,
                                   void* stream) {
  if (n <= 0 || ncols <= 0) return 0;
  if (ncols > RC_MAX_COLS) return (int)hipErrorInvalidValue;
  RcCols cols;
  cols.n = ncols;
  for (int j = 0; j < ncols; ++j) {
    const long sz = tab[3 * j + 2];
    if (sz != 1 && sz != 4 && sz != 8) return (int)hipErrorInvalidValue;
    cols.c[j] = RcCol{reinterpret_cast<const void*>(tab[3 * j]), reinterpret_cast<void*>(tab[3 * j + 1]), (int)sz, 0};
  }
  hipLaunchKernelGGL(rc_move_scalars_kernel, dim3(rc_grid(n)), dim3(RC_NT), 0, (hipStream_t)stream, cols, keep, remap,
                     n);
  return (int)hipGetLastError();
}

LZK_EXPORT int lzk_rc_remap(int* src, int* dst, long ne, int* parent, long n_new, const int* remap, long n_old,
                            void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (ne > 0)
    hipLaunchKernelGGL(rc_remap_edges_kernel, dim3(rc_grid(ne)), dim3(RC_NT), 0, st, src, dst, ne, remap, n_old);
  if (n_new > 0 && parent != nullptr)
    hipLaunchKernelGGL(rc_remap_parent_kernel, dim3(rc_grid(n_new)), dim3(RC_NT), 0, st, parent, n_new, remap, n_old);
  return (int)hipGetLastError();
}
