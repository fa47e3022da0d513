// IVF-PQ index maintenance (IVFPQIndex._finalize): rows leave and enter a
// list-sorted (CSR) index without a re-sort of all of it.
//
//   ivf_mark_count_kernel   keep[r] from the pending flags of the code row and
//                           of its vector row, and the survivors per list
//   (compact.hip)           the flagged rows are squeezed out by the stable
//                           downward compaction lzk_rc_move_rows / _scalars
//   ivf_spread_rows_kernel  the rows of one chunk [c0, c1) up to their new
//                           place, which opens the gaps the appended rows
//                           (sorted by list on their own, O(tail)) drop into
//
// In-place schedule of the spread (lzk_ivf_spread_rows), the mirror image of
// compact.hip's. Row r of list l moves to r + ins[l], ins[l] = the number of
// tail rows whose list is < l. The rows are sorted by list and ins is a prefix
// sum, so the shift is non-decreasing in r: every row moves up or stays, and
// r -> r + shift(r) is strictly increasing -- no two rows share a destination.
// Chunks of chunk_rows rows run in DESCENDING order on one stream, down to the
// first row that moves (the rows before it stay).
//   * A chunk with c0 + shift(c0) >= c1 is written directly: the launch reads
//     rows of [c0, c1) only and every destination is at or above
//     c0 + shift(c0) >= c1 -- no block can overwrite a row another block of
//     the same launch still has to read.
//   * Any other chunk overlaps its own source, so it is copied into a bounce
//     buffer of chunk_rows * row_bytes first and spread from there; the
//     kernel is ordered behind the copy on the stream.
//   * Either way a chunk writes at or above c0 only, and every later chunk
//     reads rows below c0 only, so nothing a later chunk needs is overwritten;
//     what an earlier chunk wrote is not touched either (distinct
//     destinations).
// Once the shift reaches chunk_rows every chunk above is direct.
//
// The key column (list_of) is read by every launch, so it moves last and out
// of place: from a copy (``src``) into the column, all chunks direct.
#include "ivf_spread_plan.h"
#include "lzk_common.h"

LZK_DEBUG_STATE(ivfmaint)

namespace {

constexpr int IM_NT = 256;
constexpr int IM_MAX_BLOCKS = 2048;

// One pass over the code rows. A wave of list-sorted rows almost always holds
// one or two lists: the lanes of the first active lane's list are counted by
// ballot + popcount and leave, then the next run, ... -- one atomic per run.
__global__ void ivf_mark_count_kernel(const int* __restrict__ list_of, const long* __restrict__ pos,
                                      const uint8_t* __restrict__ cdead, const uint8_t* __restrict__ vdead, long nv,
                                      long n, long ncount, int nlist, uint8_t* __restrict__ keep,
                                      unsigned long long* __restrict__ cnt) {
  const int lane = threadIdx.x & (LZK_WAVE - 1);
  const long stride = (long)gridDim.x * blockDim.x;
  for (long b = (long)blockIdx.x * blockDim.x + threadIdx.x - lane; b < n; b += stride) {  // b: wave-uniform
    const long r = b + lane;
    int k = 0, l = -1;
    if (r < n) {
      int dead = cdead ? (cdead[r] != 0) : 0;
      if (vdead) {
        const long p = pos[r];
        LZK_DCHECK(p >= 0 && p < nv);
        if (p >= 0 && p < nv) dead |= (vdead[p] != 0);
      }
      k = !dead;
      keep[r] = (uint8_t)k;
      l = list_of[r];
    }
    bool active = r < ncount && l >= 0 && l < nlist;
    unsigned long long act = __ballot(active);
    while (act) {
      const int leader = __ffsll((long long)act) - 1;
      const int l0 = __shfl(l, leader, LZK_WAVE);
      const bool same = active && l == l0;
      const unsigned long long sm = __ballot(same);
      const unsigned long long km = __ballot(same && k);
      if (lane == leader && km) atomicAdd(&cnt[l0], (unsigned long long)__popcll(km));
      act &= ~sm;
      active = active && !same;
    }
  }
}

// Row r of [c0, c1), read at src + (r - src_row0) * row_bytes, to
// dst + (r + ins[list_of[r]]) * row_bytes, VT bytes per lane, LPR lanes per
// row (a power of two <= 64) as in rc_move_rows_kernel. [lo, hi]: the shifts
// the host validated for this chunk -- a row whose shift falls outside (the
// device arrays disagree with the host's bounds) is not written at all, so a
// store can never land outside the range the launcher checked.
template <typename VT>
__global__ void ivf_spread_rows_kernel(const uint8_t* src, long src_row0, uint8_t* dst, long row_bytes,
                                       const int* __restrict__ list_of, const long* __restrict__ ins, int nlist,
                                       long c0, long c1, long lo, long hi, int lpr) {
  const long nvec = row_bytes / (long)sizeof(VT);
  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long nthr = (long)gridDim.x * blockDim.x;
  const int sub = (int)(tid % lpr);
  for (long r = c0 + tid / lpr; r < c1; r += nthr / lpr) {
    const int l = list_of[r];
    if (l < 0 || l >= nlist) continue;
    const long sh = ins[l];
    if (sh < lo || sh > hi) continue;
    const VT* s = reinterpret_cast<const VT*>(src + (size_t)(r - src_row0) * (size_t)row_bytes);
    VT* d = reinterpret_cast<VT*>(dst + (size_t)(r + sh) * (size_t)row_bytes);
    for (long v = sub; v < nvec; v += lpr) d[v] = s[v];
  }
}

inline unsigned im_grid(long work) {
  long b = (work + IM_NT - 1) / IM_NT;
  return (unsigned)(b < 1 ? 1 : (b > IM_MAX_BLOCKS ? IM_MAX_BLOCKS : b));
}

template <typename VT>
void im_launch_spread(const uint8_t* src, long src_row0, uint8_t* dst, long row_bytes, const int* list_of,
                      const long* ins, int nlist, const IvfSpreadChunk& c, hipStream_t st) {
  const long nvec = row_bytes / (long)sizeof(VT);
  int lpr = 1;
  while (lpr < 64 && lpr < nvec) lpr <<= 1;
  hipLaunchKernelGGL(ivf_spread_rows_kernel<VT>, dim3(im_grid((c.c1 - c.c0) * lpr)), dim3(IM_NT), 0, st, src,
                     src_row0, dst, row_bytes, list_of, ins, nlist, c.c0, c.c1, c.lo, c.hi, lpr);
}

}  // namespace

// keep [n] and cnt [nlist] (+= over the rows below ncount; the caller zeroes it).
LZK_EXPORT int lzk_ivf_mark_count(const int* list_of, const long* pos, const uint8_t* cdead, const uint8_t* vdead,
                                  long nv, long n, long ncount, int nlist, uint8_t* keep, long* cnt, void* stream) {
  if (n <= 0) return 0;
  if (vdead != nullptr && pos == nullptr) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(ivf_mark_count_kernel, dim3(im_grid(n)), dim3(IM_NT), 0, (hipStream_t)stream, list_of, pos,
                     cdead, vdead, nv, n, ncount, nlist, keep, reinterpret_cast<unsigned long long*>(cnt));
  return (int)hipGetLastError();
}

// One column of cap_rows rows. ``src_`` null: in place (through ``bounce`` of
// bounce_bytes where a chunk overlaps itself); else the rows are read from
// that other buffer (row r at src + r * row_bytes). ``list_of`` [n0] sorted,
// ``ins`` [nlist + 1] on the device; ``bounds`` (host): the shift at first,
// first + chunk_rows, ... and at n0 - 1. ``stats`` (host, may be null): bytes
// moved, direct chunks, bounced chunks. Nothing is launched unless the whole
// schedule is valid (ivf_spread_plan.h).
LZK_EXPORT int lzk_ivf_spread_rows(void* base_, const void* src_, long row_bytes, const int* list_of, const long* ins,
                                   int nlist, long n0, long first, long chunk_rows, const long* bounds, long cap_rows,
                                   void* bounce_, long bounce_bytes, long* stats, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  uint8_t* base = static_cast<uint8_t*>(base_);
  const uint8_t* other = static_cast<const uint8_t*>(src_);
  uint8_t* bounce = static_cast<uint8_t*>(bounce_);
  const uintptr_t al = (uintptr_t)base | (uintptr_t)other | (uintptr_t)bounce | (uintptr_t)row_bytes;
  const int vec = (al % 16 == 0) ? 16 : (al % 4 == 0) ? 4 : 1;
  hipError_t err = hipSuccess;
  const int rc = ivf_spread_plan(
      n0, first, chunk_rows, bounds, cap_rows, row_bytes, bounce ? bounce_bytes : 0, other == nullptr, stats,
      [&](const IvfSpreadChunk& c) {
        if (err != hipSuccess) return;
        const uint8_t* src = other ? other : base;
        long row0 = 0;
        if (!c.direct) {
          err = hipMemcpyAsync(bounce, base + (size_t)c.c0 * (size_t)row_bytes,
                               (size_t)(c.c1 - c.c0) * (size_t)row_bytes, hipMemcpyDeviceToDevice, st);
          if (err != hipSuccess) return;
          src = bounce;
          row0 = c.c0;
        }
        if (vec == 16)
          im_launch_spread<uint4>(src, row0, base, row_bytes, list_of, ins, nlist, c, st);
        else if (vec == 4)
          im_launch_spread<uint32_t>(src, row0, base, row_bytes, list_of, ins, nlist, c, st);
        else
          im_launch_spread<uint8_t>(src, row0, base, row_bytes, list_of, ins, nlist, c, st);
      });
  if (rc != 0) return (int)hipErrorInvalidValue;
  if (err != hipSuccess) return (int)err;
  return (int)hipGetLastError();
}
