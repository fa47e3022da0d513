// Chunk schedule of lzk_ivf_spread_rows (csrc/kernels/ivfmaint.hip): plain
// host C++, no HIP, so the arithmetic -- direct or bounce, the bounds, the
// error returns -- is shared with a CPU program that replays it under a
// sanitizer (tests/native/ivf_spread_plan_test.cpp).
//
// Rows [first, n0) of a column move up by shift(r), non-decreasing in r.
// ``bounds``: shift at the first row of every chunk (first, first +
// chunk_rows, ...) and, last, at row n0 - 1 -- nchunks + 1 values.
#pragma once

struct IvfSpreadChunk {
  long c0, c1;  // source rows [c0, c1)
  long lo, hi;  // every shift of the chunk lies in [lo, hi]
  int direct;   // destinations cannot touch the chunk's own sources
};

inline long ivf_spread_nchunks(long n0, long first, long chunk_rows) {
  return (n0 - first + chunk_rows - 1) / chunk_rows;
}

// 0, or -1 when the bounds are not a valid non-decreasing shift, the top
// destination exceeds cap_rows, or a chunk that overlaps itself does not fit
// the bounce buffer. Nothing is emitted unless everything is valid. ``emit``
// gets the chunks in execution order: DESCENDING rows. ``in_place`` false: the
// source is another buffer, so every chunk is direct. ``stats`` (may be
// null): bytes moved, direct chunks, bounced chunks.
template <class Emit>
inline int ivf_spread_plan(long n0, long first, long chunk_rows, const long* bounds, long cap_rows, long row_bytes,
                           long bounce_bytes, bool in_place, long* stats, Emit&& emit) {
  if (stats) stats[0] = stats[1] = stats[2] = 0;
  if (n0 <= 0 || first >= n0 || row_bytes <= 0) return 0;
  if (chunk_rows <= 0 || first < 0 || bounds == nullptr) return -1;
  const long nch = ivf_spread_nchunks(n0, first, chunk_rows);
  if (bounds[0] < 0) return -1;
  for (long i = 0; i < nch; ++i)
    if (bounds[i + 1] < bounds[i]) return -1;
  if (bounds[nch] > cap_rows - n0) return -1;  // row n0 - 1 lands at n0 - 1 + shift < cap_rows
  for (long i = 0; i < nch; ++i) {
    const long c0 = first + i * chunk_rows;
    const long c1 = c0 + chunk_rows < n0 ? c0 + chunk_rows : n0;
    if (bounds[i + 1] == 0) continue;
    const bool direct = !in_place || bounds[i] >= c1 - c0;
    if (!direct && (c1 - c0) * row_bytes > bounce_bytes) return -1;
  }
  for (long i = nch - 1; i >= 0; --i) {
    IvfSpreadChunk c;
    c.c0 = first + i * chunk_rows;
    c.c1 = c.c0 + chunk_rows < n0 ? c.c0 + chunk_rows : n0;
    c.lo = bounds[i];
    c.hi = bounds[i + 1];
    if (c.hi == 0) continue;  // no row of this chunk (or of any below it) moves
    c.direct = (!in_place || c.lo >= c.c1 - c.c0) ? 1 : 0;
    emit(c);
    if (stats) {
      stats[0] += (c.c1 - c.c0) * row_bytes;
      stats[c.direct ? 1 : 2] += 1;
    }
  }
  return 0;
}
