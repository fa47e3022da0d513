// The per-block row table of the selection kernels that gather a candidate set
// in LDS (expand.hip, fuse.hip): an open-addressing hash of HASH slots (a power
// of two; linear probing) keyed by the row, and a dense list of the rows in
// arrival order, capped at MAXN. The callers keep MAXN <= HASH / 2 and bound
// what they insert by MAXN, so the table never fills and a probe always ends.
//
// The LDS arrays belong to the kernel: s_key[HASH] (row of the slot, -1 =
// free; the kernel fills it with -1), s_list[MAXN], and a counter s_cnt set to
// 0, all before the barrier that precedes the first insert. What else a kernel
// keeps per row -- by slot or by list place -- it writes itself from the (h, i)
// an insert reports. The order of the dense list depends on arrival; a kernel
// must return nothing that does.
#pragma once
#include "lzk_common.h"

// Knuth's multiplicative hash, the top log2(HASH) bits
template <int HASH>
__device__ __forceinline__ unsigned lzk_rowset_hash(int row) {
  static_assert(HASH > 1 && (HASH & (HASH - 1)) == 0, "HASH is a power of two");
  return ((unsigned)row * 2654435761u) >> (32 - __builtin_ctz((unsigned)HASH));
}

// The slot of `row`, which joins the table if it is new. The one call that
// inserts a row (whatever the arrival order) appends it to the dense list at
// place i < MAXN and reports on_new(h, i), h its slot, before it returns;
// a list that is full -- the callers' bounds exclude it -- reports nothing.
// Any thread may call it; concurrent inserts of one row agree on the slot.
template <int HASH, int MAXN, class OnNew>
__device__ __forceinline__ int lzk_rowset_insert(int row, int* s_key, int* s_list, int* s_cnt, OnNew on_new) {
  unsigned h = lzk_rowset_hash<HASH>(row);
  for (;;) {
    const int k = s_key[h];
    if (k == row) return (int)h;
    if (k == -1) {
      const int old = atomicCAS(&s_key[h], -1, row);
      if (old == -1) {
        const int i = atomicAdd(s_cnt, 1);
        if (i < MAXN) {
          s_list[i] = row;
          on_new(h, i);
        }
        return (int)h;
      }
      if (old == row) return (int)h;
    }
    h = (h + 1) & (HASH - 1);
  }
}

// What the kernel keeps by slot for `row`, s_val[its slot] (after the barrier
// that ends the inserts); -1: not in the table.
template <int HASH>
__device__ __forceinline__ int lzk_rowset_find(int row, const int* s_key, const int* s_val) {
  unsigned h = lzk_rowset_hash<HASH>(row);
  for (int probes = 0; probes < HASH; ++probes) {
    const int k = s_key[h];
    if (k == row) return s_val[h];
    if (k == -1) return -1;
    h = (h + 1) & (HASH - 1);
  }
  return -1;
}
