// The per-row predicate of `where=` and the per-row prior of `boost=`, shared
// by filter.hip (the filter plan), boost.hip (the boosted column) and
// mtbias.hip (the bias columns of a served round): one text, so the three
// cannot drift. ops/filter_ops.py and ops/boost_ops.py hold the contracts.
#pragma once
#include "lzk_common.h"

// by-value scalar bounds of the predicate (ops/filter_ops.py FilterBounds)
struct LzkFilterBounds {
  double since, until, accessed_since;
  float min_sal, max_sal;
  int min_acc;
  int sup_mode;        // -1 both, 0 no super-nodes, 1 only super-nodes
  int flags;           // FB_* bits: which tests apply
  int n_shard_bits;    // shard codes covered by the shard bitmap
  int neg_shard_pass;  // rows with shard code < 0 (the default shard's label) pass the shard test
  int l2;              // bias of a passing row: 0 - sqn (1) or 0 (0)
  unsigned type_mask[8];  // 256 bits over type codes
};

namespace {

enum {
  FB_TYPES = 1, FB_SHARDS = 2, FB_MIN_SAL = 4, FB_MAX_SAL = 8, FB_SINCE = 16, FB_UNTIL = 32,
  FB_ACC_SINCE = 64, FB_MIN_ACC = 128, FB_EXCLUDE = 256
};

struct FilterCols {
  const float* sal;
  const int* acc;
  const double* last;
  const double* ts;
  const int* shard;
  const uint8_t* kind;
  const uint8_t* sup;
  const uint8_t* stored;
  const uint8_t* tcode;          // type codes (FB_TYPES)
  const unsigned* shard_bits;    // bitmap over shard codes (FB_SHARDS)
  const unsigned* exclude_bits;  // bitmap over rows (FB_EXCLUDE)
};

__device__ __forceinline__ bool fp_pass(const FilterCols& c, const LzkFilterBounds& b, long i) {
  if (c.kind[i] != 1 || c.stored[i] != 1) return false;  // memories only: NODE rows in the store
  const int f = b.flags;
  if (b.sup_mode >= 0 && (int)(c.sup[i] != 0) != b.sup_mode) return false;
  if (f & FB_TYPES) {
    const unsigned t = c.tcode[i];
    if (!((b.type_mask[t >> 5] >> (t & 31)) & 1u)) return false;
  }
  if (f & FB_SHARDS) {
    const int s = c.shard[i];
    if (s < 0) {
      if (!b.neg_shard_pass) return false;
    } else if (s >= b.n_shard_bits || !((c.shard_bits[s >> 5] >> (s & 31)) & 1u)) {
      return false;
    }
  }
  if (f & (FB_MIN_SAL | FB_MAX_SAL)) {
    const float s = c.sal[i];
    if ((f & FB_MIN_SAL) && !(s >= b.min_sal)) return false;
    if ((f & FB_MAX_SAL) && !(s <= b.max_sal)) return false;
  }
  if (f & (FB_SINCE | FB_UNTIL)) {
    const double t = c.ts[i];
    if ((f & FB_SINCE) && !(t >= b.since)) return false;
    if ((f & FB_UNTIL) && !(t < b.until)) return false;
  }
  if ((f & FB_ACC_SINCE) && !(c.last[i] >= b.accessed_since)) return false;
  if ((f & FB_MIN_ACC) && !(c.acc[i] >= b.min_acc)) return false;
  if ((f & FB_EXCLUDE) && ((c.exclude_bits[i >> 5] >> (i & 31)) & 1u)) return false;
  return true;
}

struct BoostArgs {
  double w_sal, w_freq, w_rec, scale, now, c;
};

__device__ __forceinline__ float boost_row(float base, float sal, int acc, double t, unsigned kind, double tw,
                                           const BoostArgs& a) {
#pragma clang fp contract(off)
  const double f = fmin(1.0, (double)acc / 10.0);
  const double age = fmax(0.0, a.now - t);
  const double rec = 1.0 / (1.0 + age / a.scale);
  const double B = ((a.w_sal * (double)sal + a.w_freq * f) + a.w_rec * rec) + tw;
  float p = (float)(a.c * B);
  if (!(fabsf(p) <= 3.402823466e+38f)) p = 0.0f;  // NaN or inf (a NaN salience, an fp32 overflow): no prior
  return kind == 1u ? base + p : LZK_NEG_INF;  // (a select, not a branch: the 16-byte loads stay whole)
}

}  // namespace
