// Options in the served batch: the bias columns of one multi-tenant round,
// one launch (lazzaro_amd/ops/mt_bias_ops.py holds the contract in full).
//
// A job is one distinct (tenant, filter, boost) combination of the round; the
// kernel writes n_j floats at out + out_off_j for every job j:
//
//   base(r) = job has a filter ? (pass(r) ? (l2 ? 0.0f - sqn[r] : 0.0f) : -inf)
//                              : store_bias[r]
//   out(r)  = job has a boost  ? (kind[r] == NODE ? base(r) + prior(r) : -inf)
//                              : base(r)
//
// `pass` is fp_pass and `prior` is boost_row, both from lzk_rowpred.h, the
// text filter.hip and boost.hip compile: a job's column equals, bit for bit,
// the filter plan's bias or the boosted column of that tenant. segment.hip
// takes out + out_off_j as the bias address of every query of the job.
//
// Grid. 256 threads x 4 rows: a block owns 1,024 rows of one job. blk0[njobs
// + 1] is the exclusive prefix of ceil(n_j / 1024); a block finds its job by
// a binary search of blk0 (a job with n = 0 has no block) and reads the
// descriptor, which is block-uniform, from global memory as plain C++ -- the
// type mask is indexed by a row's code, so the bounds stay in memory and are
// not copied into registers. The 256 fp64 type weights are staged in LDS only
// for a job that has them.
//
// Memory-bound: a boosted, filtered row reads about 40 B and writes 4. The
// base, salience, use-count, clock and u8 columns are read with 16-byte (u8:
// 4-byte) loads and the column is written with one 16-byte store where the
// job's pointers allow it (checked per job here, as boost.hip's launcher
// checks per call; a column that is a view one element into its buffer takes
// the 4-byte path); the predicate reads its columns row by row inside
// fp_pass, whose early exits skip most of them. Rows past n - n % 4 go row by
// row.
#include "lzk_common.h"
#include "lzk_rowpred.h"

// one job (ops/mt_bias_ops.py JOB_DTYPE mirrors this field for field)
struct LzkMtBiasJob {
  const float* sal;
  const int* acc;
  const double* last;
  const double* ts;
  const int* shard;
  const uint8_t* kind;
  const uint8_t* sup;
  const uint8_t* stored;
  const uint8_t* tcode;        // type codes: a type test or type weights (else unused)
  const float* sqn;            // |x|^2 per row: a filter with l2 (else unused)
  const float* store_bias;     // the tenant's store bias column: a job without a filter (else unused)
  long n;                      // rows of the tenant
  long out_off;                // floats into `out`, a multiple of 4
  LzkFilterBounds fb;
  double w_sal, w_freq, w_rec, scale, now, c;
  long shard_off, excl_off, tw_off;  // bytes into `aux` (multiples of 8): shard bitmap, exclusion bitmap,
                                     // 256 fp64 type weights; -1 = none
  int clock;                   // the boost's clock column: 0 last_accessed, 1 timestamp
  int flags;                   // MB_FILTER | MB_BOOST
};

namespace {

constexpr int MB_NT = 256;
constexpr int MB_RPT = 4;                  // rows per thread
constexpr int MB_ROWS = MB_NT * MB_RPT;    // rows per block
enum { MB_FILTER = 1, MB_BOOST = 2 };

__device__ __forceinline__ bool mb_aligned(const void* p, uintptr_t a) {
  return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0;
}

__global__ __launch_bounds__(MB_NT) void mt_bias_kernel(const LzkMtBiasJob* __restrict__ jobs, int njobs,
                                                        const int* __restrict__ blk0,
                                                        const unsigned char* __restrict__ aux,
                                                        float* __restrict__ out) {
  __shared__ double tw_s[256];
  const int b = blockIdx.x;
  int lo = 0, hi = njobs;  // blk0[lo] <= b < blk0[hi]: job lo is not empty and holds block b
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (blk0[mid] <= b) lo = mid; else hi = mid;
  }
  const LzkMtBiasJob& J = jobs[lo];
  const bool hasf = (J.flags & MB_FILTER) != 0, hasb = (J.flags & MB_BOOST) != 0;
  const bool types = hasb && J.tw_off >= 0;
  if (types) {  // (block-uniform)
    tw_s[threadIdx.x] = reinterpret_cast<const double*>(aux + J.tw_off)[threadIdx.x];  // (MB_NT == 256 entries)
    __syncthreads();
  }
  const long n = J.n;
  const long r0 = (long)(b - blk0[lo]) * MB_ROWS + (long)threadIdx.x * MB_RPT;
  if (r0 < 0 || r0 >= n) return;

  FilterCols c;
  c.sal = J.sal; c.acc = J.acc; c.last = J.last; c.ts = J.ts; c.shard = J.shard; c.kind = J.kind;
  c.sup = J.sup; c.stored = J.stored; c.tcode = J.tcode;
  c.shard_bits = J.shard_off >= 0 ? reinterpret_cast<const unsigned*>(aux + J.shard_off) : nullptr;
  c.exclude_bits = J.excl_off >= 0 ? reinterpret_cast<const unsigned*>(aux + J.excl_off) : nullptr;
  const LzkFilterBounds& fb = J.fb;
  const bool l2 = hasf && fb.l2 != 0;
  const BoostArgs a{J.w_sal, J.w_freq, J.w_rec, J.scale, J.now, J.c};
  const double* __restrict__ t = J.clock ? J.ts : J.last;
  const float* __restrict__ sqn = J.sqn;
  const float* __restrict__ sb = J.store_bias;
  float* __restrict__ o = out + J.out_off;

  // every pointer the 16-byte path would read or write (block-uniform)
  bool vec = mb_aligned(o, 16);
  if (l2) vec = vec && mb_aligned(sqn, 16);
  if (!hasf) vec = vec && mb_aligned(sb, 16);
  if (hasb)
    vec = vec && mb_aligned(J.sal, 16) && mb_aligned(J.acc, 16) && mb_aligned(t, 16) && mb_aligned(J.kind, 4) &&
          (!types || mb_aligned(J.tcode, 4));

  if (vec && r0 + MB_RPT <= n) {
    float4 base;
    if (hasf) {
      float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
      if (l2) q = *reinterpret_cast<const float4*>(sqn + r0);
      // (0 - |x|^2, not -|x|^2: +0 for a zero row, as filter.hip)
      base.x = fp_pass(c, fb, r0) ? (l2 ? 0.0f - q.x : 0.0f) : LZK_NEG_INF;
      base.y = fp_pass(c, fb, r0 + 1) ? (l2 ? 0.0f - q.y : 0.0f) : LZK_NEG_INF;
      base.z = fp_pass(c, fb, r0 + 2) ? (l2 ? 0.0f - q.z : 0.0f) : LZK_NEG_INF;
      base.w = fp_pass(c, fb, r0 + 3) ? (l2 ? 0.0f - q.w : 0.0f) : LZK_NEG_INF;
    } else {
      base = *reinterpret_cast<const float4*>(sb + r0);
    }
    float4 v = base;
    if (hasb) {
      const float4 s4 = *reinterpret_cast<const float4*>(J.sal + r0);
      const int4 a4 = *reinterpret_cast<const int4*>(J.acc + r0);
      const double2 t01 = *reinterpret_cast<const double2*>(t + r0);
      const double2 t23 = *reinterpret_cast<const double2*>(t + r0 + 2);
      const unsigned k4 = *reinterpret_cast<const unsigned*>(J.kind + r0);
      unsigned c4 = 0;
      if (types) c4 = *reinterpret_cast<const unsigned*>(J.tcode + r0);
      v.x = boost_row(base.x, s4.x, a4.x, t01.x, k4 & 255u, types ? tw_s[c4 & 255u] : 0.0, a);
      v.y = boost_row(base.y, s4.y, a4.y, t01.y, (k4 >> 8) & 255u, types ? tw_s[(c4 >> 8) & 255u] : 0.0, a);
      v.z = boost_row(base.z, s4.z, a4.z, t23.x, (k4 >> 16) & 255u, types ? tw_s[(c4 >> 16) & 255u] : 0.0, a);
      v.w = boost_row(base.w, s4.w, a4.w, t23.y, k4 >> 24, types ? tw_s[c4 >> 24] : 0.0, a);
    }
    *reinterpret_cast<float4*>(o + r0) = v;
  } else {
    const long r1 = r0 + MB_RPT < n ? r0 + MB_RPT : n;
    for (long r = r0; r < r1; ++r) {
      float base;
      if (hasf) base = fp_pass(c, fb, r) ? (l2 ? 0.0f - sqn[r] : 0.0f) : LZK_NEG_INF;
      else base = sb[r];
      o[r] = hasb ? boost_row(base, J.sal[r], J.acc[r], t[r], J.kind[r], types ? tw_s[J.tcode[r]] : 0.0, a) : base;
    }
  }
}

}  // namespace

// sizeof(LzkMtBiasJob): the packer checks its record layout against it.
LZK_EXPORT int lzk_mt_bias_job_bytes() { return (int)sizeof(LzkMtBiasJob); }

// Rows a block covers (blk0 is the exclusive prefix of ceil(n_j / this)).
LZK_EXPORT int lzk_mt_bias_block_rows() { return MB_ROWS; }

// The bias columns of `njobs` jobs in one launch (see the head of this file).
// `jobs`, `blk0` (njobs + 1 ints, blk0[0] = 0) and `aux` are device memory;
// `nblocks` = blk0[njobs], which the host knows (nothing is read back).
LZK_EXPORT int lzk_mt_bias(const void* jobs, int njobs, const int* blk0, const void* aux, float* out, int nblocks,
                           void* stream) {
  if (njobs < 0 || nblocks < 0) return (int)hipErrorInvalidValue;
  if (njobs == 0 || nblocks == 0) return 0;
  if (!jobs || !blk0 || !out) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(mt_bias_kernel, dim3((unsigned)nblocks), dim3(MB_NT), 0, (hipStream_t)stream,
                     (const LzkMtBiasJob*)jobs, njobs, blk0, (const unsigned char*)aux, out);
  return (int)hipGetLastError();
}
