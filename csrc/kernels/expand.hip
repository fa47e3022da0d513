// Associative (graph-expanded) search: the links of a search's nearest rows
// are walked on the device, everything reached is scored, the best `limit`
// come back. One block per query.
//
//   seeds      act_0(s) = max(cos(q, s), 0)
//   hop h      every table entry present at the start of the hop (Jacobi) with
//              sup == 0 takes the first `fanout` arcs u -> v of its visible-arc
//              CSR segment that qualify -- w[e] >= min_w, kind[v] == NODE,
//              bias[v] finite -- and proposes t = act_{h-1}(u) * (decay * min(w[e], 1))
//              (two fp32 roundings); act_h(v) = max(act_{h-1}(v), proposals)
//   result     score(v) = (1 - gamma) cos(q, v) + gamma act_H(v), the `limit`
//              largest, ties to the lower row; via = -1 when act_H is the
//              activation the row started with (its seed activation, or the 0
//              of a row that was reached), else the source row of the largest
//              proposal, ties to the lower source row
//
// A row is 0 before it is reached and every entry expands whatever its
// activation, so the candidate set depends on seeds, CSR, weights and masks
// only, never on a floating-point value. cos is over the fp32 rows and the
// fp32 query, 0 when either norm is 0. Seeds < 0 or >= n are empty and never
// read; a seed listed twice is one entry.
//
// Layout. EXP_NT = 256 threads. The query sits in LDS. The candidate table is
// lzk_rowset.h's: an open-addressing hash of EXP_HASH = 2048 slots (at most
// EXP_MAX_POOL = 1024 keys: the launcher refuses seeds * (1 + fanout)^hops
// above that, so it never fills) keyed by the row; the rows are also appended
// to a dense list in arrival order, which is what the passes iterate. Every
// slot holds two 64-bit words, the current and the next activation:
//   act_bits << 32 | rank(via),   rank(own) = 0xFFFFFFFF, rank(source u) = 0xFFFFFFFE - u
// Activations are >= +0, whose fp32 bits order as unsigned integers, so a
// 64-bit LDS atomic max takes the larger activation, then "own" before any
// source, then the lower source row -- whatever the arrival order. All slots
// start as (0, own): a row inserted during a hop needs no initialisation that
// a concurrent proposal could race with. A hop copies current to next, lets
// one lane per source walk its arcs sequentially (inserting targets,
// max-ing proposals into next), and swaps the two after a barrier. The order
// of the dense list depends on arrival; nothing that is returned does.
//
// Phases: seeds -> seed cosines -> `hops` hop passes -> cos(q, v) of every
// other entry (the bandwidth part: ncand * D * 4 bytes per query through L2)
// -> blend -> rank by counting: an entry's rank is the number of entries that
// beat it under (score, row), and ranks below `limit` are written out.
//
// Summation order: lzk_dot16.h (16 lanes per row, a fixed share of the
// dimensions per lane, one fold order), the layout of mmr.hip. One dot passes
// through at most L(D) = 4 ceil(D / 64) + 4 fp32 roundings, so
// |cos32 - cos64| <= (2 L(D) + 8) 2^-24 as derived there. An activation adds
// 2 roundings per hop to its seed's cosine error (factors <= 1 do not grow
// it); the blend's weights sum to 1, so it passes on the larger of the two
// errors plus its own roundings (1 - gamma, the product, the fma), counted as 6:
//   |score32 - score64| <= (2 L(D) + 8 + 2 hops + 6) 2^-24       (EXPAND_TOL in ops/expand_ops.py)
// Identical rows get identical cosines, so equal activations give equal bits.
#include "lzk_common.h"
#include "lzk_dot16.h"
#include "lzk_rowset.h"

namespace {

constexpr int EXP_NT = 256;
constexpr int EXP_MAX_POOL = 1024;
constexpr int EXP_HASH = 2048;
constexpr int EXP_MAX_SEEDS = 16;
constexpr int EXP_MAX_LIMIT = 64;
constexpr int EXP_MAX_D = 2048;  // the query's LDS share beside the 52 KiB table
constexpr unsigned long long EXP_OWN = 0xFFFFFFFFull;  // (activation 0, own): the word of a row not reached yet

__device__ __forceinline__ unsigned long long exp_pack(float act, unsigned rank) {
  return ((unsigned long long)__float_as_uint(act) << 32) | rank;
}

// the slot of `row`, inserted if it is new (appended to the dense list then, its slot beside it)
__device__ __forceinline__ int exp_insert(int row, int* s_key, int* s_list, int* s_slot, int* s_cnt) {
  return lzk_rowset_insert<EXP_HASH, EXP_MAX_POOL>(row, s_key, s_list, s_cnt,  // (the launcher bounds the pool)
                                                   [&](unsigned h, int i) { s_slot[i] = (int)h; });
}

__global__ __launch_bounds__(EXP_NT) void expand_select_kernel(
    const float* __restrict__ X, long ldx, int n, const float* __restrict__ Q, long ldq, int D,
    const long* __restrict__ seeds, int S, const long* __restrict__ off, const int* __restrict__ adj,
    const int* __restrict__ eid, long na, const float* __restrict__ w, long ne,
    const unsigned char* __restrict__ kind, const unsigned char* __restrict__ sup, const float* __restrict__ bias,
    int hops, int fanout, float min_w, float decay, float gamma, int limit, long* __restrict__ orow,
    float* __restrict__ oscore, long* __restrict__ ovia, int* __restrict__ ncand, int vec) {
  extern __shared__ __attribute__((aligned(16))) float s_q[];  // [Dq] the query, zero padded
  __shared__ unsigned long long s_a[EXP_HASH];  // activation words, by hash slot
  __shared__ unsigned long long s_b[EXP_HASH];
  __shared__ int s_key[EXP_HASH];               // row of the slot, -1 = free
  __shared__ int s_list[EXP_MAX_POOL];          // rows in arrival order
  __shared__ int s_slot[EXP_MAX_POOL];          // their hash slots
  __shared__ float s_cos[EXP_MAX_POOL];         // cos(q, row), then the blended score
  __shared__ int s_cnt;
  const int Dq = (D + 3) & ~3;
  const int tid = threadIdx.x, part = tid & 15, grp = tid >> 4;
  const long m = blockIdx.x;

  for (int d = tid; d < Dq; d += EXP_NT) s_q[d] = d < D ? Q[m * ldq + d] : 0.f;
  for (int h = tid; h < EXP_HASH; h += EXP_NT) {
    s_key[h] = -1;
    s_a[h] = EXP_OWN;
    s_b[h] = EXP_OWN;
  }
  if (tid == 0) s_cnt = 0;
  __syncthreads();

  // ---- seeds
  if (tid < S) {
    const long r = seeds[m * S + tid];
    if (r >= 0 && r < n) exp_insert((int)r, s_key, s_list, s_slot, &s_cnt);
  }
  __syncthreads();
  const int nseed = min(s_cnt, EXP_MAX_POOL);

  // ---- |q|: every group sums the same shares in the same order
  const float qn = sqrtf(lzk_fold16(lzk_sq16_part(s_q, D, vec, part)));

  // ---- seed cosines and activations (nseed <= 16: one row per group)
  {
    const int r = grp < nseed ? s_list[grp] : -1;
    float dot = 0.f, xx = 0.f;
    if (r >= 0) lzk_dot16_part(s_q, X + (long)r * ldx, D, vec, part, dot, xx);
    dot = lzk_fold16(dot);
    xx = lzk_fold16(xx);
    if (part == 0 && r >= 0) {
      const float c = lzk_cos(dot, qn, sqrtf(xx));
      s_cos[grp] = c;
      s_a[s_slot[grp]] = exp_pack(c > 0.f ? c : 0.f, 0xFFFFFFFFu);  // (never -0: its bits would order above every value)
    }
  }

  // ---- hops
  unsigned long long* cur = s_a;
  unsigned long long* nxt = s_b;
  for (int hop = 0; hop < hops; ++hop) {
    __syncthreads();
    const int nsrc = min(s_cnt, EXP_MAX_POOL);
    for (int h = tid; h < EXP_HASH; h += EXP_NT) nxt[h] = cur[h];
    __syncthreads();
    for (int i = tid; i < nsrc; i += EXP_NT) {
      const int u = s_list[i];
      if (sup[u]) continue;  // super-nodes live outside the shards: no neighbours
      const float au = __uint_as_float((unsigned)(cur[s_slot[i]] >> 32));
      long p = off[u], pe = off[u + 1];
      if (p < 0) p = 0;
      if (pe > na) pe = na;
      int taken = 0;
      for (; p < pe && taken < fanout; ++p) {
        const int v = adj[p];
        const int e = eid[p];
        if (v < 0 || v >= n || e < 0 || e >= ne) continue;
        const float we = w[e];
        if (!(we >= min_w) || kind[v] != 1) continue;
        const float b = bias[v];
        if (!(fabsf(b) < __builtin_huge_valf())) continue;  // (not finite: not in the store, or filtered out)
        ++taken;
        const float f = decay * fminf(we, 1.f);
        const float t = au * f;
        const int slot = exp_insert(v, s_key, s_list, s_slot, &s_cnt);
        atomicMax(&nxt[slot], exp_pack(t, 0xFFFFFFFEu - (unsigned)u));
      }
    }
    unsigned long long* tmp = cur;
    cur = nxt;
    nxt = tmp;
  }
  __syncthreads();
  const int cnt = min(s_cnt, EXP_MAX_POOL);

  // ---- cos(q, v) of the entries the hops added
  for (int i0 = nseed; i0 < cnt; i0 += EXP_NT / 16) {  // (block-uniform trip count: the folds run with whole waves)
    const int i = i0 + grp;
    const int r = i < cnt ? s_list[i] : -1;
    float dot = 0.f, xx = 0.f;
    if (r >= 0) lzk_dot16_part(s_q, X + (long)r * ldx, D, vec, part, dot, xx);
    dot = lzk_fold16(dot);
    xx = lzk_fold16(xx);
    if (part == 0 && r >= 0) s_cos[i] = lzk_cos(dot, qn, sqrtf(xx));
  }
  __syncthreads();

  // ---- blend
  const float w1 = 1.f - gamma;
  for (int i = tid; i < cnt; i += EXP_NT) {
    const float act = __uint_as_float((unsigned)(cur[s_slot[i]] >> 32));
    s_cos[i] = fmaf(gamma, act, w1 * s_cos[i]);
  }
  __syncthreads();

  // ---- rank by counting (rows are distinct, so ranks are)
  for (int i = tid; i < cnt; i += EXP_NT) {
    const float si = s_cos[i];
    const int ri = s_list[i];
    int rank = 0;
    for (int j = 0; j < cnt; ++j) rank += better(s_cos[j], s_list[j], si, ri) ? 1 : 0;
    if (rank < limit) {
      const unsigned lo = (unsigned)cur[s_slot[i]];
      orow[m * limit + rank] = ri;
      oscore[m * limit + rank] = si;
      ovia[m * limit + rank] = lo == 0xFFFFFFFFu ? -1L : (long)(0xFFFFFFFEu - lo);
    }
  }
  for (int j = cnt + tid; j < limit; j += EXP_NT) {
    orow[m * limit + j] = -1;
    oscore[m * limit + j] = LZK_NEG_INF;
    ovia[m * limit + j] = -1;
  }
  if (tid == 0) ncand[m] = cnt;
}

}  // namespace

// Graph-expanded selection for M queries. X fp32 [n, D] with row stride ldx; Q
// fp32 [M, D] with row stride ldq; seeds int64 [M, S] graph rows (< 0 or >= n:
// empty), S <= 16; (off int64 [n + 1], adj int32 [na], eid int32 [na]) the
// visible-arc CSR, w fp32 [ne] the edge weights, kind / sup uint8 [n], bias
// fp32 [n] (not finite: never a target). 1 <= hops <= 3, 1 <= fanout <= 16,
// S (1 + fanout)^hops <= 1024, min_w >= 0, 0 < decay <= 1, 0 <= gamma <= 1,
// 1 <= limit <= 64. rows int64, scores fp32, via int64 [M, limit] (padding
// -1, -inf, -1), ncand int32 [M] the candidate count.
LZK_EXPORT int lzk_expand_select(const float* X, long ldx, long n, const float* Q, long ldq, int M, int D,
                                 const long* seeds, int S, const long* off, const int* adj, const int* eid, long na,
                                 const float* w, long ne, const unsigned char* kind, const unsigned char* sup,
                                 const float* bias, int hops, int fanout, float min_w, float decay, float gamma,
                                 int limit, long* rows, float* scores, long* via, int* ncand, void* stream) {
  if (D <= 0 || D > EXP_MAX_D || S < 1 || S > EXP_MAX_SEEDS || M < 0 || n < 0 || n >= (1L << 31) - 1 || ldx < D ||
      ldq < D || na < 0 || ne < 0)
    return (int)hipErrorInvalidValue;
  if (hops < 1 || hops > 3 || fanout < 1 || fanout > 16 || limit < 1 || limit > EXP_MAX_LIMIT)
    return (int)hipErrorInvalidValue;
  long pool = S;
  for (int h = 0; h < hops; ++h) pool *= 1 + fanout;
  if (pool > EXP_MAX_POOL) return (int)hipErrorInvalidValue;
  if (!(min_w >= 0.f) || !(decay > 0.f && decay <= 1.f) || !(gamma >= 0.f && gamma <= 1.f))
    return (int)hipErrorInvalidValue;
  if (M == 0) return 0;
  if (!Q || !seeds || !rows || !scores || !via || !ncand) return (int)hipErrorInvalidValue;
  if (n > 0 && (!X || !off || !kind || !sup || !bias)) return (int)hipErrorInvalidValue;
  if (na > 0 && (!adj || !eid || !w)) return (int)hipErrorInvalidValue;
  const int vec = (D % 4 == 0) && (ldx % 4 == 0) && (((uintptr_t)X & 15) == 0);
  const size_t lds = (size_t)((D + 3) & ~3) * sizeof(float);
  hipLaunchKernelGGL(expand_select_kernel, dim3(M), dim3(EXP_NT), lds, (hipStream_t)stream, X, ldx, (int)n, Q, ldq, D,
                     seeds, S, off, adj, eid, na, w, ne, kind, sup, bias, hops, fanout, min_w, decay, gamma, limit,
                     rows, scores, via, ncand, vec);
  return (int)hipGetLastError();
}
