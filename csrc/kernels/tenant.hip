// Tenant-graph maintenance kernels: the device engine under MemorySystem
// (lazzaro_amd/engine/tenant_graph.py).
//
// One tenant's memory graph lives in HBM as structure-of-arrays:
//   nodes  sal f32 | acc i32 | last f64 | kind u8 (0 free, 1 node, 2 ghost =
//          id still referenced by an edge) | sup u8 (super-node) | shard i32 |
//          dirty u8 (changed since the last persistence commit)
//   edges  src/dst i32 | w f32 | co i32 | lu f64 | meta i32 = shard | type<<24
//          (the shard the reference stores the edge in: MemoryShard.edges)
//
// These kernels replace the per-object Python loops of the reference:
//   decay + prune      memory_shard.py:64-84 via memory_system.py:624-630, :991
//   node removal       memory_system.py:558-569 (evict: node + its shard's edges)
//   neighbour boost    memory_system.py:242-260 (visible arcs, CSR)
//   retrieval touch    buffer_graph.py:79-85
//   importance         memory_system.py:541-549
#include "lzk_common.h"

LZK_DEBUG_STATE(tenant)

namespace {

constexpr int NTB = 256;
constexpr float SAL_FLOOR = 0.2f;

__device__ __forceinline__ int block_ballot_count(int f, int* wsum) {
  unsigned long long bal = __ballot(f);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = __popcll(bal);
  __syncthreads();
  int s = 0;
#pragma unroll
  for (int i = 0; i < NTB / 64; ++i) s += wsum[i];
  return s;
}

// Salience decay towards the floor, rounded op by op exactly like the CPU
// path (an fma contraction would differ in the last ulp).
__device__ __forceinline__ float decay_sal(float s, float keep) {
#pragma clang fp contract(off)
  return s > SAL_FLOOR ? SAL_FLOOR + (s - SAL_FLOOR) * keep : SAL_FLOOR;
}

// Salience bump min(1, s + delta) in double precision, then stored as fp32:
// the reference adds Python floats (memory_system.py:242-260,
// buffer_graph.py:79-85), so this rounds exactly once like the CPU path.
__device__ __forceinline__ float bump_sal(float s, double delta) { return (float)fmin(1.0, (double)s + delta); }

// Edge pass: `steps` rounds of w *= keep (keep == 1 -> no decay), each
// rounded to fp32 like one end_conversation (a batch of B conversations is B
// rounds here, not one multiply by keep^B, so a weight at the prune
// threshold lands exactly where B sequential calls put it); flag survivors
// w >= thr (flag == nullptr -> no prune; weights only fall, so a survivor
// of the last round survived every round). Node pass (same launch,
// grid-stride): the salience of shard nodes (kind 1, not super) decays
// towards the floor, `steps` rounds.
__global__ __launch_bounds__(NTB) void tg_decay_kernel(float* __restrict__ w, long ne, float keep, float thr,
                                                       unsigned char* __restrict__ flag, int* __restrict__ block_cnt,
                                                       float* __restrict__ sal, const unsigned char* __restrict__ kind,
                                                       const unsigned char* __restrict__ sup, long nn, int do_nodes,
                                                       int steps) {
  __shared__ int wsum[NTB / 64];
  const long e = (long)blockIdx.x * NTB + threadIdx.x;
  int f = 0;
  if (e < ne) {
    float v = w[e];
    if (keep != 1.f) {
      for (int t = 0; t < steps; ++t) v *= keep;
      w[e] = v;
    }
    f = v >= thr;
    if (flag) flag[e] = (unsigned char)f;
  }
  if (flag) {
    const int s = block_ballot_count(f, wsum);
    if (threadIdx.x == 0) block_cnt[blockIdx.x] = s;
  }
  if (do_nodes) {
    for (long i = (long)blockIdx.x * NTB + threadIdx.x; i < nn; i += (long)gridDim.x * NTB) {
      if (kind[i] != 1 || sup[i]) continue;
      float s = sal[i];
      for (int t = 0; t < steps; ++t) s = decay_sal(s, keep);
      sal[i] = s;
    }
  }
}

// Node-only salience decay (when the edge grid is too small to stream nodes).
__global__ __launch_bounds__(NTB) void tg_node_decay_kernel(float* __restrict__ sal, const unsigned char* __restrict__ kind,
                                                            const unsigned char* __restrict__ sup, long nn, float keep,
                                                            int steps) {
  for (long i = (long)blockIdx.x * NTB + threadIdx.x; i < nn; i += (long)gridDim.x * NTB) {
    if (kind[i] != 1 || sup[i]) continue;
    float s = sal[i];
    for (int t = 0; t < steps; ++t) s = decay_sal(s, keep);
    sal[i] = s;
  }
}

// Node removal: an edge is dropped when an endpoint is being removed AND the
// edge lives in that endpoint's shard (the reference deletes only the removed
// node's shard's incident edges; edges other shards store survive, dangling).
// The removed rows come as a bitmap (`rmb`, bit r of word r >> 5: 1.25 MB
// at 10M rows, L2-resident, where a byte array costs a random HBM line per
// endpoint). `prev` (optional) is an earlier keep flag over the first `nprev` edges --
// the deferred prune of a consolidation segment (tg_decay_kernel run at the
// segment's start, the segment's links appended after it) -- so one
// compaction drops both; `rm` == nullptr: no removals, prev flags only.
__global__ __launch_bounds__(NTB) void tg_flag_remove_kernel(const int* __restrict__ src, const int* __restrict__ dst,
                                                             const int* __restrict__ meta, long ne,
                                                             const unsigned* __restrict__ rmb,
                                                             const int* __restrict__ shard,
                                                             const unsigned char* __restrict__ prev, long nprev,
                                                             unsigned char* __restrict__ flag,
                                                             int* __restrict__ block_cnt, int* __restrict__ npruned) {
  __shared__ int wsum[NTB / 64];
  __shared__ int wz[NTB / 64];
  const long e = (long)blockIdx.x * NTB + threadIdx.x;
  if (npruned) {  // edges the decay flagged (prev == 0): the segment's prune count
    const unsigned long long zb = __ballot(prev != nullptr && e < nprev && prev[e] == 0);
    if ((threadIdx.x & 63) == 0) wz[threadIdx.x >> 6] = __popcll(zb);
    __syncthreads();
    if (threadIdx.x == 0) {
      int z = 0;
      for (int i = 0; i < NTB / 64; ++i) z += wz[i];
      if (z) atomicAdd(npruned, z);
    }
  }
  int f = 0;
  if (e < ne) {
    f = (prev == nullptr || e >= nprev) ? 1 : (int)prev[e];
    if (f && rmb) {
      const int s = src[e], d = dst[e];
      LZK_DCHECK(s >= 0 && d >= 0);
      const bool rs = (rmb[s >> 5] >> (s & 31)) & 1u, rd = (rmb[d >> 5] >> (d & 31)) & 1u;
      if (rs || rd) {
        const int es = meta[e] & 0xFFFFFF;
        f = !((rs && shard[s] == es) || (rd && shard[d] == es));
      }
    }
    flag[e] = (unsigned char)f;
  }
  const int s = block_ballot_count(f, wsum);
  if (threadIdx.x == 0) block_cnt[blockIdx.x] = s;
}

// u8 flags -> bitmap: one thread per 32-row word.
__global__ __launch_bounds__(NTB) void pack_bits_kernel(const unsigned char* __restrict__ f, long n,
                                                        unsigned* __restrict__ bits) {
  const long wi = (long)blockIdx.x * NTB + threadIdx.x;
  const long r0 = wi * 32;
  if (r0 >= n) return;
  unsigned b = 0;
  if (r0 + 32 <= n) {
    const uint4* p = reinterpret_cast<const uint4*>(f + r0);
    const uint4 q0 = p[0], q1 = p[1];
    const unsigned w[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
      for (int k = 0; k < 4; ++k) b |= (((w[j] >> (8 * k)) & 0xFFu) != 0u ? 1u : 0u) << (4 * j + k);
  } else {
    for (long r = r0; r < n; ++r) b |= (f[r] != 0 ? 1u : 0u) << (r - r0);
  }
  bits[wi] = b;
}

// Stable scatter of flagged edges (block offsets from lzk_scan_blocks).
__global__ __launch_bounds__(NTB) void tg_compact_kernel(const unsigned char* __restrict__ flag,
                                                         const int* __restrict__ block_off, long ne,
                                                         const int* __restrict__ src, const int* __restrict__ dst,
                                                         const float* __restrict__ w, const int* __restrict__ co,
                                                         const double* __restrict__ lu, const int* __restrict__ meta,
                                                         int* __restrict__ osrc, int* __restrict__ odst,
                                                         float* __restrict__ ow, int* __restrict__ oco,
                                                         double* __restrict__ olu, int* __restrict__ ometa,
                                                         int* __restrict__ dsrc, int* __restrict__ ddst,
                                                         int* __restrict__ dmeta) {
  __shared__ int wpre[NTB / 64];
  const long e = (long)blockIdx.x * NTB + threadIdx.x;
  const int f = (e < ne) ? flag[e] : 0;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  unsigned long long bal = __ballot(f);
  const int before = __popcll(bal & ((1ull << lane) - 1ull));
  if (lane == 0) wpre[wv] = __popcll(bal);
  __syncthreads();
  int off = block_off[blockIdx.x];
  for (int i = 0; i < wv; ++i) off += wpre[i];
  if (f) {
    const int o = off + before;
    osrc[o] = src[e];
    odst[o] = dst[e];
    ow[o] = w[e];
    oco[o] = co[e];
    olu[o] = lu[e];
    ometa[o] = meta[e];
  } else if (dsrc && e < ne) {  // the dropped edges in order: index e - (kept before e)
    const long o = e - (off + before);
    dsrc[o] = src[e];
    ddst[o] = dst[e];
    dmeta[o] = meta[e];
  }
}

// Neighbour boost over the visible-arc CSR (arc a->b exists when the edge is
// stored in a's shard, the reference's MemoryShard.get_neighbors visibility).
// One wave per seed; a neighbour with w >= min_w that is a live node and not
// a seed gets last = now, sal = min(1, sal + delta) once per call: the stamp
// word holds the call's epoch, so no per-call clear of an N-sized array.
__global__ __launch_bounds__(64) void tg_boost_kernel(const long* __restrict__ off, const int* __restrict__ adj,
                                                      const int* __restrict__ eid, const float* __restrict__ w,
                                                      const int* __restrict__ seeds, int nseeds,
                                                      const unsigned char* __restrict__ kind,
                                                      const unsigned char* __restrict__ sup, float min_w, double now,
                                                      double delta, float* __restrict__ sal, double* __restrict__ last,
                                                      unsigned char* __restrict__ dirty, int* __restrict__ stamp,
                                                      int epoch, int* __restrict__ nboost) {
  const int s = seeds[blockIdx.x];
  if (s < 0 || sup[s]) return;  // super-nodes live outside the shards: no neighbours
  for (long p = off[s] + threadIdx.x; p < off[s + 1]; p += 64) {
    const int nb = adj[p];
    LZK_DCHECK(nb >= 0);
    if (w[eid[p]] < min_w || kind[nb] != 1) continue;
    bool is_seed = false;
    for (int j = 0; j < nseeds; ++j) is_seed |= (seeds[j] == nb);
    if (is_seed) continue;
    if (atomicExch(&stamp[nb], epoch) != epoch) {
      sal[nb] = bump_sal(sal[nb], delta);
      last[nb] = now;
      dirty[nb] = 1;
      atomicAdd(nboost, 1);
    }
  }
}

// Retrieval access update (BufferGraph.update_access) for a few rows.
__global__ __launch_bounds__(64) void tg_touch_kernel(const long* __restrict__ rows, int n, int* __restrict__ acc,
                                                      double* __restrict__ last, float* __restrict__ sal,
                                                      unsigned char* __restrict__ dirty, double now, double delta) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const long r = rows[i];
  LZK_DCHECK(r >= 0);
  acc[r] += 1;
  last[r] = now;
  sal[r] = bump_sal(sal[r], delta);
  dirty[r] = 1;
}

// Eviction importance in double precision (the reference scores in Python
// floats; an fp32 score would merge near-ties and change the victim order).
// Non-candidates (not a live shard node, or a super-node) get +inf.
__global__ __launch_bounds__(NTB) void tg_importance_kernel(const float* __restrict__ sal, const int* __restrict__ acc,
                                                            const double* __restrict__ last,
                                                            const unsigned char* __restrict__ kind,
                                                            const unsigned char* __restrict__ sup, long n, double now,
                                                            double* __restrict__ out) {
#pragma clang fp contract(off)
  const long i = (long)blockIdx.x * NTB + threadIdx.x;
  if (i >= n) return;
  if (kind[i] != 1 || sup[i]) {
    out[i] = __builtin_huge_val();
    return;
  }
  const double days = (now - last[i]) / 86400.0;
  out[i] = (double)sal[i] * 0.5 + fmin(1.0, (double)acc[i] / 10.0) * 0.3 + (1.0 / (1.0 + days)) * 0.2;
}

// Exactness check of a batched eviction plan (MemorySystem.consolidate_batch,
// core/batch_plan.py): the planner picked every eviction's victims from a
// pool of rows; a row OUTSIDE the pool that nothing touched must not rank
// before the pool's victims at any eviction. Event e happened after
// ev_steps[e] decays (ascending) and its last victim had the key
// (ev_imp, ev_code, ev_row); each thread walks one row through the events,
// decaying its salience exactly like tg_decay_kernel and scoring it exactly
// like tg_importance_kernel, and flags a row whose key is smaller.
__global__ __launch_bounds__(NTB) void tg_evict_verify_kernel(const float* __restrict__ sal, const int* __restrict__ acc,
                                                              const double* __restrict__ last,
                                                              const unsigned char* __restrict__ kind,
                                                              const unsigned char* __restrict__ sup,
                                                              const int* __restrict__ shard,
                                                              const unsigned char* __restrict__ pool, long n,
                                                              double now, float keep, int ne,
                                                              const int* __restrict__ ev_steps,
                                                              const double* __restrict__ ev_imp,
                                                              const int* __restrict__ ev_code,
                                                              const long* __restrict__ ev_row, int* __restrict__ bad,
                                                              const long* __restrict__ rowkey, double vmax,
                                                              int st_last, double kt, int max_code, long max_key) {
#pragma clang fp contract(off)
  const long i = (long)blockIdx.x * NTB + threadIdx.x;
  if (i >= n || kind[i] != 1 || sup[i] || pool[i]) return;
  const long key = rowkey ? rowkey[i] : i;  // a row-sharded tenant ranks rows by global number
  float s = sal[i];
  const double a = fmin(1.0, (double)acc[i] / 10.0) * 0.3;
  const double d = (1.0 / (1.0 + (now - last[i]) / 86400.0)) * 0.2;
  const int code = shard[i];
  // Shortcuts (the importance of a row at or above the floor never rises:
  // each fp32 decay step lowers s or keeps it), with vmax = the largest event
  // importance and (max_code, max_key) the largest event key:
  //  1. a closed-form lower bound of the row's importance after the last
  //     event's st_last decays -- F + (s - F) keep^st_last minus 4 ulps(1) per
  //     step of fp32 rounding -- above vmax (+1e-9): no event can rank it first;
  //  2. the exact sequential importance after st_last decays >= vmax, ties
  //     only with a row key above every event's: the same.
  // A row below the floor (s < F) is lifted to F by its first decay step and
  // stays there, so its lowest importance is the current one (s * 0.5 + a +
  // d, the loop's own formula): above vmax, no event can rank it first.
  // Everything else walks the events exactly as before.
  if (s < SAL_FLOOR) {
    if ((double)s * 0.5 + a + d > vmax + 1e-9) return;
  } else {
    const double F = (double)SAL_FLOOR;
    double lb = F + ((double)s - F) * kt - 4.0 * (double)st_last * 5.9604644775390625e-08;
    if (lb < F) lb = F;
    if (lb * 0.5 + a + d > vmax + 1e-9) return;
    float sf = s;
    for (int u = 0; u < st_last; ++u) sf = decay_sal(sf, keep);
    const double fin = (double)sf * 0.5 + a + d;
    if (fin > vmax || (fin == vmax && (code > max_code || (code == max_code && key > max_key)))) return;
  }
  int t = 0;
  for (int e = 0; e < ne; ++e) {
    const int st = ev_steps[e];
    for (; t < st; ++t) s = decay_sal(s, keep);
    const double imp = (double)s * 0.5 + a + d;
    const double vi = ev_imp[e];
    if (imp < vi || (imp == vi && (code < ev_code[e] || (code == ev_code[e] && key < ev_row[e])))) {
      bad[0] = 1;
      return;
    }
  }
}

// Node columns of m inserted / replaced rows in ONE launch (an insert used to
// be ~16 index_put / cast launches): the per-row values come from a packed
// float64 block vals [ncols, m] (exact for every f32 / i32 / u8 / f64 value)
// in the fixed column order below; a column absent from the block (bit c of
// `present` clear) takes its constant. kind / stored / dirty are constants.
//   0 sal f32 | 1 acc i32 | 2 last f64 | 3 ts f64 | 4 shard i32 | 5 sup u8 | 6 parent i32
__global__ __launch_bounds__(256) void tg_set_rows_kernel(const long* __restrict__ rows, long row0, int m,
                                                          const double* __restrict__ vals, int present,
                                                          const double* __restrict__ consts, float* __restrict__ sal,
                                                          int* __restrict__ acc, double* __restrict__ last,
                                                          double* __restrict__ ts, int* __restrict__ shard,
                                                          unsigned char* __restrict__ sup, int* __restrict__ parent,
                                                          unsigned char* __restrict__ kind,
                                                          unsigned char* __restrict__ stored,
                                                          unsigned char* __restrict__ dirty, int kind_v, int stored_v) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  // present bit 15: the rows are the first m values of vals (exact doubles)
  // instead of `rows`; bits 8-14: columns left as they are (no write);
  // kind_v / stored_v < 0: kind / stored left as they are
  int slot = 0;
  long r;
  if (present & (1 << 15)) r = (long)vals[slot++ * (long)m + j];
  else r = rows ? rows[j] : row0 + j;
  if (r < 0) return;  // a row this rank does not hold (row-sharded tenants)
  double v[7];
#pragma unroll
  for (int c = 0; c < 7; ++c) {
    if (present & (1 << c)) v[c] = vals[(long)(slot++) * m + j];
    else v[c] = consts[c];
  }
  const int skip = present >> 8;
  if (!(skip & 1)) sal[r] = (float)v[0];
  if (!(skip & 2)) acc[r] = (int)v[1];
  if (!(skip & 4)) last[r] = v[2];
  if (!(skip & 8)) ts[r] = v[3];
  if (!(skip & 16)) shard[r] = (int)v[4];
  if (!(skip & 32)) sup[r] = (unsigned char)v[5];
  if (!(skip & 64)) parent[r] = (int)v[6];
  if (kind_v >= 0) kind[r] = (unsigned char)kind_v;
  if (stored_v >= 0) stored[r] = (unsigned char)stored_v;
  dirty[r] = 1;
}

inline unsigned blocks_for(long n, int per = NTB) { return (unsigned)((n + per - 1) / per); }


// Store-search re-rank (reference LanceDBStore.search_nodes ordering,
// vector_store.py:132-140): one wave per query scores its C <= 64 candidate
// rows exactly in fp32 from the stored vectors and emits the top-k by (score
// desc, row asc). metric 0 = l2: 2<q,x> + bias[r] - |q|^2 (bias = -|x|^2, -inf
// for rows outside the store); 1 = ip: <q,x> + bias[r]; 2 = cosine:
// <q,x> / |x| + bias[r]. cand < 0 -> empty. Output rows -1 / scores -inf past
// the valid candidates. Replaces ~20 gather / GEMM / sort launches.
__global__ __launch_bounds__(256) void store_rerank_kernel(const float* __restrict__ Q, long ldq,
                                                           const float* __restrict__ X, long ldx, int D,
                                                           const float* __restrict__ sqn,
                                                           const float* __restrict__ bias,
                                                           const long* __restrict__ cand, int C, int M, int k,
                                                           int metric, float* __restrict__ os,
                                                           long* __restrict__ oi,
                                                           const unsigned char* __restrict__ kind,
                                                           long* __restrict__ oin) {
  const int lane = threadIdx.x & 63;
  const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= M) return;
  const float* qr = Q + (long)q * ldq;
  float qq = 0.f;
  for (int d = lane; d < D; d += 64) qq = fmaf(qr[d], qr[d], qq);
  qq = wave_sum(qq);
  // 16 candidates per pass, 4 lanes each (lane = 4 * c + part): every lane
  // streams its quarter of one row with independent float4 loads, so the
  // pass costs one row-read latency instead of one per candidate
  const int part = lane & 3, cl = lane >> 2;
  float my_s = LZK_NEG_INF;
  long my_r = -1;
  const bool vec = (D % 16) == 0 && (ldq % 4) == 0 && (ldx % 4) == 0;
  for (int c0 = 0; c0 < C; c0 += 16) {
    const int c = c0 + cl;
    const long r = c < C ? cand[(long)q * C + c] : -1;
    float acc = 0.f;
    if (r >= 0) {
      const float* xr = X + r * ldx;
      if (vec) {
        for (int d = part * 4; d < D; d += 16) {
          const float4 xv = *reinterpret_cast<const float4*>(xr + d);
          const float4 qv = *reinterpret_cast<const float4*>(qr + d);
          acc = fmaf(qv.x, xv.x, acc);
          acc = fmaf(qv.y, xv.y, acc);
          acc = fmaf(qv.z, xv.z, acc);
          acc = fmaf(qv.w, xv.w, acc);
        }
      } else {
        for (int d = part; d < D; d += 4) acc = fmaf(qr[d], xr[d], acc);
      }
    }
    acc += __shfl_xor(acc, 1, 64);
    acc += __shfl_xor(acc, 2, 64);
    float sc = LZK_NEG_INF;
    if (r >= 0) {
      if (metric == 0) {
        sc = 2.f * acc + bias[r] - qq;
      } else if (metric == 2) {
        const float nr = sqrtf(sqn[r]);
        sc = acc / (nr > 0.f ? nr : 1.f) + bias[r];
      } else {
        sc = acc + bias[r];
      }
    }
    // candidate c0 + j's result sits in lane 4 j; lane c0 + j takes it
    const int src = 4 * ((lane - c0) & 15);
    const float s2 = __shfl(sc, src, 64);
    const long r2 = __shfl(r, src, 64);
    if (lane >= c0 && lane < c0 + 16 && lane < C) { my_s = s2; my_r = r2; }
  }
  // rank among the wave's (score, row) pairs; -inf scores are empty
  const bool live = lane < C && my_r >= 0 && my_s != LZK_NEG_INF;
  int rank = 0;
  for (int o = 0; o < C; ++o) {
    const float s2 = __shfl(my_s, o, 64);
    const long r2 = __shfl(my_r, o, 64);
    const bool l2 = r2 >= 0 && s2 != LZK_NEG_INF;
    // equal (score, row) pairs (a row listed twice) keep their slot order
    if (l2 && o != lane && (s2 > my_s || (s2 == my_s && (r2 < my_r || (r2 == my_r && o < lane))))) ++rank;
  }
  const int nlive = __popcll(__ballot(live));
  if (live && rank < k) {
    os[(long)q * k + rank] = my_s;
    oi[(long)q * k + rank] = my_r;
    // oin (optional): the same rows with those that are not graph nodes as
    // -1 (search_memories skips them, reference memory_system.py:1467-1472)
    if (oin) oin[(long)q * k + rank] = kind[my_r] == 1 ? my_r : -1;
  }
  for (int j = nlive + lane; j < k; j += 64) {
    os[(long)q * k + j] = LZK_NEG_INF;
    oi[(long)q * k + j] = -1;
    if (oin) oin[(long)q * k + j] = -1;
  }
}


// store_rerank_kernel for narrow batches (the interactive turn): a
// 256-thread block per query, 16 lanes per candidate (4 candidates per wave
// per pass, every float4 of a lane's share issued before its FMAs), the
// scores through LDS, then wave 0 ranks them exactly like the wave kernel --
// one wave streaming 16 candidates' rows was ~23 us of a 1.9 ms search.
__global__ __launch_bounds__(256) void store_rerank_block_kernel(const float* __restrict__ Q, long ldq,
                                                                 const float* __restrict__ X, long ldx, int D,
                                                                 const float* __restrict__ sqn,
                                                                 const float* __restrict__ bias,
                                                                 const long* __restrict__ cand, int C, int M, int k,
                                                                 int metric, float* __restrict__ os,
                                                                 long* __restrict__ oi,
                                                                 const unsigned char* __restrict__ kind,
                                                                 long* __restrict__ oin) {
  __shared__ float s_s[64];
  __shared__ long s_r[64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = blockIdx.x;
  const float* qr = Q + (long)q * ldq;
  float qq = 0.f;
  for (int d = lane; d < D; d += 64) qq = fmaf(qr[d], qr[d], qq);
  qq = wave_sum(qq);
  const int part = lane & 15, g = lane >> 4;
  const bool vec = (D % 64) == 0 && (ldq % 4) == 0 && (ldx % 4) == 0;
  for (int c0 = 0; c0 < C; c0 += 16) {
    const int c = c0 + wave * 4 + g;
    const long r = c < C ? cand[(long)q * C + c] : -1;
    float acc = 0.f;
    if (r >= 0) {
      const float* xr = X + r * ldx;
      if (vec) {
#pragma unroll 4
        for (int d = part * 4; d < D; d += 64) {
          const float4 xv = *reinterpret_cast<const float4*>(xr + d);
          const float4 qv = *reinterpret_cast<const float4*>(qr + d);
          acc = fmaf(qv.x, xv.x, acc);
          acc = fmaf(qv.y, xv.y, acc);
          acc = fmaf(qv.z, xv.z, acc);
          acc = fmaf(qv.w, xv.w, acc);
        }
      } else {
        for (int d = part; d < D; d += 16) acc = fmaf(qr[d], xr[d], acc);
      }
    }
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) acc += __shfl_xor(acc, o, 64);
    if (part == 0 && c < C) {
      float sc = LZK_NEG_INF;
      if (r >= 0) {
        if (metric == 0) {
          sc = 2.f * acc + bias[r] - qq;
        } else if (metric == 2) {
          const float nr = sqrtf(sqn[r]);
          sc = acc / (nr > 0.f ? nr : 1.f) + bias[r];
        } else {
          sc = acc + bias[r];
        }
      }
      s_s[c] = sc;
      s_r[c] = r;
    }
  }
  __syncthreads();
  if (wave != 0) return;
  const float my_s = lane < C ? s_s[lane] : LZK_NEG_INF;
  const long my_r = lane < C ? s_r[lane] : -1;
  const bool live = lane < C && my_r >= 0 && my_s != LZK_NEG_INF;
  int rank = 0;
  for (int o = 0; o < C; ++o) {
    const float s2 = __shfl(my_s, o, 64);
    const long r2 = __shfl(my_r, o, 64);
    const bool l2 = r2 >= 0 && s2 != LZK_NEG_INF;
    // equal (score, row) pairs (a row listed twice) keep their slot order
    if (l2 && o != lane && (s2 > my_s || (s2 == my_s && (r2 < my_r || (r2 == my_r && o < lane))))) ++rank;
  }
  const int nlive = __popcll(__ballot(live));
  if (live && rank < k) {
    os[(long)q * k + rank] = my_s;
    oi[(long)q * k + rank] = my_r;
    if (oin) oin[(long)q * k + rank] = kind[my_r] == 1 ? my_r : -1;
  }
  for (int j = nlive + lane; j < k; j += 64) {
    os[(long)q * k + j] = LZK_NEG_INF;
    oi[(long)q * k + j] = -1;
    if (oin) oin[(long)q * k + j] = -1;
  }
}

// Consolidation's candidate re-rank in ONE launch (replaces a gather of the
// [M, c, D] rows in float64, an einsum, a division and two sorts): exact
// float64 cosine of each fact's kernel candidates -- <qn, x> / |x| with qn the
// fp64 unit fact and x the fp32 row, |x| = sqrt(fp32 |x|^2) in fp64 (the
// formula the batch planner replays) -- ranked (score desc, row asc), cut to
// k; empty slots (-inf, -1). One wave per fact, 4 lanes per candidate.
__global__ __launch_bounds__(256) void cos_rerank64_kernel(const double* __restrict__ Qn, long ldq,
                                                           const float* __restrict__ X, long ldx, int D,
                                                           const float* __restrict__ sqn,
                                                           const long* __restrict__ cand, int C, int M, int k,
                                                           double* __restrict__ os, long* __restrict__ oi) {
  const int lane = threadIdx.x & 63;
  const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= M) return;
  const double* qr = Qn + (long)q * ldq;
  const int part = lane & 3, cl = lane >> 2;
  double my_s = -__builtin_huge_val();
  long my_r = -1;
  for (int c0 = 0; c0 < C; c0 += 16) {
    const int c = c0 + cl;
    const long r = c < C ? cand[(long)q * C + c] : -1;
    double acc = 0.0;
    if (r >= 0) {
      const float* xr = X + r * ldx;
      for (int d = part; d < D; d += 4) acc = fma(qr[d], (double)xr[d], acc);
    }
    acc += __shfl_xor(acc, 1, 64);
    acc += __shfl_xor(acc, 2, 64);
    double sc = -__builtin_huge_val();
    if (r >= 0) {
      const double nr = sqrt((double)sqn[r]);
      sc = acc / (nr > 0.0 ? nr : 1.0);
    }
    const int src = 4 * ((lane - c0) & 15);
    const double s2 = __shfl(sc, src, 64);
    const long r2 = __shfl(r, src, 64);
    if (lane >= c0 && lane < c0 + 16 && lane < C) { my_s = s2; my_r = r2; }
  }
  const bool live = lane < C && my_r >= 0;
  int rank = 0;
  for (int o = 0; o < C; ++o) {
    const double s2 = __shfl(my_s, o, 64);
    const long r2 = __shfl(my_r, o, 64);
    // equal (score, row) pairs (a row listed twice) keep their slot order
    if (r2 >= 0 && o != lane && (s2 > my_s || (s2 == my_s && (r2 < my_r || (r2 == my_r && o < lane))))) ++rank;
  }
  const int nlive = __popcll(__ballot(live));
  if (live && rank < k) {
    os[(long)q * k + rank] = my_s;
    oi[(long)q * k + rank] = my_r;
  }
  for (int j = nlive + lane; j < k; j += 64) {
    os[(long)q * k + j] = -__builtin_huge_val();
    oi[(long)q * k + j] = -1;
  }
}

// Embedding-row writes of a small node insert in ONE launch (the consolidation
// segments insert ~20 facts, 43 times per 128-conversation step): per row j,
// x = e32[j] * has[j] goes to emb32[rows[j]], its bf16 copy to emb16, the
// per-row symmetric int8 copy of the bf16 values + scale (max|x|/127, 0 for a
// zero row) to emb8 / rs8 (the store search's int8 scan), |x|^2 (fp64 sum,
// stored fp32) to sqn, x_d^2 to the per-dimension sums (fp64 atomics), and
// max | |x| - 1 | over the valid rows / the largest row scale to two device
// maxima (positive floats, max on the bits). Same values as the torch path
// it replaces (ops/search.py quantize_i8_rows: round half to even).
__global__ __launch_bounds__(256) void tg_write_emb_kernel(
    const float* __restrict__ x, long ldx, const unsigned char* __restrict__ has, int m, int D,
    const long* __restrict__ rows, long row0, float* __restrict__ emb32, long ld32, u16* __restrict__ emb16,
    long ld16, signed char* __restrict__ emb8, long ld8, float* __restrict__ rs8, float* __restrict__ sqn,
    double* __restrict__ sumsq, float* __restrict__ rs_max, float* __restrict__ dv_max,
    unsigned char* __restrict__ has_emb) {
  __shared__ double red_d[4];
  __shared__ float red_f[4];
  const int j = blockIdx.x;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const float hv = (has == nullptr || has[j]) ? 1.f : 0.f;
  const long r = rows ? rows[j] : row0 + j;  // rows null: the contiguous rows row0 ..
  float v[4], vb[4];
  double s2 = 0.0;
  float am = 0.f;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int d = t + 256 * c;
    v[c] = vb[c] = 0.f;
    if (d < D) {
      v[c] = x[(long)j * ldx + d] * hv;
      emb32[r * ld32 + d] = v[c];
      const u16 b = f32_to_bf16(v[c]);
      if (emb16) emb16[r * ld16 + d] = b;
      vb[c] = bf16_to_f32(b);
      const double q2 = (double)v[c] * (double)v[c];
      s2 += q2;
      if (sumsq) atomicAdd(sumsq + d, q2);
      am = fmaxf(am, fabsf(vb[c]));
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    s2 += __shfl_xor(s2, o, 64);
    am = fmaxf(am, __shfl_xor(am, o, 64));
  }
  if (lane == 0) { red_d[w] = s2; red_f[w] = am; }
  __syncthreads();
  s2 = red_d[0] + red_d[1] + red_d[2] + red_d[3];
  am = fmaxf(fmaxf(red_f[0], red_f[1]), fmaxf(red_f[2], red_f[3]));
  if (emb8) {
    // a zero row quantises exactly (q = 0) with scale 0: it must not widen
    // the tenant's error model (rs_max) nor the scan's row-group bounds
    const float sc = am > 0.f ? am * (1.f / 127.f) : 0.f;  // torch: amax / 127.0 = amax * (1/127)
    const float den = am > 0.f ? sc : 1.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int d = t + 256 * c;
      if (d < D) emb8[r * ld8 + d] = (signed char)fminf(fmaxf(rintf(vb[c] / den), -127.f), 127.f);
    }
    if (t == 0) {
      rs8[r] = sc;
      if (rs_max && am > 0.f) atomicMax(reinterpret_cast<int*>(rs_max), __float_as_int(sc));
    }
  }
  if (t == 0) {
    sqn[r] = (float)s2;
    if (dv_max && hv > 0.f) atomicMax(reinterpret_cast<int*>(dv_max), __float_as_int((float)fabs(sqrt(s2) - 1.0)));
    if (has_emb) has_emb[r] = hv > 0.f ? 1 : 0;
  }
}

// Edge append of a consolidation segment from one pinned float64 block
// [src | dst | w | shard code] x m (exact for rows, codes and fp32 weights):
// the six edge columns at [ne, ne + m) of buffers with room for them.
__global__ __launch_bounds__(NTB) void tg_append_edges_kernel(const double* __restrict__ vals, int m, long ne,
                                                              int meta_bits, double now, int* __restrict__ src,
                                                              int* __restrict__ dst, float* __restrict__ w,
                                                              int* __restrict__ co, double* __restrict__ lu,
                                                              int* __restrict__ meta) {
  const int j = blockIdx.x * NTB + threadIdx.x;
  if (j >= m) return;
  const long o = ne + j;
  src[o] = (int)vals[j];
  dst[o] = (int)vals[(long)m + j];
  w[o] = (float)vals[2L * m + j];
  co[o] = 1;
  lu[o] = now;
  meta[o] = ((int)vals[3L * m + j] & 0xFFFFFF) | meta_bits;
}

// Segment end (consolidate_batch): the victims' (kind, sup, shard) into
// info, the live ones marked in the removal bitmap, turned into ghosts and
// unstored -- the gathers, masks and scatters of the torch formulation in
// one pass over the victims. The bitmap is persistent and all-zero between
// segments: tg_clear_bits_kernel clears the victims' words after the flags.
__global__ __launch_bounds__(NTB) void tg_victims_kernel(const long* __restrict__ rows, int nv,
                                                         unsigned char* __restrict__ kind,
                                                         const unsigned char* __restrict__ sup,
                                                         const int* __restrict__ shard,
                                                         unsigned char* __restrict__ stored, int unstore,
                                                         unsigned* __restrict__ rmb, int* __restrict__ info) {
  const int i = blockIdx.x * NTB + threadIdx.x;
  if (i >= nv) return;
  const long r = rows[i];
  const unsigned char k = kind[r];
  info[i] = k;
  info[nv + i] = sup[r];
  info[2 * nv + i] = shard[r];
  if (k == 1) {
    atomicOr(rmb + (r >> 5), 1u << (r & 31));
    kind[r] = 2;
    if (unstore) stored[r] = 0;
  }
}

__global__ __launch_bounds__(NTB) void tg_clear_bits_kernel(const long* __restrict__ rows, int nv,
                                                            unsigned* __restrict__ rmb) {
  const int i = blockIdx.x * NTB + threadIdx.x;
  if (i < nv) rmb[rows[i] >> 5] = 0u;
}

// The first rows of the shard nodes in (shard code, row) order -- the rows
// run_consolidation's profile prompt reads when no component qualifies
// (reference memory_system.py:1003-1008, BufferGraph.nodes order) -- without
// a host round trip: the host turns its per-shard live counts into targets
// (code tc[t], rows wanted tt[t], output offset to[t]) and ONE block scans
// the rows from 0 in chunks, appending each target's live rows in row order
// (block-wide ranks from ballots) until every target is met -- usually
// within the first chunk or two. out[] must be pre-filled with -1.
constexpr int FR_NT = 1024;
constexpr int FR_MAXT = 64;
struct FrTargets {  // by value (kernel arguments): no host -> device copy
  int nt;
  int tc[FR_MAXT], tt[FR_MAXT], to[FR_MAXT];
};
__global__ __launch_bounds__(FR_NT) void tg_first_rows_kernel(const unsigned char* __restrict__ kind,
                                                              const unsigned char* __restrict__ sup,
                                                              const int* __restrict__ shard, long n, FrTargets T,
                                                              long* __restrict__ out) {
  // per chunk: every wave ballots each open target once (per-target, per-wave
  // counts in LDS), ONE barrier, then each row's block-wide rank within its
  // target -- four barriers per chunk instead of three per open target
  __shared__ int s_tc[FR_MAXT], s_tt[FR_MAXT], s_to[FR_MAXT], s_found[FR_MAXT];
  __shared__ int s_cnt[FR_MAXT][FR_NT / 64];
  __shared__ int s_open;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int nt = T.nt;
  for (int t = threadIdx.x; t < nt; t += FR_NT) {
    s_tc[t] = T.tc[t];
    s_tt[t] = T.tt[t];
    s_to[t] = T.to[t];
    s_found[t] = 0;
  }
  __syncthreads();
  for (long base = 0; base < n; base += FR_NT) {
    const long r = base + threadIdx.x;
    const int c = (r < n && kind[r] == 1 && sup[r] == 0) ? shard[r] : -1;
    int j = -1;
    for (int t = 0; t < nt; ++t) j = (s_tc[t] == c) ? t : j;
    unsigned long long myb = 0;
    for (int t = 0; t < nt; ++t) {
      if (s_found[t] >= s_tt[t]) continue;  // block-uniform: s_found changes only behind barriers
      const unsigned long long b = __ballot(j == t);
      if (lane == 0) s_cnt[t][wv] = __popcll(b);
      if (j == t) myb = b;
    }
    __syncthreads();
    if (j >= 0 && s_found[j] < s_tt[j]) {
      int before = 0;
      for (int w = 0; w < wv; ++w) before += s_cnt[j][w];
      const int rank = s_found[j] + before + (int)__popcll(myb & ((1ull << lane) - 1));
      if (rank < s_tt[j]) out[s_to[j] + rank] = r;
    }
    __syncthreads();  // every lane read s_found / s_cnt
    if (threadIdx.x < nt) {
      const int t = threadIdx.x;
      if (s_found[t] < s_tt[t]) {
        int total = 0;
        for (int w = 0; w < FR_NT / 64; ++w) total += s_cnt[t][w];
        s_found[t] = min(s_tt[t], s_found[t] + total);
      }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int open = 0;
      for (int t = 0; t < nt; ++t) open |= s_found[t] < s_tt[t];
      s_open = open;
    }
    __syncthreads();
    if (!s_open) break;
  }
  // targets not met (inconsistent counts): their remaining slots read -1
  for (int t = 0; t < nt; ++t)
    for (int i = s_found[t] + threadIdx.x; i < s_tt[t]; i += FR_NT) out[s_to[t] + i] = -1;
}

}  // namespace

// ---------------------------------------------------------------- C ABI
LZK_EXPORT int lzk_tg_decay(float* w, long ne, float keep, float thr, unsigned char* flag, int* block_cnt, float* sal,
                            const unsigned char* kind, const unsigned char* sup, long nn, int decay_nodes, int steps,
                            void* stream) {
  if (steps < 0) return (int)hipErrorInvalidValue;
  long nb = (ne + NTB - 1) / NTB;
  if (nb == 0) nb = 1;
  // nodes ride in the edge launch only while its grid can stream them
  const long node_blocks = (nn + 4L * NTB - 1) / (4L * NTB);
  const bool fused = decay_nodes && (nb >= node_blocks || nb >= 2048);
  if (ne > 0 || fused)
    hipLaunchKernelGGL(tg_decay_kernel, dim3((unsigned)nb), dim3(NTB), 0, (hipStream_t)stream, w, ne, keep, thr, flag,
                       block_cnt, sal, kind, sup, nn, fused ? 1 : 0, steps);
  if (decay_nodes && !fused && nn > 0) {
    const long g = node_blocks < 4096 ? node_blocks : 4096;
    hipLaunchKernelGGL(tg_node_decay_kernel, dim3((unsigned)g), dim3(NTB), 0, (hipStream_t)stream, sal, kind, sup, nn,
                       keep, steps);
  }
  return (int)hipGetLastError();
}

// rmb: bitmap of the removed rows (lzk_pack_bits), or nullptr (prev only).
LZK_EXPORT int lzk_tg_flag_remove(const int* src, const int* dst, const int* meta, long ne, const unsigned* rmb,
                                  const int* shard, const unsigned char* prev, long nprev, unsigned char* flag,
                                  int* block_cnt, void* stream) {
  if (ne == 0) return 0;
  if (nprev < 0 || nprev > ne || (prev == nullptr && rmb == nullptr)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(tg_flag_remove_kernel, dim3(blocks_for(ne)), dim3(NTB), 0, (hipStream_t)stream, src, dst, meta,
                     ne, rmb, shard, prev, nprev, flag, block_cnt, (int*)nullptr);
  return (int)hipGetLastError();
}

// bits: (n + 31) / 32 words; f must be 16-byte aligned (a fresh allocation).
LZK_EXPORT int lzk_pack_bits(const unsigned char* f, long n, unsigned* bits, void* stream) {
  if (n <= 0) return 0;
  if ((reinterpret_cast<uintptr_t>(f) & 15) != 0) return (int)hipErrorInvalidValue;
  const long words = (n + 31) / 32;
  hipLaunchKernelGGL(pack_bits_kernel, dim3(blocks_for(words)), dim3(NTB), 0, (hipStream_t)stream, f, n, bits);
  return (int)hipGetLastError();
}

LZK_EXPORT int lzk_tg_compact(const unsigned char* flag, const int* block_off, long ne, const int* src, const int* dst,
                              const float* w, const int* co, const double* lu, const int* meta, int* osrc, int* odst,
                              float* ow, int* oco, double* olu, int* ometa, int* dsrc, int* ddst, int* dmeta,
                              void* stream) {
  if (ne == 0) return 0;
  hipLaunchKernelGGL(tg_compact_kernel, dim3(blocks_for(ne)), dim3(NTB), 0, (hipStream_t)stream, flag, block_off, ne,
                     src, dst, w, co, lu, meta, osrc, odst, ow, oco, olu, ometa, dsrc, ddst, dmeta);
  return (int)hipGetLastError();
}

LZK_EXPORT int lzk_tg_boost(const long* off, const int* adj, const int* eid, const float* w, const int* seeds,
                            int nseeds, const unsigned char* kind, const unsigned char* sup, float min_w, double now,
                            double delta, float* sal, double* last, unsigned char* dirty, int* stamp, int epoch,
                            int* nboost, void* stream) {
  if (nseeds <= 0) return 0;
  hipLaunchKernelGGL(tg_boost_kernel, dim3(nseeds), dim3(64), 0, (hipStream_t)stream, off, adj, eid, w, seeds, nseeds,
                     kind, sup, min_w, now, delta, sal, last, dirty, stamp, epoch, nboost);
  return (int)hipGetLastError();
}

LZK_EXPORT int lzk_tg_touch(const long* rows, int n, int* acc, double* last, float* sal, unsigned char* dirty,
                            double now, double delta, void* stream) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(tg_touch_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, (hipStream_t)stream, rows, n, acc,
                     last, sal, dirty, now, delta);
  return (int)hipGetLastError();
}

LZK_EXPORT int lzk_tg_importance(const float* sal, const int* acc, const double* last, const unsigned char* kind,
                                 const unsigned char* sup, long n, double now, double* out, void* stream) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(tg_importance_kernel, dim3(blocks_for(n)), dim3(NTB), 0, (hipStream_t)stream, sal, acc, last,
                     kind, sup, n, now, out);
  return (int)hipGetLastError();
}

LZK_EXPORT int lzk_tg_evict_verify(const float* sal, const int* acc, const double* last, const unsigned char* kind,
                                   const unsigned char* sup, const int* shard, const unsigned char* pool, long n,
                                   double now, float keep, int ne, const int* ev_steps, const double* ev_imp,
                                   const int* ev_code, const long* ev_row, int* bad, void* stream,
                                   const long* rowkey, double vmax, int st_last, double kt, int max_code,
                                   long max_key) {
  if (n <= 0 || ne <= 0) return 0;
  hipLaunchKernelGGL(tg_evict_verify_kernel, dim3(blocks_for(n)), dim3(NTB), 0, (hipStream_t)stream, sal, acc, last,
                     kind, sup, shard, pool, n, now, keep, ne, ev_steps, ev_imp, ev_code, ev_row, bad, rowkey, vmax,
                     st_last, kt, max_code, max_key);
  return (int)hipGetLastError();
}

// Result fields of a multi-tenant search (DistributedMemoryService): result
// (q, j) is row rows[q * k + j] of query q's tenant, whose columns live in
// separate allocations -- per-query base pointers [5][nq] (sal f32, acc i32,
// kind u8, sup u8, shard i32). One launch instead of a gather per tenant.
__global__ __launch_bounds__(256) void tg_gather_fields_kernel(const long* __restrict__ rows, int nq, int k,
                                                                const unsigned long long* __restrict__ base,
                                                                float* __restrict__ o_sal, int* __restrict__ o_acc,
                                                                unsigned char* __restrict__ o_kind,
                                                                unsigned char* __restrict__ o_sup,
                                                                int* __restrict__ o_shard) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long)nq * k) return;
  const int q = (int)(t / k);
  const long r = rows[t];
  if (r < 0) {
    o_sal[t] = 0.f; o_acc[t] = 0; o_kind[t] = 0; o_sup[t] = 0; o_shard[t] = -1;
    return;
  }
  o_sal[t] = reinterpret_cast<const float*>(base[q])[r];
  o_acc[t] = reinterpret_cast<const int*>(base[nq + q])[r];
  o_kind[t] = reinterpret_cast<const unsigned char*>(base[2 * nq + q])[r];
  o_sup[t] = reinterpret_cast<const unsigned char*>(base[3 * nq + q])[r];
  o_shard[t] = reinterpret_cast<const int*>(base[4 * nq + q])[r];
}

LZK_EXPORT int lzk_tg_gather_fields(const long* rows, int nq, int k, const void* base, float* o_sal, int* o_acc,
                                    unsigned char* o_kind, unsigned char* o_sup, int* o_shard, void* stream) {
  const long n = (long)nq * k;
  if (n <= 0) return 0;
  hipLaunchKernelGGL(tg_gather_fields_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     rows, nq, k, (const unsigned long long*)base, o_sal, o_acc, o_kind, o_sup, o_shard);
  return (int)hipGetLastError();
}

LZK_EXPORT int lzk_store_rerank(const float* Q, long ldq, const float* X, long ldx, int D, const float* sqn,
                                const float* bias, const long* cand, int C, int M, int k, int metric, float* os,
                                long* oi, const unsigned char* kind, long* oin, void* stream) {
  if (C <= 0 || C > 64 || M <= 0 || k <= 0 || metric < 0 || metric > 2 || (oin && !kind))
    return (int)hipErrorInvalidValue;
  if (M < 64)  // narrow: a block per query
    hipLaunchKernelGGL(store_rerank_block_kernel, dim3((unsigned)M), dim3(256), 0, (hipStream_t)stream, Q, ldq, X,
                       ldx, D, sqn, bias, cand, C, M, k, metric, os, oi, kind, oin);
  else
    hipLaunchKernelGGL(store_rerank_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, (hipStream_t)stream, Q,
                       ldq, X, ldx, D, sqn, bias, cand, C, M, k, metric, os, oi, kind, oin);
  return (int)hipGetLastError();
}

LZK_EXPORT int lzk_tg_set_rows(const long* rows, long row0, int m, const double* vals, int present,
                               const double* consts, float* sal, int* acc, double* last, double* ts, int* shard,
                               unsigned char* sup, int* parent, unsigned char* kind, unsigned char* stored,
                               unsigned char* dirty, int kind_v, int stored_v, void* stream) {
  if (m <= 0) return 0;
  hipLaunchKernelGGL(tg_set_rows_kernel, dim3(blocks_for(m, 256)), dim3(256), 0, (hipStream_t)stream, rows, row0, m,
                     vals, present, consts, sal, acc, last, ts, shard, sup, parent, kind, stored, dirty, kind_v,
                     stored_v);
  return (int)hipGetLastError();
}

LZK_EXPORT int lzk_tg_write_emb(const float* x, long ldx, const unsigned char* has, int m, int D, const long* rows,
                                long row0, float* emb32, long ld32, void* emb16, long ld16, void* emb8, long ld8,
                                float* rs8, float* sqn, double* sumsq, float* rs_max, float* dv_max,
                                unsigned char* has_emb, void* stream) {
  if (m <= 0) return 0;
  if (D <= 0 || D > 1024 || (emb8 && !rs8)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(tg_write_emb_kernel, dim3((unsigned)m), dim3(256), 0, (hipStream_t)stream, x, ldx, has, m, D,
                     rows, row0, emb32, ld32, (u16*)emb16, ld16, (signed char*)emb8, ld8, rs8, sqn, sumsq, rs_max,
                     dv_max, has_emb);
  return (int)hipGetLastError();
}

// Exact float64 cosine re-rank of candidate rows (cos_rerank64_kernel).
// Qn [M, D] fp64 (row stride ldq), X fp32 rows (stride ldx), cand int64 [M, C]
// (-1 empty, C <= 64), outputs [M, k] (k <= C).
LZK_EXPORT int lzk_cos_rerank64(const double* Qn, long ldq, const float* X, long ldx, int D, const float* sqn,
                                const long* cand, int C, int M, int k, double* os, long* oi, void* stream) {
  if (M <= 0) return 0;
  if (C <= 0 || C > 64 || k <= 0 || k > C || D <= 0) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(cos_rerank64_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, (hipStream_t)stream, Qn, ldq,
                     X, ldx, D, sqn, cand, C, M, k, os, oi);
  return (int)hipGetLastError();
}

// First shard-node rows (tg_first_rows_kernel): nt <= 64 targets, out[sum tt]
// pre-filled with -1 by the caller. One block, no host synchronisation.
// tc / tt / to: HOST arrays of the nt targets (passed by value to the kernel).
LZK_EXPORT int lzk_tg_first_rows(const unsigned char* kind, const unsigned char* sup, const int* shard, long n,
                                 const int* tc, const int* tt, const int* to, int nt, long* out, void* stream) {
  if (nt <= 0) return 0;
  if (nt > FR_MAXT || n < 0) return (int)hipErrorInvalidValue;
  FrTargets T;
  T.nt = nt;
  for (int t = 0; t < nt; ++t) {
    T.tc[t] = tc[t];
    T.tt[t] = tt[t];
    T.to[t] = to[t];
  }
  hipLaunchKernelGGL(tg_first_rows_kernel, dim3(1), dim3(FR_NT), 0, (hipStream_t)stream, kind, sup, shard, n, T, out);
  return (int)hipGetLastError();
}

// Row-sharded tenants (parallel/sharded_memory.py _rows_of_nums): the local
// row of each global node number through the sorted number index -- a base
// over rows [0, n0) and a delta over the rows appended since, each (sorted
// numbers, rows) -- the base winning a (never expected) tie; -1 if absent.
// rank >= 0: only rows this rank holds live (holder == rank, kind NODE).
// One launch instead of two searchsorted passes and their selects.
__device__ __forceinline__ long lower_idx(const long* __restrict__ k, long n, long v) {
  long lo = 0, hi = n;
  while (lo < hi) {
    const long mid = (lo + hi) >> 1;
    if (k[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(256) void num_rows_kernel(const long* __restrict__ nums, long add, long m,
                                                       const long* __restrict__ bk, const long* __restrict__ bo,
                                                       long nb, const long* __restrict__ dk,
                                                       const long* __restrict__ dox, long nd,
                                                       const long* __restrict__ holder,
                                                       const unsigned char* __restrict__ kind, long rank,
                                                       long* __restrict__ out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  const long v = nums[i] + add;
  long r = -1;
  long p = lower_idx(bk, nb, v);
  if (p < nb && bk[p] == v) {
    r = bo[p];
  } else {
    p = lower_idx(dk, nd, v);
    if (p < nd && dk[p] == v) r = dox[p];
  }
  if (r >= 0 && rank >= 0 && !(holder[r] == rank && kind[r] == 1)) r = -1;
  out[i] = r;
}

LZK_EXPORT int lzk_num_rows(const long* nums, long add, long m, const long* bk, const long* bo, long nb,
                            const long* dk, const long* dox, long nd, const long* holder,
                            const unsigned char* kind, long rank, long* out, void* stream) {
  if (m <= 0) return 0;
  if (nb < 0 || nd < 0 || (rank >= 0 && (!holder || !kind))) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(num_rows_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, (hipStream_t)stream, nums,
                     add, m, bk, bo, nb, dk, dox, nd, holder, kind, rank, out);
  return (int)hipGetLastError();
}

// Row-sharded cone radii (parallel/sharded_memory.py _row_cos with labels):
// cos of each row with ITS cluster's unit centroid, fp32 -- one wave per
// row, 16-B loads, a wave reduction; rows without a vector (sqn 0) -> -1.
// One read of the rows instead of a [rows x K] GEMM for one column each.
__global__ __launch_bounds__(256) void row_cent_cos_kernel(const float* __restrict__ X, long ldx, int D,
                                                           const float* __restrict__ sqn,
                                                           const long* __restrict__ rows,
                                                           const long* __restrict__ lab, long m,
                                                           const float* __restrict__ C, long ldc,
                                                           float* __restrict__ out) {
  const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (i >= m) return;
  const long r = rows[i];
  const float* x = X + r * ldx;
  const float* c = C + lab[i] * ldc;
  float acc = 0.f;
  for (int k = lane * 4; k < D; k += 256) {  // D % 4 == 0 (checked by the caller)
    const float4 a = *reinterpret_cast<const float4*>(x + k);
    const float4 b = *reinterpret_cast<const float4*>(c + k);
    acc += a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if (lane == 0) {
    const float n2 = sqn[r];
    out[i] = n2 > 0.f ? acc / sqrtf(n2) : -1.f;
  }
}

LZK_EXPORT int lzk_row_cent_cos(const float* X, long ldx, int D, const float* sqn, const long* rows,
                                const long* lab, long m, const float* C, long ldc, float* out, void* stream) {
  if (m <= 0) return 0;
  if (D <= 0 || D % 4 != 0 || ldx % 4 != 0 || ldc % 4 != 0) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(row_cent_cos_kernel, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, (hipStream_t)stream, X, ldx,
                     D, sqn, rows, lab, m, C, ldc, out);
  return (int)hipGetLastError();
}

extern "C" int lzk_scan_blocks(int* cnt, int n, int* total, void* stream);

// One segment end of consolidate_batch (TenantGraph.segment_end): victims
// (int64 rows, distinct, nv >= 0) -> info[0 .. 3 nv) = their kind / sup /
// shard before the removal, live ones ghosted (+ unstored) and their shard's
// edges flagged for removal together with the decay's deferred prune (prev,
// the keep flags of the first nprev edges): flag / bc (block offsets after
// the scan) for lzk_tg_compact, info[3 nv] = surviving edges, info[3 nv + 1]
// = edges the decay pruned. rmb: the graph's persistent all-zero bitmap of
// (n + 31) / 32 words. Five launches, one host read of info by the caller.
LZK_EXPORT int lzk_tg_seg_end(const long* vrows, int nv, unsigned char* kind, const unsigned char* sup,
                              const int* shard, unsigned char* stored, int unstore, unsigned* rmb, const int* src,
                              const int* dst, const int* meta, long ne, const unsigned char* prev, long nprev,
                              unsigned char* flag, int* bc, int* info, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (nv < 0 || nprev < 0 || nprev > ne || (ne > 0 && (flag == nullptr || bc == nullptr)))
    return (int)hipErrorInvalidValue;
  hipError_t err = hipMemsetAsync(info + 3L * nv, 0, 2 * sizeof(int), st);
  if (err != hipSuccess) return (int)err;
  if (nv > 0)
    hipLaunchKernelGGL(tg_victims_kernel, dim3(blocks_for(nv)), dim3(NTB), 0, st, vrows, nv, kind, sup, shard, stored,
                       unstore, rmb, info);
  if (ne > 0) {
    hipLaunchKernelGGL(tg_flag_remove_kernel, dim3(blocks_for(ne)), dim3(NTB), 0, st, src, dst, meta, ne,
                       nv > 0 ? rmb : nullptr, shard, prev, nprev, flag, bc, info + 3L * nv + 1);
    const int rc = lzk_scan_blocks(bc, (int)blocks_for(ne), info + 3L * nv, stream);
    if (rc != 0) return rc;
  }
  if (nv > 0) hipLaunchKernelGGL(tg_clear_bits_kernel, dim3(blocks_for(nv)), dim3(NTB), 0, st, vrows, nv, rmb);
  return (int)hipGetLastError();
}

// Segment edge append (tg_append_edges_kernel); vals: device float64 [4][m].
LZK_EXPORT int lzk_tg_append_edges(const double* vals, int m, long ne, int meta_bits, double now, int* src, int* dst,
                                   float* w, int* co, double* lu, int* meta, void* stream) {
  if (m <= 0) return 0;
  hipLaunchKernelGGL(tg_append_edges_kernel, dim3(blocks_for(m)), dim3(NTB), 0, (hipStream_t)stream, vals, m, ne,
                     meta_bits, now, src, dst, w, co, lu, meta);
  return (int)hipGetLastError();
}
