// Cross-encoder re-ranking of a search's pool (rerank=): the three kernels
// around the encoder layers (lazzaro_amd/ops/crossenc_ops.py holds the
// contract in full; models/cross_encoder.py runs the layers between them).
//
//   pair     slot b = m * P + j holds graph row r = rows[b] (< 0 or >= n: an
//            empty slot). ql = qlen[m] (0 .. 64), dl = min(dlen[r], L, max_pos
//            - 3 - ql). The sequence is [CLS] q_1..q_ql [SEP] d_1..d_dl [SEP]:
//            ql + dl + 3 tokens, token types 0 through the first [SEP] and 1
//            after it, positions 0 .. ql + dl + 2. An empty slot is [CLS]
//            [SEP] [SEP] (ql = dl = 0), so no sequence is empty.
//   lens     ce_lens_kernel: lens[b], their exclusive prefix cu[0 .. B] and
//            stat = (T, S_max) = (cu[B], the longest sequence). One block of
//            1024 threads strides over B <= 65,536 with a block scan and a
//            running carry.
//   embed    ce_embed_ln_kernel: one block of 4 waves per pair; the pair is
//            assembled in LDS from the query's ids (int32 [M, 64], shared by
//            the P pairs of m) and the memory's 16-bit row (16-byte loads
//            when the column is aligned), and wave w embeds tokens w, w + 4,
//            ...: word + position + type[type] gathered and normalised exactly
//            as encoder.hip embed_ln_kernel does -- the fp32 sum order word +
//            pos + type, wave_sum for the mean and the variance, rsqrtf, the
//            same lane-to-column map (H % 4 == 0, H <= 1024) -- into bf16 row
//            cu[b] + p. No id / position / type array is written unless the
//            three nullable output pointers ask for them (the tests).
//   head     ce_head_select_kernel: one block per query, 16 lanes per pool
//            slot. logit = <wc, tanh(pooled)> + bc over the bf16 pooler
//            output, tanhf per element, the dot in lzk_dot16.h's order (lane
//            `part` takes the float4 indices d4 == part mod 16 ascending, one
//            fmaf each, folded by xor 8, 4, 2, 1); empty slots get -inf. The
//            slots' 64-bit (logit, row) keys are sorted by one wave
//            (lzk_topk64.h's wave_sort_desc; a pool is one 64-entry block,
//            so the tournament has no merge round) and the k largest
//            come back descending, ties to the lower row, (-inf, -1) beyond
//            the pool's real rows.
//
// ce_head_tol: the distance of the logit from fp64, GIVEN the bf16 pooler
// output x (the pooler GEMM is judged by its own bound). Let S = sum |wc_i|.
//   * tanhf is within 2 ulp of tanh (the HIP math API's stated error); |tanh|
//     <= 1, so an ulp is at most 2^-24: each term wc_i tanhf(x_i) is off by at
//     most 2 |wc_i| 2^-24, S 2^-23 in all. Counted as 4 S 2^-24, twice that.
//   * the H fused multiply-adds and the 4 folds each round a partial sum of
//     magnitude at most S once: at most (H + 4) S 2^-24 in any order (the
//     classic worst case; the kernel's depth is only 4 ceil(H / 64) + 4).
//   * the bias add rounds a number of magnitude at most S + |bc| once.
//   |logit32 - logit64| <= (H + 9) (S + |bc|) 2^-24        (ce_head_tol in ops/crossenc_ops.py)
// The CPU tier sums in another order; the bound holds for every order.
#include "lzk_common.h"
#include "lzk_dot16.h"
#include "lzk_topk64.h"

namespace {

constexpr int CE_MAX_Q = 64;      // query tokens kept (MAX_QUERY_TOKENS)
constexpr int CE_MAX_L = 128;     // memory tokens kept, at most
constexpr int CE_MAX_P = 64;      // slots per pool
constexpr int CE_MAX_B = 65536;   // pairs per call
constexpr int CE_SCAN_NT = 1024;
constexpr int CE_HEAD_NT = 16 * CE_MAX_P;

// (ql, dl) of slot (m, r): the pair rule, clamped so that nothing indexed by them can leave its row
__device__ __forceinline__ void ce_pair(long r, int n, const int* __restrict__ qlen, int m,
                                        const int* __restrict__ dlen, int L, int max_pos, int& ql, int& dl) {
  ql = 0;
  dl = 0;
  if (r < 0 || r >= n) return;
  ql = min(max(qlen[m], 0), min(CE_MAX_Q, max_pos - 3));
  dl = max(min(min(dlen[r], L), max_pos - 3 - ql), 0);
}

__global__ __launch_bounds__(CE_SCAN_NT) void ce_lens_kernel(const long* __restrict__ rows, int B, int P,
                                                             const int* __restrict__ qlen,
                                                             const int* __restrict__ dlen, int n, int L, int max_pos,
                                                             int* __restrict__ lens, int* __restrict__ cu,
                                                             int* __restrict__ stat) {
  __shared__ int s_w[CE_SCAN_NT / 64];
  __shared__ int s_mx[CE_SCAN_NT / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int carry = 0, mx = 0;
  for (int base = 0; base < B; base += CE_SCAN_NT) {  // (block-uniform trip count)
    const int i = base + tid;
    int len = 0;
    if (i < B) {
      int ql, dl;
      ce_pair(rows[i], n, qlen, i / P, dlen, L, max_pos, ql, dl);
      len = ql + dl + 3;
      lens[i] = len;
      mx = max(mx, len);
    }
    int v = len;  // inclusive scan of the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(v, o, 64);
      if (lane >= o) v += t;
    }
    if (lane == 63) s_w[wave] = v;
    __syncthreads();
    int woff = 0, total = 0;
#pragma unroll
    for (int w = 0; w < CE_SCAN_NT / 64; ++w) {
      const int t = s_w[w];
      if (w < wave) woff += t;
      total += t;
    }
    if (i < B) cu[i] = carry + woff + v - len;
    carry += total;
    __syncthreads();  // s_w is written again by the next round
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) mx = max(mx, __shfl_xor(mx, o, 64));
  if (lane == 0) s_mx[wave] = mx;
  __syncthreads();
  if (tid == 0) {
    int m2 = 0;
    for (int w = 0; w < CE_SCAN_NT / 64; ++w) m2 = max(m2, s_mx[w]);
    cu[B] = carry;
    stat[0] = carry;
    stat[1] = m2;
  }
}

__global__ __launch_bounds__(256) void ce_embed_ln_kernel(
    const long* __restrict__ rows, int P, int n, const int* __restrict__ qtok, const int* __restrict__ qlen,
    const u16* __restrict__ tok, const int* __restrict__ dlen, int L, int max_pos, const int* __restrict__ cu, int T,
    int cls_id, int sep_id, int vocab, int vec, const u16* __restrict__ wemb, const u16* __restrict__ pemb,
    const u16* __restrict__ temb, const float* __restrict__ g, const float* __restrict__ bta, int H, float eps,
    u16* __restrict__ Y, int* __restrict__ oid, int* __restrict__ opos, int* __restrict__ otype) {
  constexpr int NC = 4;
  __shared__ int s_q[CE_MAX_Q];
  __shared__ __attribute__((aligned(16))) u16 s_d[CE_MAX_L];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long b = blockIdx.x;
  const int m = (int)(b / P);
  const long r = rows[b];
  int ql, dl;
  ce_pair(r, n, qlen, m, dlen, L, max_pos, ql, dl);
  const int len = ql + dl + 3;
  const long row0 = cu[b];
  if (row0 < 0 || row0 + len > T) return;  // (never: cu is ce_lens_kernel's over the same inputs; block-uniform)

  if (tid < ql) s_q[tid] = qtok[(long)m * CE_MAX_Q + tid];
  if (dl > 0) {
    const u16* dr = tok + r * (long)L;
    if (vec) {
      if (tid * 8 < dl) *reinterpret_cast<u16x8*>(s_d + tid * 8) = *reinterpret_cast<const u16x8*>(dr + tid * 8);
    } else {
      if (tid < dl) s_d[tid] = dr[tid];
    }
  }
  __syncthreads();

  for (int p = wave; p < len; p += 4) {  // (wave-uniform)
    int id, type;
    if (p == 0) { id = cls_id; type = 0; }
    else if (p <= ql) { id = s_q[p - 1]; type = 0; }
    else if (p == ql + 1) { id = sep_id; type = 0; }
    else if (p < len - 1) { id = (int)s_d[p - ql - 2]; type = 1; }
    else { id = sep_id; type = 1; }
    id = min(max(id, 0), vocab - 1);
    const long t = row0 + p;
    if (lane == 0 && oid) { oid[t] = id; opos[t] = p; otype[t] = type; }
    float v[NC][4];
    float sum = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      int col = (lane + 64 * c) * 4;
      if (col < H) {
        u16x4 a = *reinterpret_cast<const u16x4*>(wemb + (long)id * H + col);
        u16x4 pe = *reinterpret_cast<const u16x4*>(pemb + (long)p * H + col);
        u16x4 ty = *reinterpret_cast<const u16x4*>(temb + (long)type * H + col);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          v[c][u] = bf16_to_f32(a[u]) + bf16_to_f32(pe[u]) + bf16_to_f32(ty[u]);
          sum += v[c][u];
        }
      } else {
#pragma unroll
        for (int u = 0; u < 4; ++u) v[c][u] = 0.f;
      }
    }
    const float mean = wave_sum(sum) / H;
    float var = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      int col = (lane + 64 * c) * 4;
      if (col < H)
#pragma unroll
        for (int u = 0; u < 4; ++u) { float d = v[c][u] - mean; var += d * d; }
    }
    const float rstd = rsqrtf(wave_sum(var) / H + eps);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      int col = (lane + 64 * c) * 4;
      if (col < H) {
        f32x4 gg = *reinterpret_cast<const f32x4*>(g + col);
        f32x4 bb = *reinterpret_cast<const f32x4*>(bta + col);
        u16x4 o;
#pragma unroll
        for (int u = 0; u < 4; ++u) o[u] = f32_to_bf16((v[c][u] - mean) * rstd * gg[u] + bb[u]);
        *reinterpret_cast<u16x4*>(Y + t * H + col) = o;
      }
    }
  }
}

// X: the pooler's dense output before its tanh, bf16 [M * P, H] with row stride ldx
__global__ __launch_bounds__(CE_HEAD_NT) void ce_head_select_kernel(
    const u16* __restrict__ X, long ldx, int H, const long* __restrict__ rows, int P, int n,
    const float* __restrict__ wc, const float* __restrict__ bc, int k, float* __restrict__ oscore,
    long* __restrict__ orow, float* __restrict__ ologit) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) float s_w[1024];
  __shared__ float s_logit[CE_MAX_P];
  const int tid = threadIdx.x, part = tid & 15, slot = tid >> 4;
  const long m = blockIdx.x;
  for (int d = tid; d < H; d += CE_HEAD_NT) s_w[d] = wc[d];
  __syncthreads();
  long r = -1;
  if (slot < P) {  // (uniform over the 16 lanes of a slot)
    r = rows[m * P + slot];
    if (r >= n) r = -1;
  }
  float dot = 0.f;
  if (slot < P) {
    const u16* x = X + (m * P + slot) * ldx;
    const int n4 = H >> 2;
    for (int d4 = part; d4 < n4; d4 += 16) {
      const u16x4 xv = *reinterpret_cast<const u16x4*>(x + 4 * d4);
      const float4 av = *reinterpret_cast<const float4*>(s_w + 4 * d4);
      dot = fmaf(av.x, tanhf(bf16_to_f32(xv[0])), dot);
      dot = fmaf(av.y, tanhf(bf16_to_f32(xv[1])), dot);
      dot = fmaf(av.z, tanhf(bf16_to_f32(xv[2])), dot);
      dot = fmaf(av.w, tanhf(bf16_to_f32(xv[3])), dot);
    }
  }
  dot = lzk_fold16(dot);  // (every wave is whole: CE_HEAD_NT threads whatever P)
  if (slot < P && part == 0) {
    const float lg = r >= 0 ? dot + bc[0] : LZK_NEG_INF;
    s_logit[slot] = lg;
    ologit[m * P + slot] = lg;
  }
  __syncthreads();
  if (tid < 64) {
    u64 key = 0ull;
    if (tid < P) {
      const long rr = rows[m * P + tid];
      if (rr >= 0 && rr < n) key = wide_key(s_logit[tid], (int)rr);
    }
    key = wave_sort_desc(key, tid);
    if (tid < k) {
      float v;
      int row;
      wide_unkey(key, v, row);
      oscore[m * k + tid] = v;
      orow[m * k + tid] = row;
    }
  }
}

}  // namespace

// lens int32 [B], cu int32 [B + 1], stat int32 [2] = (T, S_max) of the B = M * P pairs of rows int64 [M, P]
// (< 0 or >= n: empty); qlen int32 [M], dlen int32 [n]; L the column's width, max_pos the encoder's positions.
LZK_EXPORT int lzk_ce_lens(const long* rows, int M, int P, const int* qlen, const int* dlen, long n, int L,
                           int max_pos, int* lens, int* cu, int* stat, void* stream) {
  if (M < 1 || P < 1 || P > CE_MAX_P || (long)M * P > CE_MAX_B || n < 0 || n >= (1L << 31) - 1 || L < 1 ||
      L > CE_MAX_L || max_pos < 4)
    return (int)hipErrorInvalidValue;
  if (!rows || !qlen || (n > 0 && !dlen) || !lens || !cu || !stat) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(ce_lens_kernel, dim3(1), dim3(CE_SCAN_NT), 0, (hipStream_t)stream, rows, M * P, P, qlen, dlen,
                     (int)n, L, max_pos, lens, cu, stat);
  return (int)hipGetLastError();
}

// Y bf16 [T, H]: the embedded and normalised tokens of the B = M * P pairs, pair b at rows cu[b] ..; T =
// cu[B] as read back by the caller. qtok int32 [M, 64]; tok 16-bit ids [n, L]; the tables bf16 ([vocab, H],
// [max_pos, H], [2, H]), g / b fp32 [H]. oid / opos / otype: int32 [T] each, or all null.
LZK_EXPORT int lzk_ce_embed_ln(const long* rows, int M, int P, long n, const int* qtok, const int* qlen,
                               const void* tok, const int* dlen, int L, int max_pos, const int* cu, int T, int cls_id,
                               int sep_id, int vocab, const void* wemb, const void* pemb, const void* temb,
                               const float* g, const float* b, int H, float eps, void* Y, int* oid, int* opos,
                               int* otype, void* stream) {
  if (M < 1 || P < 1 || P > CE_MAX_P || (long)M * P > CE_MAX_B || n < 0 || n >= (1L << 31) - 1 || L < 1 ||
      L > CE_MAX_L || max_pos < 4 || T < 0 || vocab < 1 || H % 4 != 0 || H < 4 || H > 64 * 4 * 4)
    return (int)hipErrorInvalidValue;
  if (cls_id < 0 || cls_id >= vocab || sep_id < 0 || sep_id >= vocab) return (int)hipErrorInvalidValue;
  if (!rows || !qtok || !qlen || (n > 0 && (!tok || !dlen)) || !cu || !wemb || !pemb || !temb || !g || !b || !Y)
    return (int)hipErrorInvalidValue;
  if ((oid || opos || otype) && !(oid && opos && otype)) return (int)hipErrorInvalidValue;
  const int vec = (L % 8 == 0) && (((uintptr_t)tok & 15) == 0);
  hipLaunchKernelGGL(ce_embed_ln_kernel, dim3((unsigned)(M * P)), dim3(256), 0, (hipStream_t)stream, rows, P, (int)n,
                     qtok, qlen, (const u16*)tok, dlen, L, max_pos, cu, T, cls_id, sep_id, vocab, vec,
                     (const u16*)wemb, (const u16*)pemb, (const u16*)temb, g, b, H, eps, (u16*)Y, oid, opos, otype);
  return (int)hipGetLastError();
}

// scores fp32 / out_rows int64 [M, k] and logits fp32 [M, P] from the pooler's dense output X bf16 [M * P, H]
// (row stride ldx), the pool rows int64 [M, P], wc fp32 [H], bc fp32 [1]. 1 <= k <= P <= 64.
LZK_EXPORT int lzk_ce_head_select(const void* X, long ldx, int H, const long* rows, int M, int P, long n,
                                  const float* wc, const float* bc, int k, float* scores, long* out_rows,
                                  float* logits, void* stream) {
  if (M < 1 || P < 1 || P > CE_MAX_P || k < 1 || k > P || n < 0 || n >= (1L << 31) - 1 || H % 4 != 0 || H < 4 ||
      H > 1024 || ldx < H || ldx % 4 != 0 || (((uintptr_t)X & 7) != 0))
    return (int)hipErrorInvalidValue;
  if (!X || !rows || !wc || !bc || !scores || !out_rows || !logits) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(ce_head_select_kernel, dim3((unsigned)M), dim3(CE_HEAD_NT), 0, (hipStream_t)stream,
                     (const u16*)X, ldx, H, rows, P, (int)n, wc, bc, k, scores, out_rows, logits);
  return (int)hipGetLastError();
}
