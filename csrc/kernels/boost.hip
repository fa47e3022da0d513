// Boosted search: the per-row score prior of `boost=` written into a bias
// column (lazzaro_amd/ops/boost_ops.py holds the contract in full).
//
//   B(r)     = ((w_sal * sal + w_freq * min(1, acc / 10))
//               + w_rec * (1 / (1 + max(0, now - t) / scale))) + tw[type code]
//   prior(r) = (float)(c * B(r)), 0 when that is not finite
//   out[r]   = kind[r] == NODE ? base[r] + prior(r) : -inf
//
// B in fp64 in exactly this order with contraction off, so the torch
// formulation and the numpy oracle reproduce every bit. Every scan route takes
// `out` as its per-row bias as it is.
//
// One elementwise pass, memory-bound: 22 B read + 4 B written per row. A
// thread takes 4 consecutive rows with 16-byte loads (two for the fp64 clock
// column, one 4-byte load for each u8 column) and one 16-byte store when every
// pointer allows it (the launcher checks the alignment; a `base` that is a
// view one element into a buffer takes the 4-byte path), a capped grid strides
// over the row groups, and the last n % 4 rows go row by row.
#include "lzk_common.h"
#include "lzk_rowpred.h"

namespace {

constexpr int NTB = 256;
constexpr int RPT = 4;           // rows per thread and step
constexpr int MAX_BLOCKS = 2048; // 256 CUs x 8 blocks: enough in flight to cover HBM latency; the rest is strided

struct BoostTable {
  double w[256];  // weight per type code (by value: 2 KiB of kernel arguments, staged into LDS)
};

// BoostArgs and boost_row: lzk_rowpred.h

template <bool VEC, bool TYPES>
__global__ __launch_bounds__(NTB) void boost_bias_kernel(const float* __restrict__ base, const float* __restrict__ sal,
                                                         const int* __restrict__ acc, const double* __restrict__ t,
                                                         const unsigned char* __restrict__ kind,
                                                         const unsigned char* __restrict__ tcode, long n,
                                                         BoostArgs a, BoostTable tab, float* __restrict__ out) {
  __shared__ double tw_s[256];
  if (TYPES) {
    tw_s[threadIdx.x] = tab.w[threadIdx.x];  // (NTB == 256 entries)
    __syncthreads();
  }
  const long groups = (n + RPT - 1) / RPT;
  for (long g = (long)blockIdx.x * NTB + threadIdx.x; g < groups; g += (long)gridDim.x * NTB) {
    const long r0 = g * RPT;
    if (VEC && r0 + RPT <= n) {
      const float4 b4 = *reinterpret_cast<const float4*>(base + r0);
      const float4 s4 = *reinterpret_cast<const float4*>(sal + r0);
      const int4 a4 = *reinterpret_cast<const int4*>(acc + r0);
      const double2 t01 = *reinterpret_cast<const double2*>(t + r0);
      const double2 t23 = *reinterpret_cast<const double2*>(t + r0 + 2);
      const unsigned k4 = *reinterpret_cast<const unsigned*>(kind + r0);
      unsigned c4 = 0;
      if (TYPES) c4 = *reinterpret_cast<const unsigned*>(tcode + r0);
      float4 o;
      o.x = boost_row(b4.x, s4.x, a4.x, t01.x, k4 & 255u, TYPES ? tw_s[c4 & 255u] : 0.0, a);
      o.y = boost_row(b4.y, s4.y, a4.y, t01.y, (k4 >> 8) & 255u, TYPES ? tw_s[(c4 >> 8) & 255u] : 0.0, a);
      o.z = boost_row(b4.z, s4.z, a4.z, t23.x, (k4 >> 16) & 255u, TYPES ? tw_s[(c4 >> 16) & 255u] : 0.0, a);
      o.w = boost_row(b4.w, s4.w, a4.w, t23.y, k4 >> 24, TYPES ? tw_s[c4 >> 24] : 0.0, a);
      *reinterpret_cast<float4*>(out + r0) = o;
    } else {
      const long r1 = r0 + RPT < n ? r0 + RPT : n;
      for (long r = r0; r < r1; ++r)
        out[r] = boost_row(base[r], sal[r], acc[r], t[r], kind[r], TYPES ? tw_s[tcode[r]] : 0.0, a);
    }
  }
}

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

// out[r] = base[r] + prior(r) over rows [0, n) (see the head of this file).
// `t`: the clock column (last_accessed or timestamp). `tcode` / `tw` (256
// doubles on the host): the type-code column and its weight table, or both
// null. `c`: 2 for L2, 1 for IP and cosine.
LZK_EXPORT int lzk_tg_boost_bias(const float* base, const float* sal, const int* acc, const double* t,
                                 const unsigned char* kind, const unsigned char* tcode, const double* tw, long n,
                                 double w_sal, double w_freq, double w_rec, double scale, double now, double c,
                                 float* out, void* stream) {
  if (n <= 0) return 0;
  if ((tcode == nullptr) != (tw == nullptr)) return (int)hipErrorInvalidValue;
  BoostArgs a{w_sal, w_freq, w_rec, scale, now, c};
  BoostTable tab;
  if (tw != nullptr)
    for (int i = 0; i < 256; ++i) tab.w[i] = tw[i];
  else
    for (int i = 0; i < 256; ++i) tab.w[i] = 0.0;
  const bool vec = aligned(base, 16) && aligned(sal, 16) && aligned(acc, 16) && aligned(t, 16) && aligned(out, 16) &&
                   aligned(kind, 4) && (tcode == nullptr || aligned(tcode, 4));
  const long groups = (n + RPT - 1) / RPT;
  long nb = (groups + NTB - 1) / NTB;
  if (nb > MAX_BLOCKS) nb = MAX_BLOCKS;
  const dim3 grid((unsigned)nb), block(NTB);
  hipStream_t st = (hipStream_t)stream;
  if (vec) {
    if (tcode != nullptr)
      hipLaunchKernelGGL((boost_bias_kernel<true, true>), grid, block, 0, st, base, sal, acc, t, kind, tcode, n, a,
                         tab, out);
    else
      hipLaunchKernelGGL((boost_bias_kernel<true, false>), grid, block, 0, st, base, sal, acc, t, kind, tcode, n, a,
                         tab, out);
  } else {
    if (tcode != nullptr)
      hipLaunchKernelGGL((boost_bias_kernel<false, true>), grid, block, 0, st, base, sal, acc, t, kind, tcode, n, a,
                         tab, out);
    else
      hipLaunchKernelGGL((boost_bias_kernel<false, false>), grid, block, 0, st, base, sal, acc, t, kind, tcode, n, a,
                         tab, out);
  }
  return (int)hipGetLastError();
}
