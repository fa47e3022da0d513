"""fp64 references of the kernels the search routes start and finish with:
``store_rerank_kernel`` / ``store_rerank_block_kernel``, ``cos_rerank64_kernel``,
``tg_write_emb_kernel`` and ``row_cent_cos_kernel`` (csrc/kernels/tenant.hip),
``seg_sum_sorted_kernel`` / ``seg_sum_kernel`` / ``centroid_kernel`` and
``pairs_kernel`` (csrc/kernels/graph.hip). Plain numpy (and ``fractions`` /
``math.fsum`` where a value has to be exact); nothing here touches a GPU, torch
or the kernel library. tests/unit/test_rerank_ref_cpu.py checks this module on
its own, tests/kernels/test_rerank_write_stages_gpu.py holds the kernels
against it.

Order. (score descending, row ascending) -- ``order`` of _ivfpq_ref.py, a
stable lexsort, so equal (score, row) pairs (a row listed twice) keep their
slot order. Missing entries are ``(-inf, -1)``.

Exact grid. Rows and queries are integers in [-8, 8], biases integers: a
product is at most 64, every partial sum of at most 2048 of them an integer
below 2^24, ``|q|^2`` and ``|x|^2`` likewise, so ``l2`` and ``ip`` scores have
the bits of the fp64 value whatever the order of the additions. A cosine score
is not exact; its ties come from identical vectors at different rows, which
both kernels score with the same instruction sequence (a candidate's slot
changes which lanes work, not what they compute). The bf16 rows of the
centroid kernels are integers in [-8, 8] too: a sum of 1000 of them is exact
in fp32, and ``sum / count`` is one correctly rounded division.

Bounds. ``gamma(n) = n u / (1 - n u)``, u = 2^-24 (_ivfpq_ref.py's docstring:
Higham, Lemma 3.1): a result whose every term went through at most n roundings
is off by at most ``gamma(n) * sum |terms|``. The terms are magnitudes (``sum
|q_d x_d|``, ``|bias|``, ``|q|^2``), never the score itself, so a bound holds
under the cancellation of ``l2`` with q ~= x. Roundings, counted from the
kernel sources:

* store_rerank, wave kernel (M >= 64): a lane chains ceil(D / 4) fmas (float4
  route: D / 16 steps of 4; scalar route: one element in four), two shuffle
  adds join the four lanes: ``n_dot = ceil(D / 4) + 2``. Block kernel (M < 64):
  16 lanes per candidate, ceil(D / 16) fmas and four shuffle adds: ``n_dot =
  ceil(D / 16) + 4``. Epilogues: ``ip`` adds the bias (1): ``gamma(n_dot + 1)
  (A + |b|)``, A = sum |q_d x_d|. ``l2`` is ``2 acc + b - qq``: the doubling is
  exact, two more roundings (one if the compiler fuses the first), and ``qq``
  = |q|^2 is a chain of ceil(D / 64) fmas per lane, six shuffle adds and the
  subtraction: ``gamma(n_dot + 2) (2 A + |b|) + gamma(ceil(D / 64) + 7)
  |q|^2``. ``cosine`` is ``acc / sqrtf(sqn) + b``: sqrtf, the division and the
  add are correctly rounded (3): ``gamma(n_dot + 3) (A / |x| + |b|)`` with
  |x| = sqrt(sqn) in fp64 from the same fp32 ``sqn``.
* cos_rerank64: the same 4-lane layout in fp64, u = 2^-53: ceil(D / 4) fmas,
  two shuffle adds, the division (sqrt of the fp32 ``sqn`` in fp64 is the
  reference's own operation). The reference's dot is exact (``Fraction``),
  rounded once, and divided once: ``cos64_bound = (ceil(D / 4) + 5) 2^-53 A /
  |x|`` covers both sides.
* write_emb: nothing accumulates in fp32. ``emb32``, the bf16 copy, ``amax``,
  ``rs8 = fl32(amax * fl32(1 / 127))`` and ``emb8 = clamp(rint(fl32(vb /
  rs8)))`` are single correctly rounded operations: bit-exact. ``|x|^2`` is a
  sum of exact fp64 squares (an fp32 square has 48 bits) over a tree of 4 + 6
  + 3 fp64 additions, then one fp32 rounding: within half an fp32 ulp of the
  exact sum, times (1 + 2^-20) for the fp64 tree (13 * 2^-53 relative is a
  2^-20 share of half an fp32 ulp = 2^-25 relative). ``sumsq`` adds one exact
  fp64 square per row and dimension in any order: 2^-53 relative per added row,
  pinned at 1e-15. ``dv_max`` is ``fl32(|sqrt(s2) - 1|)`` from the fp64 tree
  sum: one fp32 ulp covers the tree's 2^-49 and the final rounding.
* seg_sum: the sorted kernel adds two rows, then the accumulator (2 roundings
  per 8 rows per wave), and joins four waves (2); the atomic kernel adds row by
  row; both stay below ``rows + 3``: ``gamma(rows + 3) sum |x|`` per element.
  centroid: one division by the count (``gamma(rows + 4) sum |x| / count`` for
  the mean) and, normalised, ``ss = sum v^2`` (a square, ceil(D / 64) chained
  adds, six shuffle adds), the hardware ``rsqrtf`` (1 ulp = 2 u) and two
  multiplies: the norm of a returned row is within ``unit_bound(D) =
  gamma(ceil(D / 64) + 12)`` of 1 (the root halves the count of ``ss``; the
  whole count is kept). The bf16 copy is the RNE of the returned fp32 value.
* pairs: bf16 products are exact in fp32; the MFMA accumulates D of them in an
  order the hardware chooses: ``gamma(D + 1) sum |x_i x_j|``.
* row_cent_cos: a lane adds four products per step (a product and at most
  three adds, fused or not), one accumulator add per step (ceil(D / 256)
  steps), six shuffle adds, sqrtf and the division: ``gamma(ceil(D / 256) +
  13) sum |x_d c_d| / |x|``. By Cauchy-Schwarz ``sum |x_d c_d| <= |x| |c|``, so
  for a unit centroid the error is at most ``gamma(ceil(D / 256) + 13) |c|
  (1 + 2^-24)`` (``sqn`` is |x|^2 rounded to fp32): ``cent_cos_unit_bound``.
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

from tests.kernels._cand_ref import grid_queries, grid_rows, to_bf16  # noqa: F401
from tests.kernels._ivfpq_ref import NEG_INF, U_FP32, gamma, order  # noqa: F401  (one definition for all modules)

U_FP64 = 2.0 ** -53
WAVE_MIN_M = 64  # lzk_store_rerank: M < 64 -> store_rerank_block_kernel
F32 = np.float32


def cdiv(a: int, b: int) -> int:
    return -(-a // b)


# ---------------------------------------------------------------- store_rerank
def rerank_n_dot(D: int, M: int) -> int:
    """Roundings a product of the dot sees in the kernel ``M`` queries select."""
    return cdiv(D, 4) + 2 if M >= WAVE_MIN_M else cdiv(D, 16) + 4


def rerank_scores(Q, X, sqn, bias, cand, metric: str):
    """fp64 scores [M, C] of the candidate rows (-inf where ``cand < 0`` or the
    bias is -inf) and their bounds for an M-query launch."""
    Q = np.asarray(Q, dtype=F32).astype(np.float64)
    cand = np.asarray(cand, dtype=np.int64)
    M, C = cand.shape
    D = Q.shape[1]
    rows = np.clip(cand, 0, None)
    Xc = np.asarray(X, dtype=F32)[rows, :D].astype(np.float64)  # [M, C, D]
    prod = Q[:, None, :] * Xc
    dot, A = prod.sum(2), np.abs(prod).sum(2)
    b = np.asarray(bias, dtype=F32).astype(np.float64)[rows]
    live = (cand >= 0) & (b != NEG_INF)
    bf = np.where(np.isfinite(b), b, 0.0)
    nd = rerank_n_dot(D, M)
    if metric == "l2":
        qq = (Q * Q).sum(1)[:, None]
        s = 2.0 * dot + bf - qq
        bound = gamma(nd + 2) * (2.0 * A + np.abs(bf)) + gamma(cdiv(D, 64) + 7) * qq
    elif metric == "cosine":
        nr = np.sqrt(np.asarray(sqn, dtype=F32).astype(np.float64)[rows])
        nr = np.where(nr > 0, nr, 1.0)
        s = dot / nr + bf
        bound = gamma(nd + 3) * (A / nr + np.abs(bf))
    elif metric in ("ip", "dot"):
        s = dot + bf
        bound = gamma(nd + 1) * (A + np.abs(bf))
    else:
        raise ValueError(metric)
    return np.where(live, s, NEG_INF), np.where(live, bound, 0.0)


def rerank_ref(Q, X, sqn, bias, cand, k: int, metric: str, kind=None):
    """(scores fp64 [M, k], rows int64 [M, k], bounds [M, k][, node rows]):
    the live candidates by (score desc, row asc, slot asc), padded with
    (-inf, -1); ``kind``: the rows whose kind is not 1 as -1 as well."""
    cand = np.asarray(cand, dtype=np.int64)
    S, B = rerank_scores(Q, X, sqn, bias, cand, metric)
    M = cand.shape[0]
    os_ = np.full((M, k), NEG_INF)
    oi = np.full((M, k), -1, dtype=np.int64)
    ob = np.zeros((M, k))
    for q in range(M):
        live = np.nonzero(S[q] != NEG_INF)[0]
        o = live[order(S[q][live], cand[q][live])][:k]
        os_[q, : len(o)], oi[q, : len(o)], ob[q, : len(o)] = S[q][o], cand[q][o], B[q][o]
    if kind is None:
        return os_, oi, ob
    kd = np.asarray(kind)
    return os_, oi, ob, np.where((oi >= 0) & (kd[np.clip(oi, 0, None)] == 1), oi, -1)


def decided_cuts(s: np.ndarray, b: np.ndarray) -> np.ndarray:
    """For scores in reference order with bounds b: cut[j] = every computed
    score of the entries [0, j] certainly exceeds every one of (j, n) --
    ``min_{i <= j} (s_i - b_i) > max_{i > j} (s_i + b_i)``, which is what
    "the adjacent gap exceeds the sum of the two bounds" has to mean once
    bounds differ from row to row. bool [n - 1]."""
    if len(s) < 2:
        return np.zeros(0, dtype=bool)
    lo = np.minimum.accumulate(s - b)
    hi = np.maximum.accumulate((s + b)[::-1])[::-1]
    return lo[:-1] > hi[1:]


def check_ranked(got_s, got_r, S, B, cand, k: int):
    """Assert one query's kernel output (scores, rows: [k]) against the fp64
    scores / bounds / rows of its candidate list: every score within its
    bound of the fp64 score of the row returned, the rows between two decided
    cuts equal to the reference's as a multiset (a single row: that row),
    padding past the live count. Returns (undecided, adjacent) pair counts
    and the largest |error| / bound."""
    live = np.nonzero(S != NEG_INF)[0]
    o = live[order(S[live], cand[live])]
    s, b, r = S[o], B[o], cand[o]
    n = min(k, len(o))
    got_s, got_r = np.asarray(got_s, dtype=np.float64), np.asarray(got_r, dtype=np.int64)
    assert np.array_equal(got_r[n:], np.full(k - n, -1)) and np.all(got_s[n:] == NEG_INF), (got_r, got_s, n)
    # whatever the inputs, the output is sorted by its own (score desc, row asc)
    for j in range(1, n):
        assert got_s[j - 1] > got_s[j] or (got_s[j - 1] == got_s[j] and got_r[j - 1] <= got_r[j]), (j, got_s, got_r)
    cuts = decided_cuts(s, b)
    start, worst = 0, 0.0
    for j in range(len(o)):
        if j == len(o) - 1 or cuts[j]:
            lo, hi = start, min(j + 1, n)
            if lo < hi:
                want = sorted(r[start: j + 1].tolist())
                have = sorted(got_r[lo:hi].tolist())
                if j + 1 <= n:
                    assert have == want, (lo, hi, have, want)
                else:  # the block straddles k: what came back is drawn from it
                    pool = list(want)
                    for x in have:
                        assert x in pool, (lo, hi, have, want)
                        pool.remove(x)
            start = j + 1
    for j in range(n):
        c = np.nonzero((cand == got_r[j]) & (S != NEG_INF))[0]
        assert len(c), (j, got_r[j])
        err = abs(got_s[j] - S[c[0]])
        assert err <= B[c[0]], (j, got_r[j], got_s[j], S[c[0]], B[c[0]])
        if B[c[0]] > 0:
            worst = max(worst, err / B[c[0]])
    return int((~cuts).sum()), len(cuts), worst


# ---------------------------------------------------------------- cos_rerank64
def cos_rerank64_ref(Qn, X, sqn, cand, k: int):
    """(scores fp64 [M, k], rows [M, k], bounds [M, k]): the exact dot of the
    fp64 query and the fp32 row (``Fraction``), rounded once, over sqrt of the
    fp32 ``sqn`` in fp64 (1 where it is 0); every ``cand >= 0`` is live,
    duplicates keep slot order."""
    Qn = np.asarray(Qn, dtype=np.float64)
    X = np.asarray(X, dtype=F32)
    cand = np.asarray(cand, dtype=np.int64)
    M, C = cand.shape
    D = Qn.shape[1]
    S = np.full((M, C), NEG_INF)
    B = np.zeros((M, C))
    for q in range(M):
        fq = [Fraction(float(v)) for v in Qn[q]]
        memo = {}
        for c in range(C):
            r = int(cand[q, c])
            if r < 0:
                continue
            if r not in memo:
                fx = [Fraction(float(v)) for v in X[r, :D]]
                dot = sum((a * b for a, b in zip(fq, fx)), Fraction(0))
                A = sum((abs(a * b) for a, b in zip(fq, fx)), Fraction(0))
                nr = math.sqrt(float(sqn[r]))
                nr = nr if nr > 0.0 else 1.0
                memo[r] = (float(dot) / nr, (cdiv(D, 4) + 5) * U_FP64 * float(A) * (1.0 + 2.0 ** -50) / nr)
            S[q, c], B[q, c] = memo[r]
    os_ = np.full((M, k), NEG_INF)
    oi = np.full((M, k), -1, dtype=np.int64)
    ob = np.zeros((M, k))
    for q in range(M):
        live = np.nonzero(cand[q] >= 0)[0]
        o = live[order(S[q][live], cand[q][live])][:k]
        os_[q, : len(o)], oi[q, : len(o)], ob[q, : len(o)] = S[q][o], cand[q][o], B[q][o]
    return os_, oi, ob


# ---------------------------------------------------------------- write_emb
def bf16_bits(x) -> np.ndarray:
    """uint16 bf16 of fp32 values: round to nearest even on the integer bits
    (finite inputs; denormals and signed zeros go through unchanged)."""
    u = np.asarray(x, dtype=F32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_value(bits) -> np.ndarray:
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(F32)


INV127 = F32(1.0) / F32(127.0)


def quantize_def(vb):
    """The int8 quantiser's definition on fp32 rows ``vb`` [m, D]: ``rs8 =
    fl32(amax * fl32(1 / 127))`` (0 for a zero row), ``emb8 = clamp(rint(fl32(vb
    / rs8)), +-127)`` -- numpy float32 operations, each correctly rounded, rint
    to even. Returns (int8 [m, D], fp32 [m])."""
    vb = np.asarray(vb, dtype=F32)
    amax = np.abs(vb).max(1) if vb.shape[1] else np.zeros(len(vb), dtype=F32)
    rs = np.where(amax > 0, (amax * INV127).astype(F32), F32(0.0)).astype(F32)
    den = np.where(amax > 0, rs, F32(1.0)).astype(F32)
    with np.errstate(over="ignore"):
        qf = (vb / den[:, None]).astype(F32)
    q = np.clip(np.rint(qf), -127, 127).astype(np.int8)
    return q, rs


def write_emb_ref(x, has=None):
    """The embedding columns of rows ``x`` fp32 [m, D] by definition. dict:
    emb32 fp32 [m, D] (= x * has, signs of zero included), emb16 uint16 bits,
    emb8 int8, rs8 fp32 [m], has_emb uint8 [m], s2 (exact sum of squares,
    fp64 correctly rounded) and sqn = fl32(s2) [m], sumsq_inc fp64 [D] (this
    call's per-dimension increment), rs_max (over the non-zero rows, 0 if
    none) and dv_max = max fl32(|sqrt(s2) - 1|) over the ``has`` rows (0 if
    none)."""
    x = np.asarray(x, dtype=F32)
    m, D = x.shape
    hv = np.ones(m, dtype=F32) if has is None else (np.asarray(has) != 0).astype(F32)
    e32 = (x * hv[:, None]).astype(F32)
    b16 = bf16_bits(e32)
    vb = bf16_value(b16)
    q, rs = quantize_def(vb)
    sq = e32.astype(np.float64) ** 2  # exact: 24-bit significands
    s2 = np.array([math.fsum(row) for row in sq])
    inc = np.array([math.fsum(sq[:, d]) for d in range(D)])
    nz = rs > 0
    dv = np.abs(np.sqrt(s2) - 1.0).astype(F32)
    return {"emb32": e32, "emb16": b16, "emb8": q, "rs8": rs, "has_emb": (hv > 0).astype(np.uint8), "s2": s2,
            "sqn": s2.astype(F32), "sumsq_inc": inc, "rs_max": F32(rs[nz].max()) if nz.any() else F32(0.0),
            "dv_max": F32(dv[hv > 0].max()) if (hv > 0).any() else F32(0.0)}


def sqn_tol(s2) -> np.ndarray:
    """Half an fp32 ulp at the exact sum, with the 2^-20 allowance."""
    return 0.5 * np.spacing(np.asarray(s2, dtype=np.float64).astype(F32)).astype(np.float64) * (1.0 + 2.0 ** -20)


def planted_rows(D: int, rng) -> np.ndarray:
    """fp32 rows [9, D] that sit on the quantisers' edges (D >= 4): 0 bf16 ties
    to an even and 1 to an odd significand (both signs); 2 and 3 a row whose
    maximum is +-127 * 2^-7 so ``vb / rs8`` lands on .5 exactly where planted
    (k + 1/2 for even and odd k); 4 / 5 the maximum element alone at either
    sign among small ones; 6 denormals (fp32 denormal inputs, one bf16
    denormal maximum); 7 a row of -0.0 and +0.0; 8 Gaussian, scaled to a
    maximum of 1 (``error_cap_rows`` says why)."""
    R = np.zeros((9, D), dtype=F32)

    def bits(u):
        return np.array(u, dtype=np.uint32).view(F32)

    # bf16 ties: low 16 bits exactly 0x8000; kept significand bit even (..40) or odd (..41)
    tie = bits([0x3F408000, 0x3F418000, 0xBF408000, 0xBF418000, 0x3F407FFF, 0x3F408001])
    R[0] = np.resize(tie, D)
    R[1] = np.resize(tie[::-1] * F32(0.25), D)
    # fl32(1 / 127) = 2^-7 (1 + 2^-7 + 2^-14 + 2^-21), and 127 times that is 128 (1 - 2^-28), which rounds to
    # 128: amax = 127 * 2^-7 gives rs8 = 2^-7 exactly, so vb = j * 2^-8 (bf16-exact for j <= 255) has the
    # quotient j / 2 -- k + 1/2 for every odd j, with k = 0, 1, 2, 3 and 126 here
    half = np.array([j * 2.0 ** -8 for j in (1, 3, 5, 7, -1, -3, -5, -7, 253, -253)], dtype=F32)
    R[2] = np.resize(half, D)
    R[2, 0] = F32(127.0 * 2.0 ** -7)
    R[3] = -R[2]
    small = (rng.standard_normal(D) * 0.01).astype(F32)
    R[4] = small
    R[4, D - 1] = F32(0.75)
    R[5] = small
    R[5, 1] = F32(-0.75)
    den = bits([0x00000001, 0x00008000, 0x00018000, 0x80008000, 0x007FFFFF, 0x00400000])
    R[6] = np.resize(den, D)
    R[7] = np.resize(np.array([-0.0, 0.0], dtype=F32), D)
    g = rng.standard_normal(D)
    R[8] = (g / np.abs(g).max()).astype(F32)
    return R


ERR_CAP = 1.0 + 2.0 ** -22  # |vb - emb8 rs8| <= rs8 / 2 * ERR_CAP: holds where rs8 <= amax / 127 (see below)
ERR_CAP_ANY = 1.0 + 2.0 ** -17  # ... for any row: rint sees fl32(vb / rs8), off by half an ulp below 128 = 2^-18


def error_cap_rows(D: int) -> np.ndarray:
    """The rows the ERR_CAP property is asserted on: the planted rows and 28
    Gaussian rows scaled to a maximum of exactly 1. fl32(1 / 127) is below
    1 / 127, so with amax = 1 the stored scale is too, and a tie k + 1/2 that
    rounds away from vb still lands within rs8 / 2. An arbitrary maximum does
    not give that: fl32(amax * fl32(1 / 127)) exceeds amax / 127 for 45 of the
    128 bf16 significands (150 is one), and there vb = amax / 2 has the
    quotient 63.5 (1 - 2^-25.8), computed as 63.5, rounded to the even 64:
    an error of rs8 / 2 (1 + 2^-18.1)."""
    rng = np.random.default_rng(17 + D)
    x = rng.standard_normal((28, D))
    return np.concatenate([planted_rows(D, rng), (x / np.abs(x).max(1, keepdims=True)).astype(F32)]).astype(F32)


def quant_error(vb, q, rs) -> np.ndarray:
    """|vb - q rs| / (rs / 2) in fp64, 0 for zero rows."""
    rs = np.asarray(rs, dtype=np.float64)[:, None]
    err = np.abs(np.asarray(vb, dtype=np.float64) - np.asarray(q, dtype=np.float64) * rs)
    return np.where(rs > 0, err / np.where(rs > 0, rs / 2, 1.0), err)


# ---------------------------------------------------------------- seg_sum / centroids
def seg_sum_ref(X16, label, C: int):
    """fp64 per-cluster sums [C, D] of bf16-valued rows (labels < 0 skipped),
    counts int64 [C], and the per-element bound ``gamma(rows + 3) sum |x|``."""
    X = np.asarray(X16, dtype=np.float64)
    lab = np.asarray(label, dtype=np.int64)
    D = X.shape[1]
    sums, mag = np.zeros((C, D)), np.zeros((C, D))
    cnt = np.zeros(C, dtype=np.int64)
    for c in range(C):
        rows = X[lab == c]
        cnt[c] = len(rows)
        sums[c] = rows.sum(0) if len(rows) else 0.0
        mag[c] = np.abs(rows).sum(0) if len(rows) else 0.0
    bound = np.array([gamma(int(n) + 3) for n in cnt])[:, None] * mag
    return sums, cnt, bound


def unit_bound(D: int) -> float:
    return gamma(cdiv(D, 64) + 12)


def centroid_ref(X16, label, C: int, normalize: bool = True, eta: float = None):
    """(c fp64 [C, D], per-element bound, counts): mean = sum / max(1, count)
    with bound ``gamma(rows + 4) sum |x| / count``; normalised: mean / |mean|
    (a zero mean stays zero) with the bound propagated through the norm --
    with e the mean's bound, lo = |mean| - |e| and eta = unit_bound(D) (or the caller's, for another tier):
    ``(e_d / lo) (1 + eta) + |m_d| (|e| / (lo |mean|) + eta / lo)``, inf where
    lo <= 0 (a mean that cancels to within its own error has no direction)."""
    sums, cnt, _ = seg_sum_ref(X16, label, C)
    X = np.asarray(X16, dtype=np.float64)
    lab = np.asarray(label, dtype=np.int64)
    den = np.maximum(cnt, 1)[:, None].astype(np.float64)
    mean = sums / den
    mag = np.stack([np.abs(X[lab == c]).sum(0) if cnt[c] else np.zeros(X.shape[1]) for c in range(C)])
    e = np.array([gamma(int(n) + 4) for n in cnt])[:, None] * mag / den
    if not normalize:
        return mean, e, cnt
    D = X.shape[1]
    nrm = np.sqrt((mean * mean).sum(1))
    en = np.sqrt((e * e).sum(1))
    lo = nrm - en
    eta = unit_bound(D) if eta is None else eta
    out, bound = np.zeros_like(mean), np.zeros_like(mean)
    for c in range(C):
        if nrm[c] == 0.0:
            continue
        out[c] = mean[c] / nrm[c]
        if lo[c] <= 0.0:
            bound[c] = np.inf
        else:
            bound[c] = (e[c] / lo[c]) * (1.0 + eta) + np.abs(mean[c]) * (en[c] / (lo[c] * nrm[c]) + eta / lo[c])
    return out, bound, cnt


def centroid_bf16_ref(c32, pad_to: int) -> np.ndarray:
    """uint16 [C, pad_to]: the RNE bf16 bits of the fp32 centroids, zero padded."""
    c32 = np.asarray(c32, dtype=F32)
    out = np.zeros((c32.shape[0], pad_to), dtype=np.uint16)
    out[:, : c32.shape[1]] = bf16_bits(c32)
    return out


def cluster_labels(rng, sizes, n_dead: int = 0) -> np.ndarray:
    """Shuffled int32 labels: ``sizes[c]`` rows of cluster c, ``n_dead`` of -1."""
    lab = np.concatenate([np.full(s, c, dtype=np.int32) for c, s in enumerate(sizes)]
                         + [np.full(n_dead, -1, dtype=np.int32)])
    rng.shuffle(lab)
    return lab


# ---------------------------------------------------------------- pairs
def pairs_ref(X16, tau: float):
    """Three sets of (i, j), i < j, over bf16-valued rows: certainly above
    (``dot - bound > tau``), certainly below (``dot + bound <= tau``) -- the
    kernel's compare is a strict ``>`` -- and the band between them, with bound
    ``gamma(D + 1) sum_d |x_id x_jd|``."""
    X = np.asarray(X16, dtype=np.float64)
    n, D = X.shape
    S = X @ X.T
    B = gamma(D + 1) * (np.abs(X) @ np.abs(X).T)
    t = float(F32(tau))  # the kernel compares with the fp32 threshold
    iu = np.triu_indices(n, 1)
    s, b = S[iu], B[iu]
    pairs = np.stack(iu, 1)
    above, below = s - b > t, s + b <= t
    as_set = lambda m: {(int(i), int(j)) for i, j in pairs[m]}  # noqa: E731
    return as_set(above), as_set(below), as_set(~above & ~below)


PAIR_TAU = 0.95
PAIR_PLANTS = ((5, 100), (3, 130), (127, 128), (200, 256), (0, 1), (60, 61))  # in a tile, across tiles, on the edge


def pair_rows(n: int, D: int, rng) -> np.ndarray:
    """bf16-valued unit rows [n, D]: Gaussian directions (dots ~ 1 / sqrt(D),
    far below PAIR_TAU), the PAIR_PLANTS copies (dot ~ 1), and for n > 126 a
    near copy on either side of the threshold, well clear of it: rows (10, 70)
    at cos ~ 0.98 and (11, 126) at ~ 0.90."""
    X = rng.standard_normal((n, D))
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    for a, b in PAIR_PLANTS:
        if b < n:
            X[b] = X[a]
    if n > 126:
        for a, b, eps in ((10, 70, 0.2), (11, 126, 0.48)):
            z = rng.standard_normal(D)
            z -= (z @ X[a]) * X[a]
            v = X[a] + eps * z / np.linalg.norm(z)
            X[b] = v / np.linalg.norm(v)
    return to_bf16(X)


# ---------------------------------------------------------------- row_cent_cos
def cent_cos_roundings(D: int) -> int:
    return cdiv(D, 256) + 13


def cent_cos_unit_bound(D: int, cnorm: float = 1.0 + 2.0 ** -20) -> float:
    """The bound for any row against a centroid of norm at most ``cnorm``."""
    return gamma(cent_cos_roundings(D)) * cnorm * (1.0 + U_FP32)


def row_cent_cos_ref(X, D: int, sqn, rows, lab, C):
    """fp64 cos of ``X[rows[i], :D]`` with ``C[lab[i]]`` over sqrt of the fp32
    ``sqn`` (-1 where it is 0), and the bound ``gamma(ceil(D / 256) + 13) sum
    |x_d c_d| / |x|``."""
    X = np.asarray(X, dtype=F32)[np.asarray(rows), :D].astype(np.float64)
    Cc = np.asarray(C, dtype=F32)[np.asarray(lab), :D].astype(np.float64)
    n2 = np.asarray(sqn, dtype=F32).astype(np.float64)[np.asarray(rows)]
    ok = n2 > 0
    nr = np.sqrt(np.where(ok, n2, 1.0))
    cos = np.where(ok, (X * Cc).sum(1) / nr, -1.0)
    bound = np.where(ok, gamma(cent_cos_roundings(D)) * np.abs(X * Cc).sum(1) / nr, 0.0)
    return cos, bound


# ---------------------------------------------------------------- shared store_rerank cases
RERANK_MS = (1, 3, 63, 64, 65, 130)  # < 64: the block kernel, >= 64: the wave kernel
RERANK_CS = (1, 15, 16, 17, 33, 63, 64)
RERANK_DS = (4, 20, 48, 64, 100, 384, 1024)
RERANK_N = 300  # stored rows of every case
# (C, D, k code, extra row stride): every C and every D twice, every k code (0: 1, 1: 10, 2: C, 3: C + 3) and the
# three layouts (0 contiguous, 4 a padded stride the float4 route keeps, 3 one that forces the scalar route)
RERANK_COMBOS = tuple((RERANK_CS[i], RERANK_DS[(i + s) % 7], (i + s) % 4, (0, 4, 3)[(i + 2 * s) % 3])
                      for s in (0, 3) for i in range(7))
# Gaussian: wide rows get few candidates (their bounds are the widest, so their gaps must be)
GAUSS_COMBOS = ((64, 20, 1, 0), (33, 100, 2, 3), (63, 48, 3, 4), (17, 384, 1, 0), (16, 1024, 2, 4), (15, 64, 0, 3),
                (1, 4, 3, 0))
UNDECIDED_CAP = 0.01


def k_of(code: int, C: int) -> int:
    return (1, 10, C, C + 3)[code]


def rerank_inputs(kind: str, metric: str, M: int, C: int, D: int, pad: int, seed: int):
    """One store_rerank case: dict with Q fp32 [M, D], X fp32 [N, D + pad]
    (the kernel reads the view ``X[:, :D]``; the padding columns hold 1e30 so a
    read past D cannot go unnoticed), sqn, bias fp32 [N], cand int64 [M, C].
    ``kind`` "grid": integers in [-8, 8], integer biases, duplicate rows and,
    under cosine, their ties; "gauss": Gaussian rows, a third of the ``l2``
    queries a stored row plus a little noise. About one row in ten is
    tombstoned (-inf bias), about one candidate slot in ten is -1, and each
    query lists distinct rows, the planted copies among them."""
    rng = np.random.default_rng(seed)
    N = RERANK_N
    if kind == "grid":
        X = grid_rows(rng, N, D, dup=6)
        Q = grid_queries(rng, M, D)
    else:
        X = rng.standard_normal((N, D))
        for j in range(6):  # the same copies as the grid: exact ties under every metric
            X[N - 1 - 3 * j] = X[2 * j]
        Q = rng.standard_normal((M, D))
        if metric == "l2":
            for q in range(0, M, 3):
                Q[q] = X[(7 * q + 1) % N] + 1e-3 * rng.standard_normal(D)
    X = X.astype(F32)
    Q = Q.astype(F32)
    s2 = (X.astype(np.float64) ** 2).sum(1)
    sqn = s2.astype(F32)
    if metric == "l2":
        bias = -sqn.astype(np.float64)
    elif kind == "grid":
        bias = rng.integers(-4, 5, size=N).astype(np.float64)
    else:
        bias = 0.1 * rng.standard_normal(N) if metric == "ip" else np.zeros(N)
    for j in range(6):  # copies share the bias: ties on the row alone
        bias[N - 1 - 3 * j] = bias[2 * j]
    dead = rng.random(N) < 0.1
    dead[:12] = False
    dead[N - 16:] = False
    bias[dead] = NEG_INF
    cand = np.empty((M, C), dtype=np.int64)
    for q in range(M):
        j = q % 6
        head = [N - 1 - 3 * j, 2 * j][: min(C, 2)]  # the larger row first: slot order must not decide
        rest = np.setdiff1d(rng.permutation(N), head, assume_unique=False)
        rest = rng.permutation(rest)[: C - len(head)]
        cand[q] = rng.permutation(np.concatenate([head, rest]).astype(np.int64)) if q % 2 else \
            np.concatenate([head, rest]).astype(np.int64)
        if C > 3:
            cand[q, rng.random(C) < 0.1] = -1
    Xw = np.full((N, D + pad), 1e30, dtype=F32)
    Xw[:, :D] = X
    return {"Q": Q, "X": Xw, "D": D, "sqn": sqn, "bias": bias.astype(F32), "cand": cand}


def rerank_undecided(case, metric: str):
    """(undecided, adjacent) pair counts of a case by the reference alone."""
    S, B = rerank_scores(case["Q"], case["X"], case["sqn"], case["bias"], case["cand"], metric)
    und = tot = 0
    for q in range(len(S)):
        live = np.nonzero(S[q] != NEG_INF)[0]
        o = live[order(S[q][live], case["cand"][q][live])]
        cuts = decided_cuts(S[q][o], B[q][o])
        # the planted copies tie exactly and are not counted: their order is the row's, checked bit for bit
        tie = (S[q][o][:-1] == S[q][o][1:]) if len(o) > 1 else np.zeros(0, dtype=bool)
        und += int((~cuts & ~tie).sum())
        tot += len(cuts)
    return und, tot
