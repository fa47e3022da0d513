"""fp64 references of the certified int8 store search's stages
(csrc/kernels/search256.hip, csrc/kernels/scan8.hip; driven by ops/search.py
``flat_topk_i8`` / ``_rescore_above_cut`` / ``_select_with_fallback``):
``thr_prep_kernel``, the int8 scans' score, ``cand_gather_kernel``,
``cand_select_kernel`` / ``cand_select_block_kernel``, ``cand_cut_kernel`` /
``cand_cut_block_kernel``, ``cand_rescore_kernel`` / ``cand_rescore4_kernel``
and the worst-case margin of ``i8_query_kernel``. Plain numpy; nothing here
touches a GPU or the kernel library. tests/unit/test_cand_ref_cpu.py checks this
module on its own, tests/kernels/test_cand_stages_gpu.py,
test_scan8_narrow_records_gpu.py and test_i8_certified_path_gpu.py hold the
kernels against it.

Order. (score descending, row ascending) -- the kernels' ``better()`` --
missing entries ``(-inf, -1)``: ``order`` of _ivfpq_ref.py.

Exact grid. Rows and queries are integers in [-8, 8] (exact in bf16, fp32 and
int8), alpha and the int8 scales are powers of two, biases are integers: a
product is at most 64 and every partial sum of at most 2048 of them -- fma
chain, shuffle tree, any order -- is an integer below 2048 * 64 < 2^24, so a
correct kernel returns the bits of the fp64 value. The builders plant duplicate
rows, so exact ties exist.

Gaussian inputs, the bound. ``gamma(n) = n u / (1 - n u)``, u = 2^-24 (see
_ivfpq_ref.py's docstring: Higham, Lemma 3.1): summing n - 1 terms in any order
is off by at most ``gamma(n) * sum |terms|``. A re-scored entry is
``alpha * sum_d q_d x_d + bias``: D accumulated products, the multiply by alpha
and the bias add, hence ``score_bound = gamma(D + 3) (|alpha| sum |q_d x_d| +
|bias|)``.
"""
from __future__ import annotations

import numpy as np

from tests.kernels._ivfpq_ref import NEG_INF, U_FP32, gamma, order  # noqa: F401  (one definition for both modules)

FLT_MAX = float(np.finfo(np.float32).max)
CNT_MASK = 0x3FFFFFFF  # a list count's low 30 bits; bit 30 = "a record region overflowed"
CNT_OVF = 0x40000000
C_2E4 = float(np.float32(2e-4))  # the kernels' fp32 constants, as fp64 values
C_1E6 = float(np.float32(1e-6))


# ---------------------------------------------------------------- input builders
def grid_rows(rng, n: int, D: int, dup: int = 6) -> np.ndarray:
    """[n, D] integers in [-8, 8] (fp64); up to ``dup`` rows are copies of
    earlier ones (row n - 1 - 3 j = row 2 j), so exact score ties exist."""
    X = rng.integers(-8, 9, size=(n, D)).astype(np.float64)
    for j in range(dup):
        a, b = 2 * j, n - 1 - 3 * j
        if 0 <= a < b < n:
            X[b] = X[a]
    return X


def grid_queries(rng, nq: int, D: int) -> np.ndarray:
    return rng.integers(-8, 9, size=(nq, D)).astype(np.float64)


def grid_scales(rng, n: int) -> np.ndarray:
    """Powers of two in {1/4, 1/2, 1} (fp32): int8 row / query scales."""
    return (2.0 ** rng.integers(-2, 1, size=n)).astype(np.float32)


def unit_rows(rng, n: int, D: int, norm: float = 1.0) -> np.ndarray:
    X = rng.standard_normal((n, D))
    return X * (norm / np.linalg.norm(X, axis=1, keepdims=True))


def to_bf16(x: np.ndarray) -> np.ndarray:
    """Round-to-nearest-even bf16 of finite fp32-range values, as fp64."""
    u = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32).astype(np.float64)


# ---------------------------------------------------------------- thresholds
def thr_prep_ref(ts, col: int, margin=None, margin_rig=None):
    """``lzk_thr_prep``: the fp32 chain, rounded op by op (the kernel is built
    with contraction off): tau = t - 2e-4 (1 + |t|), nan -> -inf, +-inf ->
    +-FLT_MAX; thr = tau - margin; cert = thr + margin_rig, + 1e-6 (1 + |.|),
    nan / -inf -> -inf, +inf -> FLT_MAX. Returns (thr, cert) fp32 [nq]."""
    f = np.float32
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.asarray(ts, dtype=f)[:, col].copy()
        t = (t - (f(2e-4) * (f(1.0) + np.abs(t))).astype(f)).astype(f)
        t = np.where(np.isnan(t), f(NEG_INF), np.where(t == f(NEG_INF), f(-FLT_MAX), np.where(t == f(np.inf), f(FLT_MAX), t)))
        t = t.astype(f)
        th = (t - np.asarray(margin, dtype=f)).astype(f) if margin is not None else t
        c = (th + np.asarray(margin_rig, dtype=f)).astype(f) if margin_rig is not None else th
        c = (c + (f(1e-6) * (f(1.0) + np.abs(c))).astype(f)).astype(f)
        c = np.where(np.isnan(c), f(NEG_INF), np.where(c == f(np.inf), f(FLT_MAX), c)).astype(f)
    return th, c


# ---------------------------------------------------------------- int8 scan
def i8_scores(X8, rs, Q8, qs, bias, alpha: float) -> np.ndarray:
    """fp64 ``alpha qs[q] (rs[r] <q8[q], x8[r]>) + bias[r]``, [nq, nrows]."""
    Qd = np.asarray(Q8, dtype=np.float64)
    v = np.empty((Qd.shape[0], len(X8)))
    for r0 in range(0, len(X8), 16384):  # (row blocks: the fp64 copy of a long int8 matrix stays small)
        v[:, r0: r0 + 16384] = Qd @ np.asarray(X8[r0: r0 + 16384], dtype=np.float64).T
    s = float(alpha) * np.asarray(qs, dtype=np.float64)[:, None] * (v * np.asarray(rs, dtype=np.float64)[None, :])
    if bias is not None:
        with np.errstate(invalid="ignore"):
            s = s + np.asarray(bias, dtype=np.float64)[None, :]
    return s


def i8_magnitude(X8, rs, Q8, qs, bias, alpha: float) -> np.ndarray:
    """|alpha qs rs <q8, x8>| + |bias| (0 where the bias is not finite)."""
    m = np.abs(i8_scores(X8, rs, Q8, qs, None, alpha))
    if bias is not None:
        b = np.asarray(bias, dtype=np.float64)
        m = m + np.where(np.isfinite(b), np.abs(b), 0.0)[None, :]
    return m


def quantize_i8_ref(x):
    """ops.search.quantize_i8_rows in numpy fp32: (q8 int8 [n, D], s fp32 [n])."""
    xf = np.asarray(x, dtype=np.float32)
    amax = np.abs(xf).max(1)
    s = np.where(amax > 0, (amax / np.float32(127.0)).astype(np.float32), np.float32(0.0)).astype(np.float32)
    den = np.where(amax > 0, s, np.float32(1.0)).astype(np.float32)
    q = np.clip(np.rint((xf / den[:, None]).astype(np.float32)), -127, 127).astype(np.int8)
    return q, s


def margin_rig_ref(q16, d: int, smax: float, alpha: float, xn: float, q8=None, qs=None) -> np.ndarray:
    """The worst-case |int8 score - bf16 score| of TenantGraph._i8_query, fp64:
    ``(|alpha| (|eta| xn + smax / 2 sum|q| + smax / 2 sum|eta| + d 2^-23 xn |q|))
    (1 + 1e-5) + 1e-6`` with eta = q8 qs - q. ``q16`` [nq, Dp] holds the bf16
    queries' values; (q8, qs) default to :func:`quantize_i8_ref` of them."""
    q = np.asarray(q16, dtype=np.float64)
    if q8 is None:
        q8, qs = quantize_i8_ref(q)
    eta = np.asarray(q8, dtype=np.float64) * np.asarray(qs, dtype=np.float64)[:, None] - q
    smax = float(smax)
    fl = 0.5 * smax * np.abs(eta).sum(1)
    bound = (np.linalg.norm(eta[:, :d], axis=1) * xn + 0.5 * smax * np.abs(q).sum(1) + fl
             + d * 2.0 ** -23 * xn * np.linalg.norm(q, axis=1))
    return abs(float(alpha)) * bound * (1.0 + 1e-5) + 1e-6


# ---------------------------------------------------------------- gather
def gather_ref(recs, bcnt, bcap: int, nq: int, dual: bool):
    """``lzk_cand_gather``: ``recs`` [regions, bcap, 4] int32 (query, row,
    score bits, lists mask), ``bcnt`` [regions]. Per list (1 or 2) returns
    (count [nq] int64 -- the true total, bit 30 set for every query when some
    region's count exceeds bcap -- and per query the filed (row, score bits)
    pairs, sorted). Only the first min(bcnt, bcap) records of a region are read."""
    out = []
    flag = CNT_OVF if any(int(c) > bcap for c in bcnt) else 0
    for bit in ((1, 2) if dual else (1,)):
        filed = [[] for _ in range(nq)]
        for b in range(len(bcnt)):
            for e in range(min(int(bcnt[b]), bcap)):
                qq, r, sb, m = (int(v) for v in recs[b, e])
                if 0 <= qq < nq and (m & bit):
                    filed[qq].append((r, sb))
        out.append((np.array([len(f) | flag for f in filed], dtype=np.int64), [sorted(f) for f in filed]))
    return out


# ---------------------------------------------------------------- select
def select_ref(cnt, cs, ci, cap: int, kout: int, idx_offset: int = 0, need=None):
    """``lzk_cand_select``: per query the kout best of the first
    n = min(cnt & 0x3fffffff, cap) list entries; ovf = cnt > cap or (need given
    and cnt < need) -- a cnt with bit 30 set is ovf whenever cap < 2^30; -inf
    entries select as (-inf, -1). Returns (scores fp64 [nq, kout], rows int64
    [nq, kout] (+ idx_offset), ovf int32 [nq])."""
    nq = len(cnt)
    S = np.full((nq, kout), NEG_INF)
    R = np.full((nq, kout), -1, dtype=np.int64)
    ovf = np.zeros(nq, dtype=np.int32)
    for q in range(nq):
        c = int(cnt[q])
        n = min(c & CNT_MASK, cap)
        ovf[q] = 1 if (c > cap or (need is not None and c < int(need[q]))) else 0
        s = np.asarray(cs[q, :n], dtype=np.float64)
        r = np.asarray(ci[q, :n], dtype=np.int64)
        live = s != NEG_INF
        s, r = s[live], r[live]
        o = order(s, r)[:kout]
        S[q, : o.size] = s[o]
        R[q, : o.size] = r[o] + int(idx_offset)
    return S, R, ovf


# ---------------------------------------------------------------- exact scores
def score_ref(X, q, rows, bias, alpha: float):
    """fp64 ``alpha <q, X[rows]> + bias[rows]`` and ``score_bound`` =
    gamma(D + 3) (|alpha| sum |q_d x_d| + |bias|) per row (a non-finite bias
    adds nothing to the bound: the score is then that bias exactly)."""
    Xr = np.asarray(X, dtype=np.float64)[np.asarray(rows, dtype=np.int64)]
    qd = np.asarray(q, dtype=np.float64)
    s = float(alpha) * (Xr @ qd)
    mag = abs(float(alpha)) * (np.abs(Xr) @ np.abs(qd))
    if bias is not None:
        b = np.asarray(bias, dtype=np.float64)[np.asarray(rows, dtype=np.int64)]
        with np.errstate(invalid="ignore"):
            s = s + b
        mag = mag + np.where(np.isfinite(b), np.abs(b), 0.0)
    return s, gamma(Xr.shape[1] + 3) * mag


def rescore_wave_fp32(X, q, bias, alpha: float) -> np.ndarray:
    """``cand_rescore_kernel``'s arithmetic in fp32: lane l of 64 takes the
    4-element chunks l, l + 64, ... (one fma per element), then the xor
    shuffle tree o = 32 .. 1, then alpha * acc + bias. All rows of X at once."""
    return _rescore_fp32(X, q, bias, alpha, 64, (32, 16, 8, 4, 2, 1))


def rescore16_fp32(X, q, bias, alpha: float) -> np.ndarray:
    """``cand_rescore4_kernel``: 16 lanes per entry, chunks part, part + 16,
    ...; tree o = 1, 2, 4, 8."""
    return _rescore_fp32(X, q, bias, alpha, 16, (1, 2, 4, 8))


def _rescore_fp32(X, q, bias, alpha, lanes, tree):
    f = np.float32
    X = np.asarray(X, dtype=f)
    q = np.asarray(q, dtype=f)
    n, D = X.shape
    chunks = D // 4
    acc = np.zeros((n, lanes), dtype=f)
    lane = np.arange(lanes)
    for t in range((chunks + lanes - 1) // lanes):
        c = lane + lanes * t
        ok = c < chunks
        for e in range(4):
            col = np.where(ok, 4 * c + e, 0)
            prod = X[:, col].astype(np.float64) * q[col].astype(np.float64)[None, :]  # exact: 24 + 24 bits
            acc = np.where(ok[None, :], (prod + acc.astype(np.float64)).astype(f), acc)  # fma: one rounding
    for o in tree:
        acc = (acc + acc[:, lane ^ o]).astype(f)
    s = (f(alpha) * acc[:, 0]).astype(f)
    if bias is not None:
        s = (s + np.asarray(bias, dtype=f)).astype(f)
    return s


# ---------------------------------------------------------------- cut
def cut_ref(L, margin, alpha: float, floor=None):
    """``lzk_cand_cut`` from the minimum L of the k exact scores (-inf when one
    of the k is missing or not finite): ``L - m - (2e-4 |alpha| + 1e-6 (1 +
    |L|))`` in fp64 with the fp32 constants, raised to floor - m. Returns (cut,
    cut_bound) with cut_bound = 4 * 2^-24 (|L| + |m| + 1): four fp32 roundings
    at that magnitude (0 where L = -inf: that case is exact)."""
    L = np.asarray(L, dtype=np.float64)
    m = np.asarray(margin, dtype=np.float64)
    fin = np.isfinite(L)
    Lf = np.where(fin, L, 0.0)
    c = np.where(fin, Lf - m - (C_2E4 * abs(float(alpha)) + C_1E6 * (1.0 + np.abs(Lf))), NEG_INF)
    if floor is not None:
        c = np.maximum(c, float(floor) - m)
    return c, np.where(fin, 4.0 * U_FP32 * (np.abs(Lf) + np.abs(m) + 1.0), 0.0)


def cut_min_ref(X, Q, bias, alpha: float, rows, k: int, nrows: int):
    """The L of :func:`cut_ref` per query and the score_bound of the row that
    attains it: the minimum exact score of rows[q, :k], -inf when one of them
    is outside [0, nrows) or has a score that is not finite."""
    nq = rows.shape[0]
    L = np.full(nq, NEG_INF)
    B = np.zeros(nq)
    for q in range(nq):
        r = np.asarray(rows[q, :k], dtype=np.int64)
        if ((r < 0) | (r >= nrows)).any():
            continue
        s, b = score_ref(X, Q[q], r, bias, alpha)
        if not np.isfinite(s).all():
            continue
        j = int(np.argmin(s))
        L[q], B[q] = s[j], b[j]
    return L, B


# ---------------------------------------------------------------- re-score + certificate
def rescore_ref(X, Q, bias, alpha: float, cnt, cs, ci, cap: int, cut=None, floor: float = NEG_INF, tau=None,
                k_need: int = 0, need_val: int = 0, want_need: bool = True, guard: float = 0.0):
    """``lzk_cand_rescore`` / ``lzk_cand_rescore32`` on the first
    n = min(cnt & 0x3fffffff, cap) entries of each list: an entry whose scan
    score is below cut[q] becomes -inf; the others get their exact score, or
    -inf when it is below ``floor``. need[q] = 0 iff (entries with exact score
    >= floor and >= tau[q]) >= k_need, or tau[q] = -inf (tau None: -inf for
    all); else need_val. Entries past n stay as they are.

    Returns a dict: ``cs`` fp64 [nq, cap], ``bound`` (score_bound per re-scored
    entry, 0 elsewhere), ``exact`` (the re-scored entries' fp64 scores before
    the floor, nan elsewhere), ``hits`` [nq], ``need`` int32 [nq] (None unless
    want_need) and ``near`` [nq]: how many re-scored entries lie within
    ``guard * score_bound`` of tau[q] or of floor -- where a correct fp32 kernel
    may decide either way (0 on grid inputs, where scores are exact)."""
    nq = len(cnt)
    out = np.array(cs, dtype=np.float64)
    bound = np.zeros_like(out)
    hits = np.zeros(nq, dtype=np.int64)
    near = np.zeros(nq, dtype=np.int64)
    exact = np.full(out.shape, np.nan)
    need = np.zeros(nq, dtype=np.int32) if want_need else None
    for q in range(nq):
        n = min(int(cnt[q]) & CNT_MASK, cap)
        tq = NEG_INF if tau is None else float(tau[q])
        if n:
            scan = np.asarray(cs[q, :n], dtype=np.float64)
            keep = scan >= float(cut[q]) if cut is not None else np.ones(n, dtype=bool)
            ur, inv = np.unique(np.asarray(ci[q, :n], dtype=np.int64)[keep], return_inverse=True)
            s, b = score_ref(X, Q[q], ur, bias, alpha)  # (each distinct row once: lists repeat rows)
            s, b = s[inv], b[inv]
            res = np.full(n, NEG_INF)
            res[keep] = np.where(s >= floor, s, NEG_INF)
            out[q, :n] = res
            bound[q, :n][keep] = b
            exact[q, :n][keep] = s
            hits[q] = int(((s >= floor) & (s >= tq)).sum())
            if guard > 0.0:
                nr = np.zeros(s.shape, dtype=bool)
                for lvl in (tq, floor):
                    if np.isfinite(lvl):
                        nr |= np.abs(s - lvl) <= guard * b
                near[q] = int(nr.sum())
        if want_need:
            need[q] = 0 if (hits[q] >= k_need or tq == NEG_INF) else need_val
    return {"cs": out, "bound": bound, "exact": exact, "hits": hits, "need": need, "near": near}
