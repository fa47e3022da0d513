"""fp64 references of the wide-k store search (csrc/kernels/widek.hip,
ops/search.py ``flat_topk_wide`` / ``flat_topk_i8_wide``, the ``wide_k`` route
of ``TenantGraph._store_search``). Plain numpy; nothing here touches a GPU or
the kernel library. tests/unit/test_wide_ref_cpu.py checks this module on its
own, tests/kernels/test_widek_gpu.py holds the kernels against it. The select's
reference is ``select_ref`` of _cand_ref.py, which is generic in ``kout``.

Order. (score descending, row ascending), missing entries ``(-inf, -1)``:
``order`` of _ivfpq_ref.py.

Threshold rule. A row is in the 1/S sample with probability 1/S, so the
number of a query's true top-k rows inside the sample is Binomial(k, 1/S).
``spec_j`` is the smallest j <= 16 whose tail P(Binomial(k, 1/S) >= j) is at
most 1e-4 (16 if none): computed here by the recurrence of the binomial
probabilities, independently of the library's sum of ``math.comb`` terms.

Gaussian inputs, the bound (``gamma(n) = n u / (1 - n u)``, u = 2^-24; a term
that passes through at most n - 1 roundings is off by at most ``gamma(n)`` of
its magnitude). ``flat_topk_wide_kernel`` states its order: the 8 lanes of a
row each run one fma chain over their 8-element pieces (D / 8 fmas of exact
bf16 x bf16 products), three shuffle adds, ``alpha * acc`` and ``+ bias``: at
most ``D / 8 + 5`` roundings, ``wide_bound = gamma(D / 8 + 6) (|alpha| sum|q x|
+ |b|)``. The certified route's scores come from ``cand_rescore_kernel``
(``gamma(D + 3)``, _cand_ref.py ``score_ref``) or from the wide kernel (its
fallback), so end-to-end cases use ``gamma(D + 3)``, which covers both.

Decidable cases. ``gauss_case`` re-draws rows until, for every query, the
fp64 scores of ranks 1 .. k + 1 are pairwise more than twice the bound apart:
no correct fp32 kernel can return other rows or another order, and no query
has to be left out of a comparison.
"""
from __future__ import annotations

import functools

import numpy as np

from tests.kernels._cand_ref import to_bf16, unit_rows
from tests.kernels._ivfpq_ref import NEG_INF, gamma, order

P_FALLBACK = 1e-4
KC = 64  # bf16 candidates the wide route hands to the fp32 re-rank


# ---------------------------------------------------------------- threshold rule
def binom_tail(k: int, p: float, j: int) -> float:
    """P(Binomial(k, p) >= j) by the ratio recurrence pmf(i + 1) = pmf(i) (k - i) / (i + 1) p / (1 - p)."""
    if j <= 0:
        return 1.0
    if p >= 1.0:
        return 1.0 if j <= k else 0.0
    pmf = (1.0 - p) ** k
    below = 0.0
    for i in range(min(j, k + 1)):
        below += pmf
        pmf = pmf * (k - i) / (i + 1) * p / (1.0 - p)
    return max(0.0, 1.0 - below)


def spec_j(k: int, S: int, p_max: float = P_FALLBACK) -> int:
    for j in range(1, 17):
        if binom_tail(k, 1.0 / S, j) <= p_max:
            return j
    return 16


# ---------------------------------------------------------------- exact top-k
def scores64(X, Q, bias=None, alpha: float = 1.0) -> np.ndarray:
    """fp64 ``alpha <q, x> + bias`` [nq, N]; -inf where the bias is."""
    s = float(alpha) * (np.asarray(Q, dtype=np.float64) @ np.asarray(X, dtype=np.float64).T)
    if bias is not None:
        b = np.asarray(bias, dtype=np.float64)
        with np.errstate(invalid="ignore"):
            s = s + b[None, :]
        s[:, b == NEG_INF] = NEG_INF
    return s


def topk_of(S: np.ndarray, k: int, idx_offset: int = 0):
    """Per query the k best columns of S by ``order``: (scores fp64 [nq, k], rows
    int64 [nq, k] + idx_offset), (-inf, -1) past the columns that are not -inf."""
    nq, n = S.shape
    os_ = np.full((nq, k), NEG_INF)
    oi = np.full((nq, k), -1, dtype=np.int64)
    rows = np.arange(n, dtype=np.int64)
    for q in range(nq):
        live = S[q] != NEG_INF
        o = rows[live][order(S[q][live], rows[live])[:k]]
        os_[q, : o.size] = S[q][o]
        oi[q, : o.size] = o + int(idx_offset)
    return os_, oi


def topk_ref(X, Q, k: int, bias=None, alpha: float = 1.0, idx_offset: int = 0):
    """``flat_topk_wide``: the exact top-k over all rows."""
    return topk_of(scores64(X, Q, bias, alpha), k, idx_offset)


def wide_roundings(D: int) -> int:
    return D // 8 + 5


def wide_bound(X, Q, bias=None, alpha: float = 1.0, roundings: int = None) -> np.ndarray:
    """``gamma(roundings + 1) (|alpha| sum|q x| + |b|)`` [nq, N] (default: the
    wide kernel's D / 8 + 5 roundings); a non-finite bias adds nothing."""
    X = np.asarray(X, dtype=np.float64)
    n = wide_roundings(X.shape[1]) if roundings is None else int(roundings)
    mag = abs(float(alpha)) * (np.abs(np.asarray(Q, dtype=np.float64)) @ np.abs(X).T)
    if bias is not None:
        b = np.asarray(bias, dtype=np.float64)
        mag = mag + np.where(np.isfinite(b), np.abs(b), 0.0)[None, :]
    return gamma(n + 1) * mag


# ---------------------------------------------------------------- the route's contract
def store_scores64(X32, Q32, bias, metric: str) -> np.ndarray:
    """The store's fp32-precision score in fp64 (TenantGraph._store_scores):
    l2: ``2 <q, x> + bias - |q|^2``; ip: ``<q, x> + bias``; cosine: ``<q / |q|, x> /
    |x| + bias``. ``bias`` is the search's row column (-|x|^2 or 0, -inf = masked)."""
    X = np.asarray(X32, dtype=np.float64)
    Q = np.asarray(Q32, dtype=np.float64)
    b = np.asarray(bias, dtype=np.float64)[None, :]
    if metric == "cosine":
        qn = np.linalg.norm(Q, axis=1, keepdims=True)
        Q = Q / np.where(qn > 0, qn, 1.0)
    dot = Q @ X.T
    with np.errstate(invalid="ignore"):
        if metric == "l2":
            s = 2.0 * dot + b - (Q * Q).sum(1)[:, None]
        elif metric == "cosine":
            nrm = np.linalg.norm(X, axis=1)
            s = dot / np.where(nrm > 0, nrm, 1.0)[None, :] + b
        else:
            s = dot + b
    s[:, np.asarray(bias) == NEG_INF] = NEG_INF
    return s


def contract_ref(X32, Q32, bias, metric: str, k: int, kc: int = KC):
    """The wide search's contract: the ``kc`` rows with the largest bf16 score
    ``alpha <bf16(q), bf16(x)> + bias`` (alpha = 2 for l2, else 1; cosine: the
    normalised query), then the k best of those by the store's score, ties to
    the lower row. Returns (scores fp64 [nq, k], rows int64 [nq, k])."""
    Q = np.asarray(Q32, dtype=np.float64)
    if metric == "cosine":
        qn = np.linalg.norm(Q, axis=1, keepdims=True)
        Q = (Q / np.where(qn > 0, qn, 1.0)).astype(np.float32).astype(np.float64)
    alpha = 2.0 if metric == "l2" else 1.0
    _, cand = topk_ref(to_bf16(X32), to_bf16(Q), kc, bias, alpha)
    full = store_scores64(X32, Q32, bias, metric)
    os_ = np.full((Q.shape[0], k), NEG_INF)
    oi = np.full((Q.shape[0], k), -1, dtype=np.int64)
    for q in range(Q.shape[0]):
        c = cand[q][cand[q] >= 0]
        s = full[q, c]
        live = s != NEG_INF
        c, s = c[live], s[live]
        o = order(s, c)[:k]
        os_[q, : o.size], oi[q, : o.size] = s[o], c[o]
    return os_, oi


# ---------------------------------------------------------------- decidable Gaussian cases
# (name, N, D, nq, k, roundings: None = the wide kernel's, else D + 2 = the re-score kernel's)
GAUSS_CASES = {
    "wide_kernel": (4097, 128, 3, 40, None),
    "i8_k17_nq1": (10253, 128, 1, 17, 130),
    "i8_k64_nq1": (10253, 128, 1, 64, 130),
    "i8_k17_nq130": (10253, 128, 130, 17, 130),
    "i8_k64_nq130": (10253, 128, 130, 64, 130),
}
ALPHA = 2.0  # the L2 serving form: alpha = 2, bias = -|x|^2


def l2_bias(X) -> np.ndarray:
    return -(np.asarray(X, dtype=np.float32) ** 2).sum(1, dtype=np.float32)


def undecided(S: np.ndarray, B: np.ndarray, k: int):
    """(query, rank) pairs of the fp64 top-(k + 1) whose neighbour below is
    within twice the larger of the two bounds, and the rows at those ranks."""
    _, rows = topk_of(S, k + 1)
    rr = np.maximum(rows, 0)
    s = np.take_along_axis(S, rr, 1)
    b = np.take_along_axis(B, rr, 1)
    live = (rows[:, :-1] >= 0) & (rows[:, 1:] >= 0)
    with np.errstate(invalid="ignore"):
        bad = live & ((s[:, :-1] - s[:, 1:]) <= 2.0 * np.maximum(b[:, :-1], b[:, 1:]))
    return bad, rows


def near(rng, q, c: float) -> np.ndarray:
    """A bf16 unit-ish row at cosine ~c to the unit vector q."""
    u = rng.standard_normal(q.size)
    u -= (u @ q) * q
    return to_bf16((c * q + np.sqrt(1.0 - c * c) * u / np.linalg.norm(u))[None, :])[0]


CERT_PLANTED = {1: (0,), 130: (0, 43, 86)}  # the queries whose best rows sit inside every 1/S sample (S | 160)
CERT_ROWS = 12                              # planted rows per such query: more than any j <= 9 the rule gives here


@functools.lru_cache(maxsize=None)
def cert_case(name: str):
    """:func:`gauss_case` with, for the queries CERT_PLANTED, CERT_ROWS rows at
    cosine 0.98, 0.97, ... to the query planted at multiples of 160 (inside the
    sample for every stride dividing 160): the sample's j-th best then lies
    above the query's k-th score and the certificate must fire. Re-planted
    with fresh noise until every (query, rank <= k) is decided again.
    Returns (X, Q, bias, scores, bounds, planted bool [nq])."""
    N, D, nq, k, roundings = GAUSS_CASES[name]
    X0, Q, _, _, _ = gauss_case(name)
    planted = np.zeros(nq, dtype=bool)
    planted[list(CERT_PLANTED[nq])] = True
    rng = np.random.default_rng(7 + sum(map(ord, name)))
    for _ in range(50):
        X = X0.copy()
        slot = 0
        for q in np.flatnonzero(planted):
            qn = Q[q] / np.linalg.norm(Q[q])
            for i in range(CERT_ROWS):
                X[160 * slot] = near(rng, qn, 0.98 - 0.01 * i)
                slot += 1
        bias = l2_bias(X)
        S = scores64(X, Q, bias, ALPHA)
        B = wide_bound(X, Q, bias, ALPHA, roundings)
        if not undecided(S, B, k)[0].any():
            return X, Q, bias, S, B, planted
    raise AssertionError(f"{name}: the planted store did not settle")


# ---------------------------------------------------------------- the tenant case
TENANT_N, TENANT_D, TENANT_M = 4096, 96, 130
METRICS = ("l2", "ip", "cosine")


def bf16_unsafe(v: np.ndarray) -> np.ndarray:
    """Elements of v whose bf16 rounding could change under a perturbation of
    2^-21 relative (a few fp32 ulps): within that of a bf16 rounding midpoint."""
    v = np.asarray(v, dtype=np.float64)
    lo = to_bf16(v)
    ulp = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(v), 1e-30))) - 7)
    frac = np.abs(v - lo) / ulp  # 0 .. 0.5: distance to the value it rounds to; 0.5 = the midpoint
    return np.abs(frac - 0.5) < 2.0 ** -13


@functools.lru_cache(maxsize=None)
def tenant_case():
    """fp32 unit rows X [N, D] and queries Q [M, D] (norm 1.3: the cosine
    search normalises them) for ``store_search(wide_k=True)``, re-drawn until
    for every metric and query (a) no element of the normalised query sits on
    a bf16 rounding midpoint, (b) the bf16 scores of ranks 64 and 65 are more
    than twice the re-score bound ``gamma(D + 3)`` apart (the 64 candidates
    are forced) and (c) the fp32-precision scores of the 64 candidates are
    pairwise more than twice the sum of their re-rank bounds apart (the
    re-rank's rows and order are forced, for every k <= 64). Returns (X, Q)."""
    from tests.kernels._rerank_ref import rerank_scores
    N, D, M = TENANT_N, TENANT_D, TENANT_M
    rng = np.random.default_rng(77)
    X = unit_rows(rng, N, D).astype(np.float32)
    Q = (1.3 * unit_rows(rng, M, D)).astype(np.float32)
    for _ in range(200):
        bad_rows, bad_q = set(), set()
        sqn = (X.astype(np.float64) ** 2).sum(1).astype(np.float32)
        for metric in METRICS:
            Qm = tenant_query(Q, metric)
            bad_q.update(np.flatnonzero(bf16_unsafe(Qm).any(1)).tolist())
            bias, alpha = tenant_bias(X, metric), 2.0 if metric == "l2" else 1.0
            X16, Q16 = to_bf16(X), to_bf16(Qm)
            S = scores64(X16, Q16, bias, alpha)
            B = wide_bound(X16, Q16, bias, alpha, D + 2)
            s, r = topk_of(S, KC + 1)
            b = np.take_along_axis(B, r, 1)
            edge = (s[:, KC - 1] - s[:, KC]) <= 2.0 * (b[:, KC - 1] + b[:, KC])
            bad_rows.update(r[edge, KC].tolist())
            cand = r[:, :KC]
            Sr, Br = rerank_scores(Qm, X, sqn, bias, cand, metric)
            o = np.argsort(-Sr, axis=1, kind="stable")
            ss, bb, cc = (np.take_along_axis(a, o, 1) for a in (Sr, Br, cand))
            close = (ss[:, :-1] - ss[:, 1:]) <= 2.0 * (bb[:, :-1] + bb[:, 1:])
            bad_rows.update(cc[:, 1:][close].tolist())
        if not bad_rows and not bad_q:
            return X, Q
        for v in sorted(bad_rows):
            X[v] = unit_rows(rng, 1, D)[0].astype(np.float32)
        for q in sorted(bad_q):
            Q[q] = (1.3 * unit_rows(rng, 1, D))[0].astype(np.float32)
    raise AssertionError("the tenant case did not settle")


def tenant_query(Q, metric: str) -> np.ndarray:
    """The fp32 query the search scores with: normalised for cosine."""
    Q = np.asarray(Q, dtype=np.float32)
    if metric != "cosine":
        return Q
    qn = np.linalg.norm(Q.astype(np.float64), axis=1, keepdims=True)
    return (Q / np.where(qn > 0, qn, 1.0)).astype(np.float32)


def tenant_bias(X, metric: str) -> np.ndarray:
    X = np.asarray(X, dtype=np.float32)
    return l2_bias(X) if metric == "l2" else np.zeros(X.shape[0], dtype=np.float32)


def tenant_expected(X, Q, metric: str, k: int, bias=None):
    """(scores fp64 [M, k], rows [M, k], bounds [M, k]) of the wide route's
    contract on fp32 rows: the fp64 bf16 top-64, re-ranked by ``rerank_ref``."""
    from tests.kernels._rerank_ref import rerank_ref
    Qm = tenant_query(Q, metric)
    bias = tenant_bias(X, metric) if bias is None else bias
    sqn = (np.asarray(X, dtype=np.float64) ** 2).sum(1).astype(np.float32)
    _, cand = topk_ref(to_bf16(X), to_bf16(Qm), KC, bias, 2.0 if metric == "l2" else 1.0)
    return rerank_ref(Qm, X, sqn, bias, cand, k, metric)


@functools.lru_cache(maxsize=None)
def gauss_case(name: str):
    """(X, Q, bias, fp64 scores, bounds) of one GAUSS_CASES entry: bf16 values as
    fp64, unit rows and queries, bias = -|x|^2 (fp32). Rows are re-drawn until
    no (query, rank <= k) is left undecided."""
    N, D, nq, k, roundings = GAUSS_CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    X = to_bf16(unit_rows(rng, N, D))
    Q = to_bf16(unit_rows(rng, nq, D))
    for _ in range(200):
        bias = l2_bias(X)
        S = scores64(X, Q, bias, ALPHA)
        B = wide_bound(X, Q, bias, ALPHA, roundings)
        bad, rows = undecided(S, B, k)
        if not bad.any():
            return X, Q, bias, S, B
        victims = np.unique(rows[:, 1:][bad])  # the lower row of each close pair
        X[victims] = to_bf16(unit_rows(rng, victims.size, D))
    raise AssertionError(f"{name}: the store did not settle")
