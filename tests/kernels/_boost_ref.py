"""fp64 oracle of the boosted search (``boost=``; the contract is the
docstring of lazzaro_amd/ops/boost_ops.py). Plain numpy: no GPU, no kernel
library, nothing of the package.

* :func:`boost_prior_ref` / :func:`boost_bias_ref`: the op-by-op fp64 sequence
  of the prior and the column. numpy evaluates one IEEE operation per call, so
  nothing is contracted; the kernel and the torch formulation must reproduce
  every bit.
* :func:`boosted_topk_ref`: fp64 keys ``metric score + column`` ordered by
  ``_ivfpq_ref.order`` (score desc, row asc).
* The exact grid (:func:`grid_rows`, :func:`grid_meta`, ``GRID_BOOST``): rows
  and queries are +-1/8 over 64 dimensions (unit rows, every dot product a
  multiple of 1/64); salience in {0, 1/8, .., 1} at weight 1/2, access counts in
  {0, 5, 10, 20} at weight 1/4, integer clocks with ``now - t`` in {0, 1, 3, 7}
  x 1024 at ``recency_scale = 1024`` -- recency in {1, 1/2, 1/4, 1/8} -- at
  weight 1/4, type weights in {0, 1/8}. ``c * B`` is then a multiple of 1/64,
  exact in fp32, and every key is exact in any summation order: results are
  compared bit for bit, planted duplicate rows included.
* :func:`score_bound`: for other data, how far a correct fp32 score may be
  from the fp64 key.
"""
from __future__ import annotations

import numpy as np

from tests.kernels._ivfpq_ref import gamma, order

NEG_INF = float("-inf")
NODE = 1
U_FP32 = 2.0 ** -24
FLT_MAX = float(np.finfo(np.float32).max)

GRID_D = 64
GRID_NOW = 1_700_000_000.0
GRID_SCALE = 1024.0
GRID_TYPES = ("plain", "pinned")  # type weights 0 and 1/8
GRID_BOOST = {"salience": 0.5, "frequency": 0.25, "recency": 0.25, "recency_scale": GRID_SCALE,
              "type_weights": {"plain": 0.0, "pinned": 0.125, "never-seen": 0.125}, "now": GRID_NOW}


def metric_scale(metric: str) -> float:
    return 2.0 if metric == "l2" else 1.0


def boost_prior_ref(sal, acc, t, now, w_sal, w_freq, w_rec, scale, c, tcode=None, tw=None) -> np.ndarray:
    """``prior(r) = (float)(c * B(r))`` (0 where that is not finite), fp32 [n]."""
    d = np.float64
    sal = np.asarray(sal, dtype=np.float32).astype(d)
    acc = np.asarray(acc, dtype=np.int32).astype(d)
    t = np.asarray(t, dtype=d)
    with np.errstate(all="ignore"):
        f = np.fmin(d(1.0), acc / d(10.0))
        age = np.fmax(d(0.0), d(now) - t)
        rec = d(1.0) / (d(1.0) + age / d(scale))
        B = (d(w_sal) * sal + d(w_freq) * f) + d(w_rec) * rec
        B = B + (np.asarray(tw, dtype=d)[np.asarray(tcode, dtype=np.int64)] if tw is not None else d(0.0))
        p = (d(c) * B).astype(np.float32)
    return np.where(np.abs(p) <= np.float32(FLT_MAX), p, np.float32(0.0)).astype(np.float32)


def boost_bias_ref(base, kind, prior) -> np.ndarray:
    """``out[r] = base[r] + prior[r]`` (one fp32 add) where ``kind[r] == NODE``,
    -inf elsewhere."""
    base = np.asarray(base, dtype=np.float32)
    out = (base + np.asarray(prior, dtype=np.float32)).astype(np.float32)
    return np.where(np.asarray(kind) == NODE, out, np.float32(NEG_INF)).astype(np.float32)


def boost_column_ref(base, sal, acc, t, kind, now, w_sal, w_freq, w_rec, scale, c, tcode=None, tw=None):
    return boost_bias_ref(base, kind, boost_prior_ref(sal, acc, t, now, w_sal, w_freq, w_rec, scale, c, tcode, tw))


def keys_ref(X, Q, col, metric: str) -> np.ndarray:
    """fp64 ``metric score + column`` [M, n]: ``2 <q, x> - |q|^2 + col`` for L2
    (``col`` holds -|x|^2 + prior), ``<q, x> + col`` for IP, the same over the
    normalised query for cosine (unit rows). -inf where the column is."""
    X = np.asarray(X, dtype=np.float64)
    Q = np.asarray(Q, dtype=np.float64)
    col = np.asarray(col, dtype=np.float64)
    if metric == "cosine":
        qn = np.linalg.norm(Q, axis=1, keepdims=True)
        Q = Q / np.where(qn > 0, qn, 1.0)
    S = Q @ X.T
    with np.errstate(invalid="ignore"):
        if metric == "l2":
            return 2.0 * S - (Q * Q).sum(1)[:, None] + col[None, :]
        return S + col[None, :]


def topk_of_keys(keys: np.ndarray, k: int):
    """(scores fp64 [M, k], rows int64 [M, k]) by (key desc, row asc), -inf
    keys left out, (-inf, -1) once rows run out."""
    M, n = keys.shape
    S = np.full((M, k), NEG_INF)
    R = np.full((M, k), -1, dtype=np.int64)
    rows = np.arange(n)
    for q in range(M):
        ok = keys[q] > NEG_INF
        o = order(keys[q][ok], rows[ok])[:k]
        S[q, : o.size], R[q, : o.size] = keys[q][ok][o], rows[ok][o]
    return S, R


def boosted_topk_ref(X, Q, col, metric: str, k: int):
    return topk_of_keys(keys_ref(X, Q, col, metric), k)


def score_bound(X, Q, base, prior, metric: str) -> np.ndarray:
    """[M, n]: how far a correct fp32 score may be from the fp64 key
    ``metric score + (double)base + (double)prior``:
    ``gamma(D + 4) (|alpha| sum |q_d x_d| + |base| + |prior| [+ |q|^2 for L2])``
    -- ``_cand_ref.score_ref``'s form: a D-term fp32 dot in any order, the
    scale by alpha, the bias add, and for L2 the |q|^2 sum and its subtraction
    -- plus ``u |base + prior|`` for the column's own fp32 add."""
    X = np.abs(np.asarray(X, dtype=np.float64))
    Qa = np.abs(np.asarray(Q, dtype=np.float64))
    b = np.asarray(base, dtype=np.float64)
    p = np.asarray(prior, dtype=np.float64)
    fin = np.isfinite(b)
    bm = np.where(fin, np.abs(b) + np.abs(p), 0.0)
    mag = metric_scale(metric) * (Qa @ X.T) + bm[None, :]
    if metric == "l2":
        mag = mag + (Qa * Qa).sum(1)[:, None]
    return gamma(X.shape[1] + 4) * mag + U_FP32 * np.where(fin, np.abs(b + p), 0.0)[None, :]


# ------------------------------------------------------------------ the exact grid
def grid_rows(rng, n: int, D: int = GRID_D, dup: int = 6) -> np.ndarray:
    """[n, D] fp32, the first 64 entries of a row +-1/8 and the rest 0 (unit
    rows at any D >= 64); row n - 1 - 3 j is a copy of row 2 j for j < dup, so
    exact ties between distinct rows exist."""
    X = np.zeros((n, D), dtype=np.float32)
    X[:, :GRID_D] = (rng.integers(0, 2, size=(n, GRID_D)) * 2.0 - 1.0) / 8.0
    for j in range(dup):
        a, b = 2 * j, n - 1 - 3 * j
        if 0 <= a < b < n:
            X[b] = X[a]
    return X


def grid_meta(rng, n: int, dup: int = 6):
    """dict of the grid's node columns: ``sal`` fp32, ``acc`` int32, ``last``
    and ``ts`` fp64 (integers, two independent draws), ``tcode`` uint8 (an index
    into GRID_TYPES). The planted duplicate rows share every column too, so
    their keys tie and only the row number orders them."""
    m = {"sal": (rng.integers(0, 9, size=n) / 8.0).astype(np.float32),
         "acc": rng.choice(np.array([0, 5, 10, 20], dtype=np.int32), size=n),
         "last": GRID_NOW - rng.choice(np.array([0.0, 1.0, 3.0, 7.0]), size=n) * GRID_SCALE,
         "ts": GRID_NOW - rng.choice(np.array([0.0, 1.0, 3.0, 7.0]), size=n) * GRID_SCALE,
         "tcode": rng.integers(0, 2, size=n).astype(np.uint8)}
    for j in range(dup):
        a, b = 2 * j, n - 1 - 3 * j
        if 0 <= a < b < n:
            for v in m.values():
                v[b] = v[a]
    return m


def grid_column(base, meta, kind, metric: str, clock: str = "accessed", types: bool = True) -> np.ndarray:
    """The boosted column of GRID_BOOST over grid columns (type codes as in
    ``meta["tcode"]``: 0 = "plain", 1 = "pinned")."""
    tw = None
    if types:
        tw = np.zeros(256)
        tw[1] = 0.125
    b = GRID_BOOST
    return boost_column_ref(base, meta["sal"], meta["acc"], meta["last" if clock == "accessed" else "ts"], kind,
                            b["now"], b["salience"], b["frequency"], b["recency"], b["recency_scale"],
                            metric_scale(metric), meta["tcode"] if types else None, tw)


def edge_rows(n: int, now: float):
    """Columns of ``n`` rows whose first rows are the edge cases of the kernel
    test, the rest seeded random: -inf base, kind != NODE, t > now, acc 0 and
    > 10, NaN and +-inf salience, an fp32-overflowing salience, now - t = 1e12,
    type codes 0 and 254. Returns (base, sal, acc, t, kind, tcode)."""
    rng = np.random.default_rng(n)
    base = (-rng.random(n)).astype(np.float32)
    sal = rng.random(n).astype(np.float32)
    acc = rng.integers(0, 30, size=n).astype(np.int32)
    t = now - rng.random(n) * 1e6
    kind = np.where(rng.random(n) < 0.9, 1, rng.integers(0, 3, size=n)).astype(np.uint8)
    tcode = rng.choice(np.array([0, 1, 254], dtype=np.uint8), size=n)
    cases = [
        dict(base=NEG_INF), dict(kind=0), dict(kind=2), dict(t=now + 5000.0), dict(acc=0), dict(acc=11),
        dict(acc=2_000_000_000), dict(sal=np.nan), dict(sal=np.inf), dict(sal=-np.inf), dict(sal=3.0e38),
        dict(t=now - 1e12), dict(tcode=0), dict(tcode=254), dict(t=np.nan), dict(sal=np.nan, base=NEG_INF),
        dict(sal=-0.0, acc=0, base=-0.0), dict(acc=-3),
    ]
    cols = {"base": base, "sal": sal, "acc": acc, "t": t, "kind": kind, "tcode": tcode}
    for i, case in enumerate(cases):
        # spread over the row groups a thread takes (positions 0..3 of a group of 4) and the scalar tail
        r = (i * 5) % n
        if i < n:
            kind[r] = 1
            for name, v in case.items():
                cols[name][r] = v
    return base, sal, acc, t, kind, tcode
