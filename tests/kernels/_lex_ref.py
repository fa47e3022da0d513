"""numpy fp64 oracle of keyword and hybrid search (ops/lex_ops.py holds the
contract; csrc/kernels/lexical.hip and the ``*_ref`` formulations of lex_ops
are held to this file).

* the terms and the rows of slots: ``core.lexical.terms_py``;
* df, N and avgdl: :func:`stats`, recomputed from the columns;
* ``s(m, r)``: :func:`scores` -- a sparse formulation (slot by slot, the rows
  that hold a query term found with ``np.isin``, their weights through a
  dict), every operation IEEE fp64 in the contract's order, so the kernel, the
  numpy formulation and this one agree bit for bit;
* the top-k: :func:`topk`;
* the fusion: :func:`blends64` (fp64 cosines and blends over the distinct
  candidates) and :func:`fuse64`.

A fused result is held to two rules (:func:`check_fused`), with ``tol =
lex_ops.lex_tol(D)``:

1. Every query. Replaying the returned rows in fp64, each one's blend is
   within ``2 tol`` of the best blend not yet returned; the returned score is
   within ``tol`` of its fp64 value; the rows are distinct candidates; padding
   appears exactly when the candidates run out.
2. Decidable queries. Where every fp64 gap between neighbouring blends of the
   first ``k + 1`` candidates (in the oracle's order) exceeds ``2 tol`` -- or
   is exactly 0: an exact fp64 tie arises only between candidates whose inputs
   to the blend are identical (identical rows; ``alpha = 1`` with equal BM25
   scores), whose fp32 values are bit-identical too, so the row decides in
   both -- the rows equal the oracle's. At most CAP = 10 % of a case's queries
   may fall outside rule 2; the helper asserts that.
"""
from __future__ import annotations

import numpy as np

from lazzaro_amd.ops.lex_ops import lex_tol

CAP = 0.10
NEG_INF = float("-inf")


def stats(slots: np.ndarray, dl: np.ndarray):
    """(df: dict term -> rows holding it, N = rows with dl > 0, avgdl) from the columns."""
    df = {}
    for row in slots:
        for s in row:
            if s:
                t = int(s) >> 8
                df[t] = df.get(t, 0) + 1
    N = int((dl > 0).sum())
    avgdl = float(np.sum(dl.astype(np.int64))) / N if N else 1.0
    return df, N, avgdl


def idf(N: int, df: int) -> float:
    return float(np.log1p((N - df + 0.5) / (df + 0.5)))


def weights(qt: np.ndarray, df: dict, N: int) -> np.ndarray:
    w = np.zeros(qt.shape, dtype=np.float64)
    for m in range(qt.shape[0]):
        for j, t in enumerate(qt[m]):
            if t:
                w[m, j] = idf(N, df.get(int(t), 0))
    return w


def scores(slots: np.ndarray, dl: np.ndarray, qt: np.ndarray, w: np.ndarray, k1: float, b: float,
           avgdl: float) -> np.ndarray:
    """s(m, r), fp32 [M, n]."""
    M, (n, W) = qt.shape[0], slots.shape
    K = k1 * ((1.0 - b) + b * (dl.astype(np.float64) / avgdl))
    out = np.zeros((M, n), dtype=np.float32)
    terms = slots >> np.uint32(8)
    tfs = (slots & np.uint32(255)).astype(np.float64)
    for m in range(M):
        wmap = {int(t): float(x) for t, x in zip(qt[m], w[m]) if t}
        if not wmap:
            continue
        keys = np.fromiter(wmap, dtype=np.uint32)
        s = np.zeros(n, dtype=np.float64)
        for j in range(W):
            rows = np.flatnonzero(np.isin(terms[:, j], keys) & (slots[:, j] != 0))
            if rows.size == 0:
                continue
            wj = np.array([wmap[int(t)] for t in terms[rows, j]], dtype=np.float64)
            tf = tfs[rows, j]
            s[rows] = s[rows] + wj * ((tf * (k1 + 1.0)) / (tf + K[rows]))
        out[m] = s.astype(np.float32)
    return out


def topk(sc: np.ndarray, bias: np.ndarray, k: int):
    """The contract's top-k of fp32 scores [M, n]: (scores [M, k], rows [M, k])."""
    M, n = sc.shape
    os_ = np.full((M, k), NEG_INF, dtype=np.float32)
    oi = np.full((M, k), -1, dtype=np.int64)
    ok = np.isfinite(bias[:n])
    for m in range(M):
        e = [r for r in np.flatnonzero(ok & (sc[m] > 0))]
        e.sort(key=lambda r: (-float(sc[m, r]), r))
        for i, r in enumerate(e[:k]):
            os_[m, i], oi[m, i] = sc[m, r], r
    return os_, oi


def den32(w: np.ndarray, k1: float) -> np.ndarray:
    out = np.zeros(w.shape[0], dtype=np.float32)
    for m in range(w.shape[0]):
        tot = 0.0
        for x in w[m]:
            tot = tot + float(x)
        out[m] = np.float32((k1 + 1.0) * tot)
    return out


def blends64(X, Q, dpool, lpool, slots, dl, qt, w, alpha, k1, b, avgdl):
    """Per query: (the distinct candidate rows ascending, their fp64 blends)."""
    n = X.shape[0]
    X64, Q64 = X.astype(np.float64), Q.astype(np.float64)
    den = den32(w, k1)
    a = float(np.float32(alpha))
    out = []
    for m in range(Q.shape[0]):
        pool = np.asarray(lpool[m]) if dpool is None else np.concatenate([np.asarray(dpool[m]), np.asarray(lpool[m])])
        c = np.unique(pool[(pool >= 0) & (pool < n)]).astype(np.int64)
        if c.size == 0:
            out.append((c, np.zeros(0)))
            continue
        q, xc = Q64[m], X64[c]
        qn, xn = np.sqrt(q @ q), np.sqrt((xc * xc).sum(1))
        ok = (qn > 0) & (xn > 0)
        cos = np.where(ok, (xc @ q) / np.where(ok, qn * xn, 1.0), 0.0)
        s = scores(slots[c], dl[c], qt[m:m + 1], w[m:m + 1], k1, b, avgdl)[0].astype(np.float64)
        lexn = s / float(den[m]) if den[m] > 0 else np.zeros_like(s)
        out.append((c, (1.0 - a) * cos + a * lexn))
    return out


def fuse64(cb, k: int):
    """The oracle's result from :func:`blends64`: (blends [M, k], rows [M, k], decidable-gap [M])."""
    M = len(cb)
    os_ = np.full((M, k), NEG_INF)
    oi = np.full((M, k), -1, dtype=np.int64)
    gap = np.full(M, np.inf)
    for m, (c, bl) in enumerate(cb):
        o = sorted(range(len(c)), key=lambda i: (-bl[i], c[i]))
        for i, j in enumerate(o[:k]):
            os_[m, i], oi[m, i] = bl[j], c[j]
        head = [bl[j] for j in o[: k + 1]]
        d = [x - y for x, y in zip(head, head[1:]) if x != y]  # (an exact tie is decided by the row)
        if d:
            gap[m] = min(d)
    return os_, oi, gap


def undecidable(cb, k: int, D: int) -> int:
    """Queries whose oracle result rule 2 does not cover."""
    return int((fuse64(cb, k)[2] <= 2 * lex_tol(D)).sum())


def check_fused(X, Q, dpool, lpool, slots, dl, qt, w, alpha, k1, b, avgdl, k, got_s, got_r):
    """Hold (got_s, got_r) to both rules. Returns the queries left out of rule 2."""
    got_s, got_r = np.asarray(got_s), np.asarray(got_r, dtype=np.int64)
    D = X.shape[1]
    tol = lex_tol(D)
    cb = blends64(X, Q, dpool, lpool, slots, dl, qt, w, alpha, k1, b, avgdl)
    M = len(cb)
    assert got_s.shape == (M, k) and got_r.shape == (M, k)
    for m, (c, bl) in enumerate(cb):
        val = {int(r): float(x) for r, x in zip(c, bl)}
        left = dict(val)
        live = min(k, len(c))
        rows = got_r[m, :live].tolist()
        assert len(set(rows)) == live and all(r in val for r in rows), f"query {m}: rows {got_r[m]} of candidates {c}"
        assert (got_r[m, live:] == -1).all() and np.isneginf(got_s[m, live:]).all(), f"query {m}: padding {got_r[m]}"
        for i, r in enumerate(rows):
            best = max(left.values())
            assert val[r] >= best - 2 * tol, f"query {m} pick {i}: row {r} at {val[r]} but {best} is left"
            assert abs(float(got_s[m, i]) - val[r]) <= tol, f"query {m} pick {i}: {got_s[m, i]} vs {val[r]}"
            del left[r]
    _, ri, gap = fuse64(cb, k)
    clear = gap > 2 * tol
    left_out = int((~clear).sum())
    assert left_out <= CAP * M, f"{left_out} of {M} queries have an fp64 gap within 2 tol: the case decides too little"
    bad = [m for m in np.flatnonzero(clear) if not np.array_equal(got_r[m], ri[m])]
    assert not bad, f"queries {bad[:8]} differ from the fp64 order: {got_r[bad[0]]} vs {ri[bad[0]]}"
    return left_out


# ---- the shared cases of the kernel tests (GPU) and of the CPU tier
VOCAB = 4096
COMMON = 7  # the term every row with words holds


def columns(n: int, W: int, seed: int = 0):
    """Synthetic lexical columns (uint32 [n, W], int32 [n]) and a bias [n]:
    Zipf-drawn terms, the term COMMON in every row that has words; every 11th
    row has dl = 0 and no terms, every 13th has terms but full slots, rows
    5 k and 5 k + 1 (k odd) are identical, every 17th row's bias is -inf; one
    row has words (dl > 0) but no kept term."""
    rng = np.random.default_rng(seed)
    slots = np.zeros((n, W), dtype=np.uint32)
    dl = np.zeros(n, dtype=np.int32)
    p = 1.0 / np.arange(1, VOCAB + 1)
    p /= p.sum()
    for r in range(n):
        if r % 11 == 10:
            continue
        if r % 10 == 6 and (r // 5) % 2 == 1 and r >= 1:
            slots[r], dl[r] = slots[r - 1], dl[r - 1]
            continue
        cnt = W if r % 13 == 12 else int(rng.integers(1, W + 1))
        t = np.sort(np.concatenate([[COMMON], 16 + rng.choice(VOCAB, size=cnt - 1, replace=False, p=p)])).astype(
            np.uint32)
        tf = rng.integers(1, 5, size=len(t)).astype(np.uint32)
        if r % 29 == 3:
            tf[0] = 255
        slots[r, : len(t)] = (t << np.uint32(8)) | tf
        dl[r] = int(tf.sum()) + int(rng.integers(0, 6))
    if n > 40:
        slots[40], dl[40] = 0, 9
    bias = np.where(np.arange(n) % 17 == 16, -np.inf, -rng.random(n)).astype(np.float32)
    return slots, dl, bias


def queries(M: int, T: int, seed: int = 0):
    """uint32 [M, 32]: T terms a query (T = 32: the odd queries hold 31, an
    unused slot), drawn from the columns' vocabulary; every third query holds
    COMMON; one query holds only a term no row has."""
    rng = np.random.default_rng(1000 + seed)
    qt = np.zeros((M, 32), dtype=np.uint32)
    p = 1.0 / np.arange(1, VOCAB + 1)
    p /= p.sum()
    for m in range(M):
        cnt = T - 1 if (T == 32 and m % 2 == 1) else T
        t = set((16 + rng.choice(VOCAB, size=cnt, p=p)).tolist())
        while len(t) < cnt:
            t.add(int(16 + rng.integers(0, VOCAB)))
        t = sorted(t)[:cnt]
        if m % 3 == 0:
            t[0] = COMMON
        if m == 4:
            t = [VOCAB + 100]
        qt[m, : len(t)] = sorted(t)
    return qt


# (n, M, T, W, k, grid cap): see tests/kernels/test_lexical_gpu.py
SCAN_CASES = [(1, 1, 1, 8, 1, 0), (63, 8, 32, 16, 16, 0), (63, 9, 1, 32, 64, 1), (4097, 9, 32, 32, 64, 2),
              (4097, 1, 32, 8, 16, 0), (20011, 33, 32, 16, 64, 4), (20011, 8, 1, 8, 1, 3)]

# (n, D, M, P, k, alpha): the fusion cases
FUSE_CASES = [(4097, 64, 33, 16, 10, 0.0), (4097, 64, 33, 16, 10, 0.3), (4097, 64, 33, 16, 16, 1.0),
              (4097, 64, 33, 64, 16, 0.3), (4097, 768, 33, 16, 10, 0.3), (4097, 768, 33, 16, 10, 0.0),
              (4097, 768, 33, 64, 5, 1.0), (63, 64, 8, 64, 64, 0.3)]


def fuse_inputs(n, D, M, P, seed=0, W=16, k1=1.2, b=0.75):
    """Everything a fusion case needs: rows, queries, columns, terms, weights,
    a dense pool (the fp64 cosine top-P with a few slots emptied and one out
    of range) and the oracle's lexical pool (overlapping the dense pool for
    the queries whose first rows were planted near them; -1 padded where few
    rows match)."""
    rng = np.random.default_rng(77 + seed)
    X = rng.standard_normal((n, D))
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    slots, dl, bias = columns(n, W, seed)
    qt = queries(M, 32 if M > 8 else 3, seed)
    df, N, avgdl = stats(slots, dl)
    w = weights(qt, df, N)
    sc = scores(slots, dl, qt, w, k1, b, avgdl)
    _, lpool = topk(sc, bias, P)
    Q = rng.standard_normal((M, D))
    for m in range(0, M, 2):  # plant the query near its best keyword matches: the pools overlap
        hit = lpool[m][lpool[m] >= 0][:3]
        if hit.size:
            Q[m] = X[hit].sum(0) + 0.3 * Q[m]
    Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    X, Q = X.astype(np.float32), Q.astype(np.float32)
    cos = Q.astype(np.float64) @ X.astype(np.float64).T
    cos[:, ~np.isfinite(bias)] = -np.inf
    dpool = np.argsort(-cos, axis=1, kind="stable")[:, :P].astype(np.int64)
    dpool[cos[np.arange(M)[:, None], dpool] == -np.inf] = -1
    dpool = np.pad(dpool, ((0, 0), (0, P - dpool.shape[1])), constant_values=-1)  # (fewer rows than the pool)
    dpool[::4, P // 2] = -1
    dpool[1::4, 0] = n + 5
    return dict(X=X, Q=Q, slots=slots, dl=dl, bias=bias, qt=qt, w=w, avgdl=avgdl, dpool=dpool, lpool=lpool, k1=k1, b=b)


WORDS = ["alpha", "beta", "gamma", "delta", "router", "kernel", "memory", "ticket", "invoice", "garden", "violin",
         "harbor", "lantern", "orchid", "quartz", "saddle"]
E2E_QUERIES = ["LZ-4812 ticket", "violin and orchid item7", "garden", "nothing matches zzz"]
E2E_WHERE = {"min_salience": 0.5}


def e2e_inputs(n=300, D=64):
    """The small tenant of the end-to-end test: unit rows, texts of common
    words plus one of 40 item tokens, one memory (row 123) that alone holds
    "LZ-4812", saliences r % 10 / 10, and four queries -- the first far from
    row 123. Returns (X, texts, sal, queries, Q)."""
    rng = np.random.default_rng(5)
    X = rng.standard_normal((n, D))
    X = (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)
    texts = [" ".join(rng.choice(WORDS, size=int(rng.integers(3, 12)))) + f" item{r % 40}" for r in range(n)]
    texts[123] = "the ticket LZ-4812 was escalated twice, LZ-4812"
    sal = (np.arange(n) % 10 / 10.0).astype(np.float32)
    Q = np.random.default_rng(9).standard_normal((len(E2E_QUERIES), D)).astype(np.float32)
    Q[0] = -X[123] + 0.1 * Q[0]
    return X, texts, sal, list(E2E_QUERIES), Q
