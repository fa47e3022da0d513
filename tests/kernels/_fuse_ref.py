"""fp64 oracle of the multi-query fusion and the rules a result is held to
(ops/fuse_ops.py, csrc/kernels/fuse.hip). numpy only.

The oracle implements the contract of ``ops/fuse_ops.py`` literally, with a
naive dict-based union and ranks. ``rrf`` is exact: ``check_rrf`` compares
rows, scores, support and ``ncand`` for equality. ``mean`` takes the fp32
inputs and the fp32 normalised weights cast to float64; ``check_mean`` holds a
result to

1. every group, no exceptions (``check_rule1``): ``ncand`` equals the oracle's
   candidate count; returned rows are distinct members of the oracle's
   candidate set with the oracle's support; padding ``(-inf, -1, 0)`` appears
   exactly when the set runs out; each returned score is within ``tol`` of
   that row's fp64 score; replaying the result, each returned row's fp64 score
   is within ``2 tol`` of the best candidate not returned before it; fp32
   scores are non-increasing and equal bit patterns come in ascending row
   order;
2. the exact prefix: with p the first rank whose fp64 gap to the next
   candidate (rank ``k`` included) is within ``2 tol`` (p = ``k`` if there is
   none), the first p rows equal the oracle's. For a "full order" case at most
   ``CAP`` (10 %) of the groups may have p < k; the helper asserts that when
   told to (``full_order=True``).

``tol`` is ``fuse_ops.fuse_tol(D, G)`` with G the group's own size.
"""
import numpy as np

from lazzaro_amd.ops.fuse_ops import fuse_tol

CAP = 0.10

# (D, P, G, k, NG): the "full order" cases -- at most CAP of the groups have an
# fp64 gap within 2 tol inside the first k + 1 (tests/unit/test_fuse_ref_cpu.py proves it)
FULL_ORDER_CASES = [(64, 16, 4, 10, 128), (768, 16, 4, 10, 128), (100, 16, 3, 10, 128), (2048, 16, 2, 16, 64),
                    (768, 64, 16, 16, 32)]
# k = 64 over 16 pools of 64: held to rule 1 and the exact prefix, no cap. (D, P, G, k, NG, independent)
WIDE_CASES = [(768, 64, 16, 64, 32, False), (768, 64, 16, 64, 32, True)]


class Ref:
    """One group's oracle: ``rows`` the candidate set (ascending), ``score``
    per candidate (float32 for rrf, float64 for mean), ``support`` int, and
    ``order`` the candidates by (score descending, row ascending)."""
    __slots__ = ("rows", "score", "support", "order", "G")


def sizes_of(offsets):
    off = [int(o) for o in np.asarray(offsets).tolist()]
    return off, [b - a for a, b in zip(off, off[1:])]


def ranks_of(pool, n):
    """{row: rank} of one pool: 1 + the non-empty slots before the first occurrence."""
    out, seen = {}, 0
    for r in np.asarray(pool).tolist():
        if r < 0 or r >= n:
            continue
        seen += 1
        if r not in out:
            out[r] = seen
    return out


def normalised(w, sizes):
    """wn_j = (float)(w_j / sum w): fp32 weights, fp64 sum in order, one rounding."""
    w = np.asarray(w, dtype=np.float32)
    out, a = [], 0
    for n in sizes:
        ws = [float(x) for x in w[a:a + n]]
        tot = 0.0
        for x in ws:
            tot = tot + x
        out += [np.float32(x / tot) for x in ws]
        a += n
    return np.asarray(out, dtype=np.float32)


def fuse64(offsets, pools, n, mode="rrf", rrf_k=60.0, weights=None, X=None, Q=None):
    """The oracle: a list of :class:`Ref`, one per group. ``weights``: flat,
    one per sub-query (default 1)."""
    off, sizes = sizes_of(offsets)
    pools = np.asarray(pools, dtype=np.int64)
    M = pools.shape[0]
    w = np.ones(M, dtype=np.float32) if weights is None else np.asarray(weights, dtype=np.float32)
    kk = float(np.float32(rrf_k))
    if mode == "mean":
        wn = normalised(w, sizes)
        X64 = np.asarray(X).astype(np.float64)
        Q64 = np.asarray(Q).astype(np.float64).reshape(M, -1)
    out = []
    for g, G in enumerate(sizes):
        a = off[g]
        ranks = [ranks_of(pools[a + j], n) for j in range(G)]
        rows = sorted(set().union(*[set(r) for r in ranks])) if G else []
        ref = Ref()
        ref.G = G
        ref.rows = np.asarray(rows, dtype=np.int64)
        ref.support = np.asarray([sum(v in r for r in ranks) for v in rows], dtype=np.int64)
        if mode == "rrf":
            sc = []
            for v in rows:
                acc = 0.0
                for j in range(G):
                    if v in ranks[j]:
                        acc = acc + float(w[a + j]) / (kk + float(ranks[j][v]))
                sc.append(np.float32(acc))
            ref.score = np.asarray(sc, dtype=np.float32)
        else:
            x = X64[ref.rows] if rows else np.zeros((0, X64.shape[1]))
            xn = np.sqrt((x * x).sum(1))
            acc = np.zeros(len(rows))
            for j in range(G):
                q = Q64[a + j]
                den = xn * np.sqrt((q * q).sum())
                ok = den > 0
                acc = acc + float(wn[a + j]) * np.where(ok, (x @ q) / np.where(ok, den, 1.0), 0.0)
            ref.score = acc
        ref.order = np.lexsort((ref.rows, -ref.score.astype(np.float64)))
        out.append(ref)
    return out


def expected(refs, k):
    """(rows int64 [NG, k], scores fp32 [NG, k], support int32 [NG, k], ncand int32 [NG]) of the oracle."""
    NG = len(refs)
    rows = np.full((NG, k), -1, dtype=np.int64)
    scores = np.full((NG, k), -np.inf, dtype=np.float32)
    support = np.zeros((NG, k), dtype=np.int32)
    ncand = np.zeros(NG, dtype=np.int32)
    for g, ref in enumerate(refs):
        o = ref.order[:k]
        rows[g, :o.size], scores[g, :o.size], support[g, :o.size] = ref.rows[o], ref.score[o], ref.support[o]
        ncand[g] = ref.rows.size
    return rows, scores, support, ncand


def check_rrf(refs, k, rows, scores, support, ncand):
    """Equality with the oracle, bit for bit."""
    wr, ws, wp, wc = expected(refs, k)
    rows, scores = np.asarray(rows, dtype=np.int64), np.asarray(scores, dtype=np.float32)
    support, ncand = np.asarray(support, dtype=np.int32), np.asarray(ncand, dtype=np.int32)
    assert rows.shape == wr.shape and scores.shape == ws.shape and support.shape == wp.shape and ncand.shape == wc.shape
    assert np.array_equal(ncand, wc), (ncand[:8], wc[:8])
    bad = np.flatnonzero((rows != wr).any(1))
    assert bad.size == 0, f"groups {bad[:8]} differ in rows: {rows[bad[0]]} vs the oracle's {wr[bad[0]]}"
    assert np.array_equal(scores.view(np.uint32), ws.view(np.uint32)), \
        f"scores differ: {scores[(scores != ws).any(1)][:1]} vs {ws[(scores != ws).any(1)][:1]}"
    assert np.array_equal(support, wp)


def check_rule1(refs, k, rows, scores, support, ncand, D):
    rows = np.asarray(rows, dtype=np.int64)
    s32 = np.asarray(scores, dtype=np.float32)
    support = np.asarray(support, dtype=np.int64)
    ncand = np.asarray(ncand, dtype=np.int64)
    NG = len(refs)
    assert rows.shape == (NG, k) and s32.shape == (NG, k) and support.shape == (NG, k) and ncand.shape == (NG,)
    for g, ref in enumerate(refs):
        tol = fuse_tol(D, ref.G)
        C = ref.rows.size
        assert ncand[g] == C, f"group {g}: ncand {ncand[g]} vs the oracle's {C}"
        c = min(k, C)
        assert (rows[g, c:] == -1).all() and np.isneginf(s32[g, c:]).all() and (support[g, c:] == 0).all(), \
            f"group {g}: padding expected from rank {c}: {rows[g]}, {s32[g]}"
        got = rows[g, :c]
        assert (got >= 0).all(), f"group {g}: padding while {C} candidates exist: {rows[g]}"
        assert np.unique(got).size == c, f"group {g}: a row is returned twice: {got}"
        pos = np.searchsorted(ref.rows, got)
        assert (pos < C).all() and (ref.rows[np.minimum(pos, C - 1)] == got).all(), \
            f"group {g}: rows outside the candidate set: {np.setdiff1d(got, ref.rows)}"
        assert np.array_equal(support[g, :c], ref.support[pos]), f"group {g}: support {support[g, :c]}"
        d = np.abs(s32[g, :c].astype(np.float64) - ref.score[pos])
        assert (d <= tol).all(), f"group {g}: score off by {d.max()!r} (tol {tol!r}) at rank {int(d.argmax())}"
        left = np.ones(C, dtype=bool)
        for i in range(c):
            best = ref.score[left].max()
            assert ref.score[pos[i]] >= best - 2 * tol, \
                f"group {g} rank {i}: returned {ref.score[pos[i]]!r}, the best one left is {best!r} (tol {tol!r})"
            left[pos[i]] = False
            if i:
                a, b = s32[g, i - 1], s32[g, i]
                assert a >= b, f"group {g}: scores increase at rank {i}: {a!r} < {b!r}"
                if a.view(np.uint32) == b.view(np.uint32):
                    assert got[i - 1] < got[i], f"group {g}: equal scores out of row order at rank {i}"


def exact_prefix(ref, k, tol):
    """p of rule 2: the first rank whose fp64 gap to the next candidate is within 2 tol."""
    s = ref.score[ref.order].astype(np.float64)
    for i in range(min(k, s.size - 1)):
        if s[i] - s[i + 1] <= 2 * tol:
            return i
    return k


def left_out(refs, k, D):
    """The groups with an fp64 gap within 2 tol inside the first k + 1."""
    return [g for g, ref in enumerate(refs) if exact_prefix(ref, k, fuse_tol(D, ref.G)) < k]


def check_mean(refs, k, rows, scores, support, ncand, D, full_order=False):
    """Hold a ``mean`` result to both rules. Returns the number of groups
    with a gap inside the first k + 1 (asserted <= CAP of them for a
    ``full_order`` case)."""
    check_rule1(refs, k, rows, scores, support, ncand, D)
    rows = np.asarray(rows, dtype=np.int64)
    out = left_out(refs, k, D)
    if full_order:
        assert len(out) <= CAP * len(refs), \
            f"{len(out)} of {len(refs)} groups have an fp64 gap within 2 tol in their first ranks: the case decides too little"
    for g, ref in enumerate(refs):
        p = min(exact_prefix(ref, k, fuse_tol(D, ref.G)), ref.rows.size)
        want = ref.rows[ref.order[:p]]
        assert np.array_equal(rows[g, :p], want), f"group {g}: first {p} rows {rows[g, :p]} vs the oracle's {want}"
    return len(out)


def rrf_tie_groups(refs, k):
    """The groups whose first k + 1 hold two equal fp32 RRF scores."""
    out = []
    for g, ref in enumerate(refs):
        s = ref.score[ref.order][:k + 1]
        if (s[:-1] == s[1:]).any():
            out.append(g)
    return out


def shared_share(refs):
    """The share of union rows that more than one pool holds, over all groups."""
    tot = sum(r.rows.size for r in refs)
    return sum(int((r.support > 1).sum()) for r in refs) / max(tot, 1)


def recipe(D, P, G, NG, n=None, seed=0, rank=8, sigma=0.35, independent=False):
    """``_mmr_ref.recipe``'s rank-8 unit rows; a group's sub-queries are
    ``unit(unit(base) + sigma * noise / sqrt(rank))`` in the rank-8 space
    (``independent``: every sub-query a base of its own), embedded by the same
    orthonormal basis; pools are the fp64 L2 top-``P``, nearest first. Returns
    (X fp32 [n, D], Q fp32 [NG * G, D], offsets int64 [NG + 1], pools int64
    [NG * G, P])."""
    n = n if n is not None else (4097 if P > 16 else 2048)
    rng = np.random.default_rng(seed)
    B = np.linalg.qr(rng.standard_normal((D, rank)))[0].T          # [rank, D], orthonormal rows
    unit = lambda a: a / np.linalg.norm(a, axis=-1, keepdims=True)  # noqa: E731
    X = unit(rng.standard_normal((n, rank)) @ B).astype(np.float32)
    if independent:
        q8 = unit(rng.standard_normal((NG, G, rank)))
    else:
        base = unit(rng.standard_normal((NG, 1, rank)))
        q8 = unit(base + sigma * rng.standard_normal((NG, G, rank)) / np.sqrt(rank))
    Q = (q8.reshape(NG * G, rank) @ B).astype(np.float32)
    X64, Q64 = X.astype(np.float64), Q.astype(np.float64)
    s = 2.0 * Q64 @ X64.T - (X64 * X64).sum(1)[None, :]            # -|q - x|^2 + |q|^2
    pools = np.argsort(-s, axis=1, kind="stable")[:, :P].astype(np.int64)
    return X, Q, np.arange(NG + 1, dtype=np.int64) * G, pools


def mangle(pools, n, seed=0):
    """``pools`` with what a search can return and more: -1 holes mid-list
    (15 % of the slots), rows >= n (5 %), in every third pool two later slots
    that repeat an earlier slot's row, and pool ``M // 2`` all empty."""
    rng = np.random.default_rng(seed)
    p = np.array(pools, dtype=np.int64)
    M, P = p.shape
    holes = rng.random(p.shape) < 0.15
    p[holes] = -1
    p[rng.random(p.shape) < 0.05] = n + 3
    for m in range(0, M, 3):                 # a repeat: a later slot takes an earlier slot's row
        if P >= 4:
            p[m, P - 1] = p[m, 1]
            p[m, P // 2] = p[m, 0]
    p[M // 2] = -1                           # an all-empty pool
    return p
