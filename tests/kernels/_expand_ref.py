"""fp64 oracle of the associative (graph-expanded) selection and the two rules
a result is held to (ops/expand_ops.py, csrc/kernels/expand.hip). numpy only.

The oracle implements the contract of ``ops/expand_ops.py`` literally: the fp32
inputs cast to float64, ``decay`` and ``graph_weight`` taken as their fp32
values, the ``w >= min_weight`` test done in fp32, hops in Jacobi order, ties
to the lower row. ``check_against_ref`` holds a result to

1. every query, no exceptions (``check_rule1``): ``ncand`` equals the oracle's
   candidate count; returned rows are distinct members of the oracle's
   candidate set; padding appears exactly when the set runs out; each returned
   score is within ``tol`` of that row's fp64 score; fp32 scores are
   non-increasing and equal bit patterns come in ascending row order; no
   candidate that was not returned has an fp64 score above the last returned
   row's by more than ``2 tol``; each ``via`` is -1 or a source whose fp64
   proposal is within ``2 tol`` of the row's fp64 activation, and -1 only if
   the row's own activation is within ``2 tol`` of it;
2. the exact prefix: with p the first rank whose fp64 gap to the next
   candidate (rank ``limit`` included) is within ``2 tol`` (p = ``limit`` if
   there is none), the first p rows equal the oracle's. At most ``CAP`` (10 %)
   of a case's queries may have p < min(limit, 16); the helper asserts that.

``tol`` is ``expand_ops.expand_tol(D, hops)``: the kernel's stated summation
depth, 2 roundings per hop and the blend's own.
"""
import numpy as np

from lazzaro_amd.ops.expand_ops import expand_tol

CAP = 0.10
NODE = 1


class Ref:
    """One query's oracle: ``rows`` the candidate set (ascending), ``score``,
    ``act``, ``own`` float64 per candidate, ``via`` int64, ``prop`` a dict
    row -> {source row: largest fp64 proposal}, ``order`` the candidates by
    (score descending, row ascending)."""
    __slots__ = ("rows", "score", "act", "own", "via", "prop", "order")


def _settings(spec):
    from lazzaro_amd.core.expand import GraphExpand
    sp = GraphExpand.coerce(spec)
    return sp, float(np.float32(sp.decay)), float(np.float32(sp.graph_weight)), np.float32(sp.min_weight)


def _cos64(x, q):
    """cos of the rows ``x`` [c, D] with ``q`` [D] in float64, 0 when either norm is 0."""
    den = np.sqrt((x * x).sum(1)) * np.sqrt((q * q).sum())
    ok = den > 0
    return np.where(ok, (x @ q) / np.where(ok, den, 1.0), 0.0)


def expand64(X, Q, seeds, csr, w, kind, sup, bias, spec):
    """The oracle: a list of :class:`Ref`, one per query."""
    sp, lam, gam, min_w = _settings(spec)
    X = np.asarray(X)
    Q = np.asarray(Q, dtype=np.float64).reshape(-1, X.shape[1])
    seeds = np.asarray(seeds, dtype=np.int64).reshape(Q.shape[0], -1)
    off, adj, eid = (np.asarray(a, dtype=np.int64) for a in csr)
    w32 = np.asarray(w, dtype=np.float32)
    passes = w32 >= min_w                                  # (the fp32 comparison)
    wmin1 = np.minimum(w32.astype(np.float64), 1.0)
    target = (np.asarray(kind)[: X.shape[0]] == NODE) & np.isfinite(np.asarray(bias, dtype=np.float32)[: X.shape[0]])
    sup = np.asarray(sup)
    n = X.shape[0]
    # the arcs a source takes: the first `fanout` qualifying of its segment (no score involved)
    taken = {}

    def arcs(u):
        t = taken.get(u)
        if t is None:
            t = []
            if not sup[u]:
                for p in range(int(off[u]), int(off[u + 1])):
                    if len(t) >= sp.fanout:
                        break
                    v, e = int(adj[p]), int(eid[p])
                    if passes[e] and target[v]:
                        t.append((v, lam * wmin1[e]))
            taken[u] = t
        return t

    out = []
    for m in range(Q.shape[0]):
        s = np.unique(seeds[m][(seeds[m] >= 0) & (seeds[m] < n)])
        own = dict(zip(s.tolist(), np.maximum(_cos64(X[s].astype(np.float64), Q[m]), 0.0).tolist())) if s.size else {}
        act = dict(own)
        prop = {}
        for _ in range(sp.hops):
            new = dict(act)
            for u, au in act.items():                      # Jacobi: the entries and activations at the hop's start
                for v, f in arcs(u):
                    t = au * f
                    pv = prop.setdefault(v, {})
                    if t > pv.get(u, -1.0):
                        pv[u] = t
                    if v not in new:
                        new[v] = 0.0
                        own[v] = 0.0
                    if t > new[v]:
                        new[v] = t
            act = new
        r = Ref()
        r.rows = np.array(sorted(act), dtype=np.int64)
        r.act = np.array([act[v] for v in r.rows.tolist()])
        r.own = np.array([own[v] for v in r.rows.tolist()])
        r.prop = prop
        r.via = np.full(r.rows.size, -1, dtype=np.int64)
        for i, v in enumerate(r.rows.tolist()):
            pv = prop.get(v)
            if pv and max(pv.values()) > r.own[i]:
                best = max(pv.values())
                r.via[i] = min(u for u, t in pv.items() if t == best)
        cos = _cos64(X[r.rows].astype(np.float64), Q[m]) if r.rows.size else np.zeros(0)
        r.score = (1.0 - gam) * cos + gam * r.act
        r.order = np.lexsort((r.rows, -r.score))
        out.append(r)
    return out


def check_rule1(refs, limit, rows, scores, via, ncand, tol):
    """Rule 1 of the module docstring for every query."""
    rows = np.asarray(rows, dtype=np.int64)
    s32 = np.asarray(scores, dtype=np.float32)
    via = np.asarray(via, dtype=np.int64)
    ncand = np.asarray(ncand, dtype=np.int64)
    M = len(refs)
    assert rows.shape == (M, limit) and s32.shape == (M, limit) and via.shape == (M, limit) and ncand.shape == (M,)
    for m, ref in enumerate(refs):
        C = ref.rows.size
        assert ncand[m] == C, f"query {m}: ncand {ncand[m]} vs the oracle's {C}"
        k = min(limit, C)
        assert (rows[m, k:] == -1).all() and np.isneginf(s32[m, k:]).all() and (via[m, k:] == -1).all(), \
            f"query {m}: padding expected from rank {k}: {rows[m]}, {s32[m]}"
        got = rows[m, :k]
        assert (got >= 0).all(), f"query {m}: padding while {C} candidates exist: {rows[m]}"
        assert np.unique(got).size == k, f"query {m}: a row is returned twice: {got}"
        pos = np.searchsorted(ref.rows, got)
        assert (pos < C).all() and (ref.rows[np.minimum(pos, C - 1)] == got).all(), \
            f"query {m}: rows outside the candidate set: {np.setdiff1d(got, ref.rows)}"
        d = np.abs(s32[m, :k].astype(np.float64) - ref.score[pos])
        assert (d <= tol).all(), f"query {m}: score off by {d.max()!r} (tol {tol!r}) at rank {int(d.argmax())}"
        for i in range(1, k):
            a, b = s32[m, i - 1], s32[m, i]
            assert a >= b, f"query {m}: scores increase at rank {i}: {a!r} < {b!r}"
            if a.view(np.uint32) == b.view(np.uint32):
                assert got[i - 1] < got[i], f"query {m}: equal scores out of row order at rank {i}: {got[i - 1:i + 1]}"
        if k < C:
            rest = np.ones(C, dtype=bool)
            rest[pos] = False
            over = ref.score[rest].max() - ref.score[pos[-1]]
            assert over <= 2 * tol, f"query {m}: a candidate left out beats the last returned by {over!r}"
        for i in range(k):
            p, v = int(pos[i]), int(via[m, i])
            pv = ref.prop.get(int(got[i]), {})
            top = max([ref.own[p]] + list(pv.values()))
            assert abs(top - ref.act[p]) == 0.0
            if v == -1:
                assert ref.own[p] >= top - 2 * tol, f"query {m} row {got[i]}: via -1 but own {ref.own[p]!r} < {top!r}"
            else:
                assert v in pv and pv[v] >= top - 2 * tol, \
                    f"query {m} row {got[i]}: via {v} proposes {pv.get(v)!r}, the activation is {top!r}"


def exact_prefix(ref, limit, tol):
    """p of rule 2: the first rank whose fp64 gap to the next candidate is within 2 tol."""
    s = ref.score[ref.order]
    for i in range(min(limit, s.size - 1)):
        if s[i] - s[i + 1] <= 2 * tol:
            return i
    return limit


def left_out(refs, limit, tol):
    """The queries whose exact prefix is shorter than min(limit, 16)."""
    return [m for m, ref in enumerate(refs) if exact_prefix(ref, limit, tol) < min(limit, 16)]


def check_against_ref(X, Q, seeds, csr, w, kind, sup, bias, spec, limit, rows, scores, via, ncand, refs=None):
    """Hold a result to both rules. Returns the number of queries left out of
    the first min(limit, 16) ranks of rule 2 (asserted <= CAP of them)."""
    sp = _settings(spec)[0]
    tol = expand_tol(np.asarray(X).shape[1], sp.hops)
    refs = refs if refs is not None else expand64(X, Q, seeds, csr, w, kind, sup, bias, sp)
    check_rule1(refs, limit, rows, scores, via, ncand, tol)
    rows = np.asarray(rows, dtype=np.int64)
    out = left_out(refs, limit, tol)
    assert len(out) <= CAP * len(refs), \
        f"{len(out)} of {len(refs)} queries have an fp64 gap within 2 tol in their first ranks: the case decides too little"
    for m, ref in enumerate(refs):
        p = min(exact_prefix(ref, limit, tol), ref.rows.size)
        want = ref.rows[ref.order[:p]]
        assert np.array_equal(rows[m, :p], want), f"query {m}: first {p} rows {rows[m, :p]} vs the oracle's {want}"
    return len(out)


def csr_of(src, dst, n):
    """The visible-arc CSR of a one-shard edge list, as ``build_visible_csr``
    orders it: a -> b and b -> a for an edge (a, b), a self-loop once, each
    source's arcs by edge index. Returns (off int64 [n + 1], adj int32, eid int32)."""
    src = np.asarray(src, dtype=np.int64)
    dst = np.asarray(dst, dtype=np.int64)
    ne = src.size
    frm = np.stack([src, dst], 1).reshape(-1)
    to = np.stack([dst, src], 1).reshape(-1)
    ok = np.stack([np.ones(ne, bool), src != dst], 1).reshape(-1)
    e = np.repeat(np.arange(ne), 2)
    frm, to, e = frm[ok], to[ok], e[ok]
    o = np.argsort(frm, kind="stable")
    off = np.zeros(n + 1, dtype=np.int64)
    off[1:] = np.cumsum(np.bincount(frm, minlength=n)[:n])
    return off, to[o].astype(np.int32), e[o].astype(np.int32)


def recipe(D, M=128, n=2048, seed=0, deg=6, seed_k=16, rank=8):
    """Rank-8 Gaussian rows and queries embedded in R^D by a random orthonormal
    basis and unit-normalised (as ``_mmr_ref.recipe``), ``n * deg / 2`` edges
    between uniformly random pairs with w ~ U(0.05, 1) in one shard, seeds the
    fp64 cosine top-``seed_k``. Returns a dict of numpy arrays: X, Q, seeds,
    csr, w, kind, sup, bias (every row a searchable node)."""
    rng = np.random.default_rng(seed)
    B = np.linalg.qr(rng.standard_normal((D, rank)))[0].T          # [rank, D], orthonormal rows
    X = rng.standard_normal((n, rank)) @ B
    Q = rng.standard_normal((M, rank)) @ B
    X = (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)
    Q = (Q / np.linalg.norm(Q, axis=1, keepdims=True)).astype(np.float32)
    ne = n * deg // 2
    src, dst = rng.integers(0, n, ne), rng.integers(0, n, ne)
    w = rng.uniform(0.05, 1.0, ne).astype(np.float32)
    X64, Q64 = X.astype(np.float64), Q.astype(np.float64)
    cos = (Q64 @ X64.T) / (np.linalg.norm(Q64, axis=1)[:, None] * np.linalg.norm(X64, axis=1)[None, :])
    seeds = np.argsort(-cos, axis=1, kind="stable")[:, :seed_k].astype(np.int64)
    return {"X": X, "Q": Q, "seeds": seeds, "csr": csr_of(src, dst, n), "w": w,
            "kind": np.full(n, NODE, dtype=np.uint8), "sup": np.zeros(n, dtype=np.uint8),
            "bias": np.zeros(n, dtype=np.float32)}
