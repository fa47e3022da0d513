"""``lzk_expand_select`` (csrc/kernels/expand.hip) against the fp64 oracle of
tests/kernels/_expand_ref.py: recipe shapes under both rules, hand-built graphs
whose candidate sets are asserted exactly, constructed values and layouts, and
``store_search(..., expand=)`` end to end on a GPU tenant."""
import functools

import numpy as np
import pytest
import torch

from lazzaro_amd.core.expand import GraphExpand
from lazzaro_amd.ops.expand_ops import expand_select, expand_tol
from tests.kernels._expand_ref import check_against_ref, check_rule1, exact_prefix, expand64, recipe

pytestmark = pytest.mark.gpu
DEV = "cuda"
COLS = ("w", "kind", "sup", "bias")


@functools.lru_cache(maxsize=None)
def _case(D, M=128, n=2048, seed=0, seed_k=16):
    return recipe(D, M=M, n=n, seed=seed, seed_k=seed_k)


def _run(c, spec, limit, X=None):
    """``expand_select`` on the device over the case ``c`` (a dict as
    ``recipe`` returns); ``X``: a tensor already laid out on the device."""
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    Xd = X if X is not None else T(c["X"])
    out = expand_select(Xd, T(c["Q"]), T(c["seeds"]), tuple(T(a) for a in c["csr"]), *(T(c[k]) for k in COLS),
                        spec, limit)
    rows, scores, via, ncand = out
    M = len(c["Q"])
    assert rows.dtype == via.dtype == torch.long and scores.dtype == torch.float32 and ncand.dtype == torch.int32
    assert rows.shape == scores.shape == via.shape == (M, limit) and ncand.shape == (M,)
    return tuple(o.cpu().numpy() for o in out)


def _check(c, spec, limit, got, refs=None):
    return check_against_ref(c["X"], c["Q"], c["seeds"], c["csr"], *(c[k] for k in COLS), spec, limit, *got, refs=refs)


def _refs(c, spec):
    return expand64(c["X"], c["Q"], c["seeds"], c["csr"], *(c[k] for k in COLS), spec)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


SHAPES = [(20, 1, 8, 5),       # float4 path, 5 of the 16 lanes of a group loaded
          (30, 2, 4, 10),      # scalar path
          (768, 1, 8, 10), (768, 2, 7, 16), (1024, 3, 2, 16)]


@pytest.mark.parametrize("gamma", [0.3, 0.7])
@pytest.mark.parametrize("D,hops,fanout,limit", SHAPES, ids=[f"D{d}-h{h}-f{f}-k{k}" for d, h, f, k in SHAPES])
def test_recipe_shapes(D, hops, fanout, limit, gamma):
    c = _case(D)
    sp = GraphExpand(hops=hops, fanout=fanout, graph_weight=gamma)
    got = _run(c, sp, limit)
    left = _check(c, sp, limit, got)
    print(f"D={D} hops={hops} fanout={fanout} limit={limit} gamma={gamma}: {left} of {len(c['Q'])} left out of the "
          f"exact prefix; ncand {got[3].min()} .. {got[3].max()}")


@pytest.mark.parametrize("M", [1, 3, 130])
@pytest.mark.parametrize("seed_k", [1, 5, 16])
def test_batches_seed_counts_and_limits(seed_k, M):
    c = dict(_case(30 if seed_k == 5 else 20, M=130, n=512, seed=7, seed_k=seed_k))
    c["Q"], c["seeds"] = c["Q"][:M], c["seeds"][:M]
    sp = GraphExpand(hops=1, fanout=2, seed_k=seed_k)
    refs = _refs(c, sp)
    for limit in (1, 10, 64):
        got = _run(c, sp, limit)
        _check(c, sp, limit, got, refs)
        if limit == 64:  # (at most 16 * 3 = 48 candidates: the result pads)
            assert (got[3] <= seed_k * 3).all() and (got[0][:, 48:] == -1).all()


# ---- hand-built graphs: directed arcs listed per source in CSR order, one edge per arc
def _graph(c, arcs, seeds, M=1):
    """The case ``c`` with the arcs ``[(u, v, w), ...]`` (stable-sorted by
    source here) instead of its edges, and the same ``seeds`` for M queries."""
    n = len(c["X"])
    arcs = sorted(arcs, key=lambda a: a[0])
    off = np.zeros(n + 1, dtype=np.int64)
    for u, _, _ in arcs:
        off[u + 1] += 1
    g = dict(c)
    g["csr"] = (np.cumsum(off), np.array([a[1] for a in arcs], dtype=np.int32), np.arange(len(arcs), dtype=np.int32))
    g["w"] = np.array([a[2] for a in arcs], dtype=np.float32)
    g["Q"] = c["Q"][:M]
    g["seeds"] = np.tile(np.asarray(seeds, dtype=np.int64), (M, 1))
    g["kind"], g["sup"], g["bias"] = c["kind"].copy(), c["sup"].copy(), c["bias"].copy()
    return g


def _cands(g, sp, want, limit=64):
    """Run, hold to rule 1, and assert the candidate set of query 0 exactly."""
    got = _run(g, sp, limit)
    refs = _refs(g, sp)
    check_rule1(refs, limit, *got, expand_tol(g["X"].shape[1], sp.hops))
    assert refs[0].rows.tolist() == sorted(want)  # (the oracle agrees with the hand count)
    assert got[3][0] == len(want)
    if len(want) <= limit:
        assert sorted(got[0][0][: len(want)].tolist()) == sorted(want)
    return got


def test_structure_masks_and_fanout():
    c = _case(20)
    # a seed with no arcs (9); a source (3) whose below-cut arcs are interleaved: the first 2 QUALIFYING are 12 and
    # 14, the first 2 arcs are 11 and 12; a self-loop (5); two edges 6 -> 20 with different weights; a super-node
    # source (7) that does not expand; a ghost target (30) and a target whose bias is -inf (31)
    arcs = [(3, 11, 0.1), (3, 12, 0.5), (3, 13, 0.29), (3, 14, 0.9), (3, 15, 0.8),
            (5, 5, 0.9), (5, 16, 0.6),
            (6, 20, 0.4), (6, 20, 0.95),
            (7, 21, 0.9),
            (8, 30, 0.9), (8, 31, 0.9), (8, 32, 0.9)]
    g = _graph(c, arcs, [3, 5, 6, 7, 8, 9])
    q = c["X"][[3, 5, 6, 8]].sum(0)
    g["Q"] = (q / np.linalg.norm(q))[None, :].astype(np.float32)
    assert (c["X"][[3, 5, 6, 8]] @ g["Q"][0] > 0.1).all()  # (the sources have something to hand on)
    g["sup"][7] = 1
    g["kind"][30] = 2
    g["bias"][31] = -np.inf
    sp = GraphExpand(hops=1, fanout=2, seed_k=6)
    rows, scores, via, ncand = _cands(g, sp, [3, 5, 6, 7, 8, 9, 12, 14, 16, 20, 32])
    v = dict(zip(rows[0].tolist(), via[0].tolist()))
    assert v[12] == v[14] == 3 and v[16] == 5 and v[20] == 6 and v[32] == 8
    assert all(v[s] == -1 for s in (3, 6, 7, 8, 9))
    # the self-loop proposes less than the row's own activation -- or 0 = 0, where own wins the tie
    assert v[5] == -1
    # the heavier of the two parallel edges carries row 20: its fp64 activation is act(6) * 0.85 * 0.95
    r = _refs(g, sp)[0]
    a = dict(zip(r.rows.tolist(), r.act.tolist()))
    assert a[20] == pytest.approx(a[6] * float(np.float32(0.85)) * float(np.float32(0.95)), rel=1e-12)


def test_hub_contention_resolves_to_the_lowest_source():
    c = _case(20)
    q0 = c["Q"][0].astype(np.float64)
    cos = c["X"].astype(np.float64) @ q0
    seeds = np.argsort(-cos)[:16]                       # positive cosines
    hub = int(np.argsort(-cos)[40])
    X = c["X"].copy()
    for s in seeds:                                     # every seed the same row: equal activations as bits
        X[s] = c["X"][seeds[0]]
    c2 = dict(c, X=X)
    g = _graph(c2, [(int(s), hub, 1.0) for s in seeds], seeds, M=3)
    g["Q"] = c["Q"][[0, 0, 0]]
    sp = GraphExpand(hops=1, fanout=1, decay=1.0)
    rows, scores, via, ncand = _cands(g, sp, list(map(int, seeds)) + [hub], limit=32)
    for m in range(3):
        at = rows[m].tolist().index(hub)
        assert via[m, at] == seeds.min()                # 16 equal proposals: the lowest source row


def test_the_largest_reachable_table():
    # 16 seeds, fanout 7, 2 hops, all targets distinct. A source takes the same arcs in every hop, so the seeds add
    # nothing in hop 2: 16 * (1 + 7 + 49) = 912 candidates is the most this setting can reach (the table holds 1024)
    c = _case(20)
    arcs, nxt = [], 16
    level = list(range(16))
    for _ in range(2):
        new = []
        for u in level:
            for _ in range(7):
                arcs.append((u, nxt, 0.5 + 0.4 * ((nxt * 7) % 10) / 10))
                new.append(nxt)
                nxt += 1
        level = new
    assert nxt == 912 <= len(c["X"])
    g = _graph(c, arcs, list(range(16)), M=2)
    sp = GraphExpand(hops=2, fanout=7)
    assert sp.pool == 1024
    got = _cands(g, sp, list(range(912)))
    assert (got[3] == 912).all()
    _check(g, sp, 64, got)


def test_jacobi_order():
    c = _case(20)
    a, b, d, e = 100, 101, 102, 103
    # chain a -> b -> d: one hop reaches b, two reach d
    chain = _graph(c, [(a, b, 0.9), (b, d, 0.9)], [a])
    _cands(chain, GraphExpand(hops=1, seed_k=1), [a, b])
    _cands(chain, GraphExpand(hops=2, seed_k=1), [a, b, d])
    # e is first reached in hop 1 over a weak arc from a, and improved in hop 2 through b:
    # 0.9 * 0.9 * decay^2 > 0.31 * decay. With Gauss-Seidel order one hop would already reach d
    g = _graph(c, [(a, e, 0.31), (a, b, 0.9), (b, e, 0.9), (e, d, 0.9)], [a])
    g["Q"] = c["X"][a:a + 1].copy()                     # cos(q, a) = 1
    r1 = _cands(g, GraphExpand(hops=1, seed_k=1), [a, b, e])
    r2 = _cands(g, GraphExpand(hops=2, seed_k=1), [a, b, e, d])
    via1 = dict(zip(r1[0][0].tolist(), r1[2][0].tolist()))
    via2 = dict(zip(r2[0][0].tolist(), r2[2][0].tolist()))
    assert via1[e] == a and via2[e] == b and via2[d] == e and via2[b] == a and via2[a] == -1


# ---- values
def test_gamma_zero_is_the_cosine_order():
    c = _case(768, M=32)
    sp = GraphExpand(hops=2, fanout=4, graph_weight=0.0)
    got = _run(c, sp, 16)
    _check(c, sp, 16, got)
    X, Q = c["X"].astype(np.float64), c["Q"].astype(np.float64)
    for m in range(len(Q)):
        cos = X[got[0][m]] @ Q[m] / (np.linalg.norm(X[got[0][m]], axis=1) * np.linalg.norm(Q[m]))
        assert np.abs(cos - got[1][m]).max() <= expand_tol(768, 2)


def test_gamma_one_copies_the_activation_bit_for_bit():
    c = _case(20)
    a, b, d = 300, 200, 100
    g = _graph(c, [(a, b, 1.5), (b, d, 2.0)], [a])
    g["Q"] = (c["X"][a:a + 1] + 0.5 * c["X"][7:8]).astype(np.float32)
    sp = GraphExpand(hops=2, seed_k=1, decay=1.0, graph_weight=1.0)
    rows, scores, via, ncand = _cands(g, sp, [a, b, d], limit=5)
    # weights clamp to 1 and decay is 1: the three scores are one bit pattern, and the lower row goes first
    assert rows[0].tolist() == [d, b, a, -1, -1]
    assert len(set(_bits(scores[0, :3]).tolist())) == 1 and scores[0, 0] > 0
    assert via[0].tolist() == [b, a, -1, -1, -1]


def test_zero_query_non_unit_rows_and_a_zero_row():
    c = dict(_case(30, M=32, n=512, seed=5))
    c["X"] = c["X"] * np.linspace(0.25, 4.0, len(c["X"]), dtype=np.float32)[:, None]
    c["Q"] = c["Q"] * np.linspace(0.5, 3.0, len(c["Q"]), dtype=np.float32)[:, None]
    c["X"][int(c["seeds"][1, 0])] = 0.0                 # the nearest row of query 1: cosine 0 by the norm rule
    c["Q"][9] = 0.0                                     # every cosine and activation 0: ascending rows
    sp = GraphExpand(hops=2, fanout=3)
    refs = _refs(c, sp)
    got = _run(c, sp, 10)
    check_rule1(refs, 10, *got, expand_tol(30, 2))      # (query 9 ties throughout: rule 1, rows asserted here)
    assert np.isfinite(got[1]).all()
    assert got[0][9].tolist() == refs[9].rows[:10].tolist() and (got[1][9] == 0).all() and (got[2][9] == -1).all()
    keep = [m for m in range(32) if m != 9]
    c2 = dict(c, Q=c["Q"][keep], seeds=c["seeds"][keep])
    _check(c2, sp, 10, tuple(o[keep] for o in got), [refs[m] for m in keep])


def test_identical_rows_tie_to_the_lower_row_bit_for_bit():
    c = dict(_case(768, M=8))
    n = len(c["X"])
    s0 = int(c["seeds"][0, 0])
    far = int(np.argmin(c["X"].astype(np.float64) @ c["Q"][0].astype(np.float64)))
    v = c["X"][far]
    c["X"] = np.concatenate([c["X"], v[None], v[None], v[None]])      # one vector at rows n, n + 1, n + 2
    for k in ("kind", "sup", "bias"):
        c[k] = np.concatenate([c[k], c[k][:3]])
    g = _graph(c, [(s0, n + 2, 0.7), (s0, n, 0.7), (s0, n + 1, 0.7)], [s0])
    sp = GraphExpand(hops=1, seed_k=1)
    rows, scores, via, ncand = _cands(g, sp, [s0, n, n + 1, n + 2], limit=4)
    assert rows[0].tolist() == [s0, n, n + 1, n + 2]
    assert len(set(_bits(scores[0, 1:]).tolist())) == 1


def test_strided_and_misaligned_rows():
    D, limit = 768, 10
    c = _case(D)
    sp = GraphExpand(hops=1, fanout=8, graph_weight=0.7)
    refs = _refs(c, sp)
    n = len(c["X"])
    base = _run(c, sp, limit)
    _check(c, sp, limit, base, refs)
    Xt = torch.from_numpy(c["X"])

    def same(a, b):
        return all(np.array_equal(x, y) for x, y in zip((a[0], _bits(a[1]), a[2], a[3]), (b[0], _bits(b[1]), b[2], b[3])))
    # ldx > D, still 16-byte rows: the float4 path again, bit for bit
    wide = torch.full((n, D + 8), 7.0, device=DEV)
    wide[:, :D] = Xt.to(DEV)
    assert same(_run(c, sp, limit, wide[:, :D]), base)
    # an odd row stride, and a base 4 bytes off a 16-byte boundary: the scalar path at D % 4 == 0
    odd = torch.full((n, D + 3), 7.0, device=DEV)
    odd[:, :D] = Xt.to(DEV)
    flat = torch.full((n * D + 1,), 7.0, device=DEV)
    off = flat[1:].view(n, D)
    off.copy_(Xt)
    assert off.data_ptr() % 16 == 4
    a = _run(c, sp, limit, odd[:, :D])
    b = _run(c, sp, limit, off)
    _check(c, sp, limit, a, refs)
    assert same(a, b)


def test_empty_duplicate_and_out_of_range_seeds():
    c = dict(_case(20, M=32, n=512, seed=3))
    n = len(c["X"])
    s = c["seeds"].copy()
    s[0, :] = -1                              # no seed: no candidate
    s[1, 1:] = s[1, 0]                        # one row 16 times: one entry
    s[2, [0, 2]] = [n + 5, 1 << 40]           # rows the graph does not have: empty, never read
    s[3, [1, 15]] = [-7, n]
    c["seeds"] = s
    sp = GraphExpand(hops=2, fanout=3)
    got = _run(c, sp, 10)
    _check(c, sp, 10, got)
    assert got[3][0] == 0 and (got[0][0] == -1).all() and np.isneginf(got[1][0]).all()


def test_rows_that_collide_in_the_table_hash_are_separate_entries():
    """Two pairs of rows whose first probe is the same slot of the row table
    (Knuth's multiplier, the top 11 bits: csrc/include/lzk_rowset.h). (a, a2):
    a seed, listed twice, and the target it reaches in the hop. (b, b2): two
    seeds inserted side by side. Each row is one entry."""
    c = _case(20)
    ok = np.flatnonzero((c["kind"] == 1) & (c["sup"] == 0) & np.isfinite(c["bias"]))
    h = ((ok.astype(np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(21)
    full = np.flatnonzero(np.bincount(h.astype(np.int64), minlength=2048) >= 2)
    assert full.size >= 2, "no two pairs of rows share a slot: the case does not test the probing"
    (a, a2), (b, b2) = (ok[h == s][:2].tolist() for s in full[:2])
    g = _graph(c, [(a, a2, 0.9), (b, a2, 0.8)], [a, b, b2, a])
    rows, scores, via, ncand = _cands(g, GraphExpand(hops=1, fanout=2, seed_k=4), [a, a2, b, b2])
    assert (rows[0][4:] == -1).all()


def test_a_graph_without_edges_returns_the_seeds_by_cosine():
    c = _graph(_case(20, M=32, n=512, seed=3), [], [0], M=32)   # (empty adj, eid and w: null pointers on the device)
    c["seeds"] = _case(20, M=32, n=512, seed=3)["seeds"]
    sp = GraphExpand(hops=3, fanout=2)
    rows, scores, via, ncand = _run(c, sp, 16)
    _check(c, sp, 16, (rows, scores, via, ncand))
    assert (ncand == 16).all() and (via == -1).all()
    assert all(sorted(rows[m].tolist()) == sorted(c["seeds"][m].tolist()) for m in range(32))


def test_invalid_arguments_are_refused():
    c = _case(20, M=32, n=512, seed=3)
    for bad in (dict(hops=0), dict(hops=4), dict(fanout=17), dict(fanout=0), dict(seed_k=17), dict(hops=3, fanout=4),
                dict(decay=0.0), dict(decay=1.5), dict(graph_weight=-0.1), dict(graph_weight=1.5),
                dict(min_weight=-1.0)):
        with pytest.raises(ValueError):
            _run(c, bad, 10)
    for limit in (0, 65):
        with pytest.raises(ValueError):
            _run(c, 1, limit)
    with pytest.raises(ValueError):           # more seeds per query than seed_k
        _run(c, dict(seed_k=8), 10)
    from lazzaro_amd.ops import _lib
    L = _lib.lib()
    z = torch.zeros(64, device=DEV)
    zl = torch.zeros(64, dtype=torch.long, device=DEV)
    out, via = (torch.full((64,), -5, dtype=torch.long, device=DEV) for _ in range(2))
    sc = torch.zeros(64, device=DEV)
    nc = torch.zeros(4, dtype=torch.int32, device=DEV)
    INVALID = 1  # hipErrorInvalidValue

    def call(D=4, S=4, hops=1, fanout=2, min_w=0.3, decay=0.85, gamma=0.5, limit=4, n=4, ldx=4):
        return L.lzk_expand_select(z.data_ptr(), ldx, n, z.data_ptr(), 4, 1, D, zl.data_ptr(), S, zl.data_ptr(), 0, 0, 0,
                                   0, 0, zl.data_ptr(), zl.data_ptr(), z.data_ptr(), hops, fanout, min_w, decay, gamma,
                                   limit, out.data_ptr(), sc.data_ptr(), via.data_ptr(), nc.data_ptr(),
                                   _lib.stream_ptr(z.device))
    for bad in (dict(hops=0), dict(hops=4), dict(fanout=17), dict(S=17), dict(S=0), dict(S=16, hops=3, fanout=4),
                dict(limit=65), dict(limit=0), dict(decay=0.0), dict(gamma=float("nan")), dict(min_w=-1.0), dict(D=0),
                dict(D=4096), dict(n=1 << 31), dict(ldx=2)):
        assert call(**bad) == INVALID, bad
    torch.cuda.synchronize()
    assert (out == -5).all()  # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert out[:4].tolist() == [0, -1, -1, -1] and nc[0] == 1  # (all seeds are row 0: one candidate, then padding)


# ---- end to end
def test_store_search_with_expand_on_a_gpu_tenant():
    from lazzaro_amd.engine.tenant_graph import TenantGraph
    N, D, k = 4096, 96, 10
    gen = torch.Generator().manual_seed(21)
    X = torch.nn.functional.normalize(torch.randn(N, D, generator=gen), dim=1)
    g = TenantGraph(device=DEV, dim=D, capacity=N + 64)
    sh = g.shard_id("w")
    g.add_nodes([f"m{i}" for i in range(N)], [f"c{i}" for i in range(N)], X, shard=sh,
                types=["preference" if i % 3 == 0 else "semantic" for i in range(N)], stored=True)
    rng = np.random.default_rng(5)
    ne = 3 * N
    src, dst = rng.integers(0, N, ne), rng.integers(0, N, ne)
    w = rng.uniform(0.05, 1.0, ne).astype(np.float32)
    g.append_edges_host(src, dst, w, np.full(ne, sh), g.etype("relates_to"))
    g.take_dirty_rows(), g.take_dirty_edges(), g.take_deleted()
    Qall = torch.nn.functional.normalize(X[:64] + 0.5 * torch.randn(64, D, generator=gen), dim=1).to(DEV)
    sp = GraphExpand(hops=2, fanout=4)
    Xn = X.numpy()

    def oracle_check(Q, where, s, r, via, limit):
        _, seeds = g.store_search(Q, sp.seed_k, "l2", node_rows=True, where=where)
        n = g.n
        bias = g.store_bias("l2").cpu().numpy()
        if where is not None:
            bias = np.where(np.arange(n) % 3 == 0, bias, -np.inf).astype(np.float32)
        csr = tuple(t.cpu().numpy() for t in g.csr())
        refs = expand64(Xn, Q.cpu().numpy(), seeds.cpu().numpy(), csr, g.e["w"].cpu().numpy(),
                        g.kind[:n].cpu().numpy(), g.sup[:n].cpu().numpy(), bias, sp)
        ncand = np.array([x.rows.size for x in refs])
        tol = expand_tol(D, sp.hops)
        check_rule1(refs, limit, r.cpu().numpy(), s.cpu().numpy(), via.cpu().numpy(), ncand, tol)
        for m, ref in enumerate(refs):  # rule 2's exact prefix, query by query (no cap: M = 1 has no 10 %)
            p = min(exact_prefix(ref, limit, tol), ref.rows.size)
            assert r[m, :p].tolist() == ref.rows[ref.order[:p]].tolist(), m
        return refs

    n0 = g.expanded_searches
    runs = 0
    for M in (1, 64):
        Q = Qall[:M]
        for where in (None, {"types": ["preference"]}):
            plain = g.store_search(Q, k, "l2", where=where)
            again = g.store_search(Q, k, "l2", where=where, expand=None)
            assert torch.equal(plain[0].view(torch.int32), again[0].view(torch.int32)) and torch.equal(plain[1], again[1])
            s, r = g.store_search(Q, k, "l2", where=where, expand=sp)
            s3, r3, via = g.store_search_expand(Q, k, "l2", where=where, expand=sp)
            runs += 2
            assert torch.equal(r, r3) and torch.equal(s.view(torch.int32), s3.view(torch.int32))
            refs = oracle_check(Q, where, s, r, via, k)
            if where is not None:
                assert (r[r >= 0] % 3 == 0).all()
                assert all((x.rows % 3 == 0).all() for x in refs)  # a failing neighbour is not a candidate
            # with diversity=, the MMR pool is the expanded search at fetch_k
            ps, pr = g.store_search(Q, 24, "l2", where=where, expand=sp)
            ds, dr = g.store_search(Q, 5, "l2", where=where, diversity=0.5, fetch_k=24, expand=sp)
            runs += 2
            from lazzaro_amd.ops.mmr_ops import mmr_select
            pick, _ = mmr_select(g.emb32[: g.n], Q, pr, 5, 0.5)
            assert (pick >= 0).all()
            assert torch.equal(dr, torch.gather(pr, 1, pick.long()))
            assert torch.equal(ds.view(torch.int32), torch.gather(ps, 1, pick.long()).view(torch.int32))
    assert g.expanded_searches - n0 == runs
    assert g.search_ids(Qall[:3], k, "l2", expand=sp) == \
        [[f"m{i}" for i in row if i >= 0] for row in g.store_search(Qall[:3], k, "l2", expand=sp)[1].tolist()]
    # a new arc is seen by the next search (the CSR is cached per edge version)
    Q = Qall[:1]
    one = GraphExpand(hops=1, fanout=16, seed_k=1, min_weight=0.0)
    s, r, via = g.store_search_expand(Q, 64, "l2", expand=one)
    seed = int(g.store_search(Q, 1, "l2")[1][0, 0])
    have = set(r[0][r[0] >= 0].tolist())
    off = g.csr()[0]
    assert int(off[seed + 1] - off[seed]) < 16            # (room under the fanout for one more arc)
    new = next(i for i in range(N) if i not in have)
    g.append_edges_host([seed], [new], np.array([0.9], np.float32), np.array([sh]), g.etype("relates_to"))
    s2, r2, via2 = g.store_search_expand(Q, 64, "l2", expand=one)
    assert set(r2[0][r2[0] >= 0].tolist()) == have | {new}
    assert via2[0][r2[0] == new].item() == seed
