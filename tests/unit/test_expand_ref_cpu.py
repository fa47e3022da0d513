"""The fp64 oracle of the associative search (tests/kernels/_expand_ref.py)
against a brute-force path enumeration on tiny graphs, the torch formulation
``expand_select_ref`` against the oracle under both rules, and the left-out
count of every recipe case the GPU file uses -- a property of the oracle alone,
asserted here so the GPU test cannot be the one to find out."""
import functools

import numpy as np
import pytest
import torch

from lazzaro_amd.core.expand import GraphExpand
from lazzaro_amd.ops.expand_ops import EXPAND_SUM_DEPTH, expand_select, expand_select_ref, expand_tol, pool_bound
from tests.kernels._expand_ref import CAP, NODE, check_against_ref, csr_of, expand64, left_out, recipe

COLS = ("w", "kind", "sup", "bias")
SHAPES = [(20, 1, 8, 5), (30, 2, 4, 10), (768, 1, 8, 10), (768, 2, 7, 16), (1024, 3, 2, 16)]  # test_expand_gpu.SHAPES


@functools.lru_cache(maxsize=None)
def _case(D, M=128, n=2048, seed=0, seed_k=16):
    return recipe(D, M=M, n=n, seed=seed, seed_k=seed_k)


def _refs(c, sp):
    return expand64(c["X"], c["Q"], c["seeds"], c["csr"], *(c[k] for k in COLS), sp)


def _ref_run(c, sp, limit):
    T = torch.from_numpy
    out = expand_select_ref(T(c["X"]), T(c["Q"]), T(c["seeds"]), tuple(T(a) for a in c["csr"]), *(T(c[k]) for k in COLS),
                            sp, limit)
    return tuple(o.numpy() for o in out)


def test_tolerance_is_the_stated_depth():
    assert EXPAND_SUM_DEPTH(768) == 52 and EXPAND_SUM_DEPTH(20) == 8
    assert expand_tol(768, 2) == (2 * 52 + 8 + 2 * 2 + 6) * 2.0 ** -24
    assert pool_bound(GraphExpand(hops=2, fanout=7)) == 1024 and pool_bound(1) == 16 * 9


# ---- the oracle against all paths of length <= H
def _tiny(seed, n=12, D=6):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, D)).astype(np.float32)
    Q = rng.standard_normal((3, D)).astype(np.float32)
    na = int(rng.integers(10, 40))
    u, v = rng.integers(0, n, na), rng.integers(0, n, na)
    o = np.argsort(u, kind="stable")
    u, v = u[o], v[o]
    off = np.zeros(n + 1, dtype=np.int64)
    off[1:] = np.cumsum(np.bincount(u, minlength=n))
    ne = 8
    c = {"X": X, "Q": Q, "csr": (off, v.astype(np.int32), rng.integers(0, ne, na).astype(np.int32)),
         "w": rng.choice(np.array([0.1, 0.3, 0.5, 0.9, 1.7], dtype=np.float32), ne),
         "kind": rng.choice(np.array([NODE, NODE, NODE, 2], dtype=np.uint8), n),
         "sup": (rng.random(n) < 0.15).astype(np.uint8),
         "bias": np.where(rng.random(n) < 0.15, -np.inf, -1.0).astype(np.float32),
         "seeds": np.stack([rng.choice(n, 3, replace=False) for _ in range(3)]).astype(np.int64)}
    c["seeds"][1, 2] = c["seeds"][1, 0]  # a seed listed twice
    c["seeds"][2, 1] = -1                # an empty slot
    return c


@pytest.mark.parametrize("hops,fanout", [(1, 1), (1, 3), (2, 2), (3, 2), (3, 3)])
def test_oracle_equals_path_enumeration(hops, fanout):
    for seed in range(12):
        c = _tiny(seed)
        sp = GraphExpand(hops=hops, fanout=fanout, seed_k=3)
        refs = _refs(c, sp)
        for m, ref in enumerate(refs):
            # a walk from a seed starts with the seed's OWN activation whatever reached it later
            own = {int(r): float(o) for r, o in zip(ref.rows, ref.own)}
            want = _brute_paths(c, m, sp, own)
            assert ref.rows.tolist() == sorted(want), (seed, m)
            for r, a, v in zip(ref.rows.tolist(), ref.act.tolist(), ref.via.tolist()):
                assert a == want[r][0] and v == want[r][1], (seed, m, r, a, v, want[r])


def _brute_paths(c, m, sp, own):
    """Every path of at most ``hops`` arcs that starts at a seed with the
    seed's own activation: {row: (largest product, via)}. A path's value does
    not depend on what else reached its rows, which is what max-product in
    Jacobi order computes."""
    n = len(c["X"])
    off, adj, eid = c["csr"]
    lam = float(np.float32(sp.decay))
    seeds = sorted({int(s) for s in c["seeds"][m] if 0 <= s < n})
    best = {s: (own[s], -1) for s in seeds}

    def allowed(u):
        if c["sup"][u]:
            return []
        out = []
        for p in range(off[u], off[u + 1]):
            v, w = int(adj[p]), c["w"][eid[p]]
            if w >= np.float32(sp.min_weight) and c["kind"][v] == NODE and np.isfinite(c["bias"][v]):
                out.append((v, lam * min(float(w), 1.0)))
        return out[: sp.fanout]

    def rank(a, via):
        return (a, 1 if via < 0 else 0, -via)

    def walk(u, a, depth):
        if depth == sp.hops:
            return
        for v, f in allowed(u):
            t = a * f
            if v not in best:
                best[v] = (0.0, -1)      # reached: it starts from 0, which is its own
            if rank(t, u) > rank(*best[v]):
                best[v] = (t, u)
            walk(v, t, depth + 1)

    for s in seeds:
        walk(s, own[s], 0)
    return best


# ---- the torch formulation under both rules, and the left-out counts of the GPU file's cases
@pytest.mark.parametrize("gamma", [0.3, 0.7])
@pytest.mark.parametrize("D,hops,fanout,limit", SHAPES, ids=[f"D{d}-h{h}-f{f}-k{k}" for d, h, f, k in SHAPES])
def test_ref_on_the_recipe_shapes(D, hops, fanout, limit, gamma):
    c = _case(D)
    sp = GraphExpand(hops=hops, fanout=fanout, graph_weight=gamma)
    refs = _refs(c, sp)
    out = left_out(refs, limit, expand_tol(D, hops))
    assert len(out) <= CAP * len(refs)
    got = _ref_run(c, sp, limit)
    assert check_against_ref(c["X"], c["Q"], c["seeds"], c["csr"], *(c[k] for k in COLS), sp, limit, *got,
                             refs=refs) == len(out)


def test_left_out_counts_of_the_issue_table():
    # (D, hops, fanout, limit) -> queries of 128 left out, recipe seeds 0 and 7, graph_weight 0.5
    table = {(20, 1, 8, 10): (2, 0), (30, 2, 4, 10): (1, 0), (768, 1, 8, 10): (2, 3), (768, 2, 7, 16): (5, 5),
             (1024, 3, 2, 16): (4, 11)}
    for (D, hops, fanout, limit), want in table.items():
        sp = GraphExpand(hops=hops, fanout=fanout)
        got = tuple(len(left_out(_refs(_case(D, seed=s), sp), limit, expand_tol(D, hops))) for s in (0, 7))
        assert got == want, (D, hops, fanout, limit, got)
        assert max(got) <= CAP * 128


def test_left_out_counts_of_the_other_gpu_cases():
    def ok(c, sp, limit, skip=()):
        refs = [r for m, r in enumerate(_refs(c, sp)) if m not in skip]
        assert len(left_out(refs, limit, expand_tol(c["X"].shape[1], sp.hops))) <= CAP * len(refs)
    # test_batches_seed_counts_and_limits
    for seed_k in (1, 5, 16):
        full = _case(30 if seed_k == 5 else 20, M=130, n=512, seed=7, seed_k=seed_k)
        for M in (1, 3, 130):
            c = dict(full, Q=full["Q"][:M], seeds=full["seeds"][:M])
            for limit in (1, 10, 64):
                ok(c, GraphExpand(hops=1, fanout=2, seed_k=seed_k), limit)
    ok(_case(768, M=32), GraphExpand(hops=2, fanout=4, graph_weight=0.0), 16)      # test_gamma_zero_is_the_cosine_order
    ok(_case(768), GraphExpand(hops=1, fanout=8, graph_weight=0.7), 10)            # test_strided_and_misaligned_rows
    c = dict(_case(30, M=32, n=512, seed=5))                                       # test_zero_query_non_unit_rows_...
    c["X"] = c["X"] * np.linspace(0.25, 4.0, len(c["X"]), dtype=np.float32)[:, None]
    c["Q"] = c["Q"] * np.linspace(0.5, 3.0, len(c["Q"]), dtype=np.float32)[:, None]
    c["X"][int(c["seeds"][1, 0])] = 0.0
    ok(c, GraphExpand(hops=2, fanout=3), 10, skip=(9,))
    c = dict(_case(20, M=32, n=512, seed=3))                                       # test_empty_duplicate_and_..._seeds
    s = c["seeds"].copy()
    s[0, :] = -1
    s[1, 1:] = s[1, 0]
    s[2, [0, 2]] = [len(c["X"]) + 5, 1 << 40]
    s[3, [1, 15]] = [-7, len(c["X"])]
    c["seeds"] = s
    ok(c, GraphExpand(hops=2, fanout=3), 10)
    c = dict(_case(20, M=32, n=512, seed=3), csr=csr_of([], [], 512), w=np.zeros(0, np.float32))  # test_a_graph_without_edges_...
    ok(c, GraphExpand(hops=3, fanout=2), 16)


def test_cpu_tensors_take_the_torch_formulation_and_edges_of_the_contract():
    c = dict(_case(20, M=8, n=512, seed=3))
    T = torch.from_numpy
    args = (T(c["X"]), T(c["Q"]), T(c["seeds"]), tuple(T(a) for a in c["csr"]), *(T(c[k]) for k in COLS))
    a = expand_select(*args, dict(hops=2, fanout=4), 10)
    b = expand_select_ref(*args, GraphExpand(hops=2, fanout=4), 10)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    # no edges: the seeds by cosine, via -1 throughout
    empty = csr_of([], [], len(c["X"]))
    rows, scores, via, ncand = expand_select(args[0], args[1], args[2], tuple(T(x) for x in empty),
                                             torch.zeros(0), *args[5:], 1, 16)
    X64, Q64 = c["X"].astype(np.float64), c["Q"].astype(np.float64)
    for m in range(8):
        cos = X64[c["seeds"][m]] @ Q64[m]
        assert rows[m].tolist() == c["seeds"][m][np.argsort(-cos, kind="stable")].tolist()
    assert (via == -1).all() and (ncand == 16).all()
    # limit above the candidate count pads
    rows, scores, via, ncand = expand_select(*args, dict(hops=1, fanout=1, seed_k=16), 64)
    assert (ncand <= 32).all() and (rows[:, 32:] == -1).all() and torch.isneginf(scores[:, 32:]).all()
