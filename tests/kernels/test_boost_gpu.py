"""Boosted search (``boost=``) on the GPU: the column kernel
(csrc/kernels/boost.hip) against the fp64 oracle bit for bit, every search
route a boosted column can take on an exact-grid tenant (scores and rows bit
for bit against ``boosted_topk_ref``), non-grid data under the rounding bound,
the int8 certificate's own contract under a boosted bias, and the composition
with ``where=`` / ``diversity=`` / ``expand=`` end to end
(tests/kernels/_boost_ref.py; the contract is ops/boost_ops.py's docstring).

The int8 scans exist for padded widths that are multiples of 128 only
(``TenantGraph._lowp_mode``), so the int8 and lean routes run on a D = 128
tenant whose rows are the same grid rows -- +-1/8 over 64 dimensions -- zero
beyond them: still unit, every score still a multiple of 1/64, and the int8
copy of such a row is exact (+-127 at scale 1/1016). Every other route runs at
D = 64.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from lazzaro_amd.core.boost import MemoryBoost  # noqa: E402
from lazzaro_amd.core.filters import MemoryFilter  # noqa: E402
from lazzaro_amd.engine import tenant_graph as TG  # noqa: E402
from lazzaro_amd.engine.tenant_graph import NODE, TenantGraph  # noqa: E402
from lazzaro_amd.ops import boost_ops as BO  # noqa: E402
from tests.kernels import _boost_ref as R  # noqa: E402

DEV = "cuda"
NOW = 1_700_000_000.0
N, K = 4096, 10
GRID_STRIDE_ROWS = 2048 * 256 * 4  # boost.hip: MAX_BLOCKS x NTB x RPT rows per pass of the grid
SIZES = (1, 3, 255, 256, 257, 1023, 4099, (1 << 20) + 5, GRID_STRIDE_ROWS + 1027)
WEIGHTS = dict(w_sal=0.7, w_freq=0.4, w_rec=1.3)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _edge(n):
    return R.edge_rows(n, NOW)


# ------------------------------------------------------------------ the kernel against the oracle
@pytest.mark.parametrize("n", SIZES)
def test_kernel_matches_oracle_bitwise(n):
    """Every size (none but 256 and 4099 - 3 a multiple of the 4 rows a thread
    takes; the last strides the grid), every edge row, with and without the
    type table, both ``c``, two scales, and a ``base`` view one element into
    its buffer (the 4-byte path)."""
    base, sal, acc, t, kind, tcode = _edge(n)
    assert GRID_STRIDE_ROWS < SIZES[-1] and any(s % 4 for s in SIZES)
    tw = np.zeros(256)
    tw[0], tw[1], tw[254] = 0.25, 0.0, 1.5
    d = {k: _dev(v) for k, v in dict(sal=sal, acc=acc, t=t, kind=kind, tcode=tcode).items()}
    buf = torch.empty(n + 1, dtype=torch.float32, device=DEV)
    buf[1:] = _dev(base)
    views = {"aligned": _dev(base), "offset": buf[1:]}
    assert views["offset"].data_ptr() % 16 == 4 and views["aligned"].data_ptr() % 16 == 0
    big = n > 10000  # (the oracle's own time: the two long columns take one ``c`` and one scale)
    for types in (False, True):
        for c in ((2.0,) if big else (1.0, 2.0)):
            for scale in ((86400.0,) if big else (86400.0, 1e-3)):
                want = R.boost_column_ref(base, sal, acc, t, kind, NOW, scale=scale, c=c,
                                          tcode=tcode if types else None, tw=tw if types else None, **WEIGHTS)
                assert not np.isnan(want).any()
                for name, b in views.items():
                    got = BO.boost_bias(b, d["sal"], d["acc"], d["t"], d["kind"], n, scale=scale, now=NOW, c=c,
                                        tcode=d["tcode"] if types else None, tw=list(tw) if types else None,
                                        **WEIGHTS).cpu().numpy()
                    bad = np.flatnonzero(_bits(got) != _bits(want))
                    assert bad.size == 0, (name, types, c, scale, bad[:8], got[bad[:8]], want[bad[:8]])
    # the edge rows did what they are there for
    w = R.boost_column_ref(base, sal, acc, t, kind, NOW, scale=86400.0, c=1.0, **WEIGHTS)
    assert np.isneginf(w[kind != NODE]).all() and np.isneginf(w[np.isneginf(base)]).all()
    nan = np.isnan(sal) & (kind == NODE) & np.isfinite(base)
    assert np.array_equal(_bits(w[nan]), _bits(base[nan]))  # no prior, not a NaN


def test_zero_weights_reproduce_the_base_on_node_rows():
    base, sal, acc, t, kind, _ = _edge(4099)
    got = BO.boost_bias(_dev(base), _dev(sal), _dev(acc), _dev(t), _dev(kind), 4099, 0.0, 0.0, 0.0, 86400.0, NOW,
                        2.0).cpu().numpy()
    node = kind == NODE  # (0 * inf is a NaN B: no prior either)
    assert np.array_equal(_bits(got[node]), _bits(base[node] + np.float32(0.0)))
    assert np.isneginf(got[~node]).all()


# ------------------------------------------------------------------ grid tenants
def _tenant(D, seed=7, lean=False):
    """4,096 grid rows: 3,968 memories with the grid's columns, then 64 ghosts
    and 64 nodes that are not in the store; with a few links for ``expand=``."""
    rng = np.random.default_rng(seed)
    X = R.grid_rows(rng, N, D)
    meta = R.grid_meta(rng, N)
    saved = TG.LEAN_HBM
    TG.LEAN_HBM = bool(lean)  # (read when the columns are allocated; the caller lowered LOWP_MIN_ROWS)
    try:
        g = TenantGraph(device=DEV, dim=D, capacity=N)
    finally:
        TG.LEAN_HBM = saved
    m, gh = N - 128, 64
    T = torch.from_numpy
    cols = dict(sal=T(meta["sal"]), acc=T(meta["acc"]), last=T(meta["last"]), ts=T(meta["ts"]))
    types = [R.GRID_TYPES[c] for c in meta["tcode"]]
    sh = g.shard_id("w")
    g.add_nodes([f"m{i}" for i in range(m)], ["c"] * m, T(X[:m]), shard=sh, types=types[:m], stored=True,
                **{k: v[:m] for k, v in cols.items()})
    g.add_nodes([f"g{i}" for i in range(gh)], ["ghost"] * gh, T(X[m:m + gh]), shard=g.shard_id("w", live=False),
                stored=True, ghost=True, **{k: v[m:m + gh] for k, v in cols.items()})
    g.add_nodes([f"u{i}" for i in range(N - m - gh)], ["unstored"] * (N - m - gh), T(X[m + gh:]), shard=sh,
                types=types[m + gh:], stored=False, **{k: v[m + gh:] for k, v in cols.items()})
    src = rng.integers(0, m, size=3 * m)
    dst = rng.integers(0, m, size=3 * m)
    keep = src != dst
    g.append_edges_host(src[keep], dst[keep], rng.choice(np.array([0.5, 1.0], np.float32), size=int(keep.sum())),
                        np.full(int(keep.sum()), sh), g.etype("relates_to"))
    g.take_dirty_rows(), g.take_dirty_edges(), g.take_deleted()
    assert g.n == N and g.unit_rows() and g.lean == lean
    Q = R.grid_rows(rng, 128, D, dup=0)
    Q[:8] = X[[0, 2, 4, N - 1, N - 4, 900, 901, m + 3]]  # planted duplicates (exact ties), a ghost's vector
    kind = g.kind[:N].cpu().numpy()
    assert (kind[m:m + gh] != NODE).all() and (kind[:m] == NODE).all()
    return g, X, meta, torch.from_numpy(Q).to(DEV), kind


@pytest.fixture(scope="module")
def t64():
    return _tenant(64)


@pytest.fixture(scope="module")
def t128():
    return _tenant(128)


def _column(g, meta, kind, metric, where=None, clock="accessed", types=True):
    """The oracle's column over the tenant's own base: the store bias, masked
    by hand for ``where`` (independent of filter_ops)."""
    base = g.store_bias("l2" if metric == "l2" else "ip").cpu().numpy().copy()
    if where is not None:
        base[~where] = -np.inf
    return R.grid_column(base, meta, kind, metric, clock, types)


def _check_exact(g, X, Q, col, metric, k, s, r):
    S, Rr = R.boosted_topk_ref(X, Q.cpu().numpy(), col, metric, k)
    r, s = r.cpu().numpy(), s.cpu().numpy()
    assert np.array_equal(r, Rr), np.flatnonzero((r != Rr).any(1))[:8]
    assert np.array_equal(s.astype(np.float64), S)  # (every key is exact in fp32)
    assert (r >= 0).all() and (g.kind[:N].cpu().numpy()[r] == NODE).all()


def _spy(monkeypatch, g):
    calls = {"i8": 0, "bf16": 0, "exact": 0, "sparse": 0}
    import lazzaro_amd.ops.filter_ops as FO
    import lazzaro_amd.ops.search as S

    def count(obj, attr, key):
        fn = getattr(obj, attr)

        def wrapped(*a, **kw):
            calls[key] += 1
            return fn(*a, **kw)
        monkeypatch.setattr(obj, attr, wrapped)
    count(g, "_i8_candidates", "i8")
    count(g, "_exact_store", "exact")
    count(S, "flat_topk", "bf16")
    count(FO, "gather_topk", "sparse")
    return calls


def _took(calls):
    return {k for k, v in calls.items() if v}


@pytest.mark.parametrize("clock", ["accessed", "created"])
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_boost_bias_stage_both_clocks(t64, metric, clock):
    g, X, meta, Q, kind = t64
    b = dict(R.GRID_BOOST, clock=clock)
    got = g.boost_bias(b, metric).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(_column(g, meta, kind, metric, clock=clock)))
    built = g.boost_columns_built
    assert g.boost_bias(b, metric).data_ptr() == g.boost_bias(MemoryBoost(**b), metric).data_ptr()
    assert g.boost_columns_built == built  # (the same settings and ``now``: one column)
    keys = R.keys_ref(X, Q.cpu().numpy(), got, metric) * 64.0
    fin = np.isfinite(keys)
    assert np.array_equal(keys[fin], np.rint(keys[fin]))  # the grid's exactness claim, on this tenant


@pytest.mark.parametrize("metric", ["l2", "ip", "cosine"])
def test_flat_bf16_route_exact(t64, monkeypatch, metric):
    g, X, meta, Q, kind = t64
    calls = _spy(monkeypatch, g)
    M = 64
    assert M * N >= TG.KERNEL_MIN_WORK // 16
    s, r = g.store_search(Q[:M], K, metric, boost=R.GRID_BOOST)
    assert _took(calls) == {"bf16"}
    _check_exact(g, X, Q[:M], _column(g, meta, kind, metric), metric, K, s, r)


@pytest.mark.parametrize("M", [1, 8, 128])
@pytest.mark.parametrize("lean", [False, True])
def test_int8_routes_exact(t128, monkeypatch, M, lean):
    """The narrow int8 scan (M = 1, 8) and the wide one (M = 128, worst-case
    margins), over bf16 rows and on a lean tenant."""
    monkeypatch.setattr(TG, "LOWP_MIN_ROWS", 1024)
    monkeypatch.setattr(TG, "KERNEL_MIN_WORK", 16)  # (M = 1: 4,096 rows are kernel work)
    g, X, meta, Q, kind = _tenant(128, lean=True) if lean else t128
    monkeypatch.setattr(g, "LOWP_EXACT_MODE", "1", raising=False)
    calls = _spy(monkeypatch, g)
    s, r = g.store_search(Q[:M], K, "l2", boost=R.GRID_BOOST)
    assert _took(calls) == {"i8"}
    _check_exact(g, X, Q[:M], _column(g, meta, kind, "l2"), "l2", K, s, r)


FILTER = MemoryFilter(min_salience=0.875, min_access_count=20)


@pytest.mark.parametrize("route", ["sparse", "dense"])
def test_filtered_routes_exact(t64, monkeypatch, route):
    g, X, meta, Q, kind = t64
    if route == "dense":
        monkeypatch.setattr(TG, "FILTER_SPARSE_MAX_ROWS", 0)
    calls = _spy(monkeypatch, g)
    stored = g.stored[:N].cpu().numpy() == 1
    ok = (kind == NODE) & stored & (meta["sal"] >= 0.875) & (meta["acc"] >= 20)
    assert 150 <= ok.sum() <= 300
    M = 64
    for metric in ("l2", "cosine"):
        s, r = g.store_search(Q[:M], K, metric, where=FILTER, boost=R.GRID_BOOST)
        _check_exact(g, X, Q[:M], _column(g, meta, kind, metric, where=ok), metric, K, s, r)
        assert ok[r.cpu().numpy()].all()
    assert _took(calls) == ({"sparse"} if route == "sparse" else {"bf16"})


def test_k32_exact_store(t64, monkeypatch):
    g, X, meta, Q, kind = t64
    calls = _spy(monkeypatch, g)
    s, r = g.store_search(Q[:16], 32, "l2", boost=R.GRID_BOOST)
    assert _took(calls) == {"exact"}
    _check_exact(g, X, Q[:16], _column(g, meta, kind, "l2"), "l2", 32, s, r)


def test_zero_boost_is_the_empty_filter_and_none_is_plain(t64):
    g, X, meta, Q, kind = t64
    a = g.store_search(Q[:64], K, "l2", where=MemoryFilter())
    b = g.store_search(Q[:64], K, "l2", boost=0.0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    n0 = g.boosted_searches
    p = g.store_search(Q[:64], K, "l2", node_rows=True)
    q = g.store_search(Q[:64], K, "l2", node_rows=True, boost=None)
    assert torch.equal(p[0], q[0]) and torch.equal(p[1], q[1]) and g.boosted_searches == n0


def test_ivfpq_tenant_goes_flat(monkeypatch):
    """A tenant with an IVF-PQ index, ``ivf_filtered`` included: a boosted
    search never asks the index."""
    g, X, meta, Q, kind = _tenant(64, seed=9)
    g.ann_cfg = {"nlist": 16, "nprobe": 16, "m": 8, "min_rows": 1024, "rerank": 1024, "filtered": True}
    monkeypatch.setattr(TG, "FILTER_SPARSE_MAX_ROWS", 0)

    def boom(*a, **kw):
        raise AssertionError("a boosted search reached the IVF-PQ index")
    monkeypatch.setattr(g, "_ann_candidates", boom)
    s, r = g.store_search(Q[:64], K, "l2", boost=R.GRID_BOOST)
    _check_exact(g, X, Q[:64], _column(g, meta, kind, "l2"), "l2", K, s, r)
    ok = (kind == NODE) & (g.stored[:N].cpu().numpy() == 1) & (meta["sal"] >= 0.5)
    s, r = g.store_search(Q[:64], K, "l2", where={"min_salience": 0.5}, boost=R.GRID_BOOST)
    _check_exact(g, X, Q[:64], _column(g, meta, kind, "l2", where=ok), "l2", K, s, r)
    assert g.filtered_ann == 0


# ------------------------------------------------------------------ non-grid data
def _gauss_tenant(D, unit, seed):
    from tests.kernels._cand_ref import to_bf16
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, D)) * (1.0 if unit else 0.4)
    if unit:
        X /= np.linalg.norm(X, axis=1, keepdims=True)
    X = to_bf16(X).astype(np.float32)  # (the bf16 candidate scan sees exact operands)
    Q = to_bf16(rng.standard_normal((64, D)) * (1.0 if not unit else 1.0 / np.sqrt(D))).astype(np.float32)
    sal = rng.random(N).astype(np.float32)
    acc = rng.integers(0, 25, size=N).astype(np.int32)
    last = NOW - rng.random(N) * 10 * 86400.0
    g = TenantGraph(device=DEV, dim=D, capacity=N)
    T = torch.from_numpy
    g.add_nodes([f"m{i}" for i in range(N)], ["c"] * N, T(X), shard=g.shard_id("w"), sal=T(sal), acc=T(acc),
                last=T(last), ts=T(last), stored=True)
    return g, X, torch.from_numpy(Q).to(DEV), sal, acc, last


def test_non_grid_l2_within_the_rounding_bound(monkeypatch):
    """Gaussian non-unit rows, L2, the flat bf16 route: every returned score
    within the bound of its row's fp64 key, and no row left out whose fp64 key
    exceeds the k-th returned key by more than the two rows' bounds. No query
    is excused."""
    g, X, Q, sal, acc, last = _gauss_tenant(64, False, 21)
    assert not g.unit_rows()
    calls = _spy(monkeypatch, g)
    b = MemoryBoost(salience=0.5, frequency=0.3, recency=0.2, now=NOW)
    s, r = g.store_search(Q, K, "l2", boost=b)
    assert _took(calls) == {"bf16"}
    base = g.store_bias("l2").cpu().numpy()
    kind = g.kind[:N].cpu().numpy()
    prior = R.boost_prior_ref(sal, acc, last, NOW, 0.5, 0.3, 0.2, 86400.0, 2.0)
    col = R.boost_bias_ref(base, kind, prior)
    assert np.array_equal(_bits(g.boost_bias(b, "l2").cpu().numpy()), _bits(col))
    Qn = Q.cpu().numpy()
    keys = 2.0 * Qn.astype(np.float64) @ X.astype(np.float64).T - (Qn.astype(np.float64) ** 2).sum(1)[:, None] \
        + base.astype(np.float64)[None, :] + prior.astype(np.float64)[None, :]
    bound = R.score_bound(X, Qn, base, prior, "l2")
    s, r = s.cpu().numpy().astype(np.float64), r.cpu().numpy()
    assert (r >= 0).all()
    for q in range(Qn.shape[0]):
        assert len(set(r[q].tolist())) == K
        err = np.abs(s[q] - keys[q, r[q]])
        print(f"q{q}: worst score error {err.max():.3e} of bound {bound[q, r[q]].min():.3e}")
        assert (err <= bound[q, r[q]]).all(), (q, err, bound[q, r[q]])
        assert (np.diff(s[q]) <= 0).all()
        kth = r[q, np.argmin(keys[q, r[q]])]
        out = np.ones(N, dtype=bool)
        out[r[q]] = False
        over = keys[q] - keys[q, kth] - (bound[q] + bound[q, kth])
        assert not (over[out] > 0).any(), (q, np.flatnonzero(out & (over > 0))[:4])


@pytest.mark.parametrize("M", [8, 64])
def test_int8_and_bf16_routes_agree_on_unit_gaussian_rows(monkeypatch, M):
    """The certificate's own contract under a boosted bias: for M < 128 the
    int8 route returns the flat bf16 route's rows and scores."""
    g, X, Q, *_ = _gauss_tenant(128, True, 22)
    assert g.unit_rows()
    monkeypatch.setattr(TG, "KERNEL_MIN_WORK", 16)
    b = MemoryBoost(salience=0.5, frequency=0.3, recency=0.2, now=NOW)
    out = {}
    for route, min_rows in (("i8", 1024), ("bf16", 1 << 40)):
        with monkeypatch.context() as mp:
            mp.setattr(TG, "LOWP_MIN_ROWS", min_rows)
            calls = _spy(mp, g)
            out[route] = g.store_search(Q[:M], K, "l2", boost=b)
            assert _took(calls) == {route}
    assert torch.equal(out["i8"][1], out["bf16"][1]) and torch.equal(out["i8"][0], out["bf16"][0])


# ------------------------------------------------------------------ end to end
def test_boost_where_diversity_end_to_end(t64):
    """The MMR pool is the boosted, filtered search at ``fetch_k`` (the
    oracle's, bit for bit); the picks are MMR's over that pool -- held to the
    fp64 rule every query (tests/kernels/_mmr_ref.py rule 1), cosine relevance
    whatever the prior -- and the scores returned are the pool's boosted ones."""
    from lazzaro_amd.ops.mmr_ops import mmr_select
    from tests.kernels._mmr_ref import check_rule1
    g, X, meta, Q, kind = t64
    M, F = 32, 16
    kw = dict(where={"min_salience": 0.5}, boost=R.GRID_BOOST)
    ok = (kind == NODE) & (g.stored[:N].cpu().numpy() == 1) & (meta["sal"] >= 0.5)
    col = _column(g, meta, kind, "l2", where=ok)
    Qn = Q[:M].cpu().numpy()
    PS, PR = R.boosted_topk_ref(X, Qn, col, "l2", F)
    ps, pr = g.store_search(Q[:M], F, "l2", node_rows=True, **kw)
    assert np.array_equal(pr.cpu().numpy(), PR) and np.array_equal(ps.cpu().numpy().astype(np.float64), PS)
    pick, obj = mmr_select(g.emb32[:N], Q[:M], pr, K, 0.5)
    check_rule1(X, Qn, PR, K, 0.5, pick.cpu().numpy(), obj.cpu().numpy())
    s, r = g.store_search(Q[:M], K, "l2", diversity=0.5, fetch_k=F, **kw)
    assert torch.equal(r, torch.gather(pr, 1, pick.long())) and torch.equal(s, torch.gather(ps, 1, pick.long()))


def test_boost_expand_end_to_end(t64):
    from lazzaro_amd.ops.expand_ops import expand_tol
    from tests.kernels._expand_ref import exact_prefix, expand64
    g, X, meta, Q, kind = t64
    M = 16
    col = _column(g, meta, kind, "l2")
    _, seeds = R.boosted_topk_ref(X, Q[:M].cpu().numpy(), col, "l2", 16)
    plain = g.store_search(Q[:M], 16, "l2", node_rows=True)[1].cpu().numpy()
    assert not np.array_equal(np.sort(seeds, 1), np.sort(plain, 1))  # the prior changes the seeds
    s, r, via = g.store_search_expand(Q[:M], K, "l2", expand=1, boost=R.GRID_BOOST)
    s2, r2 = g.store_search(Q[:M], K, "l2", expand=1, boost=R.GRID_BOOST)
    assert torch.equal(r, r2) and torch.equal(s, s2)
    refs = expand64(X, Q[:M].cpu().numpy(), seeds, tuple(t.cpu().numpy() for t in g.csr()), g.e["w"].cpu().numpy(),
                    kind, g.sup[:N].cpu().numpy(), g.store_bias("l2").cpu().numpy(), 1)
    tol = expand_tol(64, 1)
    r, s = r.cpu().numpy(), s.cpu().numpy().astype(np.float64)
    for q, ref in enumerate(refs):
        want = ref.rows[ref.order[:K]]
        p = exact_prefix(ref, K, tol)
        assert np.array_equal(r[q, :p], want[:p]), (q, p)
        assert set(r[q].tolist()) <= set(ref.rows.tolist())
        sc = dict(zip(ref.rows.tolist(), ref.score.tolist()))
        assert max(abs(s[q, i] - sc[int(r[q, i])]) for i in range(K)) <= tol
