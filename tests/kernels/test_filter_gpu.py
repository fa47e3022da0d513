"""Filtered store search on the GPU (csrc/kernels/filter.hip):

1. the plan kernel against its torch formulation -- bias bit for bit, rows
   and count exactly;
2. the indexed scan against a float64 oracle;
3. ``TenantGraph.store_search(..., where=)`` end to end, forced onto each of
   its routes.

Oracle and excuses (parts 2 and 3). The oracle is a float64 scan of the
passing rows, sorted stably by (score descending, row ascending). A query is
excused only if the float64 gap between its k-th and (k+1)-th passing scores is
below 1e-5, and at most 1 % of a case's queries may be excused. The list
seeds of part 2 (``LIST_SEED``) and the data seed of part 3 were picked so
that the float64 oracle excuses NO query of any case; that was checked on the
CPU (``_scan_excused`` / ``_e2e_excused`` over every case return 0), so the
1 % allowance is never drawn on. Inside the top k two rows may trade places
only where their float64 scores are within 1e-5 of each other (fp32 against
float64 order of a near tie); exact ties must come back lower row first.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lazzaro_amd.core.filters import MemoryFilter
from lazzaro_amd.engine import tenant_graph as TG
from lazzaro_amd.engine.tenant_graph import GHOST, NODE, TenantGraph
from lazzaro_amd.ops import filter_ops as FO
from lazzaro_amd.ops.filter_ops import Predicate

pytestmark = pytest.mark.gpu

NEG_INF = float("-inf")
GAP = 1e-5


# ------------------------------------------------------------------ part 1: the plan kernel
PLAN_N = (1, 63, 64, 65, 1000, 4097)


def _cols(n, seed, dev):
    """Synthetic node columns: every predicate field has passing and failing
    rows, some rows are ghosts, some are not in the store, some are zero rows."""
    rng = np.random.default_rng(seed)
    c = {"sal": torch.from_numpy(rng.random(n).astype(np.float32)),
         "acc": torch.from_numpy(rng.integers(0, 10, n).astype(np.int32)),
         "last": torch.from_numpy(1000.0 + rng.integers(0, 100, n).astype(np.float64)),
         "ts": torch.from_numpy(2000.0 + rng.integers(0, 100, n).astype(np.float64)),
         "shard": torch.from_numpy(rng.integers(-1, 40, n).astype(np.int32)),
         "kind": torch.from_numpy(np.where(rng.random(n) < 0.1, GHOST, NODE).astype(np.uint8)),
         "sup": torch.from_numpy((rng.random(n) < 0.2).astype(np.uint8)),
         "stored": torch.from_numpy((rng.random(n) < 0.9).astype(np.uint8))}
    sqn = torch.from_numpy(np.where(rng.random(n) < 0.1, 0.0, 0.5 + rng.random(n)).astype(np.float32))
    tcode = torch.from_numpy(rng.integers(0, 7, n).astype(np.uint8))
    return {k: v.to(dev) for k, v in c.items()}, sqn.to(dev), tcode.to(dev)


def _check_plan(cols, pred, sqn, n, l2, tcode):
    bias, rows, count = FO.filter_plan(cols, pred, sqn, n, l2, tcode)
    rb, rr, rc = FO.filter_plan_ref(cols, pred, sqn, n, l2, tcode)
    c = int(count.cpu()[0])
    assert c == int(rc[0]) == rr.numel()
    assert bias.shape == rb.shape and torch.equal(bias.view(torch.int32), rb.view(torch.int32)), "bias bits differ"
    assert torch.equal(rows[:c], rr)
    return c


def _all_pass(cols, n):
    cols["kind"][:n] = NODE
    cols["stored"][:n] = 1


@pytest.mark.parametrize("n", PLAN_N)
def test_plan_masks(n):
    """Row masks across the wave (64) and block (256) boundaries, through the
    stored / kind columns, with the empty predicate (memories only)."""
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(n)
    masks = {"none": torch.zeros(n, dtype=torch.bool), "all": torch.ones(n, dtype=torch.bool),
             "row0": torch.arange(n) == 0, "last": torch.arange(n) == n - 1, "alternating": torch.arange(n) % 2 == 1,
             "third": torch.rand(n, generator=g) < 1 / 3,
             # a dead run longer than a block (256 rows), off the block grid
             "dead_run": ~((torch.arange(n) >= 100) & (torch.arange(n) < 700))}
    for name, m in masks.items():
        for l2 in (False, True):
            cols, sqn, tcode = _cols(n, 7, dev)
            _all_pass(cols, n)
            if name in ("third", "dead_run"):  # ghosts as well as rows that left the store
                cols["kind"][:n] = torch.where(m, NODE, GHOST).to(torch.uint8).to(dev)
            else:
                cols["stored"][:n] = m.to(torch.uint8).to(dev)
            c = _check_plan(cols, Predicate(), sqn, n, l2, tcode)
            assert c == int(m.sum()), name


FIELDS = {
    "types": dict(type_codes=[1, 4]),
    "types_none_known": dict(type_codes=[]),
    "shards": dict(shard_codes=[0, 3, 31, 32, 39]),
    "shards_default": dict(shard_codes=[5], neg_shard_pass=True),
    "shard_never_seen": dict(shard_codes=[]),  # a name the tenant never saw resolves to no code
    "min_sal": dict(min_sal=0.6),
    "max_sal": dict(max_sal=0.3),
    "since": dict(since=2050.0),
    "until": dict(until=2050.0),
    "since_eq_until": dict(since=2050.0, until=2050.0),
    "accessed": dict(accessed_since=1070.0),
    "min_acc": dict(min_acc=7),
    "sup_only": dict(sup_mode=1),
    "sup_none": dict(sup_mode=0),
    "exclude": dict(exclude_rows=[0, 1, 63, 64, 999, 4096]),
    "exclude_absent": dict(exclude_rows=[]),  # an unknown id resolves to no row
    "everything": dict(type_codes=[0, 1, 2, 3, 4], shard_codes=list(range(0, 40, 2)), neg_shard_pass=True,
                       min_sal=0.1, max_sal=0.9, since=2005.0, until=2095.0, accessed_since=1005.0, min_acc=1,
                       sup_mode=0, exclude_rows=[2, 65, 1001]),
}


@pytest.mark.parametrize("n", PLAN_N)
def test_plan_fields(n):
    """Every field alone and all together, over rows that also hold ghosts,
    rows with stored == 0 and zero vectors (bias +0, not -0)."""
    dev = torch.device("cuda")
    cols, sqn, tcode = _cols(n, 11 + n, dev)
    for name, kw in FIELDS.items():
        kw = dict(kw)
        if "exclude_rows" in kw:
            kw["exclude_rows"] = [r for r in kw["exclude_rows"] if r < n]
        for l2 in (False, True):
            c = _check_plan(cols, Predicate(**kw), sqn, n, l2, tcode)
            if name in ("types_none_known", "shard_never_seen", "since_eq_until"):
                assert c == 0, name
    full = _check_plan(cols, Predicate(), sqn, n, True, tcode)
    assert _check_plan(cols, Predicate(exclude_rows=[]), sqn, n, True, tcode) == full


def test_plan_names_resolved_by_the_graph():
    """A shard name the tenant never saw matches nothing; an excluded id
    that is absent excludes nothing; ghosts and unstored rows never pass."""
    g, _ = _graph(64, n=1000)
    torch.cuda.synchronize()  # (_filter_plan is called outside store_search's stream scope here)
    ok = ((g.kind[: g.n] == NODE) & (g.stored[: g.n] == 1)).sum().item()
    assert g._filter_plan(MemoryFilter(), True).count == ok < g.n
    assert g._filter_plan(MemoryFilter(shard_keys=["never-seen"]), True).count == 0
    assert g._filter_plan(MemoryFilter(exclude_ids=["absent-id"]), True).count == ok
    assert g._filter_plan(MemoryFilter(exclude_ids=["absent-id", g.ids[0]]), True).count == ok - 1
    p = g._filter_plan(MemoryFilter(types=["a", "never-seen"]), False)
    want = torch.nonzero((g.kind[: g.n] == NODE) & (g.stored[: g.n] == 1)
                         & torch.tensor([t == "a" for t in g.types], device=g.device)).flatten()
    assert torch.equal(p.rows.long(), want)
    assert torch.equal(p.bias == 0, torch.zeros(g.n, dtype=torch.bool, device=g.device).index_fill_(0, want, True))


# ------------------------------------------------------------------ part 2: the indexed scan
SCAN_ROWS = 8192
SCAN_D = (64, 200, 768, 67)  # 67: no 16-byte rows, the scalar tail path
SCAN_L = (1, 15, 16, 17, 255, 257, 5000)
SCAN_M = (1, 3, 64, 130)
SCAN_K = (1, 10, 16)
# seed of the row list of case (D, L): the first for which the float64 oracle
# excuses no query at any (M, k) (0 where not listed)
LIST_SEED = {(64, 257): 1, (64, 5000): 1, (200, 257): 1, (768, 16): 1, (768, 255): 2, (768, 257): 1}

_scan_cache = {}


def _scan_data(D):
    """Unit rows and queries of one width, and their float64 scores (built
    once on the CPU generator, shared by every case of that width)."""
    if D not in _scan_cache:
        g = torch.Generator().manual_seed(1000 + D)
        X = F.normalize(torch.randn(SCAN_ROWS, D, generator=g), dim=1)
        Q = F.normalize(torch.randn(max(SCAN_M), D, generator=g), dim=1)
        _scan_cache[D] = (X, Q)
    return _scan_cache[D]


def _scan_list(D, L):
    g = torch.Generator().manual_seed(77 * D + L + 100003 * LIST_SEED.get((D, L), 0))
    return torch.sort(torch.randperm(SCAN_ROWS, generator=g)[:L]).values.to(torch.int32)


def _scan_form(L):
    """(alpha, l2): odd list lengths score like L2 (2<q,x> - |x|^2), even ones like IP."""
    return (2.0, True) if L % 2 else (1.0, False)


def _oracle(S64, rows, k):
    """float64 scores [M, n] restricted to ``rows`` (ascending): top-k rows by
    (score desc, row asc), their scores, and the k / k+1 gap per query (inf
    when fewer than k + 1 rows pass)."""
    s = S64[:, rows.long()]
    o = torch.sort(s, dim=1, descending=True, stable=True)
    top = rows.long()[o.indices[:, :k]]
    gap = (o.values[:, k - 1] - o.values[:, k]) if s.shape[1] > k else torch.full((s.shape[0],), float("inf"),
                                                                                 dtype=torch.float64, device=s.device)
    return top, o.values[:, :k], gap


def _scan_scores64(X, Q, alpha, l2):
    S = alpha * (Q.double() @ X.double().T)
    return S - (X.double() ** 2).sum(1)[None, :] if l2 else S


def _scan_excused(D, L, dev="cpu"):
    """Queries the float64 oracle excuses over every (M, k) of case (D, L)."""
    X, Q = _scan_data(D)
    alpha, l2 = _scan_form(L)
    S = _scan_scores64(X.to(dev), Q.to(dev), alpha, l2)
    rows = _scan_list(D, L).to(dev)
    return sum(int((_oracle(S[:M], rows, k)[2] < GAP).sum()) for M in SCAN_M for k in SCAN_K)


def _compare(got_s, got_r, S64, rows, k, tol):
    """Result rows / scores of one case against the oracle (see the module
    docstring). Returns the number of excused queries."""
    top, tops, gap = _oracle(S64, rows, k)
    M, have = top.shape
    excused = gap < GAP
    assert int(excused.sum()) <= M // 100, f"{int(excused.sum())} of {M} queries excused"
    got_r, got_s = got_r.cpu(), got_s.cpu()
    top, tops, S = top.cpu(), tops.cpu(), S64.cpu()
    assert got_r.shape == (M, k)
    assert (got_r[:, have:] == -1).all() and (got_s[:, have:] == NEG_INF).all(), "a short list pads with -1"
    for q in torch.nonzero(~excused.cpu()).flatten().tolist():
        r = got_r[q, :have]
        assert sorted(r.tolist()) == sorted(top[q].tolist()), f"query {q}: rows {r.tolist()} != {top[q].tolist()}"
        s64 = S[q, r]
        assert ((s64 - tops[q]).abs() < GAP).all(), f"query {q}: order differs beyond a near tie"
        assert ((got_s[q, :have].double() - s64).abs() <= tol).all(), f"query {q}: score error above {tol}"
    return int(excused.sum())


def _fp32_tol(D, alpha):
    # fp32 dot of unit vectors in any summation order: (D + 2) roundings of relative 2^-24 on partial
    # sums bounded by |q||x| = 1 (Cauchy-Schwarz on the absolute products), times alpha, plus the bias add
    return (D + 4) * 2.0 ** -24 * alpha + 2.0 ** -22


@pytest.mark.parametrize("D", SCAN_D)
@pytest.mark.parametrize("L", SCAN_L)
def test_gather_topk(D, L):
    dev = torch.device("cuda")
    X, Q = _scan_data(D)
    Xd, Qd = X.to(dev), Q.to(dev)
    alpha, l2 = _scan_form(L)
    sqn = (Xd * Xd).sum(1)
    bias = (-sqn if l2 else torch.zeros_like(sqn)).contiguous()
    S64 = _scan_scores64(Xd, Qd, alpha, l2)
    rows = _scan_list(D, L).to(dev)
    for M in SCAN_M:
        for k in SCAN_K:
            s, r = FO.gather_topk(Xd, rows, L, Qd[:M].contiguous(), k, bias, alpha)
            _compare(s, r, S64[:M], rows, k, _fp32_tol(D, alpha))
            rs, rr = FO.gather_topk_ref(Xd, rows, L, Qd[:M], k, bias, alpha)
            _compare(rs, rr, S64[:M], rows, k, _fp32_tol(D, alpha))


def test_gather_topk_rows_beyond_count_are_not_read():
    """``count`` bounds the list: entries past it (here out of range) are ignored."""
    dev = torch.device("cuda")
    X, Q = _scan_data(64)
    Xd, Qd = X.to(dev), Q[:3].to(dev).contiguous()
    rows = torch.tensor([5, 9, 300, 1 << 30, -7], dtype=torch.int32, device=dev)
    bias = torch.zeros(SCAN_ROWS, device=dev)
    s, r = FO.gather_topk(Xd, rows, 3, Qd, 10, bias, 1.0)
    assert sorted(r[0, :3].tolist()) == [5, 9, 300] and (r[:, 3:] == -1).all()


@pytest.mark.parametrize("D", (64, 67))
def test_gather_topk_duplicates_lower_row_first(D):
    """Identical vectors at different rows tie exactly: the lower row comes
    first; when the list leaves the lower one out the higher takes its place."""
    dev = torch.device("cuda")
    X, Q = _scan_data(D)
    Xd, Qd = X.to(dev).clone(), Q[:5].to(dev).contiguous()
    twins = [(10, 4000), (300, 301), (7000, 20)]
    for a, b in twins:
        Xd[b] = Xd[a]
    Qd[0], Qd[1], Qd[2] = Xd[10], Xd[300], Xd[20]  # each query's best hit is a twin pair
    bias = torch.zeros(SCAN_ROWS, device=dev)
    everything = torch.arange(SCAN_ROWS, dtype=torch.int32, device=dev)
    for k in SCAN_K:
        s, r = FO.gather_topk(Xd, everything, SCAN_ROWS, Qd, k, bias, 1.0)
        assert r[:3, 0].tolist() == [10, 300, 20]
        if k > 1:
            assert r[:3, 1].tolist() == [4000, 301, 7000] and torch.equal(s[:3, 0], s[:3, 1])
        keep = torch.ones(SCAN_ROWS, dtype=torch.bool, device=dev)
        keep[[10, 300, 20]] = False
        lst = everything[keep].contiguous()
        s2, r2 = FO.gather_topk(Xd, lst, lst.numel(), Qd, k, bias, 1.0)
        assert r2[:3, 0].tolist() == [4000, 301, 7000] and torch.equal(s2[:3, 0], s[:3, 0])


# ------------------------------------------------------------------ part 3: end to end
E2E_N, E2E_M, E2E_K = 4096, 64, 10
E2E_SEED = 0
METRICS = ("l2", "ip", "cosine")
# ~1 % (40 of the 4,000 memories), ~50 %, 100 %
E2E_FILTERS = {"1pct": MemoryFilter(min_access_count=99), "50pct": MemoryFilter(types=["a"]), "100pct": MemoryFilter()}


def _graph(D, n=E2E_N, seed=E2E_SEED):
    """A GPU tenant of n unit rows: nodes with acc = row % 100 and types a / b
    alternating, 2 % ghosts and ~1 % nodes that are not in the store."""
    gen = torch.Generator().manual_seed(seed + D)
    X = F.normalize(torch.randn(n, D, generator=gen), dim=1)
    Q = F.normalize(torch.randn(E2E_M, D, generator=gen), dim=1)
    g = TenantGraph(device="cuda", dim=D, capacity=n)
    m = n - n // 50 - n // 100
    n_gh = n // 50
    g.add_nodes([f"m{i}" for i in range(m)], ["c"] * m, X[:m], shard=[g.shard_id(f"s{i % 5}") for i in range(m)],
                types=["a" if i % 2 == 0 else "b" for i in range(m)],
                sal=[0.1 + 0.8 * ((i * 37) % 101) / 101 for i in range(m)], acc=[i % 100 for i in range(m)],
                last=[float(i) for i in range(m)], ts=[float(i % 977) for i in range(m)], stored=True)
    g.add_nodes([f"g{i}" for i in range(n_gh)], ["ghost"] * n_gh, X[m:m + n_gh], shard=g.shard_id("s0", live=False),
                stored=True, ghost=True)
    rest = n - m - n_gh
    g.add_nodes([f"u{i}" for i in range(rest)], ["unstored"] * rest, X[m + n_gh:], shard=g.shard_id("s1"),
                acc=99, types="a", stored=False)
    assert g.n == n and g.unit_rows()
    return g, Q.cuda()


def _mask(g, name):
    """The passing rows of E2E_FILTERS[name], from the graph's columns (independent of filter_ops)."""
    n = g.n
    ok = (g.kind[:n] == NODE) & (g.stored[:n] == 1)
    if name == "1pct":
        ok &= g.acc[:n] >= 99
    elif name == "50pct":
        ok &= torch.tensor([t == "a" for t in g.types], device=g.device)
    return torch.nonzero(ok).flatten()


def _scores64(g, Q, metric):
    X, q = g.emb32[: g.n].double(), Q.double()
    if metric == "cosine":
        return (q / q.norm(dim=1, keepdim=True)) @ (X / X.norm(dim=1, keepdim=True)).T
    S = q @ X.T
    return 2.0 * S - (X * X).sum(1)[None, :] - (q * q).sum(1, keepdim=True) if metric == "l2" else S


def _e2e_check(g, Q, metric, name, k=E2E_K):
    s, r = g.store_search(Q, k, metric, where=E2E_FILTERS[name])
    D = g.dim
    # the re-rank kernel's fp32 score: the dot's roundings (alpha = 2 for L2) plus the bias and |q|^2 adds
    tol = (D + 4) * 2.0 ** -24 * 2.0 + 2.0 ** -21
    return _compare(s, r, _scores64(g, Q, metric), _mask(g, name).to(torch.int32), k, tol)


EVICTED = tuple(range(99, 800, 100))  # test_plan_invalidated_...: the first eight rows the 1 % filter passes


def _appended():
    return F.normalize(torch.randn(300, 64, generator=torch.Generator().manual_seed(3)), dim=1)


def _e2e_excused(D, seed=E2E_SEED, gone=(), appended=False):
    """(CPU check of the seed) queries the float64 oracle excuses over every
    end-to-end case of width D -- with ``gone`` evicted and 300 passing rows
    appended, the states test_plan_invalidated_by_eviction_and_compaction
    searches (a compaction renumbers rows and keeps their order: same gaps)."""
    gen = torch.Generator().manual_seed(seed + D)
    X = F.normalize(torch.randn(E2E_N, D, generator=gen), dim=1).double()
    Q = F.normalize(torch.randn(E2E_M, D, generator=gen), dim=1).double()
    m = E2E_N - E2E_N // 50 - E2E_N // 100
    i = torch.arange(E2E_N)
    live = i < m
    live[list(gone)] = False
    masks = {"1pct": live & (i % 100 == 99), "50pct": live & (i % 2 == 0), "100pct": live}
    if appended:
        X = torch.cat([X, _appended().double()])
        masks = {k: torch.cat([v, torch.ones(300, dtype=torch.bool)]) for k, v in masks.items()}
    bad = 0
    for metric in METRICS:
        S = Q @ X.T
        S = 2.0 * S - (X * X).sum(1)[None, :] - (Q * Q).sum(1, keepdim=True) if metric == "l2" else S
        for mk in masks.values():
            bad += int((_oracle(S, torch.nonzero(mk).flatten(), E2E_K)[2] < GAP).sum())
    return bad


@pytest.fixture(scope="module")
def tenants():
    return {D: _graph(D) for D in (64, 128)}


def _force(monkeypatch, route):
    """Module constants that pin the route of a filtered search."""
    monkeypatch.setattr(TG, "FILTER_SPARSE_MAX_ROWS", 1 << 40 if route == "sparse" else -1)
    if route == "sparse":
        return
    if route == "i8":
        monkeypatch.setattr(TG, "LOWP_MIN_ROWS", 1024)
    elif route == "exact":
        monkeypatch.setattr(TG, "KERNEL_MIN_WORK", 1 << 40)


# the int8 candidate scan exists for padded widths that are multiples of 128
# only (TenantGraph._lowp_mode), so that route is forced at D = 128; every
# other route runs at D = 64 as well
ROUTES = [(64, "sparse"), (64, "bf16"), (64, "exact"), (128, "sparse"), (128, "bf16"), (128, "i8"), (128, "exact")]


@pytest.mark.parametrize("D,route", ROUTES)
def test_store_search_where_routes(tenants, monkeypatch, D, route):
    g, Q = tenants[D]
    _force(monkeypatch, route)
    calls = {"i8": 0, "bf16": 0, "exact": 0, "sparse": 0}

    def count(obj, attr, key):
        fn = getattr(obj, attr)

        def wrapped(*a, **kw):
            calls[key] += 1
            return fn(*a, **kw)
        monkeypatch.setattr(obj, attr, wrapped)

    import lazzaro_amd.ops.search as S
    count(g, "_i8_candidates", "i8")
    count(g, "_exact_store", "exact")
    count(S, "flat_topk", "bf16")
    count(FO, "gather_topk", "sparse")
    n_cases = 0
    for metric in METRICS:
        for name in E2E_FILTERS:
            before = dict(calls)
            assert _e2e_check(g, Q, metric, name) == 0  # (the seed excuses nothing: see the module docstring)
            n_cases += 1
            took = {key for key in calls if calls[key] > before[key]}
            assert took == {route}, f"{metric} {name}: took {took}, not {route}"
    passing = _mask(g, "1pct").numel()
    assert 38 <= passing <= 42 and n_cases == 9


def test_one_percent_k10_is_not_a_post_filter(tenants):
    """The ten best of ~40 passing rows: the unfiltered search's 16 candidates hold almost none of them."""
    g, Q = tenants[64]
    _, r = g.store_search(Q, E2E_K, "l2", where=E2E_FILTERS["1pct"])
    assert (r >= 0).all()
    _, r16 = g.store_search(Q, 16, "l2")
    ok = set(_mask(g, "1pct").tolist())
    post = [len([x for x in row if x in ok]) for row in r16.tolist()]
    assert max(post) < E2E_K  # over-fetch + post-filter cannot fill ten slots


def test_where_none_calls_no_new_op(tenants, monkeypatch):
    g, Q = tenants[64]
    want = [g.store_search(Q, E2E_K, m, node_rows=nr) for m in METRICS for nr in (False, True)]

    def boom(*a, **kw):
        raise AssertionError("where=None reached a filter op")
    for name in ("filter_plan", "filter_plan_ref", "gather_topk", "gather_topk_ref"):
        monkeypatch.setattr(FO, name, boom)
    monkeypatch.setattr(g, "_filter_plan", boom)
    monkeypatch.setattr(g, "_store_search_where", boom)
    built = g.filter_plans_built
    got = [g.store_search(Q, E2E_K, m, node_rows=nr, where=None) for m in METRICS for nr in (False, True)]
    for (s0, r0), (s1, r1) in zip(want, got):
        assert torch.equal(s0, s1) and torch.equal(r0, r1)
    assert g.filter_plans_built == built


@pytest.mark.parametrize("route", ("sparse", "bf16"))
def test_plan_invalidated_by_eviction_and_compaction(monkeypatch, route):
    # its own tenant (the test mutates it); seed 2: _e2e_excused(64, 2), (64, 2, EVICTED) and
    # (64, 2, EVICTED, True) are all 0 on the CPU
    g, Q = _graph(64, seed=2)
    _force(monkeypatch, route)
    for name in E2E_FILTERS:
        _e2e_check(g, Q, "l2", name)
    built = g.filter_plans_built
    _e2e_check(g, Q, "l2", "1pct")
    assert g.filter_plans_built == built  # cached
    # evict eight of the ~40 rows the 1 % filter passes: a stale plan would still return them
    gone = list(EVICTED)
    _, r = g.store_search(Q, E2E_K, "l2", where=E2E_FILTERS["1pct"])
    assert set(r.flatten().tolist()) & set(gone)
    g.remove_nodes(gone, unstore=True)
    for name in E2E_FILTERS:
        _e2e_check(g, Q, "l2", name)
    _, r = g.store_search(Q, E2E_K, "l2", where=E2E_FILTERS["1pct"])
    assert not set(r.flatten().tolist()) & set(gone)
    g.take_dirty_rows()
    out = g.compact()
    assert out["reclaimed"] >= len(gone)
    for metric in METRICS:
        for name in E2E_FILTERS:
            _e2e_check(g, Q, metric, name)
    # rows appended after the type-code column was built
    g.add_nodes([f"new{i}" for i in range(300)], ["c"] * 300, _appended(), shard=g.shard_id("s0"), types="a", acc=99,
                stored=True)
    for name in E2E_FILTERS:
        _e2e_check(g, Q, "ip", name)
