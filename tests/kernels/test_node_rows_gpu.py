"""``TenantGraph.store_search(..., node_rows=True)`` on an MI355X: every
return path of ``_store_search`` reachable at 4,096 rows itself returns the
rows that are not graph nodes as -1 -- inside the re-rank kernel where that
runs, once in torch where it does not -- with the scores untouched.

The tenant: 4,096 x 64 unit rows, the last 32 of them store-only (ghost) rows.
Each query is a copy of one of those, so a non-node row is certain to lead the
unmarked top-k (the tests assert it: they cannot pass vacuously)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from lazzaro_amd.engine import tenant_graph as TG  # noqa: E402
from lazzaro_amd.ops import tenant_ops  # noqa: E402

DEV = "cuda"
N, D, GHOSTS, M = 4096, 64, 32, 64
METRICS = ("l2", "ip", "cosine")


@pytest.fixture(scope="module")
def tenant():
    rng = np.random.default_rng(18)
    X = rng.standard_normal((N, D)).astype(np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    g = TG.TenantGraph(device=DEV, dim=D, capacity=N)
    m = N - GHOSTS
    g.add_nodes([f"m{i}" for i in range(m)], ["c"] * m, torch.from_numpy(X[:m]), shard=g.shard_id("w"), stored=True)
    g.add_nodes([f"g{i}" for i in range(GHOSTS)], ["ghost"] * GHOSTS, torch.from_numpy(X[m:]),
                shard=g.shard_id("w", live=False), stored=True, ghost=True)
    Q = torch.from_numpy(X[m + np.arange(M) % GHOSTS]).to(DEV)
    assert int((g.kind[:N] != TG.NODE).sum()) == GHOSTS and not g.wide_k
    return g, Q


@pytest.fixture()
def routes(tenant, monkeypatch):
    """The return paths taken, in order: "kernel" (store_rerank, which marks
    in its own launch) / "exact" (_exact_store)."""
    g, taken = tenant[0], []
    rerank, exact = tenant_ops.store_rerank, g._exact_store
    monkeypatch.setattr(tenant_ops, "store_rerank", lambda *a, **kw: taken.append("kernel") or rerank(*a, **kw))
    monkeypatch.setattr(g, "_exact_store", lambda *a, **kw: taken.append("exact") or exact(*a, **kw))
    return taken


def _check(g, Q, k, metric):
    s0, r0 = g.store_search(Q, k, metric, node_rows=False)
    s1, r1 = g.store_search(Q, k, metric, node_rows=True)
    assert (r0 >= 0).all()
    other = g.kind[r0].ne(TG.NODE)
    assert other[:, 0].all() and int(other.sum()) >= Q.shape[0]  # each query's own ghost row leads its top-k
    assert (r1.lt(0) | g.kind[r1.clamp_min(0)].eq(TG.NODE)).all()
    assert torch.equal(r1, torch.where(other, torch.full_like(r0, -1), r0))
    assert torch.equal(s1.view(torch.int32), s0.view(torch.int32))  # the scores are untouched, bit for bit


@pytest.mark.parametrize("metric", METRICS)
def test_flat_scan_and_rerank_kernel_mark_node_rows(tenant, routes, metric):
    g, Q = tenant
    assert Q.shape[0] * g.n == TG.KERNEL_MIN_WORK // 16  # exactly at the threshold of the bf16 scan
    _check(g, Q, 10, metric)
    assert routes == ["kernel", "kernel"]


@pytest.mark.parametrize("metric", METRICS)
def test_exact_store_below_the_work_threshold_marks_node_rows(tenant, routes, metric):
    g, Q = tenant
    _check(g, Q[:1], 10, metric)
    assert routes == ["exact", "exact"]


@pytest.mark.parametrize("metric", METRICS)
def test_exact_store_beyond_the_candidate_slots_marks_node_rows(tenant, routes, metric):
    g, Q = tenant
    assert 32 > TG.CAND_SLOTS
    _check(g, Q, 32, metric)
    assert routes == ["exact", "exact"]
