"""Multi-query search (``fuse=``) on the CPU tier, through MemorySystem with
the hashing embedder: every public surface, the batch against the per-group
call, a singleton group against ``search_memories``, inner ``where=`` /
``boost=``, validation before the embedding call, the counters and the
dashboard parameters."""
import numpy as np
import pytest
import torch

from lazzaro_amd.core.fuse import QueryFusion
from lazzaro_amd.core.memory_system import MemorySystem
from lazzaro_amd.core.providers import HashEmbedder, LocalLLM
from tests.kernels import _fuse_ref as R

D = 32
N = 90
WORDS = ["alpha", "beta", "gamma", "router", "kernel", "memory", "garden", "violin", "harbor", "lantern", "orchid",
         "quartz", "ticket", "billing", "invoice", "sunrise"]
GROUPS = [["violin orchid garden", "orchid violin", "a garden of orchids"],
          ["router kernel memory"],
          ["harbor lantern", "quartz lantern harbor", "billing ticket", "ticket invoice billing"]]


def _system(tmp_path, name="db", **kw):
    return MemorySystem(llm_provider=LocalLLM(), embedding_provider=HashEmbedder(dim=D), enable_async=False,
                        load_from_disk=False, db_dir=str(tmp_path / name), **kw)


def _fill(ms):
    """90 memories of four common words each, embedded by the system's own
    embedder (so a query of the same words lies near them); every third is a
    preference, salience rises with the row."""
    g = ms.graph
    rng = np.random.default_rng(11)
    texts = [" ".join(rng.choice(WORDS, size=4)) for _ in range(N)]
    emb = np.asarray([ms._get_embedding(t) for t in texts], dtype=np.float32)
    types = ["preference" if i % 3 == 0 else "semantic" for i in range(N)]
    g.add_nodes([f"m{i}" for i in range(N)], texts, torch.from_numpy(emb), shard=g.shard_id("w"), types=types,
                sal=torch.linspace(0.05, 0.95, N), stored=True)


@pytest.fixture()
def ms(tmp_path):
    m = _system(tmp_path)
    _fill(m)
    yield m
    m.close()


def _ids(hits):
    return [n.id for n in hits]


def _embs(ms, qs):
    return torch.as_tensor(np.asarray([ms._get_embedding(q) for q in qs], dtype=np.float32))


def _offsets(groups):
    return np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int64)


@pytest.mark.parametrize("fuse", ["rrf", "mean", {"mode": "rrf", "pool": 24, "rrf_k": 10.5}])
def test_surfaces_agree_and_match_the_oracle(ms, fuse):
    g = ms.graph
    fu = QueryFusion.coerce(fuse)
    flat = [q for grp in GROUPS for q in grp]
    Q, off = _embs(ms, flat), _offsets(GROUPS)
    # the engine: the oracle applied to the pools the engine's own search returns
    _, pools = g.store_search(Q, fu.pool, ms.store.metric, node_rows=True)
    s, r, sup = g.store_search_fused(Q, off, 6, ms.store.metric, fuse)
    assert s.shape == r.shape == sup.shape == (3, 6) and sup.dtype == torch.int32
    X = g.emb32[: g.n].numpy()
    refs = R.fuse64(off, pools.numpy(), g.n, fu.mode, fu.rrf_k, X=X, Q=Q.numpy())
    nc = np.asarray([ref.rows.size for ref in refs])
    if fu.mode == "rrf":
        R.check_rrf(refs, 6, r.numpy(), s.numpy(), sup.numpy(), nc)
    else:
        R.check_mean(refs, 6, r.numpy(), s.numpy(), sup.numpy(), nc, D)
    assert (r >= 0).all() and int(sup.max()) > 1 and (sup[1] == 1).all()
    want = [[g.ids[x] for x in row] for row in r.tolist()]
    # every surface above it
    assert g.search_ids_fused(Q, off, 6, ms.store.metric, fuse) == want
    assert ms.vector_store.search_nodes_fused(Q, off, user_id=ms.user_id, limit=6, fuse=fuse) == want
    assert ms.vector_store.search_nodes_fused(Q.tolist(), off.tolist(), user_id=ms.user_id, limit=6, fuse=fuse) == want
    batch = ms.search_memories_fused_batch(GROUPS, limit=6, fuse=fuse)
    assert [_ids(b) for b in batch] == want
    assert [_ids(ms.search_memories_fused(grp, limit=6, fuse=fuse)) for grp in GROUPS] == want
    assert all(n.content for b in batch for n in b)


def test_a_singleton_rrf_group_is_the_plain_search(ms):
    for q in ("violin orchid garden", "router kernel"):
        plain = _ids(ms.search_memories(q, limit=7))
        assert len(plain) == 7
        assert _ids(ms.search_memories_fused([q], limit=7)) == plain
        assert _ids(ms.search_memories_fused([q], limit=7, where={"types": ["preference"]})) == \
            _ids(ms.search_memories(q, limit=7, where={"types": ["preference"]}))
    got = ms.search_memories_fused_batch([["violin orchid garden"], ["router kernel"]], limit=7)
    assert [_ids(b) for b in got] == [_ids(ms.search_memories(q, limit=7)) for q in ("violin orchid garden",
                                                                                     "router kernel")]


def test_inner_where_and_boost_reach_the_pools(ms):
    g = ms.graph
    grp = GROUPS[0]
    flt = {"types": ["preference"]}
    for fuse in ("rrf", "mean"):
        got = ms.search_memories_fused(grp, limit=10, fuse=fuse, where=flt)
        assert len(got) == 10 and all(n.type == "preference" for n in got)
    # boost: the pools are the boosted searches' rows
    Q, off = _embs(ms, grp), [0, len(grp)]
    from lazzaro_amd.core.boost import MemoryBoost
    b = MemoryBoost.coerce(2.0).at(1000.0)
    _, pools = g.store_search(Q, 16, ms.store.metric, node_rows=True, boost=b)
    _, plain_pools = g.store_search(Q, 16, ms.store.metric, node_rows=True)
    assert not torch.equal(pools, plain_pools)
    s, r, sup = g.store_search_fused(Q, off, 8, ms.store.metric, "rrf", boost=b)
    refs = R.fuse64(off, pools.numpy(), g.n, "rrf", 60.0)
    R.check_rrf(refs, 8, r.numpy(), s.numpy(), sup.numpy(), np.asarray([refs[0].rows.size]))
    # ... with where= as well; mean scores by cosine whatever the boost
    s, r, sup = g.store_search_fused(Q, off, 8, ms.store.metric, "mean", where=flt, boost=b)
    _, pools = g.store_search(Q, 16, ms.store.metric, node_rows=True, where=flt, boost=b)
    refs = R.fuse64(off, pools.numpy(), g.n, "mean", X=g.emb32[: g.n].numpy(), Q=Q.numpy())
    R.check_mean(refs, 8, r.numpy(), s.numpy(), sup.numpy(), np.asarray([refs[0].rows.size]), D)
    assert all(g.ids[x] in {f"m{i}" for i in range(0, N, 3)} for x in r[0].tolist())
    # expand= and lexical= as inner options run
    assert len(ms.search_memories_fused(grp, limit=5, expand=1)) == 5
    assert len(ms.search_memories_fused(grp, limit=5, lexical=0.5)) == 5
    assert ms.vector_store.search_nodes_fused(Q, off, user_id=ms.user_id, limit=5, lexical=0.5, query_texts=grp) == \
        [_ids(ms.search_memories_fused(grp, limit=5, lexical=0.5))]


def test_weights(ms):
    grp = GROUPS[2]
    only_last = _ids(ms.search_memories_fused(grp, limit=5, weights=[0, 0, 0, 1]))
    assert only_last == _ids(ms.search_memories(grp[3], limit=5))
    by_position = ms.search_memories_fused_batch([grp, grp[::-1]], limit=5, fuse={"weights": [0, 0, 0, 1]})
    assert _ids(by_position[0]) == only_last and _ids(by_position[1]) == _ids(ms.search_memories(grp[0], limit=5))
    per_group = ms.search_memories_fused_batch([grp, grp[:2]], limit=5, weights=[[0, 0, 0, 1], [1, 0]])
    assert _ids(per_group[0]) == only_last and _ids(per_group[1]) == _ids(ms.search_memories(grp[0], limit=5))
    mean_one = _ids(ms.search_memories_fused(grp, limit=3, fuse="mean", weights=[0, 0, 0, 1]))
    assert mean_one[0] == only_last[0]  # the nearest of the one sub-query that counts


def test_validation_comes_before_the_embedding(ms, monkeypatch):
    emb = _embs(ms, GROUPS[0])
    before = dict(ms.get_stats()["engine"])

    def boom(*a, **k):
        raise AssertionError("the embedder was called before the options were checked")
    monkeypatch.setattr(ms, "_batch_embed_any", boom)
    monkeypatch.setattr(ms, "_get_embedding", boom)
    bad = [dict(fuse="max"), dict(fuse={"pool": 65}), dict(fuse={"pool": 0}), dict(fuse={"rrf_k": 0.0}),
           dict(fuse={"mode": "rrf", "depth": 2}), dict(fuse=None), dict(limit=0), dict(limit=65),
           dict(fuse={"weights": [1.0, 2.0]}), dict(weights=[[1.0, 2.0]]), dict(weights=[[1, 1, -1]]),
           dict(fuse="mean", weights=[[0, 0, 0]]), dict(fuse={"weights": [1, float("inf"), 1]}),
           dict(expand={"hops": 9}), dict(lexical=1.5), dict(boost={"salience": -1.0})]
    for kw in bad:
        with pytest.raises(ValueError):
            ms.search_memories_fused_batch([GROUPS[0]], **kw)
        kw1 = dict(kw)
        if "weights" in kw1:
            kw1["weights"] = kw1["weights"][0]
        with pytest.raises(ValueError):
            ms.search_memories_fused(GROUPS[0], **kw1)
        kw2 = dict(kw)
        with pytest.raises(ValueError):
            ms.vector_store.search_nodes_fused(emb, [0, 3], user_id=ms.user_id, query_texts=GROUPS[0], **kw2)
        with pytest.raises(ValueError):
            ms.graph.store_search_fused(emb, [0, 3], kw2.pop("limit", 5), "l2", kw2.pop("fuse", "rrf"),
                                        query_terms=GROUPS[0], **kw2)
    for groups in ([[]], [GROUPS[0], []], [["q"] * 17]):
        with pytest.raises(ValueError):
            ms.search_memories_fused_batch(groups)
    with pytest.raises(ValueError):
        ms.search_memories_fused([])
    with pytest.raises(ValueError):
        ms.search_memories_fused("one string")
    with pytest.raises(ValueError):
        ms.graph.store_search_fused(emb, [0, 2], 5)  # offsets that do not cover the queries
    with pytest.raises(ValueError):
        ms.vector_store.search_nodes_fused(emb, [0, 3], user_id=ms.user_id, lexical=0.5)  # no texts
    with pytest.raises(NotImplementedError):
        ms.search_memories_fused(GROUPS[0], lexical=0.5, boost=1.0)
    with pytest.raises(TypeError):
        ms.search_memories_fused(GROUPS[0], diversity=0.5)  # not taken at all
    assert ms.get_stats()["engine"] == before
    assert ms.search_memories_fused_batch([]) == []


def test_surfaces_without_a_graph_raise(ms, tmp_path):
    from lazzaro_amd.core.vector_store import HBMStore
    from lazzaro_amd.parallel.service import DistributedMemoryService
    from lazzaro_amd.parallel.sharded_memory import ShardedMemorySystem
    st = HBMStore(db_dir=str(tmp_path / "plain"), device="cpu")
    st.add_nodes([{"id": "a", "content": "c", "vector": [1.0] + [0.0] * (D - 1)}], user_id="u")
    q = [[1.0] + [0.0] * (D - 1)] * 2
    with pytest.raises(NotImplementedError, match="needs the tenant's graph"):
        st.search_nodes_fused(q, [0, 2], user_id="u")
    with pytest.raises(NotImplementedError, match="where= needs the tenant's graph"):
        st.search_nodes_fused(q, [0, 2], user_id="u", where={"types": ["semantic"]})
    st.close()
    assert not hasattr(ShardedMemorySystem, "search_memories_fused")
    assert not hasattr(DistributedMemoryService, "search_memories_fused")


def test_the_counters_count(ms):
    e = ms.get_stats()["engine"]
    assert e["fused_searches"] == 0 and e["fused_groups"] == 0
    ms.search_memories("violin", limit=3)
    ms.search_memories_batch(["violin", "orchid"], limit=3)
    e = ms.get_stats()["engine"]
    assert e["fused_searches"] == 0 and e["fused_groups"] == 0
    ms.search_memories_fused(GROUPS[0])
    ms.search_memories_fused_batch(GROUPS, fuse="mean", where={"min_salience": 0.2})
    e = ms.get_stats()["engine"]
    assert e["fused_searches"] == 2 and e["fused_groups"] == 4 and e["filtered_searches"] == 1


def test_dashboard_search_parameters(ms):
    from fastapi.testclient import TestClient

    from lazzaro_amd.dashboard import api
    api.set_memory_system(ms)
    try:
        c = TestClient(api.app)
        grp = GROUPS[0]
        plain = [h["id"] for h in c.get("/api/search", params={"q": grp[0], "limit": 5}).json()]
        assert plain == _ids(ms.search_memories(grp[0], limit=5))
        assert [h["id"] for h in c.get("/api/search", params={"q": grp[0], "limit": 5, "fuse": "mean"}).json()] == plain
        for fuse in ("rrf", "mean"):
            got = c.get("/api/search", params={"q": grp[0], "also": grp[1:], "limit": 5, "fuse": fuse}).json()
            assert [h["id"] for h in got] == _ids(ms.search_memories_fused(grp, limit=5, fuse=fuse))
        got = c.get("/api/search", params={"q": grp[0], "also": grp[1:], "limit": 5, "types": "preference"}).json()
        assert [h["id"] for h in got] == _ids(ms.search_memories_fused(grp, limit=5, where={"types": ["preference"]}))
        assert ms.get_stats()["engine"]["fused_searches"] == 6
    finally:
        api.set_memory_system(None)
