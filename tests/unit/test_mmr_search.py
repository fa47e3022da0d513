"""Diversity-aware memory search (``diversity=``, ``fetch_k=``) on the CPU
tier, through MemorySystem with the hashing embedder: a tenant of
near-duplicate memories, the public surfaces, composition with ``where=`` and
with ghost rows, validation, the unsupported surfaces and the counter."""
import numpy as np
import pytest
import torch

from lazzaro_amd.core.memory_system import MemorySystem
from lazzaro_amd.core.providers import HashEmbedder, LocalLLM
from lazzaro_amd.ops.mmr_ops import MAX_FETCH_K
from tests.kernels._mmr_ref import mmr_greedy64

D = 32
TOPICS, DUPS = 6, 8
QUERY = "which async runtime does the user prefer for rust"
GAP = 2e-4  # the smallest fp64 margin a pick of the constructed tenant may have (see _fill)
QUERIES = [QUERY, "favourite food", "trip to the mountains last week"]
TYPES = ("semantic", "preference")


def _system(tmp_path, name="db", **kw):
    return MemorySystem(llm_provider=LocalLLM(), embedding_provider=HashEmbedder(dim=D), enable_async=False,
                        load_from_disk=False, db_dir=str(tmp_path / name), **kw)


def _fill(ms):
    """6 topics x 8 near-duplicate memories around the embedding q of QUERY:
    duplicate j of topic t is ``a q + b u_t + 0.02 v_j`` (unit) with
    a = 0.9 - 0.1 t - 0.01 j and q, u_t, v_j orthonormal. So cos(q, .)
    falls by 0.1 per topic and 0.01 per duplicate, two memories of a topic
    have cosine > 0.999 and memories of two topics about a a'. Inserted in a
    shuffled order; id "t<t>d<j>"; odd duplicates are preferences.

    At diversity 0.5 a memory of a fresh topic scores 0.5 a - 0.5 * 0.9 a
    = 0.05 a against the first pick: 5e-4 between two duplicates (less
    2e-4 where they share v_j with a pick), 5e-3 between topics -- hundreds
    of times the fp32 error at this size (GAP)."""
    g = ms.graph
    q = np.asarray(ms._get_embedding(QUERY), dtype=np.float64)
    rng = np.random.default_rng(11)
    B = np.linalg.qr(np.concatenate([q[:, None], rng.standard_normal((D, TOPICS + DUPS))], 1))[0].T
    qd, U, V = B[0] * np.sign(B[0] @ q), B[1:1 + TOPICS], B[1 + TOPICS:]
    ids, rows, types = [], [], []
    for t in range(TOPICS):
        for j in range(DUPS):
            a = 0.9 - 0.1 * t - 0.01 * j
            rows.append(a * qd + np.sqrt(1.0 - a * a - 0.0004) * U[t] + 0.02 * V[j])
            ids.append(f"t{t}d{j}")
            types.append(TYPES[j % 2])
    o = rng.permutation(len(ids))
    g.add_nodes([ids[i] for i in o], [f"memory {ids[i]}" for i in o],
                torch.from_numpy(np.asarray(rows)[o].astype(np.float32)), shard=g.shard_id("rust"),
                types=[types[i] for i in o], stored=True)
    return qd


@pytest.fixture()
def ms(tmp_path):
    m = _system(tmp_path)
    _fill(m)
    yield m
    m.close()


def _ids(hits):
    return [n.id for n in hits]


def _topic(i):
    return i.split("d")[0]


def _oracle_ids(ms, query, k, delta, fetch_k, where=None, drop=()):
    """The fp64 greedy picks over the pool the plain search returns at
    k = fetch_k (rows of ``drop`` ids removed), as ids, and the fp64 gap."""
    g = ms.graph
    q = torch.as_tensor(np.asarray(ms._get_embedding(query), dtype=np.float32))
    _, rows = g.store_search(q, fetch_k, ms.store.metric, where=where)
    rows = rows.clone()
    for i in drop:
        rows[rows == g.row_of[i]] = -1
    X = g.emb32[: g.n].cpu().numpy()
    pick, _, gap = mmr_greedy64(X, q[None, :].numpy(), rows.numpy(), k, delta)
    return [g.ids[int(rows[0, s])] for s in pick[0] if s >= 0], float(gap[0])


def test_near_duplicates_collapse_to_one_per_topic(ms):
    plain = _ids(ms.search_memories(QUERY, limit=5))
    assert plain == [f"t0d{j}" for j in range(5)]  # five copies of one idea
    got = _ids(ms.search_memories(QUERY, limit=5, diversity=0.5, fetch_k=48))
    want, gap = _oracle_ids(ms, QUERY, 5, 0.5, 48)
    assert gap > GAP, gap  # (the margins are large by construction: fp32 cannot flip a pick)
    assert got == want == ["t0d0", "t1d0", "t2d0", "t3d0", "t4d0"]
    assert got[0] == plain[0] and len({_topic(i) for i in got}) == 5
    # the default pool (16 = two topics here) still alternates between what it holds
    small = _ids(ms.search_memories(QUERY, limit=5, diversity=0.5))
    assert small == _oracle_ids(ms, QUERY, 5, 0.5, 16)[0]
    assert small[0] == plain[0] and {_topic(i) for i in small} == {"t0", "t1"}
    # diversity 0: the pool by cosine, which for unit rows is the plain order
    assert _ids(ms.search_memories(QUERY, limit=5, diversity=0.0)) == plain


def test_surfaces_agree(ms):
    kw = dict(limit=4, diversity=0.5, fetch_k=40)
    single = [_ids(ms.search_memories(q, **kw)) for q in QUERIES]
    assert all(len(s) == 4 for s in single)
    assert [_ids(r) for r in ms.search_memories_batch(QUERIES, **kw)] == single
    batches = [QUERIES[:2], QUERIES[2:], QUERIES]
    streamed = [[_ids(r) for r in b] for b in ms.search_memories_stream(batches, **kw)]
    assert streamed == [single[:2], single[2:], single]
    emb = ms._get_embedding(QUERY)
    st = ms.vector_store
    assert st.search_nodes(emb, user_id=ms.user_id, limit=4, diversity=0.5, fetch_k=40) == single[0]
    assert st.search_nodes_batch([emb], user_id=ms.user_id, limit=4, diversity=0.5, fetch_k=40) == [single[0]]
    assert ms.graph.search_ids(torch.as_tensor(emb, dtype=torch.float32), 4, ms.store.metric, diversity=0.5,
                               fetch_k=40) == [single[0]]
    for q, s in zip(QUERIES, single):
        assert s == _oracle_ids(ms, q, 4, 0.5, 40)[0]


def test_none_is_the_plain_search(ms):
    for q in QUERIES:
        want = _ids(ms.search_memories(q, limit=6))
        assert _ids(ms.search_memories(q, limit=6, diversity=None, fetch_k=None)) == want
        assert [_ids(r) for r in ms.search_memories_batch([q], limit=6, diversity=None)] == [want]
    g = ms.graph
    q = torch.as_tensor(np.asarray(ms._get_embedding(QUERY), dtype=np.float32))
    a = g.store_search(q, 6, "l2")
    b = g.store_search(q, 6, "l2", diversity=None, fetch_k=None)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert ms.get_stats()["engine"]["mmr_searches"] == 0


def test_scores_are_the_pool_scores_in_pick_order(ms):
    g = ms.graph
    q = torch.as_tensor(np.asarray(ms._get_embedding(QUERY), dtype=np.float32))
    for metric in ("l2", "cosine", "ip"):
        ps, pr = g.store_search(q, 40, metric)
        s, r = g.store_search(q, 5, metric, diversity=0.5, fetch_k=40)
        assert [g.ids[i] for i in r[0].tolist()] == ["t0d0", "t1d0", "t2d0", "t3d0", "t4d0"]
        for sc, row in zip(s[0].tolist(), r[0].tolist()):
            at = (pr[0] == row).nonzero()
            assert at.numel() == 1 and ps[0, int(at)].item() == sc  # gathered: bit-equal
    # a pool larger than the tenant: padding once it ran out
    s, r = g.store_search(q, 60, "l2", diversity=0.3, fetch_k=64)
    assert (r[0, :48] >= 0).all() and len(set(r[0, :48].tolist())) == 48
    assert (r[0, 48:] == -1).all() and torch.isneginf(s[0, 48:]).all()


def test_composes_with_where(ms):
    flt = {"types": ["preference"]}
    got = ms.search_memories(QUERY, limit=5, where=flt, diversity=0.5, fetch_k=24)
    assert len(got) == 5 and all(n.type == "preference" for n in got)
    want, gap = _oracle_ids(ms, QUERY, 5, 0.5, 24, where=flt)
    assert gap > GAP and _ids(got) == want == ["t0d1", "t1d1", "t2d1", "t3d1", "t4d1"]
    assert [_ids(r) for r in ms.search_memories_batch([QUERY], limit=5, where=flt, diversity=0.5, fetch_k=24)] == [want]
    e = ms.get_stats()["engine"]
    assert e["filtered_searches"] == 3 and e["mmr_searches"] == 2  # (the oracle's pool search is filtered too)
    assert ms.search_memories(QUERY, limit=5, where={"types": ["no-such-type"]}, diversity=0.5) == []


def test_a_ghost_in_the_pool_takes_no_pick(ms):
    g = ms.graph
    qd = np.asarray(ms._get_embedding(QUERY), dtype=np.float64)
    qd /= np.linalg.norm(qd)
    X = g.emb32[: g.n].double().numpy()
    u = X[g.row_of["t5d0"]] - (X[g.row_of["t5d0"]] @ qd) * qd
    ghost = 0.95 * qd + np.sqrt(1 - 0.95 ** 2) * u / np.linalg.norm(u)  # nearer to the query than any memory
    g.add_nodes(["ghost0"], ["ghost"], torch.from_numpy(ghost[None, :].astype(np.float32)),
                shard=g.shard_id("rust", live=False), stored=True, ghost=True)
    q = torch.as_tensor(np.asarray(ms._get_embedding(QUERY), dtype=np.float32))
    assert g.ids[int(g.store_search(q, 16, "l2")[1][0, 0])] == "ghost0"  # it leads the pool
    want, gap = _oracle_ids(ms, QUERY, 5, 0.5, 48, drop=["ghost0"])
    assert gap > GAP and want[0] == "t0d0"
    for got in (ms.search_memories(QUERY, limit=5, diversity=0.5, fetch_k=48),
                ms.search_memories_batch([QUERY], limit=5, diversity=0.5, fetch_k=48)[0]):
        assert _ids(got) == want and len(got) == 5
    # had the ghost been a candidate it would have been the first pick
    assert _oracle_ids(ms, QUERY, 5, 0.5, 48)[0][0] == "ghost0"


def test_validation(ms):
    emb = ms._get_embedding(QUERY)
    q = torch.as_tensor(emb, dtype=torch.float32)
    bad = [dict(limit=5, diversity=0.5, fetch_k=MAX_FETCH_K + 1), dict(limit=20, diversity=0.5, fetch_k=16),
           dict(limit=5, diversity=1.5), dict(limit=5, diversity=-0.01), dict(limit=5, diversity=float("nan")),
           dict(limit=5, fetch_k=16), dict(limit=MAX_FETCH_K + 1, diversity=0.5), dict(limit=0, diversity=0.5)]
    for kw in bad:
        with pytest.raises(ValueError):
            ms.search_memories(QUERY, **kw)
        with pytest.raises(ValueError):
            ms.search_memories_batch([QUERY], **kw)
        with pytest.raises(ValueError):
            list(ms.search_memories_stream([[QUERY]], **kw))
        with pytest.raises(ValueError):
            ms.vector_store.search_nodes(emb, user_id=ms.user_id, **kw)
        kw = dict(kw)
        with pytest.raises(ValueError):
            ms.graph.store_search(q, kw.pop("limit"), "l2", **kw)
    assert ms.get_stats()["engine"]["mmr_searches"] == 0
    # the limits themselves are accepted
    assert len(ms.search_memories(QUERY, limit=40, diversity=1.0, fetch_k=MAX_FETCH_K)) == 40
    assert len(ms.search_memories(QUERY, limit=33, diversity=0.0)) == 33  # (default pool: min(64, 2 limit))


def test_out_of_scope_surfaces_raise(ms, tmp_path):
    from lazzaro_amd.core.vector_store import HBMStore
    from lazzaro_amd.parallel.service import DistributedMemoryService
    from lazzaro_amd.parallel.sharded_memory import ShardedMemorySystem
    emb = ms._get_embedding("q")
    for kw in (dict(diversity=0.5), dict(diversity=0.5, fetch_k=32)):
        with pytest.raises(NotImplementedError):
            ms.vector_store.search_nodes_multi([emb], [ms.user_id], **kw)
        # the checks come first: no distributed set-up is needed to reach them
        with pytest.raises(NotImplementedError):
            ShardedMemorySystem.search_memories_batch(None, ["q"], **kw)
        with pytest.raises(NotImplementedError):
            DistributedMemoryService.search_routed(None, ["u"], ["q"], **kw)
        with pytest.raises(NotImplementedError):
            next(DistributedMemoryService.search_routed_stream(None, [(["u"], ["q"])], **kw))
        with pytest.raises(NotImplementedError):
            DistributedMemoryService.search_global_batch(None, ["q"], **kw)
        with pytest.raises(NotImplementedError):
            DistributedMemoryService.search_global(None, torch.zeros(D), **kw)
    # a tenant of a store that has no graph attached has no fp32 rows to compare
    st = HBMStore(db_dir=str(tmp_path / "plain"), device="cpu")
    st.add_nodes([{"id": "a", "content": "c", "vector": [1.0] + [0.0] * (D - 1)}], user_id="u")
    assert st.search_nodes([1.0] + [0.0] * (D - 1), user_id="u") == ["a"]
    with pytest.raises(NotImplementedError):
        st.search_nodes([1.0] + [0.0] * (D - 1), user_id="u", diversity=0.5)
    with pytest.raises(NotImplementedError):
        st.search_nodes_batch([[1.0] + [0.0] * (D - 1)], user_id="u", diversity=0.5)
    st.close()


def test_dashboard_search_parameters(ms):
    from fastapi.testclient import TestClient

    from lazzaro_amd.dashboard import api
    api.set_memory_system(ms)
    try:
        c = TestClient(api.app)
        plain = [h["id"] for h in c.get("/api/search", params={"q": QUERY, "limit": 5}).json()]
        assert plain == [f"t0d{j}" for j in range(5)]
        got = [h["id"] for h in c.get("/api/search", params={"q": QUERY, "limit": 5, "diversity": 0.5,
                                                             "fetch_k": 48}).json()]
        assert got == ["t0d0", "t1d0", "t2d0", "t3d0", "t4d0"]
        both = [h["id"] for h in c.get("/api/search", params={"q": QUERY, "limit": 3, "diversity": 0.5, "fetch_k": 24,
                                                              "types": "preference"}).json()]
        assert both == ["t0d1", "t1d1", "t2d1"]
        assert [h["id"] for h in c.get("/api/search", params={"q": QUERY, "limit": 5, "diversity": 0.5}).json()] == \
            _ids(ms.search_memories(QUERY, limit=5, diversity=0.5))
    finally:
        api.set_memory_system(None)


def test_counter(ms):
    assert ms.get_stats()["engine"]["mmr_searches"] == 0
    ms.search_memories(QUERY)  # plain: counts nothing
    ms.search_memories(QUERY, where={"types": ["semantic"]})
    assert ms.get_stats()["engine"]["mmr_searches"] == 0
    ms.search_memories(QUERY, diversity=0.3)
    ms.search_memories_batch(QUERIES, limit=3, diversity=0.3)  # one store search per batch
    list(ms.search_memories_stream([QUERIES, QUERIES[:1]], limit=3, diversity=0.3, where={"types": ["semantic"]}))
    e = ms.get_stats()["engine"]
    assert e["mmr_searches"] == 4 and e["filtered_searches"] == 3
