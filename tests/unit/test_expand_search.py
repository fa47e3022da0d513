"""Associative memory search (``expand=``) on the CPU tier, through
MemorySystem with the hashing embedder: a memory that answers only through a
link, the public surfaces, composition with ``where=`` and ``diversity=``,
validation, the unsupported surfaces and the counter."""
import numpy as np
import pytest
import torch

from lazzaro_amd.core.expand import MAX_LIMIT, GraphExpand
from lazzaro_amd.core.memory_system import MemorySystem
from lazzaro_amd.core.providers import HashEmbedder, LocalLLM
from tests.kernels._expand_ref import expand64

D = 32
FILLERS = 20
QUERY = "what about the deadline?"
QUERIES = [QUERY, "favourite food", "trip to the mountains last week"]


def _system(tmp_path, name="db", **kw):
    return MemorySystem(llm_provider=LocalLLM(), embedding_provider=HashEmbedder(dim=D), enable_async=False,
                        load_from_disk=False, db_dir=str(tmp_path / name), **kw)


def _fill(ms):
    """Around the embedding q of QUERY (unit rows ``a q + sqrt(1 - a^2) u_i``,
    the u_i orthonormal): "deadline" at cosine 0.9, FILLERS memories at
    0.30, 0.29, ... 0.11 (odd ones preferences), and "friday" at 0.05 -- the
    farthest of all, not even a seed -- linked to "deadline" with weight 0.9
    and to "f19" with 0.2 (below the cut). Expanded by one hop with the
    defaults, "friday" scores 0.5 * 0.05 + 0.5 * (0.9 * 0.85 * 0.9) = 0.369
    against the fillers' own cosines of at most 0.30: margins of 0.07, far
    above any fp32 error at this size."""
    g = ms.graph
    q = np.asarray(ms._get_embedding(QUERY), dtype=np.float64)
    rng = np.random.default_rng(11)
    B = np.linalg.qr(np.concatenate([q[:, None], rng.standard_normal((D, FILLERS + 2))], 1))[0].T
    qd, U = B[0] * np.sign(B[0] @ q), B[1:]
    ids = ["deadline"] + [f"f{i}" for i in range(FILLERS)] + ["friday"]
    cos = [0.9] + [0.30 - 0.01 * i for i in range(FILLERS)] + [0.05]
    rows = np.stack([a * qd + np.sqrt(1.0 - a * a) * u for a, u in zip(cos, U)])
    o = rng.permutation(len(ids))
    g.add_nodes([ids[i] for i in o], [f"memory {ids[i]}" for i in o], torch.from_numpy(rows[o].astype(np.float32)),
                shard=g.shard_id("work"), types=["preference" if ids[i][0] == "f" and ids[i][1:].isdigit()
                                                 and int(ids[i][1:]) % 2 else "semantic" for i in o], stored=True)
    r = g.row_of
    sh = g.shard_id("work")
    g.append_edges_host([r["friday"], r["friday"]], [r["deadline"], r["f19"]], np.array([0.9, 0.2], np.float32),
                        np.array([sh, sh]), g.etype("relates_to"))
    return qd


@pytest.fixture()
def ms(tmp_path):
    m = _system(tmp_path)
    _fill(m)
    yield m
    m.close()


def _ids(hits):
    return [n.id for n in hits]


def _q(ms, text=QUERY):
    return torch.as_tensor(np.asarray(ms._get_embedding(text), dtype=np.float32))


def _oracle_ids(ms, query, k, spec, where_ok=None):
    """The fp64 oracle over the tenant's own seeds, as ids."""
    g = ms.graph
    sp = GraphExpand.coerce(spec)
    q = _q(ms, query)
    n = g.n
    bias = g.store_bias("l2").numpy().copy()
    _, seeds = g.store_search(q, sp.seed_k, ms.store.metric, node_rows=True)
    if where_ok is not None:
        bias[[i for i in range(n) if not where_ok(g.ids[i])]] = -np.inf
        seeds = torch.where(torch.isfinite(torch.from_numpy(bias))[seeds.clamp_min(0)] & (seeds >= 0), seeds,
                            torch.full_like(seeds, -1))
    ref = expand64(g.emb32[:n].numpy(), q[None, :].numpy(), seeds.numpy(), tuple(t.numpy() for t in g.csr()),
                   g.e["w"].numpy(), g.kind[:n].numpy(), g.sup[:n].numpy(), bias, sp)[0]
    return [g.ids[int(r)] for r in ref.rows[ref.order[:k]]]


def test_a_linked_memory_comes_back_only_with_expand(ms):
    plain = _ids(ms.search_memories(QUERY, limit=3))
    assert plain == ["deadline", "f0", "f1"]
    assert "friday" not in _ids(ms.search_memories(QUERY, limit=FILLERS + 1))  # the farthest of all
    got = _ids(ms.search_memories(QUERY, limit=3, expand=1))
    assert got == ["deadline", "friday", "f0"] == _oracle_ids(ms, QUERY, 3, 1)
    # graph_weight 0: the candidates by cosine -- friday is reached, and last
    assert _ids(ms.search_memories(QUERY, limit=3, expand={"graph_weight": 0.0})) == plain
    assert _ids(ms.search_memories(QUERY, limit=64, expand={"graph_weight": 0.0}))[-1] == "friday"
    # the cut: with min_weight above 0.9 the link does not carry, and nothing else is linked
    assert _ids(ms.search_memories(QUERY, limit=3, expand={"min_weight": 0.95})) == plain
    # via: friday was carried by deadline, the seeds by themselves
    g = ms.graph
    s, r, via = g.store_search_expand(_q(ms), 3, "l2", expand=1)
    assert [g.ids[i] for i in r[0].tolist()] == got
    assert via[0].tolist() == [-1, g.row_of["deadline"], -1]
    assert s[0, 1].item() == pytest.approx(0.5 * 0.05 + 0.5 * 0.9 * 0.85 * 0.9, abs=1e-5)
    # two hops reach f19 through friday's weak link only if the cut lets it pass
    two = GraphExpand(hops=2, fanout=4, min_weight=0.1, graph_weight=1.0)
    s, r, via = g.store_search_expand(_q(ms), 64, "l2", expand=two)
    at = r[0].tolist().index(g.row_of["f19"])
    assert via[0, at].item() == g.row_of["friday"] or via[0, at].item() == -1  # (f19 is a seed too: own 0.11 may win)
    assert s[0, at].item() == pytest.approx(max(0.11, 0.9 * 0.85 * 0.9 * 0.85 * 0.2), abs=1e-5)


def test_surfaces_agree(ms):
    kw = dict(limit=4, expand=GraphExpand(hops=1))
    single = [_ids(ms.search_memories(q, **kw)) for q in QUERIES]
    assert all(len(s) == 4 for s in single) and "friday" in single[0]
    assert [_ids(r) for r in ms.search_memories_batch(QUERIES, **kw)] == single
    batches = [QUERIES[:2], QUERIES[2:], QUERIES]
    assert [[_ids(r) for r in b] for b in ms.search_memories_stream(batches, **kw)] == [single[:2], single[2:], single]
    emb = ms._get_embedding(QUERY)
    st = ms.vector_store
    assert st.search_nodes(emb, user_id=ms.user_id, limit=4, expand=1) == single[0]
    assert st.search_nodes_batch([emb], user_id=ms.user_id, limit=4, expand={"hops": 1}) == [single[0]]
    assert ms.graph.search_ids(_q(ms), 4, ms.store.metric, expand=1) == [single[0]]
    for q, s in zip(QUERIES, single):
        assert s == _oracle_ids(ms, q, 4, 1)


def test_none_is_the_plain_search(ms):
    for q in QUERIES:
        want = _ids(ms.search_memories(q, limit=6))
        assert _ids(ms.search_memories(q, limit=6, expand=None)) == want
        assert [_ids(r) for r in ms.search_memories_batch([q], limit=6, expand=None)] == [want]
    g = ms.graph
    a = g.store_search(_q(ms), 6, "l2")
    b = g.store_search(_q(ms), 6, "l2", expand=None)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert ms.get_stats()["engine"]["expanded_searches"] == 0


def test_composes_with_where_and_diversity(ms):
    # friday is "semantic": a filter on preferences masks it as a target as well
    flt = {"types": ["preference"]}
    got = ms.search_memories(QUERY, limit=5, where=flt, expand=1)
    assert _ids(got) == ["f1", "f3", "f5", "f7", "f9"] and all(n.type == "preference" for n in got)
    flt = {"types": ["semantic"]}
    got = _ids(ms.search_memories(QUERY, limit=3, where=flt, expand=1))
    assert got == ["deadline", "friday", "f0"]
    assert got == _oracle_ids(ms, QUERY, 3, 1, where_ok=lambda i: not (i[1:].isdigit() and int(i[1:]) % 2))
    # with diversity= the MMR pool is the expanded search at fetch_k
    g = ms.graph
    from lazzaro_amd.ops.mmr_ops import mmr_select
    ps, pr = g.store_search(_q(ms), 16, "l2", node_rows=True, expand=1)
    s, r = g.store_search(_q(ms), 4, "l2", node_rows=True, diversity=0.3, fetch_k=16, expand=1)
    pick, _ = mmr_select(g.emb32[: g.n], _q(ms)[None, :], pr, 4, 0.3)
    assert torch.equal(r, torch.gather(pr, 1, pick.long())) and torch.equal(s, torch.gather(ps, 1, pick.long()))
    assert g.row_of["friday"] in pr[0].tolist()
    assert _ids(ms.search_memories(QUERY, limit=4, diversity=0.3, fetch_k=16, expand=1)) == \
        [g.ids[i] for i in r[0].tolist()]


def test_validation(ms):
    emb = ms._get_embedding(QUERY)
    bad = [dict(expand=0), dict(expand=4), dict(expand={"hops": 0}), dict(expand={"fanout": 17}),
           dict(expand={"fanout": 0}), dict(expand={"seed_k": 17}), dict(expand={"seed_k": 0}),
           dict(expand=2),                                  # 16 * 9^2 = 1296 > 1024 with the default fanout
           dict(expand={"hops": 3, "fanout": 4}),           # 16 * 5^3 = 2000
           dict(expand=1, limit=MAX_LIMIT + 1), dict(expand=1, limit=0),
           dict(expand={"graph_weight": 1.5}), dict(expand={"graph_weight": -0.1}),
           dict(expand={"decay": 0.0}), dict(expand={"decay": 1.01}), dict(expand={"decay": float("nan")}),
           dict(expand={"min_weight": -0.5}), dict(expand={"no_such_field": 1})]
    for kw in bad:
        kw = dict({"limit": 5}, **kw)
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
            ms.graph.store_search(_q(ms), kw.pop("limit"), "l2", **kw)
    with pytest.raises(TypeError):
        ms.search_memories(QUERY, expand="two")
    assert ms.get_stats()["engine"]["expanded_searches"] == 0
    # the limits themselves are accepted
    # (16 seeds and friday: everything this graph lets them reach)
    assert len(ms.search_memories(QUERY, limit=MAX_LIMIT, expand=GraphExpand(hops=2, fanout=7))) == 17
    assert len(ms.search_memories(QUERY, limit=5, expand=dict(hops=3, fanout=3, seed_k=16, decay=1.0,
                                                              graph_weight=1.0, min_weight=0.0))) == 5


def test_out_of_scope_surfaces_raise(ms, tmp_path):
    from lazzaro_amd.core.vector_store import HBMStore
    from lazzaro_amd.parallel.service import DistributedMemoryService
    from lazzaro_amd.parallel.sharded_memory import ShardedMemorySystem
    emb = ms._get_embedding("q")
    for kw in (dict(expand=1), dict(expand=GraphExpand(hops=2, fanout=4))):
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
    # a tenant of a store that has no graph attached has no links to follow
    st = HBMStore(db_dir=str(tmp_path / "plain"), device="cpu")
    st.add_nodes([{"id": "a", "content": "c", "vector": [1.0] + [0.0] * (D - 1)}], user_id="u")
    assert st.search_nodes([1.0] + [0.0] * (D - 1), user_id="u") == ["a"]
    with pytest.raises(NotImplementedError):
        st.search_nodes([1.0] + [0.0] * (D - 1), user_id="u", expand=1)
    with pytest.raises(NotImplementedError):
        st.search_nodes_batch([[1.0] + [0.0] * (D - 1)], user_id="u", expand=1)
    st.close()


def test_dashboard_search_parameters(ms):
    from fastapi.testclient import TestClient

    from lazzaro_amd.dashboard import api
    api.set_memory_system(ms)
    try:
        c = TestClient(api.app)
        plain = [h["id"] for h in c.get("/api/search", params={"q": QUERY, "limit": 3}).json()]
        assert plain == ["deadline", "f0", "f1"]
        got = [h["id"] for h in c.get("/api/search", params={"q": QUERY, "limit": 3, "hops": 1}).json()]
        assert got == ["deadline", "friday", "f0"]
        got = [h["id"] for h in c.get("/api/search", params={"q": QUERY, "limit": 3, "fanout": 4,
                                                             "graph_weight": 0.0}).json()]
        assert got == plain
        both = [h["id"] for h in c.get("/api/search", params={"q": QUERY, "limit": 3, "hops": 1,
                                                              "types": "semantic"}).json()]
        assert both == ["deadline", "friday", "f0"]
    finally:
        api.set_memory_system(None)


def test_counter_and_a_new_link_is_seen(ms):
    assert ms.get_stats()["engine"]["expanded_searches"] == 0
    ms.search_memories(QUERY)  # plain: counts nothing
    ms.search_memories(QUERY, diversity=0.3)
    assert ms.get_stats()["engine"]["expanded_searches"] == 0
    ms.search_memories(QUERY, expand=1)
    ms.search_memories_batch(QUERIES, limit=3, expand=1)  # one store search per batch
    list(ms.search_memories_stream([QUERIES, QUERIES[:1]], limit=3, expand=1, where={"types": ["semantic"]}))
    ms.search_memories(QUERY, limit=3, expand=1, diversity=0.3)
    e = ms.get_stats()["engine"]
    assert e["expanded_searches"] == 5 and e["filtered_searches"] == 2 and e["mmr_searches"] == 2
    # a link added after a search is followed by the next one (the CSR is cached per edge version)
    g = ms.graph
    assert _ids(ms.search_memories(QUERY, limit=2, expand=1)) == ["deadline", "friday"]
    sh = g.shard_id("work")
    g.append_edges_host([g.row_of["deadline"]], [g.row_of["f18"]], np.array([1.0], np.float32), np.array([sh]),
                        g.etype("relates_to"))
    # f18: 0.5 * 0.12 + 0.5 * (0.9 * 0.85) = 0.4425 > friday's 0.369
    assert _ids(ms.search_memories(QUERY, limit=3, expand=1)) == ["deadline", "f18", "friday"]
