"""Keyword and hybrid search (``lexical=``) on the CPU tier, through
MemorySystem with the hashing embedder: a memory only a literal token finds,
the public surfaces, composition with ``where=`` and ``diversity=``,
validation, the unsupported surfaces, the lexicon's upkeep and the counters."""
import numpy as np
import pytest
import torch

from lazzaro_amd.core.lexical import LexicalSearch
from lazzaro_amd.core.memory_system import MemorySystem
from lazzaro_amd.core.providers import HashEmbedder, LocalLLM

D = 32
N_FILL = 60
QUERY = "LZ-4812"
QUERIES = [QUERY, "violin orchid", "harbor lantern quartz"]
WORDS = ["alpha", "beta", "gamma", "router", "kernel", "memory", "garden", "violin", "harbor", "lantern", "orchid",
         "quartz"]


def _system(tmp_path, name="db", **kw):
    return MemorySystem(llm_provider=LocalLLM(), embedding_provider=HashEmbedder(dim=D), enable_async=False,
                        load_from_disk=False, db_dir=str(tmp_path / name), **kw)


def _fill(ms):
    """60 memories of common words with cos(q, .) spread over [-0.15, 0.2]
    around the embedding q of QUERY, and two that hold the token: "needle"
    (semantic) at cosine -0.2 and "needle2" (preference) at -0.25 -- further
    from the query than 50 others, so no dense top-5 holds them. With the
    token twice in a short memory, lexn is about 0.6: at alpha 0.5 the needle
    blends to about 0.2, twice the best other memory's 0.5 * 0.2."""
    g = ms.graph
    q = np.asarray(ms._get_embedding(QUERY), dtype=np.float64)
    q /= np.linalg.norm(q)
    rng = np.random.default_rng(4)

    def at(c):
        u = rng.standard_normal(D)
        u -= (u @ q) * q
        return c * q + np.sqrt(1 - c * c) * u / np.linalg.norm(u)

    cosines = np.linspace(-0.15, 0.2, N_FILL)
    rows = [at(c) for c in cosines] + [at(-0.2), at(-0.25)]
    texts = [" ".join(rng.choice(WORDS, size=8)) for _ in range(N_FILL)]
    texts += ["ticket LZ-4812 reopened LZ-4812", "LZ-4812 billing preference LZ-4812"]
    ids = [f"m{i}" for i in range(N_FILL)] + ["needle", "needle2"]
    types = ["semantic" if i % 2 == 0 else "preference" for i in range(N_FILL)] + ["semantic", "preference"]
    g.add_nodes(ids, texts, torch.from_numpy(np.asarray(rows, dtype=np.float32)), shard=g.shard_id("w"), types=types,
                stored=True)


@pytest.fixture()
def ms(tmp_path):
    m = _system(tmp_path)
    _fill(m)
    yield m
    m.close()


def _ids(hits):
    return [n.id for n in hits]


def test_finds_a_literal_token(ms):
    plain = _ids(ms.search_memories(QUERY, limit=5))
    assert len(plain) == 5 and "needle" not in plain and "needle2" not in plain
    for alpha in (0.5, 1.0):
        got = _ids(ms.search_memories(QUERY, limit=5, lexical=alpha))
        assert got[:2] == ["needle", "needle2"], (alpha, got)
    # keyword search alone returns the matches and nothing else
    assert _ids(ms.search_memories(QUERY, limit=5, lexical=1.0)) == ["needle", "needle2"]
    # alpha = 0: the union of the pools by cosine -- the dense order for unit rows
    assert _ids(ms.search_memories(QUERY, limit=5, lexical=0.0)) == plain
    s, r = ms.graph.lexical_topk([QUERY, "no such token"], 4)
    assert [ms.graph.ids[i] for i in r[0].tolist() if i >= 0] == ["needle", "needle2"]
    assert (r[1] == -1).all() and torch.isneginf(s[1]).all() and (s[0, :2] > 0).all()


def test_surfaces_agree(ms):
    kw = dict(limit=4, lexical={"alpha": 0.4, "pool": 24})
    single = [_ids(ms.search_memories(q, **kw)) for q in QUERIES]
    assert all(len(s) == 4 for s in single) and single[0][0] == "needle"
    assert [_ids(r) for r in ms.search_memories_batch(QUERIES, **kw)] == single
    batches = [QUERIES[:2], QUERIES[2:], QUERIES]
    assert [[_ids(r) for r in b] for b in ms.search_memories_stream(batches, **kw)] == [single[:2], single[2:], single]
    embs = [ms._get_embedding(q) for q in QUERIES]
    st = ms.vector_store
    assert st.search_nodes(embs[0], user_id=ms.user_id, query_text=QUERIES[0], **kw) == single[0]
    assert st.search_nodes_batch(embs, user_id=ms.user_id, query_texts=QUERIES, **kw) == single
    Q = torch.as_tensor(np.asarray(embs), dtype=torch.float32)
    lx = LexicalSearch(alpha=0.4, pool=24)
    assert ms.graph.search_ids(Q, 4, ms.store.metric, lexical=lx, query_terms=QUERIES) == single
    # the terms themselves serve as well as the texts
    from lazzaro_amd.core.lexical import query_terms
    assert ms.graph.search_ids(Q, 4, ms.store.metric, lexical=lx, query_terms=query_terms(QUERIES)) == single
    # scores: descending blends in [-1, 1]
    s, r = ms.graph.store_search(Q, 4, ms.store.metric, lexical=lx, query_terms=QUERIES)
    assert (s[:, :-1] >= s[:, 1:]).all() and (s.abs() <= 1).all() and (r >= 0).all()


def test_where_is_honoured(ms):
    flt = {"types": ["preference"]}
    for alpha in (0.5, 1.0):
        got = ms.search_memories(QUERY, limit=5, where=flt, lexical=alpha)
        assert got and all(n.type == "preference" for n in got)
        assert _ids(got)[0] == "needle2" and "needle" not in _ids(got)
    assert [_ids(r) for r in ms.search_memories_batch([QUERY], limit=5, where=flt, lexical=1.0)] == [["needle2"]]
    assert ms.search_memories(QUERY, limit=5, where={"types": ["no-such-type"]}, lexical=0.5) == []
    assert ms.search_memories(QUERY, limit=5, where={"exclude_ids": ["needle", "needle2"]}, lexical=1.0) == []


def test_composes_with_diversity(ms):
    from lazzaro_amd.ops.mmr_ops import mmr_select
    g = ms.graph
    q = torch.as_tensor(np.asarray(ms._get_embedding(QUERY), dtype=np.float32))[None, :]
    ps, pr = g.store_search(q, 16, ms.store.metric, node_rows=True, lexical=0.5, query_terms=[QUERY])
    pick, _ = mmr_select(g.emb32[: g.n], q, pr, 4, 0.3)
    want = [g.ids[int(pr[0, p])] for p in pick[0].tolist()]
    got = _ids(ms.search_memories(QUERY, limit=4, lexical=0.5, diversity=0.3))
    assert got == want and len(set(got)) == 4 and "needle" in [g.ids[int(i)] for i in pr[0].tolist()]
    assert [_ids(r) for r in ms.search_memories_batch([QUERY], limit=4, lexical=0.5, diversity=0.3)] == [want]
    e = ms.get_stats()["engine"]
    assert e["mmr_searches"] == 2 and e["lexical_searches"] == 3


def test_validation(ms):
    emb = ms._get_embedding(QUERY)
    q = torch.as_tensor(emb, dtype=torch.float32)
    bad = [dict(lexical=-0.1), dict(lexical=1.5), dict(lexical=float("nan")), dict(lexical=True), dict(lexical="0.5"),
           dict(lexical={"pool": 16}), dict(lexical={"alpha": 0.5, "pool": 65}), dict(lexical={"alpha": 0.5, "pool": 0}),
           dict(lexical={"alpha": 0.5, "pool": 4}), dict(lexical={"alpha": 0.5, "k1": -1.0}),
           dict(lexical={"alpha": 0.5, "k1": float("inf")}), dict(lexical={"alpha": 0.5, "b": 1.5}),
           dict(lexical={"alpha": 0.5, "b": -0.5}), dict(lexical={"alpha": 0.5, "rank": 1}),
           dict(lexical={"alpha": 0.5, "pool": 2.5}), dict(lexical=0.5, limit=17),
           dict(lexical=0.5, diversity=0.5, fetch_k=32)]  # (the pool of the fused search must hold fetch_k)
    before = ms.get_stats()["engine"]["lexical_searches"]
    for kw in bad:
        kw = dict({"limit": 5}, **kw)
        with pytest.raises(ValueError):
            ms.search_memories(QUERY, **kw)
        with pytest.raises(ValueError):
            ms.search_memories_batch([QUERY], **kw)
        with pytest.raises(ValueError):
            list(ms.search_memories_stream([[QUERY]], **kw))
        with pytest.raises(ValueError):
            ms.vector_store.search_nodes(emb, user_id=ms.user_id, query_text=QUERY, **kw)
        kw2 = dict(kw)
        with pytest.raises(ValueError):
            ms.graph.store_search(q, kw2.pop("limit"), "l2", query_terms=[QUERY], **kw2)
    # lexical without text
    with pytest.raises(ValueError):
        ms.vector_store.search_nodes(emb, user_id=ms.user_id, lexical=0.5)
    with pytest.raises(ValueError):
        ms.vector_store.search_nodes_batch([emb], user_id=ms.user_id, lexical=0.5)
    with pytest.raises(ValueError):
        ms.vector_store.search_nodes_batch([emb, emb], user_id=ms.user_id, lexical=0.5, query_texts=[QUERY])
    with pytest.raises(ValueError):
        ms.graph.store_search(q, 5, "l2", lexical=0.5)
    with pytest.raises(ValueError):
        ms.graph.store_search(q, 5, "l2", lexical=0.5, query_terms=[QUERY, QUERY])  # two texts, one query
    with pytest.raises(ValueError):
        ms.search_memories(None, lexical=0.5)
    assert ms.get_stats()["engine"]["lexical_searches"] == before and ms.graph._lexicon is None
    # the limits themselves are accepted
    assert len(ms.search_memories(QUERY, limit=40, lexical={"alpha": 0.0, "pool": 64, "k1": 0.0, "b": 1.0})) == 40
    assert len(ms.search_memories(QUERY, limit=16, lexical=0)) == 16


def test_out_of_scope_surfaces_raise(ms, tmp_path):
    from lazzaro_amd.core.vector_store import HBMStore
    from lazzaro_amd.parallel.service import DistributedMemoryService
    from lazzaro_amd.parallel.sharded_memory import ShardedMemorySystem
    emb = ms._get_embedding("q")
    q = torch.as_tensor(emb, dtype=torch.float32)
    kw = dict(lexical=0.5)
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
    # with expand= or boost=
    for other in (dict(expand=1), dict(boost=0.5)):
        with pytest.raises(NotImplementedError):
            ms.search_memories("q", lexical=0.5, **other)
        with pytest.raises(NotImplementedError):
            ms.search_memories_batch(["q"], lexical=0.5, **other)
        with pytest.raises(NotImplementedError):
            ms.vector_store.search_nodes(emb, user_id=ms.user_id, lexical=0.5, query_text="q", **other)
        with pytest.raises(NotImplementedError):
            ms.graph.store_search(q, 5, "l2", lexical=0.5, query_terms=["q"], **other)
    # a tenant of a store that has no graph attached has no contents to read
    st = HBMStore(db_dir=str(tmp_path / "plain"), device="cpu")
    st.add_nodes([{"id": "a", "content": "c", "vector": [1.0] + [0.0] * (D - 1)}], user_id="u")
    with pytest.raises(NotImplementedError):
        st.search_nodes([1.0] + [0.0] * (D - 1), user_id="u", lexical=0.5, query_text="c")
    with pytest.raises(NotImplementedError):
        st.search_nodes_batch([[1.0] + [0.0] * (D - 1)], user_id="u", lexical=0.5, query_texts=["c"])
    st.close()
    # a tenant without fp32 rows
    g = ms.graph
    keep, g.emb32 = g.emb32, None
    try:
        with pytest.raises(NotImplementedError):
            g.store_search(q, 5, "l2", lexical=1.0, query_terms=["q"])
    finally:
        g.emb32 = keep
    assert ms.get_stats()["engine"]["lexical_searches"] == 0


def _same_as_fresh(g):
    from lazzaro_amd.engine.lexicon import Lexicon
    got, want = g.lexicon().state(), Lexicon(g, g.lexical_slots).sync().state()
    for a, b in zip(got, want):
        assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b
    return got


def test_lexicon_upkeep(tmp_path):
    ms = _system(tmp_path, merge_mode="pairwise")
    try:
        _fill(ms)
        g = ms.graph
        assert g._lexicon is None  # nothing is built before the first lexical search
        assert _ids(ms.search_memories(QUERY, limit=2, lexical=1.0)) == ["needle", "needle2"]
        n0 = g.n
        assert _same_as_fresh(g)[4] == n0 and g._lexicon.builds == 1
        # appended rows
        g.add_nodes(["new0", "new1"], ["zebra LZ-4812", "zebra crossing"], torch.from_numpy(
            np.eye(D, dtype=np.float32)[:2]), shard=g.shard_id("w"), stored=True)
        assert g._lexicon.covered == n0
        assert sorted(_ids(ms.search_memories("zebra", limit=5, lexical=1.0))) == ["new0", "new1"]
        _same_as_fresh(g)
        # a re-added id: its content is rewritten in place
        g.add_nodes(["new1"], ["giraffe crossing"], torch.from_numpy(np.eye(D, dtype=np.float32)[1:2]),
                    shard=g.shard_id("w"), stored=True)
        assert _ids(ms.search_memories("zebra", limit=5, lexical=1.0)) == ["new0"]
        assert _ids(ms.search_memories("giraffe", limit=5, lexical=1.0)) == ["new1"]
        _same_as_fresh(g)
        # NodeView.content = ...
        ms.buffer.get_node("needle").content = "nothing to see"
        assert sorted(_ids(ms.search_memories(QUERY, limit=5, lexical=1.0))) == ["needle2", "new0"]
        _same_as_fresh(g)
        # a pairwise merge: "a | b" holds both contents' words
        v = np.zeros((2, D), dtype=np.float32)
        v[:, 5], v[1, 6] = 1.0, 1e-3
        g.add_nodes(["dup0", "dup1"], ["walrus tusk", "walrus ivory"], torch.from_numpy(v), shard=g.shard_id("w"),
                    stored=True)
        assert _ids(ms.search_memories("ivory", limit=5, lexical=1.0)) == ["dup1"]
        assert ms._merge_similar_nodes(0.99) >= 1
        assert _ids(ms.search_memories("ivory", limit=5, lexical=1.0)) == ["dup0"]
        _same_as_fresh(g)
        # eviction: the row is no longer returned; its terms count until the next rebuild (the documented limit)
        g.remove_nodes([g.row_of["new0"]], drop_edges=True, unstore=True)
        assert _ids(ms.search_memories("zebra", limit=5, lexical=1.0)) == []
        st = _same_as_fresh(g)
        builds = g._lexicon.builds
        # compact(): the evicted and the merged row leave (once nothing pending refers to them), the rows
        # behind them slide down, the epoch moves; the lexicon is dropped and rebuilt over the survivors
        g.take_dirty_rows(), g.take_dirty_edges(), g.take_deleted()
        moved = g.row_of["dup0"]
        out = g.compact()
        assert out["reclaimed"] > 0 and g.row_epoch == out["epoch"] == 1 and g.row_of["dup0"] < moved
        assert g._lexicon.builds == builds and g._lexicon.epoch == 0  # (nothing happens before the next use)
        assert _ids(ms.search_memories("ivory", limit=5, lexical=1.0)) == ["dup0"]  # (a row that moved)
        assert _ids(ms.search_memories("zebra", limit=5, lexical=1.0)) == []
        assert sorted(_ids(ms.search_memories(QUERY, limit=5, lexical=1.0))) == ["needle2"]  # (new0 is gone)
        assert g._lexicon.builds == builds + 1 and g._lexicon.epoch == 1
        assert g._lexicon.covered == g.n == len(st[1]) - out["reclaimed"]
        fresh = _same_as_fresh(g)
        # the evicted row's terms no longer count: the rebuild's df table has lost "zebra"
        from lazzaro_amd.core.lexical import term_id
        assert term_id("zebra") in st[2].tolist() and term_id("zebra") not in fresh[2].tolist()
        e = ms.get_stats()["engine"]
        assert e["lexicon_rows"] == g.n and e["lexicon_builds"] == g._lexicon.builds
    finally:
        ms.close()


def test_none_is_the_plain_search_and_the_counters_count(ms, monkeypatch):
    import lazzaro_amd.engine.lexicon as lexmod
    import lazzaro_amd.ops.lex_ops as ops

    def boom(*a, **k):
        raise AssertionError("lexical=None reached the new code")
    for mod, names in ((ops, ("lex_topk", "lex_fuse", "lex_topk_ref", "lex_fuse_ref", "tile_tables")),
                       (lexmod, ("Lexicon",))):
        for name in names:
            monkeypatch.setattr(mod, name, boom)
    g = ms.graph
    for qy in QUERIES:
        want = _ids(ms.search_memories(qy, limit=6))
        assert _ids(ms.search_memories(qy, limit=6, lexical=None)) == want
        assert [_ids(r) for r in ms.search_memories_batch([qy], limit=6, lexical=None)] == [want]
        assert [[_ids(r) for r in b] for b in ms.search_memories_stream([[qy]], limit=6, lexical=None)] == [[want]]
    q = torch.as_tensor(np.asarray(ms._get_embedding(QUERY), dtype=np.float32))
    for kw in ({}, {"where": {"types": ["semantic"]}}, {"diversity": 0.3}):
        a = g.store_search(q, 6, "l2", **kw)
        b = g.store_search(q, 6, "l2", lexical=None, query_terms=[QUERY], **kw)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    e = ms.get_stats()["engine"]
    assert e["lexical_searches"] == 0 and e["lexicon_rows"] == 0 and e["lexicon_builds"] == 0 and g._lexicon is None
    monkeypatch.undo()
    ms.search_memories(QUERY, lexical=0.5)
    ms.search_memories_batch(QUERIES, limit=3, lexical=1.0)  # one store search per batch
    list(ms.search_memories_stream([QUERIES, QUERIES[:1]], limit=3, lexical=0.3, where={"types": ["semantic"]}))
    g.lexical_topk(QUERIES, 3)
    e = ms.get_stats()["engine"]
    assert e["lexical_searches"] == 5 and e["lexicon_rows"] == g.n and e["lexicon_builds"] == 1


def test_lexical_slots_setting(tmp_path):
    from lazzaro_amd.config import MemoryConfig
    assert MemoryConfig().lexical_slots == 16
    m = _system(tmp_path, index_params={"lexical_slots": 8})
    try:
        _fill(m)
        assert _ids(m.search_memories(QUERY, limit=2, lexical=1.0)) == ["needle", "needle2"]
        assert m.graph._lexicon.W == 8 and m.graph._lexicon.slots.shape[1] == 8
    finally:
        m.close()
    with pytest.raises(ValueError):
        _system(tmp_path, name="bad", index_params={"lexical_slots": 12})


def test_dashboard_search_parameters(ms):
    from fastapi.testclient import TestClient

    from lazzaro_amd.dashboard import api
    api.set_memory_system(ms)
    try:
        c = TestClient(api.app)
        plain = [h["id"] for h in c.get("/api/search", params={"q": QUERY, "limit": 5}).json()]
        assert "needle" not in plain
        got = [h["id"] for h in c.get("/api/search", params={"q": QUERY, "limit": 5, "lexical": 0.5}).json()]
        assert got[:2] == ["needle", "needle2"]
        got = [h["id"] for h in c.get("/api/search", params={"q": QUERY, "limit": 20, "lexical": 1.0,
                                                             "lexical_pool": 32, "types": "preference"}).json()]
        assert got == ["needle2"]
    finally:
        api.set_memory_system(None)
