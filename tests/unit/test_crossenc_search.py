"""Cross-encoder re-ranking (``rerank=``) on the CPU tier, through MemorySystem
with the hashing embedder and a random-init ``tiny`` re-ranker: every public
surface against the oracle's selection over the returned logits, the pool
against the inner search, validation before any work, the surfaces that do not
take it, the token column's upkeep, the counters, and ``rerank=None``."""
import numpy as np
import pytest
import torch

from lazzaro_amd.core.crossenc import CrossRerank
from lazzaro_amd.core.memory_system import MemorySystem
from lazzaro_amd.core.providers import HashEmbedder, LocalLLM
from lazzaro_amd.core.search_spec import SearchSpec
from tests.kernels import _crossenc_ref as R

D = 32
N = 40
WORDS = ["alpha", "beta", "gamma", "router", "kernel", "memory", "garden", "violin", "harbor", "lantern", "orchid",
         "quartz", "ticket", "billing", "invoice", "sunrise"]
QUERIES = ["which violin does the orchid garden prefer?", "router kernel memory", "billing"]


def _system(tmp_path, name="db", index_params=None, **kw):
    ip = {"reranker": "tiny"} if index_params is None else index_params
    return MemorySystem(llm_provider=LocalLLM(), embedding_provider=HashEmbedder(dim=D), enable_async=False,
                        load_from_disk=False, db_dir=str(tmp_path / name), index_params=ip, **kw)


def _fill(ms, n=N):
    g = ms.graph
    rng = np.random.default_rng(11)
    texts = [" ".join(rng.choice(WORDS, size=int(rng.integers(1, 9)))) for _ in range(n)]
    emb = np.asarray([ms._get_embedding(t) for t in texts], dtype=np.float32)
    types = ["preference" if i % 3 == 0 else "semantic" for i in range(n)]
    g.add_nodes([f"m{i}" for i in range(n)], texts, torch.from_numpy(emb), shard=g.shard_id("w"), types=types,
                sal=torch.linspace(0.05, 0.95, n), stored=True)
    return texts


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


def _oracle_logits(g, pool, queries):
    """fp64 logits [M, P] of the engine's pool, from the contents."""
    ce = g.reranker
    col = g.token_column()
    tok, dlen = col.state()
    from lazzaro_amd.ops.crossenc_ops import as_query_tokens
    qtok, qlen = as_query_tokens(queries, ce.tokenizer)
    pairs = R.pair_assembly(pool.numpy(), qtok, qlen, tok, dlen, ce.cfg.max_pos, col.L, *ce.special_ids)
    lg, _ = R.forward64(R.params64(ce.p), ce.cfg, pairs)
    return R.pool_logits(lg.numpy(), pool.numpy(), g.n)


@pytest.mark.parametrize("inner", [{}, {"where": {"types": ["preference"]}}, {"lexical": 0.5}, {"boost": 0.5},
                                   {"expand": 1}], ids=["plain", "where", "lexical", "boost", "expand"])
def test_surfaces_agree_and_match_the_oracle(ms, inner):
    g = ms.graph
    Q = _embs(ms, QUERIES)
    P, k = 8, 3
    terms = {"query_terms": QUERIES} if "lexical" in inner else {}
    s, r, lg = g.store_search_rerank(Q, k, ms.store.metric, rerank=P, query_tokens=QUERIES, **inner, **terms)
    assert s.shape == r.shape == (3, k) and lg.shape == (3, P) and r.dtype == torch.long and lg.dtype == torch.float32
    # the pool: the inner options' own search at k = P with node_rows
    _, pool = g.store_search(Q, P, ms.store.metric, node_rows=True, **inner, **terms)
    assert torch.equal(torch.isinf(lg), pool < 0)
    # the logits: the fp64 oracle over the contents' tokens (fp32 tier: the bound of test_crossenc_ref_cpu)
    want = _oracle_logits(g, pool, QUERIES)
    live = ~np.isinf(want)
    assert np.abs(lg.double().numpy()[live] - want[live]).max() <= 1e-4
    # the result: the oracle's selection over the returned logits; the score is the logit
    ws, wr = R.select(lg.double().numpy(), pool.numpy(), k)
    assert np.array_equal(r.numpy(), wr) and np.array_equal(s.double().numpy(), ws) and (r >= 0).all()
    s2, r2 = g.store_search(Q, k, ms.store.metric, rerank={"pool": P}, query_tokens=QUERIES, **inner, **terms)
    assert torch.equal(s2, s) and torch.equal(r2, r)
    # tokens given as (ids, lens)
    from lazzaro_amd.ops.crossenc_ops import as_query_tokens
    qtok, qlen = as_query_tokens(QUERIES, g.reranker.tokenizer)
    s3, r3 = g.store_search(Q, k, ms.store.metric, rerank=CrossRerank(P), query_tokens=(qtok[:, :40], qlen), **inner,
                            **terms)
    assert torch.equal(r3, r) and int(qlen.max()) <= 40
    # every surface above it
    want_ids = [[g.ids[x] for x in row] for row in r.tolist()]
    assert g.search_ids(Q, k, ms.store.metric, rerank=P, query_tokens=QUERIES, **inner, **terms) == want_ids
    st = ms.vector_store
    assert st.search_nodes_batch(Q, user_id=ms.user_id, limit=k, rerank=P, query_texts=QUERIES, **inner) == want_ids
    assert st.search_nodes(Q[0], user_id=ms.user_id, limit=k, rerank=P, query_text=QUERIES[0], **inner) == want_ids[0]
    assert [_ids(b) for b in ms.search_memories_batch(QUERIES, limit=k, rerank=P, **inner)] == want_ids
    assert [_ids(ms.search_memories(q, limit=k, rerank={"pool": P}, **inner)) for q in QUERIES] == want_ids
    got = list(ms.search_memories_stream([QUERIES[:2], QUERIES[2:]], limit=k, rerank=P, **inner))
    assert [_ids(b) for batch in got for b in batch] == want_ids


def test_defaults_and_the_pool_range(ms):
    assert CrossRerank.coerce(True) == CrossRerank(16) == CrossRerank.coerce({}) and CrossRerank.coerce(None) is None
    assert CrossRerank.coerce(24).pool == 24 and CrossRerank.coerce(CrossRerank(7)).pool == 7
    assert CrossRerank.coerce(False) is None and SearchSpec.of(5, rerank=False) is None
    assert len(ms.search_memories(QUERIES[0], limit=16, rerank=True)) == 16
    assert len(ms.search_memories(QUERIES[0], limit=5, rerank=64)) == 5
    assert len(ms.search_memories(QUERIES[0], limit=1, rerank=1)) == 1
    spec = SearchSpec.of(5, where={"types": ["preference"]}, rerank=True)
    assert spec.rerank == CrossRerank(16) and spec.only("where", "expand", "boost", "lexical").rerank is None
    assert spec.only("expand", "boost") is None and set(spec.kwargs(query_text="q")) == {"where", "rerank", "query_text"}
    assert SearchSpec.of(5, **{k: v for k, v in spec.kwargs().items()}) == spec


def test_validation_comes_before_any_work(ms, tmp_path, monkeypatch):
    g = ms.graph
    calls = []
    monkeypatch.setattr(ms, "_get_embedding", lambda *a, **k: calls.append(a) or [0.0] * D)
    monkeypatch.setattr(ms, "_batch_embed_any", lambda *a, **k: calls.append(a) or torch.zeros((1, D)))
    for bad in (0, 65, -3, 2.5, "16", {"pool": 4}, {"pool": 16, "blend": 0.5}, {"size": 16}, 4, [16]):
        with pytest.raises(ValueError):  # out of range, below the limit 5, an unknown field, a wrong type
            ms.search_memories("q", limit=5, rerank=bad)
        with pytest.raises(ValueError):
            ms.search_memories_batch(["q"], limit=5, rerank=bad)
    with pytest.raises(ValueError):
        ms.search_memories(None, limit=5, rerank=True)  # a missing query text
    with pytest.raises(ValueError):
        ms.search_memories_batch(["q", None], limit=5, rerank=True)
    with pytest.raises(ValueError):
        next(ms.search_memories_stream([["q", 3]], limit=5, rerank=True))
    with pytest.raises(NotImplementedError):  # two final selectors
        ms.search_memories("q", limit=5, rerank=True, diversity=0.3)
    with pytest.raises(NotImplementedError):
        ms.search_memories_batch(["q"], limit=5, rerank=True, fetch_k=20)
    assert calls == []
    monkeypatch.undo()
    q = _embs(ms, ["q"])
    with pytest.raises(ValueError):
        g.store_search(q, 5, "l2", rerank=True)  # no query_tokens=
    with pytest.raises(ValueError):
        g.store_search_rerank(q, 5, "l2", rerank=None, query_tokens=["q"])
    with pytest.raises(ValueError):
        g.store_search(q, 5, "l2", rerank=True, query_tokens=["q", "r"])  # one query, the tokens of two
    with pytest.raises(ValueError):
        g.store_search(q, 5, "l2", rerank=True, query_tokens=(np.zeros((1, 65), np.int32), np.zeros(1, np.int32)))
    with pytest.raises(ValueError):
        ms.vector_store.search_nodes(q[0], user_id=ms.user_id, limit=5, rerank=True)  # no query_text=
    with pytest.raises(ValueError):
        ms.vector_store.search_nodes_batch(q, user_id=ms.user_id, limit=5, rerank=True, query_texts=["a", "b"])
    with pytest.raises(NotImplementedError):
        g.store_search(q, 5, "l2", rerank=True, query_tokens=["q"], diversity=0.5)
    with pytest.raises(ValueError):  # the lexical pool must hold the re-ranker's
        ms.search_memories("q", limit=5, rerank=32, lexical={"alpha": 0.5, "pool": 16})
    assert ms.get_stats()["engine"]["reranked_searches"] == 0 and g._token_column is None


def test_a_store_without_a_reranker_raises_before_any_work(tmp_path, monkeypatch):
    m = _system(tmp_path, name="off", index_params={})
    try:
        _fill(m, 10)
        calls = []
        monkeypatch.setattr(m, "_get_embedding", lambda *a, **k: calls.append(a) or [0.0] * D)
        monkeypatch.setattr(m, "_batch_embed_any", lambda *a, **k: calls.append(a) or torch.zeros((1, D)))
        with pytest.raises(ValueError, match="reranker"):
            m.search_memories("q", limit=3, rerank=True)
        with pytest.raises(ValueError, match="reranker"):
            m.search_memories_batch(["q"], limit=3, rerank=8)
        with pytest.raises(ValueError, match="reranker"):
            next(m.search_memories_stream([["q"]], limit=3, rerank=8))
        assert calls == []
        q = torch.zeros((1, D))
        with pytest.raises(ValueError, match="reranker"):
            m.graph.store_search(q, 3, "l2", rerank=True, query_tokens=["q"])
        with pytest.raises(ValueError, match="reranker"):
            m.graph.store_search_rerank(q, 3, "l2", rerank=True, query_tokens=["q"])
        with pytest.raises(ValueError, match="reranker"):
            m.vector_store.search_nodes_batch(q, user_id=m.user_id, limit=3, rerank=True, query_texts=["q"])
        with pytest.raises(ValueError, match="reranker"):
            m.graph.token_column()
    finally:
        m.close()


def test_store_settings(tmp_path):
    import inspect
    from lazzaro_amd.config import MemoryConfig
    from lazzaro_amd.core.vector_store import HBMStore
    c = MemoryConfig()
    assert (c.reranker, c.reranker_weights, c.reranker_vocab, c.rerank_doc_tokens) == (None, None, None, 64)
    assert "reranker" not in inspect.signature(MemorySystem.__init__).parameters
    for bad in ({"reranker": "no-such-model"}, {"reranker": "tiny", "rerank_doc_tokens": 48},
                {"rerank_doc_tokens": 256}):
        with pytest.raises(ValueError):
            HBMStore(db_dir=str(tmp_path / "bad"), device="cpu", **bad)
    # a vocabulary above 65,536 does not fit the column's 16-bit ids
    from lazzaro_amd.models import encoder as enc
    from lazzaro_amd.models.cross_encoder import CrossEncoder
    big = enc.EncoderConfig("big-vocab", 128, 1, 2, 256, vocab=70000, max_pos=128)
    with pytest.raises(ValueError, match="16-bit"):
        CrossEncoder(big, device="cpu")
    m = _system(tmp_path, name="l32", index_params={"reranker": "tiny", "rerank_doc_tokens": 32})
    try:
        _fill(m, 12)
        assert len(m.search_memories(QUERIES[1], limit=3, rerank=4)) == 3
        col = m.graph._token_column
        assert col.L == 32 and col.tok.shape[1] == 32 and col.tok.dtype == torch.int16 and col.dlen.dtype == torch.int32
        assert col.nbytes() == m.graph.n * (2 * 32 + 4)
    finally:
        m.close()


def test_out_of_scope_surfaces_raise(ms, tmp_path):
    from lazzaro_amd.core.vector_store import HBMStore
    from lazzaro_amd.parallel.service import DistributedMemoryService
    from lazzaro_amd.parallel.sharded_memory import ShardedMemorySystem
    emb = ms._get_embedding("q")
    q = torch.as_tensor(emb, dtype=torch.float32)[None]
    kw = dict(rerank=True)
    with pytest.raises(NotImplementedError):
        ms.search_memories_fused(["a", "b"], limit=3, **kw)
    with pytest.raises(NotImplementedError):
        ms.search_memories_fused_batch([["a", "b"]], limit=3, **kw)
    with pytest.raises(NotImplementedError):
        ms.vector_store.search_nodes_fused(q, [0, 1], user_id=ms.user_id, limit=3, query_texts=["a"], **kw)
    with pytest.raises(NotImplementedError):
        ms.graph.store_search_fused(q, [0, 1], 3, **kw)
    with pytest.raises(NotImplementedError):
        ms.graph.search_ids_fused(q, [0, 1], 3, **kw)
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
    # a tenant of a store that has no graph attached has no contents to read
    st = HBMStore(db_dir=str(tmp_path / "plain"), device="cpu", reranker="tiny")
    st.add_nodes([{"id": "a", "content": "c", "vector": [1.0] + [0.0] * (D - 1)}], user_id="u")
    with pytest.raises(NotImplementedError):
        st.search_nodes([1.0] + [0.0] * (D - 1), user_id="u", rerank=1, limit=1, query_text="c")
    with pytest.raises(NotImplementedError):
        st.search_nodes_batch([[1.0] + [0.0] * (D - 1)], user_id="u", rerank=1, limit=1, query_texts=["c"])
    st.close()
    assert ms.get_stats()["engine"]["reranked_searches"] == 0


def _same_as_fresh(g):
    from lazzaro_amd.engine.token_column import TokenColumn
    col = g.token_column()
    got = col.state()
    want = TokenColumn(g, col.tokenizer, col.L, g.reranker.cfg.vocab).sync().state()
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # and the contract's rule, text by text
    tok = col.tokenizer
    for r in (0, g.n // 2, g.n - 1):
        body = tok.encode(g.content[r] or "", col.L + 2)[1:-1]
        assert got[1][r] == len(body) and got[0][r, :len(body)].tolist() == body and not got[0][r, len(body):].any()
    return got


def test_token_column_upkeep(tmp_path):
    ms = _system(tmp_path)
    try:
        _fill(ms)
        g = ms.graph
        assert g._token_column is None  # nothing is built before the first re-ranked search
        ms.search_memories(QUERIES[0], limit=2)
        assert g._token_column is None and ms.get_stats()["engine"]["token_column_builds"] == 0
        ms.search_memories(QUERIES[0], limit=2, rerank=4)
        n0 = g.n
        col = g._token_column
        assert len(_same_as_fresh(g)[1]) == n0 and col.builds == 1
        # appended rows (one longer than L: its first L pieces are kept)
        long_text = " ".join(WORDS * 8)
        g.add_nodes(["new0", "new1"], [long_text, ""], torch.from_numpy(np.eye(D, dtype=np.float32)[:2]),
                    shard=g.shard_id("w"), stored=True)
        assert col.covered == n0
        st = _same_as_fresh(g)
        assert col.covered == n0 + 2 and st[1][n0] == col.L and st[1][n0 + 1] == 0 and col.builds == 1
        # a re-added id: its content is rewritten in place
        g.add_nodes(["new1"], ["giraffe crossing"], torch.from_numpy(np.eye(D, dtype=np.float32)[1:2]),
                    shard=g.shard_id("w"), stored=True)
        assert _same_as_fresh(g)[1][g.row_of["new1"]] > 0
        # NodeView.content = ...
        ms.buffer.get_node("m3").content = "nothing to see"
        assert col.dirty == [g.row_of["m3"]]
        st = _same_as_fresh(g)
        assert st[1][g.row_of["m3"]] == len(col.tokenizer.encode("nothing to see", 66)) - 2 and col.builds == 1
        # compact(): rows move, the epoch changes; the column is dropped and rebuilt at the next use
        g.remove_nodes([g.row_of["m1"]], drop_edges=True, unstore=True)
        g.take_dirty_rows(), g.take_dirty_edges(), g.take_deleted()
        moved = g.row_of["new0"]
        out = g.compact()
        assert out["reclaimed"] > 0 and g.row_of["new0"] < moved and col.builds == 1 and col.epoch == 0
        ms.search_memories(QUERIES[0], limit=2, rerank=4)
        assert col.builds == 2 and col.epoch == g.row_epoch == 1 and col.covered == g.n
        assert _same_as_fresh(g)[1][g.row_of["new0"]] == col.L
        # another L: a new column, counted as a build
        g.rerank_doc_tokens = 32
        ms.search_memories(QUERIES[0], limit=2, rerank=4)
        assert g._token_column is not col and g._token_column.L == 32 and g._token_column.builds == 3
        _same_as_fresh(g)
        assert ms.get_stats()["engine"]["token_column_builds"] == 3
    finally:
        ms.close()


def test_none_is_the_plain_search_and_the_counters_count(ms, monkeypatch):
    import lazzaro_amd.engine.token_column as colmod
    import lazzaro_amd.models.cross_encoder as cemod
    import lazzaro_amd.ops.crossenc_ops as ops

    def boom(*a, **k):
        raise AssertionError("rerank=None reached the new code")
    for mod, names in ((ops, ("ce_lens", "ce_embed_ln", "ce_head_select", "as_query_tokens", "body_pieces")),
                       (colmod, ("TokenColumn",)), (cemod.CrossEncoder, ("rerank", "pooled"))):
        for name in names:
            monkeypatch.setattr(mod, name, boom)
    g = ms.graph
    for qy in QUERIES:
        want = _ids(ms.search_memories(qy, limit=6))
        assert _ids(ms.search_memories(qy, limit=6, rerank=None)) == want
        assert [_ids(r) for r in ms.search_memories_batch([qy], limit=6, rerank=None)] == [want]
        assert [[_ids(r) for r in b] for b in ms.search_memories_stream([[qy]], limit=6, rerank=None)] == [[want]]
    q = _embs(ms, QUERIES[:1])
    for kw in ({}, {"where": {"types": ["semantic"]}}, {"diversity": 0.3}, {"boost": 0.5}):
        a = g.store_search(q, 6, "l2", **kw)
        b = g.store_search(q, 6, "l2", rerank=None, query_tokens=QUERIES[:1], **kw)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    e = ms.get_stats()["engine"]
    assert e["reranked_searches"] == e["rerank_pairs"] == e["token_column_builds"] == 0 and g._token_column is None
    monkeypatch.undo()
    ms.search_memories(QUERIES[0], rerank=True)                       # 1 x 16
    ms.search_memories_batch(QUERIES, limit=3, rerank=8)              # one store search per batch: 3 x 8
    list(ms.search_memories_stream([QUERIES, QUERIES[:1]], limit=3, rerank=4, where={"types": ["semantic"]}))  # 16
    g.store_search_rerank(_embs(ms, QUERIES[:2]), 2, "l2", rerank=2, query_tokens=QUERIES[:2])  # 2 x 2
    e = ms.get_stats()["engine"]
    assert e["reranked_searches"] == 5 and e["rerank_pairs"] == 16 + 24 + 12 + 4 + 4 and e["token_column_builds"] == 1


def test_an_empty_tenant_and_short_pools(tmp_path):
    m = _system(tmp_path, name="empty")
    try:
        assert m.search_memories("q", limit=3, rerank=True) == []
        _fill(m, 4)
        got = m.search_memories_batch(QUERIES, limit=3, rerank=8, where={"types": ["preference"]})
        assert [len(b) for b in got] == [2, 2, 2]  # rows 0 and 3 pass: the padding is dropped
        s, r, lg = m.graph.store_search_rerank(_embs(m, QUERIES), 3, "l2", rerank=8, query_tokens=QUERIES)
        assert (r[:, :3] >= 0).all() and torch.isinf(lg[:, 4:]).all() and not torch.isinf(lg[:, :4]).any()
        s, r, lg = m.graph.store_search_rerank(_embs(m, QUERIES), 6, "l2", rerank=8, query_tokens=QUERIES)
        assert (r[:, 4:] == -1).all() and torch.isinf(s[:, 4:]).all() and (r[:, :4] >= 0).all()
    finally:
        m.close()


def test_dashboard_search_parameters(ms):
    from fastapi.testclient import TestClient

    from lazzaro_amd.dashboard import api
    api.set_memory_system(ms)
    try:
        c = TestClient(api.app)
        q = QUERIES[0]
        got = [h["id"] for h in c.get("/api/search", params={"q": q, "limit": 4, "rerank": "true"}).json()]
        assert got == _ids(ms.search_memories(q, limit=4, rerank=True))
        got = [h["id"] for h in c.get("/api/search", params={"q": q, "limit": 4, "rerank": "true", "rerank_pool": 32,
                                                             "types": "preference"}).json()]
        assert got == _ids(ms.search_memories(q, limit=4, rerank=32, where={"types": ["preference"]}))
        plain = [h["id"] for h in c.get("/api/search", params={"q": q, "limit": 4, "rerank_pool": 32}).json()]
        assert plain == _ids(ms.search_memories(q, limit=4))  # given alone it changes nothing
    finally:
        api.set_memory_system(None)
