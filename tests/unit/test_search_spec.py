"""``SearchSpec`` (core/search_spec.py): the search options coerced and checked
once, the refusals of the surfaces that take none, the stores that have no
graph, and every surface answering alike for every option set that composes.
A CPU tenant of 64 rows x 32 dims."""
from dataclasses import fields

import numpy as np
import pytest
import torch

from lazzaro_amd.core.boost import MemoryBoost
from lazzaro_amd.core.expand import MAX_LIMIT, GraphExpand
from lazzaro_amd.core.filters import MAX_EXCLUDE_IDS
from lazzaro_amd.core.memory_system import MemorySystem
from lazzaro_amd.core.providers import HashEmbedder, LocalLLM
from lazzaro_amd.core.search_spec import SearchSpec
from lazzaro_amd.core.vector_store import HBMStore
from lazzaro_amd.engine.tenant_graph import TenantGraph
from lazzaro_amd.ops.mmr_ops import MAX_FETCH_K
from lazzaro_amd.parallel.service import DistributedMemoryService
from lazzaro_amd.parallel.sharded_memory import ShardedMemorySystem
from tests.parity._differential_scenario import MemStore

D, N, K = 32, 64, 4
NOW = 1_700_000_000.0
DAY = 86400.0
QUERIES = ["violin orchid", "harbor lantern quartz", "kernel memory router"]
WORDS = ["alpha", "beta", "gamma", "router", "kernel", "memory", "garden", "violin", "harbor", "lantern", "orchid",
         "quartz"]


def _system(tmp_path, name="db", **kw):
    return MemorySystem(llm_provider=LocalLLM(), embedding_provider=HashEmbedder(dim=D), enable_async=False,
                        load_from_disk=False, db_dir=str(tmp_path / name), **kw)


def _rows():
    rng = np.random.default_rng(18)
    X = rng.standard_normal((N, D))
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    texts = [" ".join(rng.choice(WORDS, size=6)) for _ in range(N)]
    return [f"m{i}" for i in range(N)], texts, X.astype(np.float32), rng


def _fill(ms):
    """64 unit rows of common words, every other one a preference, saliences,
    uses and ages spread out, and a ring of links with a chord every 4 rows."""
    g = ms.graph
    ids, texts, X, rng = _rows()
    sh = g.shard_id("w")
    g.add_nodes(ids, texts, torch.from_numpy(X), shard=sh, types=["semantic" if i % 2 == 0 else "preference"
                                                                  for i in range(N)],
                sal=rng.uniform(0.1, 1.0, N).tolist(), acc=rng.integers(0, 12, N).tolist(),
                last=(NOW - DAY * rng.uniform(0.0, 30.0, N)).tolist(), ts=[NOW - 40 * DAY] * N, stored=True)
    src = list(range(N)) + list(range(0, N, 4))
    dst = [(i + 1) % N for i in range(N)] + [(i + 17) % N for i in range(0, N, 4)]
    g.append_edges_host(src, dst, rng.uniform(0.4, 0.9, len(src)).astype(np.float32), np.full(len(src), sh),
                        g.etype("relates_to"))


@pytest.fixture(scope="module")
def ms(tmp_path_factory):
    m = _system(tmp_path_factory.mktemp("spec"))
    _fill(m)
    yield m
    m.close()


def _ids(hits):
    return [n.id for n in hits]


W = {"types": ["semantic"]}
B = {"recency": 0.5, "salience": 0.3, "frequency": 0.2, "now": NOW}  # (a fixed ``now``: the surfaces share a clock)
E = {"hops": 1, "seed_k": 8}
L = {"alpha": 0.4, "pool": 24}
DV = {"diversity": 0.4}
ONE_OF_EACH = dict(where=W, diversity=0.5, fetch_k=32, expand=1, boost=1.0, lexical=0.5)


# ---------------------------------------------------------------- SearchSpec.of
def test_of_none_is_the_plain_search():
    assert SearchSpec.of(5) is None
    assert SearchSpec.of(0, None, None, None, None, None, None) is None  # (the limit is the plain search's business)


def test_of_coerces_and_is_idempotent(monkeypatch):
    import lazzaro_amd.core.boost as CB
    calls = []
    monkeypatch.setattr(CB, "_clock", lambda: calls.append(1) or NOW)
    for kw in (dict(where=W, diversity=0.5, fetch_k=16, expand=1, boost=1.0), dict(boost={"recency": 1.0}),
               dict(where=W, lexical=0.5, diversity=1), dict(expand=E)):
        del calls[:]
        a = SearchSpec.of(K, **kw)
        b = SearchSpec.of(K, **{f.name: getattr(a, f.name) for f in fields(a)})
        assert a == b and len(calls) == ("boost" in kw), kw
        assert SearchSpec.of(K, **a.kwargs()) == a
        assert set(a.kwargs()) == {f.name for f in fields(a) if getattr(a, f.name) is not None} >= set(kw)
        assert a.boost is None or a.boost.now == NOW
        assert a.diversity is None or isinstance(a.diversity, float)
    a = SearchSpec.of(K, boost=MemoryBoost(recency=1.0, now=5.0))
    assert a.boost.now == 5.0 and not calls  # a ``now`` that is set stays
    # the texts of a lexical search join the keyword arguments, and only those of a lexical search
    assert SearchSpec.of(K, lexical=0.5).kwargs(query_text="q")["query_text"] == "q"
    assert "query_text" not in SearchSpec.of(K, where=W).kwargs(query_text="q")


BAD_VALUE = (
    # tests/unit/test_lexical_search.py::test_validation
    [dict(lexical=-0.1), dict(lexical=1.5), dict(lexical=float("nan")), dict(lexical=True), dict(lexical="0.5"),
     dict(lexical={"pool": 16}), dict(lexical={"alpha": 0.5, "pool": 65}), dict(lexical={"alpha": 0.5, "pool": 0}),
     dict(lexical={"alpha": 0.5, "pool": 4}), dict(lexical={"alpha": 0.5, "k1": -1.0}),
     dict(lexical={"alpha": 0.5, "k1": float("inf")}), dict(lexical={"alpha": 0.5, "b": 1.5}),
     dict(lexical={"alpha": 0.5, "b": -0.5}), dict(lexical={"alpha": 0.5, "rank": 1}),
     dict(lexical={"alpha": 0.5, "pool": 2.5}), dict(lexical=0.5, limit=17),
     dict(lexical=0.5, diversity=0.5, fetch_k=32)]
    # tests/unit/test_mmr_search.py::test_validation
    + [dict(limit=5, diversity=0.5, fetch_k=MAX_FETCH_K + 1), dict(limit=20, diversity=0.5, fetch_k=16),
       dict(limit=5, diversity=1.5), dict(limit=5, diversity=-0.01), dict(limit=5, diversity=float("nan")),
       dict(limit=5, fetch_k=16), dict(limit=MAX_FETCH_K + 1, diversity=0.5), dict(limit=0, diversity=0.5)]
    # tests/unit/test_expand_search.py::test_validation
    + [dict(expand=0), dict(expand=4), dict(expand={"hops": 0}), dict(expand={"fanout": 17}),
       dict(expand={"fanout": 0}), dict(expand={"seed_k": 17}), dict(expand={"seed_k": 0}), dict(expand=2),
       dict(expand={"hops": 3, "fanout": 4}), dict(expand=1, limit=MAX_LIMIT + 1), dict(expand=1, limit=0),
       dict(expand={"graph_weight": 1.5}), dict(expand={"graph_weight": -0.1}), dict(expand={"decay": 0.0}),
       dict(expand={"decay": 1.01}), dict(expand={"decay": float("nan")}), dict(expand={"min_weight": -0.5}),
       dict(expand={"no_such_field": 1})]
    # tests/unit/test_boost_search.py::test_validation
    + [dict(boost=b) for b in (
        -1.0, float("nan"), 8.5, {"salience": -0.1}, {"recency": float("inf")}, {"recency_scale": 0.0},
        {"clock": "modified"}, {"type_weights": {"a": -1.0}}, {"now": float("nan")}, {"no_such_field": 1},
        {"salience": 2.0, "frequency": 1.5, "recency": 1.0},
        {"salience": 2.0, "recency": 1.5, "type_weights": {"a": 0.75}})]
    # tests/unit/test_filtered_search.py
    + [dict(where={"typos": ["a"]}), dict(where={"exclude_ids": [f"x{i}" for i in range(MAX_EXCLUDE_IDS + 1)]})]
    # a limit that only the expansion bounds, with a boost beside it
    + [dict(boost=1.0, expand=1, limit=65)])
BAD_TYPE = [dict(expand="two"), dict(boost="much"), dict(where=["types"])]


@pytest.mark.parametrize("kw", BAD_VALUE, ids=repr)
def test_of_raises_value_errors(kw):
    kw = dict(kw)
    with pytest.raises(ValueError):
        SearchSpec.of(kw.pop("limit", 5), **kw)


@pytest.mark.parametrize("kw", BAD_TYPE, ids=repr)
def test_of_raises_type_errors(kw):
    with pytest.raises(TypeError):
        SearchSpec.of(5, **kw)


def test_of_refuses_what_does_not_compose():
    for other in (dict(expand=1), dict(boost=0.5)):
        with pytest.raises(NotImplementedError):
            SearchSpec.of(5, lexical=0.5, **other)
    # the limits themselves are accepted
    assert SearchSpec.of(MAX_LIMIT, expand=GraphExpand(hops=2, fanout=7), boost=1.0).expand.fanout == 7
    assert SearchSpec.of(40, lexical={"alpha": 0.0, "pool": 64}, diversity=1.0, fetch_k=MAX_FETCH_K).fetch_k == 64
    assert SearchSpec.of(40, expand=1, diversity=0.5).diversity == 0.5  # (the pool bounds the limit then)


# ---------------------------------------------------------------- refusals
DMS = DistributedMemoryService
SURFACES = {
    "search_nodes_multi": lambda kw: HBMStore.search_nodes_multi(None, [[0.0] * D], ["u"], **kw),
    "ShardedMemorySystem.search_memories_batch":
        lambda kw: ShardedMemorySystem.search_memories_batch(None, ["q"], **kw),
    "DistributedMemoryService.search_routed": lambda kw: DMS.search_routed(None, ["u"], ["q"], **kw),
    "DistributedMemoryService.search_routed_stream":
        lambda kw: next(DMS.search_routed_stream(None, [(["u"], ["q"])], **kw)),
    "DistributedMemoryService.search_global_batch": lambda kw: DMS.search_global_batch(None, ["q"], **kw),
    "DistributedMemoryService.search_global": lambda kw: DMS.search_global(None, torch.zeros(D), **kw),
}


@pytest.mark.parametrize("option", sorted(ONE_OF_EACH))
@pytest.mark.parametrize("surface", sorted(SURFACES))
def test_surfaces_that_take_no_option_refuse(surface, option):
    # the check comes first: ``self`` is None, no distributed set-up is needed to reach it
    with pytest.raises(NotImplementedError) as e:
        SURFACES[surface]({option: ONE_OF_EACH[option]})
    assert f"{option}=" in str(e.value) and surface in str(e.value)


def test_refuse_names_the_first_option_set():
    SearchSpec.refuse("here", where=None, boost=None)
    with pytest.raises(NotImplementedError, match=r"here .* boost="):
        SearchSpec.refuse("here", where=None, boost=0.0, lexical=1.0)


# ---------------------------------------------------------------- stores without the tenant's graph
def test_a_store_without_the_graph_answers_the_plain_search_only(tmp_path):
    st = HBMStore(db_dir=str(tmp_path / "plain"), device="cpu")
    e0 = [1.0] + [0.0] * (D - 1)
    st.add_nodes([{"id": "a", "content": "c", "vector": e0}], user_id="u")
    assert st.search_nodes(e0, user_id="u") == ["a"] and st.search_nodes_batch([e0], user_id="u") == [["a"]]
    for name in ("where", "diversity", "expand", "boost", "lexical"):
        kw = {name: ONE_OF_EACH[name]}
        with pytest.raises(NotImplementedError, match=f"{name}="):
            st.search_nodes(e0, user_id="u", query_text="q", **kw)
        with pytest.raises(NotImplementedError, match=f"{name}="):
            st.search_nodes_batch([e0], user_id="u", query_texts=["q"], **kw)
    st.close()


class RecordingStore(MemStore):
    """A store of the reference's interface and nothing more: ``search_nodes``
    takes (emb, user_id, limit) and any other keyword is a TypeError."""

    def __init__(self):
        super().__init__()
        self.calls = []

    def search_nodes(self, query_vector, user_id="default", limit=5):
        self.calls.append(("search_nodes", user_id, limit))
        return super().search_nodes(query_vector, user_id, limit)


class RecordingBatchStore(RecordingStore):
    def search_nodes_batch(self, query_vectors, user_id="default", limit=5):
        self.calls.append(("search_nodes_batch", user_id, limit))
        return [MemStore.search_nodes(self, q, user_id, limit) for q in query_vectors]


@pytest.mark.parametrize("store_cls", (RecordingStore, RecordingBatchStore))
def test_a_store_of_the_reference_interface(tmp_path, monkeypatch, store_cls):
    st = store_cls()
    m = _system(tmp_path, store=st)
    try:
        ids, texts, X, _ = _rows()
        m.graph.add_nodes(ids, texts, torch.from_numpy(X), shard=m.graph.shard_id("w"), stored=True)
        st.add_nodes([{"id": i, "content": t, "embedding": x.tolist()} for i, t, x in zip(ids, texts, X)],
                     user_id=m.user_id)
        del st.calls[:]
        want = [_ids(m.search_memories(q, limit=K)) for q in QUERIES]
        assert all(len(w) == K for w in want) and st.calls == [("search_nodes", m.user_id, K)] * 3
        del st.calls[:]
        assert [_ids(r) for r in m.search_memories_batch(QUERIES, limit=K)] == want
        assert [[_ids(r) for r in b] for b in m.search_memories_stream([QUERIES], limit=K)] == [want]
        batched = store_cls is RecordingBatchStore
        assert st.calls == ([("search_nodes_batch", m.user_id, K)] * 2 if batched
                            else [("search_nodes", m.user_id, K)] * 6)
        # an option needs the bound store's graph: refused before anything is embedded
        embeds = []
        monkeypatch.setattr(m, "_get_embedding", lambda *a, **kw: embeds.append(a))
        monkeypatch.setattr(m, "_batch_embed_any", lambda *a, **kw: embeds.append(a))
        del st.calls[:]
        for name in ("where", "diversity", "expand", "boost", "lexical"):
            kw = {name: ONE_OF_EACH[name]}
            with pytest.raises(NotImplementedError, match=f"{name}="):
                m.search_memories(QUERIES[0], limit=K, **kw)
            with pytest.raises(NotImplementedError, match=f"{name}="):
                m.search_memories_batch(QUERIES, limit=K, **kw)
            with pytest.raises(NotImplementedError, match=f"{name}="):
                next(m.search_memories_stream([QUERIES], limit=K, **kw))
        assert not embeds and not st.calls
    finally:
        m.close()


# ---------------------------------------------------------------- every surface, every composable option set
OPTION_SETS = [dict(where=W), DV, dict(DV, fetch_k=24), dict(expand=E), dict(boost=B), dict(lexical=L),
               dict(where=W, **DV), dict(where=W, expand=E), dict(where=W, boost=B), dict(where=W, lexical=L),
               dict(DV, expand=E), dict(DV, boost=B), dict(DV, lexical=L),
               dict(where=W, boost=B, expand=E, **DV)]


@pytest.mark.parametrize("kw", [{}] + OPTION_SETS, ids=lambda kw: "+".join(sorted(kw)) or "plain")
def test_surfaces_agree(ms, kw):
    lex = "lexical" in kw
    single = [_ids(ms.search_memories(q, limit=K, **kw)) for q in QUERIES]
    assert all(len(s) == K and len(set(s)) == K for s in single)
    if "where" in kw:
        assert all(int(i[1:]) % 2 == 0 for s in single for i in s)
    assert [_ids(r) for r in ms.search_memories_batch(QUERIES, limit=K, **kw)] == single
    assert [[_ids(r) for r in b] for b in ms.search_memories_stream([QUERIES], limit=K, **kw)] == [single]
    embs = [ms._get_embedding(q) for q in QUERIES]
    st, g, metric = ms.vector_store, ms.graph, ms.store.metric
    for q, e, s in zip(QUERIES, embs, single):
        assert st.search_nodes(e, user_id=ms.user_id, limit=K, **dict(kw, query_text=q) if lex else kw) == s
    assert st.search_nodes_batch(embs, user_id=ms.user_id, limit=K,
                                 **dict(kw, query_texts=QUERIES) if lex else kw) == single
    Q = torch.as_tensor(np.asarray(embs), dtype=torch.float32)
    ekw = dict(kw, query_terms=QUERIES) if lex else kw
    assert g.search_ids(Q, K, metric, **ekw) == single
    _, r = g.store_search(Q, K, metric, node_rows=True, **ekw)
    assert [[g.ids[x] for x in row if x >= 0] for row in r.tolist()] == single
    # the coerced options serve as well as the given ones
    spec = SearchSpec.of(K, **kw)
    if spec is not None:
        assert [_ids(r) for r in ms.search_memories_batch(QUERIES, limit=K, **spec.kwargs())] == single


def test_each_option_changes_the_answer(ms):
    """(the table above would pass if every option were ignored alike)"""
    plain = _ids(ms.search_memories(QUERIES[0], limit=K))
    for kw in (dict(where=W), DV, dict(expand=E), dict(boost=B), dict(lexical=L)):
        assert _ids(ms.search_memories(QUERIES[0], limit=K, **kw)) != plain, kw


# ---------------------------------------------------------------- no side channel
def test_no_nodes_marked_attribute(ms):
    assert not hasattr(TenantGraph, "_nodes_marked") and not hasattr(ms.graph, "_nodes_marked")
