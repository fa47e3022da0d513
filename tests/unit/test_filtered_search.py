"""Filtered memory search (``where=``) on the CPU tier: every MemoryFilter
field against a list comprehension over Node views, through MemorySystem with
the hashing embedder; the public surfaces, counters and limits."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lazzaro_amd.core.filters import MAX_EXCLUDE_IDS, MemoryFilter
from lazzaro_amd.core.memory_system import MemorySystem
from lazzaro_amd.core.providers import HashEmbedder, LocalLLM

D = 32
N = 240
TYPES = ("semantic", "preference", "episodic")
SHARDS = ("work", "home", "travel")
T0 = 1_700_000_000.0
QUERIES = ["what did the user say about work", "favourite food", "trip to the mountains last week"]


def _system(tmp_path, name="db", **kw):
    return MemorySystem(llm_provider=LocalLLM(), embedding_provider=HashEmbedder(dim=D), enable_async=False,
                        load_from_disk=False, db_dir=str(tmp_path / name), **kw)


def _fill(ms, n=N, seed=0):
    """n nodes with varied metadata, then rows a filtered search must never
    return: ghosts (store-only rows) and nodes that are not in the store."""
    g = ms.graph
    rng = np.random.default_rng(seed)
    X = F.normalize(torch.from_numpy(rng.standard_normal((n + 16, D)).astype(np.float32)), dim=1)
    ids = [f"m{i}" for i in range(n)]
    g.add_nodes(ids, [f"memory {i}" for i in range(n)], X[:n],
                shard=[g.shard_id(SHARDS[i % 3]) for i in range(n)], types=[TYPES[(i // 2) % 3] for i in range(n)],
                sal=[float(np.float32(0.05 + 0.9 * rng.random())) for _ in range(n)],
                acc=[int(rng.integers(0, 9)) for _ in range(n)],
                last=[T0 + 50.0 * i for i in range(n)], ts=[T0 + 100.0 * (i % 60) for i in range(n)],
                sup=[1 if i % 17 == 0 else 0 for i in range(n)], stored=True)
    g.add_nodes([f"ghost{i}" for i in range(8)], ["ghost"] * 8, X[n:n + 8], shard=g.shard_id("work", live=False),
                stored=True, ghost=True)
    g.add_nodes([f"loose{i}" for i in range(8)], ["not in the store"] * 8, X[n + 8:], shard=g.shard_id("work"),
                stored=False)
    return ids


@pytest.fixture()
def ms(tmp_path):
    m = _system(tmp_path)
    _fill(m)
    yield m
    m.close()


def _memories(ms):
    """Node views of every memory: a graph node that is in the store."""
    g = ms.graph
    stored = g.stored[: g.n].cpu().numpy()
    nodes = [ms.buffer.get_node(i) for i in g.ids]
    return [nd for r, nd in enumerate(nodes) if nd is not None and stored[r] == 1]


def _ids(hits):
    return [n.id for n in hits]


def _expect(ms, query, pred, limit):
    """The unfiltered ranking of the whole tenant, restricted to the
    memories that pass ``pred``: what a filtered search must return."""
    ok = {n.id for n in _memories(ms) if pred(n)}
    ranked = _ids(ms.search_memories(query, limit=ms.graph.n))
    return [i for i in ranked if i in ok][:limit], ok


F32 = np.float32
CASES = [
    ("types", dict(types=["preference"]), lambda n: n.type == "preference"),
    ("types2", dict(types=["preference", "episodic", "never-seen"]), lambda n: n.type in ("preference", "episodic")),
    ("shard", dict(shard_keys=["work"]), lambda n: n.shard_key == "work"),
    ("shard_unknown", dict(shard_keys=["no-such-topic"]), lambda n: False),
    ("min_sal", dict(min_salience=0.6), lambda n: F32(n.salience) >= F32(0.6)),
    ("max_sal", dict(max_salience=0.3), lambda n: F32(n.salience) <= F32(0.3)),
    ("sal_band", dict(min_salience=0.25, max_salience=0.75), lambda n: F32(0.25) <= F32(n.salience) <= F32(0.75)),
    ("since", dict(since=T0 + 3000.0), lambda n: n.timestamp >= T0 + 3000.0),
    ("until", dict(until=T0 + 1000.0), lambda n: n.timestamp < T0 + 1000.0),
    ("window", dict(since=T0 + 1000.0, until=T0 + 1100.0), lambda n: T0 + 1000.0 <= n.timestamp < T0 + 1100.0),
    ("empty_window", dict(since=T0 + 1000.0, until=T0 + 1000.0), lambda n: False),
    ("accessed", dict(accessed_since=T0 + 50.0 * 200), lambda n: n.last_accessed >= T0 + 50.0 * 200),
    ("acc", dict(min_access_count=5), lambda n: n.access_count >= 5),
    ("super_only", dict(super_nodes=True), lambda n: n.is_super_node),
    ("super_none", dict(super_nodes=False), lambda n: not n.is_super_node),
    ("exclude", dict(exclude_ids=["m3", "m4", "m5", "not-an-id", "ghost1"]), lambda n: n.id not in ("m3", "m4", "m5")),
    ("empty", dict(), lambda n: True),
    ("all", dict(types=["semantic", "episodic"], shard_keys=["work", "home"], min_salience=0.2, max_salience=0.9,
                 since=T0 + 500.0, until=T0 + 5500.0, accessed_since=T0 + 1000.0, min_access_count=1,
                 super_nodes=False, exclude_ids=["m30", "m31"]),
     lambda n: (n.type in ("semantic", "episodic") and n.shard_key in ("work", "home")
                and F32(0.2) <= F32(n.salience) <= F32(0.9) and T0 + 500.0 <= n.timestamp < T0 + 5500.0
                and n.last_accessed >= T0 + 1000.0 and n.access_count >= 1 and not n.is_super_node
                and n.id not in ("m30", "m31"))),
]


@pytest.mark.parametrize("name,fields,pred", CASES, ids=[c[0] for c in CASES])
def test_field_semantics(ms, name, fields, pred):
    flt = MemoryFilter(**fields)
    for q in QUERIES[:2]:
        want5, ok = _expect(ms, q, pred, 5)
        assert _ids(ms.search_memories(q, limit=5, where=flt)) == want5
        # a limit above the passing count returns every passing memory, once, and nothing else
        everything = _ids(ms.search_memories(q, limit=ms.graph.n, where=flt))
        assert sorted(everything) == sorted(ok) and len(set(everything)) == len(everything)
    if name not in ("shard_unknown", "empty_window"):
        assert ok, "the case must select something"


def test_ghosts_and_unstored_rows_take_no_slot(ms):
    got = _ids(ms.search_memories(QUERIES[0], limit=ms.graph.n, where=MemoryFilter()))
    assert len(got) == N and not any(i.startswith(("ghost", "loose")) for i in got)


def test_limit_above_passing_count(ms):
    flt = MemoryFilter(types=["preference"], shard_keys=["travel"], min_salience=0.5)
    want, ok = _expect(ms, QUERIES[1], lambda n: n.type == "preference" and n.shard_key == "travel"
                       and F32(n.salience) >= F32(0.5), 1000)
    assert 0 < len(ok) < 40
    assert _ids(ms.search_memories(QUERIES[1], limit=len(ok) + 7, where=flt)) == want


def test_type_rewritten_by_readding_an_id(ms):
    g = ms.graph
    flt = MemoryFilter(types=["procedural"])
    assert ms.search_memories(QUERIES[0], limit=5, where=flt) == []  # builds the type-code column
    r = g.row_of["m10"]
    g.add_nodes(["m10", "fresh"], ["rewritten", "appended"], g.emb32[[r, r + 1]].clone(),
                shard=g.shard_id("work"), types=["procedural", "procedural"], stored=True)
    assert sorted(_ids(ms.search_memories(QUERIES[0], limit=5, where=flt))) == ["fresh", "m10"]
    # ... and through a node view
    ms.buffer.get_node("m11").type = "procedural"
    assert sorted(_ids(ms.search_memories(QUERIES[0], limit=5, where=flt))) == ["fresh", "m10", "m11"]
    old = TYPES[(10 // 2) % 3]
    assert "m10" not in _ids(ms.search_memories(QUERIES[0], limit=g.n, where={"types": [old]}))


def test_scalar_write_through_a_view_invalidates_the_plan(ms):
    flt = MemoryFilter(min_salience=0.99)
    assert ms.search_memories(QUERIES[0], limit=5, where=flt) == []
    ms.buffer.get_node("m7").salience = 1.0
    assert _ids(ms.search_memories(QUERIES[0], limit=5, where=flt)) == ["m7"]


def test_too_many_types_raises(tmp_path):
    m = _system(tmp_path, "many")
    g = m.graph
    n = 256
    X = F.normalize(torch.randn(n, D, generator=torch.Generator().manual_seed(1)), dim=1)
    g.add_nodes([f"t{i}" for i in range(n)], ["c"] * n, X, shard=g.shard_id("s"), types=[f"type{i}" for i in range(n)],
                stored=True)
    with pytest.raises(OverflowError):
        m.search_memories("q", where={"types": ["type3"]})
    assert len(m.search_memories("q", limit=n, where={"min_salience": 0.0})) == n  # other fields still work
    m.close()


def test_exclude_ids_limit():
    MemoryFilter(exclude_ids=[f"x{i}" for i in range(MAX_EXCLUDE_IDS)])
    with pytest.raises(ValueError):
        MemoryFilter(exclude_ids=[f"x{i}" for i in range(MAX_EXCLUDE_IDS + 1)])
    with pytest.raises(ValueError):
        MemoryFilter.from_dict({"exclude_ids": [f"x{i}" for i in range(MAX_EXCLUDE_IDS + 1)]})


def test_filter_round_trip_and_key():
    f = MemoryFilter(types=["b", "a"], shard_keys="work", min_salience=0.5, until=9, min_access_count=2,
                     super_nodes=False, exclude_ids={"z", "y"})
    d = f.to_dict()
    assert d == {"types": ["a", "b"], "shard_keys": ["work"], "min_salience": 0.5, "until": 9.0,
                 "min_access_count": 2, "super_nodes": False, "exclude_ids": ["y", "z"]}
    g = MemoryFilter.from_dict(d)
    assert g == f and g.key() == f.key() and hash(g) == hash(f) and len({f.key(): 1, g.key(): 2}) == 1
    assert MemoryFilter(types=["a"]).key() != MemoryFilter(shard_keys=["a"]).key()
    assert MemoryFilter.from_dict({}) == MemoryFilter() and MemoryFilter().to_dict() == {}
    with pytest.raises(ValueError):
        MemoryFilter.from_dict({"typos": ["a"]})
    with pytest.raises(TypeError):
        MemoryFilter.coerce(["types"])
    with pytest.raises(Exception):
        f.types = None  # frozen


def test_dict_accepted_everywhere(ms):
    d = {"types": ["episodic"], "min_salience": 0.4}
    flt = MemoryFilter.from_dict(d)
    q = QUERIES[2]
    want = _ids(ms.search_memories(q, limit=6, where=flt))
    assert want and _ids(ms.search_memories(q, limit=6, where=d)) == want
    assert [_ids(r) for r in ms.search_memories_batch([q], limit=6, where=d)] == [want]
    emb = ms._get_embedding(q)
    assert ms.vector_store.search_nodes(emb, user_id=ms.user_id, limit=6, where=d) == want
    assert ms.vector_store.search_nodes_batch([emb], user_id=ms.user_id, limit=6, where=d) == [want]
    _, rows = ms.graph.store_search(torch.as_tensor(emb, dtype=torch.float32), 6, ms.store.metric, where=d)
    assert [ms.graph.ids[r] for r in rows[0].tolist() if r >= 0] == want


def test_batch_and_stream_equal_single_calls(ms):
    flt = MemoryFilter(shard_keys=["home", "travel"], super_nodes=False)
    single = [_ids(ms.search_memories(q, limit=4, where=flt)) for q in QUERIES]
    assert [_ids(r) for r in ms.search_memories_batch(QUERIES, limit=4, where=flt)] == single
    batches = [QUERIES[:2], QUERIES[2:], QUERIES]
    streamed = [[_ids(r) for r in b] for b in ms.search_memories_stream(batches, limit=4, where=flt)]
    assert streamed == [[_ids(r) for r in ms.search_memories_batch(b, limit=4, where=flt)] for b in batches]
    assert streamed == [single[:2], single[2:], single]


def test_counters_and_plan_cache(ms):
    e0 = ms.get_stats()["engine"]
    assert (e0["filtered_searches"], e0["filter_plans_built"], e0["filtered_sparse"]) == (0, 0, 0)
    ms.search_memories(QUERIES[0])  # unfiltered: counts nothing
    flt = MemoryFilter(types=["semantic"])
    for _ in range(3):
        ms.search_memories_batch(QUERIES, limit=3, where=flt)
    e = ms.get_stats()["engine"]
    assert e["filtered_searches"] == 3 and e["filter_plans_built"] == 1  # the plan is cached
    assert e["filtered_sparse"] == 0  # (the indexed scan is the GPU's route)
    ms.search_memories_batch(QUERIES, limit=3, where={"types": ["episodic"]})
    g = ms.graph
    g.touch([0, 1])  # a retrieval touch writes acc / last: the plans built before it are not served again
    ms.search_memories_batch(QUERIES, limit=3, where=flt)
    e = ms.get_stats()["engine"]
    assert e["filtered_searches"] == 5 and e["filter_plans_built"] == 3
    assert len(g._filter_plans) == 1


def test_plan_follows_eviction_and_compaction(ms):
    g = ms.graph
    flt = MemoryFilter(shard_keys=["work"])
    q = QUERIES[0]
    before = _ids(ms.search_memories(q, limit=g.n, where=flt))
    gone = before[:5]
    g.remove_nodes([g.row_of[i] for i in gone], unstore=True)
    after = _ids(ms.search_memories(q, limit=g.n, where=flt))
    assert after == [i for i in before if i not in gone]
    g.take_dirty_rows()  # (as a commit does: dirty rows are not reclaimed)
    out = ms.compact_memory()
    assert out["reclaimed"] >= 5 and g.row_epoch == 1
    assert _ids(ms.search_memories(q, limit=g.n, where=flt)) == after
    assert _ids(ms.search_memories(q, limit=g.n, where={"types": ["preference"]})) == [
        i for i in _ids(ms.search_memories(q, limit=g.n)) if ms.buffer.get_node(i).type == "preference"]


def test_out_of_scope_surfaces_raise(ms, tmp_path):
    from lazzaro_amd.core.vector_store import HBMStore
    from lazzaro_amd.parallel.service import DistributedMemoryService
    from lazzaro_amd.parallel.sharded_memory import ShardedMemorySystem
    w = {"types": ["semantic"]}
    emb = ms._get_embedding("q")
    with pytest.raises(NotImplementedError):
        ms.vector_store.search_nodes_multi([emb], [ms.user_id], where=w)
    # the checks come first: no distributed set-up is needed to reach them
    with pytest.raises(NotImplementedError):
        ShardedMemorySystem.search_memories_batch(None, ["q"], where=w)
    with pytest.raises(NotImplementedError):
        DistributedMemoryService.search_routed(None, ["u"], ["q"], where=w)
    with pytest.raises(NotImplementedError):
        DistributedMemoryService.search_global_batch(None, ["q"], where=w)
    with pytest.raises(NotImplementedError):
        DistributedMemoryService.search_global(None, torch.zeros(D), where=w)
    # a tenant of a store that has no graph attached cannot evaluate a predicate
    st = HBMStore(db_dir=str(tmp_path / "plain"), device="cpu")
    st.add_nodes([{"id": "a", "content": "c", "vector": [1.0] + [0.0] * (D - 1)}], user_id="u")
    assert st.search_nodes([1.0] + [0.0] * (D - 1), user_id="u") == ["a"]
    with pytest.raises(NotImplementedError):
        st.search_nodes([1.0] + [0.0] * (D - 1), user_id="u", where=w)
    with pytest.raises(NotImplementedError):
        st.search_nodes_batch([[1.0] + [0.0] * (D - 1)], user_id="u", where=w)
    st.close()


def test_dashboard_search_parameters(ms):
    from fastapi.testclient import TestClient

    from lazzaro_amd.dashboard import api
    api.set_memory_system(ms)
    try:
        c = TestClient(api.app)
        q = QUERIES[0]
        plain = [h["id"] for h in c.get("/api/search", params={"q": q, "limit": 5}).json()]
        assert plain == _ids(ms.search_memories(q, limit=5))
        got = c.get("/api/search", params={"q": q, "limit": 5, "types": "preference,episodic", "shard_keys": "work",
                                           "min_salience": 0.3, "max_salience": 0.95, "since": T0, "until": T0 + 5000,
                                           "accessed_since": T0, "min_access_count": 1, "super_nodes": "false",
                                           "exclude_ids": "m1,m2"}).json()
        want = ms.search_memories(q, limit=5, where=MemoryFilter(
            types=["preference", "episodic"], shard_keys=["work"], min_salience=0.3, max_salience=0.95, since=T0,
            until=T0 + 5000, accessed_since=T0, min_access_count=1, super_nodes=False, exclude_ids=["m1", "m2"]))
        assert want and [h["id"] for h in got] == _ids(want)
        assert all(h["shard"] == "work" for h in got)
        assert c.get("/api/search", params={"q": q, "shard_keys": "no-such-topic"}).json() == []
    finally:
        api.set_memory_system(None)
