"""Boosted memory search (``boost=``) on the CPU tier, through MemorySystem
with the hashing embedder: recency deciding between equally near memories, a
far memory that enters only once its prior outweighs the gap, the public
surfaces against the fp64 oracle, composition with ``where=`` / ``diversity=``
/ ``expand=``, validation, the unsupported surfaces, the column cache and the
counters."""
import numpy as np
import pytest
import torch

from lazzaro_amd.core.boost import MemoryBoost
from lazzaro_amd.core.expand import GraphExpand
from lazzaro_amd.core.filters import MemoryFilter
from lazzaro_amd.core.memory_system import MemorySystem
from lazzaro_amd.core.providers import HashEmbedder, LocalLLM
from tests.kernels import _boost_ref as R

D = 32
FILLERS = 20
NOW = 1_700_000_000.0
DAY = 86400.0
QUERY = "what about the deadline?"
QUERIES = [QUERY, "favourite food", "trip to the mountains last week"]


def _system(tmp_path, name="db", **kw):
    return MemorySystem(llm_provider=LocalLLM(), embedding_provider=HashEmbedder(dim=D), enable_async=False,
                        load_from_disk=False, db_dir=str(tmp_path / name), **kw)


def _fill(ms):
    """Around the embedding q of QUERY (unit rows ``a q + sqrt(1 - a^2) u_i``,
    the u_i orthonormal): "old" and "new" at the same cosine 0.8 ("old" takes
    the lower row; last accessed 30 days / 1 hour before NOW), FILLERS
    memories at 0.60, 0.58, ... 0.22, all 10 days old (odd ones preferences),
    and "far" at 0.10, accessed at NOW, salience 1, used 10 times. Every other
    memory has salience 0.5 and was never used. L2 scores are 2 cos - 2, so a
    boost of w trades 2 w against 2 cos."""
    g = ms.graph
    q = np.asarray(ms._get_embedding(QUERY), dtype=np.float64)
    rng = np.random.default_rng(11)
    B = np.linalg.qr(np.concatenate([q[:, None], rng.standard_normal((D, FILLERS + 3))], 1))[0].T
    qd, U = B[0] * np.sign(B[0] @ q), B[1:]
    ids = ["old", "new"] + [f"f{i}" for i in range(FILLERS)] + ["far"]
    cos = [0.8, 0.8] + [0.60 - 0.02 * i for i in range(FILLERS)] + [0.10]
    rows = np.stack([a * qd + np.sqrt(1.0 - a * a) * u for a, u in zip(cos, U)])
    rows[1] = rows[0]  # ("new" IS "old"'s vector: equally near for every query, bit for bit)
    last = [NOW - 30 * DAY, NOW - 3600.0] + [NOW - 10 * DAY] * FILLERS + [NOW]
    g.add_nodes(ids, [f"memory {i}" for i in ids], torch.from_numpy(rows.astype(np.float32)), shard=g.shard_id("work"),
                types=["semantic", "semantic"] + ["preference" if i % 2 else "semantic" for i in range(FILLERS)]
                + ["episodic"], sal=[0.5] * (FILLERS + 2) + [1.0], acc=[0] * (FILLERS + 2) + [10],
                last=last, ts=[NOW - 40 * DAY] * (FILLERS + 3), stored=True)
    sh = g.shard_id("work")
    r = g.row_of
    g.append_edges_host([r["far"]], [r["f19"]], np.array([0.9], np.float32), np.array([sh]), g.etype("relates_to"))
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


def _oracle(ms, queries, k, boost, where_ok=None, metric="l2"):
    """(scores, rows) of the fp64 oracle over the tenant's own columns."""
    g = ms.graph
    n = g.n
    b = MemoryBoost.coerce(boost)
    base = g.store_bias("l2" if metric == "l2" else "ip").cpu().numpy().copy()
    if where_ok is not None:
        base[[i for i in range(n) if not where_ok(g.ids[i])]] = -np.inf
    tw = tcode = None
    if b.type_weights:
        names = sorted(set(g.types))
        tcode = np.asarray([names.index(t) for t in g.types], dtype=np.uint8)
        tw = np.zeros(256)
        for i, t in enumerate(names):
            tw[i] = b.type_weights.get(t, 0.0)
    t = (g.last if b.clock == "accessed" else g.ts)[:n].cpu().numpy()
    col = R.boost_column_ref(base, g.sal[:n].cpu().numpy(), g.acc[:n].cpu().numpy(), t, g.kind[:n].cpu().numpy(), b.now, b.salience,
                             b.frequency, b.recency, b.recency_scale, R.metric_scale(metric), tcode, tw)
    Q = np.stack([_q(ms, q).cpu().numpy() for q in queries])
    return R.boosted_topk_ref(g.emb32[:n].cpu().numpy(), Q, col, metric, k) + (col,)


def _oracle_ids(ms, query, k, boost, where_ok=None):
    g = ms.graph
    return [g.ids[int(r)] for r in _oracle(ms, [query], k, boost, where_ok)[1][0] if r >= 0]


def test_recency_decides_between_equally_near_memories(ms):
    assert ms.graph.row_of["old"] < ms.graph.row_of["new"]
    assert _ids(ms.search_memories(QUERY, limit=3)) == ["old", "new", "f0"]  # a tie: the lower row
    b = {"recency": 0.5, "now": NOW}
    got = _ids(ms.search_memories(QUERY, limit=3, boost=b))
    assert got == ["new", "old", "f0"] == _oracle_ids(ms, QUERY, 3, b)
    # the far memory: cos 0.10 against f2's 0.56 at rank 5 -- a gap of 0.92 in L2 score. Its prior under
    # ``w`` x importance is 2 w (0.5 + 0.3 + 0.2) = 2 w against about 2 w (0.25 + 0 + 0.2 / 11) for f2
    for w, inside in ((0.25, False), (0.5, False), (0.75, True), (1.5, True)):
        b = MemoryBoost(**dict(MemoryBoost.coerce(w).to_dict(), now=NOW))
        got = _ids(ms.search_memories(QUERY, limit=5, boost=b))
        assert ("far" in got) == inside, (w, got)
        assert got == _oracle_ids(ms, QUERY, 5, b)
    assert "far" not in _ids(ms.search_memories(QUERY, limit=FILLERS + 2))  # the farthest of all
    # the scores returned are score + prior, exactly
    g = ms.graph
    b = MemoryBoost(recency=0.5, salience=0.25, now=NOW)
    s, r = g.store_search(_q(ms), 6, "l2", boost=b)
    S, Rr, col = _oracle(ms, [QUERY], 6, b)
    assert np.array_equal(r.cpu().numpy(), Rr)
    tol = (D + 4) * 2.0 ** -24 * 2.0 + 2.0 ** -21  # (the re-rank's fp32 score; test_filter_gpu's form)
    assert np.abs(s.cpu().numpy() - S).max() <= tol
    assert np.array_equal(g.boost_bias(b, "l2").cpu().numpy().view(np.uint32), col.view(np.uint32))
    plain = g.store_search(_q(ms), g.n, "l2")
    pos = {int(x): i for i, x in enumerate(plain[1][0].tolist())}
    prior = R.boost_prior_ref(g.sal[: g.n].cpu().numpy(), g.acc[: g.n].cpu().numpy(), g.last[: g.n].cpu().numpy(), NOW, 0.25, 0.0, 0.5,
                              DAY, 2.0)
    for sc, row in zip(s[0].tolist(), r[0].tolist()):
        assert sc == pytest.approx(plain[0][0, pos[row]].item() + float(prior[row]), abs=1e-6)


@pytest.mark.parametrize("boost", [0.8, {"recency": 0.6, "salience": 0.2, "clock": "created"},
                                   MemoryBoost(frequency=0.5, recency=0.3, recency_scale=3600.0,
                                               type_weights={"episodic": 0.4, "never-seen": 1.0})])
def test_surfaces_agree_with_the_oracle(ms, boost):
    b = MemoryBoost.coerce(boost).at(NOW)
    forms = [b, b.to_dict()] + ([dict(boost, now=NOW)] if isinstance(boost, dict) else [])
    want = [_oracle_ids(ms, q, 4, b) for q in QUERIES]
    assert all(len(w) == 4 for w in want)
    emb = ms._get_embedding(QUERY)
    st = ms.vector_store
    for f in forms:
        kw = dict(limit=4, boost=f)
        assert [_ids(ms.search_memories(q, **kw)) for q in QUERIES] == want
        assert [_ids(r) for r in ms.search_memories_batch(QUERIES, **kw)] == want
        batches = [QUERIES[:2], QUERIES[2:], QUERIES]
        assert [[_ids(r) for r in x] for x in ms.search_memories_stream(batches, **kw)] == [want[:2], want[2:], want]
        assert st.search_nodes(emb, user_id=ms.user_id, limit=4, boost=f) == want[0]
        assert st.search_nodes_batch([emb], user_id=ms.user_id, limit=4, boost=f) == [want[0]]
        assert ms.graph.search_ids(_q(ms), 4, ms.store.metric, boost=f) == [want[0]]
        _, r = ms.graph.store_search(_q(ms), 4, ms.store.metric, boost=f)
        assert [ms.graph.ids[i] for i in r[0].tolist()] == want[0]
    for metric in ("ip", "cosine"):
        s, r = ms.graph.store_search(_q(ms), 4, metric, boost=b)
        S, Rr, _ = _oracle(ms, [QUERY], 4, b, metric=metric)
        assert np.array_equal(r.cpu().numpy(), Rr) and np.abs(s.cpu().numpy() - S).max() <= 1e-5


def test_the_float_form_and_the_clock(ms, monkeypatch):
    import lazzaro_amd.core.boost as CB
    calls = []  # ``now=None`` reads the clock -- once per call
    monkeypatch.setattr(CB, "_clock", lambda: calls.append(1) or NOW)
    want = _oracle_ids(ms, QUERY, 5, MemoryBoost(salience=0.5, frequency=0.3, recency=0.2, now=NOW))
    assert _ids(ms.search_memories(QUERY, limit=5, boost=1.0)) == want and len(calls) == 1
    assert [_ids(r) for r in ms.search_memories_batch([QUERY, QUERY], limit=5, boost=1.0)] == [want, want]
    assert len(calls) == 2
    out = list(ms.search_memories_stream([[QUERY], [QUERY], [QUERY]], limit=5, boost=1))
    assert [_ids(r[0]) for r in out] == [want] * 3 and len(calls) == 3  # one reading for the whole stream
    assert ms.graph.boost_columns_built == 1  # (the clock stood still: one column served them all)


def test_none_is_the_plain_search_and_zero_is_the_empty_filter(ms):
    g = ms.graph
    g.add_nodes(["ghost"], ["store-only"], _q(ms)[None, :], shard=g.shard_id("work", live=False), stored=True,
                ghost=True)  # the nearest row of all, and not a memory
    for q in QUERIES:
        want = _ids(ms.search_memories(q, limit=6))
        assert _ids(ms.search_memories(q, limit=6, boost=None)) == want
        assert [_ids(r) for r in ms.search_memories_batch([q], limit=6, boost=None)] == [want]
    a = g.store_search(_q(ms), 6, "l2")
    b = g.store_search(_q(ms), 6, "l2", boost=None)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[1][0, 0].item() == g.row_of["ghost"]
    assert ms.get_stats()["engine"]["boosted_searches"] == 0
    for zero in (0.0, {}, MemoryBoost(), {"type_weights": {"semantic": 0.0}}):
        for metric in ("l2", "ip", "cosine"):
            z = g.store_search(_q(ms), 6, metric, boost=zero)
            w = g.store_search(_q(ms), 6, metric, where=MemoryFilter())
            assert torch.equal(z[0], w[0]) and torch.equal(z[1], w[1])
            assert g.row_of["ghost"] not in z[1][0].tolist()  # memories only, node_rows or not
    base = g.store_bias("l2")
    col = g.boost_bias(0.0, "l2")
    node = g.kind[: g.n] == 1
    assert torch.equal(col[node], base[node]) and torch.isneginf(col[~node]).all()


def test_composes_with_where_diversity_and_expand(ms):
    from lazzaro_amd.ops.expand_ops import expand_select
    from lazzaro_amd.ops.mmr_ops import mmr_select
    from tests.kernels._expand_ref import expand64
    from tests.kernels._mmr_ref import check_rule1
    g = ms.graph
    b = MemoryBoost(recency=1.0, salience=0.5, now=NOW)
    flt = {"types": ["semantic"]}
    sem = lambda i: not (i[0] == "f" and i[1:].isdigit() and int(i[1:]) % 2) and i != "far"  # noqa: E731
    got = ms.search_memories(QUERY, limit=5, where=flt, boost=b)
    assert _ids(got) == _oracle_ids(ms, QUERY, 5, b, sem) and all(n.type == "semantic" for n in got)
    assert _ids(got)[:2] == ["new", "old"]
    col = _oracle(ms, [QUERY], 1, b, sem)[2]
    assert np.array_equal(g.boost_bias(b, "l2", where=flt).cpu().numpy().view(np.uint32), col.view(np.uint32))
    # diversity: the pool is the boosted search at fetch_k, the picks MMR's over it by cosine
    n = g.n
    q = _q(ms)
    PS, PR, _ = _oracle(ms, [QUERY], 16, b)
    ps, pr = g.store_search(q, 16, "l2", node_rows=True, boost=b)
    assert np.array_equal(pr.cpu().numpy(), PR) and g.row_of["far"] in PR[0].tolist()
    pick, obj = mmr_select(g.emb32[:n], q[None, :].to(g.device), pr, 4, 0.3)
    check_rule1(g.emb32[:n].cpu().numpy(), q[None, :].cpu().numpy(), PR, 4, 0.3, pick.cpu().numpy(), obj.cpu().numpy())
    s, r = g.store_search(q, 4, "l2", diversity=0.3, fetch_k=16, boost=b)
    assert torch.equal(r, torch.gather(pr, 1, pick.long())) and torch.equal(s, torch.gather(ps, 1, pick.long()))
    assert _ids(ms.search_memories(QUERY, limit=4, diversity=0.3, fetch_k=16, boost=b)) == \
        [g.ids[i] for i in r[0].tolist()]
    # expand: the seeds are the boosted search at seed_k; the blend stays cosine. "far" is a seed only
    # when boosted, and only then is its link to f19 walked
    sp = {"seed_k": 4, "graph_weight": 1.0, "min_weight": 0.5}
    _, SR, _ = _oracle(ms, [QUERY], 4, b)
    assert g.row_of["far"] in SR[0].tolist() and "far" not in _ids(ms.search_memories(QUERY, limit=4))
    ref = expand64(g.emb32[:n].cpu().numpy(), q[None, :].cpu().numpy(), SR, tuple(t.cpu().numpy() for t in g.csr()), g.e["w"].cpu().numpy(),
                   g.kind[:n].cpu().numpy(), g.sup[:n].cpu().numpy(), g.store_bias("l2").cpu().numpy(), sp)[0]
    want = [g.ids[int(x)] for x in ref.rows[ref.order[:5]]]
    s, r, via = g.store_search_expand(q, 5, "l2", expand=sp, boost=b)
    assert [g.ids[i] for i in r[0].tolist() if i >= 0] == want and "f19" in want
    assert via[0, want.index("f19")].item() == g.row_of["far"]
    rows, scores, _, _ = expand_select(g.emb32[:n], q[None, :].to(g.device), torch.from_numpy(SR).to(g.device), g.csr(),
                                       g.e["w"], g.kind, g.sup,
                                       g.store_bias("l2"), GraphExpand(**sp), 5)
    assert torch.equal(rows, r) and torch.equal(scores, s)  # (cosine blend: no prior in the scores)
    assert _ids(ms.search_memories(QUERY, limit=5, expand=sp, boost=b)) == want
    assert "f19" not in [g.ids[i] for i in g.store_search_expand(q, 5, "l2", expand=sp)[1][0].tolist() if i >= 0]


def test_validation(ms):
    emb = ms._get_embedding(QUERY)
    bad = [-1.0, float("nan"), 8.5, {"salience": -0.1}, {"recency": float("inf")}, {"recency_scale": 0.0},
           {"clock": "modified"}, {"type_weights": {"a": -1.0}}, {"now": float("nan")}, {"no_such_field": 1},
           {"salience": 2.0, "frequency": 1.5, "recency": 1.0}, {"salience": 2.0, "recency": 1.5,
                                                                  "type_weights": {"a": 0.75}}]
    for b in bad:
        kw = dict(limit=5, boost=b)
        with pytest.raises(ValueError):
            ms.search_memories(QUERY, **kw)
        with pytest.raises(ValueError):
            ms.search_memories_batch([QUERY], **kw)
        with pytest.raises(ValueError):
            list(ms.search_memories_stream([[QUERY]], **kw))
        with pytest.raises(ValueError):
            ms.vector_store.search_nodes(emb, user_id=ms.user_id, **kw)
        with pytest.raises(ValueError):
            ms.graph.store_search(_q(ms), 5, "l2", boost=b)
        with pytest.raises(ValueError):
            ms.graph.boost_bias(b, "l2")
    with pytest.raises(TypeError):
        ms.search_memories(QUERY, boost="much")
    assert ms.get_stats()["engine"]["boosted_searches"] == 0
    assert len(ms.search_memories(QUERY, limit=5, boost={"salience": 2.0, "frequency": 1.0, "recency": 1.0})) == 5


def test_out_of_scope_surfaces_raise(ms, tmp_path):
    from lazzaro_amd.core.vector_store import HBMStore
    from lazzaro_amd.parallel.service import DistributedMemoryService
    from lazzaro_amd.parallel.sharded_memory import ShardedMemorySystem
    emb = ms._get_embedding("q")
    for kw in (dict(boost=1.0), dict(boost={"recency": 0.5}), dict(boost=MemoryBoost(salience=1.0))):
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
    st = HBMStore(db_dir=str(tmp_path / "plain"), device="cpu")
    st.add_nodes([{"id": "a", "content": "c", "vector": [1.0] + [0.0] * (D - 1)}], user_id="u")
    assert st.search_nodes([1.0] + [0.0] * (D - 1), user_id="u") == ["a"]
    with pytest.raises(NotImplementedError):
        st.search_nodes([1.0] + [0.0] * (D - 1), user_id="u", boost=1.0)
    with pytest.raises(NotImplementedError):
        st.search_nodes_batch([[1.0] + [0.0] * (D - 1)], user_id="u", boost=1.0)
    st.close()


def test_dashboard_search_parameters(ms):
    from fastapi.testclient import TestClient

    from lazzaro_amd.dashboard import api
    api.set_memory_system(ms)
    try:
        c = TestClient(api.app)
        plain = [h["id"] for h in c.get("/api/search", params={"q": QUERY, "limit": 3}).json()]
        assert plain == ["old", "new", "f0"]
        # the clock is the wall clock here: years after NOW, every recency is ~0 and salience and use decide
        # (salience 1 and ten uses against 0.5 and none: 2 x (0.5 x 0.5 + 0.3) = 1.1 of L2 score, more than the
        # 1.0 "far" lies behind f0 and less than the 1.4 behind "old")
        got = [h["id"] for h in c.get("/api/search", params={"q": QUERY, "limit": 5, "boost": 1.0}).json()]
        # ("new" before "old": what is left of recency, ~1e-5, still breaks their tie)
        assert got == ["new", "old", "far", "f0", "f1"]
        assert ms.graph.boosted_searches == 1
        # a scale of 1,000 years makes every memory recent alike, "new" a little more so
        got = [h["id"] for h in c.get("/api/search", params={"q": QUERY, "limit": 2, "boost": 4.0,
                                                             "boost_recency_scale": 3.2e10}).json()]
        assert got[:1] == ["far"]
        both = [h["id"] for h in c.get("/api/search", params={"q": QUERY, "limit": 3, "boost": 1.5,
                                                              "types": "semantic"}).json()]
        assert both == ["new", "old", "f0"]
        assert c.get("/api/search", params={"q": QUERY, "boost_recency_scale": 5.0}).json()[0]["id"] == "old"
        assert ms.graph.boosted_searches == 3
    finally:
        api.set_memory_system(None)


def test_counters_and_the_column_cache(ms):
    g = ms.graph
    e = ms.get_stats()["engine"]
    assert e["boosted_searches"] == 0 and e["boost_columns_built"] == 0
    ms.search_memories(QUERY)  # plain: counts nothing
    ms.search_memories(QUERY, diversity=0.3)
    assert ms.get_stats()["engine"]["boosted_searches"] == 0
    b = {"recency": 0.5, "now": NOW}
    ms.search_memories(QUERY, boost=b)
    ms.search_memories_batch(QUERIES, limit=3, boost=b)  # one store search per batch
    e = ms.get_stats()["engine"]
    assert e["boosted_searches"] == 2 and e["boost_columns_built"] == 1  # the same ``now``: one column
    list(ms.search_memories_stream([QUERIES, QUERIES[:1]], limit=3, boost=b, where={"types": ["semantic"]}))
    ms.search_memories(QUERY, limit=3, boost=b, diversity=0.3)
    ms.search_memories(QUERY, limit=3, boost=b, expand=1)
    e = ms.get_stats()["engine"]
    assert e["boosted_searches"] == 6 and e["filtered_searches"] == 2 and e["mmr_searches"] == 2
    assert e["expanded_searches"] == 1 and e["boost_columns_built"] == 2  # + the filtered one
    ms.search_memories(QUERY, boost=dict(b, now=NOW + 1.0))  # a fresh ``now``: a fresh column
    ms.search_memories(QUERY, boost=b, limit=3)  # ("l2" unfiltered is still one of the two kept)
    assert g.boost_columns_built == 3 and len(g._boost_cols) == 2
    # a retrieval touch in between rebuilds the column, and the touched row's recency shows
    built = g.boost_columns_built
    assert _ids(ms.search_memories(QUERY, limit=2, boost=b)) == ["new", "old"] and g.boost_columns_built == built
    g.touch([g.row_of["old"]], now=NOW)
    assert _ids(ms.search_memories(QUERY, limit=2, boost=b)) == ["old", "new"] == _oracle_ids(ms, QUERY, 2, b)
    assert g.boost_columns_built == built + 1
    # ... as does a scalar write through a node view (no version bump: _meta_gen)
    g.set_scalar(g.row_of["new"], "last", NOW + 5.0)
    b2 = dict(b, now=NOW + 5.0)
    assert _ids(ms.search_memories(QUERY, limit=2, boost=b2)) == ["new", "old"] == _oracle_ids(ms, QUERY, 2, b2)


def test_column_follows_eviction_and_compaction(ms):
    g = ms.graph
    b = {"recency": 0.5, "now": NOW}
    assert _ids(ms.search_memories(QUERY, limit=3, boost=b)) == ["new", "old", "f0"]
    g.remove_nodes([g.row_of["new"], g.row_of["f0"]], drop_edges=True, unstore=True)
    got = _ids(ms.search_memories(QUERY, limit=3, boost=b))
    assert got == ["old", "f1", "f2"] == _oracle_ids(ms, QUERY, 3, b)  # ghosts take no slot
    g.take_dirty_rows(), g.take_dirty_edges(), g.take_deleted()  # (as after a commit: nothing pins the two rows)
    n0, epoch = g.n, g.row_epoch
    g.compact()
    assert g.n == n0 - 2 and g.row_epoch == epoch + 1 and g._boost_cols is None
    assert _ids(ms.search_memories(QUERY, limit=3, boost=b)) == ["old", "f1", "f2"] == _oracle_ids(ms, QUERY, 3, b)
    assert g.boost_bias(b, "l2").numel() == g.n
