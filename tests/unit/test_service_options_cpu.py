"""Options in the served batch, CPU tier: the request form of
``DistributedMemoryService.serve`` (a ``search_memories`` request with a dict
of options), its validation and JSON normal form, the torch formulation of the
round's bias columns against the numpy oracle, and the surfaces that keep
refusing options."""
import json

import numpy as np
import pytest
import torch

from lazzaro_amd.core.boost import MemoryBoost
from lazzaro_amd.core.filters import MemoryFilter
from lazzaro_amd.core.search_spec import SearchSpec
from lazzaro_amd.core.vector_store import HBMStore
from lazzaro_amd.parallel import Communicator
from lazzaro_amd.parallel.service import DistributedMemoryService, node_dict

D = 32
NOW = 1_700_000_000.0
TYPES = ("preference", "fact", "event")


def _service(tmp_path, users=("a", "b", "c")):
    from lazzaro_amd.core.memory_system import MemorySystem
    from lazzaro_amd.core.providers import HashEmbedder, LocalLLM
    emb = HashEmbedder(dim=D)

    def factory(user, load_from_disk=True):
        return MemorySystem(llm_provider=LocalLLM(), embedding_provider=emb, enable_async=False,
                            db_dir=str(tmp_path), user_id=user, device="cpu", load_from_disk=load_from_disk,
                            max_buffer_size=10 ** 6)
    svc = DistributedMemoryService(Communicator.local(), factory)
    rng = np.random.default_rng(4)
    for j, u in enumerate(users):
        g = svc.system(u).graph
        n = 40 + 7 * j
        texts = [f"{u} likes topic {i} of project {i % 5}" for i in range(n)]
        g.add_nodes([f"{u}_{i}" for i in range(n)], texts, torch.tensor(emb.batch_embed(texts)),
                    shard=g.shard_id("work"), types=[TYPES[i % 3] for i in range(n)],
                    sal=rng.random(n).astype(np.float32).tolist(), acc=rng.integers(0, 20, n).tolist(),
                    last=(NOW - rng.random(n) * 1e6).tolist(), stored=True, now=NOW)
    return svc


def test_serve_applies_the_options_of_a_request(tmp_path):
    """The test that fails without the feature: the options dict of a served
    ``search_memories`` request used to be dropped, silently."""
    svc = _service(tmp_path)
    q = "topic 3 of project 3"
    where = {"types": ["preference"]}
    got = svc.serve([("a", "search_memories", q, 3, {"where": where})])[0]
    want = svc.system("a").search_memories(q, 3, where=where)
    assert len(got) == 3 and all(n["type"] == "preference" for n in got)
    assert [n["id"] for n in got] == [n.id for n in want]
    plain = svc.serve([("a", "search_memories", q, 3)])[0]
    assert [n["id"] for n in plain] != [n["id"] for n in got]  # (the filter does change this query's answer)
    svc.close()


def test_every_option_is_served_per_tenant_on_the_cpu(tmp_path):
    svc = _service(tmp_path)
    boost = {"salience": 1.0, "recency": 0.5, "now": NOW}
    reqs = [("a", "search_memories", "topic 1", 4),
            ("b", "search_memories", "topic 2", 4, {"where": {"min_salience": 0.5}, "boost": boost}),
            ("c", "search_memories", "topic 3", 3, {"diversity": 0.5}),
            ("a", "search_memories", "project 4", 5, {"boost": boost}),
            ("b", "search_memories", "project 1", 2, {"expand": 1, "where": {"types": ["fact", "event"]}}),
            ("c", "search_memories", "topic 9", 2, None),
            ("c", "search_memories", "likes topic 7", 2, {"lexical": 0.5})]
    got = svc.serve(reqs)
    for req, r in zip(reqs, got):
        opts = (req[4] if len(req) > 4 else None) or {}
        want = svc.system(req[0]).search_memories_batch([req[2]], req[3], **opts)[0]
        assert list(r) == [node_dict(n) for n in want], req
    st = svc.stats()
    assert st["mt_option_requests"] == 5 and st["mt_option_fallbacks"] == 5 and st["mt_bias_jobs"] == 0
    assert list(svc.serve_stream([reqs, reqs[:3]])) == [got, got[:3]]
    svc.close()


@pytest.mark.parametrize("options", [{"wher": {}}, {"where": {"typ": ["x"]}}, {"boost": -1.0}, {"boost": "high"},
                                     {"diversity": 2.0}, {"where": 5}, ["where"], {"boost": {"clock": "never"}}])
def test_bad_options_raise_on_the_sender_before_any_exchange(tmp_path, options):
    svc = _service(tmp_path, users=("a",))

    def no_exchange(outgoing):
        raise AssertionError("the exchange ran before the options were checked")
    svc._exchange = no_exchange
    with pytest.raises(ValueError):
        svc.serve([("a", "search_memories", "q", 3), ("a", "search_memories", "q", 3, options)])
    with pytest.raises(ValueError):
        svc.serve([("a", "search_memories", "q", 3, {"where": {}}, "one too many")])
    svc.close()


def test_a_boost_without_now_reads_the_clock_once_per_round(tmp_path, monkeypatch):
    from lazzaro_amd.core import boost as B
    reads = []
    monkeypatch.setattr(B, "_clock", lambda: reads.append(1) or NOW + len(reads))
    svc = _service(tmp_path)
    seen = []
    exchange = svc._exchange
    svc._exchange = lambda out: seen.append(json.loads(json.dumps(out))) or exchange(out)
    svc.serve([("a", "search_memories", "q", 3, {"boost": 0.5}), ("b", "search_memories", "q", 3, {"boost": 1.0}),
               ("c", "search_memories", "q", 3, {"boost": {"salience": 1.0, "now": 5.0}})])
    assert len(reads) == 1
    nows = [item[3][2]["boost"]["now"] for item in seen[0][0]]
    assert nows == [NOW + 1, NOW + 1, 5.0]
    svc.close()


SPECS = [dict(where={"types": ["b", "a"], "exclude_ids": ["z", "y"], "since": 0.1, "super_nodes": False}),
         dict(boost=MemoryBoost(salience=0.3, recency=0.7, clock="created", type_weights={"a": 0.25}, now=NOW + 0.1)),
         dict(where=MemoryFilter(min_salience=1 / 3, shard_keys=["work"]), boost=0.5),
         dict(diversity=0.3, fetch_k=24, where={"min_access_count": 2}),
         dict(expand={"hops": 2, "fanout": 4}, boost={"frequency": 1.0, "now": 1.5}),
         dict(lexical={"alpha": 0.25, "pool": 32}, where={"until": 9.5}),
         dict(rerank=32, where={"accessed_since": 1e9})]


@pytest.mark.parametrize("options", SPECS)
def test_the_normal_form_survives_json(options):
    spec = SearchSpec.of(5, **options)
    wire = json.loads(json.dumps(spec.as_dict()))
    back = SearchSpec.of(5, **wire)
    assert back == spec
    assert back.as_dict() == spec.as_dict()
    if spec.where is not None:
        assert MemoryFilter.from_dict(json.loads(json.dumps(spec.where.to_dict()))) == spec.where
        assert back.where.key() == spec.where.key()
    if spec.boost is not None:
        assert MemoryBoost.coerce(json.loads(json.dumps(spec.boost.to_dict()))) == spec.boost
        assert back.boost.key() == spec.boost.key() and back.boost.now == spec.boost.now
    assert spec.bias_only == (set(options) <= {"where", "boost"})


def test_mt_bias_ref_equals_the_oracle():
    """The torch formulation (the CPU tier of ``mt_bias``) against the numpy
    oracle, bit for bit, over the jobs of the GPU kernel test; and the arena
    ``mt_bias`` lays out on the CPU."""
    from lazzaro_amd.ops.mt_bias_ops import mt_bias, mt_bias_ref
    from tests.kernels._mtbias_cases import cases
    from tests.kernels._mtbias_ref import job_column_ref
    cs, _ = cases("cpu")
    jobs = [g._mt_bias_job(flt, boost, metric) for _, g, flt, boost, metric in cs]
    cols = mt_bias_ref(jobs)
    arena, offs = mt_bias(jobs)
    passing = 0
    for (label, g, flt, boost, metric), job, col, off in zip(cs, jobs, cols, offs):
        want = job_column_ref(job)
        assert col.dtype == torch.float32 and col.shape == (g.n,), label
        assert np.array_equal(col.numpy().view(np.int32), want.view(np.int32)), label
        assert off % 4 == 0 and torch.equal(arena[off: off + g.n].view(torch.int32), col.view(torch.int32)), label
        # the per-tenant column: existing code, a second reference
        if g.n:
            ref = g.boost_bias(boost, metric, where=flt) if boost is not None else g._filter_plan(flt, metric == "l2").bias
            assert torch.equal(ref.view(torch.int32), col.view(torch.int32)), label
        passing += int(np.isfinite(want).sum())
    assert passing > 5000  # (the jobs do let rows through)


def test_the_other_surfaces_still_refuse():
    DMS = DistributedMemoryService
    for kw in ({"where": {"types": ["fact"]}}, {"boost": 0.5}):
        for call in (lambda: HBMStore.search_nodes_multi(None, [[0.0] * D], ["u"], **kw),
                     lambda: DMS.search_routed(None, ["u"], ["q"], **kw),
                     lambda: next(DMS.search_routed_stream(None, [(["u"], ["q"])], **kw)),
                     lambda: DMS.search_global_batch(None, ["q"], **kw),
                     lambda: DMS.search_global(None, torch.zeros(D), **kw)):
            with pytest.raises(NotImplementedError):
                call()
