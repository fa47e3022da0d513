"""Options in the served batch on one GPU: ``search_memories`` requests that
carry ``where`` / ``boost`` ride the fused multi-tenant scan -- one
``lzk_mt_bias`` launch writes a bias column per distinct (tenant, filter,
boost) of the round and ``segment_topk`` reads it through the per-query bias
address -- and return what each tenant's own ``search_memories_batch([q],
limit, **options)`` returns.

How results are compared. Both sides are fp32 scans in different summation
orders, so ids are compared under the repository's two rules against an fp64
oracle of the scores, ``key(r) = 2 <q, x_r> + col[r] - |q|^2`` over the fp32
rows, the fp32 query and the fp32 bias column ``col`` of the tenant's own code
(``_filter_plan(...).bias`` / ``boost_bias(...)``; the kernel test shows
``lzk_mt_bias`` writes the same bits):

1. the returned ids equal the oracle's, in order, up to the first position
   whose fp64 key lies within ``2 tol`` of the next row's;
2. every returned id's key is within ``2 tol`` of the best key left out.

``tol`` bounds |fp32 score - key| for segment.hip's summation order at D = 64,
unit rows and queries (|q|, |x| <= 1 + 2^-20), u = 2^-24: a lane (8 per row)
sums D / 32 = 2 pieces, each a 4-term fma chain (4 roundings), with 1 rounding
between them; three shuffle adds follow: at most 4 + 1 + 3 = 8 < 9 roundings
on any product, so |a - <q, x>| <= gamma_9 sum |q_d x_d| <= 9.01 u. ``alpha =
2`` is exact: 18.02 u. ``+ bias`` rounds once, u |2 a + col| <= u (2 + 1 + 2)
(|col| <= |x|^2 + prior, and the priors here are <= c * 1 = 2), and ``+ qbias``
once more, <= 6 u. tol = 30 u = 30 * 2^-24 ~ 1.8e-6. The per-tenant reference
scans in other orders with no more roundings per product at this width, and is
held to the same rules. (``test_nothing_stale_is_served_after_a_touch`` boosts
with frequency 1 + recency 1: its priors reach c * 2 = 4, for which the same
sum gives 34 u. It is held to the 30 u derived above all the same: the smaller
bound excuses fewer near-ties and makes both rules stricter, never looser.)

Condition: at most 5 % of the requests may contain a near-tie (two of the
oracle's top ``limit + 1`` keys within ``2 tol``). The seed (SEED) was picked
so that the oracle alone meets this -- checked on the CPU tier's tensors, where
no request of the 200 has one -- and the test asserts it on the device's.
"""
import hashlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
TOL = 30 * U
SEED = 11
NOW = 1_700_000_000.0
TYPES = ("preference", "fact", "event", "semantic")
FILTERS = [{"types": ["preference", "fact"]},
           {"min_salience": 0.4, "shard_keys": ["work", "default"]},
           {"since": NOW - 1.5e6, "until": NOW - 1.1e6},
           {"min_access_count": 5, "super_nodes": False},
           {"types": ["event", "never-seen"], "accessed_since": NOW - 6e5}]
BOOSTS = [{"salience": 0.5, "frequency": 0.3, "recency": 0.2, "now": NOW},
          {"salience": 0.2, "recency": 0.6, "recency_scale": 3600.0 * 24 * 3, "clock": "created", "now": NOW + 500.0,
           "type_weights": {"preference": 0.2, "never-seen": 0.2}}]


class RandEmbedder:
    """text -> a fixed pseudo-random unit vector (tests/kernels/test_service_gpu.py's)."""

    def __init__(self, dim=64):
        self.dim = dim

    def _v(self, t):
        seed = int.from_bytes(hashlib.md5(t.encode()).digest()[:4], "little")
        v = np.random.default_rng(seed).standard_normal(self.dim).astype(np.float32)
        return (v / np.linalg.norm(v)).tolist()

    def embed(self, t):
        return self._v(t)

    def batch_embed(self, ts):
        return [self._v(t) for t in ts]


def build_service(db, device="cuda", tenants=24, tag="t"):
    from lazzaro_amd.core.memory_system import MemorySystem
    from lazzaro_amd.core.providers import LocalLLM
    from lazzaro_amd.parallel import Communicator
    from lazzaro_amd.parallel.service import DistributedMemoryService
    emb = RandEmbedder()

    def factory(user, load_from_disk=True):
        return MemorySystem(llm_provider=LocalLLM(), embedding_provider=emb, enable_async=False, db_dir=str(db),
                            user_id=user, device=device, load_from_disk=load_from_disk, max_buffer_size=10 ** 6)
    comm = Communicator.local(torch.device("cuda")) if device == "cuda" else Communicator.local()
    svc = DistributedMemoryService(comm, factory)
    users = [f"{tag}{i}" for i in range(tenants)]
    rng = np.random.default_rng(SEED)
    for j, u in enumerate(users):
        g = svc.system(u).graph
        n = 50 + 37 * j
        texts = [f"{u} memory {i}" for i in range(n)]
        work, home = g.shard_id("work"), g.shard_id("home")
        g.add_nodes([f"{u}_n{i}" for i in range(n)], texts, torch.tensor(emb.batch_embed(texts), device=device),
                    shard=rng.choice(np.array([work, home, -1]), n).tolist(),
                    types=[TYPES[int(t)] for t in rng.integers(0, 4, n)],
                    sal=rng.random(n).astype(np.float32).tolist(), acc=rng.integers(0, 15, n).tolist(),
                    last=(NOW - rng.random(n) * 1e6).tolist(), ts=(NOW - 2e6 + rng.random(n) * 1e6).tolist(),
                    sup=(rng.random(n) < 0.1).astype(np.uint8).tolist(), stored=True, now=NOW)
    return svc, users, emb


def make_requests(users, n=200, seed=SEED, tag="query"):
    """A third without options, a third with one of five filters, a third
    with a filter and a boost (explicit ``now``)."""
    rng = np.random.default_rng(seed + 1)
    reqs = []
    for q in range(n):
        u = users[int(rng.integers(len(users)))]
        k = int(rng.integers(1, 9))
        base = (u, "search_memories", f"{tag} {q}", k)
        f = FILTERS[int(rng.integers(len(FILTERS)))]
        if q % 3 == 1:
            base += ({"where": f},)
        elif q % 3 == 2:
            base += ({"where": f, "boost": BOOSTS[int(rng.integers(len(BOOSTS)))]},)
        reqs.append(base)
    return reqs


def oracle_keys(svc, emb, req):
    """fp64 keys of one request over its tenant's rows (-inf: not eligible)."""
    g = svc.system(req[0]).graph
    opts = req[4] if len(req) > 4 else {}
    with g.on_stream():
        if opts.get("boost") is not None:
            col = g.boost_bias(opts["boost"], "l2", where=opts.get("where"))
        elif opts.get("where") is not None:
            from lazzaro_amd.core.filters import MemoryFilter
            col = g._filter_plan(MemoryFilter.coerce(opts["where"]), True).bias
        else:
            col = g.store_bias("l2")
        X = g.emb32[: g.n].double().cpu().numpy()
        col = col[: g.n].double().cpu().numpy()
    q = np.asarray(emb.embed(req[2]), dtype=np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return 2.0 * (X @ q) + col - float(q @ q)


def near_tie(keys, k):
    s = np.sort(keys[np.isfinite(keys)])[::-1][: k + 1]
    return bool(s.size > 1 and (s[:-1] - s[1:] <= 2 * TOL).any())


def check_ids(ids, g, keys, k, what):
    """The two rules of this file's header."""
    rows = [g.row_of[i] for i in ids]
    order = sorted(np.nonzero(np.isfinite(keys))[0].tolist(), key=lambda r: (-keys[r], r))
    assert len(rows) == min(k, len(order)) and len(set(rows)) == len(rows), what
    for j, r in enumerate(rows):
        if j + 1 < len(order) and keys[order[j]] - keys[order[j + 1]] <= 2 * TOL:
            break  # a near-tie: the order is free from here
        assert r == order[j], (what, j, rows, order[:k])
    left = [r for r in order if r not in set(rows)]
    if left:
        assert all(keys[r] >= keys[left[0]] - 2 * TOL for r in rows), (what, rows, order[:k])


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    svc, users, emb = build_service(tmp_path_factory.mktemp("mt_options"))
    reqs = make_requests(users)
    ref = []
    for r in reqs:  # the reference, computed once: each request through its tenant's own search
        opts = r[4] if len(r) > 4 else {}
        ref.append([n.id for n in svc.system(r[0]).search_memories_batch([r[2]], r[3], **opts)[0]])
    yield svc, users, emb, reqs, ref
    svc.close()


def test_mixed_round_matches_per_tenant(world):
    svc, users, emb, reqs, ref = world
    before = dict(svc.stats())
    got = svc.serve(reqs)
    st = svc.stats()
    with_opts = [r for r in reqs if len(r) > 4]
    assert len(with_opts) in (133, 134) and len(reqs) == 200
    assert st["mt_option_requests"] - before["mt_option_requests"] == len(with_opts)
    assert st["mt_option_fallbacks"] == before["mt_option_fallbacks"]
    combos = {(r[0], repr(sorted(r[4]["where"].items())), repr(r[4].get("boost"))) for r in with_opts}
    assert st["mt_bias_jobs"] - before["mt_bias_jobs"] == len(combos) and len(combos) < len(with_opts)
    ties = 0
    for r, g_ids, r_ids in zip(reqs, got, ref):
        g = svc.system(r[0]).graph
        keys = oracle_keys(svc, emb, r)
        ids = [n["id"] for n in g_ids]
        check_ids(ids, g, keys, r[3], ("served", r))
        check_ids(r_ids, g, keys, r[3], ("per tenant", r))
        if near_tie(keys, r[3]):
            ties += 1
        else:
            assert ids == r_ids, r
        if len(r) > 4:  # memories that pass, and only those
            f = r[4]["where"]
            for n in g_ids:
                assert "types" not in f or n["type"] in f["types"]
                assert "min_salience" not in f or n["salience"] >= np.float32(f["min_salience"])
                assert "min_access_count" not in f or n["access_count"] >= f["min_access_count"]
                assert f.get("super_nodes") is not False or not n["is_super_node"]
    assert ties <= 0.05 * len(reqs), ties
    assert sum(len(x) > 0 for x, r in zip(got, reqs) if len(r) > 4) > 100  # the filters do let memories through


def test_requests_without_options_are_not_disturbed(world):
    svc, users, emb, reqs, ref = world
    mixed = svc.serve(reqs)
    plain_reqs = [r for r in reqs if len(r) == 4]
    plain = svc.serve(plain_reqs)
    assert [list(x) for x, r in zip(mixed, reqs) if len(r) == 4] == [list(x) for x in plain]
    assert [[n["id"] for n in x] for x in plain] == [i for i, r in zip(ref, reqs) if len(r) == 4]


def test_serve_stream_equals_serve_per_round(world):
    svc, users, emb, reqs, ref = world
    rounds = [make_requests(users, 64, seed=20 + r, tag=f"round {r}") for r in range(5)]
    want = [[list(x) for x in svc.serve(r)] for r in rounds]
    got = [[list(x) for x in out] for out in svc.serve_stream(rounds)]
    assert got == want


def test_other_options_are_answered_per_tenant_and_counted(world):
    svc, users, emb, reqs, ref = world
    before = dict(svc.stats())
    extra = (users[3], "search_memories", "query 7", 4, {"diversity": 0.5})
    other = (users[5], "search_memories", "query 8", 3, {"expand": 1, "where": FILTERS[0]})
    got = svc.serve(reqs[:30] + [extra] + reqs[30:60] + [other])
    st = svc.stats()
    assert st["mt_option_fallbacks"] - before["mt_option_fallbacks"] == 2
    for r, out in ((extra, got[30]), (other, got[61])):
        want = svc.system(r[0]).search_memories_batch([r[2]], r[3], **r[4])[0]
        assert [n["id"] for n in out] == [n.id for n in want] and len(out) == r[3]
    assert [[n["id"] for n in x] for x in got[:30] + got[31:61]] == [
        [n["id"] for n in x] for x in svc.serve(reqs[:60])]


def test_nothing_stale_is_served_after_a_touch(tmp_path):
    """A chat turn between two rounds touches rows of one tenant (its
    retrieval bumps their access counts and last-access times): the next
    round's boosted results equal the per-tenant reference computed after it."""
    svc, users, emb = build_service(tmp_path, tenants=6, tag="c")
    boost = {"frequency": 1.0, "recency": 1.0, "recency_scale": 1e5, "now": NOW}
    reqs = [(u, "search_memories", f"{users[2]} memory {q}", 6, {"where": {"max_salience": 0.9}, "boost": boost})
            for q, u in enumerate(users * 4)]
    first = [[n["id"] for n in x] for x in svc.serve(reqs)]
    g = svc.system(users[2]).graph
    acc0 = g.acc[: g.n].clone()
    svc.serve([(users[2], "start_conversation"), (users[2], "chat", f"{users[2]} memory 3"),
               (users[2], "chat", f"{users[2]} memory 9")])
    touched = torch.nonzero(g.acc[: g.n] != acc0).flatten().tolist()
    assert touched, "the chat turns touched no row"
    second = [[n["id"] for n in x] for x in svc.serve(reqs)]
    for r, ids, old in zip(reqs, second, first):
        ms = svc.system(r[0])
        want = [n.id for n in ms.search_memories_batch([r[2]], r[3], **r[4])[0]]
        keys = oracle_keys(svc, emb, r)
        check_ids(ids, ms.graph, keys, r[3], r)
        if not near_tie(keys, r[3]):
            assert ids == want, r
        if r[0] != users[2]:
            assert ids == old
    assert any(ids != old for r, ids, old in zip(reqs, second, first) if r[0] == users[2]), \
        "the touch changed no boosted result: the test shows nothing"
    svc.close()
