"""Options in the served batch across ranks (CPU, gloo, 2 ranks): a
``search_memories`` request with an options dict sent from rank 0 to a tenant
owned by rank 1 crosses the exchange in its JSON normal form and returns what
the owner's own search returns."""
import functools
import json

import numpy as np

from tests.distributed.test_dist_gloo import spawn

USERS = [f"user{i}" for i in range(6)]
NOW = 1_700_000_000.0
TYPES = ("preference", "fact", "event")
OPTIONS = [{"where": {"types": ["preference"]}},
           {"where": {"min_salience": 0.5, "exclude_ids": ["user1_3", "user3_3"]}, "boost": {"salience": 1.0, "now": NOW}},
           {"boost": 0.5},  # (no ``now``: the sender reads the clock, the owner must use that reading)
           {"diversity": 0.5, "where": {"types": ["fact", "event"]}},
           {"expand": 1}]


def _factory(db, user, load_from_disk=True):
    from lazzaro_amd.core.memory_system import MemorySystem
    from lazzaro_amd.core.providers import HashEmbedder, LocalLLM
    return MemorySystem(llm_provider=LocalLLM(), embedding_provider=HashEmbedder(dim=32), enable_async=False,
                        db_dir=db, user_id=user, device="cpu", max_buffer_size=10 ** 6, load_from_disk=load_from_disk)


def _workload(comm, db):
    import torch

    from lazzaro_amd.core import boost as B
    from lazzaro_amd.core.providers import HashEmbedder
    from lazzaro_amd.parallel.service import DistributedMemoryService, node_dict
    svc = DistributedMemoryService(comm, functools.partial(_factory, db), owner=lambda u: int(u[4:]) % 2)
    emb = HashEmbedder(dim=32)
    for u in USERS:
        if svc.is_local(u):
            g = svc.system(u).graph
            rng = np.random.default_rng(int(u[4:]))
            n = 30 + 5 * int(u[4:])
            texts = [f"{u} note {i} about topic {i % 7}" for i in range(n)]
            g.add_nodes([f"{u}_{i}" for i in range(n)], texts, torch.tensor(emb.batch_embed(texts)),
                        shard=g.shard_id("work"), types=[TYPES[i % 3] for i in range(n)],
                        sal=rng.random(n).astype(np.float32).tolist(), acc=rng.integers(0, 20, n).tolist(),
                        last=(NOW - rng.random(n) * 1e6).tolist(), stored=True, now=NOW)
    B._clock = lambda: NOW + 1000.0 + comm.rank  # (each rank's clock reads differently: the sender's must win)
    remote = [u for u in USERS if svc.owner(u) == 1]
    reqs = []
    if comm.rank == 0:  # every request crosses to rank 1
        for j, u in enumerate(remote * 2):
            reqs.append((u, "search_memories", f"note about topic {j}", 4, OPTIONS[j % len(OPTIONS)]))
        reqs.append((remote[0], "search_memories", "note about topic 2", 4))
    got = svc.serve(reqs)
    want = None
    if comm.rank == 1:  # the owner's own search of the same requests, with rank 0's clock reading
        want = []
        for j, u in enumerate(remote * 2):
            opts = dict(OPTIONS[j % len(OPTIONS)])
            if opts.get("boost") == 0.5:
                opts["boost"] = B.MemoryBoost.coerce(0.5).at(NOW + 1000.0)
            want.append([node_dict(n) for n in svc.system(u).search_memories_batch([f"note about topic {j}"], 4,
                                                                                    **opts)[0]])
        want.append([node_dict(n) for n in svc.system(remote[0]).search_memories_batch(["note about topic 2"], 4)[0]])
    stats = svc.stats()
    svc.close()
    return json.dumps({"got": [list(x) for x in got], "want": want, "stats": stats, "n": len(reqs)})


def test_options_cross_ranks(tmp_path):
    outs = spawn(2, functools.partial(_workload, db=str(tmp_path / "db")))
    d = {r: json.loads(v) for r, v in outs.items()}
    assert d[0]["n"] == 7 and len(d[0]["got"]) == 7 and d[1]["got"] == []
    assert d[0]["got"] == d[1]["want"]
    assert all(len(x) == 4 for x in d[0]["got"])
    assert all(n["type"] == "preference" for n in d[0]["got"][0])
    assert d[1]["stats"]["mt_option_requests"] == 6 and d[1]["stats"]["mt_option_fallbacks"] == 6
    assert d[0]["stats"]["mt_option_requests"] == 0
