"""Options in the served batch: what per-request ``where=`` / ``boost=`` cost
in the multi-tenant round of ``DistributedMemoryService.serve_stream``.

Setup (synthetic): ``--tenants`` tenants x about ``--rows`` x ``--dim`` unit
rows on one GPU, four node types, creation times uniform over 1e6 s, rounds of
``--batch`` ``search_memories`` requests with random-init encoder weights.
Arms, interleaved, medians of ``--reps`` repetitions of ``--steps`` pipelined
rounds each (ms per round, wall clock ending in a device synchronise):

* ``none``           no options: the reference point, same run;
* ``where``          a types + since filter on every request (passes about 10 %);
* ``boost``          ``boost=0.5`` on every request;
* ``both``           the filter and the boost;
* ``both_distinct``  the filter and the boost, every request of a round on its
                     own tenant (every request a distinct job), 8 distinct
                     filters in all.

Also: ``lzk_mt_bias`` alone over the jobs of one ``both`` round between HIP
events, the launches queued behind a long matrix product (bench_fuse.py's
``event_ms``), beside its model bytes against the float4-copy rate; and 64 of
the same filtered requests answered one ``search_memories_batch(where=)`` call
per request, the only way before this (64 timed, scaled to the batch). That
kernel figure is a warm-cache one (one 26 MB job set, launched over and over);
``kernel_cold`` is one job per tenant, each launch alone between events after
1 GiB of other writes. ``host_pieces_of_one_both_round`` times the host steps of
one round one by one. The populated heap is frozen out of the garbage collector
(``gc.freeze()``): a full collection over the tenants' strings costs tens of ms
and would land in one repetition of one arm or another.

``--compare-tree PATH`` instead measures ``none`` alone in this tree and in
another built checkout of the project, in alternating child processes
(bench_rerank.py's step): what a round without options costs against a tree
without the feature.

Every step runs in a child process under its own ``timeout``. Writes JSON
files into ``--out`` and prints one JSON line."""
import argparse
import json
import os
import random
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOW = 1_700_000_000.0
TYPES = ("preference", "fact", "event", "semantic")
WORDS = "memory user likes python graph kernel music travel project deadline family hobby".split()
_hold = None


def log(*a):
    print(f"[{time.strftime('%H:%M:%S')}]", *a, file=sys.stderr, flush=True)


def summary(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
            "reps_ms": [round(x, 4) for x in v]}


def event_ms(fn, iters=20):
    """ms per call between two HIP events around ``iters`` back-to-back calls
    queued behind a product of two 8,192 x 8,192 matrices."""
    import torch
    global _hold
    if _hold is None:
        _hold = torch.randn(8192, 8192, device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.mm(_hold, _hold)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def build(a):
    import tempfile

    import torch

    from lazzaro_amd.core.embedders import OnDeviceEmbedder
    from lazzaro_amd.core.memory_system import MemorySystem
    from lazzaro_amd.core.providers import LocalLLM
    from lazzaro_amd.core.vector_store import HBMStore
    from lazzaro_amd.parallel import Communicator
    from lazzaro_amd.parallel.service import DistributedMemoryService
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    emb = OnDeviceEmbedder(a.model, device=dev, max_len=32)
    db = tempfile.mkdtemp(prefix="lzmtopt_")
    store = HBMStore(db_dir=db, device=dev)

    def factory(user, load_from_disk=False):
        return MemorySystem(llm_provider=LocalLLM(), embedding_provider=emb, enable_async=False, db_dir=db,
                            user_id=user, store=store, device=dev, load_from_disk=load_from_disk,
                            max_buffer_size=10 ** 9, enable_caching=False)
    svc = DistributedMemoryService(Communicator.local(), factory)
    users = [f"user{i}" for i in range(a.tenants)]
    rng = random.Random(0)
    gen = torch.Generator(device=dev).manual_seed(0)
    cpu = torch.Generator().manual_seed(0)
    t0 = time.time()
    rows = 0
    for j, u in enumerate(users):
        g = svc.system(u).graph
        n = rng.randint(a.rows // 4, a.rows * 7 // 4)
        V = torch.randn(n, a.dim, device=dev, generator=gen)
        V /= V.norm(dim=1, keepdim=True)
        g.add_nodes([f"{u}_m{i}" for i in range(n)], [f"memory {i} of {u}" for i in range(n)], V,
                    shard=g.shard_id("default"), types=[TYPES[i & 3] for i in range(n)],
                    sal=torch.rand(n, generator=cpu), acc=torch.randint(0, 20, (n,), generator=cpu),
                    last=NOW - torch.rand(n, generator=cpu, dtype=torch.float64) * 1e6,
                    ts=NOW - torch.rand(n, generator=cpu, dtype=torch.float64) * 1e6, stored=True, now=NOW)
        g.store_bias("l2")
        rows += n
        if j % 2000 == 0:
            log(f"{j}/{len(users)} tenants, {rows:,} rows ({time.time() - t0:.0f}s)")
    torch.cuda.synchronize()
    svc.warm_table()
    # the tenants hold millions of Python strings: a full collection over them takes tens of ms and would
    # land in one repetition of one arm or another. Move them out of the collector's reach, as a server
    # does after loading (the young generations keep running).
    import gc
    gc.collect()
    gc.freeze()
    return svc, users, rows, round(time.time() - t0, 1)


def filt(i):
    """Filter ``i`` of 8: two of four types and the newest fifth: about 10 %."""
    return {"types": ["preference", "fact"], "since": NOW - 2e5 - 1e3 * (i % 8)}


def rounds(a, users, arm, seed):
    rng = random.Random(seed)
    out = []
    for _ in range(a.steps):
        us = rng.sample(users, a.batch) if arm == "both_distinct" else [rng.choice(users) for _ in range(a.batch)]
        reqs = []
        for q, u in enumerate(us):
            r = (u, "search_memories", " ".join(rng.choice(WORDS) for _ in range(12)), a.k)
            if arm == "where":
                r += ({"where": filt(0)},)
            elif arm == "boost":
                r += ({"boost": {"salience": 0.25, "frequency": 0.15, "recency": 0.1, "now": NOW}},)
            elif arm in ("both", "both_distinct"):
                r += ({"where": filt(q if arm == "both_distinct" else 0),
                       "boost": {"salience": 0.25, "frequency": 0.15, "recency": 0.1, "now": NOW}},)
            reqs.append(r)
        out.append(reqs)
    return out


def timed(svc, rr):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in svc.serve_stream(rr):
        pass
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / len(rr)


def step_none(a):
    svc, users, rows, pop = build(a)
    for r in rounds(a, users, "none", 1)[:2]:
        svc.serve(r)
    t = [timed(svc, rounds(a, users, "none", 10 + i)) for i in range(a.reps)]
    svc.close()
    return {"step": "none", "tag": a.tag, "rows_total": rows, "populate_s": pop, "none": summary(t)}


def step_ab(a):
    import numpy as np
    import torch

    from lazzaro_amd.ops import _lib
    from lazzaro_amd.ops import mt_bias_ops as MB
    svc, users, rows, pop = build(a)
    arms = ["none", "where", "boost", "both"] + (["both_distinct"] if a.tenants >= a.batch else [])
    out = {"step": "ab", "tenants": a.tenants, "rows_total": rows, "dim": a.dim, "k": a.k, "batch": a.batch,
           "steps": a.steps, "reps": a.reps, "populate_s": pop, "copy_tbps": a.copy_tbps, "model": a.model}
    t0 = time.perf_counter()
    for u in users:  # every tenant's type-code column, built once per tenant like an index at load
        svc.system(u).graph._type_codes()
    torch.cuda.synchronize()
    out["type_code_columns_first_build_s"] = round(time.perf_counter() - t0, 2)
    for arm in arms:  # warm-up: code objects, the staging buffers
        for r in rounds(a, users, arm, 1)[:2]:
            svc.serve(r)
    t = {arm: [] for arm in arms}
    before = dict(svc.stats())
    for i in range(a.reps):
        for arm in arms:  # interleaved
            t[arm].append(timed(svc, rounds(a, users, arm, 10 + i)))
    out["ms_per_round"] = {arm: summary(v) for arm, v in t.items()}
    out["counters"] = {k: v - before[k] for k, v in svc.stats().items()}
    for arm in arms[1:]:
        out["ms_per_round"][arm]["minus_none_ms"] = round(
            out["ms_per_round"][arm]["median_ms"] - out["ms_per_round"]["none"]["median_ms"], 4)
    log("ms per round:", {arm: out["ms_per_round"][arm]["median_ms"] for arm in arms})
    # the kernel alone over the jobs of one `both` round
    reqs = rounds(a, users, "both", 99)[0]
    from lazzaro_amd.core.search_spec import SearchSpec
    jobs, seen = [], set()
    for u, _, _, k, o in reqs:
        spec = SearchSpec.of(k, **o)
        if (u, spec.where.key()) not in seen:
            seen.add((u, spec.where.key()))
            jobs.append(svc.system(u).graph._mt_bias_job(spec.where, spec.boost, "l2"))
    offs, total = MB._offsets(jobs)
    rec, blk0, aux = MB._pack(jobs, offs)
    host = torch.from_numpy(np.concatenate(
        [rec.view(np.uint8).reshape(-1), blk0.view(np.uint8), np.zeros((-blk0.nbytes) % 8, np.uint8), aux]))
    dbuf = host.cuda()
    arena = torch.empty(total, dtype=torch.float32, device="cuda")
    jb, bb = rec.nbytes, (blk0.nbytes + 7) & ~7
    L, base = _lib.lib(), dbuf.data_ptr()

    def launch():
        _lib.check(L.lzk_mt_bias(base, len(jobs), base + jb, base + jb + bb, arena.data_ptr(), int(blk0[-1]),
                                 _lib.stream_ptr(arena.device)), "lzk_mt_bias")
    launch()
    torch.cuda.synchronize()
    kt = [event_ms(launch) for _ in range(a.reps)]
    nrows = sum(int(j.n) for j in jobs)
    # per row: kind + stored + tcode (3 B), ts (8 B, the since test, read for the rows that pass the type test:
    # counted for all), sqn (4), sal + acc (8), last (8), kind again is cached; 4 B written
    model = nrows * (3 + 8 + 4 + 8 + 8 + 4)
    k = summary(kt)
    k.update(jobs=len(jobs), rows=nrows, blocks=int(blk0[-1]), model_bytes=model,
             model_tbps=round(model / (k["median_ms"] * 1e-3) / 1e12, 3))
    k["share_of_copy_rate"] = round(k["model_tbps"] / a.copy_tbps, 3)
    t0 = time.perf_counter()
    MB._pack(jobs, offs)
    k["host_pack_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    out["kernel"] = k
    out["kernel"]["note"] = "the same 26 MB job set launched 20 times back to back: reads served by L2 / MALL"
    # cold: one job per tenant (every column of every tenant, more than the 256 MB last-level cache together
    # with what the flush writes), each launch alone between events after 1 GiB of other writes
    alljobs = [svc.system(u).graph._mt_bias_job(spec.where, spec.boost, "l2") for u in users]
    offs2, total2 = MB._offsets(alljobs)
    rec2, blk2, aux2 = MB._pack(alljobs, offs2)
    d2 = torch.from_numpy(np.concatenate(
        [rec2.view(np.uint8).reshape(-1), blk2.view(np.uint8), np.zeros((-blk2.nbytes) % 8, np.uint8), aux2])).cuda()
    arena2 = torch.empty(total2, dtype=torch.float32, device="cuda")
    jb2, bb2, base2 = rec2.nbytes, (blk2.nbytes + 7) & ~7, d2.data_ptr()
    flush = torch.empty(1 << 28, dtype=torch.float32, device="cuda")
    cold = []
    for _ in range(a.reps):
        flush.add_(1.0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.check(L.lzk_mt_bias(base2, len(alljobs), base2 + jb2, base2 + jb2 + bb2, arena2.data_ptr(),
                                 int(blk2[-1]), _lib.stream_ptr(arena2.device)), "lzk_mt_bias")
        e1.record()
        e1.synchronize()
        cold.append(e0.elapsed_time(e1))
    nrows2 = sum(int(j.n) for j in alljobs)
    kc = summary(cold)
    kc.update(jobs=len(alljobs), rows=nrows2, model_bytes=nrows2 * 35,
              model_tbps=round(nrows2 * 35 / (kc["median_ms"] * 1e-3) / 1e12, 3))
    kc["share_of_copy_rate"] = round(kc["model_tbps"] / a.copy_tbps, 3)
    out["kernel_cold"] = kc
    del flush, arena2, d2, alljobs
    log("lzk_mt_bias cold:", kc["median_ms"], "ms for", kc["jobs"], "jobs;", kc["model_tbps"], "TB/s model")
    # where the host time of an options round goes: the pieces of one `both` round, each timed alone
    from lazzaro_amd.parallel.service import DistributedMemoryService as S
    host = {}
    t0 = time.perf_counter()
    wires = [S._wire_options(list(r[2:]), []) for r in reqs]
    host["sender_validate_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    t0 = time.perf_counter()
    specs = [SearchSpec.of(r[3], **w[0]) for r, w in zip(reqs, wires)]
    host["owner_rebuild_spec_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    t0 = time.perf_counter()
    jb_ = [svc.system(r[0]).graph._mt_bias_job(sp.where, sp.boost, "l2") for r, sp in zip(reqs, specs)]
    host["job_build_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    o_, _ = MB._offsets(jb_)
    t0 = time.perf_counter()
    MB._pack(jb_, o_)
    host["pack_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    host["requests"] = len(reqs)
    out["host_pieces_of_one_both_round"] = host
    log("host pieces:", host)
    log("lzk_mt_bias:", k["median_ms"], "ms for", len(jobs), "jobs,", nrows, "rows;", k["model_tbps"], "TB/s model")
    # the same filtered requests, one search_memories_batch(where=) per request
    reqs = rounds(a, users, "where", 98)[0][:64]
    for u, _, q, kk, o in reqs[:4]:
        svc.system(u).search_memories_batch([q], kk, **o)
    per = []
    for i in range(min(a.reps, 3)):
        reqs = rounds(a, users, "where", 200 + i)[0][:64]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for u, _, q, kk, o in reqs:
            svc.system(u).search_memories_batch([q], kk, **o)
        torch.cuda.synchronize()
        per.append((time.perf_counter() - t0) * 1e3)
    out["per_request_where"] = dict(summary(per), requests_timed=64,
                                    scaled_to_batch_ms=round(statistics.median(per) * a.batch / 64, 2))
    svc.close()
    return out


def compare(a, base):
    """``none`` in the other tree and in this one, alternating processes."""
    runs = {"other": [], "this": []}
    for i in range(a.rounds):
        for tag, tree in (("other", os.path.abspath(a.compare_tree)), ("this", ROOT)):
            log("round", i, tag)
            p = subprocess.run(["timeout", "-k", "10", str(a.step_timeout)] + base +
                               ["--step", "none", "--tree", tree, "--tag", tag], stdout=subprocess.PIPE, text=True)
            if p.returncode != 0:
                log(f"{tag} failed with exit status {p.returncode}: stopping")
                return p.returncode
            runs[tag].append(json.loads(p.stdout.strip().splitlines()[-1]))
    v = {tag: [x for r in runs[tag] for x in r["none"]["reps_ms"]] for tag in runs}
    res = {"step": "compare", "tenants": a.tenants, "dim": a.dim, "k": a.k, "batch": a.batch, "steps": a.steps,
           "rounds": a.rounds, "reps_per_round": a.reps, "other": summary(v["other"]), "this": summary(v["this"])}
    res["this_minus_other_ms"] = round(res["this"]["median_ms"] - res["other"]["median_ms"], 4)
    res["other_spread_ms"] = round(res["other"]["max_ms"] - res["other"]["min_ms"], 4)
    res["within_the_other_trees_spread"] = abs(res["this_minus_other_ms"]) <= res["other_spread_ms"]
    with open(os.path.join(a.out, f"none_vs_other_tree_{a.tenants}.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tenants", type=int, default=8192)
    ap.add_argument("--rows", type=int, default=800, help="mean memories per tenant")
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--model", default="bge-base")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=6, help="pipelined rounds per repetition")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--copy-tbps", type=float, default=6.29, help="the float4 copy rate the model is set against")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r30", "mt_options"))
    ap.add_argument("--step-timeout", type=int, default=900)
    ap.add_argument("--compare-tree", default="", help="another built checkout: measure the no-options round against it")
    ap.add_argument("--rounds", type=int, default=2, help="alternations of --compare-tree")
    ap.add_argument("--step", default="", help="(internal) run one step in this process")
    ap.add_argument("--tree", default=ROOT, help="(internal) the checkout whose package a step imports")
    ap.add_argument("--tag", default="this", help="(internal)")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    if a.step:
        sys.path.insert(0, a.tree)
        res = {"ab": step_ab, "none": step_none}[a.step](a)
        if a.step == "ab":
            with open(os.path.join(a.out, f"ab_{a.tenants}x{a.rows}x{a.dim}.json"), "w") as f:
                json.dump(res, f, indent=1)
        print(json.dumps(res))
        return 0
    base = [sys.executable, os.path.abspath(__file__)]
    for name in ("tenants", "rows", "dim", "model", "batch", "steps", "k", "reps", "copy_tbps", "out"):
        base += ["--" + name.replace("_", "-"), str(getattr(a, name))]
    if a.compare_tree:
        return compare(a, base)
    log("step ab")
    rc = subprocess.run(["timeout", "-k", "10", str(a.step_timeout)] + base + ["--step", "ab"]).returncode
    if rc != 0:
        log(f"step ab failed with exit status {rc}: stopping")
    return rc


if __name__ == "__main__":
    sys.exit(main())
