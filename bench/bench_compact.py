"""Row reclamation on one large tenant (``TenantGraph.compact``, compact.hip):
``--rows`` x ``--dim`` unit rows in one TenantGraph, ``--dead`` of them removed
and unstored at scattered positions, then

(a) ``compact()`` through the kernels: wall time (host bookkeeping of the id
    columns included), device time of the column moves, bytes moved, bytes / time
    (a direct-path move reads and writes each kept byte once, so read + write
    traffic is twice that; the ceiling is the device's float4-copy rate);
(b) the same reclamation by the torch formulation (COMPACT_KERNEL = False,
    out of place: ``col[:m] = col[keep_idx]``);
(c) ``store_search`` time for ``--batch`` queries and for 1 query, before and
    after (the scan is row-bound: the expected change is the row ratio);
(d) peak HBM during the compaction against the tenant's footprint.

(a) and (b) alternate on freshly built tenants (``--runs`` each, interleaved
on the one device). Prints one JSON line; ``--out`` also writes it."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def log(*a):
    print(f"[{time.strftime('%H:%M:%S')}]", *a, file=sys.stderr, flush=True)


def build(TG, dev, N, D, dead, ids, seed=3):
    g = TG.TenantGraph(device=dev, dim=D, capacity=N)
    code = g.shard_id("default")
    gen = torch.Generator(device=dev).manual_seed(seed)
    C = torch.randn(4096, D, device=dev, generator=gen)
    C /= C.norm(dim=1, keepdim=True)
    chunk = 1 << 21
    for c0 in range(0, N, chunk):
        c1 = min(N, c0 + chunk)
        X = C[torch.randint(0, 4096, (c1 - c0,), device=dev, generator=gen)] + 0.05 * torch.randn(
            c1 - c0, D, device=dev, generator=gen)
        X /= X.norm(dim=1, keepdim=True)
        g.add_nodes(ids[c0:c1], [""] * (c1 - c0), X, shard=code, stored=True, want_rows=False)
        del X
    g.clear_tracking()
    vic = np.sort(np.random.default_rng(seed).choice(N, size=dead, replace=False))
    g.remove_nodes(vic.tolist(), drop_edges=False, unstore=True)
    g.take_deleted()
    torch.cuda.synchronize(dev)
    return g, C


def time_search(g, Q, k, reps):
    g.store_search(Q, k)
    g.store_search(Q, k)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        g.store_search(Q, k)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ts), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=15_000_000)
    ap.add_argument("--dead", type=int, default=5_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from lazzaro_amd.engine import tenant_graph as TG
    from lazzaro_amd.utils.tracing import tracer
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    N, D = a.rows, a.dim
    ids = [f"n{i}" for i in range(N)]
    res = {"metric": "row reclamation", "rows": N, "dead": a.dead, "dim": D, "kernel": [], "torch": []}
    search = None
    for run in range(a.runs):
        for mode in ("kernel", "torch"):
            t0 = time.time()
            g, C = build(TG, dev, N, D, a.dead, ids)
            log(f"run {run} {mode}: built in {time.time() - t0:.0f}s")
            if search is None:  # (c), once: before ...
                gen = torch.Generator(device=dev).manual_seed(11)
                Q = C[torch.randint(0, 4096, (a.batch,), device=dev, generator=gen)] + 0.06 * torch.randn(
                    a.batch, D, device=dev, generator=gen)
                Q /= Q.norm(dim=1, keepdim=True)
                search = {"rows_before": g.n, f"before_ms_{a.batch}q": time_search(g, Q, a.k, a.reps),
                          "before_ms_1q": time_search(g, Q[:1], a.k, a.reps)}
            TG.COMPACT_KERNEL = mode == "kernel"
            torch.cuda.synchronize(dev)
            foot = torch.cuda.memory_allocated(dev)
            torch.cuda.reset_peak_memory_stats(dev)
            tracer.reset()
            tracer.enable(True)  # device time of the column moves (hipEvents): the "compact_move" stage
            t0 = time.perf_counter()
            out = g.compact()
            torch.cuda.synchronize(dev)
            el = time.perf_counter() - t0
            peak = torch.cuda.max_memory_allocated(dev)
            mv = tracer.summary().get("compact_move", {}).get("total_ms", 0.0) / 1e3
            tracer.enable(False)
            TG.COMPACT_KERNEL = True
            res[mode].append({"s": round(el, 4), "move_s": round(mv, 4), "bytes_moved": out["bytes_moved"],
                              "moved_GBps": round(out["bytes_moved"] / el / 1e9, 1),
                              "move_GBps": round(out["bytes_moved"] / mv / 1e9, 1) if mv else None,
                              "footprint_GiB": round(foot / 2**30, 2), "peak_GiB": round(peak / 2**30, 2),
                              "peak_over_footprint_GiB": round((peak - foot) / 2**30, 3),
                              "rows_after": out["rows_after"], "reclaimed": out["reclaimed"]})
            log(mode, res[mode][-1])
            if "rows_after" not in search:  # ... and after
                search.update({"rows_after": g.n, f"after_ms_{a.batch}q": time_search(g, Q, a.k, a.reps),
                               "after_ms_1q": time_search(g, Q[:1], a.k, a.reps)})
                log("search", search)
            del g
            torch.cuda.empty_cache()
    res["store_search"] = search
    for mode in ("kernel", "torch"):
        res[f"{mode}_median_s"] = round(statistics.median(r["s"] for r in res[mode]), 4)
        res[f"{mode}_median_move_s"] = round(statistics.median(r["move_s"] for r in res[mode]), 4)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
