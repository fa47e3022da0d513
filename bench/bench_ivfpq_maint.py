"""IVF-PQ maintenance in place (``IVFPQIndex.remove / add -> _finalize``,
csrc/kernels/ivfmaint.hip + compact.hip) against the full stable sort
(``_finalize_ref``, what every finalize was before).

(a) a codes-only index of ``--rows`` x ``--m`` bytes, arrays generated
    directly (no training): append 1,024 rows, remove 1,024 ids, both, and
    remove 10 % -- ``_finalize`` time and peak HBM over the index's footprint
    for the torch formulation and for the kernel path, alternating on the one
    index, and the bytes / time of the wide in-place moves (the same kind of
    move profiles/r7/compaction measured at 1.83 TB/s);
(b) ``--graph-rows`` x ``--graph-dim`` unit rows in one TenantGraph with
    index="ivfpq": evict 1 %, compact, and the wall time to the first search
    afterwards with the index maintained, against the rebuild (re-train on a
    262,144-row sample + re-encode of every row) a compaction used to cost.

Prints one JSON line; ``--out`` also writes it."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

R7_MOVE_GBPS = 1830.0  # profiles/r7/compaction: device rate of the in-place row move


def log(*a):
    print(f"[{time.strftime('%H:%M:%S')}]", *a, file=sys.stderr, flush=True)


def build_index(IVFPQIndex, dev, n, m, nlist, slack):
    gen = torch.Generator(device=dev).manual_seed(0)
    idx = IVFPQIndex(m, nlist=nlist, m=m, device=dev)
    idx.centroids = torch.nn.functional.normalize(torch.randn(nlist, m, device=dev, generator=gen), dim=1)
    idx.centroids16 = idx._pad(idx.centroids)
    idx.codebooks = 0.1 * torch.randn(m, 256, 1, device=dev, generator=gen)
    cap = n + slack
    lists = torch.sort(torch.randint(0, nlist, (n,), device=dev, generator=gen)).values
    codes = torch.empty((cap, m), dtype=torch.uint8, device=dev)
    for c0 in range(0, n, 1 << 24):
        c1 = min(n, c0 + (1 << 24))
        codes[c0:c1] = torch.randint(0, 256, (c1 - c0, m), dtype=torch.uint8, device=dev, generator=gen)
    # the setters take exact-size arrays; the buffers behind them carry the slack for the appends
    idx.codes = codes[:n]
    idx._codes, idx.cap = codes, cap
    for name, t in (("_list", lists.to(torch.int32)), ("_pos", torch.arange(n, device=dev)),
                    ("_vids", torch.arange(n, device=dev))):
        buf = torch.zeros(cap, dtype=t.dtype, device=dev)
        buf[:n] = t
        setattr(idx, name, buf)
    idx.list_off = torch.zeros(nlist + 1, dtype=torch.int64, device=dev)
    idx.list_off[1:] = torch.cumsum(torch.bincount(lists, minlength=nlist), 0)
    return idx


def change(idx, case, gen, next_id):
    dev = idx.device
    if case in ("append_1024", "both_1024"):
        idx.add(torch.randn(1024, idx.dim, device=dev, generator=gen), ids=torch.arange(next_id, next_id + 1024))
        next_id += 1024
    if case in ("remove_1024", "both_1024", "remove_10pct"):
        k = 1024 if case != "remove_10pct" else len(idx) // 10
        live = idx._vids[: idx.nv]
        idx.remove(live[torch.randperm(idx.nv, device=dev, generator=gen)[:k]])
    return next_id


def bench_index(a, dev, n, res):
    from lazzaro_amd.index import ivfpq as IV
    t0 = time.time()
    idx = build_index(IV.IVFPQIndex, dev, n, a.m, a.nlist, slack=1 << 16)
    log(f"{n} rows built in {time.time() - t0:.0f}s")
    gen = torch.Generator(device=dev).manual_seed(1)
    next_id = n
    out = {}
    for case in ("append_1024", "remove_1024", "both_1024", "remove_10pct"):
        out[case] = {}
        for mode in ("torch", "kernel") * a.runs:
            next_id = change(idx, case, gen, next_id)
            rows = idx.n
            torch.cuda.synchronize(dev)
            foot = torch.cuda.memory_allocated(dev)
            torch.cuda.reset_peak_memory_stats(dev)
            idx.last_maint = None
            t0 = time.perf_counter()
            if mode == "kernel":
                idx._finalize()
            else:
                idx._finalize_ref()
            torch.cuda.synchronize(dev)
            el = time.perf_counter() - t0
            peak = torch.cuda.max_memory_allocated(dev) - foot
            r = {"s": round(el, 5), "rows": rows, "peak_over_footprint_MiB": round(peak / 2**20, 1),
                 "peak_B_per_row": round(peak / rows, 2)}
            if mode == "kernel" and idx.last_maint:
                mv = idx.last_maint
                r.update(bytes_moved=mv["bytes_moved"], direct=mv["direct"], bounced=mv["bounced"],
                         moved_GBps_whole_call=round(mv["bytes_moved"] / el / 1e9, 1),
                         r7_move_GBps=R7_MOVE_GBPS)
            out[case].setdefault(mode, []).append(r)
            log(n, case, mode, r)
        for mode in ("torch", "kernel"):
            out[case][f"{mode}_best_s"] = min(r["s"] for r in out[case][mode])
    res[f"index_{n}"] = out
    del idx
    torch.cuda.empty_cache()


def bench_graph(a, dev, res):
    from lazzaro_amd.engine import tenant_graph as TG
    N, D = a.graph_rows, a.graph_dim
    ids = [f"n{i}" for i in range(N)]
    g = TG.TenantGraph(device=dev, dim=D, capacity=N)
    g.ann_cfg = {"nlist": a.nlist, "nprobe": 32, "m": a.m, "min_rows": 1_000_000}
    code = g.shard_id("default")
    gen = torch.Generator(device=dev).manual_seed(3)
    C = torch.nn.functional.normalize(torch.randn(4096, D, device=dev, generator=gen), dim=1)
    t0 = time.time()
    for c0 in range(0, N, 1 << 21):
        c1 = min(N, c0 + (1 << 21))
        X = C[torch.randint(0, 4096, (c1 - c0,), device=dev, generator=gen)] + 0.05 * torch.randn(
            c1 - c0, D, device=dev, generator=gen)
        X /= X.norm(dim=1, keepdim=True)
        g.add_nodes(ids[c0:c1], [""] * (c1 - c0), X, shard=code, stored=True, want_rows=False)
        del X
    g.clear_tracking()
    log(f"graph built in {time.time() - t0:.0f}s")
    Q = torch.nn.functional.normalize(C[:64] + 0.06 * torch.randn(64, D, device=dev, generator=gen), dim=1)
    t0 = time.perf_counter()
    g.store_search(Q, 10)
    torch.cuda.synchronize(dev)
    out = {"rows": N, "dim": D, "first_build_s": round(time.perf_counter() - t0, 3)}
    vic = np.sort(np.random.default_rng(3).choice(N, size=N // 100, replace=False))
    g.remove_nodes(vic.tolist(), drop_edges=False, unstore=True)
    g.take_deleted()
    t0 = time.perf_counter()
    c = g.compact()
    torch.cuda.synchronize(dev)
    out["compact_s"] = round(time.perf_counter() - t0, 3)
    out["reclaimed"] = c["reclaimed"]
    t0 = time.perf_counter()
    g.store_search(Q, 10)
    torch.cuda.synchronize(dev)
    out["first_search_maintained_s"] = round(time.perf_counter() - t0, 4)
    out["ann_rebuilds"], out["index_maint"] = g.ann_rebuilds, g._ann.last_maint
    t0 = time.perf_counter()
    g.store_search(Q, 10)
    torch.cuda.synchronize(dev)
    out["steady_search_s"] = round(time.perf_counter() - t0, 4)
    g._ann_stale = True  # what a compaction did before: the next search re-trains and re-encodes
    t0 = time.perf_counter()
    g.store_search(Q, 10)
    torch.cuda.synchronize(dev)
    out["first_search_rebuild_s"] = round(time.perf_counter() - t0, 3)
    log("graph", out)
    res["tenant_graph"] = out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="*", default=[10_000_000, 100_000_000])
    ap.add_argument("--m", type=int, default=64)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--runs", type=int, default=3)  # the first of each mode also warms up
    ap.add_argument("--graph-rows", type=int, default=10_000_000)
    ap.add_argument("--graph-dim", type=int, default=768)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = {"metric": "IVF-PQ maintenance in place", "m": a.m, "nlist": a.nlist}
    for n in a.rows:
        bench_index(a, dev, n, res)
    if a.graph_rows:
        bench_graph(a, dev, res)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
