"""Diversity-aware store search on one tenant (``TenantGraph.store_search(...,
diversity=)``, mmr.hip): ``--rows`` x ``--dim`` unit rows, ``limit = --k``.

For M in ``--batches`` and every pool size in ``--fetch``: ``--reps``
interleaved repetitions of a timed window each of

``none``    ``store_search(Q, k)``: the plain search, the reference point;
``pool``    ``store_search(Q, fetch_k)`` alone: what a pool above the 16
            candidate slots costs before any selection;
``mmr``     ``store_search(Q, k, diversity=, fetch_k=)``: pool + selection +
            the gathers;

and the selection kernel's own time from HIP events (``mmr_select`` over the
pool's rows), beside its traffic model: (k - 1) rounds re-read the F pool rows
through L2, ``k * F * D * 4`` bytes per query.

The step runs in a child process under its own ``timeout``. Writes one JSON
file into ``--out`` and prints one JSON line."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def log(*a):
    print(f"[{time.strftime('%H:%M:%S')}]", *a, file=sys.stderr, flush=True)


def build(a):
    import torch

    from lazzaro_amd.engine import tenant_graph as TG
    dev = torch.device("cuda")
    N, D = a.rows, a.dim
    g = TG.TenantGraph(device=dev, dim=D, capacity=N)
    code = g.shard_id("default")
    gen = torch.Generator(device=dev).manual_seed(3)
    chunk = 1 << 19
    for c0 in range(0, N, chunk):
        c1 = min(N, c0 + chunk)
        X = torch.randn(c1 - c0, D, device=dev, generator=gen)
        X /= X.norm(dim=1, keepdim=True)
        g.add_nodes([f"n{i}" for i in range(c0, c1)], [""] * (c1 - c0), X, shard=code, stored=True, want_rows=False)
        del X
    g.clear_tracking()
    Q = torch.randn(max(a.batches), D, device=dev, generator=gen)
    Q /= Q.norm(dim=1, keepdim=True)
    torch.cuda.synchronize()
    assert g.unit_rows()
    return g, Q


def window(fn, budget_s=0.25, min_iters=3, max_iters=200):
    """ms per call over one timed window ending in a device synchronise."""
    import torch
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    one = time.perf_counter() - t0
    iters = max(min_iters, min(max_iters, int(budget_s / max(one, 1e-6))))
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def event_ms(fn, iters=20):
    """ms per call between two HIP events around ``iters`` back-to-back calls."""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def summary(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
            "reps_ms": [round(x, 4) for x in v]}


def step_ab(a):
    from lazzaro_amd.ops.mmr_ops import mmr_select
    g, Q = build(a)
    out = {"step": "ab", "rows": a.rows, "dim": a.dim, "k": a.k, "metric": a.metric, "diversity": a.diversity,
           "reps": a.reps, "table": []}
    for M in a.batches:
        Qm = Q[:M].contiguous()
        for F in a.fetch:
            runs = {"none": lambda: g.store_search(Qm, a.k, a.metric),
                    "pool": lambda: g.store_search(Qm, F, a.metric),
                    "mmr": lambda: g.store_search(Qm, a.k, a.metric, diversity=a.diversity, fetch_k=F)}
            res = {}
            for r in runs:  # warm-up: code objects, the routes' workspaces
                res[r] = runs[r]()
                runs[r]()
            pool_rows = res["pool"][1]
            X = g.emb32[: g.n]
            kern = lambda: mmr_select(X, Qm, pool_rows, a.k, a.diversity)  # noqa: E731
            kern()
            t = {r: [] for r in runs}
            tk = []
            for _ in range(a.reps):
                for r in runs:  # interleaved
                    t[r].append(window(runs[r]))
                tk.append(event_ms(kern))
            moved = float((res["mmr"][1] != res["none"][1]).any(dim=1).float().mean())
            row = {"M": M, "fetch_k": F, **{r: summary(v) for r, v in t.items()}, "mmr_kernel": summary(tk),
                   "model_l2_bytes_per_query": a.k * F * a.dim * 4, "model_l2_bytes": M * a.k * F * a.dim * 4,
                   "share_of_queries_whose_result_changed": round(moved, 4)}
            row["mmr_minus_none_ms"] = round(row["mmr"]["median_ms"] - row["none"]["median_ms"], 4)
            row["mmr_minus_pool_ms"] = round(row["mmr"]["median_ms"] - row["pool"]["median_ms"], 4)
            row["kernel_l2_gbps"] = round(row["model_l2_bytes"] / (row["mmr_kernel"]["median_ms"] * 1e-3) / 1e9, 1)
            log(f"M={M} fetch_k={F}: none {row['none']['median_ms']} ms  pool {row['pool']['median_ms']} ms  mmr "
                f"{row['mmr']['median_ms']} ms  kernel {row['mmr_kernel']['median_ms']} ms "
                f"({row['kernel_l2_gbps']} GB/s of the model)")
            out["table"].append(row)
    out["counters"] = {"mmr_searches": g.mmr_searches}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 21)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--metric", default="l2")
    ap.add_argument("--diversity", type=float, default=0.5)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 1024])
    ap.add_argument("--fetch", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12", "mmr"))
    ap.add_argument("--step-timeout", type=int, default=420)
    ap.add_argument("--step", default="", help="(internal) run one step in this process")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    if a.step:
        res = {"ab": step_ab}[a.step](a)
        with open(os.path.join(a.out, f"{a.step}_{a.rows}x{a.dim}.json"), "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res))
        return 0
    base = [sys.executable, os.path.abspath(__file__), "--rows", str(a.rows), "--dim", str(a.dim), "--k", str(a.k),
            "--metric", a.metric, "--diversity", str(a.diversity), "--reps", str(a.reps), "--out", a.out,
            "--batches", *map(str, a.batches), "--fetch", *map(str, a.fetch)]
    for step in ("ab",):
        log("step", step)
        rc = subprocess.run(["timeout", "-k", "10", str(a.step_timeout)] + base + ["--step", step]).returncode
        if rc != 0:
            log(f"step {step} failed with exit status {rc}: stopping")
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
