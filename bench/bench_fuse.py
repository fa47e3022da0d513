"""Multi-query store search on one tenant (``TenantGraph.store_search_fused``,
fuse.hip): ``--rows`` x ``--dim`` unit rows, L2, ``limit = --k``.

A cell is (NG groups, G sub-queries each, pool, mode). A group's sub-queries
are ``unit(base + sigma * noise / sqrt(dim))`` around a random unit base, so
their pools overlap in part. Per cell, ``--reps`` interleaved repetitions of a
timed window each of

``plain``   ``store_search(Q, pool, node_rows=True)`` of the same ``M = NG * G``
            queries: the pool search, code the feature does not touch -- the
            reference point of the row, measured in the same run;
``fused``   ``store_search_fused(Q, offsets, k, fuse=)``: pools + fusion;

and the fusion kernel's own time from HIP events (``fuse_select`` over the
pools), beside the mean candidate count and -- ``mean`` -- the traffic model:
every candidate row gathered once through L2, ``ncand * D * 4`` bytes per
group. The ``--wide`` cells run at ``pool = 64`` with ``wide_k`` on.

Every step runs in a child process under its own ``timeout``. Writes JSON files
into ``--out`` and prints one JSON line per step."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COPY_GBPS = 6290.0  # the float4-copy rate the traffic model is set against


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
    torch.cuda.synchronize()
    assert g.unit_rows()
    return g, gen


def queries(gen, NG, G, D, sigma, dev):
    import torch
    base = torch.randn(NG, 1, D, device=dev, generator=gen)
    base /= base.norm(dim=2, keepdim=True)
    q = base + sigma * torch.randn(NG, G, D, device=dev, generator=gen) / D ** 0.5
    q /= q.norm(dim=2, keepdim=True)
    return q.reshape(NG * G, D).contiguous()


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


_hold = None


def event_ms(fn, iters=20):
    """ms per call between two HIP events around ``iters`` back-to-back calls.
    A product of two 8,192 x 8,192 matrices is enqueued first, so the calls
    queue up behind it and the events span the device's work, not the pace at
    which Python issues launches (about 35 us each, above the rrf kernel)."""
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


def summary(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
            "reps_ms": [round(x, 4) for x in v]}


def step_ab(a):
    import numpy as np
    import torch

    from lazzaro_amd.core.fuse import QueryFusion
    from lazzaro_amd.ops.fuse_ops import launch
    g, gen = build(a)
    out = {"step": "ab", "rows": a.rows, "dim": a.dim, "k": a.k, "metric": a.metric, "sigma": a.sigma, "reps": a.reps,
           "table": []}
    X = g.emb32[: g.n]
    cells = [(ng, gs, a.pool, False) for ng, gs in a.cells] + [(ng, gs, 64, True) for ng, gs in a.wide]
    for NG, G, pool, wide in cells:
        g.wide_k = wide
        Q = queries(gen, NG, G, a.dim, a.sigma, X.device)
        off = np.arange(NG + 1, dtype=np.int64) * G
        plain = lambda: g.store_search(Q, pool, a.metric, node_rows=True)  # noqa: E731
        pools = plain()[1]
        plain()
        for mode in (("rrf",) if wide else ("rrf", "mean")):
            fu = QueryFusion(mode=mode, pool=pool)
            fused = lambda: g.store_search_fused(Q, off, a.k, a.metric, fu)  # noqa: E731
            mean = mode == "mean"
            w_d = torch.full((NG * G,), float(np.float32(1.0 / G)) if mean else 1.0, device=X.device)
            off_d = torch.from_numpy(off).to(X.device)
            pc = pools.contiguous()
            kern = lambda: launch(X if mean else None, Q if mean else None, off_d, G, pc, w_d, fu, a.k, g.n)  # noqa: E731
            fused(), fused()
            nc = kern()[3]
            ncand = float(nc.double().mean())
            runs = {"plain": plain, "fused": fused}
            t = {r: [] for r in runs}
            tk = []
            for _ in range(a.reps):
                for r in runs:  # interleaved
                    t[r].append(window(runs[r]))
                tk.append(event_ms(kern))
            row = {"NG": NG, "G": G, "M": NG * G, "pool": pool, "wide_k": wide, "mode": mode,
                   **{r: summary(v) for r, v in t.items()}, "fuse_kernel": summary(tk), "mean_ncand": round(ncand, 2),
                   "min_ncand": int(nc.min()), "max_ncand": int(nc.max())}
            row["fused_minus_plain_ms"] = round(row["fused"]["median_ms"] - row["plain"]["median_ms"], 4)
            row["kernel_share_of_the_difference"] = round(row["fuse_kernel"]["median_ms"] /
                                                          max(row["fused_minus_plain_ms"], 1e-9), 3)
            if mode == "mean":
                row["model_l2_bytes_per_group"] = int(ncand * a.dim * 4)
                row["model_l2_bytes"] = int(NG * ncand * a.dim * 4)
                if NG > 1:  # (a single group is one block through dependent phases: latency, not a rate)
                    gbps = row["model_l2_bytes"] / (row["fuse_kernel"]["median_ms"] * 1e-3) / 1e9
                    row["kernel_l2_gbps"] = round(gbps, 1)
                    row["share_of_copy_rate"] = round(gbps / COPY_GBPS, 4)
            log(f"NG={NG} G={G} pool={pool} {mode}: plain {row['plain']['median_ms']} ms  fused "
                f"{row['fused']['median_ms']} ms  kernel {row['fuse_kernel']['median_ms']} ms  ncand {row['mean_ncand']}")
            out["table"].append(row)
    g.wide_k = False
    out["counters"] = {"fused_searches": g.fused_searches, "fused_groups": g.fused_groups,
                       "wide_searches": g.wide_searches}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 21)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--pool", type=int, default=16)
    ap.add_argument("--sigma", type=float, default=0.35)
    ap.add_argument("--metric", default="l2")
    ap.add_argument("--cells", nargs="+", default=["1,4", "1,16", "128,8", "64,16"], help="NG,G pairs at --pool")
    ap.add_argument("--wide", nargs="*", default=["1,4", "128,8"], help="NG,G pairs at pool = 64 with wide_k on (rrf)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19", "fuse"))
    ap.add_argument("--step-timeout", type=int, default=420)
    ap.add_argument("--step", default="", help="(internal) run one step in this process")
    a = ap.parse_args()
    pairs = lambda v: [tuple(int(x) for x in s.split(",")) for s in v]  # noqa: E731
    a.cells, a.wide = pairs(a.cells), pairs(a.wide)
    os.makedirs(a.out, exist_ok=True)
    if a.step:
        sys.path.insert(0, ROOT)
        res = step_ab(a)
        with open(os.path.join(a.out, f"ab_{a.rows}x{a.dim}.json"), "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res))
        return 0
    base = [sys.executable, os.path.abspath(__file__), "--rows", str(a.rows), "--dim", str(a.dim), "--k", str(a.k),
            "--pool", str(a.pool), "--sigma", str(a.sigma), "--metric", a.metric, "--reps", str(a.reps), "--out", a.out,
            "--cells", *(f"{x},{y}" for x, y in a.cells), "--wide", *(f"{x},{y}" for x, y in a.wide)]
    log("step ab")
    rc = subprocess.run(["timeout", "-k", "10", str(a.step_timeout)] + base + ["--step", "ab"]).returncode
    if rc != 0:
        log(f"step ab failed with exit status {rc}: stopping")
    return rc


if __name__ == "__main__":
    sys.exit(main())
