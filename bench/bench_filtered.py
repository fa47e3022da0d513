"""Filtered store search on one tenant (``TenantGraph.store_search(..., where=)``,
filter.hip): ``--rows`` x ``--dim`` unit rows with synthetic metadata (a
uniform salience column: ``min_salience = 1 - s`` passes a scattered fraction
``s`` of the rows).

Steps, each a child process under its own ``timeout`` (the driver stops at the
first step that fails):

``ab``       for M in ``--batches`` and every selectivity in ``--sel``: the
             indexed scan (sparse route, FILTER_SPARSE_MAX_ROWS forced up)
             against the dense masked route (forced down) and ``where=None``,
             plans cached, ``--reps`` interleaved repetitions of a timed window
             each. Gives the crossover the constant is set from.
``passall``  a filter every row passes (plan cached, default routing) against
             ``where=None``: medians and the min-max spread of ``where=None``
             over the interleaved repetitions.

Writes one JSON file per step into ``--out`` and prints one JSON line."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEL = (1.0, 0.5, 0.1, 0.01, 0.001, 0.0001)


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
        g.add_nodes([f"n{i}" for i in range(c0, c1)], [""] * (c1 - c0), X, shard=code,
                    sal=torch.rand(c1 - c0, device=dev, generator=gen), stored=True, want_rows=False)
        del X
    g.clear_tracking()
    Q = torch.randn(max(a.batches), D, device=dev, generator=gen)
    Q /= Q.norm(dim=1, keepdim=True)
    torch.cuda.synchronize()
    assert g.unit_rows()
    return TG, g, Q


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


def summary(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
            "reps_ms": [round(x, 4) for x in v]}


def step_ab(a):
    from lazzaro_amd.core.filters import MemoryFilter
    TG, g, Q = build(a)
    out = {"step": "ab", "rows": a.rows, "dim": a.dim, "k": a.k, "metric": a.metric, "reps": a.reps, "table": []}
    for M in a.batches:
        Qm = Q[:M].contiguous()
        for s in a.sel:
            flt = MemoryFilter(min_salience=1.0 - s) if s < 1.0 else MemoryFilter()
            runs = {"sparse": lambda: g.store_search(Qm, a.k, a.metric, where=flt),
                    "dense": lambda: g.store_search(Qm, a.k, a.metric, where=flt),
                    "none": lambda: g.store_search(Qm, a.k, a.metric)}
            force = {"sparse": 1 << 40, "dense": -1, "none": 0}
            t = {r: [] for r in runs}
            rows = {}
            for r in runs:  # warm-up: code objects, the plan, the route's workspaces
                TG.FILTER_SPARSE_MAX_ROWS = force[r]
                rows[r] = runs[r]()[1]
                runs[r]()
            count = g._filter_plan(flt, a.metric == "l2").count
            same = bool((rows["sparse"] == rows["dense"]).all())
            for _ in range(a.reps):
                for r in runs:  # interleaved
                    TG.FILTER_SPARSE_MAX_ROWS = force[r]
                    t[r].append(window(runs[r]))
            row = {"M": M, "selectivity": s, "count": count, "sparse_equals_dense": same,
                   **{r: summary(v) for r, v in t.items()}}
            log(f"M={M} sel={s} count={count} sparse {row['sparse']['median_ms']} ms  dense "
                f"{row['dense']['median_ms']} ms  none {row['none']['median_ms']} ms  same={same}")
            out["table"].append(row)
    for M in a.batches:
        wins = [r["count"] for r in out["table"] if r["M"] == M and r["sparse"]["median_ms"] < r["dense"]["median_ms"]]
        out[f"largest_count_sparse_wins_M{M}"] = max(wins) if wins else 0
    out["counters"] = {"filtered_searches": g.filtered_searches, "filter_plans_built": g.filter_plans_built,
                       "filtered_sparse": g.filtered_sparse, "filtered_ann": g.filtered_ann}
    return out


def step_passall(a):
    from lazzaro_amd.core.filters import MemoryFilter
    TG, g, Q = build(a)
    flt = MemoryFilter()
    out = {"step": "passall", "rows": a.rows, "dim": a.dim, "k": a.k, "metric": a.metric, "reps": max(a.reps, 5),
           "sparse_max_row_reads": TG.FILTER_SPARSE_MAX_ROWS, "table": []}
    for M in a.batches:
        Qm = Q[:M].contiguous()
        runs = {"none": lambda: g.store_search(Qm, a.k, a.metric),
                "passall": lambda: g.store_search(Qm, a.k, a.metric, where=flt)}
        for r in runs:
            runs[r]()
            runs[r]()
        built = g.filter_plans_built
        t = {r: [] for r in runs}
        for _ in range(max(a.reps, 5)):
            for r in runs:
                t[r].append(window(runs[r]))
        assert g.filter_plans_built == built, "the pass-all plan was rebuilt inside the timed windows"
        row = {"M": M, **{r: summary(v) for r, v in t.items()}}
        row["none_spread_ms"] = round(row["none"]["max_ms"] - row["none"]["min_ms"], 4)
        row["passall_minus_none_ms"] = round(row["passall"]["median_ms"] - row["none"]["median_ms"], 4)
        log(f"M={M} none {row['none']['median_ms']} ms (spread {row['none_spread_ms']})  pass-all "
            f"{row['passall']['median_ms']} ms")
        out["table"].append(row)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 21)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--metric", default="l2")
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 1024])
    ap.add_argument("--sel", type=float, nargs="+", default=list(SEL))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r9", "filtered_search"))
    ap.add_argument("--step-timeout", type=int, default=420)
    ap.add_argument("--step", default="", help="(internal) run one step in this process")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    if a.step:
        res = {"ab": step_ab, "passall": step_passall}[a.step](a)
        with open(os.path.join(a.out, f"{a.step}_{a.rows}x{a.dim}.json"), "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res))
        return 0
    base = [sys.executable, os.path.abspath(__file__), "--rows", str(a.rows), "--dim", str(a.dim), "--k", str(a.k),
            "--metric", a.metric, "--reps", str(a.reps), "--out", a.out, "--batches", *map(str, a.batches),
            "--sel", *map(str, a.sel)]
    for step in ("ab", "passall"):
        log("step", step)
        rc = subprocess.run(["timeout", "-k", "10", str(a.step_timeout)] + base + ["--step", step]).returncode
        if rc != 0:
            log(f"step {step} failed with exit status {rc}: stopping")
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
