"""Associative store search on one tenant (``TenantGraph.store_search(...,
expand=)``, expand.hip): ``--rows`` x ``--dim`` unit rows, a synthetic graph of
``--deg`` arcs per node (rows * deg / 2 edges between uniformly random pairs,
w ~ U(0.05, 1), one shard), ``limit = --k``.

For M in ``--batches`` and every ``hops,fanout`` in ``--settings``: ``--reps``
interleaved repetitions of a timed window each of

``none``    ``store_search(Q, k)``: the plain search, the reference point;
``seed``    ``store_search(Q, seed_k, node_rows=True)`` alone: the seed search;
``expand``  ``store_search(Q, k, expand=)``: seeds + expansion, end to end;

and the expansion kernel's own time from HIP events (``expand_select`` over the
seed rows), beside its traffic model: the cosines of the candidates gathered
through L2, ``ncand * D * 4`` bytes per query with the measured mean ``ncand``.

``--compare-tree PATH`` instead measures ``none`` alone in this tree and in
another checkout of the project (built), in alternating child processes: what
``expand=None`` costs against a tree without the feature.

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


def log(*a):
    print(f"[{time.strftime('%H:%M:%S')}]", *a, file=sys.stderr, flush=True)


def build(a, edges=True):
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
    Q = torch.randn(max(a.batches), D, device=dev, generator=gen)
    Q /= Q.norm(dim=1, keepdim=True)
    if edges:
        ne = N * a.deg // 2
        src = torch.randint(0, N, (ne,), device=dev, generator=gen)
        dst = torch.randint(0, N, (ne,), device=dev, generator=gen)
        w = torch.rand(ne, device=dev, generator=gen) * 0.95 + 0.05
        g.append_edges(src.int(), dst.int(), w, torch.full((ne,), code, dtype=torch.int32, device=dev))
    g.clear_tracking()
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
    import torch

    from lazzaro_amd.core.expand import GraphExpand
    from lazzaro_amd.ops.expand_ops import expand_select
    g, Q = build(a)
    t0 = time.perf_counter()
    csr = g.csr()
    torch.cuda.synchronize()
    out = {"step": "ab", "rows": a.rows, "dim": a.dim, "k": a.k, "metric": a.metric, "deg": a.deg,
           "edges": g.num_edges, "arcs": int(csr[1].numel()), "csr_build_ms": round((time.perf_counter() - t0) * 1e3, 1),
           "reps": a.reps, "table": []}
    X = g.emb32[: g.n]
    bias = g.store_bias("l2" if a.metric == "l2" else "ip")
    for M in a.batches:
        Qm = Q[:M].contiguous()
        for hops, fanout in a.settings:
            sp = GraphExpand(hops=hops, fanout=fanout)
            runs = {"none": lambda: g.store_search(Qm, a.k, a.metric),
                    "seed": lambda: g.store_search(Qm, sp.seed_k, a.metric, node_rows=True),
                    "expand": lambda: g.store_search(Qm, a.k, a.metric, expand=sp)}
            res = {}
            for r in runs:  # warm-up: code objects, the routes' workspaces
                res[r] = runs[r]()
                runs[r]()
            seeds = res["seed"][1]
            kern = lambda: expand_select(X, Qm, seeds, csr, g.e["w"], g.kind, g.sup, bias, sp, a.k)  # noqa: E731
            ncand = float(kern()[3].float().mean())
            t = {r: [] for r in runs}
            tk = []
            for _ in range(a.reps):
                for r in runs:  # interleaved
                    t[r].append(window(runs[r]))
                tk.append(event_ms(kern))
            moved = float((res["expand"][1] != res["none"][1]).any(dim=1).float().mean())
            row = {"M": M, "hops": hops, "fanout": fanout, "seed_k": sp.seed_k,
                   **{r: summary(v) for r, v in t.items()}, "expand_kernel": summary(tk), "mean_ncand": round(ncand, 1),
                   "model_l2_bytes_per_query": int(ncand * a.dim * 4), "model_l2_bytes": int(M * ncand * a.dim * 4),
                   "share_of_queries_whose_result_changed": round(moved, 4)}
            row["expand_minus_none_ms"] = round(row["expand"]["median_ms"] - row["none"]["median_ms"], 4)
            row["expand_minus_seed_ms"] = round(row["expand"]["median_ms"] - row["seed"]["median_ms"], 4)
            row["kernel_l2_gbps"] = round(row["model_l2_bytes"] / (row["expand_kernel"]["median_ms"] * 1e-3) / 1e9, 1)
            log(f"M={M} hops={hops} fanout={fanout}: none {row['none']['median_ms']} ms  seed "
                f"{row['seed']['median_ms']} ms  expand {row['expand']['median_ms']} ms  kernel "
                f"{row['expand_kernel']['median_ms']} ms (ncand {row['mean_ncand']}, {row['kernel_l2_gbps']} GB/s of "
                "the model)")
            out["table"].append(row)
    out["counters"] = {"expanded_searches": g.expanded_searches}
    return out


def step_none(a):
    """``store_search(Q, k)`` alone, in whichever tree ``--tree`` names."""
    g, Q = build(a, edges=False)
    out = {"step": "none", "tree": a.tag, "rows": a.rows, "dim": a.dim, "k": a.k, "metric": a.metric, "reps": a.reps,
           "table": []}
    for M in a.batches:
        Qm = Q[:M].contiguous()
        run = lambda: g.store_search(Qm, a.k, a.metric)  # noqa: E731
        run(), run()
        row = {"M": M, "none": summary([window(run) for _ in range(a.reps)])}
        log(f"[{a.tag}] M={M}: none {row['none']}")
        out["table"].append(row)
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
    res = {"step": "compare", "rows": a.rows, "dim": a.dim, "k": a.k, "metric": a.metric, "rounds": a.rounds,
           "reps_per_round": a.reps, "table": []}
    for j, M in enumerate(a.batches):
        v = {tag: [x for r in runs[tag] for x in r["table"][j]["none"]["reps_ms"]] for tag in runs}
        row = {"M": M, "other": summary(v["other"]), "this": summary(v["this"])}
        row["this_minus_other_ms"] = round(row["this"]["median_ms"] - row["other"]["median_ms"], 4)
        row["other_spread_ms"] = round(row["other"]["max_ms"] - row["other"]["min_ms"], 4)
        row["within_the_other_trees_spread"] = abs(row["this_minus_other_ms"]) <= row["other_spread_ms"]
        res["table"].append(row)
    with open(os.path.join(a.out, f"none_vs_other_tree_{a.rows}x{a.dim}.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 21)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--deg", type=int, default=6)
    ap.add_argument("--metric", default="l2")
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 1024])
    ap.add_argument("--settings", nargs="+", default=["1,8", "2,7"], help="hops,fanout pairs")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13", "expand"))
    ap.add_argument("--step-timeout", type=int, default=420)
    ap.add_argument("--compare-tree", default="", help="another built checkout: measure expand=None against it")
    ap.add_argument("--rounds", type=int, default=2, help="alternations of --compare-tree")
    ap.add_argument("--step", default="", help="(internal) run one step in this process")
    ap.add_argument("--tree", default=ROOT, help="(internal) the checkout whose package a step imports")
    ap.add_argument("--tag", default="this", help="(internal)")
    a = ap.parse_args()
    a.settings = [tuple(int(x) for x in s.split(",")) if isinstance(s, str) else s for s in a.settings]
    os.makedirs(a.out, exist_ok=True)
    if a.step:
        sys.path.insert(0, a.tree)
        res = {"ab": step_ab, "none": step_none}[a.step](a)
        if a.step == "ab":
            with open(os.path.join(a.out, f"{a.step}_{a.rows}x{a.dim}.json"), "w") as f:
                json.dump(res, f, indent=1)
        print(json.dumps(res))
        return 0
    base = [sys.executable, os.path.abspath(__file__), "--rows", str(a.rows), "--dim", str(a.dim), "--k", str(a.k),
            "--deg", str(a.deg), "--metric", a.metric, "--reps", str(a.reps), "--out", a.out,
            "--batches", *map(str, a.batches), "--settings", *(f"{h},{f}" for h, f in a.settings)]
    if a.compare_tree:
        return compare(a, base)
    for step in ("ab",):
        log("step", step)
        rc = subprocess.run(["timeout", "-k", "10", str(a.step_timeout)] + base + ["--step", step]).returncode
        if rc != 0:
            log(f"step {step} failed with exit status {rc}: stopping")
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
