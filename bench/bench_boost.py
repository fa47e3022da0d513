"""Boosted store search on one tenant (``TenantGraph.store_search(...,
boost=)``, boost.hip): ``--rows`` x ``--dim`` unit rows, L2, ``limit = --k``.

For M in ``--batches``: ``--reps`` interleaved repetitions of a timed window
each of

``none``         ``store_search(Q, k)``: the plain search, the reference point;
``boost_cached`` ``store_search(Q, k, boost=)`` with a fixed ``now``: the
                 column comes from the cache, the scan runs under it;
``boost_fresh``  the same with a fresh ``now`` every call: one column built
                 per search;

the column kernel's own time between two HIP events beside its traffic model
(22 B read + 4 B written per row) and that model's rate against the float4
copy rate (``--copy-tbps``); and the int8 candidate stage
(``TenantGraph._i8_candidates``: query quantisation, scan, select and
certificate) between HIP events under the store bias and under the boosted
column -- the tiered prefilter bounds each 4-row quad by the quad's largest
bias, and neighbouring rows' priors differ.

``--step kernel`` (run it under a kernel trace) launches the column kernel
alone over ``--rows`` rows: aligned and with ``base`` one element into its
buffer, with and without the type table.

``--compare-tree PATH`` instead measures ``none`` alone in this tree and in
another checkout of the project (built), in alternating child processes: what
``boost=None`` costs against a tree without the feature.

Every step runs in a child process under its own ``timeout``. Writes JSON
files into ``--out`` and prints one JSON line."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOW = 1_700_000_000.0
BYTES_PER_ROW = 26


def log(*a):
    print(f"[{time.strftime('%H:%M:%S')}]", *a, file=sys.stderr, flush=True)


def build(a, meta=True):
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
        kw = {}
        if meta:  # salience U(0, 1), 0 .. 19 uses, last accessed within 30 days of NOW
            m = c1 - c0
            kw = dict(sal=torch.rand(m, device=dev, generator=gen),
                      acc=torch.randint(0, 20, (m,), device=dev, generator=gen, dtype=torch.int32),
                      last=NOW - 30 * 86400.0 * torch.rand(m, device=dev, generator=gen, dtype=torch.float64))
        g.add_nodes([f"n{i}" for i in range(c0, c1)], [""] * (c1 - c0), X, shard=code, stored=True, want_rows=False,
                    **kw)
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


def event_ms(fn, iters=20, busy=None):
    """ms per call between two HIP events around ``iters`` back-to-back calls.
    ``busy``: device work enqueued before the first event, long enough for the
    host to enqueue all the calls behind it -- the events then bracket device
    time alone (a call whose kernel is shorter than its own enqueue would
    otherwise be timed at the host's rate)."""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if busy is not None:
        busy()
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

    from lazzaro_amd.core.boost import MemoryBoost
    from lazzaro_amd.ops.boost_ops import boost_bias
    g, Q = build(a)
    n = g.n
    b = MemoryBoost.coerce(a.boost).at(NOW)
    tick = [0]

    def fresh():
        tick[0] += 1
        return MemoryBoost(**dict(b.to_dict(), now=NOW + tick[0]))
    out = {"step": "ab", "rows": a.rows, "dim": a.dim, "k": a.k, "metric": "l2", "boost": b.to_dict(), "reps": a.reps,
           "model_bytes_per_row": BYTES_PER_ROW, "copy_tbps": a.copy_tbps, "table": []}
    base = g.store_bias("l2")
    kern = lambda: boost_bias(base, g.sal, g.acc, g.last, g.kind, n, b.salience, b.frequency, b.recency,  # noqa: E731
                              b.recency_scale, NOW, 2.0)
    col = kern()
    assert torch.equal(col, g.boost_bias(b, "l2"))
    A = torch.randn(8192, 8192, device=base.device)
    busy = lambda: torch.mm(A, A)  # noqa: E731  (several ms of device work: 20 launches queue up behind it)
    busy()
    for M in a.batches:
        Qm = Q[:M].contiguous()
        runs = {"none": lambda: g.store_search(Qm, a.k, "l2"),
                "boost_cached": lambda: g.store_search(Qm, a.k, "l2", boost=b),
                "boost_fresh": lambda: g.store_search(Qm, a.k, "l2", boost=fresh())}
        res = {}
        for r in runs:  # warm-up: code objects, the routes' workspaces
            res[r] = runs[r]()
            runs[r]()
        q16 = g._q16(Qm)
        scan = {"store_bias": lambda: g._i8_candidates(Qm, q16, 16, base, 2.0),
                "boosted_bias": lambda: g._i8_candidates(Qm, q16, 16, col, 2.0)}
        for s in scan.values():
            s()
        t = {r: [] for r in runs}
        tk, ts = [], {s: [] for s in scan}
        for _ in range(a.reps):
            for r in runs:  # interleaved
                t[r].append(window(runs[r]))
            tk.append(event_ms(kern, busy=busy))
            for s in scan:
                ts[s].append(event_ms(scan[s]))
        moved = float((res["boost_cached"][1] != res["none"][1]).any(dim=1).float().mean())
        row = {"M": M, **{r: summary(v) for r, v in t.items()}, "boost_kernel": summary(tk),
               "i8_candidates": {s: summary(v) for s, v in ts.items()},
               "share_of_queries_whose_result_changed": round(moved, 4)}
        km = row["boost_kernel"]["median_ms"]
        row["kernel_model_tbps"] = round(n * BYTES_PER_ROW / (km * 1e-3) / 1e12, 3)
        row["kernel_share_of_copy_rate"] = round(row["kernel_model_tbps"] / a.copy_tbps, 3)
        for r in ("boost_cached", "boost_fresh"):
            row[f"{r}_minus_none_ms"] = round(row[r]["median_ms"] - row["none"]["median_ms"], 4)
        row["fresh_minus_cached_ms"] = round(row["boost_fresh"]["median_ms"] - row["boost_cached"]["median_ms"], 4)
        row["fresh_minus_cached_minus_kernel_ms"] = round(row["fresh_minus_cached_ms"] - km, 4)
        row["i8_boosted_minus_store_ms"] = round(row["i8_candidates"]["boosted_bias"]["median_ms"]
                                                 - row["i8_candidates"]["store_bias"]["median_ms"], 4)
        log(f"M={M}: none {row['none']['median_ms']} ms  cached {row['boost_cached']['median_ms']} ms  fresh "
            f"{row['boost_fresh']['median_ms']} ms  kernel {km} ms ({row['kernel_model_tbps']} TB/s of the model)  "
            f"i8 stage {row['i8_candidates']['store_bias']['median_ms']} -> "
            f"{row['i8_candidates']['boosted_bias']['median_ms']} ms")
        out["table"].append(row)
    out["counters"] = {"boosted_searches": g.boosted_searches, "boost_columns_built": g.boost_columns_built}
    return out


def step_kernel(a):
    """The column kernel alone, 50 launches of each variant, for a kernel trace."""
    import torch

    from lazzaro_amd.ops.boost_ops import boost_bias
    dev = torch.device("cuda")
    n = a.rows
    gen = torch.Generator(device=dev).manual_seed(3)
    buf = -torch.rand(n + 1, device=dev, generator=gen)
    sal = torch.rand(n, device=dev, generator=gen)
    acc = torch.randint(0, 20, (n,), device=dev, generator=gen, dtype=torch.int32)
    last = NOW - 30 * 86400.0 * torch.rand(n, device=dev, generator=gen, dtype=torch.float64)
    kind = torch.ones(n, dtype=torch.uint8, device=dev)
    tcode = torch.randint(0, 4, (n,), device=dev, generator=gen, dtype=torch.uint8)
    tw = [0.1 * (i % 4) for i in range(256)]
    base = buf[:n].clone()
    for b_, types in ((base, False), (base, True), (buf[1:], False), (buf[1:], True)):
        for _ in range(50):
            boost_bias(b_, sal, acc, last, kind, n, 0.5, 0.3, 0.2, 86400.0, NOW, 2.0, tcode if types else None,
                       tw if types else None)
    torch.cuda.synchronize()
    return {"step": "kernel", "rows": n, "launches_per_variant": 50,
            "variants": ["aligned", "aligned+types", "offset", "offset+types"], "model_bytes_per_row": BYTES_PER_ROW}


def step_none(a):
    """``store_search(Q, k)`` alone, in whichever tree ``--tree`` names."""
    g, Q = build(a, meta=False)
    out = {"step": "none", "tree": a.tag, "rows": a.rows, "dim": a.dim, "k": a.k, "metric": "l2", "reps": a.reps,
           "table": []}
    for M in a.batches:
        Qm = Q[:M].contiguous()
        run = lambda: g.store_search(Qm, a.k, "l2")  # noqa: E731
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
    res = {"step": "compare", "rows": a.rows, "dim": a.dim, "k": a.k, "metric": "l2", "rounds": a.rounds,
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
    ap.add_argument("--boost", type=float, default=1.0, help="the float form: w x the reference's importance")
    ap.add_argument("--copy-tbps", type=float, default=6.29, help="the float4 copy rate the model is set against")
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 1024])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14", "boost"))
    ap.add_argument("--step-timeout", type=int, default=420)
    ap.add_argument("--compare-tree", default="", help="another built checkout: measure boost=None against it")
    ap.add_argument("--rounds", type=int, default=2, help="alternations of --compare-tree")
    ap.add_argument("--step", default="", help="(internal) run one step in this process")
    ap.add_argument("--tree", default=ROOT, help="(internal) the checkout whose package a step imports")
    ap.add_argument("--tag", default="this", help="(internal)")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    if a.step:
        sys.path.insert(0, a.tree)
        res = {"ab": step_ab, "none": step_none, "kernel": step_kernel}[a.step](a)
        if a.step == "ab":
            with open(os.path.join(a.out, f"{a.step}_{a.rows}x{a.dim}.json"), "w") as f:
                json.dump(res, f, indent=1)
        print(json.dumps(res))
        return 0
    base = [sys.executable, os.path.abspath(__file__), "--rows", str(a.rows), "--dim", str(a.dim), "--k", str(a.k),
            "--boost", str(a.boost), "--copy-tbps", str(a.copy_tbps), "--reps", str(a.reps), "--out", a.out,
            "--batches", *map(str, a.batches)]
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
