"""Wide store search on one tenant (``TenantGraph.wide_k``, widek.hip):
``--rows`` x ``--dim`` unit rows, L2.

For M in ``--batches`` and k in ``--ks``: ``--reps`` interleaved repetitions
of a timed window each of

``off``      ``store_search(Q, k)`` with ``wide_k`` off: today's route (the
             exact fp32 scan for k > 16) and the reference point of the cell;
``on``       the same call with ``wide_k`` on (the certified int8 route for
             16 < k <= 64; k <= 16 takes the same code either way);

and per M ``mmr_off`` / ``mmr_on``: ``store_search(Q, 10, diversity=0.5,
fetch_k=64)`` under both settings. Beside them, between HIP events, on the
lists of the last ``on`` search: ``lzk_cand_select_wide`` alone, and the masked
fallback launch when no query is flagged; read back after the timing: the mean
list length, the queries the search sent to the exact fallback, and the share
of result rows equal between the two arms.

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
    import torch

    from lazzaro_amd.ops import search as S
    g, Q = build(a)
    out = {"step": "ab", "rows": a.rows, "dim": a.dim, "metric": "l2", "reps": a.reps, "table": [], "mmr": []}

    def search(flag, Qm, k, **kw):
        g.wide_k = flag
        try:
            return g.store_search(Qm, k, "l2", **kw)
        finally:
            g.wide_k = False

    # the lists of the last wide search: (args of the select, the fallback flags)
    seen = {}
    inner = S._select_with_fallback_wide

    def spy(X16, Q16, k, bias, alpha, cnt, cs, ci, cap, need=None, ovf_sink=None):
        sink = []
        r = inner(X16, Q16, k, bias, alpha, cnt, cs, ci, cap, need=need, ovf_sink=sink)
        seen.update(X16=X16, Q16=Q16, k=k, bias=bias, alpha=alpha, cnt=cnt, cs=cs, ci=ci, cap=cap, need=need,
                    ovf=sink[0][0])
        return r
    S._select_with_fallback_wide = spy

    for M in a.batches:
        Qm = Q[:M].contiguous()
        for k in a.ks:
            runs = {"off": lambda: search(False, Qm, k), "on": lambda: search(True, Qm, k)}
            res = {}
            for r in runs:  # warm-up: code objects, the routes' workspaces
                res[r] = runs[r]()
                runs[r]()
            t = {r: [] for r in runs}
            for _ in range(a.reps):
                for r in runs:  # interleaved
                    t[r].append(window(runs[r]))
            row = {"M": M, "k": k, **{r: summary(v) for r, v in t.items()},
                   "share_of_rows_equal": round(float((res["on"][1] == res["off"][1]).float().mean()), 6)}
            row["speedup"] = round(row["off"]["median_ms"] / row["on"]["median_ms"], 2)
            if k > 16:
                seen.clear()
                n0 = g.wide_searches
                runs["on"]()
                assert g.wide_searches == n0 + 1 and seen, "the wide route was not taken"
                w = dict(seen)
                sel = lambda: S.cand_select_wide(w["cnt"], w["cs"], w["ci"], w["cap"], w["k"], need=w["need"])  # noqa: E731
                none = torch.zeros(M, dtype=torch.int32, device=Qm.device)
                o = (torch.empty((M, w["k"]), device=Qm.device), torch.empty((M, w["k"]), dtype=torch.long, device=Qm.device))
                fb = lambda: S._flat_topk_wide(w["X16"], w["Q16"], w["k"], w["bias"], w["alpha"], 0, None,  # noqa: E731
                                               q_active=none, out=o)
                sel(), fb()
                ts, tf = [], []
                for _ in range(a.reps):
                    ts.append(event_ms(sel))
                    tf.append(event_ms(fb))
                row["select_wide_kernel"] = summary(ts)
                row["masked_fallback_none_flagged"] = summary(tf)
                # read back after the timing
                row["list_cap"] = int(w["cap"])
                row["mean_list_length"] = round(float((w["cnt"] & 0x3FFFFFFF).float().mean()), 1)
                row["fallback_queries"] = int((w["ovf"] != 0).sum())
                row["sample_rank_j"] = S.wide_spec_j(w["k"], S.CAND_STRIDE)
            log(f"M={M} k={k}: off {row['off']['median_ms']} ms  on {row['on']['median_ms']} ms  x{row['speedup']}  "
                + (f"select {row['select_wide_kernel']['median_ms']} ms  idle fallback "
                   f"{row['masked_fallback_none_flagged']['median_ms']} ms  list {row['mean_list_length']}  "
                   f"fallback queries {row['fallback_queries']}" if k > 16 else ""))
            out["table"].append(row)
        runs = {"mmr_off": lambda: search(False, Qm, 10, diversity=0.5, fetch_k=64),
                "mmr_on": lambda: search(True, Qm, 10, diversity=0.5, fetch_k=64)}
        res = {}
        for r in runs:
            res[r] = runs[r]()
            runs[r]()
        t = {r: [] for r in runs}
        for _ in range(a.reps):
            for r in runs:
                t[r].append(window(runs[r]))
        row = {"M": M, "limit": 10, "fetch_k": 64, "diversity": 0.5, **{r: summary(v) for r, v in t.items()},
               "share_of_rows_equal": round(float((res["mmr_on"][1] == res["mmr_off"][1]).float().mean()), 6)}
        row["speedup"] = round(row["mmr_off"]["median_ms"] / row["mmr_on"]["median_ms"], 2)
        log(f"M={M} mmr: off {row['mmr_off']['median_ms']} ms  on {row['mmr_on']['median_ms']} ms  x{row['speedup']}")
        out["mmr"].append(row)
    out["counters"] = {"wide_searches": g.wide_searches, "mmr_searches": g.mmr_searches}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 21)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 1024])
    ap.add_argument("--ks", type=int, nargs="+", default=[16, 32, 64])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16", "wide_k"))
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
    base = [sys.executable, os.path.abspath(__file__), "--rows", str(a.rows), "--dim", str(a.dim), "--reps", str(a.reps),
            "--out", a.out, "--batches", *map(str, a.batches), "--ks", *map(str, a.ks)]
    for step in ("ab",):
        log("step", step)
        rc = subprocess.run(["timeout", "-k", "10", str(a.step_timeout)] + base + ["--step", step]).returncode
        if rc != 0:
            log(f"step {step} failed with exit status {rc}: stopping")
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
