"""Filtered search through a tenant's IVF-PQ index (``ann_cfg["filtered"]``,
ivfpq_filter.hip + the ``_f`` scans of ivfpq.hip) against the dense masked
route of the same build: ``--rows`` x ``--dim`` clustered unit rows with a
uniform salience column (``min_salience = 1 - s`` passes a scattered fraction
``s`` of the rows), L2, k = ``--k``.

For every batch size in ``--batches`` and passing fraction in ``--sel``:

* ``ann``    the filtered index route (forced: FILTER_ANN_MAX_SCALE raised, the
             indexed fp32 scan switched off);
* ``dense``  the dense masked scan (the switch off, the indexed scan off);
* ``sparse`` the indexed fp32 scan of the listed rows, where the default
             routing would take it (rows x query tiles <= FILTER_SPARSE_MAX_ROWS)

as medians of ``--reps`` interleaved repetitions of a timed window each, plans
and filtered lists cached; recall@k of ``ann`` and ``dense`` against the exact
fp64 filtered top-k (M = 1: ``--single`` queries searched one at a time); and
the time to build the filtered lists of the plan (IVFPQIndex.filter_rows).

Writes ``<out>/filtered_ivfpq_<rows>x<dim>.json`` and prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEL = (0.125, 0.25, 0.5, 1.0)


def log(*a):
    print(f"[{time.strftime('%H:%M:%S')}]", *a, file=sys.stderr, flush=True)


def build(a):
    import torch

    from lazzaro_amd.engine import tenant_graph as TG
    dev = torch.device("cuda")
    N, D = a.rows, a.dim
    g = TG.TenantGraph(device=dev, dim=D, capacity=N)
    g.ann_cfg = {"nlist": a.nlist, "nprobe": a.nprobe, "m": a.pq_m, "min_rows": min(1_000_000, N), "filtered": True}
    code = g.shard_id("default")
    gen = torch.Generator(device=dev).manual_seed(3)
    C = max(64, N // 512)
    cen = torch.nn.functional.normalize(torch.randn(C, D, device=dev, generator=gen), dim=1)
    chunk = 1 << 19
    for c0 in range(0, N, chunk):
        c1 = min(N, c0 + chunk)
        lab = torch.randint(0, C, (c1 - c0,), device=dev, generator=gen)
        X = cen[lab] + 0.5 * torch.randn(c1 - c0, D, device=dev, generator=gen) / D ** 0.5
        X /= X.norm(dim=1, keepdim=True)
        g.add_nodes([f"n{i}" for i in range(c0, c1)], [""] * (c1 - c0), X, shard=code,
                    sal=torch.rand(c1 - c0, device=dev, generator=gen), stored=True, want_rows=False)
        del X
    g.clear_tracking()
    nq = max(max(a.batches), a.single)
    src = torch.randint(0, N, (nq,), device=dev, generator=gen)
    Q = g.emb32[src] + 0.3 * torch.randn(nq, D, device=dev, generator=gen) / D ** 0.5
    Q /= Q.norm(dim=1, keepdim=True)
    torch.cuda.synchronize()
    assert g.unit_rows()
    return TG, g, Q.contiguous()


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


def truth_l2(g, Q, bias, k, chunk=1 << 17):
    """Exact fp64 top-k rows of 2 <q, x> - |x|^2 over the rows whose bias is
    finite (ties to the lower row)."""
    import torch
    n = g.n
    Q64 = Q.double()
    best_s = torch.full((Q.shape[0], 0), float("-inf"), dtype=torch.float64, device=Q.device)
    best_i = torch.zeros((Q.shape[0], 0), dtype=torch.long, device=Q.device)
    for c0 in range(0, n, chunk):
        c1 = min(n, c0 + chunk)
        X = g.emb32[c0:c1].double()
        s = 2.0 * (Q64 @ X.T) - (X * X).sum(1)[None, :]
        s = torch.where(torch.isneginf(bias[c0:c1])[None, :], torch.full_like(s, float("-inf")), s)
        ts, ti = torch.topk(s, min(k, c1 - c0), dim=1)
        cs, ci = torch.cat([best_s, ts], 1), torch.cat([best_i, ti + c0], 1)
        o = torch.sort(cs, dim=1, descending=True, stable=True).indices[:, :k]
        best_s, best_i = torch.gather(cs, 1, o), torch.gather(ci, 1, o)
    return best_i


def recall(found, truth):
    f, t = found.cpu().tolist(), truth.cpu().tolist()
    return round(sum(len(set(a) & set(b)) for a, b in zip(f, t)) / sum(len(b) for b in t), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 21)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 1024])
    ap.add_argument("--sel", type=float, nargs="+", default=list(SEL))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--single", type=int, default=64, help="queries searched one at a time for the M = 1 recall")
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--nprobe", type=int, default=32)
    ap.add_argument("--pq-m", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11", "filtered_ivfpq"))
    a = ap.parse_args()
    import torch

    from lazzaro_amd.core.filters import MemoryFilter
    from lazzaro_amd.index.ivfpq import filtered_nprobe
    os.makedirs(a.out, exist_ok=True)
    t0 = time.perf_counter()
    TG, g, Q = build(a)
    log(f"tenant {a.rows} x {a.dim} built in {time.perf_counter() - t0:.1f} s")
    t0 = time.perf_counter()
    g.store_search(Q[:1], a.k, "l2")  # builds the index
    torch.cuda.synchronize()
    idx = g._ann
    log(f"index nlist={idx.nlist} m={idx.m} built in {time.perf_counter() - t0:.1f} s")
    sparse_max, scale = TG.FILTER_SPARSE_MAX_ROWS, TG.FILTER_ANN_MAX_SCALE
    out = {"rows": a.rows, "dim": a.dim, "k": a.k, "metric": "l2", "reps": a.reps, "nlist": idx.nlist,
           "nprobe": a.nprobe, "m": idx.m, "rerank": 1024, "filter_ann_max_scale": scale,
           "filter_sparse_max_rows": sparse_max, "table": []}

    def route(r, fn):
        g.ann_cfg["filtered"] = r == "ann"
        TG.FILTER_ANN_MAX_SCALE = 1 << 30
        TG.FILTER_SPARSE_MAX_ROWS = sparse_max if r == "sparse" else -1
        try:
            return fn()
        finally:
            TG.FILTER_SPARSE_MAX_ROWS, TG.FILTER_ANN_MAX_SCALE = sparse_max, scale

    for s in a.sel:
        flt = MemoryFilter(min_salience=1.0 - s) if s < 1.0 else MemoryFilter()
        plan = g._filter_plan(flt, True)
        count = plan.count
        tr = truth_l2(g, Q, plan.bias, a.k)
        build_ms = summary([window(lambda: idx.filter_rows(plan.bias, max_rows=count, keep_mask=False))
                            for _ in range(a.reps)])
        for M in a.batches:
            Qm = Q[:M].contiguous()
            routes = ["ann", "dense"] + (["sparse"] if count * -(-M // 8) <= sparse_max else [])
            search = lambda: g.store_search(Qm, a.k, "l2", where=flt)  # noqa: E731
            rows = {}
            for r in routes:  # warm-up: code objects, the plan's lists, the route's workspaces
                rows[r] = route(r, search)[1]
                route(r, search)
            t = {r: [] for r in routes}
            for _ in range(a.reps):
                for r in routes:  # interleaved
                    t[r].append(route(r, lambda: window(search)))
            rec = {}
            for r in ("ann", "dense"):
                if M == 1:
                    got = torch.cat([route(r, lambda: g.store_search(Q[i:i + 1], a.k, "l2", where=flt))[1]
                                     for i in range(a.single)])
                    rec[r] = recall(got, tr[: a.single])
                else:
                    rec[r] = recall(rows[r], tr[:M])
            row = {"M": M, "fraction": s, "count": count, "scale": round(a.rows / max(count, 1), 3),
                   "nprobe": filtered_nprobe(a.nprobe, idx.nlist, g.n, count), "list_build": build_ms,
                   "recall_ann": rec["ann"], "recall_dense": rec["dense"], **{r: summary(v) for r, v in t.items()}}
            row["ann_over_dense"] = round(row["ann"]["median_ms"] / row["dense"]["median_ms"], 3)
            log(f"M={M} fraction={s} count={count} nprobe={row['nprobe']} ann {row['ann']['median_ms']} ms "
                f"(recall {rec['ann']})  dense {row['dense']['median_ms']} ms (recall {rec['dense']})"
                + (f"  sparse {row['sparse']['median_ms']} ms" if "sparse" in row else "")
                + f"  list build {build_ms['median_ms']} ms")
            out["table"].append(row)
    out["counters"] = {"filtered_searches": g.filtered_searches, "filter_plans_built": g.filter_plans_built,
                       "filtered_sparse": g.filtered_sparse, "filtered_ann": g.filtered_ann,
                       "ann_rebuilds": g.ann_rebuilds}
    with open(os.path.join(a.out, f"filtered_ivfpq_{a.rows}x{a.dim}.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
