"""Keyword and hybrid store search on one tenant (``TenantGraph.store_search(
..., lexical=)``, lexical.hip): ``--rows`` x ``--dim`` unit rows with
synthetic contents -- 8 to 24 words drawn from a Zipf vocabulary of
``--vocab`` words plus two unique tokens per row -- L2, ``limit = --k``,
``pool`` 16.

For M in ``--batches``: ``--reps`` interleaved repetitions of a timed window
each of

``none``         ``store_search(Q, k)``: the plain search, the reference point;
``lexical_leg``  ``lexical_topk(terms, 16)``: the BM25 leg alone (tables, scan, merge);
``lexical_0.3``  ``store_search(Q, k, lexical=0.3, query_terms=)``;
``lexical_1.0``  the same at alpha 1: no dense search;

then ``lex_scan`` (the scan kernel), ``lex_merge`` (the merge of its partial
lists) and ``lex_fuse``, each alone between HIP events, the scan beside its
traffic model of ``n * (4 W + 4)`` bytes per tile of 8 queries and that
model's rate against the float4 copy rate (``--copy-tbps``); once per run: the first build of the lexicon (one
measurement) and an append of 1,024 rows (the median of 3; host tokenisation,
upload and the df merge, wall clock).

``--compare-tree PATH`` instead measures ``none`` alone in this tree and in
another checkout of the project (built), in alternating child processes: what
``lexical=None`` costs against a tree without the feature.

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


def log(*a):
    print(f"[{time.strftime('%H:%M:%S')}]", *a, file=sys.stderr, flush=True)


def contents(a, lo, hi):
    """Texts of rows [lo, hi): a pool of 65,536 Zipf-drawn word lists, row r
    taking entry r mod 65,536 plus its own two tokens."""
    import numpy as np
    pool = getattr(contents, "pool", None)
    if pool is None:
        rng = np.random.default_rng(17)
        p = 1.0 / np.arange(1, a.vocab + 1)
        p /= p.sum()
        lens = rng.integers(8, 25, size=1 << 16)
        draws = rng.choice(a.vocab, size=int(lens.sum()), p=p)
        words = [f"w{i}" for i in range(a.vocab)]
        pool, at = [], 0
        for n in lens:
            pool.append(" ".join(words[i] for i in draws[at:at + n]))
            at += n
        contents.pool = pool
    return [f"{pool[r & 0xFFFF]} u{r} t{r * 7 + 1}" for r in range(lo, hi)]


def queries(a, M):
    """M query texts: three Zipf words and, for every other query, a row's unique token."""
    import numpy as np
    rng = np.random.default_rng(23)
    p = 1.0 / np.arange(1, a.vocab + 1)
    p /= p.sum()
    d = rng.choice(a.vocab, size=(M, 3), p=p)
    rows = rng.integers(0, a.rows, size=M)
    return [f"w{x} w{y} w{z}" + (f" u{r}" if m % 2 == 0 else "") for m, ((x, y, z), r) in enumerate(zip(d, rows))]


def build(a, texts=True):
    import torch

    from lazzaro_amd.engine import tenant_graph as TG
    dev = torch.device("cuda")
    N, D = a.rows, a.dim
    g = TG.TenantGraph(device=dev, dim=D, capacity=N + 2048)
    code = g.shard_id("default")
    gen = torch.Generator(device=dev).manual_seed(3)
    chunk = 1 << 19
    for c0 in range(0, N, chunk):
        c1 = min(N, c0 + chunk)
        X = torch.randn(c1 - c0, D, device=dev, generator=gen)
        X /= X.norm(dim=1, keepdim=True)
        g.add_nodes([f"n{i}" for i in range(c0, c1)], contents(a, c0, c1) if texts else [""] * (c1 - c0), X,
                    shard=code, stored=True, want_rows=False)
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


def event_ms(fn, iters=10):
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
    import numpy as np
    import torch

    from lazzaro_amd.core.lexical import LexicalSearch, query_terms
    from lazzaro_amd.ops import _lib
    from lazzaro_amd.ops.lex_ops import _check_terms, lex_fuse, tile_tables
    from lazzaro_amd.ops.search import cand_select_wide
    g, Q = build(a)
    n, dev = g.n, g.device
    out = {"step": "ab", "rows": a.rows, "dim": a.dim, "k": a.k, "metric": "l2", "pool": 16, "vocab": a.vocab,
           "reps": a.reps, "copy_tbps": a.copy_tbps, "table": []}
    t0 = time.perf_counter()
    lx = g.lexicon()
    torch.cuda.synchronize()
    out["lexicon_first_build_s"] = round(time.perf_counter() - t0, 3)
    W = lx.W
    out.update(slots=W, lexicon_bytes=int(n * (4 * W + 4)), distinct_terms=int(len(lx.df_terms)), N=lx.N,
               avgdl=round(lx.avgdl, 3))
    log(f"lexicon: first build {out['lexicon_first_build_s']} s, {out['distinct_terms']} terms, avgdl {out['avgdl']}")
    bias = g._lex_bias("l2", None)
    L = _lib.lib()
    for M in a.batches:
        Qm = Q[:M].contiguous()
        texts = queries(a, M)
        qt = query_terms(texts)
        w = lx.weights(qt)
        l03, l10 = LexicalSearch(alpha=0.3), LexicalSearch(alpha=1.0)
        runs = {"none": lambda: g.store_search(Qm, a.k, "l2"),
                "lexical_leg": lambda: g.lexical_topk(qt, 16),
                "lexical_0.3": lambda: g.store_search(Qm, a.k, "l2", lexical=l03, query_terms=qt),
                "lexical_1.0": lambda: g.store_search(Qm, a.k, "l2", lexical=l10, query_terms=qt)}
        res = {}
        for r in runs:  # warm-up: code objects, the routes' workspaces
            res[r] = runs[r]()
            runs[r]()
        # the kernels alone: tables uploaded once
        utab, uw = tile_tables(*_check_terms(qt, w))
        utab_d, uw_d = torch.from_numpy(utab.view(np.int32)).to(dev), torch.from_numpy(uw).to(dev)
        nblk = int(L.lzk_lex_scan_blocks(n, M, 0))
        ps = torch.empty((M, nblk * 64), dtype=torch.float32, device=dev)
        pi = torch.empty((M, nblk * 64), dtype=torch.int32, device=dev)
        sl, dl = lx.slots[:n], lx.dl[:n]

        def scan():
            _lib.check(L.lzk_lex_scan(sl.data_ptr(), dl.data_ptr(), bias.data_ptr(), n, W, utab_d.data_ptr(),
                                      uw_d.data_ptr(), M, 1.2, 0.75, lx.avgdl, nblk, ps.data_ptr(), pi.data_ptr(),
                                      _lib.stream_ptr(dev)), "lzk_lex_scan")

        def merge():
            return cand_select_wide(None, ps, pi, nblk * 64, 16)
        scan()
        _, lp, _ = merge()
        _, dp = g.store_search(Qm, 16, "l2", True)
        fuse = lambda: lex_fuse(g.emb32[:n], Qm, dp, lp, lx.slots, lx.dl, qt, w, 0.3, a.k, 1.2, 0.75, lx.avgdl)  # noqa: E731
        fuse()
        t = {r: [] for r in runs}
        tk = {"lex_scan": [], "lex_merge": [], "lex_fuse": []}
        for _ in range(a.reps):
            for r in runs:  # interleaved
                t[r].append(window(runs[r]))
            tk["lex_scan"].append(event_ms(scan))
            tk["lex_merge"].append(event_ms(merge))
            tk["lex_fuse"].append(event_ms(fuse))
        found = float((res["lexical_1.0"][1][::2, 0] >= 0).float().mean())
        row = {"M": M, "scan_row_blocks": nblk, **{r: summary(v) for r, v in t.items()},
               **{r: summary(v) for r, v in tk.items()}, "share_of_token_queries_with_a_match": round(found, 4)}
        tiles = -(-M // 8)
        sm = row["lex_scan"]["median_ms"]
        row["scan_model_bytes"] = int(tiles * n * (4 * W + 4))
        row["scan_model_tbps"] = round(row["scan_model_bytes"] / (sm * 1e-3) / 1e12, 3)
        row["scan_share_of_copy_rate"] = round(row["scan_model_tbps"] / a.copy_tbps, 3)
        for r in ("lexical_leg", "lexical_0.3", "lexical_1.0"):
            row[f"{r}_over_none"] = round(row[r]["median_ms"] / row["none"]["median_ms"], 3)
        log(f"M={M}: none {row['none']['median_ms']} ms  leg {row['lexical_leg']['median_ms']} ms  0.3 "
            f"{row['lexical_0.3']['median_ms']} ms  1.0 {row['lexical_1.0']['median_ms']} ms  scan {sm} ms "
            f"({row['scan_model_tbps']} TB/s of the model)  merge {row['lex_merge']['median_ms']} ms  fuse "
            f"{row['lex_fuse']['median_ms']} ms")
        out["table"].append(row)
    # an append of 1,024 rows: the next lexical use tokenises and uploads them
    gen = torch.Generator(device=dev).manual_seed(5)
    app = []
    for i in range(3):
        X = torch.randn(1024, a.dim, device=dev, generator=gen)
        X /= X.norm(dim=1, keepdim=True)
        c0 = a.rows + 1024 * i
        g.add_nodes([f"a{j}" for j in range(c0, c0 + 1024)], contents(a, c0, c0 + 1024), X,
                    shard=g.shard_id("default"), stored=True, want_rows=False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        g.lexicon()
        torch.cuda.synchronize()
        app.append((time.perf_counter() - t0) * 1e3)
    out["append_1024_rows"] = summary(app)
    out["counters"] = {"lexical_searches": g.lexical_searches, "lexicon_builds": g._lexicon.builds,
                       "lexicon_rows": g._lexicon.covered}
    return out


def step_none(a):
    """``store_search(Q, k)`` alone, in whichever tree ``--tree`` names."""
    g, Q = build(a, texts=False)
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
    ap.add_argument("--vocab", type=int, default=50000)
    ap.add_argument("--copy-tbps", type=float, default=6.29, help="the float4 copy rate the model is set against")
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 1024])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17", "lexical"))
    ap.add_argument("--step-timeout", type=int, default=420)
    ap.add_argument("--compare-tree", default="", help="another built checkout: measure lexical=None against it")
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
            with open(os.path.join(a.out, f"{a.step}_{a.rows}x{a.dim}.json"), "w") as f:
                json.dump(res, f, indent=1)
        print(json.dumps(res))
        return 0
    base = [sys.executable, os.path.abspath(__file__), "--rows", str(a.rows), "--dim", str(a.dim), "--k", str(a.k),
            "--vocab", str(a.vocab), "--copy-tbps", str(a.copy_tbps), "--reps", str(a.reps), "--out", a.out,
            "--batches", *map(str, a.batches)]
    if a.compare_tree:
        return compare(a, base)
    log("step ab")
    rc = subprocess.run(["timeout", "-k", "10", str(a.step_timeout)] + base + ["--step", "ab"]).returncode
    if rc != 0:
        log(f"step ab failed with exit status {rc}: stopping")
    return rc


if __name__ == "__main__":
    sys.exit(main())
