"""Cross-encoder re-ranked store search on one tenant (``TenantGraph.
store_search(..., rerank=)``, crossenc.hip + the encoder kernels): ``--rows`` x
``--dim`` unit rows with bench_lexical.py's synthetic contents, L2, ``limit =
--k``, re-ranker ``--model`` (random-init), ``L = --doc-tokens``.

For every (M, pool) of ``--batches`` x ``--pools`` (a pool above 16 runs under
``wide_k``): ``--reps`` interleaved repetitions of a timed window each of

``none``    ``store_search(Q, k)``: the plain search, the reference point;
``pool``    ``store_search(Q, pool, node_rows=True)``: the first stage alone;
``rerank``  ``store_search(Q, k, rerank=pool, query_tokens=)``;

then, over the same pools, each stage alone between HIP events queued behind
device work, summed over the chunks of queries: ``lens``, ``embed``, ``layers``,
``pooler``, ``head`` -- with the packed token count T, the layers beside
``CrossEncoder.flops(T)`` and the embed kernel beside its byte model (per
token three bf16 table rows read and one written, ``8 H`` bytes, plus the
ids) against the float4 copy rate (``--copy-tbps``). Once per run: the first
build of the token column (one measurement) and an append of 1,024 rows (the
median of 3; host tokenisation and upload, wall clock).

``--compare-tree PATH`` instead measures ``none`` alone in this tree and in
another checkout of the project (built), in alternating child processes
(bench_lexical.py's step): what ``rerank=None`` costs against a tree without
the feature.

Every step runs in a child process under its own ``timeout``. Writes JSON
files into ``--out`` and prints one JSON line."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_lexical import build, compare, contents, event_ms, log, queries, step_none, summary, window  # noqa: E402


def step_ab(a):
    import torch

    from lazzaro_amd.models.cross_encoder import CE_TOKEN_BUDGET, CrossEncoder
    from lazzaro_amd.models.encoder import _to_dev
    from lazzaro_amd.ops import crossenc_ops as X
    from lazzaro_amd.ops import encoder_ops as E
    from lazzaro_amd.ops.crossenc_ops import as_query_tokens
    g, Q = build(a)
    n, dev = g.n, g.device
    ce = g.reranker = CrossEncoder(a.model, device=dev)
    g.rerank_doc_tokens = a.doc_tokens
    c, p = ce.cfg, ce.p
    H, L = c.hidden, a.doc_tokens
    out = {"step": "ab", "rows": a.rows, "dim": a.dim, "k": a.k, "metric": "l2", "model": c.name, "doc_tokens": L,
           "token_budget": CE_TOKEN_BUDGET, "reps": a.reps, "copy_tbps": a.copy_tbps, "table": []}
    t0 = time.perf_counter()
    col = g.token_column()
    torch.cuda.synchronize()
    out["token_column_first_build_s"] = round(time.perf_counter() - t0, 3)
    out["token_column_bytes"] = col.nbytes()
    out["mean_doc_tokens"] = round(float(col.dlen[:n].float().mean()), 2)
    log(f"token column: first build {out['token_column_first_build_s']} s, {out['token_column_bytes']} bytes, "
        f"mean dlen {out['mean_doc_tokens']}")
    cls_id, sep_id = ce.special_ids
    for M in a.batches:
        Qm = Q[:M].contiguous()
        qtok, qlen = as_query_tokens(queries(a, M), ce.tokenizer)
        for P in a.pools:
            g.wide_k = P > 16
            runs = {"none": lambda: g.store_search(Qm, a.k, "l2"),
                    "pool": lambda: g.store_search(Qm, P, "l2", True),
                    "rerank": lambda: g.store_search(Qm, a.k, "l2", rerank=P, query_tokens=(qtok, qlen))}
            for r in runs:  # warm-up: code objects, the routes' workspaces
                runs[r](), runs[r]()
            # the stages alone, chunk by chunk, over the pools the first stage returns
            _, pool = g.store_search(Qm, P, "l2", True)
            pool = pool.contiguous()
            qt_d, ql_d = _to_dev(torch.from_numpy(qtok), dev), _to_dev(torch.from_numpy(qlen), dev)
            chunks = ce.chunks(qlen, P, L)
            prep, T_all = [], 0
            for a0, b0 in chunks:
                r = pool[a0:b0]
                lens, cu, st = X.ce_lens(r, ql_d[a0:b0], col.dlen[:n], c.max_pos, L)
                T, S = st.cpu().tolist()
                x = X.ce_embed_ln(r, qt_d[a0:b0], ql_d[a0:b0], col.tok, col.dlen[:n], cu, T, c.max_pos, L, cls_id,
                                  sep_id, p["word"], p["pos"], p["type"], p["emb_g"], p["emb_b"], c.eps)
                hc = ce.layers(x, lens, cu, r.numel(), S)
                dense = E.linear(hc, p["pool_w"], p["pool_b"])
                prep.append((r, qt_d[a0:b0], ql_d[a0:b0], lens, cu, T, S, x, hc, dense))
                T_all += T

            def each(fn):
                return lambda: [fn(*q) for q in prep]
            stages = {
                "lens": each(lambda r, qt, ql, lens, cu, T, S, x, hc, dense: X.ce_lens(
                    r, ql, col.dlen[:n], c.max_pos, L)),
                "embed": each(lambda r, qt, ql, lens, cu, T, S, x, hc, dense: X.ce_embed_ln(
                    r, qt, ql, col.tok, col.dlen[:n], cu, T, c.max_pos, L, cls_id, sep_id, p["word"], p["pos"],
                    p["type"], p["emb_g"], p["emb_b"], c.eps)),
                "layers": each(lambda r, qt, ql, lens, cu, T, S, x, hc, dense: ce.layers(x, lens, cu, r.numel(), S)),
                "pooler": each(lambda r, qt, ql, lens, cu, T, S, x, hc, dense: E.linear(hc, p["pool_w"], p["pool_b"])),
                "head": each(lambda r, qt, ql, lens, cu, T, S, x, hc, dense: X.ce_head_select(
                    dense, r, p["cls_w"], p["cls_b"], a.k, n)),
            }
            t = {r: [] for r in runs}
            tk = {s: [] for s in stages}
            for _ in range(a.reps):
                for r in runs:  # interleaved
                    t[r].append(window(runs[r], min_iters=2))
                for s in stages:
                    tk[s].append(event_ms(stages[s], iters=3))
            row = {"M": M, "pool_size": P, "wide_k": bool(g.wide_k), "pairs": M * P, "chunks": len(chunks), "T": T_all,
                   "tokens_per_pair": round(T_all / (M * P), 2), **{r: summary(v) for r, v in t.items()},
                   **{s: summary(v) for s, v in tk.items()}}
            lm, em = row["layers"]["median_ms"], row["embed"]["median_ms"]
            row["layers_flops"] = ce.flops(T_all)
            row["layers_tflops"] = round(row["layers_flops"] / (lm * 1e-3) / 1e12, 2)
            row["embed_model_bytes"] = int(T_all * (8 * H + 4))
            row["embed_model_tbps"] = round(row["embed_model_bytes"] / (em * 1e-3) / 1e12, 3)
            row["embed_share_of_copy_rate"] = round(row["embed_model_tbps"] / a.copy_tbps, 3)
            row["rerank_minus_pool_ms"] = round(row["rerank"]["median_ms"] - row["pool"]["median_ms"], 4)
            log(f"M={M} P={P}: none {row['none']['median_ms']} ms  pool {row['pool']['median_ms']} ms  rerank "
                f"{row['rerank']['median_ms']} ms | T {T_all} lens {row['lens']['median_ms']} embed {em} "
                f"({row['embed_model_tbps']} TB/s) layers {lm} ({row['layers_tflops']} TFLOP/s) pooler "
                f"{row['pooler']['median_ms']} head {row['head']['median_ms']} ms")
            out["table"].append(row)
            del prep, stages
    g.wide_k = False
    # an append of 1,024 rows: the next re-ranked search tokenises and uploads them
    gen = torch.Generator(device=dev).manual_seed(5)
    app = []
    for i in range(3):
        Xn = torch.randn(1024, a.dim, device=dev, generator=gen)
        Xn /= Xn.norm(dim=1, keepdim=True)
        c0 = a.rows + 1024 * i
        g.add_nodes([f"a{j}" for j in range(c0, c0 + 1024)], contents(a, c0, c0 + 1024), Xn,
                    shard=g.shard_id("default"), stored=True, want_rows=False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        g.token_column()
        torch.cuda.synchronize()
        app.append((time.perf_counter() - t0) * 1e3)
    out["append_1024_rows"] = summary(app)
    out["counters"] = {"reranked_searches": g.reranked_searches, "rerank_pairs": g.rerank_pairs,
                       "token_column_builds": g.token_column_builds}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 21)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--vocab", type=int, default=50000)
    ap.add_argument("--model", default="minilm-l6")
    ap.add_argument("--doc-tokens", type=int, default=64)
    ap.add_argument("--copy-tbps", type=float, default=6.29, help="the float4 copy rate the model is set against")
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--pools", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r29", "rerank"))
    ap.add_argument("--step-timeout", type=int, default=900)
    ap.add_argument("--compare-tree", default="", help="another built checkout: measure rerank=None against it")
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
            "--model", a.model, "--doc-tokens", str(a.doc_tokens), "--batches", *map(str, a.batches),
            "--pools", *map(str, a.pools)]
    if a.compare_tree:
        return compare(a, base)
    log("step ab")
    rc = subprocess.run(["timeout", "-k", "10", str(a.step_timeout)] + base + ["--step", "ab"]).returncode
    if rc != 0:
        log(f"step ab failed with exit status {rc}: stopping")
    return rc


if __name__ == "__main__":
    sys.exit(main())
