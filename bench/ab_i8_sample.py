"""Interleaved A/B of the store search's threshold sample on the headline's
store search (10M x 768 random unit rows, 1024 random unit queries, k = 10,
L2): the bf16 lane kernel over emb16[::64] (search.I8_SAMPLE off) vs the int8
sample kernel over emb8 in place (on), 3 rounds x AB_REPS store searches each
in one process. Then, once each, the two sample calls alone (the kernels
without the rest of the search). Prints one JSON line per round and a final
one: per-round ms, medians, the off arm's max-min spread, whether the gain is
at least 2.5x that spread, whether both arms return identical rows and
scores, and each arm's queries sent to the exact fallback in its last search."""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ARMS = (("bf16_sample", False), ("i8_sample", True))


def main():
    from lazzaro_amd.engine.tenant_graph import TenantGraph
    from lazzaro_amd.ops import search as S

    dev = torch.device("cuda", 0)
    N, D, nq = int(os.environ.get("AB_ROWS", 10_000_000)), 768, int(os.environ.get("AB_Q", 1024))
    g = TenantGraph(device=dev)
    g._set_dim(D)
    g.reserve(N)
    gen = torch.Generator(device=dev).manual_seed(1)
    code = g.shard_id("work")
    for r0 in range(0, N, 1 << 20):
        r1 = min(N, r0 + (1 << 20))
        v = torch.randn(r1 - r0, D, device=dev, generator=gen)
        g.add_nodes([f"n{i}" for i in range(r0, r1)], [""] * (r1 - r0), v / v.norm(dim=1, keepdim=True),
                    shard=code, stored=True)
    Q = torch.randn(nq, D, device=dev, generator=gen)
    Q = Q / Q.norm(dim=1, keepdim=True)
    reps = int(os.environ.get("AB_REPS", "20"))
    out = {"rows": N, "queries": nq, "reps": reps, "rounds": []}
    res, fb = {}, {}
    try:
        for rnd in range(3):
            row = {}
            for name, on in ARMS:
                S.I8_SAMPLE = on
                for _ in range(2):
                    r = g.store_search(Q, 10, "l2")
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(reps):
                    r = g.store_search(Q, 10, "l2")
                torch.cuda.synchronize()
                row[name] = round((time.perf_counter() - t0) / reps * 1e3, 3)
                res[name] = r
            out["rounds"].append(row)
            print(json.dumps(row), flush=True)
        for name, on in ARMS:  # one untimed search per arm with the fallback count on
            S.I8_SAMPLE, S.SPEC_STATS = on, []
            g.store_search(Q, 10, "l2")
            fb[name] = int(sum(int(x) for x in S.SPEC_STATS))
    finally:
        S.I8_SAMPLE = True
        S.SPEC_STATS = None
    a, b = res["bf16_sample"], res["i8_sample"]
    out["same_rows"] = bool(torch.equal(a[1], b[1]))
    out["same_scores"] = bool(torch.equal(a[0], b[0]))
    out["fallback_queries"] = fb
    for k, _ in ARMS:
        ms = [r[k] for r in out["rounds"]]
        out[k + "_ms_min"] = min(ms)
        out[k + "_ms_median"] = statistics.median(ms)
        out[k + "_ms_spread"] = round(max(ms) - min(ms), 3)
    out["gain_ms"] = round(out["bf16_sample_ms_median"] - out["i8_sample_ms_median"], 3)
    out["gain_over_off_spread"] = round(out["gain_ms"] / max(out["bf16_sample_ms_spread"], 1e-3), 2)
    out["gain_counts"] = bool(out["gain_ms"] >= 2.5 * out["bf16_sample_ms_spread"])

    # the two sample calls alone
    bias = g.store_bias("l2")
    q16 = g._q16(Q)
    q8, qs = S.quantize_i8_rows(q16)

    def timed(fn):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return round((time.perf_counter() - t0) / reps * 1e3, 3)

    bs = bias[:N:64].contiguous()
    out["sample_alone_ms"] = {
        "bf16_lane": timed(lambda: S._flat_topk_lane(g.emb16[:N:64], q16, 16, 16, bs, None, None, 2.0, 0, None)),
        "i8": timed(lambda: S.sample_topk_i8(g.emb8[:N], g.rs8, q8, qs, 16, 64, bias=bias, alpha=2.0)),
    }
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
