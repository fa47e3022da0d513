"""Interleaved A/B of the int8 scan's candidate epilogue on the headline's
store search (10M x 768 random unit rows, 1024 random unit queries, k = 10,
L2): OPT 24 (every int32 sum converted to float, then the float column
prefilter) vs OPT 88 (bit 6: the tiered prefilter on the int32 sums -- a quad
bound per accumulator register group, scores only for quads that clear the
threshold), 3 rounds x AB_REPS store searches each in one process. Then, once
each, the raw scan kernel (lzk_flat_cand_i8 alone): the GEMM without the
epilogue (OPT 28), both epilogues with every threshold at +inf (no candidate
passes) and at the 1/64 sample's k-th best (the store search's regime).
Prints one JSON line per round and a final one: per-round ms, medians, the
float epilogue's spread and whether both return identical rows and scores."""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VARIANTS = (("float_prefilter", 24), ("tiered_prefilter", 88))


def main():
    from lazzaro_amd.engine.tenant_graph import TenantGraph
    from lazzaro_amd.ops import _lib
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
    L = _lib.lib()
    reps = int(os.environ.get("AB_REPS", "20"))
    out = {"rows": N, "queries": nq, "reps": reps, "rounds": []}
    res = {}
    for rnd in range(3):
        row = {}
        for name, opt in VARIANTS:
            L.lzk_set_i8_opt(opt)
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
    L.lzk_set_i8_opt(-1)
    a = res[VARIANTS[0][0]]
    out["same_rows"] = all(bool(torch.equal(a[1], res[k][1])) for k, _ in VARIANTS[1:])
    out["same_scores"] = all(bool(torch.equal(a[0], res[k][0])) for k, _ in VARIANTS[1:])
    for k, _ in VARIANTS:
        ms = [r[k] for r in out["rounds"]]
        out[k + "_ms_min"] = min(ms)
        out[k + "_ms_median"] = statistics.median(ms)
        out[k + "_ms_spread"] = round(max(ms) - min(ms), 3)
    out["gain_ms"] = round(out["float_prefilter_ms_median"] - out["tiered_prefilter_ms_median"], 3)
    out["gain_beats_spread"] = bool(out["gain_ms"] > out["float_prefilter_ms_spread"])

    # the raw scan kernel, once each: where the epilogue's time goes
    bias = g.store_bias("l2")
    q16 = g._q16(Q)
    q8, qs = S.quantize_i8_rows(q16)
    st = _lib.stream_ptr(dev)
    cap = 2048
    cnt, cs, ci = S._cand_lists(dev, nq, cap, 0)
    grid = L.lzk_cand_grid_f8(N, nq)
    bbuf, bcap, bcnt = S._blk_records(dev, grid, nq, 16, 64, 1)
    inf = torch.full((nq,), float("inf"), device=dev)
    kth = S._sample_threshold(g.emb16[:N], q16, 10, 16, bias, None, None, 2.0, 64).float().contiguous()

    def raw(opt, thr):
        L.lzk_set_i8_opt(opt)

        def run():
            _lib.check(L.lzk_flat_cand_i8(g.emb8.data_ptr(), g.emb8.stride(0), N, q8.data_ptr(), q8.stride(0), nq, D,
                                          bias.data_ptr(), g.rs8.data_ptr(), qs.data_ptr(), 2.0, thr.data_ptr(), cap,
                                          cnt.data_ptr(), cs.data_ptr(), ci.data_ptr(), bbuf.data_ptr(), bcap,
                                          bcnt.data_ptr(), st), "lzk_flat_cand_i8")
        for _ in range(2):
            run()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            run()
        torch.cuda.synchronize()
        ms = round((time.perf_counter() - t0) / reps * 1e3, 3)
        return ms, int(bcnt.sum())

    probes = {}
    probes["gemm_only"] = raw(28, inf)[0]
    for name, opt in VARIANTS:
        probes[name + "_thr_inf"] = raw(opt, inf)[0]
        ms, n = raw(opt, kth)
        probes[name + "_thr_sample_kth"] = ms
        probes[name + "_records"] = n
    L.lzk_set_i8_opt(-1)
    out["raw_scan_ms"] = probes
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
