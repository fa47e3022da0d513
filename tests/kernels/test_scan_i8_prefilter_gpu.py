"""The int8 store scan's tiered integer prefilter (search256.hip, OPT bit 6,
``lzk_set_i8_opt(88)``) appends exactly the records of the float epilogue
(``lzk_set_i8_opt(24)``): ``lzk_flat_cand_i8`` + ``lzk_cand_gather`` called
directly on a CU budget of 4, so a few persistent blocks walk several tiles
each; partial last row tile, partial query tile, 1 / 3 / 6 K tiles.

The reference of a case is computed once: the float epilogue with every
threshold at -inf appends every finite score (no filter is involved), which
gives the kernel's own score bits for all (query, row) pairs -- checked against
fp64 -- and the records expected at any other thresholds are its scores >= thr.
Both epilogues must return that set, as (row, score bits) per query.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from lazzaro_amd.ops import _lib  # noqa: E402
from lazzaro_amd.ops import search as S  # noqa: E402

DEV = "cuda"
K = 10
OPT_FLOAT, OPT_TIER = 24, 88
SHAPES = [(D, n, nq) for D in (128, 384, 768) for n in (600, 1301) for nq in (256, 300)]
KINDS = ["unit", "unit_bias", "negative", "zero", "norms", "thr_pinf", "thr_ninf", "thr_exact", "bias_inf"]
NEG_INF = float("-inf")


def _scan(X8, rs, Q8, qs, bias, alpha, thr, opt):
    """One candidate pass + gather: (counts [nq], scores [nq, N] with -inf where
    (query, row) was not appended). cap = N holds every score of a query."""
    L = _lib.lib()
    N, Dp = X8.shape
    nq = Q8.shape[0]
    cap = N
    cnt = torch.zeros(nq, dtype=torch.int32, device=DEV)
    cs = torch.full((nq, cap), float("nan"), device=DEV)
    ci = torch.full((nq, cap), -1, dtype=torch.int32, device=DEV)
    grid = L.lzk_cand_grid_f8(N, nq)
    assert 1 < grid <= 4
    bcap = N * nq + 16  # a block's records can never overflow
    bbuf = torch.empty(grid * bcap * 16, dtype=torch.uint8, device=DEV)
    bcnt = torch.zeros(grid, dtype=torch.int32, device=DEV)
    st = _lib.stream_ptr(torch.device(DEV))
    L.lzk_set_i8_opt(opt)
    _lib.check(L.lzk_flat_cand_i8(X8.data_ptr(), X8.stride(0), N, Q8.data_ptr(), Q8.stride(0), nq, Dp, _lib.ptr(bias),
                                  rs.data_ptr(), qs.data_ptr(), float(alpha), thr.data_ptr(), cap, cnt.data_ptr(),
                                  cs.data_ptr(), ci.data_ptr(), bbuf.data_ptr(), bcap, bcnt.data_ptr(), st),
               "lzk_flat_cand_i8")
    _lib.check(L.lzk_cand_gather(bbuf.data_ptr(), bcap, bcnt.data_ptr(), grid, cap, nq, cnt.data_ptr(),
                                 cs.data_ptr(), ci.data_ptr(), None, None, None, st), "lzk_cand_gather")
    torch.cuda.synchronize()
    assert int(bcnt.max()) <= bcap and int(cnt.max()) <= cap and int(cnt.min()) >= 0
    live = torch.arange(cap, device=DEV)[None, :] < cnt[:, None]
    qi, pi = live.nonzero(as_tuple=True)
    rows = ci[qi, pi].long()
    assert bool(((rows >= 0) & (rows < N)).all())
    M = torch.full((nq, N), NEG_INF, device=DEV)
    M[qi, rows] = cs[qi, pi]
    # a (query, row) filed twice would leave fewer distinct cells than records
    assert torch.equal((M != NEG_INF).sum(1).int(), cnt)
    return cnt, M


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _data(kind, D, N, nq, gen):
    """fp32 rows / queries, whether the scan gets a bias, alpha."""
    X = torch.randn(N, D, device=DEV, generator=gen)
    X = X / X.norm(dim=1, keepdim=True)
    Q = torch.randn(nq, D, device=DEV, generator=gen)
    Q = Q / Q.norm(dim=1, keepdim=True)
    with_bias = kind != "unit"
    if kind == "negative":  # rows in the positive orthant, queries = -rows: every sum is negative
        X = X.abs()
        Q = -X[:nq].clone()
    elif kind == "zero":
        X[5] = 0.0
        X[N - 2] = 0.0  # one in the partial last tile
        Q[3] = 0.0
        Q[nq - 1] = 0.0
    elif kind == "norms":  # norms 1000x apart inside every 4-row quad
        X = X * torch.tensor([1.0, 1e-3, 0.03, 1.0], device=DEV).repeat((N + 3) // 4)[:N, None]
    return X, Q, with_bias, (2.0 if with_bias else 1.0)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D,N,nq", SHAPES)
def test_tiered_prefilter_appends_the_float_epilogues_records_gpu(D, N, nq, kind):
    L = _lib.lib()
    gen = torch.Generator(device=DEV).manual_seed(1000 * D + N + nq)
    X, Q, with_bias, alpha = _data(kind, D, N, nq, gen)
    X16, Q16 = X.to(torch.bfloat16), Q.to(torch.bfloat16)
    bias = -(X16.float() ** 2).sum(1).contiguous() if with_bias else None
    if kind == "bias_inf":
        bias[::3] = NEG_INF
    X8, rs = S.quantize_i8_rows(X16)
    Q8, qs = S.quantize_i8_rows(Q16)
    if kind == "zero":
        assert float(rs[5]) == 0.0 and float(qs[3]) == 0.0
    kslot = L.lzk_flat_topk_kslot(K)
    samp = max(1, N // (16 * kslot))
    thr = S._sample_threshold(X16, Q16, K, kslot, bias, None, None, alpha, samp).float().contiguous()
    L.lzk_set_cu_budget(4)
    try:
        # the reference: every finite score, from the float epilogue without any filter
        ninf = torch.full((nq,), NEG_INF, device=DEV)
        cnt_all, full = _scan(X8, rs, Q8, qs, bias, alpha, ninf, OPT_FLOAT)
        v = Q8.double() @ X8.double().T  # exact: |sum| < 2^24
        al = alpha * qs.double()[:, None]
        ref = al * (v * rs.double()[None, :]) + (bias.double()[None, :] if with_bias else 0.0)
        fin = torch.isfinite(ref)
        assert torch.equal(full != NEG_INF, fin)  # all but the -inf-biased rows, none beyond nrows
        mag = (al * (v * rs.double()[None, :])).abs() + (bias.double().abs()[None, :] if with_bias else 0.0)
        err = (full.double() - ref).abs()
        assert bool((err[fin] <= 2.5e-7 * mag[fin] + 1e-30).all())  # two fp32 roundings of the parts

        if kind == "thr_pinf":
            thr = torch.full((nq,), float("inf"), device=DEV)
        elif kind == "thr_ninf":
            thr = ninf
        elif kind == "thr_exact":
            # each query's threshold IS its K-th largest score: that record must be appended
            thr = torch.topk(full, K, dim=1).values[:, K - 1].contiguous()
            assert bool(torch.isfinite(thr).all())
        elif kind == "zero":
            thr[3] = 0.0  # a zero query (al = 0): every score equals the bias
            thr[nq - 1] = NEG_INF
        want = torch.where((full >= thr[:, None]) & (full != NEG_INF), full, torch.full_like(full, NEG_INF))
        got = {}
        for opt in (OPT_FLOAT, OPT_TIER):
            cnt, M = _scan(X8, rs, Q8, qs, bias, alpha, thr, opt)
            got[opt] = (cnt, M)
            assert _same_bits(M, want), (kind, opt, int((M != want).sum()))
        assert torch.equal(got[OPT_FLOAT][0], got[OPT_TIER][0])
        assert _same_bits(got[OPT_FLOAT][1], got[OPT_TIER][1])
        n_rec = int(got[OPT_TIER][0].sum())
        if kind == "thr_pinf":
            assert n_rec == 0
        elif kind == "thr_ninf":
            assert n_rec == int(fin.sum()) and torch.equal(got[OPT_TIER][0], cnt_all)
        elif kind == "thr_exact":
            assert int(got[OPT_TIER][0].min()) >= K
        else:
            assert n_rec >= K * (nq - 2)  # the sample's K-th best bounds the K-th best from below
    finally:
        L.lzk_set_cu_budget(0)
        L.lzk_set_i8_opt(-1)


@pytest.mark.parametrize("D", [128, 384, 768])
def test_flat_topk_i8_with_tiered_prefilter_matches_bf16_gpu(D):
    """The whole int8 search on the tiered epilogue == on the float epilogue
    == the bf16 scan's top-10 (scores up to accumulation order)."""
    L = _lib.lib()
    N, nq = 1301, 300
    gen = torch.Generator(device=DEV).manual_seed(7 + D)
    X, Q, _, alpha = _data("unit_bias", D, N, nq, gen)
    X16, Q16 = X.to(torch.bfloat16), Q.to(torch.bfloat16)
    bias = -(X16.float() ** 2).sum(1).contiguous()
    bias[::7] = NEG_INF
    X8, rs = S.quantize_i8_rows(X16)
    Q8, qs = S.quantize_i8_rows(Q16)
    s16, r16 = S.flat_topk(X16, Q16, K, bias=bias, alpha=alpha)
    margin = torch.full((nq,), 0.05, device=DEV)  # ~1e-3 of int8 error at these sizes
    L.lzk_set_cu_budget(4)
    try:
        res = {}
        for opt in (OPT_FLOAT, OPT_TIER):
            L.lzk_set_i8_opt(opt)
            res[opt] = S.flat_topk_i8(X8, rs, Q8, qs, X16, Q16, K, bias=bias, alpha=alpha, margin=margin)
        torch.cuda.synchronize()
    finally:
        L.lzk_set_cu_budget(0)
        L.lzk_set_i8_opt(-1)
    assert torch.equal(res[OPT_FLOAT][1], res[OPT_TIER][1]) and _same_bits(res[OPT_FLOAT][0], res[OPT_TIER][0])
    s8, r8 = res[OPT_TIER]
    assert torch.equal(r8.sort(1).values, r16.sort(1).values)
    assert torch.allclose(s8, s16, atol=1e-4, rtol=0)
    assert not bool((r8 % 7 == 0).any())
