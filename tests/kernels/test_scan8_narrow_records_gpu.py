"""The narrow-batch int8 scan (scan8.hip ``scan8_narrow_kernel``, nq <= 128)
record for record: ``lzk_scan8_narrow`` + ``lzk_cand_gather`` over its grid * 8
wave regions, called directly, against tests/kernels/_cand_ref.py
``i8_scores``. All eight query-tile templates (nq 1..128 -> 1..8 tiles of 16),
both K builds (Dp = 768: the 12-chunk, 128-VGPR one; any other Dp: 16 chunks),
bias / no bias, row counts around the 16-row block and its 4-row quads, and
one long case per K build whose waves walk three and two blocks (the
two-buffer trip loop).

Grid inputs (int8 in [-8, 8], power-of-two scales, alpha = 2, integer bias):
the appended scores carry the fp64 bits, so the record set at any threshold
is known exactly, ties included. Quantised Gaussian inputs: the thr = -inf
pass yields the kernel's own bits (checked against fp64 to two fp32 roundings,
2.5e-7 x magnitude, as in test_scan_i8_prefilter_gpu.py); the set at any other
threshold is then exact.

Observed on one MI355X: the 155 cases take 5.6 s together; the slowest is the
first one run (0.67 s, it loads the library), the long cases 0.06 and 0.24 s.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from lazzaro_amd.ops import _lib  # noqa: E402
from lazzaro_amd.ops import search as S  # noqa: E402
from tests.kernels import _cand_ref as R  # noqa: E402

DEV = "cuda"
K = 10
NEG_INF = float("-inf")
NQS = [1, 15, 16, 17, 33, 49, 65, 81, 100, 127, 128]  # 1, 1, 1, 2, 3, 4, 5, 6, 7, 8, 8 query tiles
DPS = [64, 128, 384, 768, 1024]
NROWS = [1, 15, 16, 17, 2051]


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(dtype) if dtype is not None else t).to(DEV)


def _scan(X8, rs, Q8, qs, bias, alpha, thr, capw=None):
    """One narrow pass + gather. Returns (counts [nq], M [nq, N] fp32 with -inf
    where (query, row) was not appended, region counts, capw, record buffer)."""
    L = _lib.lib()
    N, Dp = X8.shape
    nq = Q8.shape[0]
    grid = L.lzk_scan8_narrow_grid(N)
    regions = grid * 8
    nblk = (N + 15) // 16
    if capw is None:  # every (row, query) of the blocks a wave walks, rows past nrows included
        capw = ((nblk + regions - 1) // regions) * 16 * nq + 16
    bbuf = torch.zeros((regions * capw + 4, 4), dtype=torch.int32, device=DEV)
    bbuf[regions * capw:] = -77  # nothing is written past the last region
    bcnt = torch.full((regions,), -1, dtype=torch.int32, device=DEV)
    cap = N
    cnt = torch.zeros(nq, dtype=torch.int32, device=DEV)
    cs = torch.full((nq, cap), float("nan"), device=DEV)
    ci = torch.full((nq, cap), -1, dtype=torch.int32, device=DEV)
    st = _lib.stream_ptr(torch.device(DEV))
    _lib.check(L.lzk_scan8_narrow(X8.data_ptr(), X8.stride(0), N, Q8.data_ptr(), Q8.stride(0), nq, Dp, _lib.ptr(bias),
                                  rs.data_ptr(), qs.data_ptr(), float(alpha), thr.data_ptr(), bbuf.data_ptr(), capw,
                                  bcnt.data_ptr(), st), "lzk_scan8_narrow")
    _lib.check(L.lzk_cand_gather(bbuf.data_ptr(), capw, bcnt.data_ptr(), regions, cap, nq, cnt.data_ptr(),
                                 cs.data_ptr(), ci.data_ptr(), None, None, None, st), "lzk_cand_gather")
    torch.cuda.synchronize()
    assert bool((bbuf[regions * capw:] == -77).all())
    assert int(bcnt.min()) >= 0
    M = None
    if int(bcnt.max()) <= capw:
        assert int(cnt.max()) <= cap and int(cnt.min()) >= 0, (int(cnt.max()), cap)
        live = torch.arange(cap, device=DEV)[None, :] < cnt[:, None]
        qi, pi = live.nonzero(as_tuple=True)
        rows = ci[qi, pi].long()
        assert bool(((rows >= 0) & (rows < N)).all())  # rows past nrows never appear
        M = torch.full((nq, N), NEG_INF, device=DEV)
        M[qi, rows] = cs[qi, pi]
        assert torch.equal((M != NEG_INF).sum(1).int(), cnt)  # no (query, row) filed twice
    return cnt, M, bcnt, capw, bbuf


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _grid_inputs(rng, N, nq, Dp, with_bias):
    X8 = rng.integers(-8, 9, size=(N, Dp), dtype=np.int8)  # grid_rows' values, as int8 (the long cases: 100 MB)
    rs = R.grid_scales(rng, N)
    bias = rng.integers(-64, 65, size=N).astype(np.float32) if with_bias else None
    # exact ties across a 16-row block boundary (rows 15 | 16) and into the ragged 4-row tail (N - 4 | N - 3 ..)
    for a, b in ((15, 16), (N - 4, N - 3), (N - 4, N - 1)):
        if 0 <= a < N and 0 <= b < N:
            X8[b], rs[b] = X8[a], rs[a]
            if with_bias:
                bias[b] = bias[a]
    if with_bias and N > 2:
        bias[rng.integers(0, N, size=max(1, N // 5))] = NEG_INF
    return X8, rs, R.grid_queries(rng, nq, Dp).astype(np.int8), R.grid_scales(rng, nq), bias


def _check_grid(N, nq, Dp, with_bias, seed):
    rng = np.random.default_rng(seed)
    alpha = 2.0
    X8, rs, Q8, qs, bias = _grid_inputs(rng, N, nq, Dp, with_bias)
    ref = R.i8_scores(X8, rs, Q8, qs, bias, alpha)
    assert np.abs(ref[np.isfinite(ref)]).max(initial=0.0) < 2.0 ** 24
    d = (_dev(X8, torch.int8), _dev(rs), _dev(Q8, torch.int8), _dev(qs), _dev(bias) if with_bias else None)
    e_all = _dev(ref, torch.float32)  # exact: the fp64 values are fp32 numbers
    fin = e_all != NEG_INF
    ninf = torch.full((nq,), NEG_INF, device=DEV)
    cnt, M, _, _, _ = _scan(*d, alpha, ninf)
    assert _same_bits(M, e_all), int((M != e_all).sum())  # exactly the finite scores, with the fp64 bits
    assert torch.equal(cnt, fin.sum(1).int())
    # thr_exact: a query's threshold IS one of its scores -- the K-th largest, or (odd queries) the score of
    # row 15, which ties with row 16 in the next 16-row block: every tied record must be appended
    kk = min(K, N)
    thr = torch.topk(e_all, kk, dim=1).values[:, kk - 1].clone()
    if N > 16:
        odd = torch.arange(nq, device=DEV) % 2 == 1
        thr = torch.where(odd & (e_all[:, 15] != NEG_INF), e_all[:, 15], thr)
    thr = torch.where(thr == NEG_INF, torch.zeros_like(thr), thr).contiguous()
    want = torch.where((e_all >= thr[:, None]) & fin, e_all, torch.full_like(e_all, NEG_INF))
    cnt, M, _, _, _ = _scan(*d, alpha, thr)
    assert _same_bits(M, want), int((M != want).sum())
    cnt, M, bcnt, _, _ = _scan(*d, alpha, torch.full((nq,), float("inf"), device=DEV))
    assert int(cnt.sum()) == 0 and int(bcnt.sum()) == 0 and bool((M == NEG_INF).all())
    return d, e_all


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("Dp", DPS)
@pytest.mark.parametrize("nq", NQS)
def test_narrow_scan_grid_records_gpu(nq, Dp, with_bias):
    for N in NROWS:
        _check_grid(N, nq, Dp, with_bias, 1000 * nq + Dp + N)


@pytest.mark.parametrize("Dp", [64, 768])
def test_narrow_scan_three_trip_loop_gpu(Dp):
    """nrows = 16 * 8 * (2 g + 3) + 5 with g the launch's grid at that size:
    the first waves walk three 16-row blocks (fa, fb, fa again), the others
    two; Dp = 768 is the 12-chunk build, 64 the 16-chunk one."""
    L = _lib.lib()
    g = L.lzk_scan8_narrow_grid(1 << 24)  # the full grid (rows enough for every wave)
    N = 16 * 8 * (2 * g + 3) + 5
    assert L.lzk_scan8_narrow_grid(N) == g
    nblk, stride = (N + 15) // 16, 8 * g
    assert 2 * stride < nblk < 3 * stride
    _check_grid(N, 5, Dp, True, 31 + Dp)


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("Dp", DPS)
@pytest.mark.parametrize("nq", [1, 17, 100, 128])
def test_narrow_scan_quantised_gaussian_records_gpu(nq, Dp, with_bias):
    alpha = 2.0 if with_bias else 1.0
    for N in (17, 2051):
        gen = torch.Generator(device=DEV).manual_seed(7 * nq + Dp + N)
        X = torch.randn(N, Dp, device=DEV, generator=gen)
        X = (X / X.norm(dim=1, keepdim=True)).to(torch.bfloat16)
        Q = torch.randn(nq, Dp, device=DEV, generator=gen)
        Q = (Q / Q.norm(dim=1, keepdim=True)).to(torch.bfloat16)
        X[N // 2] = 0.0
        bias = -(X.float() ** 2).sum(1).contiguous() if with_bias else None
        if with_bias:
            bias[::3] = NEG_INF
        X8, rs = S.quantize_i8_rows(X)
        Q8, qs = S.quantize_i8_rows(Q)
        ninf = torch.full((nq,), NEG_INF, device=DEV)
        cnt, full, _, _, _ = _scan(X8, rs, Q8, qs, bias, alpha, ninf)
        host = [t.cpu().numpy() if t is not None else None for t in (X8, rs, Q8, qs, bias)]
        ref = R.i8_scores(*host, alpha)
        mag = R.i8_magnitude(*host, alpha)
        fin = np.isfinite(ref)
        got = full.cpu().numpy().astype(np.float64)
        assert np.array_equal(got != NEG_INF, fin)
        assert (np.abs(got[fin] - ref[fin]) <= 2.5e-7 * mag[fin] + 1e-30).all()  # two fp32 roundings of the parts
        kk = min(K, int(fin.sum(1).min()))
        thr = torch.topk(full, kk, dim=1).values[:, kk - 1].contiguous()
        assert bool(torch.isfinite(thr).all())
        want = torch.where((full >= thr[:, None]) & (full != NEG_INF), full, torch.full_like(full, NEG_INF))
        cnt, M, _, _, _ = _scan(X8, rs, Q8, qs, bias, alpha, thr)
        assert _same_bits(M, want), int((M != want).sum())
        assert int(cnt.min()) >= kk


@pytest.mark.parametrize("Dp", [128, 768])
def test_narrow_scan_agrees_with_the_wide_scan_gpu(Dp):
    """Both int8 scans compute alpha qs (rs v) + bias from the same exact
    int32 v: their scores agree within the two fp32 roundings either may place
    differently (2.5e-7 x magnitude), nq = 100, nrows = 2051."""
    L = _lib.lib()
    N, nq, alpha = 2051, 100, 2.0
    gen = torch.Generator(device=DEV).manual_seed(Dp)
    X = torch.randn(N, Dp, device=DEV, generator=gen)
    X = (X / X.norm(dim=1, keepdim=True)).to(torch.bfloat16)
    Q = torch.randn(nq, Dp, device=DEV, generator=gen)
    Q = (Q / Q.norm(dim=1, keepdim=True)).to(torch.bfloat16)
    bias = -(X.float() ** 2).sum(1).contiguous()
    X8, rs = S.quantize_i8_rows(X)
    Q8, qs = S.quantize_i8_rows(Q)
    ninf = torch.full((nq,), NEG_INF, device=DEV)
    _, narrow, _, _, _ = _scan(X8, rs, Q8, qs, bias, alpha, ninf)
    cap = N
    cnt = torch.zeros(nq, dtype=torch.int32, device=DEV)
    cs = torch.full((nq, cap), float("nan"), device=DEV)
    ci = torch.full((nq, cap), -1, dtype=torch.int32, device=DEV)
    st = _lib.stream_ptr(torch.device(DEV))
    L.lzk_set_cu_budget(4)
    try:
        grid = L.lzk_cand_grid_f8(N, nq)
        assert 1 < grid <= 4
        bcap = N * nq + 16
        bbuf = torch.empty(grid * bcap * 16, dtype=torch.uint8, device=DEV)
        bcnt = torch.zeros(grid, dtype=torch.int32, device=DEV)
        _lib.check(L.lzk_flat_cand_i8(X8.data_ptr(), X8.stride(0), N, Q8.data_ptr(), Q8.stride(0), nq, Dp,
                                      bias.data_ptr(), rs.data_ptr(), qs.data_ptr(), alpha, ninf.data_ptr(), cap,
                                      cnt.data_ptr(), cs.data_ptr(), ci.data_ptr(), bbuf.data_ptr(), bcap,
                                      bcnt.data_ptr(), st), "lzk_flat_cand_i8")
        _lib.check(L.lzk_cand_gather(bbuf.data_ptr(), bcap, bcnt.data_ptr(), grid, cap, nq, cnt.data_ptr(),
                                     cs.data_ptr(), ci.data_ptr(), None, None, None, st), "lzk_cand_gather")
        torch.cuda.synchronize()
    finally:
        L.lzk_set_cu_budget(0)
    assert bool((cnt == N).all())
    rows = ci.long()
    assert bool(((rows >= 0) & (rows < N)).all())
    wide = torch.full((nq, N), NEG_INF, device=DEV)
    wide.scatter_(1, rows, cs)
    mag = R.i8_magnitude(*[t.cpu().numpy() for t in (X8, rs, Q8, qs, bias)], alpha)
    err = (narrow.double() - wide.double()).abs().cpu().numpy()
    assert (err <= 2.5e-7 * mag + 1e-30).all(), float((err / mag).max())


def test_narrow_scan_full_regions_flag_every_query_gpu():
    """capw = 8: every wave that walks a block overflows its region. The
    region counts keep the true totals, a region holds only its own wave's
    first 8 records (nothing is written past it), and the gather marks every
    query's count with bit 30 while still filing those records."""
    L = _lib.lib()
    rng = np.random.default_rng(3)
    N, nq, Dp, alpha = 2051, 33, 128, 2.0
    X8, rs, Q8, qs, bias = _grid_inputs(rng, N, nq, Dp, False)
    d = (_dev(X8, torch.int8), _dev(rs), _dev(Q8, torch.int8), _dev(qs), None)
    ninf = torch.full((nq,), NEG_INF, device=DEV)
    cnt, M, bcnt, capw, bbuf = _scan(*d, alpha, ninf, capw=8)
    assert M is None and capw == 8
    regions = bcnt.numel()
    nblk = (N + 15) // 16
    blocks = np.array([len(range(w, nblk, regions)) for w in range(regions)])
    rows_w = np.array([sum(min(16, N - 16 * b) for b in range(w, nblk, regions)) for w in range(regions)])
    assert np.array_equal(bcnt.cpu().numpy(), rows_w * nq)  # every (query, row) of the wave's blocks, counted
    assert (blocks > 0).any()
    c = cnt.cpu().numpy().astype(np.int64)
    assert ((c & R.CNT_OVF) != 0).all()  # every query flagged
    rec = bbuf[: regions * 8].view(regions, 8, 4).cpu().numpy()
    filed = np.zeros(nq, dtype=np.int64)
    ref = R.i8_scores(X8, rs, Q8, qs, None, alpha).astype(np.float32)
    for w in range(regions):
        n = min(8, int(rows_w[w]) * nq)
        r = rec[w, :n]
        assert ((r[:, 1] // 16) % regions == w).all() and (r[:, 1] < N).all(), w  # the wave's own rows only
        assert ((r[:, 0] >= 0) & (r[:, 0] < nq) & (r[:, 3] == 1)).all()
        assert np.array_equal(r[:, 2], ref[r[:, 0], r[:, 1]].view(np.int32))
        assert (rec[w, n:] == 0).all()
        np.add.at(filed, r[:, 0], 1)
    assert np.array_equal(c & R.CNT_MASK, filed)  # the first capw records of each region are still filed
