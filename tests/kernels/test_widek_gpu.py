"""The wide-k store search (k = 17 .. 64) on the GPU against the fp64
references of tests/kernels/_wide_ref.py and _cand_ref.py: the two kernels of
csrc/kernels/widek.hip (``lzk_cand_select_wide``, ``lzk_flat_topk_wide`` and its
masked variant), ``ops.search.flat_topk_i8_wide`` end to end, and
``TenantGraph.store_search`` with ``wide_k=True``. Grid inputs are compared bit
for bit; the Gaussian cases are the decidable ones of _wide_ref.py (proved so
in tests/unit/test_wide_ref_cpu.py), so rows are compared exactly and scores
within the derived bound, no query left out."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from lazzaro_amd.engine import tenant_graph as TG  # noqa: E402
from lazzaro_amd.ops import _lib  # noqa: E402
from lazzaro_amd.ops import search as S  # noqa: E402
from tests.kernels import _boost_ref as BR  # noqa: E402
from tests.kernels import _cand_ref as R  # noqa: E402
from tests.kernels import _wide_ref as W  # noqa: E402

DEV = "cuda"
NEG_INF = float("-inf")
F32 = np.float32


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(dtype) if dtype is not None else t).to(DEV)


def _np(t):
    return t.cpu().numpy()


# ================================================================ lzk_cand_select_wide
def _lists(rng, nq, cap, kout):
    """Grid lists: integer scores in [-40, 40] (many equal), rows below 3 cap
    drawn with repeats, -inf entries, equal (score, row) pairs planted; counts
    0, kout - 1, kout, cap, cap + 1, a count with bit 30 set, then random."""
    cs = rng.integers(-40, 41, size=(nq, cap)).astype(F32)
    ci = rng.integers(0, 3 * cap, size=(nq, cap)).astype(np.int32)
    cs[rng.random((nq, cap)) < 0.05] = NEG_INF
    for q in range(nq):
        m = min(cap, 40)
        cs[q, :m:4] = 40.0                       # a plateau at the top: only the row decides
        if cap >= 8:
            cs[q, 5], ci[q, 5] = cs[q, 1], ci[q, 1]  # the same (score, row) twice
            ci[q, 6] = ci[q, 2]                      # one row under two scores
    special = [0, kout - 1, kout, cap, cap + 1, (cap // 2) | R.CNT_OVF, cap | R.CNT_OVF]
    cnt = np.array([special[q % len(special)] if q < 2 * len(special) else rng.integers(0, cap + 1)
                    for q in range(nq)], dtype=np.int64)
    need = np.where(rng.random(nq) < 0.5, (cnt & R.CNT_MASK) + 1, np.maximum((cnt & R.CNT_MASK) - 1, 0)).astype(np.int32)
    need[::5] = 0
    return cnt.astype(np.int32), cs, ci, need


def _select(cnt, cs, ci, cap, kout, idx_offset=0, need=None, q_active=None, out=None):
    s, r, ovf = S.cand_select_wide(_dev(cnt) if cnt is not None else None, _dev(cs), _dev(ci), cap, kout,
                                   idx_offset=idx_offset, need=_dev(need) if need is not None else None,
                                   q_active=q_active, out=out)
    torch.cuda.synchronize()
    return _np(s), _np(r), _np(ovf)


@pytest.mark.parametrize("nq", [1, 5, 70])
@pytest.mark.parametrize("kout", [17, 32, 33, 63, 64])
def test_select_wide_against_select_ref_gpu(kout, nq):
    rng = np.random.default_rng(100 * kout + nq)
    for cap in (64, 100, 2048, 16384):
        cnt, cs, ci, need = _lists(rng, nq, cap, kout)
        for use_need, off in ((False, 0), (True, 1000003)):
            nd = need if use_need else None
            e_s, e_r, e_o = R.select_ref(cnt.astype(np.int64) & 0xFFFFFFFF, cs, ci, cap, kout, off, nd)
            s, r, ovf = _select(cnt, cs, ci, cap, kout, off, nd)
            assert np.array_equal(ovf, e_o), (cap, np.flatnonzero(ovf != e_o)[:8])
            assert np.array_equal(r, e_r), (cap, np.flatnonzero((r != e_r).any(1))[:8])
            assert np.array_equal(s.astype(np.float64), e_s)


def test_select_wide_walks_lists_past_its_lds_in_pieces_gpu():
    """cap = 40,000 > the 16,384 entries staged at once: three pieces, the
    running best 64 carried in block 0; the best entries sit in the last."""
    rng = np.random.default_rng(9)
    nq, cap, kout = 3, 40000, 64
    cnt, cs, ci, _ = _lists(rng, nq, cap, kout)
    cnt[:] = [cap, 16384 + 70, cap - 1]
    cs[0, -30:] = 41.0
    cs[2, 16383:16390] = 42.0
    e_s, e_r, e_o = R.select_ref(cnt, cs, ci, cap, kout)
    s, r, ovf = _select(cnt, cs, ci, cap, kout)
    assert np.array_equal(r, e_r) and np.array_equal(s.astype(np.float64), e_s) and np.array_equal(ovf, e_o)


def test_select_wide_smallest_tournaments_nan_and_negative_zero_gpu():
    """The shared tournament (csrc/include/lzk_topk64.h) called with a running
    best in block 0: one staged block (cap = 64), three with the last partly
    filled (130 of cap = 192), and the shortest list that takes two pieces
    (16,384 + 100). A nan selects as -inf does; -0 and +0 are one score, so
    the row decides among them."""
    rng = np.random.default_rng(12)
    nq, kout = 2, 64
    for cap, c in ((64, 64), (192, 130), (16384 + 100, 16384 + 100)):
        _, cs, ci, _ = _lists(rng, nq, cap, kout)
        cs = -np.abs(cs)  # (the zeros, every drawn one a -0, are the plateau at the top)
        cnt = np.full(nq, c, dtype=np.int32)
        for at, sc, row in ((3, np.nan, 1), (7, -0.0, 50), (9, 0.0, 20), (11, -0.0, 35), (c - 2, -0.0, 10),
                            (c - 1, np.nan, 2)):
            cs[:, at], ci[:, at] = sc, row
        e_s, e_r, e_o = R.select_ref(cnt, np.where(np.isnan(cs), F32(NEG_INF), cs), ci, cap, kout)
        s, r, ovf = _select(cnt, cs, ci, cap, kout)
        assert np.array_equal(r, e_r), (cap, r[0], e_r[0])
        assert np.array_equal(s.astype(np.float64), e_s) and np.array_equal(ovf, e_o)
        assert not np.isnan(s).any()
        for q in range(nq):  # (the case means what it says: the four zeros are among the 64)
            assert {10, 20, 35, 50} <= {int(x) for x, v in zip(r[q], s[q]) if v == 0.0}, (cap, r[q])


def test_select_wide_as_a_masked_merge_gpu():
    """cnt null (every list full), q_active given: inactive queries' outputs
    stay as they were; nothing at all is written when none is active."""
    rng = np.random.default_rng(10)
    nq, cap, kout = 9, 192, 40
    _, cs, ci, _ = _lists(rng, nq, cap, kout)
    full = np.full(nq, cap, dtype=np.int64)
    e_s, e_r, _ = R.select_ref(full, cs, ci, cap, kout, 7)
    for act in (np.array([1, 0, 0, 1, 1, 0, 1, 0, 1], np.int32), np.zeros(nq, np.int32)):
        out = (torch.full((nq, kout), 123.0, device=DEV), torch.full((nq, kout), -77, dtype=torch.long, device=DEV))
        s, r, _ = _select(None, cs, ci, cap, kout, 7, None, _dev(act), out)
        on = act != 0
        assert np.array_equal(r[on], e_r[on]) and np.array_equal(s[on].astype(np.float64), e_s[on])
        assert (r[~on] == -77).all() and (s[~on] == 123.0).all()


def test_select_wide_refuses_invalid_arguments_gpu():
    L = _lib.lib()
    z = torch.zeros(64, device=DEV)
    zi = torch.zeros(64, dtype=torch.int32, device=DEV)
    ol = torch.zeros(64, dtype=torch.long, device=DEV)
    for cap, nq, kout in ((64, 1, 65), (64, 1, 0), (0, 1, 17), (64, 0, 17)):
        assert L.lzk_cand_select_wide(None, z.data_ptr(), zi.data_ptr(), cap, nq, kout, 0, z.data_ptr(), ol.data_ptr(),
                                      None, None, None, _lib.stream_ptr(z.device)) == 1, (cap, nq, kout)
    torch.cuda.synchronize()


# ================================================================ lzk_flat_topk_wide
def _wide(X, Q, k, bias=None, alpha=2.0, n_chunks=None, idx_offset=0):
    s, r = S.flat_topk_wide(_dev(X, torch.bfloat16), _dev(Q, torch.bfloat16), k, bias=None if bias is None else _dev(bias),
                            alpha=alpha, n_chunks=n_chunks, idx_offset=idx_offset)
    torch.cuda.synchronize()
    return _np(s).astype(np.float64), _np(r)


@pytest.mark.parametrize("N", [1, 63, 64, 65, 300, 4097, 10253])
def test_flat_topk_wide_grid_bit_for_bit_gpu(N):
    """Integer rows and queries in [-8, 8] (planted duplicate rows: exact ties),
    alpha = 2, bias = -|x|^2 with -inf rows, or none: every fp32 partial sum is
    an integer below 2^24, so the kernel returns the fp64 bits. One chunk and
    several, tiles of 960 rows and partial ones."""
    for D in (64, 128, 768):
        rng = np.random.default_rng(N + D)
        X = R.grid_rows(rng, N, D)
        Qall = R.grid_queries(rng, 130, D)
        bias = (-(X * X).sum(1)).astype(F32)
        bias[rng.random(N) < 0.1] = NEG_INF
        for (nq, k), b, nch in zip(((1, 17), (3, 40), (130, 64)), (bias, None, bias), (None, 3, 5)):
            Q = Qall[:nq]
            e_s, e_r = W.topk_ref(X, Q, k, b, 2.0, 11)
            s, r = _wide(X, Q, k, b, 2.0, nch, 11)
            assert np.array_equal(r, e_r), (D, nq, k, np.flatnonzero((r != e_r).any(1))[:8])
            assert np.array_equal(s, e_s), (D, nq, k)


def test_flat_topk_wide_fewer_live_rows_than_k_gpu():
    rng = np.random.default_rng(5)
    X, Q = R.grid_rows(rng, 4097, 64), R.grid_queries(rng, 3, 64)
    bias = np.full(4097, NEG_INF, dtype=F32)
    live = np.array([0, 959, 960, 1023, 1024, 4096, 2000])
    bias[live] = 3.0
    s, r = _wide(X, Q, 40, bias, 1.0)
    e_s, e_r = W.topk_ref(X, Q, 40, bias, 1.0)
    assert np.array_equal(r, e_r) and np.array_equal(s, e_s)
    assert (r[:, 7:] == -1).all() and (s[:, 7:] == NEG_INF).all() and (np.sort(r[:, :7], 1) == np.sort(live)).all()
    s, r = _wide(X, Q, 17, np.full(4097, NEG_INF, dtype=F32), 1.0)
    assert (r == -1).all() and (s == NEG_INF).all()


def test_flat_topk_wide_masked_leaves_inactive_queries_alone_gpu():
    rng = np.random.default_rng(6)
    N, D, nq, k = 4097, 128, 130, 40
    X, Q = R.grid_rows(rng, N, D), R.grid_queries(rng, nq, D)
    bias = (-(X * X).sum(1)).astype(F32)
    e_s, e_r = W.topk_ref(X, Q, k, bias, 2.0)
    X16, Q16, b = _dev(X, torch.bfloat16), _dev(Q, torch.bfloat16), _dev(bias)
    for act in ((rng.random(nq) < 0.3).astype(np.int32), np.zeros(nq, np.int32)):
        out = (torch.full((nq, k), 5.5, device=DEV), torch.full((nq, k), -9, dtype=torch.long, device=DEV))
        S._flat_topk_wide(X16, Q16, k, b, 2.0, 0, 3, q_active=_dev(act), out=out)
        torch.cuda.synchronize()
        s, r = _np(out[0]).astype(np.float64), _np(out[1])
        on = act != 0
        assert np.array_equal(r[on], e_r[on]) and np.array_equal(s[on], e_s[on])
        assert (r[~on] == -9).all() and (s[~on] == 5.5).all()


def test_flat_topk_wide_gaussian_rows_exact_scores_within_the_bound_gpu():
    X, Q, bias, Sc, B = W.gauss_case("wide_kernel")
    k = W.GAUSS_CASES["wide_kernel"][3]
    e_s, e_r = W.topk_of(Sc, k)
    for nch in (None, 4):
        s, r = _wide(X, Q, k, bias, W.ALPHA, nch)
        assert np.array_equal(r, e_r)
        err = np.abs(s - e_s) / np.take_along_axis(B, e_r, 1)
        print(f"n_chunks={nch}: largest |score - fp64| / bound = {err.max():.3f}")
        assert (err <= 1.0).all()


def test_flat_topk_wide_refuses_invalid_arguments_gpu():
    X16 = torch.zeros((64, 64), dtype=torch.bfloat16, device=DEV)
    with pytest.raises(AssertionError):
        S.flat_topk_wide(X16, X16[:2], 65)
    L = _lib.lib()
    z = torch.zeros(4096, device=DEV)
    args = lambda D, ldx, k: (X16.data_ptr(), ldx, 64, X16.data_ptr(), 64, 2, None, 1.0, D, 1, z.data_ptr(), z.data_ptr(),  # noqa: E731
                              k, 0, z.data_ptr(), z.data_ptr(), _lib.stream_ptr(z.device))
    for D, ldx, k in ((60, 64, 17), (64, 60, 17), (64, 64, 65), (4096, 4096, 17), (64, 32, 17)):
        assert L.lzk_flat_topk_wide(*args(D, ldx, k)) == 1, (D, ldx, k)
    torch.cuda.synchronize()


# ================================================================ flat_topk_i8_wide
N8, D8 = 10253, 128


def _i8_search(X, Q, bias, k, margin_mode="rig", monkeypatch=None, sink=None):
    """flat_topk_i8_wide the way TenantGraph._i8_candidates_wide drives it:
    margin_rig = the worst case of ``i8_query``; margin = the same ("rig") or the
    statistical one ("stat"). Returns (scores, rows, margin, margin_rig, the
    ``need`` flags handed to the select -- with a monkeypatch only)."""
    nq = Q.shape[0]
    X16, Q16, b = _dev(X, torch.bfloat16), _dev(Q, torch.bfloat16), _dev(bias)
    X8, rs = S.quantize_i8_rows(X16)
    xn = float(np.linalg.norm(X, axis=1).max()) + 2.0 ** -7
    sumsq = (X16.double() ** 2).sum(0).contiguous()
    smax = rs.max().reshape(1).contiguous()
    q8, qs, margin, mr = S.i8_query(Q16, D8, sumsq, X.shape[0], smax, W.ALPHA, 3.0, xn)
    mg = mr if margin_mode == "rig" else margin
    seen = {}
    if monkeypatch is not None:
        inner = S._select_with_fallback_wide

        def spy(*a, **kw):
            seen["need"] = kw.get("need")
            if sink is not None:
                kw["ovf_sink"] = sink
            return inner(*a, **kw)
        monkeypatch.setattr(S, "_select_with_fallback_wide", spy)
    s, r = S.flat_topk_i8_wide(X8, rs, q8, qs, X16, Q16, k, bias=b, alpha=W.ALPHA, margin=mg, margin_rig=mr)
    torch.cuda.synchronize()
    need = _np(seen["need"]) if seen.get("need") is not None else None
    i8 = (_np(X8), _np(rs), _np(q8), _np(qs))
    return _np(s).astype(np.float64), _np(r), _np(mg).astype(np.float64), _np(mr).astype(np.float64), need, i8


def _unit_grid(rng, n, nq):
    """Unit rows whose scores are exact in every precision: 64 entries of +-1/8
    (``_boost_ref.grid_rows``), planted duplicates; queries likewise."""
    X = BR.grid_rows(rng, n, D8).astype(np.float64)
    Q = BR.grid_rows(rng, nq, D8, dup=0).astype(np.float64)
    Q[: min(nq, 3)] = X[[0, 2, n - 1][: min(nq, 3)]]
    return X, Q


@pytest.mark.parametrize("margin_mode", ["rig", "stat"])
@pytest.mark.parametrize("nq", [1, 130])
@pytest.mark.parametrize("k", [17, 64])
def test_i8_wide_grid_equals_the_bf16_topk_gpu(k, nq, margin_mode):
    """Unit grid rows: 65 score levels over 10,253 rows, so the k-th score is a
    plateau of hundreds of rows and only the row number orders them."""
    rng = np.random.default_rng(k + nq)
    X, Q = _unit_grid(rng, N8, nq)
    bias = W.l2_bias(X)
    bias[rng.random(N8) < 0.05] = NEG_INF
    e_s, e_r = W.topk_ref(X, Q, k, bias, W.ALPHA)
    s, r = _i8_search(X, Q, bias, k, margin_mode)[:2]
    assert np.array_equal(r, e_r), np.flatnonzero((r != e_r).any(1))[:8]
    assert np.array_equal(s, e_s)


def _cert_reference(X, Q, bias, Sc, B, k, j, mg, mr, i8):
    """Which queries the certificate must send to the fallback, from fp64: the
    level is the sample's j-th best int8 score less its slack, - margin +
    margin_rig, + slack; a query is certified iff its k-th bf16 score reaches
    it. ``amb``: the k-th score within 4 bounds of the level (either way)."""
    X8, rs, q8, qs = i8
    Sx = max(1, min(64, N8 // 256))
    s8 = R.i8_scores(X8[::Sx], rs[::Sx], q8, qs, bias[::Sx], W.ALPHA)
    s8 = np.where(np.isnan(s8), NEG_INF, s8)
    sJ = -np.sort(-s8, axis=1)[:, j - 1]
    tau = sJ - R.C_2E4 * (1.0 + np.abs(sJ))
    cert = tau - mg + mr
    cert = cert + R.C_1E6 * (1.0 + np.abs(cert))
    e_s, e_r = W.topk_of(Sc, k)
    kth = e_s[:, k - 1]
    b = np.take_along_axis(B, e_r, 1)[:, k - 1] + 8 * R.U_FP32 * (1.0 + np.abs(sJ) + np.abs(mg) + np.abs(mr))
    return kth >= cert, np.abs(kth - cert) <= 4.0 * b


@pytest.mark.parametrize("margin_mode", ["rig", "stat"])
@pytest.mark.parametrize("nq", [1, 130])
@pytest.mark.parametrize("k", [17, 64])
def test_i8_wide_gaussian_and_the_certificate_gpu(k, nq, margin_mode, monkeypatch):
    """The repaired Gaussian store with, for a few queries, 12 near rows
    planted inside the sample: the result equals the fp64 ranking, and the
    queries sent to the fallback are exactly those the reference predicts --
    every planted one, and of the others those whose k-th score misses the
    certificate level."""
    name = f"i8_k{k}_nq{nq}"
    X, Q, bias, Sc, B, planted = W.cert_case(name)
    Sx = max(1, min(64, N8 // 256))
    j = S.wide_spec_j(k, Sx)
    assert 160 % Sx == 0 and j < W.CERT_ROWS
    s, r, mg, mr, need, i8 = _i8_search(X, Q, bias, k, margin_mode, monkeypatch)
    e_s, e_r = W.topk_of(Sc, k)
    assert np.array_equal(r, e_r), np.flatnonzero((r != e_r).any(1))[:8]
    assert (np.abs(s - e_s) <= np.take_along_axis(B, e_r, 1)).all()
    certified, amb = _cert_reference(X, Q, bias, Sc, B, k, j, mg, mr, i8)
    fb = need != 0
    print(f"{name} {margin_mode}: j={j}, fallback {int(fb.sum())} of {nq}, inside the guard {int(amb.sum())}")
    assert not certified[planted].any() and not amb[planted].any() and fb[planted].all()
    assert amb.sum() <= max(1, 0.05 * nq) - (nq == 1)
    assert np.array_equal(fb[~amb], ~certified[~amb])
    if nq == 1:  # the single query above is a planted one: the same store without the planted rows
        X, Q, bias, Sc, B = W.gauss_case(name)
        s, r, mg, mr, need, i8 = _i8_search(X, Q, bias, k, margin_mode, monkeypatch)
        e_s, e_r = W.topk_of(Sc, k)
        assert np.array_equal(r, e_r) and (np.abs(s - e_s) <= np.take_along_axis(B, e_r, 1)).all()
        certified, amb = _cert_reference(X, Q, bias, Sc, B, k, j, mg, mr, i8)
        assert not amb.any() and np.array_equal(need != 0, ~certified)


@pytest.mark.parametrize("nq", [1, 130])
@pytest.mark.parametrize("k", [17, 64])
def test_i8_wide_threshold_forced_too_high_is_still_exact_gpu(k, nq, monkeypatch):
    """WIDE_J = 1: tau is the sample's best score, above most queries' k-th:
    exact all the same, the flagged set equal to the reference's."""
    name = f"i8_k{k}_nq{nq}"
    X, Q, bias, Sc, B, planted = W.cert_case(name)
    monkeypatch.setattr(S, "WIDE_J", 1)
    s, r, mg, mr, need, i8 = _i8_search(X, Q, bias, k, "rig", monkeypatch)
    e_s, e_r = W.topk_of(Sc, k)
    assert np.array_equal(r, e_r)
    assert (np.abs(s - e_s) <= np.take_along_axis(B, e_r, 1)).all()
    certified, amb = _cert_reference(X, Q, bias, Sc, B, k, 1, mg, mr, i8)
    fb = need != 0
    print(f"{name} j=1: fallback {int(fb.sum())} of {nq}, inside the guard {int(amb.sum())}")
    assert np.array_equal(fb[~amb], ~certified[~amb]) and fb[planted].all()
    assert fb.sum() > planted.sum() or nq == 1  # (the best of 257 sample rows beats the k-th of 10,253 for many)


@pytest.mark.parametrize("nq", [1, 130])
@pytest.mark.parametrize("k", [17, 64])
def test_i8_wide_overflowing_lists_resolve_ties_by_row_gpu(k, nq, monkeypatch):
    """Every row equals query 0 and the list capacity is shrunk to 64: every
    list overflows, the masked wide kernel recomputes them, ties go by row."""
    rng = np.random.default_rng(50 + nq)
    Q = R.to_bf16(R.unit_rows(rng, nq, D8))
    X = np.repeat(Q[:1], N8, axis=0)
    bias = W.l2_bias(X)
    dead = [0, 1, 5, 4096, 4100]
    bias[dead] = NEG_INF
    for name in ("NARROW_CAP", "WIDE_CAP_MIN"):
        monkeypatch.setattr(S, name, 64)
    monkeypatch.setattr(S, "WIDE_LIST_FACTOR", 0)
    sink = []
    s, r = _i8_search(X, Q, bias, k, "rig", monkeypatch, sink)[:2]
    ovf, cnt = sink[0]
    assert bool((ovf == 1).all()) and int(cnt.min()) > 64
    want = np.array([i for i in range(k + 5) if i not in dead][:k])
    assert np.array_equal(r, np.repeat(want[None, :], nq, 0))
    for q in range(nq):
        e, b = R.score_ref(X, Q[q], want, bias, W.ALPHA)
        assert (np.abs(s[q] - e) <= b).all(), q
    # the Gaussian store under the same capacity: overflow for most queries, still exact
    Xg, Qg, bg, Sc, B, _ = W.cert_case(f"i8_k{k}_nq{nq}")
    s, r = _i8_search(Xg, Qg, bg, k, "rig")[:2]
    e_s, e_r = W.topk_of(Sc, k)
    assert np.array_equal(r, e_r) and (np.abs(s - e_s) <= np.take_along_axis(B, e_r, 1)).all()


@pytest.mark.parametrize("nq", [1, 130])
def test_i8_wide_fewer_live_rows_than_k_gpu(nq):
    X, Q, bias, _, _, _ = W.cert_case(f"i8_k17_nq{nq}")
    bias = np.full(N8, NEG_INF, dtype=F32)
    live = np.array([7, 120, 160, 5000, 9000, 10252, 64])
    bias[live] = W.l2_bias(X)[live]
    e_s, e_r = W.topk_ref(X, Q, 17, bias, W.ALPHA)
    s, r = _i8_search(X, Q, bias, 17)[:2]
    assert np.array_equal(r, e_r) and (r[:, 7:] == -1).all() and (s[:, 7:] == NEG_INF).all() and (r[:, :7] >= 0).all()
    b = W.wide_bound(X, Q, bias, W.ALPHA, D8 + 2)
    assert (np.abs(s[:, :7] - e_s[:, :7]) <= np.take_along_axis(b, e_r[:, :7], 1)).all()


# ================================================================ TenantGraph.store_search(wide_k=True)
def _graph(X, n_ghost=0, n_unstored=0, meta=None, edges=False, seed=0):
    n, D = X.shape
    g = TG.TenantGraph(device=DEV, dim=D, capacity=n)
    T = torch.from_numpy
    m = n - n_ghost - n_unstored
    sh = g.shard_id("w")
    cols = {} if meta is None else dict(sal=T(meta["sal"]), acc=T(meta["acc"]), last=T(meta["last"]), ts=T(meta["ts"]))
    types = ["plain" if i % 3 else "pinned" for i in range(n)] if meta is None else [BR.GRID_TYPES[c] for c in meta["tcode"]]
    g.add_nodes([f"m{i}" for i in range(m)], ["c"] * m, T(X[:m]), shard=sh, types=types[:m], stored=True,
                **{k: v[:m] for k, v in cols.items()})
    if n_ghost:
        g.add_nodes([f"g{i}" for i in range(n_ghost)], ["ghost"] * n_ghost, T(X[m:m + n_ghost]),
                    shard=g.shard_id("w", live=False), stored=True, ghost=True,
                    **{k: v[m:m + n_ghost] for k, v in cols.items()})
    if n_unstored:
        g.add_nodes([f"u{i}" for i in range(n_unstored)], ["unstored"] * n_unstored, T(X[m + n_ghost:]), shard=sh,
                    types=types[m + n_ghost:], stored=False, **{k: v[m + n_ghost:] for k, v in cols.items()})
    if edges:
        rng = np.random.default_rng(seed)
        src, dst = rng.integers(0, m, size=3 * m), rng.integers(0, m, size=3 * m)
        keep = src != dst
        g.append_edges_host(src[keep], dst[keep], rng.choice(np.array([0.5, 1.0], F32), size=int(keep.sum())),
                            np.full(int(keep.sum()), sh), g.etype("relates_to"))
    g.take_dirty_rows(), g.take_dirty_edges(), g.take_deleted()
    assert g.n == n and g.unit_rows() and not g.lean and g.emb8 is not None and g.emb8.dtype == torch.int8
    return g


@pytest.fixture
def small_tenants(monkeypatch):
    monkeypatch.setattr(TG, "LOWP_MIN_ROWS", 1024)


@functools.lru_cache(maxsize=None)
def _gauss_graph():
    X, Q = W.tenant_case()
    return _graph(X), X, Q


def _spy_exact(monkeypatch):
    calls = []
    inner = TG.TenantGraph._exact_store

    def spy(self, *a, **kw):
        calls.append(1)
        return inner(self, *a, **kw)
    monkeypatch.setattr(TG.TenantGraph, "_exact_store", spy)
    return calls


@pytest.mark.parametrize("metric", W.METRICS)
@pytest.mark.parametrize("M", [1, 130])
def test_store_search_wide_equals_the_contract_gpu(M, metric, small_tenants, monkeypatch):
    """Gaussian fp32 unit rows: the k best by the store's fp32 score among the
    64 rows with the largest bf16 score (_wide_ref.tenant_case forces both
    stages), k = 17, 40, 64; the exact scan is not consulted, the counter moves."""
    g, X, Q = _gauss_graph()
    calls = _spy_exact(monkeypatch)
    g.wide_k = True
    try:
        for k in (17, 40, 64):
            n0 = g.wide_searches
            s, r = g.store_search(_dev(Q[:M]), k, metric)
            torch.cuda.synchronize()
            assert g.wide_searches == n0 + 1 and not calls
            e_s, e_r, e_b = W.tenant_expected(X, Q[:M], metric, k)
            assert np.array_equal(_np(r), e_r), (k, np.flatnonzero((_np(r) != e_r).any(1))[:8])
            assert (np.abs(_np(s).astype(np.float64) - e_s) <= e_b).all()
    finally:
        g.wide_k = False
    s, r = g.store_search(_dev(Q[:M]), 40, metric)   # the flag off: today's exact scan
    assert len(calls) == 1 and g.wide_searches == n0 + 1


@functools.lru_cache(maxsize=None)
def _grid_graph():
    rng = np.random.default_rng(31)
    n = 4096
    X = BR.grid_rows(rng, n, 128)  # (64 entries of +-1/8, then zeros: the int8 copy needs Dp % 128 == 0)
    meta = BR.grid_meta(rng, n)
    g = _graph(X, n_ghost=64, n_unstored=64, meta=meta, edges=True)
    Q = BR.grid_rows(rng, 130, 128, dup=0)
    Q[:6] = X[[0, 2, 4, n - 1, n - 4, 900]]
    return g, X, torch.from_numpy(Q).to(DEV)


def _on_off(g, fn):
    g.wide_k = False
    off = fn()
    g.wide_k = True
    try:
        n0 = g.wide_searches
        on = fn()
        moved = g.wide_searches - n0
    finally:
        g.wide_k = False
    torch.cuda.synchronize()
    return on, off, moved


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("M", [1, 130])
def test_store_search_wide_grid_equals_the_flag_off_bit_for_bit_gpu(M, small_tenants, monkeypatch):
    """Unit grid rows (scores exact in bf16, fp32 and fp64; plateaus of equal
    scores): every composition returns the bits of the same call with the flag
    off, which runs the exact fp32 scan."""
    g, X, Qall = _grid_graph()
    Q = Qall[:M]
    calls = _spy_exact(monkeypatch)
    for metric in W.METRICS:
        for k in (17, 40, 64):
            on, off, moved = _on_off(g, lambda: g.store_search(Q, k, metric))
            assert _same(on, off) and moved == 1, (metric, k)
    assert len(calls) == 9  # the flag-off calls only
    for kw in (dict(node_rows=True), dict(where={"types": ["pinned"]}), dict(boost=BR.GRID_BOOST),
               dict(where={"types": ["pinned"]}, boost=BR.GRID_BOOST)):
        on, off, moved = _on_off(g, lambda: g.store_search(Q, 40, "l2", **kw))
        assert _same(on, off) and moved == 1, kw
        assert bool((on[1] >= 0).any())


def test_store_search_wide_mmr_pool_and_expand_gpu(small_tenants):
    from lazzaro_amd.ops.mmr_ops import mmr_select
    from tests.kernels._mmr_ref import check_rule1
    g, X, Q = _gauss_graph()
    Qd = _dev(Q[:64])
    g.wide_k = True
    try:
        n0 = g.wide_searches
        ps, pr = g.store_search(Qd, 64, "l2")
        s, r = g.store_search(Qd, 10, "l2", diversity=0.5, fetch_k=64)
        assert g.wide_searches == n0 + 2
        pick, obj = mmr_select(g.emb32[: g.n], Qd, pr, 10, 0.5)
        p = pick.long()
        assert (pick >= 0).all() and torch.equal(r, torch.gather(pr, 1, p))
        assert torch.equal(s.view(torch.int32), torch.gather(ps, 1, p).view(torch.int32))
        check_rule1(X, Q[:64], _np(pr), 10, 0.5, _np(pick), _np(obj))
        e_s, e_r, _ = W.tenant_expected(X, Q[:64], "l2", 64)
        assert np.array_equal(_np(pr), e_r)  # the pool is the wide contract's
    finally:
        g.wide_k = False
    gg, _, Qg = _grid_graph()
    for M in (1, 130):
        # (an expanded search seeds from at most 16 rows and ranks its own pool: limit = 64 never reaches the
        # store search with k > 16, so the flag must change nothing)
        on, off, moved = _on_off(gg, lambda: gg.store_search_expand(Qg[:M], 64, "l2", expand={"hops": 1}))
        assert _same(on, off) and moved == 0 and bool((on[1] >= 0).any())


def test_wide_k_through_the_public_surface_gpu(small_tenants, tmp_path):
    from lazzaro_amd.core.memory_system import MemorySystem
    from lazzaro_amd.core.providers import HashEmbedder, LocalLLM
    m = MemorySystem(llm_provider=LocalLLM(), embedding_provider=HashEmbedder(dim=64), enable_async=False,
                     load_from_disk=False, db_dir=str(tmp_path / "db"), device=DEV, index_params={"wide_k": True})
    try:
        assert m.graph.wide_k is True and m.get_stats()["engine"]["wide_searches"] == 0
    finally:
        m.close()
