"""Every stage of the certified int8 store search behind the scan, called
directly through ``_lib.lib()`` on hand-built lists and records and held
against tests/kernels/_cand_ref.py: ``lzk_thr_prep``, ``lzk_cand_gather``,
``lzk_cand_select``, ``lzk_cand_cut``, ``lzk_cand_rescore`` /
``lzk_cand_rescore32``. Exact-grid inputs (integers in [-8, 8], power-of-two
alpha, integer bias) are compared bit for bit, ties included; Gaussian inputs
within the derived bounds of the reference module.

Every row index a kernel may dereference -- also a kernel that is wrong --
lies inside the allocation: "row -1" and "row >= nrows" are presented to the
cut kernel through an ``nrows`` smaller than the allocation and an X (and
bias) that starts one row into a larger tensor; list slots past a query's
count hold nan scores and an ordinary row.

Observed on one MI355X: the 330 cases take 7.9 s together; the slowest,
test_cand_rescore_and_certificate_gpu[64-2048-1-gauss], 0.41 s.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from lazzaro_amd.ops import _lib  # noqa: E402
from lazzaro_amd.ops import search as S  # noqa: E402,F401  (registers the entry points' signatures)
from tests.kernels import _cand_ref as R  # noqa: E402

DEV = "cuda"
NEG_INF = float("-inf")
DS = [4, 252, 256, 260, 768, 1024, 2048]


def _st():
    return _lib.stream_ptr(torch.device(DEV))


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(dtype) if dtype is not None else t).to(DEV)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def _f32bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.int32)


# ================================================================ lzk_thr_prep
@pytest.mark.parametrize("mode", ["m+r", "m", "r", "none", "m+r, no cert"])
@pytest.mark.parametrize("nq", [1, 255, 256, 257])
def test_thr_prep_bits_gpu(nq, mode):
    """thr / cert bit-equal to the fp32 torch chain (thr_prep_ref), the list
    counts zeroed; a strided sample (ldts = 7, col = 3)."""
    L = _lib.lib()
    rng = np.random.default_rng(nq)
    fm = R.FLT_MAX
    special = np.array([np.inf, -np.inf, np.nan, fm, -fm, 0.0, 1e-42, -1e-42, 1.0, -3e38, 3e38])
    t = rng.standard_normal(nq) * 10.0 ** rng.integers(-6, 7, size=nq)
    pos = rng.permutation(nq)[: min(nq, special.size)]
    t[pos] = special[: pos.size] if nq > 1 else np.nan
    ts = rng.standard_normal((nq, 7)).astype(np.float32)
    ts[:, 3] = t.astype(np.float32)
    has_m, has_r, has_c = "m" in mode.split(",")[0], "r" in mode.split(",")[0], "no cert" not in mode
    m = np.abs(rng.standard_normal(nq)).astype(np.float32) if has_m else None
    mr = (1.5 * np.abs(rng.standard_normal(nq))).astype(np.float32) if has_r else None
    d_ts, d_m, d_mr = _dev(ts), (_dev(m) if has_m else None), (_dev(mr) if has_r else None)
    thr = torch.full((nq + 1,), 7.0, device=DEV)
    cert = torch.full((nq + 1,), 7.0, device=DEV)
    cnt = torch.full((nq + 1,), 0x12345678, dtype=torch.int32, device=DEV)
    _lib.check(L.lzk_thr_prep(d_ts.data_ptr(), 7, 3, _lib.ptr(d_m), _lib.ptr(d_mr), nq, thr.data_ptr(),
                              cert.data_ptr() if has_c else None, cnt.data_ptr(), _st()), "lzk_thr_prep")
    torch.cuda.synchronize()
    e_thr, e_cert = R.thr_prep_ref(ts, 3, m, mr)
    assert np.array_equal(_bits(thr[:nq]), e_thr.view(np.int32))
    if has_c:
        assert np.array_equal(_bits(cert[:nq]), e_cert.view(np.int32))
    else:
        assert bool((cert == 7.0).all())
    assert bool((cnt[:nq] == 0).all())
    assert float(thr[nq]) == 7.0 and float(cert[nq]) == 7.0 and int(cnt[nq]) == 0x12345678  # nothing past nq


# ================================================================ lzk_cand_gather
def _gather_case(nq, dual, over):
    rng = np.random.default_rng(17 * nq + 2 * dual + over)
    bcap, regions = 600, 3
    bcnt = np.array([bcap + 50 if over else bcap, 137, 5 if over else 0], dtype=np.int32)
    recs = np.zeros((regions, bcap, 4), dtype=np.int32)
    recs[..., 0] = rng.integers(0, nq, size=(regions, bcap))
    hot = rng.random((regions, bcap)) < 0.35
    recs[..., 0][hot] = 0  # query 0 receives more than cap records
    recs[..., 1] = rng.integers(0, 1 << 20, size=(regions, bcap))
    recs[..., 2] = rng.standard_normal((regions, bcap)).astype(np.float32).view(np.int32)
    recs[..., 3] = rng.integers(0, 4, size=(regions, bcap)) if dual else rng.integers(0, 2, size=(regions, bcap))
    bad = rng.random((regions, bcap)) < 0.1  # padding queries: ignored
    recs[..., 0][bad] = rng.choice([-1, nq, nq + 7, 1 << 30], size=int(bad.sum()))
    return recs, bcnt, bcap, regions


@pytest.mark.parametrize("over", [0, 1])
@pytest.mark.parametrize("dual", [0, 1])
@pytest.mark.parametrize("nq", [5, 63, 64, 100])
def test_cand_gather_files_records_gpu(nq, dual, over):
    """nq < 64: the wave-aggregated path; nq >= 64: one atomic per record.
    Counts exactly; lists as multisets (a list past ``cap`` keeps cap of its
    records); a region with bcnt > bcap flags every query (bit 30) and its
    first bcap records are still filed; records past min(bcnt, bcap) are not."""
    L = _lib.lib()
    recs, bcnt, bcap, regions = _gather_case(nq, dual, over)
    cap = 40
    lists = []
    for _ in range(2 if dual else 1):
        lists.append((torch.zeros(nq + 1, dtype=torch.int32, device=DEV),
                      torch.full((nq + 1, cap), float("nan"), device=DEV),
                      torch.full((nq + 1, cap), -5, dtype=torch.int32, device=DEV)))
    d_recs, d_bcnt = _dev(recs), _dev(bcnt)
    a, b = lists[0], (lists[1] if dual else (None, None, None))
    _lib.check(L.lzk_cand_gather(d_recs.data_ptr(), bcap, d_bcnt.data_ptr(), regions, cap, nq, a[0].data_ptr(),
                                 a[1].data_ptr(), a[2].data_ptr(), _lib.ptr(b[0]), _lib.ptr(b[1]), _lib.ptr(b[2]),
                                 _st()), "lzk_cand_gather")
    torch.cuda.synchronize()
    ref = R.gather_ref(recs, bcnt, bcap, nq, bool(dual))
    assert int(ref[0][0][0] & R.CNT_MASK) > cap  # query 0 overflows its list
    for (cnt, cs, ci), (e_cnt, e_filed) in zip(lists, ref):
        assert np.array_equal(cnt[:nq].cpu().numpy().astype(np.int64), e_cnt)
        assert bool(((e_cnt & R.CNT_OVF) != 0).all()) == bool(over)
        assert int(cnt[nq]) == 0 and bool((ci[nq] == -5).all())  # nothing past the last query
        hs, hi = _bits(cs), ci.cpu().numpy()
        for q in range(nq):
            tot = int(e_cnt[q]) & R.CNT_MASK
            n = min(tot, cap)
            got = sorted(zip(hi[q, :n].tolist(), hs[q, :n].tolist()))
            if tot <= cap:
                assert got == e_filed[q], q
            else:  # which cap of the records were kept depends on the order of the atomics
                pool = list(e_filed[q])
                for g in got:
                    pool.remove(g)  # ValueError: a record the reference never filed (or filed fewer times)
            assert (hi[q, n:] == -5).all(), q  # only min(count, cap) slots written


# ================================================================ lzk_cand_select
SEL_CAP = 16400
SEL_LENS = [16385, 0, 10, 1025, SEL_CAP, 1, 2, 3, 4, 7, 8, 9, 15, 16, 63, 64, 65, 1023, 1024, 16384]
SEL_P = 32771  # prime > cap: (a + p b) mod P is injective in p < P


@functools.lru_cache(maxsize=None)
def _select_case(nq):
    """Lists of one batch size (shared by every kslot / kout): per-query lengths
    from SEL_LENS, counts past cap and counts with bit 30, score kinds by
    q % 4: 9 distinct values (mass ties), 2001 values, Gaussian with -inf
    entries, all -inf. Returns host arrays, device tensors and the top-16
    reference (a prefix of which is the reference of any kout <= 16)."""
    rng = np.random.default_rng(5 + nq)
    cap = SEL_CAP
    lens = np.array([SEL_LENS[q % len(SEL_LENS)] for q in range(nq)], dtype=np.int64)
    cnt = lens.copy()
    for q in range(nq):
        if q % 7 == 2:
            cnt[q] = cap + 7 + q  # overflowed: ovf = 1, the first cap entries are read
            lens[q] = cap
        elif q % 7 == 4 or nq == 1:
            cnt[q] = lens[q] | R.CNT_OVF  # a record region overflowed: ovf = 1, the low 30 bits count
    p = np.arange(cap, dtype=np.int64)[None, :]
    ci = ((rng.integers(0, SEL_P, size=(nq, 1)) + p * rng.integers(1, SEL_P, size=(nq, 1))) % SEL_P).astype(np.int32)
    srt = np.sort(ci, axis=1)
    assert (srt[:, 1:] != srt[:, :-1]).all()  # a row appears once per list
    cs = np.empty((nq, cap), dtype=np.float32)
    for q in range(nq):
        kind = q % 4
        if kind == 0:
            cs[q] = rng.integers(-4, 5, size=cap)
        elif kind == 1:
            cs[q] = rng.integers(-1000, 1001, size=cap)
        elif kind == 2:
            cs[q] = rng.standard_normal(cap)
            cs[q][rng.random(cap) < 0.3] = NEG_INF
        else:
            cs[q] = NEG_INF
        n = int(lens[q])
        cs[q, n:] = np.nan  # slots past the list are never read: nan (which no comparison would select anyway)
        cs[q, n + 1:: 2] = 3e38  # and, every other one, a score that would win
        ci[q, n:] = 3
    ref_s, ref_r, _ = R.select_ref(cnt, cs, ci, cap, 16)
    return cnt, cs, ci, _dev(cnt, torch.int32), _dev(cs), _dev(ci), ref_s, ref_r


@pytest.mark.parametrize("kslot,kout", [(1, 1), (2, 1), (2, 2), (4, 1), (4, 4), (8, 1), (8, 8), (10, 1), (10, 10),
                                        (16, 1), (16, 16)])
@pytest.mark.parametrize("nq", [1, 5, 63, 64, 67, 300])
def test_cand_select_bits_gpu(nq, kslot, kout):
    """nq in {1, 5, 63}: cand_select_block_kernel (a block per query; 16385
    entries force its second 16 x 1024 round); nq in {64, 67, 300}:
    cand_select_kernel (a wave per query). Scores, rows (ties: smaller row
    first; -inf entries as (-inf, -1)) and ovf bit-equal to select_ref, with
    need null / idx_offset 0 and a need mix / idx_offset 2^33 + 5."""
    L = _lib.lib()
    cnt, cs, ci, d_cnt, d_cs, d_ci, ref_s, ref_r = _select_case(nq)
    cap = SEL_CAP
    need = cnt + (np.arange(nq) % 3 - 1)  # cnt - 1, cnt, cnt + 1: the last one is "too few entries"
    d_need = _dev(need, torch.int32)
    for off, nd, d_nd in ((0, None, None), ((1 << 33) + 5, need, d_need)):
        os_ = torch.full((nq + 1, kout), 9.0, device=DEV)
        oi = torch.full((nq + 1, kout), 9, dtype=torch.long, device=DEV)
        ovf = torch.full((nq + 1,), 9, dtype=torch.int32, device=DEV)
        _lib.check(L.lzk_cand_select(d_cnt.data_ptr(), d_cs.data_ptr(), d_ci.data_ptr(), cap, nq, kslot, kout, off,
                                     os_.data_ptr(), oi.data_ptr(), ovf.data_ptr(), _lib.ptr(d_nd), _st()),
                   "lzk_cand_select")
        torch.cuda.synchronize()
        e_ovf = ((cnt > cap) | ((cnt < nd) if nd is not None else False)).astype(np.int32)
        e_r = np.where(ref_r[:, :kout] >= 0, ref_r[:, :kout] + off, -1)
        assert np.array_equal(ovf[:nq].cpu().numpy(), e_ovf)
        assert np.array_equal(_bits(os_[:nq]), _f32bits(ref_s[:, :kout])), (off,)
        assert np.array_equal(oi[:nq].cpu().numpy(), e_r), (off,)
        assert int(ovf[nq]) == 9 and bool((oi[nq] == 9).all())
    if nq >= 5:
        assert e_ovf[2] == 1 and e_ovf[4] == 1 and (e_ovf == 0).any()


# ================================================================ lzk_cand_cut
CUT_NR = 64  # rows allocated (plus one in front); the kernel is told nrows = CUT_NR - 4
CUT_SHAPES = [(1, 10, 16), (63, 10, 16), (64, 10, 16), (130, 10, 16), (5, 17, 32)]


def _rows_table(rng, nq, k, ldr, nrows, with_bias):
    """[nq, ldr] int64 and each query's kind (q % 5): 0 k real rows, 1 a -1 among
    the first k, 2 a row >= nrows (inside the allocation), 3 a row whose bias is
    -inf (row 0), 4 a row whose bias is nan (row 1)."""
    rows = np.stack([rng.permutation(np.arange(2, nrows))[:ldr] for _ in range(nq)]).astype(np.int64)
    for q in range(nq):
        j = int(rng.integers(0, k))
        kind = q % 5
        if kind == 1:
            rows[q, j] = -1
        elif kind == 2:
            rows[q, j] = nrows + int(rng.integers(0, CUT_NR - nrows))
        elif kind == 3 and with_bias:
            rows[q, j] = 0
        elif kind == 4 and with_bias:
            rows[q, j] = 1
    return rows


@functools.lru_cache(maxsize=None)
def _cut_data(D, f32, kind):
    """X [1 + CUT_NR rows, ldx = D + 8] (the kernel sees the view from row 1),
    bias likewise; values as fp64 for the reference."""
    rng = np.random.default_rng(1000 * D + 2 * f32 + (kind == "grid"))
    nqmax = 130
    if kind == "grid":
        X, Q = R.grid_rows(rng, 1 + CUT_NR, D), R.grid_queries(rng, nqmax, D)
        bias = rng.integers(-64, 65, size=1 + CUT_NR).astype(np.float64)
    else:
        X, Q = R.unit_rows(rng, 1 + CUT_NR, D), R.unit_rows(rng, nqmax, D)
        X, Q = (X.astype(np.float32).astype(np.float64), Q.astype(np.float32).astype(np.float64)) if f32 else (
            R.to_bf16(X), R.to_bf16(Q))
        bias = -(X.astype(np.float32) ** 2).sum(1).astype(np.float64)
    bias[1 + 0], bias[1 + 1] = NEG_INF, np.nan
    dt = torch.float32 if f32 else torch.bfloat16
    Xd = torch.zeros((1 + CUT_NR, D + 8), dtype=dt, device=DEV)
    Xd[:, :D] = _dev(X, dt)
    Qd = torch.zeros((nqmax, D + 4), dtype=dt, device=DEV)
    Qd[:, :D] = _dev(Q, dt)
    return X[1:], Q, bias[1:], Xd, Qd, _dev(bias, torch.float32)


@pytest.mark.parametrize("kind", ["grid", "gauss"])
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("f32", [0, 1])
@pytest.mark.parametrize("nq,k,ldr", CUT_SHAPES)
def test_cand_cut_gpu(nq, k, ldr, f32, D, kind):
    """nq in {1, 63} (k <= 16): cand_cut_block_kernel; nq in {64, 130} and
    (nq 5, k 17): cand_cut_kernel. |cut - cut_ref| <= cut_bound (grid: L is
    exact; Gaussian: + score_bound of the minimising row); a missing row, a row
    >= nrows, a -inf or nan bias give -inf, or floor - margin, exactly."""
    L = _lib.lib()
    X, Q, bias, Xd, Qd, bd = _cut_data(D, f32, kind)
    nrows = CUT_NR - 4
    rng = np.random.default_rng(nq + k)
    m = rng.integers(0, 17, size=nq) / 8.0
    d_m = _dev(m, torch.float32)
    Xv, bv = Xd[1:], bd[1:]  # row -1 of the view is allocated
    for with_bias, alpha in ((True, 2.0), (False, 1.0)):
        rows = _rows_table(rng, nq, k, ldr, nrows, with_bias)
        d_rows = _dev(rows)
        Lq, B = R.cut_min_ref(X, Q, bias if with_bias else None, alpha, rows, k, nrows)
        if nq >= 5:
            assert np.isfinite(Lq).any() and (Lq == NEG_INF).sum() >= (4 if with_bias and nq >= 63 else 1)
        fin = Lq[np.isfinite(Lq)]
        for floor in (None, float(np.round(np.median(fin))) if kind == "grid" else float(np.float32(np.median(fin)))):
            cut = torch.full((nq + 1,), 9.0, device=DEV)
            _lib.check(L.lzk_cand_cut(Xv.data_ptr(), Xv.stride(0), nrows, Qd.data_ptr(), Qd.stride(0), D, nq, f32,
                                      bv.data_ptr() if with_bias else None, alpha, d_rows.data_ptr(), ldr, k,
                                      d_m.data_ptr(), 0.0 if floor is None else floor, int(floor is not None),
                                      cut.data_ptr(), _st()), "lzk_cand_cut")
            torch.cuda.synchronize()
            got = cut[:nq].cpu().numpy().astype(np.float64)
            e, eb = R.cut_ref(Lq, m, alpha, floor)
            miss = Lq == NEG_INF
            e_miss = np.full(nq, NEG_INF) if floor is None else (np.float32(floor) - m.astype(np.float32)).astype(
                np.float64)
            assert np.array_equal(got[miss], e_miss[miss])  # -inf, or floor - m (one fp32 subtraction): exact
            tol = eb + (B if kind == "gauss" else 0.0)
            assert (np.abs(got[~miss] - e[~miss]) <= tol[~miss]).all(), float(
                (np.abs(got[~miss] - e[~miss]) / tol[~miss]).max())
            if floor is not None:
                assert (got >= e_miss).all()
            assert float(cut[nq]) == 9.0


# ================================================================ lzk_cand_rescore / lzk_cand_rescore32
RS_NR = 384  # rows; the last two are zero rows with bias = floor and floor - 1 (grid)
K_NEED = 10
NEED_VAL = 4242
RS_LENS = ["cap", "cap+9", 257, 0, 1, 255, 256, "flag"]


def _split(nq):
    return 1 if nq >= 64 else max(1, min(64, 256 // nq))


@functools.lru_cache(maxsize=None)
def _rs_data(D, f32, kind):
    rng = np.random.default_rng(77 * D + 2 * f32 + (kind == "grid"))
    nqmax = 200
    if kind == "grid":
        X, Q = R.grid_rows(rng, RS_NR, D), R.grid_queries(rng, nqmax, D)
        bias = rng.integers(-64, 65, size=RS_NR).astype(np.float64)
        floor = -5.0
        X[-2:] = 0.0
        bias[-2], bias[-1] = floor, floor - 1.0  # exact score == floor (kept) and just below it (dropped)
    else:
        X, Q = R.unit_rows(rng, RS_NR, D), R.unit_rows(rng, nqmax, D)
        X, Q = (X.astype(np.float32).astype(np.float64), Q.astype(np.float32).astype(np.float64)) if f32 else (
            R.to_bf16(X), R.to_bf16(Q))
        bias = -(X.astype(np.float32) ** 2).sum(1).astype(np.float64)
        floor = None  # per (alpha, bias): the median score
    dt = torch.float32 if f32 else torch.bfloat16
    Xd = torch.zeros((RS_NR, D + 8), dtype=dt, device=DEV)
    Xd[:, :D] = _dev(X, dt)
    Qd = torch.zeros((nqmax, D + 4), dtype=dt, device=DEV)
    Qd[:, :D] = _dev(Q, dt)
    return X, Q, bias, floor, Xd, Qd, _dev(bias, torch.float32)


def _rs_lists(rng, nq, cap, s_all, b_all, floor, variant, guard):
    """Hand-built lists of one launch. Per query: tau = a level with rows on
    both sides (grid: the exact score of one listed row; Gaussian: between two
    scores), a planted number of kept entries that reach it -- K_NEED - 1,
    K_NEED, K_NEED + 1, K_NEED + 5, 0, or tau = -inf -- placed 256 entries apart
    where the list is long enough (different blockIdx.y groups of the split
    kernel); entries from rows that reach tau but whose scan score is below the
    cut (not counted), entries AT the cut (kept). Gaussian: rows within
    ``guard`` score bounds of tau or floor are not listed as kept entries."""
    cnt = np.zeros(nq, dtype=np.int64)
    cs = np.full((nq, cap), np.nan, dtype=np.float32)
    ci = np.zeros((nq, cap), dtype=np.int32)
    cut = (100.0 + np.arange(nq) * 0.5).astype(np.float32)
    tau = np.zeros(nq, dtype=np.float32)
    plan = [K_NEED - 1, K_NEED, K_NEED + 1, K_NEED + 5, 0, -1]
    for q in range(nq):
        ln = RS_LENS[(q + variant) % len(RS_LENS)]
        n = cap if ln in ("cap", "cap+9") else (cap - 3 if ln == "flag" else ln)
        cnt[q] = cap + 9 if ln == "cap+9" else (n | R.CNT_OVF if ln == "flag" else n)
        s, b = s_all[q], b_all[q]
        above = np.sort(np.unique(s[s > floor]))
        if guard == 0.0:
            tq = above[len(above) // 2]
            clear = np.ones(RS_NR, dtype=bool)
        else:
            i = len(above) // 2
            tq = float(np.float32(0.5 * (above[i - 1] + above[i])))
            clear = (np.abs(s - tq) > 2 * guard * b) & (np.abs(s - floor) > 2 * guard * b)
        h = plan[(q + variant) % len(plan)]
        tau[q] = NEG_INF if h < 0 else tq
        hit_rows = np.flatnonzero((s >= tq) & clear)
        hit_rows = hit_rows[np.argsort(s[hit_rows], kind="stable")]  # first: the row AT tau (grid)
        other = np.flatnonzero((s < tq) & clear)
        anyrow = np.arange(RS_NR)
        kept = rng.random(n) < 0.3
        ci[q, :n] = np.where(kept, other[rng.integers(0, other.size, size=n)], anyrow[rng.integers(0, RS_NR, size=n)])
        h = max(h, 0)
        hp = np.arange(h) * 256 if (h - 1) * 256 < n else np.arange(min(h, n))
        kept[hp] = True
        ci[q, hp] = hit_rows[np.arange(hp.size) % hit_rows.size]
        if guard == 0.0 and n >= 200:  # grid: the zero rows whose score is the floor / one under it, re-scored
            kept[n - 3: n - 1] = True
            ci[q, n - 3: n - 1] = [RS_NR - 2, RS_NR - 1]
        sc = np.where(kept, cut[q] + rng.integers(0, 3, size=n), cut[q] - rng.integers(1, 4, size=n)).astype(np.float32)
        below = np.flatnonzero(~kept)[:2]
        sc[below] = np.nextafter(cut[q], np.float32(NEG_INF))  # one ulp under the cut: dropped
        cs[q, :n] = sc
    return cnt, cs, ci, cut, tau


def _rescore(L, f32, Xd, Qd, nq, D, bias_d, alpha, cnt, cap, cs, ci, cut, floor, tau, k_need, need_val, need):
    fn, name = (L.lzk_cand_rescore32, "lzk_cand_rescore32") if f32 else (L.lzk_cand_rescore, "lzk_cand_rescore")
    _lib.check(fn(Xd.data_ptr(), Xd.stride(0), Qd.data_ptr(), Qd.stride(0), nq, D, _lib.ptr(bias_d), alpha,
                  cnt.data_ptr(), cap, cs.data_ptr(), ci.data_ptr(), _lib.ptr(cut), floor, _lib.ptr(tau), k_need,
                  need_val, _lib.ptr(need), _st()), name)


RS_CASES = [(nq, D) for nq in (4, 64) for D in DS] + [(nq, D) for nq in (1, 5, 63, 200) for D in (260, 768)]


@pytest.mark.parametrize("kind", ["grid", "gauss"])
@pytest.mark.parametrize("f32", [0, 1])
@pytest.mark.parametrize("nq,D", RS_CASES)
def test_cand_rescore_and_certificate_gpu(nq, D, f32, kind):
    """nq in {1, 4, 5, 63}: cand_rescore4_kernel over split = 64, 64, 51, 4
    blocks per query (lists of 256 split + 300 entries, hits 256 apart, the
    cross-block counters); nq in {64, 200}: cand_rescore_kernel (cap 700).
    f32 = 0: lzk_cand_rescore (bf16 rows), 1: lzk_cand_rescore32. Three launches
    with different plants: two on one stream, one on a second stream -- each
    ``need`` must be right on its own. Then cut null, need null, tau null.
    Grid: bits; Gaussian: |cs - ref| <= score_bound, need predicted from fp64
    with no listed entry within 4 score bounds of tau or floor."""
    L = _lib.lib()
    X, Q, bias, floor_g, Xd, Qd, bd = _rs_data(D, f32, kind)
    split = _split(nq)
    assert split == {1: 64, 4: 64, 5: 51, 63: 4, 64: 1, 200: 1}[nq]
    cap = 256 * split + 300 if split > 1 else 700
    rng = np.random.default_rng(9 * nq + D)
    guard = 0.0 if kind == "grid" else 4.0
    side = torch.cuda.Stream()
    seen = set()
    for variant in range(3):
        alpha, b, b_d = (2.0, bias, bd) if variant < 2 else (1.0, None, None)
        sb = [R.score_ref(X, Q[q], np.arange(RS_NR), b, alpha) for q in range(nq)]
        s_all, b_all = np.stack([v[0] for v in sb]), np.stack([v[1] for v in sb])
        floor = floor_g if kind == "grid" else float(np.float32(np.median(s_all)))
        cnt, cs, ci, cut, tau = _rs_lists(rng, nq, cap, s_all, b_all, floor, variant, guard)
        ref = R.rescore_ref(X, Q, b, alpha, cnt, cs, ci, cap, cut, floor, tau, K_NEED, NEED_VAL, guard=guard)
        assert int(ref["near"].sum()) == 0  # no decision a correct fp32 kernel could take either way
        seen.update(int(h) for h in ref["hits"])
        d_cnt, d_cs, d_ci, d_cut, d_tau = _dev(cnt, torch.int32), _dev(cs), _dev(ci), _dev(cut), _dev(tau)
        need = torch.full((nq + 1,), -7, dtype=torch.int32, device=DEV)
        if variant == 2:
            side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side if variant == 2 else torch.cuda.current_stream()):
            _rescore(L, f32, Xd, Qd, nq, D, b_d, alpha, d_cnt, cap, d_cs, d_ci, d_cut, floor, d_tau, K_NEED, NEED_VAL,
                     need)
        torch.cuda.synchronize()
        _check_rescore(kind, d_cs, cs, ref, cnt, cap)
        assert np.array_equal(need[:nq].cpu().numpy(), ref["need"]), (variant, ref["hits"].tolist())
        assert int(need[nq]) == -7
        if variant == 0:
            # cut null: every entry re-scored; need null: nothing written; tau null + need: certified
            for mode in ("cut null", "need null", "tau null"):
                d_cs2 = _dev(cs)
                need2 = torch.full((nq + 1,), -7, dtype=torch.int32, device=DEV)
                c_ = None if mode == "cut null" else d_cut
                t_ = None if mode == "tau null" else d_tau
                n_ = None if mode == "need null" else need2
                _rescore(L, f32, Xd, Qd, nq, D, b_d, alpha, d_cnt, cap, d_cs2, d_ci, c_, floor, t_, K_NEED, NEED_VAL, n_)
                torch.cuda.synchronize()
                r2 = R.rescore_ref(X, Q, b, alpha, cnt, cs, ci, cap, None if c_ is None else cut, floor,
                                   None if t_ is None else tau, K_NEED, NEED_VAL, want_need=n_ is not None, guard=guard)
                if mode == "cut null" and kind == "gauss":
                    # every entry is re-scored here, also rows near tau / floor: compare scores only where clear
                    _check_rescore(kind, d_cs2, cs, r2, cnt, cap, loose_floor=floor)
                    continue
                _check_rescore(kind, d_cs2, cs, r2, cnt, cap)
                if n_ is None:
                    assert bool((need2 == -7).all())
                else:
                    assert np.array_equal(need2[:nq].cpu().numpy(), r2["need"]), mode
                    if mode == "tau null":
                        assert (r2["need"] == 0).all()
    assert {K_NEED - 1, K_NEED, K_NEED + 1} <= seen, seen  # one short of, at and one past the certificate's count


def _check_rescore(kind, d_cs, cs_in, ref, cnt, cap, loose_floor=None):
    got = d_cs.cpu().numpy()
    nq = len(cnt)
    for q in range(nq):
        n = min(int(cnt[q]) & R.CNT_MASK, cap)
        assert np.array_equal(got[q, n:].view(np.int32), cs_in[q, n:].view(np.int32)), q  # past the list: untouched
        g, e, b = got[q, :n].astype(np.float64), ref["cs"][q, :n], ref["bound"][q, :n]
        if kind == "grid":
            assert np.array_equal(got[q, :n].view(np.int32), _f32bits(e)), q
            continue
        if loose_floor is not None:  # entries within 4 bounds of the floor may fall on either side of it
            amb = np.abs(ref["exact"][q, :n] - loose_floor) <= 4.0 * b
            sel = ~amb
            g, e, b = g[sel], e[sel], b[sel]
        dead = e == NEG_INF
        assert np.array_equal(g == NEG_INF, dead), q
        assert (np.abs(g[~dead] - e[~dead]) <= b[~dead]).all(), q
