"""The filtered IVF-PQ kernels -- ``lzk_ivfpq_filter_rows``
(csrc/kernels/ivfpq_filter.hip) and ``lzk_ivfpq_scan_f`` / ``_scan_deep_f`` /
``_scan_thresh_f`` (csrc/kernels/ivfpq.hip) -- called directly on crafted
tensors and held against tests/kernels/_ivfpq_filter_ref.py, then the index
and the TenantGraph route built on them.

Inputs and layout are those of test_ivfpq_scan_gpu.py: lists of 0, 1, 3, 63,
255, 256, 257 and 700 rows (+ the 5,120-row list for the deep scan), probes
with a -1, exact-grid tables compared bit for bit (tie order and ``(-inf, -1)``
padding included), Gaussian tables held to ``pq_bound``. Every output is
sentinel-filled with a guard region behind it.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from lazzaro_amd.index.ivfpq import IVFPQIndex  # noqa: E402  (registers the entry points' signatures)
from lazzaro_amd.ops import _lib  # noqa: E402
from tests.kernels import _filtered_tenant as T  # noqa: E402
from tests.kernels import _ivfpq_filter_ref as FR  # noqa: E402
from tests.kernels import _ivfpq_ref as R  # noqa: E402

DEV = "cuda"
NQ, NPROBE = 3, 4
PROBES = np.array([[7, -1, 0, 1], [6, 5, 7, 2], [4, 3, 7, 6]], dtype=np.int32)
PROBES_DEEP = np.array([[8, -1, 0, 1], [6, 5, 7, 8], [4, 3, 7, 6]], dtype=np.int32)
SENT_F, SENT_I = 12345.5, -7  # no grid score is fractional, no row negative but -1
GUARD = 64
INVALID = 1  # hipErrorInvalidValue


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _st():
    return _lib.stream_ptr(torch.device(DEV))


def _outs(n, idt=torch.int32):
    return (torch.full((n + GUARD,), SENT_F, dtype=torch.float32, device=DEV),
            torch.full((n + GUARD,), SENT_I, dtype=idt, device=DEV))


def _untouched(os_, oi, start=0):
    return bool((os_[start:] == SENT_F).all()) and bool((oi[start:] == SENT_I).all())


def _same_bits(got32: np.ndarray, want64: np.ndarray) -> bool:
    return np.array_equal(got32.view(np.int32), want64.astype(np.float32).view(np.int32))


# ------------------------------------------------------------------ lzk_ivfpq_filter_rows
NLIST_B = 9


def _build_case(n_codes: int, kind: int):
    """pos: a random permutation; vids: ids inside the allow column, -1 and
    ids past it; lists: a random split of the code rows with empty lists."""
    rng = np.random.default_rng(100 * n_codes + kind)
    n_ids = max(4, (2 * n_codes) // 3)
    pos = rng.permutation(n_codes).astype(np.int64)
    vids = rng.integers(0, n_ids, size=n_codes).astype(np.int64)
    vids[rng.random(n_codes) < 0.1] = -1
    vids[rng.random(n_codes) < 0.1] = n_ids + rng.integers(0, 5)
    vids[rng.random(n_codes) < 0.03] = np.iinfo(np.int64).max
    if kind == FR.KIND_U8:
        allow = rng.choice(np.array([0, 0, 1, 7, 255], dtype=np.uint8), size=n_ids)
        allow[0] = 1
    else:
        allow = rng.choice(np.array([-np.inf, -np.inf, 0.0, -0.0, -3.0e38, 2.5], dtype=np.float32), size=n_ids)
        allow[0] = -1.0
    vids[pos[0]] = 0  # code row 0 passes: the count is never 0
    cuts = np.sort(rng.integers(0, n_codes + 1, size=NLIST_B - 1))
    cuts[2] = cuts[1]  # an empty list inside
    off = np.concatenate([[0], np.sort(cuts), [n_codes]]).astype(np.int64)
    return pos, vids, allow, off, n_ids


def _filter_rows(pos, vids, allow, kind, n_ids, off, max_rows, n_codes):
    L = _lib.lib()
    frows = torch.full((max_rows + GUARD,), SENT_I, dtype=torch.int32, device=DEV)
    foff = torch.full((NLIST_B + 1 + GUARD,), SENT_I, dtype=torch.int64, device=DEV)
    ws = torch.zeros(int(L.lzk_ivfpq_filter_rows_ws(n_codes)) + GUARD, dtype=torch.int32, device=DEV)
    ws[-GUARD:] = SENT_I
    d = [_dev(a) for a in (pos, vids, allow, off)]
    rc = L.lzk_ivfpq_filter_rows(d[0].data_ptr(), d[1].data_ptr(), n_codes, d[2].data_ptr(), kind, n_ids,
                                 d[3].data_ptr(), NLIST_B, max_rows, frows.data_ptr(), foff.data_ptr(),
                                 ws.data_ptr(), _st())
    torch.cuda.synchronize()
    assert bool((ws[-GUARD:] == SENT_I).all())
    return rc, frows.cpu().numpy(), foff.cpu().numpy()


@pytest.mark.parametrize("kind", (FR.KIND_U8, FR.KIND_BIAS))
@pytest.mark.parametrize("n_codes", (1, 63, 64, 65, 1535))
def test_filter_rows_exact(n_codes, kind):
    pos, vids, allow, off, n_ids = _build_case(n_codes, kind)
    fr, fo, cnt = FR.filter_rows_ref(pos, vids, allow, kind, off)
    assert 1 <= cnt <= n_codes and (n_codes < 63 or cnt < n_codes)
    rc, frows, foff = _filter_rows(pos, vids, allow, kind, n_ids, off, n_codes, n_codes)
    assert rc == 0
    assert np.array_equal(frows[:cnt], fr) and (frows[cnt:] == SENT_I).all()
    assert np.array_equal(foff[: NLIST_B + 1], fo) and (foff[NLIST_B + 1:] == SENT_I).all() and foff[NLIST_B] == cnt


@pytest.mark.parametrize("kind", (FR.KIND_U8, FR.KIND_BIAS))
@pytest.mark.parametrize("n_codes", (1, 63, 64, 65, 1535))
def test_filter_rows_overflow(n_codes, kind):
    """``max_rows`` below the count: the list stops there, nothing lands at
    or past ``frows[max_rows]``, every offset stops at ``max_rows``."""
    pos, vids, allow, off, n_ids = _build_case(n_codes, kind)
    cnt = FR.filter_rows_ref(pos, vids, allow, kind, off)[2]
    for max_rows in sorted({0, cnt // 2, cnt - 1}):
        fr, fo, _ = FR.filter_rows_ref(pos, vids, allow, kind, off, max_rows)
        assert max_rows < cnt and fo.max() == max_rows == fo[-1]
        rc, frows, foff = _filter_rows(pos, vids, allow, kind, n_ids, off, max_rows, n_codes)
        assert rc == 0
        assert np.array_equal(frows[:max_rows], fr) and (frows[max_rows:] == SENT_I).all()
        assert np.array_equal(foff[: NLIST_B + 1], fo) and (foff[NLIST_B + 1:] == SENT_I).all()


def test_filter_rows_rejections():
    pos, vids, allow, off, n_ids = _build_case(65, 0)
    L = _lib.lib()
    d = [_dev(a) for a in (pos, vids, allow, off)]
    frows = torch.full((65 + GUARD,), SENT_I, dtype=torch.int32, device=DEV)
    foff = torch.full((NLIST_B + 1 + GUARD,), SENT_I, dtype=torch.int64, device=DEV)
    ws = torch.zeros(8, dtype=torch.int32, device=DEV)

    def call(pos_=d[0], vids_=d[1], allow_=d[2], kind=0, off_=d[3], frows_=frows, foff_=foff, ws_=ws, n=65, cap=65):
        rc = L.lzk_ivfpq_filter_rows(_lib.ptr(pos_), _lib.ptr(vids_), n, _lib.ptr(allow_), kind, n_ids, _lib.ptr(off_),
                                     NLIST_B, cap, _lib.ptr(frows_), _lib.ptr(foff_), _lib.ptr(ws_), _st())
        torch.cuda.synchronize()
        return rc
    for what, kw in {"no pos": dict(pos_=None), "no vids": dict(vids_=None), "no allow": dict(allow_=None),
                     "allow_kind 2": dict(kind=2), "no list_off": dict(off_=None), "no frows": dict(frows_=None),
                     "no foff": dict(foff_=None), "no workspace": dict(ws_=None), "n_codes < 0": dict(n=-1),
                     "n_codes 2^31": dict(n=1 << 31), "max_rows < 0": dict(cap=-1)}.items():
        assert call(**kw) == INVALID, what
        assert bool((frows == SENT_I).all()) and bool((foff == SENT_I).all()), what


# ------------------------------------------------------------------ shared scan inputs
@functools.lru_cache(maxsize=None)
def _case(kind: str, M: int, deep: bool = False):
    """The inputs of test_ivfpq_scan_gpu.py's ``_case`` (same seeds)."""
    rng = np.random.default_rng((17 if kind == "grid" else 23) * 1000 + M + deep)
    off = R.layout(R.LIST_SIZES + ((R.DEEP_LIST,) if deep else ()))
    if kind == "grid":
        codes = R.grid_codes(rng, off, M)
        lut, coarse = R.grid_lut(rng, NQ, NPROBE, M)
    else:
        codes, lut, coarse = R.gauss_inputs(rng, off, NQ, NPROBE, M)
    probes = PROBES_DEEP if deep else PROBES
    c = dict(M=M, off=off, codes=codes, lut=lut, coarse=coarse, probes=probes)
    c["d"] = {k: _dev(c[k]) for k in ("off", "codes", "lut", "coarse", "probes")}
    return c


def _mask(c, what: str, seed: int = 0) -> np.ndarray:
    n = c["codes"].shape[0]
    rng = np.random.default_rng(seed + 7)
    if what == "all":
        return np.ones(n, dtype=bool)
    if what == "none":
        return np.zeros(n, dtype=bool)
    if what == "half":
        return rng.random(n) < 0.5
    if what == "1in64":
        m = np.zeros(n, dtype=bool)
        m[5::64] = True  # (row 5: in the 63-row list's span too)
        return m
    raise KeyError(what)


class Lists:
    """(frows, foff) of a mask over the code rows, on the host and the device
    (the device row list is never empty: a few spare entries follow it)."""

    def __init__(self, c, mask):
        self.mask = mask
        self.fr, self.fo = FR.lists_of_mask(mask, c["off"])
        self.d_fr = _dev(np.concatenate([self.fr, np.zeros(GUARD, dtype=np.int32)]))
        self.d_fo = _dev(self.fo)
        assert self.d_fr.dtype == torch.int32 and self.d_fo.dtype == torch.int64


def _scan_f(c, ls, kslot, frows=True, foff=True):
    d = c["d"]
    n = NQ * NPROBE * kslot
    os_, oi = _outs(n)
    rc = _lib.lib().lzk_ivfpq_scan_f(d["codes"].data_ptr(), ls.d_fo.data_ptr() if foff else 0,
                                     ls.d_fr.data_ptr() if frows else 0, d["probes"].data_ptr(),
                                     d["coarse"].data_ptr(), d["lut"].data_ptr(), NQ, NPROBE, c["M"], kslot,
                                     os_.data_ptr(), oi.data_ptr(), _st())
    torch.cuda.synchronize()
    return rc, os_, oi


def _scan_plain(c, kslot):
    d = c["d"]
    n = NQ * NPROBE * kslot
    os_, oi = _outs(n)
    rc = _lib.lib().lzk_ivfpq_scan(d["codes"].data_ptr(), d["off"].data_ptr(), d["probes"].data_ptr(),
                                   d["coarse"].data_ptr(), d["lut"].data_ptr(), NQ, NPROBE, c["M"], kslot,
                                   os_.data_ptr(), oi.data_ptr(), _st())
    torch.cuda.synchronize()
    return rc, os_, oi


@functools.lru_cache(maxsize=None)
def _scan_f16(M: int, what: str):
    c = _case("grid", M)
    ls = Lists(c, _mask(c, what))
    return ls, FR.scan_f_ref(c["codes"], ls.fo, ls.fr, c["probes"], c["coarse"], c["lut"], 16)


@functools.lru_cache(maxsize=None)
def _scan32(M: int):
    c = _case("grid", M)
    return R.scan_ref(c["codes"], c["off"], c["probes"], c["coarse"], c["lut"], 32)


# ------------------------------------------------------------------ lzk_ivfpq_scan_f
@pytest.mark.parametrize("what", ("all", "none", "half", "1in64"))
@pytest.mark.parametrize("kslot", (1, 4, 10, 16))
@pytest.mark.parametrize("M", (8, 64, 128))
def test_scan_f_exact(M, kslot, what):
    c = _case("grid", M)
    ls, (S, Rw) = _scan_f16(M, what)
    n = NQ * NPROBE * kslot
    rc, os_, oi = _scan_f(c, ls, kslot)
    assert rc == 0 and _untouched(os_, oi, n)
    got_s = os_[:n].cpu().numpy().reshape(NQ, NPROBE, kslot)
    got_r = oi[:n].cpu().numpy().reshape(NQ, NPROBE, kslot)
    assert np.array_equal(got_r, Rw[..., :kslot]), (got_r, Rw[..., :kslot])
    assert _same_bits(got_s, S[..., :kslot])
    assert ls.mask[got_r[got_r >= 0]].all()
    if what == "all":  # the unfiltered kernel's output, bit for bit
        rc0, os0, oi0 = _scan_plain(c, kslot)
        assert rc0 == 0 and torch.equal(oi0, oi) and torch.equal(os0.view(torch.int32), os_.view(torch.int32))
    if what == "none":
        assert (got_r == -1).all() and np.isneginf(got_s).all()
    if what == "1in64":  # lists of 1 or 2 passing rows: mostly padding, rows reported as code rows
        assert int((got_r[0, 0] >= 0).sum()) == min(kslot, 11) and (got_r[0, 0][got_r[0, 0] >= 0] % 64 == 5).all()


@pytest.mark.parametrize("kslot", (1, 4, 10, 16))
@pytest.mark.parametrize("M", (8, 64, 128))
def test_scan_f_without_each_lists_top_k(M, kslot):
    """The mask clears exactly the unfiltered top-K of every list a query
    probes: the filtered scan returns ranks K+1..2K of the unfiltered order."""
    c = _case("grid", M)
    S32, R32 = _scan32(M)
    n = NQ * NPROBE * kslot
    for q in range(NQ):
        mask = np.ones(c["codes"].shape[0], dtype=bool)
        top = R32[q, :, :kslot]
        mask[top[top >= 0]] = False
        ls = Lists(c, mask)
        rc, os_, oi = _scan_f(c, ls, kslot)
        assert rc == 0 and _untouched(os_, oi, n)
        got_s = os_[:n].cpu().numpy().reshape(NQ, NPROBE, kslot)[q]
        got_r = oi[:n].cpu().numpy().reshape(NQ, NPROBE, kslot)[q]
        assert np.array_equal(got_r, R32[q, :, kslot:2 * kslot]), (q, got_r)
        assert _same_bits(got_s, S32[q, :, kslot:2 * kslot])


@pytest.mark.parametrize("M", (8, 64, 128))
def test_scan_f_gaussian_bound(M):
    c = _case("gauss", M)
    K = 16
    ls = Lists(c, _mask(c, "half", seed=M))
    rc, os_, oi = _scan_f(c, ls, K)
    assert rc == 0
    got_s = os_[: NQ * NPROBE * K].cpu().numpy().reshape(NQ, NPROBE, K)
    got_r = oi[: NQ * NPROBE * K].cpu().numpy().reshape(NQ, NPROBE, K)
    worst = 0.0
    for q in range(NQ):
        for p in range(NPROBE):
            l = int(c["probes"][q, p])
            pr = ls.fr[ls.fo[l]:ls.fo[l + 1]].astype(np.int64) if l >= 0 else np.zeros(0, dtype=np.int64)
            nv = min(K, pr.size)
            s, r = got_s[q, p], got_r[q, p]
            assert (r[nv:] == -1).all() and np.isneginf(s[nv:]).all()
            if nv == 0:
                continue
            rows = r[:nv].astype(np.int64)
            assert np.isin(rows, pr).all() and np.unique(rows).size == nv
            assert np.array_equal(R.order(s[:nv].astype(np.float64), rows), np.arange(nv))
            s64 = R.pq_scores(c["codes"][pr], c["lut"][q], c["coarse"][q, p])
            bd = R.pq_bound(c["codes"][pr], c["lut"][q], c["coarse"][q, p])
            at = np.searchsorted(pr, rows)
            err = np.abs(s[:nv].astype(np.float64) - s64[at])
            worst = max(worst, float((err / bd[at]).max()))
            assert (err <= bd[at]).all(), (q, p, err, bd[at])
            out = np.ones(pr.size, dtype=bool)
            out[at] = False
            if out.any():
                assert (s64[out] - bd[out]).max() <= (s64[at] + bd[at]).min()
    print(f"scan_f M={M}: worst |err| / bound = {worst:.3g}")


# ------------------------------------------------------------------ lzk_ivfpq_scan_deep_f
def _deep_f(c, ls, frows=True, foff=True):
    d = c["d"]
    W = _lib.lib().lzk_ivfpq_deep_width()
    n = NQ * NPROBE * W
    os_, oi = _outs(n)
    rc = _lib.lib().lzk_ivfpq_scan_deep_f(d["codes"].data_ptr(), ls.d_fo.data_ptr() if foff else 0,
                                          ls.d_fr.data_ptr() if frows else 0, d["probes"].data_ptr(),
                                          d["coarse"].data_ptr(), d["lut"].data_ptr(), NQ, NPROBE, c["M"],
                                          os_.data_ptr(), oi.data_ptr(), _st())
    torch.cuda.synchronize()
    return rc, os_, oi, W


@pytest.mark.parametrize("what", ("half", "few", "none"))
@pytest.mark.parametrize("M", (8, 32, 128))
def test_scan_deep_f_exact(M, what):
    """'few': the 5,120-row list keeps 100 rows -- positions 0..99 of the
    filtered list belong to threads 0..99, so waves 2 and 3 emit only -1."""
    c = _case("grid", M, True)
    if what == "few":
        mask = _mask(c, "half", seed=1)
        a, b = int(c["off"][8]), int(c["off"][9])
        mask[a:b] = False
        mask[a + np.random.default_rng(M).choice(b - a, 100, replace=False)] = True
    else:
        mask = _mask(c, what)
    ls = Lists(c, mask)
    rc, os_, oi, W = _deep_f(c, ls)
    n = NQ * NPROBE * W
    assert rc == 0 and _untouched(os_, oi, n)
    SD, RD = FR.deep_f_ref(c["codes"], ls.fo, ls.fr, c["probes"], c["coarse"], c["lut"], W)
    got_s = os_[:n].cpu().numpy().reshape(NQ, NPROBE, 4, W // 4)
    got_r = oi[:n].cpu().numpy().reshape(NQ, NPROBE, 4, W // 4)
    assert np.array_equal(got_r, RD)
    assert _same_bits(got_s, SD)
    assert mask[got_r[got_r >= 0]].all()
    big = got_r[0, 0]  # query 0 probes the 5,120-row list first
    if what == "few":
        assert [int((big[w] >= 0).sum()) for w in range(4)] == [64, 36, 0, 0]
    elif what == "half":  # ~2,560 passing rows, 10 per thread: every wave's segment is full
        assert (big >= 0).all()
    else:
        assert (got_r == -1).all() and np.isneginf(got_s).all()


# ------------------------------------------------------------------ lzk_ivfpq_scan_thresh_f
def _thresh_f(c, ls, thr, cap, frows=True, foff=True):
    d = c["d"]
    os_, oi = _outs(NQ * cap)
    cnt = torch.zeros(NQ, dtype=torch.int32, device=DEV)
    t = _dev(np.asarray(thr, dtype=np.float32))
    rc = _lib.lib().lzk_ivfpq_scan_thresh_f(d["codes"].data_ptr(), ls.d_fo.data_ptr() if foff else 0,
                                            ls.d_fr.data_ptr() if frows else 0, d["probes"].data_ptr(),
                                            d["coarse"].data_ptr(), d["lut"].data_ptr(), t.data_ptr(), NQ, NPROBE,
                                            c["M"], cap, cnt.data_ptr(), os_.data_ptr(), oi.data_ptr(), _st())
    torch.cuda.synchronize()
    return rc, cnt.cpu().numpy(), os_, oi


def _thresh_lists(c, M):
    """Half of the rows pass -- among them the 700-row list's four tied rows."""
    mask = _mask(c, "half", seed=2 * M)
    ties = int(c["off"][7]) + np.array([300, 301, 364, 556])
    mask[ties] = True
    return Lists(c, mask), ties


@pytest.mark.parametrize("thr_kind", ("ninf", "tie"))
@pytest.mark.parametrize("M", (8, 48, 128))
def test_scan_thresh_f_exact(M, thr_kind):
    c = _case("grid", M)
    ls, ties = _thresh_lists(c, M)
    cap = 1600
    if thr_kind == "ninf":
        thr = np.full(NQ, -np.inf)
    else:  # per query the score of the four tied rows: '>' for '>=' would lose them
        thr = np.array([R.pq_scores(c["codes"][ties[:1]], c["lut"][q],
                                    c["coarse"][q, int(np.nonzero(c["probes"][q] == 7)[0][0])])[0] for q in range(NQ)])
    want = FR.thresh_f_ref(c["codes"], ls.fo, ls.fr, c["probes"], c["coarse"], c["lut"], thr)
    rc, cnt, os_, oi = _thresh_f(c, ls, thr, cap)
    assert rc == 0 and _untouched(os_, oi, NQ * cap)
    s_all, r_all = os_[: NQ * cap].cpu().numpy().reshape(NQ, cap), oi[: NQ * cap].cpu().numpy().reshape(NQ, cap)
    for q in range(NQ):
        wr, ws = want[q]
        if thr_kind == "tie":
            assert int((ws == thr[q]).sum()) >= 4 and np.isin(ties, wr).all() and wr.size < cap
        else:  # everything that passes in the probed lists, nothing else
            passing = sum(int(ls.fo[l + 1] - ls.fo[l]) for l in c["probes"][q] if l >= 0)
            assert wr.size == passing and 300 < passing < 701 * 2
        assert cnt[q] == wr.size
        o = np.argsort(r_all[q, : cnt[q]], kind="stable")
        assert np.array_equal(r_all[q, : cnt[q]][o], wr)
        assert _same_bits(s_all[q, : cnt[q]][o], ws)
        assert ls.mask[wr].all()
        assert (s_all[q, cnt[q]:] == SENT_F).all() and (r_all[q, cnt[q]:] == SENT_I).all()


@pytest.mark.parametrize("M", (8, 48, 128))
def test_scan_thresh_f_overflow(M):
    """cap below the qualifying count: ``cnt`` runs on, the cap slots hold
    distinct qualifying passing rows with their scores, nothing past them."""
    c = _case("grid", M)
    ls, _ = _thresh_lists(c, M)
    cap = 100
    args = (c["codes"], ls.fo, ls.fr, c["probes"], c["coarse"], c["lut"])
    thr = np.array([np.sort(s)[-300] for _, s in FR.thresh_f_ref(*args, np.full(NQ, -np.inf))])
    want = FR.thresh_f_ref(*args, thr)
    rc, cnt, os_, oi = _thresh_f(c, ls, thr, cap)
    assert rc == 0 and _untouched(os_, oi, NQ * cap)
    s_all, r_all = os_[: NQ * cap].cpu().numpy().reshape(NQ, cap), oi[: NQ * cap].cpu().numpy().reshape(NQ, cap)
    for q in range(NQ):
        wr, ws = want[q]
        assert cap < 300 <= wr.size and cnt[q] == wr.size
        rows = r_all[q]
        assert np.unique(rows).size == cap and np.isin(rows, wr).all()
        assert _same_bits(s_all[q], ws[np.searchsorted(wr, rows)])


# ------------------------------------------------------------------ rejections
def test_filtered_scans_refuse_missing_lists():
    c = _case("grid", 16)
    ls = Lists(c, _mask(c, "half"))
    for kw in (dict(frows=False), dict(foff=False), dict(frows=False, foff=False)):
        rc, os_, oi = _scan_f(c, ls, 10, **kw)
        assert rc == INVALID and _untouched(os_, oi), kw
        rc, os_, oi, _ = _deep_f(c, ls, **kw)
        assert rc == INVALID and _untouched(os_, oi), kw
        rc, cnt, os_, oi = _thresh_f(c, ls, np.full(NQ, -np.inf), 64, **kw)
        assert rc == INVALID and (cnt == 0).all() and _untouched(os_, oi), kw
    rc, os_, oi = _scan_f(c, ls, 10)  # (the same call with both lists runs)
    assert rc == 0 and not _untouched(os_, oi)


# ------------------------------------------------------------------ the index on top
def _crowded(n, d, seed):
    """Unit rows, five in six of them within a small cap around one direction."""
    g = torch.Generator().manual_seed(seed)
    u = torch.nn.functional.normalize(torch.randn(1, d, generator=g), dim=1)
    x = torch.randn(n, d, generator=g)
    x[: n * 5 // 6] = u + 0.1 * x[: n * 5 // 6] / d ** 0.5
    return torch.nn.functional.normalize(x[torch.randperm(n, generator=g)], dim=1)


@pytest.fixture(scope="module")
def crowded_index():
    """The crowded index of test_ivfpq_scan_gpu.py and a mask over its ids
    that half of them pass; ids past the mask's end fail."""
    n, d = 6000, 64
    idx = IVFPQIndex(d, nlist=8, m=8, device=DEV, keep_vectors="int8")
    x = _crowded(n, d, 11).to(DEV)
    idx.train(x, iters=2)
    idx.add(x)
    idx._finalize()
    sizes = (idx.list_off[1:] - idx.list_off[:-1]).cpu().numpy()
    assert sizes.sum() == n and sizes.max() >= n // 2, sizes
    big = int(sizes.argmax())
    others = [l for l in range(8) if l != big]
    probes = np.array([[big, others[0], -1, others[1]], [others[2], big, others[3], others[4]],
                       [others[5], others[6], others[0], big]], dtype=np.int32)
    rng = np.random.default_rng(3)
    lut = rng.integers(-1024, 1025, size=(NQ, 8, 256)).astype(np.float32)
    coarse = rng.integers(-1024, 1025, size=(NQ, NPROBE)).astype(np.float32)
    mask = rng.random(n - 200) < 0.5
    ci = dict(idx=idx, codes=idx.codes.cpu().numpy(), off=idx.list_off.cpu().numpy(), probes=probes, lut=lut,
              coarse=coarse, mask=mask)
    ci["fr"], ci["fo"], ci["count"] = FR.filter_rows_ref(idx._pos[: idx.n].cpu().numpy(), idx._vids.cpu().numpy(),
                                                         mask.astype(np.uint8), FR.KIND_U8, ci["off"])
    assert ci["fo"][big + 1] - ci["fo"][big] > 1024  # more passing rows in one list than its deep pool holds
    return ci


@pytest.mark.parametrize("kind", ("bool", "bias"))
def test_index_filter_rows_gpu(crowded_index, kind):
    ci = crowded_index
    idx = ci["idx"]
    m = torch.from_numpy(ci["mask"])
    allow = m if kind == "bool" else torch.where(m, torch.zeros(m.numel()), torch.tensor(float("-inf")))
    fl = idx.filter_rows(allow.to(DEV))
    torch.cuda.synchronize()
    assert fl.gen == idx.order_gen and fl.rows.dtype == torch.int32 and fl.rows.numel() == idx.n
    assert np.array_equal(fl.off.cpu().numpy(), ci["fo"])
    assert np.array_equal(fl.rows[: ci["count"]].cpu().numpy(), ci["fr"])
    tight = idx.filter_rows(allow.to(DEV), max_rows=ci["count"])  # the exact count: nothing is cut
    assert tight.rows.numel() == ci["count"] and np.array_equal(tight.rows.cpu().numpy(), ci["fr"])
    assert np.array_equal(tight.off.cpu().numpy(), ci["fo"])


@pytest.mark.parametrize("k", (1, 7, 10, 16))
def test_filtered_scan_gpu_is_the_exact_filtered_topk(crowded_index, k):
    ci = crowded_index
    fl = ci["idx"].filter_rows(torch.from_numpy(ci["mask"]).to(DEV))
    S, Rw = FR.scan_f_ref(ci["codes"], ci["fo"], ci["fr"], ci["probes"], ci["coarse"], ci["lut"], k)
    want_s, want_r = R.merge_topk(S, Rw, k)
    s, r = ci["idx"]._scan_gpu(_dev(ci["probes"]), _dev(ci["coarse"]), _dev(ci["lut"]), k, fl)
    torch.cuda.synchronize()
    assert np.array_equal(r.cpu().numpy(), want_r)
    assert _same_bits(s.cpu().numpy(), want_s)
    # ... which is the unfiltered full ranking with the failing rows dropped
    Sa, Ra = R.scan_ref(ci["codes"], ci["off"], ci["probes"], ci["coarse"], ci["lut"], 6000)
    full_s, full_r = R.merge_topk(Sa, Ra, 3 * 6000)
    passing = np.zeros(6000, dtype=bool)
    passing[ci["fr"]] = True
    for q in range(NQ):
        keep = (full_r[q] >= 0) & passing[np.maximum(full_r[q], 0)]
        assert np.array_equal(full_r[q][keep][:k], want_r[q])


def test_filtered_scan_candidates_hold_the_exact_filtered_top_r(crowded_index):
    ci = crowded_index
    Rn = 600
    idx = ci["idx"]
    fl = idx.filter_rows(torch.from_numpy(ci["mask"]).to(DEV), max_rows=ci["count"])
    W = _lib.lib().lzk_ivfpq_deep_width()
    args = (ci["codes"], ci["fo"], ci["fr"], ci["probes"], ci["coarse"], ci["lut"])
    S, Rw = FR.scan_f_ref(*args, Rn)
    want_s, want_r = R.merge_topk(S, Rw, Rn)
    thr, _ = R.merge_topk(*FR.deep_f_ref(*args, W), Rn)
    counts = [r.size for r, _ in FR.thresh_f_ref(*args, thr[:, Rn - 1])]
    s, r = idx._scan_candidates(_dev(ci["probes"]), _dev(ci["coarse"]), _dev(ci["lut"]), Rn, fl)
    torch.cuda.synchronize()
    assert idx.last_candidates.cpu().tolist() == counts and min(counts) >= Rn
    s, r = s.cpu().numpy(), r.cpu().numpy()
    assert _same_bits(s, want_s)  # torch.topk leaves the order among equal scores open: rows per score level
    passing = np.zeros(6000, dtype=bool)
    passing[ci["fr"]] = True
    for q in range(NQ):
        assert np.unique(r[q]).size == Rn and (r[q] >= 0).all() and passing[r[q]].all()
        last = want_s[q, -1]
        assert set(r[q][s[q] > last].tolist()) == set(want_r[q][want_s[q] > last].tolist())
    # the public forms: ids of the filtered top-R, every one passing
    q = idx.centroids[int(ci["probes"][0, 0])][None, :] + 0.0  # the crowded list's centroid: that list is probed
    ids = idx.candidate_ids(q, Rn, 4, allow=fl)
    m = np.concatenate([ci["mask"], np.zeros(200, dtype=bool)])
    got = ids.cpu().numpy()
    assert (got >= 0).all() and m[got].all() and np.unique(got[0]).size == Rn
    s10, i10 = idx.search(q, 10, nprobe=4, rerank=Rn, allow=fl)
    assert m[i10.cpu().numpy()].all()


# ------------------------------------------------------------------ the tenant graph's route
def test_tenant_graph_filtered_route_equals_flat_gpu(monkeypatch):
    from lazzaro_amd.engine import tenant_graph as TG
    monkeypatch.setattr(TG, "FILTER_SPARSE_MAX_ROWS", 0)
    steps = []
    for step, g, (s1, r1), t, (s2, r2) in T.run(DEV):
        torch.cuda.synchronize()
        steps.append(step)
        assert g.filtered_ann == len(steps) and t.filtered_ann == 0, step
        assert g.filtered_sparse == 0 and g._ann is not None and t._ann is None
        assert torch.equal(r1, r2), (step, r1, r2)
        assert torch.equal(s1.view(torch.int32), s2.view(torch.int32)), step
        assert bool((r1 >= 0).all()) and bool((g.sal[r1.flatten()] >= 0.5).all())
    assert steps == ["first", "evicted", "rewritten"]
    assert g.ann_rebuilds == 0 and g.ann_upserts == 40 and g.ann_removed > 0
