"""The IVF-PQ query kernels of csrc/kernels/ivfpq.hip -- ``lzk_ivfpq_scan``,
``lzk_ivfpq_scan_deep``, ``lzk_ivfpq_scan_thresh``, ``lzk_rerank`` -- called
directly on crafted tensors and held against the fp64 references of
tests/kernels/_ivfpq_ref.py.

Exact-grid inputs (small integers: every fp32 partial sum is exact, see
_ivfpq_ref.py) are compared bit for bit, tie order and ``(-inf, -1)`` padding
included; equal scores are planted at row distances 1, 64 and 256 around every
K. Gaussian inputs are held to the order-free bound ``gamma_n sum |terms|``.
The shared lists have 0, 1, 3, 63, 255, 256, 257 and 700 rows (the last one
ends the code array); the probes include a -1, the empty and the 1-row list.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from lazzaro_amd.index.ivfpq import IVFPQIndex  # noqa: E402  (registers the entry points' signatures)
from lazzaro_amd.ops import _lib  # noqa: E402
from lazzaro_amd.utils.faults import KernelError  # noqa: E402
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
    """Sentinel-filled outputs of n entries plus a guard region."""
    return (torch.full((n + GUARD,), SENT_F, dtype=torch.float32, device=DEV),
            torch.full((n + GUARD,), SENT_I, dtype=idt, device=DEV))


def _untouched(os_, oi, start=0):
    return bool((os_[start:] == SENT_F).all()) and bool((oi[start:] == SENT_I).all())


def _same_bits(got32: np.ndarray, want64: np.ndarray) -> bool:
    return np.array_equal(got32.view(np.int32), want64.astype(np.float32).view(np.int32))


@functools.lru_cache(maxsize=None)
def _case(kind: str, M: int, deep: bool = False):
    """Inputs of one (family, M) on the shared lists (+ the 5120-row list)."""
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
    assert c["d"]["off"].dtype == torch.int64 and c["d"]["probes"].dtype == torch.int32
    return c


@functools.lru_cache(maxsize=None)
def _scan16(kind: str, M: int, deep: bool = False):
    c = _case(kind, M, deep)
    return R.scan_ref(c["codes"], c["off"], c["probes"], c["coarse"], c["lut"], 16)


def _scan(c, kslot, M=None):
    d = c["d"]
    n = NQ * NPROBE * kslot
    os_, oi = _outs(n)
    rc = _lib.lib().lzk_ivfpq_scan(d["codes"].data_ptr(), d["off"].data_ptr(), d["probes"].data_ptr(),
                                   d["coarse"].data_ptr(), d["lut"].data_ptr(), NQ, NPROBE, M or c["M"], kslot,
                                   os_.data_ptr(), oi.data_ptr(), _st())
    torch.cuda.synchronize()
    return rc, os_, oi


# ------------------------------------------------------------------ lzk_ivfpq_scan
@pytest.mark.parametrize("kslot", (1, 4, 10, 16))
@pytest.mark.parametrize("M", (8, 16, 32, 48, 64, 96, 128))
def test_scan_exact(M, kslot):
    c = _case("grid", M)
    S, Rw = _scan16("grid", M)
    rc, os_, oi = _scan(c, kslot)
    assert rc == 0 and _untouched(os_, oi, NQ * NPROBE * kslot)
    n = NQ * NPROBE * kslot
    got_s = os_[:n].cpu().numpy().reshape(NQ, NPROBE, kslot)
    got_r = oi[:n].cpu().numpy().reshape(NQ, NPROBE, kslot)
    want_s, want_r = S[..., :kslot], Rw[..., :kslot]
    assert np.array_equal(got_r, want_r), (got_r, want_r)
    assert _same_bits(got_s, want_s)
    if kslot < 16:  # the planted tie straddles K in the 700-row list: the lower row is in, its twin is next
        for q, p in ((0, 0), (1, 2), (2, 2)):
            assert S[q, p, kslot - 1] == S[q, p, kslot] and Rw[q, p, kslot - 1] < Rw[q, p, kslot]


@pytest.mark.parametrize("M", (8, 64, 128))
def test_scan_gaussian_bound(M):
    c = _case("gauss", M)
    K = 16
    rc, os_, oi = _scan(c, K)
    assert rc == 0
    got_s = os_[: NQ * NPROBE * K].cpu().numpy().reshape(NQ, NPROBE, K)
    got_r = oi[: NQ * NPROBE * K].cpu().numpy().reshape(NQ, NPROBE, K)
    worst = 0.0
    for q in range(NQ):
        for p in range(NPROBE):
            l = int(c["probes"][q, p])
            r0, r1 = (int(c["off"][l]), int(c["off"][l + 1])) if l >= 0 else (0, 0)
            nv = min(K, r1 - r0)
            s, r = got_s[q, p], got_r[q, p]
            assert (r[nv:] == -1).all() and np.isneginf(s[nv:]).all()
            if nv == 0:
                continue
            rows = r[:nv]
            assert ((rows >= r0) & (rows < r1)).all() and np.unique(rows).size == nv
            # returned in the kernel's own order: fp32 score desc, row asc
            assert np.array_equal(R.order(s[:nv].astype(np.float64), rows), np.arange(nv))
            s64 = R.pq_scores(c["codes"][r0:r1], c["lut"][q], c["coarse"][q, p])
            bd = R.pq_bound(c["codes"][r0:r1], c["lut"][q], c["coarse"][q, p])
            err = np.abs(s[:nv].astype(np.float64) - s64[rows - r0])
            worst = max(worst, float((err / bd[rows - r0]).max()))
            assert (err <= bd[rows - r0]).all(), (q, p, err, bd[rows - r0])
            out = np.ones(r1 - r0, dtype=bool)
            out[rows - r0] = False
            if out.any():  # fp32(a) >= fp32(b) for a returned, b left out: s64(b) - bd(b) <= s64(a) + bd(a)
                assert (s64[out] - bd[out]).max() <= (s64[rows - r0] + bd[rows - r0]).min()
    print(f"scan M={M}: worst |err| / bound = {worst:.3g}")


# ------------------------------------------------------------------ lzk_ivfpq_scan_deep
def _deep(c, nq=NQ, nprobe=NPROBE, M=None):
    d = c["d"]
    W = _lib.lib().lzk_ivfpq_deep_width()
    n = NQ * NPROBE * W
    os_, oi = _outs(n)
    rc = _lib.lib().lzk_ivfpq_scan_deep(d["codes"].data_ptr(), d["off"].data_ptr(), d["probes"].data_ptr(),
                                        d["coarse"].data_ptr(), d["lut"].data_ptr(), nq, nprobe, M or c["M"],
                                        os_.data_ptr(), oi.data_ptr(), _st())
    torch.cuda.synchronize()
    return rc, os_, oi, W


@pytest.mark.parametrize("M", (8, 32, 128))
def test_scan_deep_exact(M):
    c = _case("grid", M, True)
    rc, os_, oi, W = _deep(c)
    assert rc == 0 and W % 4 == 0 and _untouched(os_, oi, NQ * NPROBE * W)
    SD, RD = R.deep_ref(c["codes"], c["off"], c["probes"], c["coarse"], c["lut"], W)
    got_s = os_[: NQ * NPROBE * W].cpu().numpy().reshape(NQ, NPROBE, 4, W // 4)
    got_r = oi[: NQ * NPROBE * W].cpu().numpy().reshape(NQ, NPROBE, 4, W // 4)
    assert np.array_equal(got_r, RD)
    assert _same_bits(got_s, SD)
    _, R16 = _scan16("grid", M, True)
    for q in range(NQ):
        for p in range(NPROBE):
            for w in range(4):  # every wave segment sorted by (score desc, row asc), padding last
                s, r = got_s[q, p, w], got_r[q, p, w]
                nv = int((r >= 0).sum())
                assert (r[:nv] >= 0).all() and np.isneginf(s[nv:]).all()
                assert np.array_equal(R.order(s[:nv].astype(np.float64), r[:nv]), np.arange(nv))
            want = R16[q, p][R16[q, p] >= 0]
            assert set(want.tolist()) <= set(got_r[q, p].reshape(-1).tolist())
    # the cuts are live: the planted lane of the 5120-row list loses 4 of its 20 rows, the 257-row list pads
    lane = c["off"][8] + R.DEEP_LANE + 256 * np.arange(20)
    assert len(set(lane.tolist()) & set(got_r[0, 0, 0].tolist())) == 16
    assert [int((got_r[1, 0, w] >= 0).sum()) for w in range(4)] == [65, 64, 64, 64]


# ------------------------------------------------------------------ lzk_ivfpq_scan_thresh
def _thresh(c, thr, cap, nq=NQ, nprobe=NPROBE, M=None):
    d = c["d"]
    os_, oi = _outs(NQ * cap)
    cnt = torch.zeros(NQ, dtype=torch.int32, device=DEV)
    t = _dev(np.asarray(thr, dtype=np.float32))
    rc = _lib.lib().lzk_ivfpq_scan_thresh(d["codes"].data_ptr(), d["off"].data_ptr(), d["probes"].data_ptr(),
                                          d["coarse"].data_ptr(), d["lut"].data_ptr(), t.data_ptr(), nq, nprobe,
                                          M or c["M"], cap, cnt.data_ptr(), os_.data_ptr(), oi.data_ptr(), _st())
    torch.cuda.synchronize()
    return rc, cnt.cpu().numpy(), os_, oi


def _tie_thr(c):
    """Per query the score of the 700-row list's four tied rows (tier 12)."""
    thr = np.zeros(NQ)
    for q in range(NQ):
        p = int(np.nonzero(c["probes"][q] == 7)[0][0])
        r = int(c["off"][7]) + 300
        thr[q] = R.pq_scores(c["codes"][r:r + 1], c["lut"][q], c["coarse"][q, p])[0]
    return thr


@pytest.mark.parametrize("thr_kind", ("ninf", "pinf", "tie"))
@pytest.mark.parametrize("M", (8, 48, 128))
def test_scan_thresh_exact(M, thr_kind):
    """Appends are atomic: compared as sets. -inf takes every probed row, +inf
    none (the sentinel-filled outputs stay untouched), and a threshold equal
    to the score of four planted ties takes them (``>=``)."""
    c = _case("grid", M)
    cap = 1600  # the fullest query probes 257 + 256 + 700 + 3 rows
    thr = {"ninf": np.full(NQ, -np.inf), "pinf": np.full(NQ, np.inf)}.get(thr_kind)
    if thr is None:
        thr = _tie_thr(c)
    want = R.thresh_ref(c["codes"], c["off"], c["probes"], c["coarse"], c["lut"], thr)
    rc, cnt, os_, oi = _thresh(c, thr, cap)
    assert rc == 0 and _untouched(os_, oi, NQ * cap)
    s_all, r_all = os_[: NQ * cap].cpu().numpy().reshape(NQ, cap), oi[: NQ * cap].cpu().numpy().reshape(NQ, cap)
    for q in range(NQ):
        wr, ws = want[q]
        if thr_kind == "tie":  # several rows sit exactly on the threshold: '>' for '>=' would lose them
            assert int((ws == thr[q]).sum()) >= 4 and wr.size < cap
        assert cnt[q] == wr.size
        o = np.argsort(r_all[q, : cnt[q]], kind="stable")
        assert np.array_equal(r_all[q, : cnt[q]][o], wr)
        assert _same_bits(s_all[q, : cnt[q]][o], ws)
        assert (s_all[q, cnt[q]:] == SENT_F).all() and (r_all[q, cnt[q]:] == SENT_I).all()
    if thr_kind == "ninf":
        assert list(cnt) == [701, 1216, 1275]
    if thr_kind == "pinf":
        assert (cnt == 0).all() and _untouched(os_, oi)


@pytest.mark.parametrize("M", (8, 48, 128))
def test_scan_thresh_overflow(M):
    """cap below the qualifying count: the count runs on, the cap slots hold
    distinct qualifying rows with their scores, nothing lands past them."""
    c = _case("grid", M)
    cap = 100
    args = (c["codes"], c["off"], c["probes"], c["coarse"], c["lut"])
    # each query's 300th best score: at least 300 of its 701 or more rows qualify, not all
    thr = np.array([np.sort(s)[-300] for _, s in R.thresh_ref(*args, np.full(NQ, -np.inf))])
    want = R.thresh_ref(*args, thr)
    rc, cnt, os_, oi = _thresh(c, thr, cap)
    assert rc == 0 and _untouched(os_, oi, NQ * cap)
    s_all, r_all = os_[: NQ * cap].cpu().numpy().reshape(NQ, cap), oi[: NQ * cap].cpu().numpy().reshape(NQ, cap)
    for q in range(NQ):
        wr, ws = want[q]
        assert cap < wr.size < 701 and cnt[q] == wr.size
        rows = r_all[q]
        assert np.unique(rows).size == cap and np.isin(rows, wr).all()
        assert _same_bits(s_all[q], ws[np.searchsorted(wr, rows)])


# ------------------------------------------------------------------ lzk_rerank
NV = 5000
KK = ((1, 1), (4, 3), (10, 10), (16, 16))
RS = (1, 15, 16, 17, 200, 513)
RR_CASES = [(fmt, D, pad) for fmt, Ds in ((0, (128, 384)), (1, (256, 768)), (2, (256, 768))) for D in Ds
            for pad in (0, 16, 48)]


@functools.lru_cache(maxsize=2)
def _vectors(kind: str, fmt: int, D: int):
    rng = np.random.default_rng(fmt * 10000 + D + (0 if kind == "grid" else 5))
    if kind == "grid":
        vals, scale = R.grid_vectors(rng, NV, D)
        Q = R.grid_queries(rng, NQ, D)
    else:
        vals = (rng.integers(-127, 128, size=(NV, D)) if fmt == 2 else rng.standard_normal((NV, D))).astype(np.float32)
        scale = rng.uniform(0.005, 0.02, NV).astype(np.float32)
        Q = rng.standard_normal((NQ, D)).astype(np.float32)
    raw = R.encode_rows(vals, fmt, R.row_bytes(fmt, D))
    V64 = R.decode_rows(raw, fmt, D, scale)
    return raw, scale, Q, V64, V64 @ Q[0].astype(np.float64)


def _padded(raw: np.ndarray, pad: int) -> np.ndarray:
    out = np.full((raw.shape[0], raw.shape[1] + pad), 0x7F, dtype=np.uint8)
    out[:, : raw.shape[1]] = raw
    return out


def _row_lists(rng, s0: np.ndarray, Rn: int, kout: int):
    """[NQ, Rn] candidate rows, no row twice in a list. Query 0: -1
    interspersed, and -- where the list is long enough -- a pair of duplicate
    vector rows (a, a + NV / 2) ranked kout-th and (kout+1)-th, plus another
    pair inside the top. Query 1: all -1. Query 2: kout - 1 valid rows."""
    rows = np.full((NQ, Rn), -1, dtype=np.int64)
    slots = np.array([c for c in range(Rn) if c % 5 != 2])
    nv = slots.size
    pair = None
    if nv >= kout + 1:
        med = np.median(s0)
        a = int(np.argmin(np.abs(s0[:500] - med)))
        above = np.nonzero(s0 > s0[a])[0]
        below = np.nonzero(s0 < s0[a])[0]
        top = []
        if kout - 1 >= 2:  # the best of the duplicated rows and its twin lead the list
            b = int(np.argmax(s0[:500]))
            top = [b, b + NV // 2]
            above = above[s0[above] < s0[b]]
        top = top + rng.choice(above, kout - 1 - len(top), replace=False).tolist()
        rest = rng.choice(below, nv - kout - 1, replace=False).tolist()
        valid = np.array(top + [a, a + NV // 2] + rest, dtype=np.int64)
        pair = (a, a + NV // 2)
    else:
        valid = rng.choice(NV, nv, replace=False).astype(np.int64)
    rows[0, slots] = rng.permutation(valid)
    few = min(Rn, kout - 1)
    if few:
        rows[2, Rn - few:] = rng.choice(NV, few, replace=False)
    return rows, pair


def _rerank(raw_d, ldv, fmt, scale_d, rows, Q, D, kslot, kout):
    nq, Rn = rows.shape
    os_, oi = _outs(nq * kout, torch.int64)
    rows_d, Q_d = _dev(rows), _dev(Q)
    rc = _lib.lib().lzk_rerank(raw_d.data_ptr(), ldv, fmt, _lib.ptr(scale_d), rows_d.data_ptr(), nq, Rn,
                               Q_d.data_ptr(), D, kslot, kout, os_.data_ptr(), oi.data_ptr(), _st())
    torch.cuda.synchronize()
    return rc, os_, oi


@pytest.mark.parametrize("kslot,kout", KK)
@pytest.mark.parametrize("fmt,D,pad", RR_CASES)
def test_rerank_exact(fmt, D, pad, kslot, kout):
    raw, scale, Q, V64, s0 = _vectors("grid", fmt, D)
    ldv = raw.shape[1] + pad
    raw_d = _dev(_padded(raw, pad))
    scale_d = _dev(scale) if fmt else None
    rng = np.random.default_rng(D + pad + kout)
    for Rn in RS:
        rows, pair = _row_lists(rng, s0, Rn, kout)
        want_s, want_r = R.rerank_ref(V64, rows, Q, kout)
        if pair is not None:  # the duplicates straddle kout: the lower row is the last one in
            assert want_r[0, kout - 1] == pair[0] and pair[1] in rows[0] and pair[1] not in want_r[0]
            if kout >= 3:
                assert want_r[0, 1] == want_r[0, 0] + NV // 2 and want_s[0, 0] == want_s[0, 1]
        rc, os_, oi = _rerank(raw_d, ldv, fmt, scale_d, rows, Q, D, kslot, kout)
        assert rc == 0 and _untouched(os_, oi, NQ * kout), Rn
        got_s = os_[: NQ * kout].cpu().numpy().reshape(NQ, kout)
        got_r = oi[: NQ * kout].cpu().numpy().reshape(NQ, kout)
        assert np.array_equal(got_r, want_r), (Rn, got_r, want_r)
        assert _same_bits(got_s, want_s), (Rn, got_s, want_s)
        assert (got_r[1] == -1).all() and int((got_r[2] >= 0).sum()) == min(Rn, kout - 1)


@pytest.mark.parametrize("fmt,D", ((0, 384), (1, 768), (2, 768)))
def test_rerank_gaussian_bound(fmt, D):
    raw, scale, Q, V64, _ = _vectors("gauss", fmt, D)
    Rn, K, pad = 200, 16, 16
    rng = np.random.default_rng(fmt)
    rows = np.stack([rng.choice(NV, Rn, replace=False) for _ in range(NQ)]).astype(np.int64)
    rows[0, ::7] = -1
    rc, os_, oi = _rerank(_dev(_padded(raw, pad)), raw.shape[1] + pad, fmt, _dev(scale) if fmt else None, rows, Q, D,
                          K, K)
    assert rc == 0
    got_s = os_[: NQ * K].cpu().numpy().reshape(NQ, K)
    got_r = oi[: NQ * K].cpu().numpy().reshape(NQ, K)
    s64, _ = R.rerank_scores(V64, rows, Q)
    bd = R.rerank_bound(V64, rows, Q)
    worst = 0.0
    for q in range(NQ):
        assert (got_r[q] >= 0).all() and np.unique(got_r[q]).size == K
        assert np.array_equal(R.order(got_s[q].astype(np.float64), got_r[q]), np.arange(K))
        pos = np.array([int(np.nonzero(rows[q] == r)[0][0]) for r in got_r[q]])  # each returned row is a candidate
        err = np.abs(got_s[q].astype(np.float64) - s64[q, pos])
        worst = max(worst, float((err / bd[q, pos]).max()))
        assert (err <= bd[q, pos]).all(), (q, err, bd[q, pos])
        out = rows[q] >= 0
        out[pos] = False
        assert (s64[q, out] - bd[q, out]).max() <= (s64[q, pos] + bd[q, pos]).min()
    print(f"rerank fmt={fmt} D={D}: worst |err| / bound = {worst:.3g}")


# ------------------------------------------------------------------ launcher rejections
def test_rerank_rejections():
    """Refused before any launch: nonzero status, outputs untouched."""
    D, Rn, n = 256, 8, 32
    raw = torch.zeros((n, 2 * D + 16), dtype=torch.uint8, device=DEV)
    scale = torch.ones(n, dtype=torch.float32, device=DEV)
    rows = torch.zeros((2, 40705), dtype=torch.int64, device=DEV)
    rows[:] = torch.arange(40705, device=DEV) % n
    Q = torch.zeros((2, 2 * D), dtype=torch.float32, device=DEV)
    os_, oi = _outs(2 * 16, torch.int64)
    L = _lib.lib()

    def call(ldv=D, fmt=2, vs=scale, R_=Rn, D_=D, kslot=10, kout=10):
        rc = L.lzk_rerank(raw.data_ptr(), ldv, fmt, _lib.ptr(vs), rows.data_ptr(), 2, R_, Q.data_ptr(), D_, kslot,
                          kout, os_.data_ptr(), oi.data_ptr(), _st())
        torch.cuda.synchronize()
        return rc
    bad = {
        "row bytes not a multiple of 256 (int8)": dict(D_=192, ldv=192),
        "row bytes not a multiple of 256 (bf16)": dict(D_=64, fmt=0, ldv=128, vs=None),
        "ldv not a multiple of 16": dict(ldv=D + 8),
        "kout > kslot": dict(kslot=4, kout=5),
        "fmt 3": dict(fmt=3),
        "fmt -1": dict(fmt=-1),
        "fp8 without scales": dict(fmt=1, vs=None),
        "int8 without scales": dict(fmt=2, vs=None),
        "kslot 5": dict(kslot=5, kout=3),
        "R = 0": dict(R_=0),
        "query + scores past 160 KiB of LDS": dict(R_=40705),
    }
    for what, kw in bad.items():
        assert call(**kw) == INVALID, what
        assert _untouched(os_, oi), what
    assert (D + 40704) * 4 == 160 * 1024  # the largest R the launcher takes at D = 256 is one below the refused one


def test_scan_rejections():
    c = _case("grid", 16)
    for what, (M, kslot) in {"M 24": (24, 10), "M 0": (0, 10), "kslot 5": (16, 5), "kslot 0": (16, 0)}.items():
        d = c["d"]
        os_, oi = _outs(NQ * NPROBE * 16)
        rc = _lib.lib().lzk_ivfpq_scan(d["codes"].data_ptr(), d["off"].data_ptr(), d["probes"].data_ptr(),
                                       d["coarse"].data_ptr(), d["lut"].data_ptr(), NQ, NPROBE, M, kslot,
                                       os_.data_ptr(), oi.data_ptr(), _st())
        torch.cuda.synchronize()
        assert rc == INVALID and _untouched(os_, oi), what
    for what, kw in {"nq 0": dict(nq=0), "nprobe 0": dict(nprobe=0), "M 24": dict(M=24)}.items():
        rc, os_, oi, _ = _deep(c, **kw)
        assert rc == INVALID and _untouched(os_, oi), "deep " + what
        rc, cnt, os_, oi = _thresh(c, np.full(NQ, -np.inf), 64, **kw)
        assert rc == INVALID and (cnt == 0).all() and _untouched(os_, oi), "thresh " + what
    # cap = 0 (the buffers still hold room: nothing may be written)
    d = c["d"]
    os_, oi = _outs(64)
    cnt = torch.zeros(NQ, dtype=torch.int32, device=DEV)
    thr = torch.full((NQ,), float("-inf"), device=DEV)
    rc = _lib.lib().lzk_ivfpq_scan_thresh(d["codes"].data_ptr(), d["off"].data_ptr(), d["probes"].data_ptr(),
                                          d["coarse"].data_ptr(), d["lut"].data_ptr(), thr.data_ptr(), NQ, NPROBE, 16,
                                          0, cnt.data_ptr(), os_.data_ptr(), oi.data_ptr(), _st())
    torch.cuda.synchronize()
    assert rc == INVALID and int(cnt.abs().sum()) == 0 and _untouched(os_, oi)


# ------------------------------------------------------------------ the Python composition
def _crowded(n, d, seed):
    """Unit rows, five in six of them within a small cap around one direction."""
    g = torch.Generator().manual_seed(seed)
    u = torch.nn.functional.normalize(torch.randn(1, d, generator=g), dim=1)
    x = torch.randn(n, d, generator=g)
    x[: n * 5 // 6] = u + 0.1 * x[: n * 5 // 6] / d ** 0.5
    return torch.nn.functional.normalize(x[torch.randperm(n, generator=g)], dim=1)


@pytest.fixture(scope="module")
def crowded_index():
    n, d = 6000, 64
    idx = IVFPQIndex(d, nlist=8, m=8, device=DEV, keep_vectors="int8")
    x = _crowded(n, d, 11).to(DEV)
    idx.train(x, iters=2)
    idx.add(x)
    idx._finalize()
    sizes = (idx.list_off[1:] - idx.list_off[:-1]).cpu().numpy()
    assert sizes.sum() == n and sizes.max() >= n // 2, sizes  # one list holds most rows
    big = int(sizes.argmax())
    others = [l for l in range(8) if l != big]
    probes = np.array([[big, others[0], -1, others[1]], [others[2], big, others[3], others[4]],
                       [others[5], others[6], others[0], big]], dtype=np.int32)
    rng = np.random.default_rng(3)
    # exact-grid tables; real codes use every byte value, so no planted tiers: integer sums tie often enough
    lut = rng.integers(-1024, 1025, size=(NQ, 8, 256)).astype(np.float32)
    coarse = rng.integers(-1024, 1025, size=(NQ, NPROBE)).astype(np.float32)
    return dict(idx=idx, codes=idx.codes.cpu().numpy(), off=idx.list_off.cpu().numpy(), probes=probes, lut=lut,
                coarse=coarse)


@pytest.mark.parametrize("k", (1, 7, 10, 16))
def test_scan_gpu_is_the_exact_topk(crowded_index, k):
    """``_scan_gpu`` (scan + ``lzk_topk_merge``) == the exact top-k over the
    probed lists, ties in (score desc, row asc) order."""
    ci = crowded_index
    S, Rw = R.scan_ref(ci["codes"], ci["off"], ci["probes"], ci["coarse"], ci["lut"], k)
    want_s, want_r = R.merge_topk(S, Rw, k)
    s, r = ci["idx"]._scan_gpu(_dev(ci["probes"]), _dev(ci["coarse"]), _dev(ci["lut"]), k)
    torch.cuda.synchronize()
    assert np.array_equal(r.cpu().numpy(), want_r)
    assert _same_bits(s.cpu().numpy(), want_s)


def test_scan_deep_pools_match_reference(crowded_index):
    ci = crowded_index
    k = 600
    W = _lib.lib().lzk_ivfpq_deep_width()
    SD, RD = R.deep_ref(ci["codes"], ci["off"], ci["probes"], ci["coarse"], ci["lut"], W)
    want_s, want_r = R.merge_topk(SD, RD, k)
    s, r = ci["idx"]._scan_deep(_dev(ci["probes"]), _dev(ci["coarse"]), _dev(ci["lut"]), k)
    torch.cuda.synchronize()
    s, r = s.cpu().numpy(), r.cpu().numpy()
    assert _same_bits(s, want_s)  # torch.topk leaves the order among equal scores open: rows per score level
    for q in range(NQ):
        assert np.unique(r[q]).size == k
        last = want_s[q, -1]
        assert set(r[q][s[q] > last].tolist()) == set(want_r[q][want_s[q] > last].tolist())
        pool = dict(zip(RD[q].reshape(-1).tolist(), SD[q].reshape(-1).tolist()))
        assert all(pool.get(int(a)) == float(b) for a, b in zip(r[q], s[q]))
    # the crowded list holds more good rows than its pool: the pooled k-th score is below the true one
    S, Rw = R.scan_ref(ci["codes"], ci["off"], ci["probes"], ci["coarse"], ci["lut"], k)
    true_s, _ = R.merge_topk(S, Rw, k)
    assert (want_s[:, -1] <= true_s[:, -1]).all() and (want_s[:, -1] < true_s[:, -1]).any()


def test_scan_candidates_hold_the_exact_top_r(crowded_index):
    """The two-pass design's claim: the appended set holds the exact PQ top-R
    however the neighbours concentrate."""
    ci = crowded_index
    Rn = 600
    W = _lib.lib().lzk_ivfpq_deep_width()
    args = (ci["codes"], ci["off"], ci["probes"], ci["coarse"], ci["lut"])
    S, Rw = R.scan_ref(*args, Rn)
    want_s, want_r = R.merge_topk(S, Rw, Rn)
    thr, _ = R.merge_topk(*R.deep_ref(*args, W), Rn)
    counts = [r.size for r, _ in R.thresh_ref(*args, thr[:, Rn - 1])]
    s, r = ci["idx"]._scan_candidates(_dev(ci["probes"]), _dev(ci["coarse"]), _dev(ci["lut"]), Rn)
    torch.cuda.synchronize()
    assert ci["idx"].last_candidates.cpu().tolist() == counts and min(counts) >= Rn
    s, r = s.cpu().numpy(), r.cpu().numpy()
    assert _same_bits(s, want_s)
    for q in range(NQ):
        assert np.unique(r[q]).size == Rn and (r[q] >= 0).all()
        last = want_s[q, -1]
        assert set(r[q][s[q] > last].tolist()) == set(want_r[q][want_s[q] > last].tolist())
        l = np.searchsorted(ci["off"], r[q], side="right") - 1  # each row carries the score of its own list's probe
        for a, b, li in zip(r[q], s[q], l):
            p = int(np.nonzero(ci["probes"][q] == li)[0][0])
            assert float(b) == R.pq_scores(ci["codes"][a:a + 1], ci["lut"][q], ci["coarse"][q, p])[0]


def test_search_with_a_rerank_depth_past_the_lds_limit(monkeypatch):
    """``lzk_rerank`` keeps the query and one score per candidate in LDS and
    refuses (D + R) * 4 > 160 KiB. ``search`` must then take the library
    path, not raise; one candidate fewer still runs the fused kernel. (An
    index whose kept rows are a multiple of 256 bytes: at d = 64 the fused
    re-rank is never chosen.)"""
    n, d = 3000, 256
    idx = IVFPQIndex(d, nlist=8, m=8, device=DEV, keep_vectors="int8")
    x = _crowded(n, d, 12).to(DEV)
    idx.train(x, iters=2)
    idx.add(x)
    q = x[:2] + 0.05 * torch.randn(2, d, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1)) / d ** 0.5
    fits = 160 * 1024 // 4 - d
    assert idx._rerank_gpu_ok(10)
    fused = []
    real = IVFPQIndex._rerank_gpu
    monkeypatch.setattr(IVFPQIndex, "_rerank_gpu", lambda self, *a: (fused.append(a[1].shape[1]), real(self, *a))[1])
    s_fit, i_fit = idx.search(q, 10, nprobe=4, rerank=fits)
    s1, i1 = idx.search(q, 10, nprobe=4, rerank=fits + 1)
    assert fused == [fits]
    monkeypatch.setattr(IVFPQIndex, "_rerank_gpu_ok", lambda self, k: False)
    s2, i2 = idx.search(q, 10, nprobe=4, rerank=fits + 1)
    torch.cuda.synchronize()
    assert fused == [fits]
    assert torch.equal(s1, s2) and torch.equal(i1, i2)
    assert bool((i1 >= 0).all()) and bool((i1[:, 0] == torch.arange(2, device=DEV)).all())
    # both depths cover every probed row, so the fused kernel and the library path rank the same candidates;
    # each is within gamma_{d+2} sum |v q| <= gamma_{d+2} |v| |q| of the exact product, |q| = 1, |v| <= 1.02
    torch.testing.assert_close(s_fit, s2, atol=2 * R.gamma(d + 2) * 1.02, rtol=0)
    with pytest.raises(KernelError):  # the launcher's own refusal is what search now avoids
        idx._rerank_gpu(torch.nn.functional.normalize(q, dim=1),
                        torch.zeros((2, fits + 1), dtype=torch.int64, device=DEV), 10)
