"""The kernels the search routes start and finish with, held against the fp64
reference tests/kernels/_rerank_ref.py (its docstring counts the roundings
behind every bound used here): ``store_rerank_kernel`` /
``store_rerank_block_kernel``, ``cos_rerank64_kernel``, ``tg_write_emb_kernel``
and ``row_cent_cos_kernel`` (tenant.hip), ``seg_sum_sorted_kernel`` /
``seg_sum_kernel`` / ``centroid_kernel`` and ``pairs_kernel`` (graph.hip),
through the exported functions and the op wrappers that call them.

store_rerank. M in {1, 3, 63} runs the block kernel, {64, 65, 130} the wave
kernel; ``RERANK_COMBOS`` pairs every C in {1, 15, 16, 17, 33, 63, 64} with two
D of {4, 20, 48, 64, 100, 384, 1024} (the float4 route, the scalar route of
each kernel, and D = 48: float4 in the wave kernel, scalar in the block
kernel), every k in {1, 10, C, C + 3} and three layouts of X (contiguous, a row
stride padded by 4 and one padded by 3, which forces the scalar route; the
padding holds 1e30). Outputs are prefilled with a sentinel that no case can
produce, so an unwritten slot fails. Exact grid: ``l2`` / ``ip`` scores and rows
are compared bit for bit, ties included; ``cosine`` (not exact) and the Gaussian
cases go through ``check_ranked``: every score within its bound, the output
sorted by its own (score, row), the rows between two decided cuts equal to the
reference's. Duplicates: a row listed twice or three times comes back as often
(both kernels ranked (score, row) only, gave the copies one slot and left the
last live slot unwritten: fixed with this test, the slot-order rule of
``cos_rerank64_kernel``).

write_emb. Bit-exact against the definition (``write_emb_ref``): emb32 (signs
of zero included), the bf16 bits, emb8, rs8, has_emb and the running maximum of
the row scales; ``sqn`` within half an fp32 ulp (1 + 2^-20) of the exact sum,
``sumsq`` within 1e-15 relative per added row, ``dv_max`` within one fp32 ulp. A
zero row leaves the scale maximum unchanged (its ``| |x| - 1 |`` is 1 by
definition and does enter ``dv_max`` when ``has`` is set); a ``has`` = 0 row
leaves both maxima unchanged. The error-model cap ``|vb - emb8 rs8| <= rs8 / 2
(1 + 2^-22)`` is asserted for every element of the planted rows and of Gaussian
rows scaled to a maximum of 1 -- NOT of arbitrary rows: the definition itself
exceeds it (tests/unit/test_rerank_ref_cpu.py
``test_quantiser_error_cap_exhaustive``: ``vb = amax / 2`` quantises to 64 with
an error of ``rs8 / 2 (1 + 2^-18.1)`` for 45 of the 128 bf16 significands of
amax, e.g. 150, because ``fl32(amax * fl32(1 / 127))`` lies above ``amax / 127``
there and the tie 63.5 rounds to the even 64). For arbitrary rows the derived
cap ``1 + 2^-17`` is asserted, and the kernel equals the definition bit for bit.

centroids, pairs, row_cent_cos, cos_rerank64: see the tests' docstrings.
``pairs_above`` with a buffer smaller than the result used to return a
timing-dependent subset; it now runs once more with room for the count (fixed
with ``test_pairs_overflow_gpu``).

Observed on one MI355X: the 129 cases take 7.1 s together; the slowest,
test_cos_rerank64_gpu[64-384-2] (its exact-dot reference), 0.64 s. Largest
|value - fp64| / bound: store_rerank wave kernel l2 0.27, ip 0.42, cosine 0.46;
block kernel l2 0.19, ip 0.28, cosine 0.21; cos_rerank64 0.55; centroids 0.10
(normalised 0.07); row_cent_cos 0.08. On the kernels as they were before the
two fixes, the 30 duplicate cases fail on the sentinel ("an output slot was
left unwritten") and the overflow case returns 8 of its pairs.
"""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from lazzaro_amd.ops import _lib  # noqa: E402
from lazzaro_amd.ops import graph_ops as G  # noqa: E402
from lazzaro_amd.ops import search as S  # noqa: E402,F401  (registers lzk_cos_rerank64)
from lazzaro_amd.ops import tenant_ops as T  # noqa: E402
from tests.kernels import _rerank_ref as R  # noqa: E402

DEV = "cuda"
NEG_INF = float("-inf")
SENT_F, SENT_I = -7.25e6, -77  # what an output holds before a launch
F32 = np.float32
METRICS = ("l2", "ip", "cosine")

WORST = {}  # kernel -> largest |value - fp64| / bound seen


def _st():
    return _lib.stream_ptr(torch.device(DEV))


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(dtype) if dtype is not None else t).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _note(name, v):
    WORST[name] = max(WORST.get(name, 0.0), float(v))
    print(f"worst |err| / bound [{name}]: {WORST[name]:.4f}")


def _poison(nbytes: int) -> None:
    """Leave 0x5A bytes in the block the caching allocator hands out next for
    a request of this size: a ``torch.empty`` output cannot hold zeros or a
    stale right answer by luck."""
    t = torch.full((max(1, nbytes),), 0x5A, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    del t


# ---------------------------------------------------------------- store_rerank
def _rerank_launch(case, k: int, metric: str, kind=None):
    """lzk_store_rerank on sentinel-filled outputs, X as the [N, D] view of the
    wider buffer. Returns numpy (scores fp32, rows, node rows or None)."""
    D = case["D"]
    Q, Xw = _dev(case["Q"]), _dev(case["X"])
    X = Xw[:, :D]
    sqn, bias, cand = _dev(case["sqn"]), _dev(case["bias"]), _dev(case["cand"])
    M, C = cand.shape
    os_ = torch.full((M, k), SENT_F, dtype=torch.float32, device=DEV)
    oi = torch.full((M, k), SENT_I, dtype=torch.long, device=DEV)
    kd = _dev(kind, torch.uint8) if kind is not None else None
    oin = torch.full((M, k), SENT_I, dtype=torch.long, device=DEV) if kind is not None else None
    rc = _lib.lib().lzk_store_rerank(Q.data_ptr(), Q.stride(0), X.data_ptr(), X.stride(0), D, sqn.data_ptr(),
                                     bias.data_ptr(), cand.data_ptr(), C, M, k, T._METRIC_CODE[metric],
                                     os_.data_ptr(), oi.data_ptr(), _lib.ptr(kd), _lib.ptr(oin), _st())
    assert rc == 0, rc
    torch.cuda.synchronize()
    s, r = _np(os_), _np(oi)
    assert not (s == F32(SENT_F)).any() and not (r == SENT_I).any(), "an output slot was left unwritten"
    if oin is not None:
        assert not (_np(oin) == SENT_I).any(), "a node-row slot was left unwritten"
    return s, r, (_np(oin) if oin is not None else None)


def _assert_bits(case, k, metric, s, r):
    es, er, _ = R.rerank_ref(case["Q"], case["X"], case["sqn"], case["bias"], case["cand"], k, metric)
    assert np.array_equal(r, er), (np.argwhere(r != er)[:5], r[r != er][:5], er[r != er][:5])
    assert np.array_equal(s, es.astype(F32)), np.argwhere(s != es.astype(F32))[:5]


def _assert_ranked(case, k, metric, s, r, name):
    Sx, Bx = R.rerank_scores(case["Q"], case["X"], case["sqn"], case["bias"], case["cand"], metric)
    und = tot = 0
    worst = 0.0
    for q in range(len(Sx)):
        u, t, w = R.check_ranked(s[q], r[q], Sx[q], Bx[q], case["cand"][q], k)
        und, tot, worst = und + u, tot + t, max(worst, w)
    _note(name, worst)
    return und, tot


@pytest.mark.parametrize("M", R.RERANK_MS)
@pytest.mark.parametrize("metric", METRICS)
def test_store_rerank_grid_gpu(metric, M):
    """Exact grid, every combo: l2 / ip bit for bit (scores, rows, padding,
    ties by row); cosine within its bound, ordered, exact where decided."""
    for i, (C, D, kc, pad) in enumerate(R.RERANK_COMBOS):
        case = R.rerank_inputs("grid", metric, M, C, D, pad, seed=100 * M + i)
        k = R.k_of(kc, C)
        s, r, _ = _rerank_launch(case, k, metric)
        if metric == "cosine":
            _assert_ranked(case, k, metric, s, r, "store_rerank grid cosine")
        else:
            _assert_bits(case, k, metric, s, r)


@pytest.mark.parametrize("M", R.RERANK_MS)
@pytest.mark.parametrize("metric", METRICS)
def test_store_rerank_gauss_gpu(metric, M):
    """Gaussian rows (l2: a third of the queries next to a stored row): every
    score within its bound, rows equal to the reference's wherever the
    reference decides; the undecided share is the reference's own figure
    (test_rerank_ref_cpu.py proves it at most 1 % per case)."""
    for i, (C, D, kc, pad) in enumerate(R.GAUSS_COMBOS):
        case = R.rerank_inputs("gauss", metric, M, C, D, pad, seed=1000 * M + D)
        k = R.k_of(kc, C)
        s, r, _ = _rerank_launch(case, k, metric)
        _assert_ranked(case, k, metric, s, r, f"store_rerank {'wave' if M >= 64 else 'block'} {metric}")
        und, tot = R.rerank_undecided(case, metric)
        assert und <= R.UNDECIDED_CAP * max(tot, 1), (C, D, und, tot)


@pytest.mark.parametrize("M", (3, 64))
@pytest.mark.parametrize("metric", METRICS)
def test_store_rerank_edges_gpu(metric, M):
    """A query whose candidates are all -1, one whose candidates are all
    tombstoned, a zero row under cosine (sqn 0: the score is its bias), l2 with
    q equal to a stored row (score exactly 0 on the grid), the node-row output,
    and the op wrapper on a poisoned allocation."""
    C, D, k = 17, 64, 20
    case = R.rerank_inputs("grid", metric, M, C, D, 0, seed=7 + M)
    X, Q, cand, bias, sqn = case["X"], case["Q"], case["cand"], case["bias"], case["sqn"]
    X[20] = 0.0
    sqn[20] = 0.0
    bias[20] = -float(sqn[20]) if metric == "l2" else 2.0
    bias[30:30 + C] = NEG_INF
    cand[0] = -1
    cand[1] = np.arange(30, 30 + C)
    cand[2, :4] = (20, 5, 40, 20 + 1)
    Q[2] = X[5]
    kind = (np.arange(R.RERANK_N) % 3 != 0).astype(np.uint8)  # 1 = a graph node
    s, r, rn = _rerank_launch(case, k, metric, kind=kind)
    es, er, _, en = R.rerank_ref(Q, X, sqn, bias, cand, k, metric, kind=kind)
    assert np.all(r[0] == -1) and np.all(s[0] == NEG_INF) and np.all(r[1] == -1) and np.all(s[1] == NEG_INF)
    assert np.all(rn[:2] == -1)
    if metric == "cosine":
        _assert_ranked(case, k, metric, s, r, "store_rerank grid cosine")
        assert 20 in r[2] and s[2][list(r[2]).index(20)] == F32(2.0)
        assert np.array_equal(rn, np.where((r >= 0) & (kind[np.clip(r, 0, None)] == 1), r, -1))
    else:
        assert np.array_equal(r, er) and np.array_equal(s, es.astype(F32)) and np.array_equal(rn, en)
    if metric == "l2" and bias[5] != NEG_INF:
        assert s[2][list(r[2]).index(5)] == 0.0
    # the wrapper allocates its outputs itself
    _poison(M * k * 8)
    _poison(M * k * 4)
    ws, wr = T.store_rerank(_dev(Q), _dev(X)[:, :D], _dev(sqn), _dev(bias), _dev(cand), k, metric)
    assert np.array_equal(_np(ws), s) and np.array_equal(_np(wr), r)
    ws, wn = T.store_rerank(_dev(Q), _dev(X)[:, :D], _dev(sqn), _dev(bias), _dev(cand), k, metric,
                            kind=_dev(kind, torch.uint8))
    assert np.array_equal(_np(ws), s) and np.array_equal(_np(wn), rn)


@pytest.mark.parametrize("C,kc", [(16, 2), (16, 3), (64, 2), (33, 1), (3, 3)])
@pytest.mark.parametrize("M", (3, 64))
@pytest.mark.parametrize("metric", METRICS)
def test_store_rerank_duplicates_gpu(metric, M, C, kc):
    """A row listed twice (and one listed three times) behaves as in the torch
    tier: every copy is kept, next to its twins, and every slot up to the live
    count is written -- the sentinel prefill makes an unwritten slot fail."""
    D = 48
    case = R.rerank_inputs("grid", metric, M, C, D, 0, seed=31 * M + C)
    cand = case["cand"]
    for q in range(M):
        a = cand[q, 0] if cand[q, 0] >= 0 else 7
        cand[q, 0] = cand[q, C - 1] = a  # first and last slot: the copies are far apart in the wave
        if C >= 16:
            b = cand[q, 5] if cand[q, 5] >= 0 else 9
            cand[q, 5] = cand[q, 6] = cand[q, 11] = b
    k = R.k_of(kc, C)
    s, r, _ = _rerank_launch(case, k, metric)
    es, er, _ = R.rerank_ref(case["Q"], case["X"], case["sqn"], case["bias"], cand, k, metric)
    if metric == "cosine":
        _assert_ranked(case, k, metric, s, r, "store_rerank grid cosine")
    else:
        assert np.array_equal(r, er) and np.array_equal(s, es.astype(F32))
    if kc >= 2:  # k >= C: every live copy is in the output
        for q in range(M):
            live = cand[q][(cand[q] >= 0) & (case["bias"][np.clip(cand[q], 0, None)] != NEG_INF)]
            assert sorted(r[q][r[q] >= 0].tolist()) == sorted(live.tolist())
    # the wrapper on a poisoned allocation: what a caller of store_search sees
    _poison(M * k * 8)
    _poison(M * k * 4)
    ws, wr = T.store_rerank(_dev(case["Q"]), _dev(case["X"])[:, :D], _dev(case["sqn"]), _dev(case["bias"]),
                            _dev(cand), k, metric)
    assert np.array_equal(_np(ws), s) and np.array_equal(_np(wr), r)


# ---------------------------------------------------------------- cos_rerank64
COS64_CASES = ((1, 3, 1), (15, 4, 5), (16, 100, 6), (17, 384, 3), (33, 3, 9), (63, 100, 2), (64, 384, 2), (64, 4, 9))


def _cos64_launch(Qn, Xw, D, sqn, cand, k):
    M, C = cand.shape
    Qd, Xd = _dev(Qn), _dev(Xw)
    X = Xd[:, :D]
    os_ = torch.full((M, k), SENT_F, dtype=torch.float64, device=DEV)
    oi = torch.full((M, k), SENT_I, dtype=torch.long, device=DEV)
    cd, sd = _dev(cand), _dev(sqn)
    rc = _lib.lib().lzk_cos_rerank64(Qd.data_ptr(), Qd.stride(0), X.data_ptr(), X.stride(0), D, sd.data_ptr(),
                                     cd.data_ptr(), C, M, k, os_.data_ptr(), oi.data_ptr(), _st())
    torch.cuda.synchronize()
    return rc, _np(os_), _np(oi)


@pytest.mark.parametrize("C,D,M", COS64_CASES)
def test_cos_rerank64_gpu(C, D, M):
    """Exact-dot reference (``Fraction``): rows equal, scores within
    (ceil(D / 4) + 5) 2^-53 sum|q x| / |x|, for k in {1, 10, C}; k = C + 3 is
    refused by the launcher (``_rerank_cos`` then takes the torch tier) and
    leaves the outputs untouched. Candidate lists hold -1 slots, a query of
    only -1, identical vectors at two rows (ties by row), a row listed twice
    (both kept) and a zero row with sqn 0 (score 0)."""
    rng = np.random.default_rng(5 * C + D)
    N, pad = 120, (0, 4, 3)[C % 3]
    X = rng.standard_normal((N, D)).astype(F32)
    X[N - 1] = X[0]
    X[N - 4] = X[2]
    X[10] = 0.0
    sqn = (X.astype(np.float64) ** 2).sum(1).astype(F32)
    Xw = np.full((N, D + pad), 1e30, dtype=F32)
    Xw[:, :D] = X
    Qn = rng.standard_normal((M, D))
    Qn /= np.linalg.norm(Qn, axis=1, keepdims=True)
    cand = np.stack([rng.permutation(np.arange(3, N - 4))[:C] for _ in range(M)]).astype(np.int64)
    for q in range(M):
        head = [N - 1, 0, 10, N - 4, 2][:C]
        cand[q, : len(head)] = head
        if C > 8:
            cand[q, rng.random(C) < 0.1] = -1
            cand[q, C - 1] = cand[q, 6] = 50  # a row listed twice
    if M > 2:
        cand[M - 1] = -1
    for k in sorted({1, min(10, C), C}):
        rc, s, r = _cos64_launch(Qn, Xw, D, sqn, cand, k)
        assert rc == 0
        es, er, eb = R.cos_rerank64_ref(Qn, X, sqn, cand, k)
        assert np.array_equal(r, er), (k, np.argwhere(r != er)[:5])
        assert np.array_equal(s == NEG_INF, es == NEG_INF)
        fin = es != NEG_INF
        err = np.abs(s[fin] - es[fin])
        assert np.all(err <= eb[fin]), (k, float((err / np.maximum(eb[fin], 1e-300)).max()))
        if fin.any() and (eb[fin] > 0).any():
            _note("cos_rerank64", (err[eb[fin] > 0] / eb[fin][eb[fin] > 0]).max())
    rc, s, r = _cos64_launch(Qn, Xw, D, sqn, cand, C + 3)
    assert rc != 0 and np.all(s == SENT_F) and np.all(r == SENT_I)


# ---------------------------------------------------------------- write_emb
def _graph(cap: int, D: int, w16: int, w8: int):
    """The columns ``ops.tenant_ops.write_emb`` touches, prefilled so that an
    unwritten element shows: sentinels in the first D columns, zeros beyond."""
    g = types.SimpleNamespace()
    g.emb32 = torch.full((cap, D), SENT_F, dtype=torch.float32, device=DEV)
    g.emb16 = torch.zeros((cap, w16), dtype=torch.bfloat16, device=DEV)
    g.emb16[:, :D] = 3.0
    g.emb8 = torch.zeros((cap, w8), dtype=torch.int8, device=DEV)
    g.emb8[:, :D] = 99
    g.rs8 = torch.full((cap,), SENT_F, dtype=torch.float32, device=DEV)
    g.sqn = torch.full((cap,), SENT_F, dtype=torch.float32, device=DEV)
    g.sumsq = torch.zeros(D, dtype=torch.float64, device=DEV)
    g._rs8_max = torch.zeros((), dtype=torch.float32, device=DEV)
    g.has_emb = torch.full((cap,), 7, dtype=torch.uint8, device=DEV)
    return g


def _bits32(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _check_rows(g, rows, ref, D):
    rows = np.asarray(rows)
    assert np.array_equal(_bits32(_np(g.emb32)[rows]), _bits32(ref["emb32"])), "emb32"
    b16 = _np(g.emb16.view(torch.int16)).view(np.uint16)[rows]
    assert np.array_equal(b16[:, :D], ref["emb16"]), np.argwhere(b16[:, :D] != ref["emb16"])[:5]
    assert not b16[:, D:].any(), "emb16 beyond D"
    e8 = _np(g.emb8)[rows]
    assert np.array_equal(e8[:, :D], ref["emb8"]), np.argwhere(e8[:, :D] != ref["emb8"])[:5]
    assert not e8[:, D:].any(), "emb8 beyond D"
    assert np.array_equal(_bits32(_np(g.rs8)[rows]), _bits32(ref["rs8"])), "rs8"
    assert np.array_equal(_np(g.has_emb)[rows], ref["has_emb"]), "has_emb"
    sq = _np(g.sqn)[rows].astype(np.float64)
    assert np.all(np.abs(sq - ref["s2"]) <= R.sqn_tol(ref["s2"])), (sq, ref["s2"])
    # the error model of the certified int8 search, in fp64, on what the kernel wrote
    vb = R.bf16_value(b16[:, :D]).astype(np.float64)
    rs = _np(g.rs8)[rows].astype(np.float64)[:, None]
    err = np.abs(vb - e8[:, :D].astype(np.float64) * rs)
    assert np.all(err <= rs / 2 * R.ERR_CAP_ANY), "derived cap"
    nz = rs[:, 0] > 0
    assert np.all(np.abs(e8[:, :D].astype(np.int32)).max(1)[nz] == 127) and not e8[~nz].any()
    return err, rs


def _ulp32(v):
    return float(np.spacing(F32(v)))


def _emb_rows(D: int, m: int, rng) -> np.ndarray:
    """m rows: the planted ones first (all nine when m allows, else picked by
    D so that every planted row is written alone somewhere), a zero row, unit
    Gaussian rows and plain Gaussian rows."""
    P = R.planted_rows(D, rng)
    if m < 12:
        i0 = (R.RERANK_DS.index(D) if D in R.RERANK_DS else D) * m
        return P[[(i0 + j) % len(P) for j in range(m)]]
    G_ = rng.standard_normal((m - 10, D))
    G_[::2] /= np.linalg.norm(G_[::2], axis=1, keepdims=True)
    return np.concatenate([P, np.zeros((1, D)), G_]).astype(F32)


@pytest.mark.parametrize("D", (4, 100, 256, 257, 768, 1024))
def test_write_emb_definition_gpu(D):
    """Three launches into one set of columns: 37 contiguous rows (every
    planted row, a zero row, Gaussian rows), 2 scattered rows that replace
    existing ones under a ``has`` mask, and 1 row; then a zero row and a masked
    row against fresh maxima."""
    rng = np.random.default_rng(D)
    cap, w16, w8 = 64, ((D + 63) // 64) * 64 + 64, ((D + 127) // 128) * 128
    g = _graph(cap, D, w16, w8)
    dv = torch.zeros(1, dtype=torch.float32, device=DEV)
    before32 = _np(g.emb32).copy()
    total = np.zeros(D)
    added = 0
    rs_max = dv_max = 0.0
    steps = (("row0", 3, _emb_rows(D, 37, rng), None), ("rows", [20, 5], _emb_rows(D, 2, rng), [1, 0]),
             ("rows", [41], _emb_rows(D, 1, rng), None), ("row0", 50, _emb_rows(D, 2, rng)[::-1].copy(), [0, 1]))
    written = set()
    for how, where, x, has in steps:
        m = len(x)
        ref = R.write_emb_ref(x, has)
        hd = _dev(np.asarray(has, dtype=np.uint8)) if has is not None else None
        if how == "row0":
            rows = list(range(where, where + m))
            T.write_emb(g, _dev(x), hd, None, dv, row0=where, has_emb=True)
        else:
            rows = where
            T.write_emb(g, _dev(x), hd, _dev(np.asarray(rows, dtype=np.int64)), dv, has_emb=True)
        torch.cuda.synchronize()
        written |= set(rows)
        _check_rows(g, rows, ref, D)
        total += ref["sumsq_inc"]
        added += m
        rs_max, dv_max = max(rs_max, float(ref["rs_max"])), max(dv_max, float(ref["dv_max"]))
        assert float(g._rs8_max) == rs_max, (float(g._rs8_max), rs_max)
        assert abs(float(dv[0]) - dv_max) <= _ulp32(dv_max), (float(dv[0]), dv_max)
        assert np.all(np.abs(_np(g.sumsq) - total) <= 1e-15 * added * total), "sumsq"
    rest = sorted(set(range(cap)) - written)
    assert np.array_equal(_np(g.emb32)[rest], before32[rest]) and np.all(_np(g.has_emb)[rest] == 7)
    # a zero row: the scale maximum stays; a has = 0 row: both maxima stay
    g._rs8_max.fill_(0.125)
    dv.fill_(0.25)
    T.write_emb(g, _dev(_emb_rows(D, 37, rng)[:1]), _dev(np.zeros(1, dtype=np.uint8)), None, dv, row0=60)
    assert float(g._rs8_max) == 0.125 and float(dv[0]) == 0.25
    T.write_emb(g, _dev(np.zeros((1, D), dtype=F32)), None, None, dv, row0=61)
    assert float(g._rs8_max) == 0.125 and float(dv[0]) == 1.0 and float(g.rs8[61]) == 0.0
    assert not _np(g.emb8)[61].any() and float(g.sqn[61]) == 0.0


@pytest.mark.parametrize("D", (4, 100, 768, 1024))
def test_write_emb_error_model_cap_gpu(D):
    """|vb - emb8 rs8| <= rs8 / 2 (1 + 2^-22) and a maximum of +-127, in fp64,
    for every element of the planted rows and of Gaussian rows scaled to a
    maximum of exactly 1 (the module docstring says why not of every row)."""
    x = R.error_cap_rows(D)
    g = _graph(40, D, D + 64, D + 128)
    dv = torch.zeros(1, dtype=torch.float32, device=DEV)
    T.write_emb(g, _dev(x), None, None, dv, row0=1, has_emb=True)
    torch.cuda.synchronize()
    err, rs = _check_rows(g, list(range(1, 1 + len(x))), R.write_emb_ref(x), D)
    assert np.all(err <= rs / 2 * R.ERR_CAP), float((err / np.maximum(rs / 2, 1e-300)).max() - 1)


def test_torch_quantiser_on_device_is_the_definition_gpu():
    """``quantize_i8_rows`` on the device (the writer of the int8 column for
    inserts above WRITE_EMB_MAX_ROWS) multiplies by fl32(1 / 127) like the
    kernel: scale and values are the definition's, bit for bit. (On the CPU
    torch divides; test_rerank_ref_cpu.py says what differs.)"""
    rng = np.random.default_rng(23)
    x = np.concatenate([R.planted_rows(256, rng), rng.standard_normal((300, 256)).astype(F32)])
    vb = R.bf16_value(R.bf16_bits(x))
    q, rs = R.quantize_def(vb)
    tq, ts = S.quantize_i8_rows(_dev(vb).to(torch.bfloat16))
    assert np.array_equal(_bits32(_np(ts)), _bits32(rs)) and np.array_equal(_np(tq), q)


@pytest.mark.parametrize("D,m", [(1028, 37), (768, 37), (768, 2), (100, 1)])
def test_add_nodes_embedding_columns_gpu(D, m):
    """``TenantGraph.add_nodes``: D = 1028 takes the chunked torch path (no
    int8 copy above 1024), D <= 1024 the kernel; both give the definition's
    columns, and the graph's ``max_norm_dev`` is the reference's ``dv_max``."""
    from lazzaro_amd.engine.tenant_graph import TenantGraph
    rng = np.random.default_rng(3 * D + m)
    x = _emb_rows(D, m, rng)
    ref = R.write_emb_ref(x)
    g = TenantGraph(device=DEV)
    g.add_nodes([f"a{i}" for i in range(m)], [""] * m, _dev(x), shard=g.shard_id("work"), stored=True)
    torch.cuda.synchronize()
    assert g.n == m
    assert np.array_equal(_bits32(_np(g.emb32[:m, :D])), _bits32(ref["emb32"]))
    b16 = _np(g.emb16[:m].view(torch.int16)).view(np.uint16)
    assert np.array_equal(b16[:, :D], ref["emb16"]) and not b16[:, D:].any()
    assert np.all(np.abs(_np(g.sqn[:m]).astype(np.float64) - ref["s2"]) <= R.sqn_tol(ref["s2"]))
    assert np.array_equal(_np(g.has_emb[:m]), ref["has_emb"])
    assert np.all(np.abs(_np(g.sumsq) - ref["sumsq_inc"]) <= 1e-15 * m * ref["sumsq_inc"])
    assert abs(g.max_norm_dev - float(ref["dv_max"])) <= _ulp32(ref["dv_max"])
    if D <= 1024:
        assert g.emb8 is not None and g.emb8.dtype == torch.int8
        e8 = _np(g.emb8[:m])
        assert np.array_equal(e8[:, :D], ref["emb8"]) and not e8[:, D:].any()
        assert np.array_equal(_bits32(_np(g.rs8[:m])), _bits32(ref["rs8"]))
        assert float(g._rs8_max) == float(ref["rs_max"])
    else:
        assert g.emb8 is None or g.emb8.dtype != torch.int8


# ---------------------------------------------------------------- centroids
CENT_SIZES = tuple(range(18)) + (1000,)  # the 8-row stride and the 4-wave tail on 0 .. 17 rows, and a long cluster


def _cent_rows(kind, D, rng):
    lab = R.cluster_labels(rng, CENT_SIZES, n_dead=25)
    n = len(lab)
    if kind == "grid":
        X = rng.integers(-8, 9, size=(n, D)).astype(np.float64)
        two = np.nonzero(lab == 2)[0]
        X[two[1]] = -X[two[0]]  # a mean that cancels to zero exactly
    else:
        X = R.to_bf16(rng.standard_normal((n, D)))
    return X, lab


def _centroids(X, lab, C, normalize, pad_to, stride_pad=8):
    n, D = X.shape
    Xw = torch.full((n, D + stride_pad), 1e30, dtype=torch.bfloat16, device=DEV)
    Xw[:, :D] = _dev(X.astype(F32)).to(torch.bfloat16)
    _poison(C * D * 4)
    _poison(C * pad_to * 2)
    c32, c16, cnt = G.centroids(Xw[:, :D], _dev(lab), C, normalize=normalize, pad_to=pad_to)
    torch.cuda.synchronize()
    return _np(c32), _np(c16.view(torch.int16)).view(np.uint16), _np(cnt)


@pytest.mark.parametrize("D", (4, 252, 256, 260, 2048))
@pytest.mark.parametrize("atomic", (False, True))
def test_centroids_gpu(monkeypatch, atomic, D):
    """Clusters of 0 .. 17 and 1000 rows, 25 rows labelled -1, rows a strided
    view. Counts exact; on the exact grid the means equal ``fl32(sum / count)``
    bit for bit (both paths); Gaussian means and normalised centroids within
    their bounds; normalised rows unit within ``unit_bound``; empty clusters
    and a mean that cancels give zero rows; the bf16 copy is the RNE of the
    returned fp32 value and its padding is zero."""
    monkeypatch.setattr(G, "SEG_SUM_ATOMIC", atomic)
    rng = np.random.default_rng(D + atomic)
    C, pad_to = len(CENT_SIZES), ((D + 63) // 64) * 64 + 64
    X, lab = _cent_rows("grid", D, rng)
    sums, cnt_ref, _ = R.seg_sum_ref(X, lab, C)
    c32, c16, cnt = _centroids(X, lab, C, False, pad_to)
    assert np.array_equal(cnt, cnt_ref) and np.array_equal(cnt, CENT_SIZES)
    want = (sums.astype(F32) / np.maximum(cnt_ref, 1).astype(F32)[:, None]).astype(F32)
    assert np.array_equal(_bits32(c32 + F32(0.0)), _bits32(want + F32(0.0))), np.argwhere(c32 != want)[:5]
    assert np.array_equal(c16, R.centroid_bf16_ref(c32, pad_to))
    c32, c16, cnt = _centroids(X, lab, C, True, pad_to)
    assert not c32[0].any() and not c32[2].any() and not c16[0].any() and not c16[2].any()
    assert np.array_equal(c16, R.centroid_bf16_ref(c32, pad_to))
    X, lab = _cent_rows("gauss", D, rng)
    for normalize in (False, True):
        ref, bound, cnt_ref = R.centroid_ref(X, lab, C, normalize=normalize)
        c32, c16, cnt = _centroids(X, lab, C, normalize, pad_to)
        assert np.array_equal(cnt, cnt_ref)
        err = np.abs(c32.astype(np.float64) - ref)
        assert np.all(err <= bound), np.argwhere(err > bound)[:5]
        fin = np.isfinite(bound) & (bound > 0)
        _note("centroids" + (" normalised" if normalize else ""), (err[fin] / bound[fin]).max())
        assert not c32[0].any()
        assert np.array_equal(c16, R.centroid_bf16_ref(c32, pad_to)) and not c16[:, D:].any()
        if normalize:
            nrm = np.sqrt((c32.astype(np.float64) ** 2).sum(1))[1:]
            assert np.all(np.abs(nrm - 1.0) <= R.unit_bound(D)), np.abs(nrm - 1.0).max()


# ---------------------------------------------------------------- pairs
@pytest.mark.parametrize("D", (64, 128, 768))
@pytest.mark.parametrize("n", (1, 2, 127, 128, 129, 257))
def test_pairs_gpu(n, D):
    """Every certainly-above pair is returned, no certainly-below one, each
    pair once with i < j in (i, j) order; the band between holds at most 1 %
    of the returned pairs (the planted ones are far from tau)."""
    rng = np.random.default_rng(n * 1000 + D)
    X = R.pair_rows(n, D, rng)
    above, below, band = R.pairs_ref(X, R.PAIR_TAU)
    got = _np(G.pairs_above(_dev(X.astype(F32)).to(torch.bfloat16), R.PAIR_TAU))
    assert got.dtype == np.int32 and got.shape == (len(got), 2)
    pairs = [tuple(p) for p in got.tolist()]
    assert all(i < j for i, j in pairs) and pairs == sorted(set(pairs))
    assert above <= set(pairs) and not (set(pairs) & below)
    assert len(set(pairs) & band) <= 0.01 * max(len(pairs), 1)
    if n >= 2:
        assert (0, 1) in above
    if n > 130:
        assert {(5, 100), (3, 130), (127, 128), (10, 70)} <= above and (11, 126) in below


def test_pairs_overflow_gpu():
    """A buffer of 8 for 66 + pairs: the complete set comes back (the count is
    known after the first launch; the second has room for it)."""
    rng = np.random.default_rng(9)
    n, D = 129, 128
    X = R.pair_rows(n, D, rng)
    for r in (20, 21, 22, 23, 24, 25, 26, 27, 90, 101, 128):  # 12 rows equal to row 19: 66 pairs
        X[r] = X[19]
    above, below, band = R.pairs_ref(X, R.PAIR_TAU)
    assert len(above) >= 66 and not band
    Xd = _dev(X.astype(F32)).to(torch.bfloat16)
    got = {tuple(p) for p in _np(G.pairs_above(Xd, R.PAIR_TAU, max_pairs=8)).tolist()}
    assert got == above
    assert {tuple(p) for p in _np(G.pairs_above(Xd, R.PAIR_TAU, max_pairs=len(above))).tolist()} == above
    assert {tuple(p) for p in _np(G.pairs_above(Xd, R.PAIR_TAU)).tolist()} == above


# ---------------------------------------------------------------- row_cent_cos
@pytest.mark.parametrize("D", (4, 64, 252, 760, 2048))
def test_row_cent_cos_gpu(D):
    """Values within gamma(ceil(D / 256) + 13) sum|x c| / |x| of the fp64
    cosine; -1 exactly for a row without a vector; rows a padded view. The
    unit-centroid form of the bound stays below the slack its consumer
    subtracts, for every D up to 2048."""
    from lazzaro_amd.parallel.sharded_memory import ShardedMemorySystem
    rng = np.random.default_rng(D)
    N, K, m = 90, 7, 37
    X = (rng.standard_normal((N, D)) * rng.uniform(0.2, 3.0, size=(N, 1))).astype(F32)
    X[13] = 0.0
    sqn = (X.astype(np.float64) ** 2).sum(1).astype(F32)
    Cc = rng.standard_normal((K, D))
    Cc = (Cc / np.linalg.norm(Cc, axis=1, keepdims=True)).astype(F32)
    rows = rng.integers(0, N, size=m)
    rows[:3] = (13, 0, 13)
    rows[5] = rows[6]
    lab = rng.integers(0, K, size=m)
    lab[4] = lab[5] = int(np.argmax(np.abs(Cc @ X[rows[4]])))
    Xw = torch.full((N, D + 12), 1e30, dtype=torch.float32, device=DEV)
    Xw[:, :D] = _dev(X)
    _poison(m * 4)
    got = _np(T.row_centroid_cos(Xw[:, :D], D, _dev(sqn), _dev(rows), _dev(lab), _dev(Cc)))
    cos, bound = R.row_cent_cos_ref(X, D, sqn, rows, lab, Cc)
    assert got[0] == -1.0 and got[2] == -1.0
    err = np.abs(got.astype(np.float64) - cos)
    assert np.all(err <= bound), (err / np.maximum(bound, 1e-300)).max()
    _note("row_cent_cos", (err[bound > 0] / bound[bound > 0]).max())
    cn = float(np.linalg.norm(Cc.astype(np.float64), axis=1).max())
    assert cn <= 1.0 + 2.0 ** -20 and np.all(bound <= R.cent_cos_unit_bound(D))
    assert all(R.cent_cos_unit_bound(d) < ShardedMemorySystem.REACH_SLACK for d in range(4, 2049, 4))
