"""The certified int8 store search (ops.search ``flat_topk_i8``) end to end
on data where it can actually go wrong, against the fp64 ranking of the bf16
inputs (tests/kernels/_cand_ref.py) -- not against another kernel.

N = 10,253 rows, D = 128, k = 10: the smallest store at which the threshold
sample has stride S = 64 and the speculative threshold is on; nq = 5 takes
the narrow scan (scan8.hip), the block-per-query select / cut and the split
re-score, nq = 200 the persistent 256 x 256 scan and the wave kernels. Rows are
bf16, or ``LeanRows`` (fp32 rows holding the bf16 values, margins widened by
2^-8 |q| |x| as TenantGraph._i8_candidates does). ``margin_rig`` comes from
``i8_query`` with smax = the largest row scale and xn = the largest row norm +
2^-7. Every store is repaired on the host until, per query, the fp64 scores of
ranks 1 .. k + 1 differ by more than 16 score bounds, so the expected rows are
unambiguous for any correct fp32 re-score.

Observed on one MI355X: the 29 cases take 5.0 s together; the slowest,
test_near_ties_below_the_int8_noise_gpu[200-False-rig], 1.1 s (it builds the
nq = 200 store on the host).
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from lazzaro_amd.ops import _lib  # noqa: E402
from lazzaro_amd.ops import search as S  # noqa: E402
from tests.kernels import _cand_ref as R  # noqa: E402

DEV = "cuda"
N, D, K = 10253, 128, 10
ALPHA = 2.0
NEG_INF = float("-inf")
GAP = 16.0   # ranks 1 .. k + 1 are this many score bounds apart
TIE_NORM = 1.5
GUARD = 4.0  # a certificate decision this close to its level may go either way
F32 = np.float32


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(dtype) if dtype is not None else t).to(DEV)


def _bias_of(X):
    return -(X.astype(F32) ** 2).sum(1, dtype=F32)


def _scores(X, Q, bias):
    return ALPHA * (Q @ X.T) + bias.astype(np.float64)[None, :]


def _top(s, n):
    rows = np.argsort(-s, axis=1, kind="stable")[:, :n]  # (score desc, row asc)
    return np.take_along_axis(s, rows, 1), rows


def _bound_at(X, Q, bias, rows):
    return np.stack([R.score_ref(X, Q[q], rows[q], bias, ALPHA)[1] for q in range(Q.shape[0])])


def _near(rng, mean, c=0.98):
    u = rng.standard_normal(D)
    return R.to_bf16((c * mean + np.sqrt(1.0 - c * c) * u / np.linalg.norm(u))[None, :])[0]


def _repair(rng, X, Q, bias, protected, pure=None):
    """Replace rows with fresh Gaussian ones until ranks 1 .. K + 1 of every
    query are more than GAP score bounds apart (``protected``: row -> the
    direction it was planted around), and the top K of the queries ``pure``
    are protected rows only. Returns the replaced rows."""
    gone = []
    for _ in range(60):
        s, rows = _top(_scores(X, Q, bias), K + 1)
        b = _bound_at(X, Q, bias, rows)
        bad = (s[:, :-1] - s[:, 1:]) <= GAP * np.maximum(b[:, :-1], b[:, 1:])
        victims = set()
        if pure is not None:
            victims.update(int(r) for r in rows[pure, :K].ravel() if int(r) not in protected)
        if not bad.any() and not victims:
            return gone
        for q, i in zip(*np.nonzero(bad)):
            lo, hi = int(rows[q, i + 1]), int(rows[q, i])
            victims.add(lo if lo not in protected or hi in protected else hi)
        for v in sorted(victims):
            if v in protected:  # a planted row keeps its role: the same direction, fresh noise
                X[v] = _near(rng, protected[v])
                continue
            X[v] = R.to_bf16(R.unit_rows(rng, 1, D))[0]
            gone.append(v)
        bias[:] = _bias_of(X)
    raise AssertionError("the store did not settle")


@functools.lru_cache(maxsize=None)
def _store(kind, nq):
    """(X, Q, bias, planted queries, fp64 scores) of one scenario: bf16 values
    as fp64, bias = -|x|^2 in fp32 (alpha = 2: the L2 search)."""
    rng = np.random.default_rng({"ties": 1, "cert": 2, "few": 3}[kind] * 1000 + nq)
    X = R.to_bf16(R.unit_rows(rng, N, D))
    Q = R.to_bf16(R.unit_rows(rng, nq, D))
    planted = np.zeros(nq, dtype=bool)
    protected = {}
    owner = np.full(N, -1)
    if kind == "cert":
        # a third of the queries, in groups of 5 mutually orthogonal ones: ten rows close to the group's mean
        # direction sit at multiples of the sample stride and are the true top-10 of each query of the group
        planted[::3] = True
        pq = np.flatnonzero(planted)
        slots = iter(rng.permutation(np.arange(0, N, 64)))
        for g0 in range(0, pq.size, 5):
            grp = pq[g0: g0 + 5]
            G = np.linalg.qr(Q[grp].T)[0].T * np.sign(np.sum(np.linalg.qr(Q[grp].T)[0].T * Q[grp], axis=1))[:, None]
            Q[grp] = R.to_bf16(G)
            mean = Q[grp].sum(0) / np.linalg.norm(Q[grp].sum(0))
            for _ in range(K):  # (scores too close to each other are settled by _repair)
                r = int(next(slots))
                X[r] = _near(rng, mean)
                protected[r] = mean
    bias = _bias_of(X)
    if kind == "ties":
        # per query 40 rows whose scores straddle its k-th best ~7.5e-4 apart: under the ~2e-3 int8 error (the
        # int8 order of these rows is scrambled), over GAP bounds (the bf16 order is not). They have norm 1.5:
        # with bias = -|x|^2 they score about -2.25 for every other query, far below its top rows, so one
        # query's cluster never displaces another's
        pool = iter(rng.permutation(N))
        for q in range(nq):
            s = _scores(X, Q[q: q + 1], bias)[0]
            top = np.sort(s)[::-1][: K + 2]
            T = top[K - 5]  # 5 rows above it + 4 planted ones: this row becomes the k-th best, rivals on both sides
            qn = Q[q] / np.linalg.norm(Q[q])
            lvl = T + rng.uniform(-0.036, 0.005, size=800)
            a = (lvl + TIE_NORM ** 2) / (ALPHA * np.linalg.norm(Q[q]))
            U = rng.standard_normal((800, D))
            U -= (U @ qn)[:, None] * qn[None, :]
            U /= np.linalg.norm(U, axis=1, keepdims=True)
            C = R.to_bf16(a[:, None] * qn[None, :] + np.sqrt(TIE_NORM ** 2 - a ** 2)[:, None] * U)
            cs = ALPHA * (C @ Q[q]) + _bias_of(C).astype(np.float64)
            taken, n_hi, n_lo = list(top), 0, 0
            for j in np.argsort(np.abs(cs - T)):
                hi = cs[j] > T
                if (n_hi >= 4 if hi else n_lo >= 36) or np.abs(np.array(taken) - cs[j]).min() < 7e-4:
                    continue
                r = int(next(pool))
                X[r], owner[r] = C[j], q
                taken.append(cs[j])
                n_hi, n_lo = n_hi + hi, n_lo + (not hi)
                if n_hi + n_lo == 40:
                    break
            bias = _bias_of(X)
    if kind == "few":
        live = rng.permutation(N)[:7]
        live[0] = 64 * 3  # one of the seven is a sample row
        dead = np.ones(N, dtype=bool)
        dead[live] = False
    gone = _repair(rng, X, Q, bias, protected, planted if kind == "cert" else None)
    owner[gone] = -1
    if kind == "ties":
        s, rows = _top(_scores(X, Q, bias), K + 15)
        for q in range(nq):  # the cluster is still there: the k-th best and its neighbours ARE planted rows
            assert (owner == q).sum() >= 30 and (owner[rows[q, K - 4: K + 12]] == q).sum() >= 10, q
            assert min(s[q, K - 2] - s[q, K - 1], s[q, K - 1] - s[q, K]) < 1.2e-3, q  # a rival closer than the int8 error
    if kind == "few":
        bias[dead] = NEG_INF
    sc = _scores(X, Q, bias)
    if kind == "cert":
        _, rows = _top(sc, K)
        assert (rows[planted] % 64 == 0).all()  # the planted queries' true top-10 lies inside the 1/S sample
    return X, Q, bias, planted, sc


def _search(X, Q, bias, lean, margin_mode="rig", monkeypatch=None):
    """flat_topk_i8 the way TenantGraph._i8_candidates drives it. Returns
    (scores, rows, margin_rig, the ``need`` handed to the select -- with a
    monkeypatch only) on the host."""
    L = _lib.lib()
    nq = Q.shape[0]
    X16, Q16 = _dev(X, torch.bfloat16), _dev(Q, torch.bfloat16)
    b = _dev(bias)
    X8, rs = S.quantize_i8_rows(X16)
    norms = np.linalg.norm(X, axis=1)
    xn = float(norms.max()) + 2.0 ** -7
    sumsq = (X16.double() ** 2).sum(0).contiguous()
    smax = rs.max().reshape(1).contiguous()
    q8, qs, margin, mr = S.i8_query(Q16, D, sumsq, N, smax, ALPHA, 3.0, xn)
    rows_op = X16
    if lean:
        X32, Q32 = X16.float().contiguous(), Q16.float().contiguous()
        w = ALPHA * 2.0 ** -8 * Q32.norm(dim=1) * float(norms.max())
        mr = (mr + w).contiguous()
        rows_op = S.LeanRows(X32, D, Q32)
    mg = {"rig": mr, "zero": torch.zeros_like(mr)}[margin_mode]
    seen = {}
    if monkeypatch is not None:
        inner = S._select_with_fallback

        def spy(*a, **kw):
            seen["need"] = kw.get("need")
            return inner(*a, **kw)
        monkeypatch.setattr(S, "_select_with_fallback", spy)
    kslot = L.lzk_flat_topk_kslot(K)
    assert max(1, min(64, N // (16 * kslot))) == 64 and 64 >= S.SPEC_MIN_STRIDE  # S = 64, speculative threshold on
    s, r = S.flat_topk_i8(X8, rs, q8, qs, rows_op, Q16, K, bias=b, alpha=ALPHA, margin=mg, margin_rig=mr)
    torch.cuda.synchronize()
    need = seen["need"].cpu().numpy() if seen.get("need") is not None else None
    return s.cpu().numpy().astype(np.float64), r.cpu().numpy(), mr.cpu().numpy().astype(np.float64), need


def _assert_exact(X, Q, bias, sc, s, r):
    e_s, e_r = _top(sc, K)
    e_r = np.where(e_s == NEG_INF, -1, e_r)
    assert np.array_equal(r, e_r), np.flatnonzero((r != e_r).any(1))[:8]
    b = _bound_at(X, Q, bias, np.maximum(e_r, 0))
    live = e_s != NEG_INF
    assert np.array_equal(s == NEG_INF, ~live)
    assert (np.abs(s[live] - e_s[live]) <= b[live]).all()


@pytest.mark.parametrize("margin_mode", ["rig", "zero"])
@pytest.mark.parametrize("lean", [False, True])
@pytest.mark.parametrize("nq", [5, 200])
def test_near_ties_below_the_int8_noise_gpu(nq, lean, margin_mode):
    """40 planted rows per query straddle its k-th best ~7.5e-4 apart, under the
    int8 error: the scan's order of them is scrambled, the result must not be.
    margin = margin_rig, and margin = 0 with margin_rig kept (a scan threshold
    without allowance: the certificate and the fallback carry the result)."""
    X, Q, bias, _, sc = _store("ties", nq)
    s, r, _, _ = _search(X, Q, bias, lean, margin_mode)
    _assert_exact(X, Q, bias, sc, s, r)


@pytest.mark.parametrize("lean", [False, True])
@pytest.mark.parametrize("nq", [5, 200])
def test_certificate_fires_exactly_when_it_must_gpu(nq, lean, monkeypatch):
    """A third of the queries have their true top-10 inside the 1/S sample, so
    their speculative threshold (the sample's 3rd / 5th best) sits above their
    k-th score: the certificate must send them to the fallback. The others
    go there iff fewer than k rows have a bf16 score >= the certificate level
    (fp64 prediction; queries whose k-th score is within GUARD score bounds of
    the level may go either way and are not counted).
    Observed: nq = 5: 0 of 3 unplanted queries inside the guard, 3 certified,
    2 queries sent to the fallback; nq = 200: 0 of 133 inside the guard (0 %),
    131 certified, 69 sent to the fallback (bf16 and lean rows alike)."""
    X, Q, bias, planted, sc = _store("cert", nq)
    monkeypatch.setattr(S, "SPEC_STATS", [])
    s, r, mr, need = _search(X, Q, bias, lean, "rig", monkeypatch)
    stats = [int(v) for v in S.SPEC_STATS]
    _assert_exact(X, Q, bias, sc, s, r)
    # the certificate level from fp64: the sample's J-th best, minus its slack, - margin + margin_rig, + slack
    J = S.SPEC_J_NARROW if nq < S.NARROW_MAX_Q else S.SPEC_J
    sJ = np.sort(sc[:, ::64], axis=1)[:, ::-1][:, J - 1]
    tau = sJ - R.C_2E4 * (1.0 + np.abs(sJ))
    cert = tau - mr + mr
    cert = cert + R.C_1E6 * (1.0 + np.abs(cert))
    e_s, e_r = _top(sc, K)
    kth = e_s[:, K - 1]
    b = _bound_at(X, Q, bias, e_r)[:, K - 1] + R.gamma(D + 3) * (1.0 + np.abs(sJ))  # (+ the sample's own rounding)
    amb = np.abs(kth - cert) <= GUARD * b
    certified = kth >= cert
    assert not certified[planted].any() and not amb[planted].any()
    un = ~planted
    print(f"nq={nq} lean={lean}: unplanted {int(un.sum())}, inside the guard {int((amb & un).sum())}, "
          f"certified {int((certified & un & ~amb).sum())}, fallback count {stats}")
    assert (amb & un).sum() <= 0.05 * un.sum()
    assert (certified & un & ~amb).sum() >= 0.5 * un.sum()
    assert need is not None and len(stats) == 1
    fb = need != 0
    assert fb[planted].all()  # every planted query went to the exact fallback
    clear = un & ~amb
    assert np.array_equal(fb[clear], ~certified[clear])  # and of the others exactly those the reference predicts
    lo = int(planted.sum() + (~certified & clear).sum())
    assert lo <= stats[0] <= lo + int((amb & un).sum()) and stats[0] == int(fb.sum())


@pytest.mark.parametrize("lean", [False, True])
@pytest.mark.parametrize("nq", [5, 200])
def test_fewer_live_rows_than_k_gpu(nq, lean):
    """All but 7 rows carry bias = -inf: the 7, then (-inf, -1) padding."""
    X, Q, bias, _, sc = _store("few", nq)
    assert (np.isfinite(sc).sum(1) == 7).all()
    s, r, _, _ = _search(X, Q, bias, lean)
    _assert_exact(X, Q, bias, sc, s, r)
    assert (r[:, 7:] == -1).all() and (s[:, 7:] == NEG_INF).all() and (r[:, :7] >= 0).all()


@pytest.mark.parametrize("lean", [False, True])
@pytest.mark.parametrize("nq", [5, 200])
def test_overflowing_lists_resolve_ties_by_row_gpu(nq, lean, monkeypatch):
    """Every row equals query 0, so each query scores all rows alike and every
    list overflows (cnt > cap; the narrow list capacity lowered so that it
    does at this N): _select_with_fallback recomputes them, the lean variant
    through _lean_fallback over 4096-row blocks whose partial results merge.
    Ties resolve by row: the ten smallest live rows."""
    rng = np.random.default_rng(50 + nq)
    Q = R.to_bf16(R.unit_rows(rng, nq, D))
    X = np.repeat(Q[:1], N, axis=0)
    bias = _bias_of(X)
    bias[[0, 1, 5, 4096, 4100]] = NEG_INF
    monkeypatch.setattr(S, "NARROW_CAP", 2048)
    monkeypatch.setattr(S.LeanRows, "CHUNK", 4096)
    sink = []
    inner = S._select_with_fallback

    def spy(*a, **kw):
        kw["ovf_sink"] = sink
        return inner(*a, **kw)
    monkeypatch.setattr(S, "_select_with_fallback", spy)
    s, r, _, _ = _search(X, Q, bias, lean)
    ovf, cnt = sink[0]
    assert bool((ovf == 1).all()) and int(cnt.min()) > 16 * 10 * 64  # every list past its capacity
    want = np.array([2, 3, 4, 6, 7, 8, 9, 10, 11, 12])
    assert np.array_equal(r, np.repeat(want[None, :], nq, 0))
    e, b = R.score_ref(X, Q[0], want, bias, ALPHA)
    for q in range(nq):
        e, b = R.score_ref(X, Q[q], want, bias, ALPHA)
        assert (np.abs(s[q] - e) <= b).all(), q


@pytest.mark.parametrize("nq", [1, 7, 300])
@pytest.mark.parametrize("d,Dp", [(100, 128), (100, 384), (384, 384)])
def test_i8_query_kernel_below_the_padded_width_gpu(d, Dp, nq):
    """lzk_i8_query with d < Dp (zero padding): q8 / qs equal quantize_i8_rows,
    margin_rig within 1e-5 of the fp64 reference and never below it by more
    than 1e-6 relative."""
    rng = np.random.default_rng(d + Dp + nq)
    q = np.zeros((nq, Dp))
    q[:, :d] = R.to_bf16(R.unit_rows(rng, nq, d))
    if nq > 1:
        q[nq // 2] = 0.0
    Xs = R.to_bf16(R.unit_rows(rng, 500, d))
    Q16 = _dev(q, torch.bfloat16)
    sumsq = _dev((Xs ** 2).sum(0))
    assert sumsq.dtype == torch.float64
    smax_v, xn = float(np.abs(Xs).max() / 127.0), 1.0 + 2.0 ** -7
    smax = torch.tensor([smax_v], dtype=torch.float32, device=DEV)
    for alpha in (1.0, 2.0):
        q8, qs, margin, mr = S.i8_query(Q16, d, sumsq, 500, smax, alpha, 3.0, xn)
        torch.cuda.synchronize()
        e8, es = S.quantize_i8_rows(Q16)
        assert torch.equal(q8, e8) and torch.equal(qs, es)
        ref = R.margin_rig_ref(q, d, float(smax[0]), alpha, xn, q8.cpu().numpy(), qs.cpu().numpy())
        got = mr.cpu().numpy().astype(np.float64)
        assert np.allclose(got, ref, rtol=1e-5, atol=0.0)
        assert (got >= ref * (1.0 - 1e-6)).all(), float((got / ref).min())
        assert bool((margin >= 0).all()) and bool((mr >= margin).all())
