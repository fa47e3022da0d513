"""The cross-tenant tile-table search (csrc/kernels/mtscan.hip) stage by stage
and end to end, held against tests/kernels/_mt_ref.py: ``lzk_mt_sample``,
``lzk_mt_cand`` and ``lzk_mt_rerank`` through ``_lib.lib()`` on hand-built
tenants (plain tensors: fp32 rows, bf16 rows of stride Dp, bias, kind bytes and
the address tables), then ``mt_topk``. Exact-grid inputs (integers in [-8, 8],
bias ``-|x|^2``, alpha 2 or 1) are compared bit for bit, ties included;
Gaussian inputs (rows of norm 1 and 4) within the derived bounds of the
reference module.

Every address a kernel may dereference -- also a kernel that is wrong -- lies
inside a live allocation: a tenant's columns are allocated rounded up to a
whole tile plus one spare tile, the per-slot address tables name a spare
allocation of the largest tenant's size at every unused slot, the tile arrays
carry spare entries that repeat tile 0, the candidate and result buffers sit
between canary regions that are checked afterwards, and every tensor stays
referenced until after the synchronize. No case relies on a fault.

Observed on one MI355X: the 108 cases take 7.6 s together; the slowest,
test_mt_sample_bits_gpu[64] (the first case: it loads the library), 0.44 s,
then test_mt_topk_grid_bits_gpu[768-10-300], 0.38 s.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from lazzaro_amd.ops import _lib  # noqa: E402
from lazzaro_amd.ops import search as S  # noqa: E402
from tests.kernels import _mt_ref as R  # noqa: E402

DEV = "cuda"
NEG_INF = float("-inf")
EINVAL = 1  # hipErrorInvalidValue
GUARD = 1024  # canary elements on either side of a guarded buffer


def _st():
    return _lib.stream_ptr(torch.device(DEV))


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(dtype) if dtype is not None else t).to(DEV)


def _f32bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.int32)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


class Guarded:
    """``n`` elements between two canary regions of one allocation."""

    def __init__(self, n, dtype, fill, canary):
        self.buf = torch.full((n + 2 * GUARD,), canary, dtype=dtype, device=DEV)
        self.t = self.buf[GUARD: GUARD + n]
        self.t.fill_(fill)
        self.canary = canary

    def intact(self):
        c = torch.full((GUARD,), self.canary, dtype=self.buf.dtype, device=DEV)
        return bool(torch.equal(self.buf[:GUARD], c)) and bool(torch.equal(self.buf[-GUARD:], c))


class DevTenants:
    """Tenants on the device and their tables. ``tab`` is the reference Table
    (sort=False: tiles in list order; sort=True: ascending slots) and the tile
    arrays here follow it."""

    def __init__(self, tenants, Dp, sort):
        self.tab = tab = R.Table(tenants, sort=sort)
        self.tenants = tenants
        self.Dp, self.D = Dp, tab.D
        D = tab.D
        self.cols = {}
        amax = 0
        for t in tenants:
            n = len(t.bias)
            na = -(-n // R.MT_TILE) * R.MT_TILE + R.MT_TILE
            amax = max(amax, na)
            x32 = torch.zeros((na, D), dtype=torch.float32, device=DEV)
            x32[:n] = _dev(t.X)
            x16 = torch.zeros((na, Dp), dtype=torch.bfloat16, device=DEV)
            x16[:n, :D] = x32[:n].to(torch.bfloat16)
            b = torch.zeros(na, dtype=torch.float32, device=DEV)  # spare rows: a finite bias, a live node
            b[:n] = _dev(t.bias)
            kind = torch.full((na,), R.NODE, dtype=torch.uint8, device=DEV)
            kind[:n] = _dev(t.kind)
            self.cols[t.slot] = (x32, x16, b, kind)
        self.spare = (torch.zeros((amax, D), dtype=torch.float32, device=DEV),
                      torch.zeros(amax, dtype=torch.float32, device=DEV),
                      torch.zeros(amax, dtype=torch.uint8, device=DEV))
        nslot = max(t.slot for t in tenants) + 2
        pe = np.full(nslot, self.spare[0].data_ptr(), dtype=np.int64)
        pb = np.full(nslot, self.spare[1].data_ptr(), dtype=np.int64)
        pk = np.full(nslot, self.spare[2].data_ptr(), dtype=np.int64)
        for s, (x32, _, b, kind) in self.cols.items():
            pe[s], pb[s], pk[s] = x32.data_ptr(), b.data_ptr(), kind.data_ptr()
        self.p_e32, self.p_bias, self.p_kind = _dev(pe), _dev(pb), _dev(pk)
        # tile arrays (+ 8 spare entries repeating tile 0)
        tx = [self.cols[int(s)][1].data_ptr() + int(r0) * Dp * 2 for s, r0 in zip(tab.t_slot, tab.t_row0)]
        tb = [self.cols[int(s)][2].data_ptr() + int(r0) * 4 for s, r0 in zip(tab.t_slot, tab.t_row0)]

        def pad(a, dt):
            a = list(a)
            return _dev(np.array(a + a[:1] * 8, dtype=dt))
        self.t_x, self.t_b = pad(tx, np.int64), pad(tb, np.int64)
        self.t_n, self.t_slot, self.t_row0 = pad(tab.t_n, np.int32), pad(tab.t_slot, np.int32), pad(tab.t_row0, np.int32)
        self.n_tiles = tab.n_tiles

    def mt_tiles(self):
        """ops.search.MtTiles of the tenants in LIST order (unsorted slots)."""
        ts = self.tenants
        return S.MtTiles(np.array([t.slot for t in ts], np.int64), np.array([len(t.bias) for t in ts], np.int64),
                         np.array([self.cols[t.slot][1].data_ptr() for t in ts], np.int64),
                         np.array([self.cols[t.slot][2].data_ptr() for t in ts], np.int64), self.Dp, DEV)

    def queries16(self, Q):
        q = torch.zeros((Q.shape[0], self.Dp), dtype=torch.bfloat16, device=DEV)
        q[:, : self.D] = _dev(Q).to(torch.bfloat16)
        return q


def _force_stored(t: R.Tenant, rows):
    for r in rows:
        t.bias[r] = R.l2_bias(t.X[r: r + 1])[0]


MIXES = {1: [255], 7: [1, 63, 64, 65, 255, 257], 9: [256, 257, 700, 65, 1, 64],
         13: [1, 63, 64, 65, 255, 256, 257, 700, 1, 65]}


@functools.lru_cache(maxsize=None)
def _stage_case(n_tiles, D, Dp, family, norm=1.0):
    """Tenants of the tile mix (unsorted slots with gaps, list order kept), on
    the device, and 300 queries; the first tenant's row 0 and its planted copies
    are stored."""
    rng = np.random.default_rng(100 * n_tiles + D + (family == "grid"))
    counts = MIXES[n_tiles]
    tenants = R.make_tenants(rng, counts, R.e2e_slots(rng, len(counts)), D, family, norm=norm)
    for t in tenants:
        _force_stored(t, [0, len(t.bias) - 1])
    dt = DevTenants(tenants, Dp, sort=False)
    assert dt.n_tiles == n_tiles
    Q = (R.grid_queries(rng, 300, D) if family == "grid" else R.unit_rows(rng, 300, D)).astype(np.float32)
    return dt, Q


# ================================================================ lzk_mt_sample
@pytest.mark.parametrize("Dp", [64, 128, 768, 1032])
def test_mt_sample_bits_gpu(Dp):
    """Sample rows and biases bit-equal to sample_ref (a sample row with bias
    -inf included; Dp = 1032: the copy loop's second, partial round); nothing
    written past the last sample row."""
    L = _lib.lib()
    D = 96 if Dp == 128 else Dp
    rng = np.random.default_rng(Dp)
    counts = [257, 1, 65, 700, 64]
    tenants = R.make_tenants(rng, counts, R.e2e_slots(rng, len(counts)), D, "grid")
    tenants[0].bias[64] = NEG_INF
    tenants[3].bias[256] = NEG_INF
    dt = DevTenants(tenants, Dp, sort=False)
    s_tile, s_row, rows, bias = dt.tab.sample_ref(Dp)
    ns = s_tile.size
    assert ns == 5 + 1 + 2 + 4 + 4 + 3 + 1 and int((bias == NEG_INF).sum()) >= 2
    d_tile, d_row = _dev(s_tile, torch.int32), _dev(s_row, torch.int32)
    out = Guarded(ns * Dp, torch.bfloat16, 7.0, 3.0)
    outb = Guarded(ns, torch.float32, 7.0, 3.0)
    _lib.check(L.lzk_mt_sample(dt.t_x.data_ptr(), dt.t_b.data_ptr(), d_tile.data_ptr(), d_row.data_ptr(), ns, Dp, Dp,
                               out.t.data_ptr(), outb.t.data_ptr(), _st()), "lzk_mt_sample")
    torch.cuda.synchronize()
    want = torch.from_numpy(rows).to(torch.bfloat16).view(torch.int16)
    assert torch.equal(out.t.cpu().view(torch.int16).reshape(ns, Dp), want)
    assert np.array_equal(_bits(outb.t), _f32bits(bias))
    assert out.intact() and outb.intact()
    # argument checks: no launch
    for bad_ns, bad_dp, bad_ld in ((0, Dp, Dp), (-3, Dp, Dp), (ns, Dp - 4, Dp), (ns, Dp, Dp - 8)):
        out.t.fill_(7.0)
        rc = L.lzk_mt_sample(dt.t_x.data_ptr(), dt.t_b.data_ptr(), d_tile.data_ptr(), d_row.data_ptr(), bad_ns, bad_ld,
                             bad_dp, out.t.data_ptr(), outb.t.data_ptr(), _st())
        torch.cuda.synchronize()
        assert rc == EINVAL and bool((out.t == 7.0).all())


# ================================================================ lzk_mt_cand
def _run_cand(dt, Q16, nq, alpha, thr, cap):
    """One candidate pass into guarded lists. Returns (cnt [nq], cs bits
    [nq, cap], ci [nq, cap], canaries intact)."""
    L = _lib.lib()
    cnt = Guarded(nq, torch.int32, 0, 0x5a5a5a5a)
    cs = Guarded(nq * cap, torch.float32, float("nan"), 3.0)
    ci = Guarded(nq * cap, torch.int32, -7, 0x5a5a5a5a)
    d_thr = _dev(np.asarray(thr, dtype=np.float32))
    _lib.check(L.lzk_mt_cand(dt.t_x.data_ptr(), dt.t_b.data_ptr(), dt.t_n.data_ptr(), dt.n_tiles, dt.Dp,
                             Q16.data_ptr(), dt.Dp, nq, dt.Dp, float(alpha), d_thr.data_ptr(), cap, cnt.t.data_ptr(),
                             cs.t.data_ptr(), ci.t.data_ptr(), _st()), "lzk_mt_cand")
    torch.cuda.synchronize()
    ok = cnt.intact() and cs.intact() and ci.intact()
    return cnt.t.cpu().numpy(), _bits(cs.t).reshape(nq, cap), ci.t.cpu().numpy().reshape(nq, cap), ok


def _assert_lists_equal(cnt, csb, ci, ref, cap):
    for q, (ids, sc) in enumerate(ref):
        assert int(cnt[q]) == ids.size, q
        n = ids.size
        o = np.argsort(ci[q, :n], kind="stable")
        assert np.array_equal(ci[q, :n][o], ids), q  # nothing missing, nothing twice, nothing past a tile's count
        assert np.array_equal(csb[q, :n][o], _f32bits(sc)), q
        assert (ci[q, n:] == -7).all(), q


CAND_CASES = [(t, nq, 64, 64) for t in (1, 7, 9, 13) for nq in (1, 255, 256, 257, 300)] + \
             [(t, nq, D, Dp) for (D, Dp) in ((96, 128), (192, 192), (768, 768)) for t in (1, 7, 9, 13) for nq in (1, 300)]


@pytest.mark.parametrize("n_tiles,nq,D,Dp", CAND_CASES)
def test_mt_cand_grid_bits_gpu(n_tiles, nq, D, Dp):
    """Exact grid: every query's list, sorted, equals cand_ref as a set of (id,
    score bits) for thr = -inf (every stored row), + inf (none) and a value
    several duplicate rows attain (all of them members), alpha 2; alpha 1 at
    the tied threshold as well. Grids of 1, 7, 9, 13 blocks (and twice that
    for nq > 256): both branches of xcd_remap, grids that are no multiple of 8.
    Then cap = 8: cnt counts on, exactly 8 genuine members are written, the
    canaries around cnt / cs / ci are intact."""
    dt, Qall = _stage_case(n_tiles, D, Dp, "grid")
    Q = Qall[:nq]
    Q16 = dt.queries16(Q)
    tab = dt.tab
    cap = tab.N + 8
    for alpha in (2.0, 1.0):
        s, _ = tab.scan(Q, alpha, Dp)
        tied = s[:, 0].copy()  # the first tenant's row 0: stored, and planted again elsewhere
        assert (np.isfinite(tied)).all() and ((s == tied[:, None]).sum(1) >= 2).all()
        for thr in ((np.full(nq, NEG_INF), np.full(nq, np.inf), tied) if alpha == 2.0 else (tied,)):
            cnt, csb, ci, ok = _run_cand(dt, Q16, nq, alpha, thr, cap)
            assert ok
            ref = tab.cand_ref(Q, alpha, thr, Dp)
            if thr[0] == NEG_INF:
                assert all(ids.size == int(tab.stored.sum()) for ids, _ in ref)
            _assert_lists_equal(cnt, csb, ci, ref, cap)
    # a list that overflows: cap = 8
    thr = np.full(nq, NEG_INF)
    ref = tab.cand_ref(Q, 2.0, thr, Dp)
    cnt, csb, ci, ok = _run_cand(dt, Q16, nq, 2.0, thr, 8)
    assert ok
    for q, (ids, sc) in enumerate(ref):
        assert ids.size > 8 and int(cnt[q]) == ids.size, q
        got = ci[q]
        assert np.unique(got).size == 8 and np.isin(got, ids).all(), q
        pos = np.searchsorted(ids, got)
        assert np.array_equal(csb[q], _f32bits(sc[pos])), q


@pytest.mark.parametrize("D,norm", [(64, 1.0), (768, 1.0), (64, 4.0), (768, 4.0)])
def test_mt_cand_gauss_membership_gpu(D, norm):
    """Gaussian rows, 13 tiles, 300 queries, the threshold at each query's 40th
    best fp64 score: a row at or above thr + bound is a member, a row below thr
    - bound is not, every recorded score is within the bound of the fp64 one."""
    dt, Q = _stage_case(13, D, D, "gauss", norm)
    tab = dt.tab
    nq = Q.shape[0]
    s, b = tab.scan(Q, 2.0, D)
    thr = np.sort(np.where(np.isfinite(s), s, NEG_INF), axis=1)[:, -40].astype(np.float32).astype(np.float64)
    cap = tab.N + 8
    cnt, csb, ci, ok = _run_cand(dt, dt.queries16(Q), nq, 2.0, thr, cap)
    assert ok
    cs = csb.view(np.float32).astype(np.float64)
    worst = 0.0
    for q in range(nq):
        n = int(cnt[q])
        ids = ci[q, :n]
        assert np.unique(ids).size == n
        f = tab.flat_of_cid(ids)  # asserts: every id names a row inside its tile's count
        member = np.zeros(tab.N, dtype=bool)
        member[f] = True
        fin = np.isfinite(s[q])
        assert member[fin & (s[q] >= thr[q] + b[q])].all(), q
        assert not member[~fin | (s[q] < thr[q] - b[q])].any(), q
        err = np.abs(cs[q, :n] - s[q][f]) / b[q][f]
        worst = max(worst, float(err.max()))
        assert (err <= 1.0).all(), (q, float(err.max()))
    print(f"scan |error| / bound, worst: {worst:.3f}")


def test_mt_cand_argument_checks_gpu():
    L = _lib.lib()
    dt, Q = _stage_case(1, 64, 64, "grid")
    Q16 = dt.queries16(Q[:4])
    cnt = Guarded(4, torch.int32, 0, 0x5a5a5a5a)
    cs = Guarded(4 * 300, torch.float32, float("nan"), 3.0)
    ci = Guarded(4 * 300, torch.int32, -7, 0x5a5a5a5a)
    thr = torch.full((4,), NEG_INF, device=DEV)

    def call(n_tiles=1, ldx=64, ldq=64, nq=4, D=64, cap=300):
        rc = L.lzk_mt_cand(dt.t_x.data_ptr(), dt.t_b.data_ptr(), dt.t_n.data_ptr(), n_tiles, ldx, Q16.data_ptr(), ldq,
                           nq, D, 2.0, thr.data_ptr(), cap, cnt.t.data_ptr(), cs.t.data_ptr(), ci.t.data_ptr(), _st())
        torch.cuda.synchronize()
        return rc
    for kw in (dict(D=96, ldx=96, ldq=96), dict(D=32, ldx=64), dict(ldx=32), dict(ldq=32), dict(n_tiles=1 << 23),
               dict(n_tiles=0), dict(nq=0), dict(cap=0)):
        assert call(**kw) == EINVAL, kw
    assert bool((cnt.t == 0).all()) and bool((ci.t == -7).all()) and cnt.intact() and ci.intact() and cs.intact()
    assert call() == 0 and int(cnt.t[0]) == int(dt.tab.stored.sum())


# ================================================================ lzk_mt_rerank
RR_COUNTS = [257, 1, 65, 300]
RR_SLOTS = [9, 2, 30, 4]  # unsorted: the tile table's slot column is 9 9 2 30 4 4


@functools.lru_cache(maxsize=None)
def _rerank_case(D, family):
    rng = np.random.default_rng(31 * D + (family == "grid"))
    tenants = R.make_tenants(rng, RR_COUNTS, RR_SLOTS, D, family, norm=4.0 if D == 96 else 1.0)
    t0 = tenants[0]
    _force_stored(t0, [0, 1, 2, 3, 4, 5])
    t0.kind[[0, 2, 5]] = R.NODE
    t0.kind[1] = R.GHOST  # stored, not a node
    t0.kind[3] = R.FREE
    t0.bias[6] = NEG_INF  # a node that is not stored
    t0.kind[6] = R.NODE
    dt = DevTenants(tenants, D, sort=False)
    assert dt.tab.t_slot.tolist() == [9, 9, 2, 30, 4, 4]
    Q = (R.grid_queries(rng, 5, D) if family == "grid" else R.unit_rows(rng, 5, D)).astype(np.float32)
    Q[1] = t0.X[1] if family == "grid" else (t0.X[1] / np.linalg.norm(t0.X[1]))  # on the ghost: it ranks first
    Q[3] = t0.X[3] if family == "grid" else (t0.X[3] / np.linalg.norm(t0.X[3]))  # on the free row
    return dt, Q


def _rerank_lists(rng, tab, M, C):
    """[M, C] candidate ids: distinct per list; the first tenant's rows 0..6
    (ghost, free, unstored among them) and the rows planted as their copies in
    the other tenants first -- as many as fit --, then random rows; -1 holes in
    the middle and at the end; list 2 is all -1."""
    special = list(range(7))  # tile 0, rows 0..6
    for j, t in enumerate(tab.tenants[1:], start=1):
        n = len(t.bias)
        if n > 1:  # its last rows are copies of the first tenant's first rows
            m = min(n, 5)
            tl = np.nonzero(tab.t_ten == j)[0]
            for r in range(n - m, n):
                ti = tl[r // R.MT_TILE]
                special.append(int(ti) * R.MT_TILE + r % R.MT_TILE)
    cand = np.full((M, C), -1, dtype=np.int64)
    for q in range(M):
        if q == 2:
            continue
        pool = special + [int(c) for c in rng.permutation(tab.cid) if int(c) not in special]
        ids = np.array(pool[:C], dtype=np.int64)
        ids = ids[rng.permutation(C)]
        if C >= 10:
            ids[rng.permutation(C)[: C // 5]] = -1  # holes in the middle
            ids[C - 2:] = -1  # and at the end
        cand[q] = ids
    return cand


def _assert_ranked(gS, gK, eS, eK, eB, raw, rawB, tab, ex, bd, cand, exact):
    """Bit equality (grid) or, for Gaussian inputs: the same keys with scores
    within the bound; where the keys differ, every rank holds a row whose fp64
    score is within twice the bound of the reference's score at that rank."""
    if exact:
        assert np.array_equal(gK, eK)
        assert np.array_equal(_f32bits(gS), _f32bits(eS))
        return
    flat = {int(k): i for i, k in enumerate(tab.key)}
    for q in range(gK.shape[0]):
        if np.array_equal(gK[q], eK[q]):
            fin = eK[q] >= 0
            assert (np.abs(gS[q][fin] - eS[q][fin]) <= eB[q][fin]).all(), q
            assert (gS[q][~fin] == NEG_INF).all(), q
            continue
        live = gK[q][gK[q] >= 0]
        assert np.unique(live).size == live.size, q
        f = tab.flat_of_cid(cand[q][cand[q] >= 0])
        dead = f[(tab.kind[f] != R.NODE) & (ex[q][f] != NEG_INF)]
        for j in range(gK.shape[1]):
            if raw[q, j] == NEG_INF:
                assert gK[q, j] == -1 and gS[q, j] == NEG_INF, (q, j)
            elif gK[q, j] >= 0:
                i = flat[int(gK[q, j])]
                assert tab.kind[i] == R.NODE and abs(gS[q, j] - ex[q][i]) <= bd[q][i], (q, j)
                assert abs(ex[q][i] - raw[q, j]) <= 2.0 * max(bd[q][i], rawB[q, j]), (q, j)
            else:
                assert gS[q, j] == NEG_INF and (np.abs(ex[q][dead] - raw[q, j]) <= 2.0 * rawB[q, j]).any(), (q, j)


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("family", ["grid", "gauss"])
@pytest.mark.parametrize("D,ldq", [(40, 40), (64, 64), (64, 66), (96, 96), (768, 768)])
def test_mt_rerank_gpu(D, ldq, family, metric):
    """C in {1, 10, 16, 17, 32, 64} x k in {1, 6, 10, 16, C} (k <= C), M cycling
    through 1, 3, 4, 5 (a partial last block): scores and keys equal rerank_ref
    -- bit for bit on the grid, within the re-rank bound on Gaussian rows (norm 4
    at D = 96). D = 40 and ldq = 66 take the scalar path. Lists hold -1 holes,
    an all -1 list, rows planted in several tenants (ties broken by key under
    an unsorted slot column), ghost / free / unstored rows; queries 1 and 3 sit
    on the ghost and on the free row, so these rank below k, others above.
    The redo word is set exactly where a non-node took one of the k ranks and
    left alone elsewhere; nothing is written past query M - 1."""
    L = _lib.lib()
    dt, Q = _rerank_case(D, family)
    tab = dt.tab
    rng = np.random.default_rng(D + ldq)
    Qd = torch.zeros((5, ldq), dtype=torch.float32, device=DEV)
    Qd[:, :D] = _dev(Q)
    ms = [1, 3, 4, 5]
    n = 0
    seen_low = seen_high = False
    for C in (1, 10, 16, 17, 32, 64):
        for k in sorted({kk for kk in (1, 6, 10, 16, C) if kk <= C}):
            M = ms[n % 4]
            n += 1
            cand = _rerank_lists(rng, tab, M, C)
            d_cand = _dev(cand)
            os_ = Guarded(M * k, torch.float32, 9.0, 3.0)
            ok_ = Guarded(M * k, torch.long, 9, 0x5a5a5a5a)
            redo = Guarded(M, torch.int32, 0, 0x5a5a5a5a)
            if M > 2:
                redo.t[2] = 5  # the all -1 list: left alone
            _lib.check(L.lzk_mt_rerank(Qd.data_ptr(), ldq, D, d_cand.data_ptr(), C, M, k, dt.t_slot.data_ptr(),
                                       dt.t_row0.data_ptr(), dt.p_e32.data_ptr(), dt.p_bias.data_ptr(),
                                       dt.p_kind.data_ptr(), 0 if metric == "l2" else 1, os_.t.data_ptr(),
                                       ok_.t.data_ptr(), redo.t.data_ptr(), _st()), "lzk_mt_rerank")
            torch.cuda.synchronize()
            assert os_.intact() and ok_.intact() and redo.intact()
            eS, eK, eB, ghost = tab.rerank_ref(Q[:M], cand, k, metric)
            gS = os_.t.cpu().numpy().astype(np.float64).reshape(M, k)
            gK = ok_.t.cpu().numpy().reshape(M, k)
            ex, bd = tab.exact(Q[:M], metric)
            raw, rawB = _raw_ranks(tab, ex, bd, cand, k)
            _assert_ranked(gS, gK, eS, eK, eB, raw, rawB, tab, ex, bd, cand, family == "grid")
            want_redo = ghost.astype(np.int32)
            if M > 2:
                assert not ghost[2] and (eK[2] == -1).all()
                want_redo[2] = 5
            if family == "grid" or np.array_equal(gK, eK):
                assert np.array_equal(redo.t.cpu().numpy(), want_redo), (C, k)
            seen_low |= bool(ghost.any())
            seen_high |= bool((~ghost[[q for q in range(M) if q != 2]]).any()) and C > k
    assert seen_low and seen_high


def _raw_ranks(tab, ex, bd, cand, k):
    """The first k ranked fp64 scores of each list before non-nodes are
    masked, and their bounds."""
    M = cand.shape[0]
    raw = np.full((M, k), NEG_INF)
    rawB = np.zeros((M, k))
    for q in range(M):
        f = tab.flat_of_cid(cand[q][cand[q] >= 0])
        f = f[ex[q][f] != NEG_INF]
        o = f[R.order(ex[q][f], tab.key[f])[:k]]
        raw[q, : o.size], rawB[q, : o.size] = ex[q][o], bd[q][o]
    return raw, rawB


def test_mt_rerank_argument_checks_gpu():
    L = _lib.lib()
    dt, Q = _rerank_case(64, "grid")
    Qd = _dev(Q)
    cand = _dev(np.zeros((5, 64), dtype=np.int64))
    os_ = Guarded(5 * 64, torch.float32, 9.0, 3.0)
    ok_ = Guarded(5 * 64, torch.long, 9, 0x5a5a5a5a)

    def call(C=16, k=6, M=5, ldq=64):
        rc = L.lzk_mt_rerank(Qd.data_ptr(), ldq, 64, cand.data_ptr(), C, M, k, dt.t_slot.data_ptr(),
                             dt.t_row0.data_ptr(), dt.p_e32.data_ptr(), dt.p_bias.data_ptr(), dt.p_kind.data_ptr(), 0,
                             os_.t.data_ptr(), ok_.t.data_ptr(), None, _st())
        torch.cuda.synchronize()
        return rc
    for kw in (dict(k=17), dict(C=65, k=6), dict(ldq=32), dict(C=0), dict(k=0), dict(M=0)):
        assert call(**kw) == EINVAL, kw
    assert bool((os_.t == 9.0).all()) and bool((ok_.t == 9).all())
    assert call() == 0 and os_.intact() and ok_.intact()  # (a null redo word is allowed)


# ================================================================ mt_topk
@functools.lru_cache(maxsize=None)
def _e2e_grid(D):
    """About 12k grid rows in 48 tenants (unsorted slots with gaps), 300
    queries of which the first ones sit on the row planted in every larger
    tenant (a tie group of about 35 at the top: it straddles the 16th place)
    and on ghosts."""
    rng = np.random.default_rng(4000 + D)
    counts = R.e2e_counts()
    tenants = R.make_tenants(rng, counts, R.e2e_slots(rng, len(counts)), D, "grid")
    dt = DevTenants(tenants, D, sort=True)
    Q = R.grid_queries(rng, 300, D).astype(np.float32)
    Q[0] = tenants[0].X[0]
    ghosts = [(t, int(r)) for t in tenants for r in np.nonzero((t.kind != R.NODE) & np.isfinite(t.bias))[0]]
    for j, (t, r) in enumerate(ghosts[:20]):
        Q[(1 + 3 * j) % 300] = t.X[r]
    return dt, Q, dt.mt_tiles()


def _topk(dt, tiles, Q, k, metric="l2"):
    s, key, ovf = S.mt_topk(tiles, _dev(Q), k, dt.p_e32, dt.p_bias, dt.p_kind, metric)
    torch.cuda.synchronize()
    return s.cpu().numpy().astype(np.float64), key.cpu().numpy(), ovf.cpu().numpy()


def _sample_thr(tab, Q, Dp):
    """fp64 value of mt_topk's threshold on grid inputs (scores are exact)."""
    _, _, rows, sb = tab.sample_ref(Dp)
    with np.errstate(invalid="ignore"):
        ss = 2.0 * (R.to_bf16(Q.astype(np.float64)) @ rows[:, : Q.shape[1]].T) + sb[None, :]
    if ss.shape[1] < R.KC:
        return np.full(Q.shape[0], NEG_INF)
    t = np.sort(ss, axis=1)[:, -R.KC]
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(t), t - 2e-4 * (1.0 + np.abs(t)), NEG_INF)


GRID_E2E = [(64, k, nq) for k in (1, 6, 10, 16) for nq in (1, 63, 64, 300)] + [(768, 10, 300), (768, 16, 64)]


@functools.lru_cache(maxsize=None)
def _e2e_grid_ref(D, k):
    """The references of all 300 queries, computed once per (D, k) (a batch of
    nq queries is a prefix): scan scores' descending sort, the fp64 threshold,
    rerank_ref of the fp64 top-16, global_ref."""
    dt, Q, _ = _e2e_grid(D)
    tab = dt.tab
    sn, _ = tab.scan(Q, 2.0, D)
    srt = np.sort(np.where(np.isfinite(sn), sn, NEG_INF), axis=1)[:, ::-1][:, :32]
    n_in = (sn >= _sample_thr(tab, Q, D)[:, None]).sum(1)
    eS, eK, _, ghost = tab.rerank_ref(Q, tab.top_cand(Q, 2.0, D), k, "l2")
    cS, cK, _ = tab.global_ref(Q, k, "l2")
    return srt, n_in, eS, eK, ghost, cS, cK


@pytest.mark.parametrize("D,k,nq", GRID_E2E)
def test_mt_topk_grid_bits_gpu(D, k, nq):
    """mt_topk over a table built from an UNSORTED slot list: keys and score
    bits equal rerank_ref of the fp64 top-16 by (score desc, key asc) -- where
    a tie group straddles the 16th place the key-smallest rows are expected --,
    and ovf is set exactly for the queries with a non-node among their k best
    stored rows (no list overflows here, shown from the reference). Queries
    that need no redo also equal the route contract, global_ref. nq = 63 / 64:
    either side of cand_select's block / wave switch."""
    dt, Qall, tiles = _e2e_grid(D)
    tab = dt.tab
    assert tiles.slot.tolist() == tab.t_slot.tolist() and tiles.row0.tolist() == tab.t_row0.tolist()
    assert [t.slot for t in dt.tenants] != sorted(t.slot for t in dt.tenants)
    srt, n_in, eS, eK, ghost, cS, cK = (a[:nq] for a in _e2e_grid_ref(D, k))
    assert srt[0, R.KC - 1] == srt[0, R.KC]  # query 0: an exact tie across the 16th place
    assert (n_in <= 8192).all()  # no list overflows mt_topk's cap
    gS, gK, ovf = _topk(dt, tiles, Qall[:nq], k)
    assert np.array_equal(gK, eK)
    assert np.array_equal(_f32bits(gS), _f32bits(eS))
    assert np.array_equal(ovf != 0, ghost)
    if nq >= 63:
        assert ghost.any() and not ghost.all()
    assert np.array_equal(gK[~ghost], cK[~ghost]) and np.array_equal(_f32bits(gS[~ghost]), _f32bits(cS[~ghost]))


@pytest.mark.parametrize("which", ["small sample", "unstored sample", "overflow"])
def test_mt_topk_threshold_edges_gpu(which, monkeypatch):
    """A table whose sample holds fewer than 16 rows and a table whose sample
    rows are all unstored: the threshold is -inf and the result still exact.
    A -inf threshold over more than ``cap`` rows: ovf = 1 for every query."""
    rng = np.random.default_rng(len(which))
    if which == "overflow":
        dt, Q, tiles = _e2e_grid(64)
        Q = Q[:70]
        monkeypatch.setattr(S, "_mt_threshold", lambda Xs, bs, Q16, *a: torch.full(
            (Q16.shape[0],), NEG_INF, dtype=torch.float32, device=Q16.device))
        assert int(dt.tab.stored.sum()) > 8192
        _, _, ovf = _topk(dt, tiles, Q, 6)
        assert (ovf == 1).all()
        return
    counts = [1, 63, 65] if which == "small sample" else [257, 300, 700, 65, 64]
    tenants = R.make_tenants(rng, counts, R.e2e_slots(rng, len(counts)), 64, "grid",
                             unstore_samples=which == "unstored sample")
    dt = DevTenants(tenants, 64, sort=True)
    tab = dt.tab
    tiles = dt.mt_tiles()
    Q = R.grid_queries(rng, 70, 64).astype(np.float32)
    _, _, _, sb = tab.sample_ref(64)
    if which == "small sample":
        assert sb.size < R.KC
    else:
        assert sb.size >= R.KC and (sb == NEG_INF).all() and int(tab.stored.sum()) > 1000
    assert (_sample_thr(tab, Q, 64) == NEG_INF).all()
    for k in (6, 16):
        eS, eK, _, ghost = tab.rerank_ref(Q, tab.top_cand(Q, 2.0, 64), k, "l2")
        gS, gK, ovf = _topk(dt, tiles, Q, k)
        assert np.array_equal(gK, eK) and np.array_equal(_f32bits(gS), _f32bits(eS))
        assert np.array_equal(ovf != 0, ghost)


@functools.lru_cache(maxsize=None)
def _e2e_gauss(D, norm):
    tenants, Q = R.e2e_gauss(D, norm)
    dt = DevTenants(tenants, D, sort=True)
    return dt, Q, dt.mt_tiles()


@pytest.mark.parametrize("D,norm,k", [(64, 1.0, 6), (64, 1.0, 10), (768, 1.0, 6), (768, 1.0, 10),
                                      (64, 4.0, 10), (768, 4.0, 10)])
def test_mt_topk_gauss_gpu(D, norm, k):
    """Gaussian rows (no ghosts), L2. For every decidable query (all but at
    most 1 in 20; test_mt_ref_cpu.py shows it for these inputs): the keys are
    distinct stored nodes, each score is within the re-rank bound of its row's
    fp64 score, scores do not increase, and every returned row's fp64 score is
    at least the fp64 k-th best minus twice the bound."""
    dt, Q, tiles = _e2e_gauss(D, norm)
    tab = dt.tab
    dec = tab.decidable(Q, k, "l2", D)
    assert (~dec).sum() * 20 <= dec.size
    ex, bd = tab.exact(Q, "l2")
    gS, gK, ovf = _topk(dt, tiles, Q, k)
    flat = {int(key): i for i, key in enumerate(tab.key)}
    f = np.nonzero(tab.stored)[0]
    assert (ovf == 0).all()
    for q in np.nonzero(dec)[0]:
        assert (gK[q] >= 0).all() and np.unique(gK[q]).size == k, q
        rows = np.array([flat[int(x)] for x in gK[q]])
        assert tab.stored[rows].all() and (tab.kind[rows] == R.NODE).all(), q
        assert (np.abs(gS[q] - ex[q][rows]) <= bd[q][rows]).all(), q
        assert (np.diff(gS[q]) <= 0).all(), q
        kth = np.sort(ex[q][f])[-k]
        assert (ex[q][rows] >= kth - 2.0 * bd[q][f].max()).all(), q


@pytest.mark.parametrize("table,D,norm", [("e2e", 64, 1.0), ("e2e", 768, 1.0), ("e2e", 64, 4.0), ("e2e", 768, 4.0),
                                          ("margin", 64, 4.0), ("margin", 768, 4.0), ("margin", 768, 1.0)])
def test_mt_threshold_keeps_the_top16_gpu(table, D, norm):
    """The sampled threshold (_mt_threshold: the sample's 16th best by the lane
    kernel, lowered by 2e-4 (1 + |thr|)) against the MFMA candidate pass: every
    row of the fp64 top-16 of the bf16-input scores is in the candidate list.
    The margin is valid iff no such row is lost -- the two kernels accumulate in
    different orders. "margin" tables are covered almost completely by their
    sample, so the threshold is the score of the very row that has to stay;
    norm 4 puts the scores near -16.

    Observed on one MI355X: no row is lost, and none is lost with the margin
    removed either -- the lane kernel (32x32x16 MFMA) and mt_cand_kernel
    (16x16x32 MFMA) both accumulate K in ascending order and gave the same bits
    for all 5760 sample scores compared on the "margin" tables. The margin is
    valid; on this hardware it is not what keeps the rows in."""
    L = _lib.lib()
    if table == "e2e":
        dt, Q, tiles = _e2e_gauss(D, norm)
    else:
        tenants, Q = R.margin_gauss(D, norm)
        dt = DevTenants(tenants, D, sort=True)
        tiles = dt.mt_tiles()
    tab = dt.tab
    nq = Q.shape[0]
    Q16 = dt.queries16(Q)
    ns = tiles.n_sample
    Xs = torch.empty((ns, D), dtype=torch.bfloat16, device=DEV)
    bs = torch.empty((ns,), dtype=torch.float32, device=DEV)
    _lib.check(L.lzk_mt_sample(tiles.x.data_ptr(), tiles.b.data_ptr(), tiles.s_tile.data_ptr(),
                               tiles.s_row.data_ptr(), ns, D, D, Xs.data_ptr(), bs.data_ptr(), _st()), "lzk_mt_sample")
    kslot = L.lzk_flat_topk_kslot(R.KC)
    thr = S._mt_threshold(Xs, bs, Q16, R.KC, kslot, 2.0)
    torch.cuda.synchronize()
    thr = thr.cpu().numpy().astype(np.float64)
    assert np.isfinite(thr).all()
    cap = tab.N + 8
    cnt, csb, ci, ok = _run_cand(dt, Q16, nq, 2.0, thr, cap)
    assert ok
    sn, _ = tab.scan(Q, 2.0, D)
    f = np.nonzero(tab.stored)[0]
    lost = []
    for q in range(nq):
        top = f[R.order(sn[q][f], tab.key[f])[: R.KC]]
        got = set(ci[q, : int(cnt[q])].tolist())
        lost += [(q, int(tab.cid[i])) for i in top if int(tab.cid[i]) not in got]
    assert not lost, lost[:8]
