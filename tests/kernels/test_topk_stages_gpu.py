"""The oldest search kernels stage by stage, held against the fp64 reference
tests/kernels/_topk_ref.py: the lane path of ``flat_topk`` (search.hip
``flat_topk_kernel`` / ``topk_merge_kernel`` / ``topk_merge64_kernel``), the
tenant-segment search (segment.hip ``segment_topk_kernel``, tenant.hip
``tg_gather_fields_kernel``) and the k-means assign (search256.hip
``flat_top1_kernel`` / ``flat_top1_grouped_kernel`` / ``top1_decode_kernel``),
through the exported functions called the way ``_flat_topk_lane``,
``segment_topk_ptrs``, ``flat_top1``, ``assign_two_level`` and
``gather_fields`` call them.

Exact grid (integers in [-8, 8], alpha 1 or 2, integer biases with -inf
tombstones, power-of-two scales): scores, rows and empty slots are compared
with ``array_equal``, ties included. Gaussian inputs (the cases
test_topk_ref_cpu.py proves decidable): ``Decision.check`` of the reference --
every score within the derived bound of the fp64 score of the row returned,
every must row returned, every returned row in must + may, consecutive rows
ordered up to their bounds, exact rows where the query is decidable; no query
is left out. Every output sits between canary regions that are checked
afterwards, prefilled with a sentinel. Every address a kernel may dereference
lies inside a live allocation (rows are clamped by the kernels to their count;
segments are slices of one arena); no case relies on a fault. The
register-staging variants of ``flat_topk_kernel`` (``lzk_set_search_staging(0)``)
are not run: nothing in the package selects them.

The partial-list cases (``PARTIAL_CASES``; every one has duplicate rows, about
one tombstone in ten where it has a bias, and where it has labels a query
label of -1 and one no row carries):

  n1-*      N = 1: one row, every other row of the tile clamped; nq across tiles
  t127/128/129  one tile less a row / exactly / plus a row (``full_tile`` on
            and off), the same for the query tile
  c3/c7     forced chunk counts (7 normalises to fewer), lib = the library's own
  n257-*    a last chunk of one row; n1000-* eight tiles: the running list
            across tiles of one chunk (c1) and across chunks
  d128/d768 2 and 12 K-steps per tile
  k*        every slot 1, 2, 4, 8, 10, 16
  -/b/l/bl  the four bias / label template variants; a1 = alpha 1 with small
            integer biases instead of ``-|x|^2``
  ldx/ldq   a row stride above D for X, for Q, for both
  one-*     the slot's best rows all offered to ONE of the four lists of one
            chunk (three queries: lists 0, 3, 2 of chunks 0, 1, 2), every slot
  ties      copies of a query across lists (rows 3, 7), wave rows (3, 67),
            tiles (3, 131) and chunks (3, 515), slot 1, 2, 4 (the smaller row
            must win at every level) and 16
  dead      a chunk whose rows are all tombstoned; few = a chunk with fewer
            live rows than the slot

What no input can reach (so no case here tries): in ``segment_topk_kernel``'s
4-way merge the pointers sum to j < kout <= K when they are tested, so
``p[a] >= K`` is never true (the one-wave planting drains a list to K only
after the last round); in ``push`` the first compare ``v > s[K - 1]`` only
gates the insertion network, whose own strict compares decide every tie.

Observed on one MI355X: the 175 cases take 3.6 s together; the slowest,
test_partial_lists_bits_gpu[n1-q1-lib-k1] (the first case: it loads the
library), 0.27 s, then test_partial_lists_bits_gpu[n257-q257-c7-k16-b], 0.09 s.
Largest |score - fp64| / bound on the Gaussian cases: flat_topk 0.011,
segment_topk bf16 0.038, fp32 0.045, flat_top1 0.010.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from lazzaro_amd.ops import _lib  # noqa: E402
from lazzaro_amd.ops import search as S  # noqa: E402
from tests.kernels import _topk_ref as R  # noqa: E402

DEV = "cuda"
NEG_INF = float("-inf")
GUARD = 1024  # canary elements on either side of a guarded buffer
SENT_F, SENT_I = -7.25e6, -77  # what an output holds before the launch
CAN_F, CAN_I = 3.5e7, 0x5A5A5A5A  # canaries

WORST = {}  # kernel -> largest |score - fp64| / bound seen on the Gaussian cases


def _st():
    return _lib.stream_ptr(torch.device(DEV))


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(dtype) if dtype is not None else t).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _f64(t):
    return _np(t).astype(np.float64)


class Guarded:
    """``n`` elements, prefilled with a sentinel, between two canary regions of
    one allocation."""

    def __init__(self, n, dtype):
        fl = dtype.is_floating_point
        self.canary = CAN_F if fl else (CAN_I if dtype != torch.uint8 else 0x5A)
        self.sent = SENT_F if fl else (SENT_I if dtype != torch.uint8 else 0xEE)
        self.buf = torch.full((n + 2 * GUARD,), self.canary, dtype=dtype, device=DEV)
        self.t = self.buf[GUARD: GUARD + n]
        self.t.fill_(self.sent)

    def ptr(self):
        return self.t.data_ptr()

    def intact(self):
        c = torch.full((GUARD,), self.canary, dtype=self.buf.dtype, device=DEV)
        return bool(torch.equal(self.buf[:GUARD], c)) and bool(torch.equal(self.buf[-GUARD:], c))


def _strided16(a, pad):
    """bf16 device matrix of the fp64 values ``a`` with row stride D + pad (the
    padding holds 9.0: a kernel reading past D would change integer scores)."""
    n, D = a.shape
    full = torch.full((max(n, 1), D + pad), 9.0, dtype=torch.bfloat16, device=DEV)
    v = full[:n, :D]
    v.copy_(_dev(a, torch.bfloat16))
    return v


def _l2_bias(X):
    return (-(np.asarray(X, dtype=np.float64) ** 2).sum(1)).astype(np.float32)


# ================================================================ lzk_flat_topk_partial
def P(name, N, nq, D, ch, kslot, var, alpha=2.0, ldx=0, ldq=0, plant=None):
    return pytest.param(dict(N=N, nq=nq, D=D, ch=ch, kslot=kslot, var=var, alpha=alpha, ldx=ldx, ldq=ldq, plant=plant),
                        id=name)


PARTIAL_CASES = [
    P("n1-q1-lib-k1", 1, 1, 64, None, 1, ""),
    P("n1-q257-c1-k16-bl", 1, 257, 64, 1, 16, "bl"),
    P("n1-q128-c7-k4-b", 1, 128, 128, 7, 4, "b"),
    P("t127-q127-lib-k4-b", 127, 127, 64, None, 4, "b"),
    P("t128-q128-c1-k8", 128, 128, 64, 1, 8, ""),
    P("t129-q129-c3-k2-l", 129, 129, 64, 3, 2, "l"),
    P("t127-q257-c3-k10-bl", 127, 257, 64, 3, 10, "bl"),
    P("t128-q1-c7-k16-b", 128, 1, 64, 7, 16, "b"),
    P("t129-q1-lib-k1-l", 129, 1, 128, None, 1, "l"),
    P("t128-q127-lib-k2-bl-d768", 128, 127, 768, None, 2, "bl"),
    P("n257-q1-c3-k10-bl-d128", 257, 1, 128, 3, 10, "bl"),
    P("n257-q257-c7-k16-b", 257, 257, 64, 7, 16, "b"),
    P("n257-q128-lib-k8-d768", 257, 128, 768, None, 8, ""),
    P("n257-q129-c1-k4-l", 257, 129, 64, 1, 4, "l"),
    P("n1000-q1-lib-k16-b", 1000, 1, 64, None, 16, "b"),
    P("n1000-q127-c7-k10-bl-d128", 1000, 127, 128, 7, 10, "bl"),
    P("n1000-q129-c3-k4-b-d768", 1000, 129, 768, 3, 4, "b"),
    P("n1000-q257-c1-k1", 1000, 257, 64, 1, 1, ""),
    P("n1000-q128-c1-k2-l", 1000, 128, 64, 1, 2, "l"),
    P("n1000-q257-lib-k8-bl", 1000, 257, 64, None, 8, "bl"),
    P("n128-q257-lib-k1-b-a1", 128, 257, 128, None, 1, "b", alpha=1.0),
    P("n1000-q5-c3-k10-bl-a1", 1000, 5, 64, 3, 10, "bl", alpha=1.0),
    P("n257-q127-c3-k16-ldx", 257, 127, 64, 3, 16, "b", ldx=64),
    P("n257-q129-c3-k8-ldq", 257, 129, 128, 3, 8, "bl", ldq=8),
    P("n1000-q5-c7-k4-ldx-ldq-d768", 1000, 5, 768, 7, 4, "b", ldx=8, ldq=136),
    P("one-k1", 1000, 5, 64, 3, 1, "b", plant="one"),
    P("one-k2", 1000, 5, 64, 3, 2, "bl", plant="one"),
    P("one-k4", 1000, 5, 64, 3, 4, "", alpha=1.0, plant="one"),
    P("one-k8", 1000, 5, 128, 3, 8, "b", plant="one"),
    P("one-k10", 1000, 5, 64, 3, 10, "b", plant="one"),
    P("one-k16", 1000, 129, 64, 3, 16, "bl", plant="one"),
    P("ties-k1-c7", 1000, 5, 64, 7, 1, "b", plant="ties"),
    P("ties-k2-c7", 1000, 5, 64, 7, 2, "bl", plant="ties"),
    P("ties-k4-c1", 1000, 5, 64, 1, 4, "", alpha=1.0, plant="ties"),
    P("ties-k16-lib", 1000, 130, 64, None, 16, "b", plant="ties"),
    P("dead-k16-c7", 1000, 5, 64, 7, 16, "b", plant="dead"),
    P("dead-k1-c7-l", 1000, 129, 64, 7, 1, "bl", plant="dead"),
    P("few-k8-c3", 257, 5, 64, 3, 8, "b", plant="few"),
    P("few-k16-c7-l", 1000, 5, 128, 7, 16, "bl", plant="few"),
    P("few-k2-c3", 257, 129, 64, 3, 2, "b", plant="few"),
]

TIE_ROWS = (3, 7, 67, 131, 515)


def build_partial(c):
    """Inputs (numpy) and the reference partial lists of one case."""
    N, nq, D = c["N"], c["nq"], c["D"]
    rng = np.random.default_rng(N * 1000 + nq * 7 + D + c["kslot"])
    X = R.grid_rows(rng, N, D, dup=min(6, N // 4))
    Q = R.grid_queries(rng, nq, D)
    has_b, has_l = "b" in c["var"], "l" in c["var"]
    rl = rng.integers(0, 3, size=N).astype(np.int32) if has_l else None
    ql = rng.choice(np.array([-1, 0, 1, 2, 5], dtype=np.int32), size=nq) if has_l else None
    nch = R.chunking(N, c["ch"])[1] if c["ch"] else R.lib_chunks(N, nq)
    rpc = R.chunking(N, nch)[0]
    assert R.chunking(N, nch)[1] == nch
    planted = {}
    if c["plant"] == "one":
        for q, (ck, li) in enumerate(((0, 0), (1, 3), (2, 2))):
            rows = R.one_list_rows(ck * rpc, min(N, (ck + 1) * rpc), li, c["kslot"], rng)
            R.plant(X, Q[q], rows)
            planted[q] = rows
    elif c["plant"] == "ties":
        R.plant_ties(X, Q[0], TIE_ROWS)
        planted[0] = np.array(TIE_ROWS)
    tomb = rng.random(N) < 0.1
    for rows in planted.values():
        tomb[rows] = False
    if c["plant"] == "dead":
        tomb[rpc: 2 * rpc] = True
    elif c["plant"] == "few":
        tomb[rpc: min(N, 2 * rpc)] = True
        tomb[rpc + 5: rpc + 5 + min(c["kslot"] - 1, 3)] = False  # chunk 1: fewer live rows than the slot
    bias = None
    if has_b:
        bias = _l2_bias(X) if c["alpha"] == 2.0 else rng.integers(-40, 41, size=N).astype(np.float32)
        if c["alpha"] != 2.0:
            for rows in planted.values():
                bias[rows] = 0.0
        bias[tomb] = NEG_INF
    if has_l:
        for q in planted:
            ql[q] = -1
    Sc = R.flat_scores(X, Q, bias, rl, ql, c["alpha"])
    for q, rows in planted.items():
        assert R.is_top(Sc[q], np.sort(rows) if c["plant"] == "ties" else rows), "planting failed"
        if c["plant"] == "one":
            assert np.unique(R.flat_list_of(rows)).size == 1 and np.unique(rows // rpc).size == 1
    ps, pi, nch2 = R.partial_of_scores(Sc, nch, c["kslot"])
    assert nch2 == nch
    if c["plant"] == "dead" and has_b:
        assert (pi[:, 1] == -1).all()
    if c["plant"] == "few" and has_b:
        assert ((pi[:, 1] >= 0).sum(1) < c["kslot"]).all()
    return dict(X=X, Q=Q, bias=bias, rl=rl, ql=ql, nch=nch, ps=ps, pi=pi, S=Sc)


def run_partial(c, b, active=None, ps_g=None, pi_g=None):
    L = _lib.lib()
    N, nq, D, kslot, nch = c["N"], c["nq"], c["D"], c["kslot"], b["nch"]
    X16, Q16 = _strided16(b["X"], c["ldx"]), _strided16(b["Q"], c["ldq"])
    bias = _dev(b["bias"]) if b["bias"] is not None else None
    rl = _dev(b["rl"]) if b["rl"] is not None else None
    ql = _dev(b["ql"]) if b["ql"] is not None else None
    ps_g = ps_g or Guarded(nq * nch * kslot, torch.float32)
    pi_g = pi_g or Guarded(nq * nch * kslot, torch.int32)
    args = (X16.data_ptr(), X16.stride(0), N, Q16.data_ptr(), Q16.stride(0), nq, _lib.ptr(bias), _lib.ptr(rl),
            _lib.ptr(ql), float(c["alpha"]), D, kslot, nch, ps_g.ptr(), pi_g.ptr())
    if active is None:
        rc = L.lzk_flat_topk_partial(*args, _st())
    else:
        rc = L.lzk_flat_topk_partial_masked(*args, active.data_ptr(), _st())
    torch.cuda.synchronize()
    assert rc == 0
    assert ps_g.intact() and pi_g.intact()
    return ps_g, pi_g


@pytest.mark.parametrize("c", PARTIAL_CASES)
def test_partial_lists_bits_gpu(c):
    """Every (query, chunk) list of ``lzk_flat_topk_partial`` equals partial_ref:
    scores, rows and the (-inf, -1) padding."""
    L = _lib.lib()
    b = build_partial(c)
    if c["ch"] is None:
        assert L.lzk_flat_topk_chunks(c["N"], c["nq"], S.TARGET_WGS) == b["nch"]
    ps_g, pi_g = run_partial(c, b)
    shape = (c["nq"], b["nch"], c["kslot"])
    assert np.array_equal(_np(pi_g.t).reshape(shape).astype(np.int64), b["pi"])
    assert np.array_equal(_f64(ps_g.t).reshape(shape), b["ps"])


MASK_CASE = dict(N=257, nq=300, D=64, ch=3, kslot=8, var="bl", alpha=2.0, ldx=0, ldq=0, plant=None)


@pytest.mark.parametrize("mask", ["tile0-off", "tile1-part", "one-query", "none", "all"])
def test_masked_partial_and_merge_gpu(mask):
    """``lzk_flat_topk_partial_masked`` / ``lzk_topk_merge_masked``: the lists of
    a 128-query tile without an active query and the result rows of inactive
    queries keep the sentinel; active queries equal the unmasked reference."""
    L = _lib.lib()
    c = MASK_CASE
    nq, kslot, k = c["nq"], c["kslot"], 5
    b = build_partial(c)
    nch = b["nch"]
    act = np.ones(nq, dtype=np.int32)
    if mask == "tile0-off":
        act[:128] = 0
    elif mask == "tile1-part":
        act[:128] = 0
        act[128:256:3] = 0
        act[290:] = 0
    elif mask == "one-query":
        act[:] = 0
        act[299] = 1
    elif mask == "none":
        act[:] = 0
    active = _dev(act)
    ps_g, pi_g = run_partial(c, b, active=active)
    gs, gi = _f64(ps_g.t).reshape(nq, nch, kslot), _np(pi_g.t).reshape(nq, nch, kslot).astype(np.int64)
    tile_on = np.array([act[t * 128: (t + 1) * 128].any() for t in range(3)])
    on = act.astype(bool)
    off_tile = ~tile_on[np.arange(nq) // 128]
    assert np.array_equal(gs[on], b["ps"][on]) and np.array_equal(gi[on], b["pi"][on])
    assert (gs[off_tile] == SENT_F).all() and (gi[off_tile] == SENT_I).all()
    # the merge of the active queries only
    os_g, oi_g = Guarded(nq * k, torch.float32), Guarded(nq * k, torch.int64)
    off = (1 << 31) + 3
    rc = L.lzk_topk_merge_masked(ps_g.ptr(), pi_g.ptr(), nch * kslot, nq, kslot, k, off, os_g.ptr(), oi_g.ptr(),
                                 active.data_ptr(), _st())
    torch.cuda.synchronize()
    assert rc == 0 and os_g.intact() and oi_g.intact()
    ws, wi = R.merge_ref(b["ps"], b["pi"], k, off)
    ms, mi = _f64(os_g.t).reshape(nq, k), _np(oi_g.t).reshape(nq, k)
    assert np.array_equal(ms[on], ws[on]) and np.array_equal(mi[on], wi[on])
    assert (ms[~on] == SENT_F).all() and (mi[~on] == SENT_I).all()
    ds, di = R.topk_of_scores(b["S"], k, off)
    assert np.array_equal(ws, ds) and np.array_equal(wi, np.where(di >= 0, di, -1))


# ================================================================ lzk_topk_merge
def hand_lists(rng, nq, ncand, wide=False):
    """Hand-built candidate lists [nq, ncand]: few distinct integer scores
    (ties in different lanes' shares), rows unique per query and in no order,
    about a quarter of the entries empty (row -1), some live rows with a -inf
    score; query 0 all equal scores, query 1 rows descending with ascending
    scores, query 2 all empty, query 3 all -inf."""
    ps = rng.integers(-3, 4, size=(nq, ncand)).astype(np.float32)
    pi = np.stack([rng.permutation(4 * ncand)[:ncand] for _ in range(nq)]).astype(np.int64)
    if not wide:  # spread over [0, 2^31 - 1): multiplication modulo the prime 2^31 - 1 keeps the rows distinct
        pi = (pi * 8388593 + 12345) % ((1 << 31) - 1)
        pi[4, pi[4].argmax()] = (1 << 31) - 2  # the largest row below the kernels' "none" mark
    pi[1] = np.sort(pi[1])[::-1]
    ps[1] = np.arange(ncand) // 3
    assert all(np.unique(r).size == ncand for r in pi)
    pi[rng.random((nq, ncand)) < 0.25] = -1
    ps[rng.random((nq, ncand)) < 0.1] = NEG_INF
    ps[0] = 2.0
    pi[2] = -1
    ps[3] = NEG_INF
    return ps, pi


@pytest.mark.parametrize("kslot,kout", [(1, 1), (2, 2), (4, 3), (8, 5), (10, 9), (16, 16)])
@pytest.mark.parametrize("ncand", [1, 63, 64, 65, 256])
def test_merge_hand_built_gpu(ncand, kslot, kout):
    """``lzk_topk_merge`` on lists no scan produced, ``idx_offset`` 0 and above
    2^31 (never added to an empty slot)."""
    L = _lib.lib()
    nq = 9  # three blocks of four waves, the last one partial
    rng = np.random.default_rng(ncand * 100 + kslot)
    ps, pi = hand_lists(rng, nq, ncand)
    d_ps, d_pi = _dev(ps), _dev(pi.astype(np.int32))
    for off in (0, (1 << 31) + 12345):
        os_g, oi_g = Guarded(nq * kout, torch.float32), Guarded(nq * kout, torch.int64)
        rc = L.lzk_topk_merge(d_ps.data_ptr(), d_pi.data_ptr(), ncand, nq, kslot, kout, off, os_g.ptr(), oi_g.ptr(),
                              _st())
        torch.cuda.synchronize()
        assert rc == 0 and os_g.intact() and oi_g.intact()
        ws, wi = R.merge_ref(ps, pi, kout, off)
        assert np.array_equal(_np(oi_g.t).reshape(nq, kout), wi)
        assert np.array_equal(_f64(os_g.t).reshape(nq, kout), ws)
    assert L.lzk_topk_merge(d_ps.data_ptr(), d_pi.data_ptr(), ncand, nq, kslot, kslot + 1, 0, 0, 0, _st()) != 0


@pytest.mark.parametrize("nq", [1, 3, 63])
def test_two_level_merge_gpu(nq):
    """``_flat_topk_lane`` with ``_merge_groups`` > 1 (few queries, 32 chunks)
    against the one-level reference, row offset above 2^31."""
    N, D, k, kslot, nch = 4096, 64, 9, 10, 32
    assert S._merge_groups(nq, nch) > 1
    rng = np.random.default_rng(nq)
    X = R.grid_rows(rng, N, D)
    Q = R.grid_queries(rng, nq, D)
    R.plant_ties(X, Q[0], [5, 133, 2049, 4000])  # ties across the merge groups
    bias = _l2_bias(X)
    bias[rng.random(N) < 0.1] = NEG_INF
    bias[[5, 133, 2049, 4000]] = -float(Q[0] @ Q[0])
    off = (1 << 31) + 1
    gs, gi = S._flat_topk_lane(_dev(X, torch.bfloat16), _dev(Q, torch.bfloat16), k, kslot, _dev(bias), None, None,
                               2.0, off, nch)
    ws, wi = R.topk_of_scores(R.flat_scores(X, Q, bias, None, None, 2.0), k, off)
    assert np.array_equal(_np(gi), wi) and np.array_equal(_f64(gs), ws)
    assert wi[0, :4].tolist() == [5 + off, 133 + off, 2049 + off, 4000 + off]


# ================================================================ lzk_topk_merge64
@pytest.mark.parametrize("kout", [1, 4, 5, 10, 11, 16, 17, 32])
@pytest.mark.parametrize("ncand", [0, 1, 63, 65])
def test_merge64_hand_built_gpu(ncand, kout):
    """``lzk_topk_merge64``: ids above 2^40, ties broken by id, every template's
    lower edge (kout 1, 5, 11, 17) and upper edge, an empty candidate axis."""
    L = _lib.lib()
    nq = 9
    rng = np.random.default_rng(ncand * 100 + kout)
    ps, pi = hand_lists(rng, nq, max(ncand, 1), wide=True)
    ps, pi = ps[:, :ncand], pi[:, :ncand]
    pi = np.where(pi >= 0, (pi << 21) + (1 << 40) + 1, -1)
    ps = np.where((pi >= 0) | (ps == NEG_INF), ps, NEG_INF).astype(np.float32)
    d_ps, d_pi = _dev(ps.reshape(-1)), _dev(pi.reshape(-1))
    keep = torch.zeros(8, dtype=torch.int64, device=DEV)  # a live address for the empty case
    os_g, oi_g = Guarded(nq * kout, torch.float32), Guarded(nq * kout, torch.int64)
    rc = L.lzk_topk_merge64(d_ps.data_ptr() if ncand else keep.data_ptr(), d_pi.data_ptr() if ncand else keep.data_ptr(),
                            ncand, nq, kout, os_g.ptr(), oi_g.ptr(), _st())
    torch.cuda.synchronize()
    assert rc == 0 and os_g.intact() and oi_g.intact()
    ws, wi = R.merge64_ref(ps, pi, kout)
    assert np.array_equal(_np(oi_g.t).reshape(nq, kout), wi)
    assert np.array_equal(_f64(os_g.t).reshape(nq, kout), ws)
    if ncand:
        assert wi[wi >= 0].min() > (1 << 40)


# ================================================================ lzk_segment_topk
SEG_SIZES = (0, 1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1000)
SEG_KS = (1, 2, 3, 4, 5, 8, 10, 16)
# (bias, scale, query bias, alpha): the serving form first
SEG_FORMS = ((True, False, True, 2.0), (True, True, True, 2.0), (False, False, False, 1.0), (False, True, True, 1.0))
PLANT_N = 32 * 16 + 5


def build_segments(D, seed):
    """The segments of one launch, as slices of one arena: SEG_SIZES, then the
    planted ones -- "lane": the 16 best rows all in lane 13's residue class;
    "wave": all in wave 2; "ties": copies of the query across lanes (3, 7),
    waves (3, 12, 40) and 32-row rounds (3, 67); "few": two live rows; "dead":
    none. Returns per segment (rows, query, bias, scale, planted rows or None)."""
    rng = np.random.default_rng(seed)
    segs = []
    for n in SEG_SIZES:
        x = R.grid_rows(rng, n, D, dup=min(6, n // 4))
        b = _l2_bias(x)
        if n > 3:
            b[rng.random(n) < 0.1] = NEG_INF
        segs.append([x, R.grid_queries(rng, 1, D)[0], b, None])
    for kind in ("lane", "wave", "ties", "few", "dead"):
        n = {"lane": PLANT_N, "wave": PLANT_N, "ties": 100, "few": 33, "dead": 9}[kind]
        x = R.grid_rows(rng, n, D)
        q = R.grid_queries(rng, 1, D)[0]
        rows = None
        if kind == "lane":
            rows = R.one_lane_rows(n, 13, 16, rng)
            R.plant(x, q, rows)
        elif kind == "wave":
            rows = R.one_wave_rows(n, 2, 16, rng)
            R.plant(x, q, rows)
        elif kind == "ties":
            rows = np.array([3, 7, 12, 40, 67])
            R.plant_ties(x, q, rows)
        b = _l2_bias(x)
        if kind == "few":
            b[:] = NEG_INF
            b[[4, 20]] = -3.0
        elif kind == "dead":
            b[:] = NEG_INF
        else:
            t = rng.random(n) < 0.1
            t[rows] = False
            b[t] = NEG_INF
        segs.append([x, q, b, rows])
    out = []
    for x, q, b, rows in segs:
        sc = (2.0 ** rng.integers(-2, 1, size=len(x))).astype(np.float32)
        if rows is not None:
            sc[rows] = 1.0
        out.append((x, q, b, sc, rows))
    return out


def seg_reference(segs, form, dtype):
    """Full fp64 score vector of every segment under ``form`` and a check that
    the plantings hold in it."""
    use_b, use_s, use_q, alpha = form
    vec = []
    for x, q, b, sc, rows in segs:
        s, _ = R.segment_scores(x, q, b if use_b else None, sc if use_s else None, alpha,
                                -float(q @ q) if use_q else 0.0, dtype)
        if rows is not None:  # (5 rows: the tie planting, returned by row; 16: the planted order)
            assert R.is_top(s, np.sort(rows) if len(rows) == 5 else rows), "planting failed"
        vec.append(s)
    return vec


@pytest.mark.parametrize("dtype,D", [("bf16", 64), ("bf16", 128), ("bf16", 768), ("bf16", 2048),
                                     ("fp32", 32), ("fp32", 96), ("fp32", 384), ("fp32", 2048)])
def test_segment_topk_bits_gpu(dtype, D):
    """``lzk_segment_topk`` over every size, k and form in one arena with
    ``ld > D``: scores, rows and empty slots bit for bit."""
    L = _lib.lib()
    tdt = torch.bfloat16 if dtype == "bf16" else torch.float32
    esz = 2 if dtype == "bf16" else 4
    segs = build_segments(D, 7 * D + esz)
    nq = len(segs)
    ld = D + (8 if dtype == "bf16" else 4)
    n_all = sum(len(s[0]) for s in segs)
    arena = torch.full((n_all + 1, ld), 9.0, dtype=tdt, device=DEV)
    a_b = torch.zeros(n_all + 1, dtype=torch.float32, device=DEV)
    a_s = torch.ones(n_all + 1, dtype=torch.float32, device=DEV)
    offs, o = [], 0
    for x, q, b, sc, _ in segs:
        n = len(x)
        if n:
            arena[o: o + n, :D] = _dev(x, tdt)
            a_b[o: o + n] = _dev(b)
            a_s[o: o + n] = _dev(sc)
        offs.append(o)
        o += n
    Q = _strided16(np.stack([s[1] for s in segs]), 8) if dtype == "bf16" else None
    if Q is None:
        qfull = torch.full((nq, D + 4), 9.0, dtype=torch.float32, device=DEV)
        Q = qfull[:, :D]
        Q.copy_(_dev(np.stack([s[1] for s in segs]), torch.float32))
    offs_a = np.array(offs, dtype=np.int64)
    xptr = _dev(arena.data_ptr() + offs_a * ld * esz)
    bptr = _dev(a_b.data_ptr() + offs_a * 4)
    sptr = _dev(a_s.data_ptr() + offs_a * 4)
    nrows = _dev(np.array([len(s[0]) for s in segs], dtype=np.int32))
    qb = _dev(np.array([-float(s[1] @ s[1]) for s in segs], dtype=np.float32))
    for form in SEG_FORMS:
        use_b, use_s, use_q, alpha = form
        vec = seg_reference(segs, form, dtype)
        for k in SEG_KS:
            kslot = L.lzk_flat_topk_kslot(k)
            assert kslot == R.kslot_of(k)
            os_g, oi_g = Guarded(nq * k, torch.float32), Guarded(nq * k, torch.int64)
            rc = L.lzk_segment_topk(xptr.data_ptr(), nrows.data_ptr(), ld, bptr.data_ptr() if use_b else 0,
                                    sptr.data_ptr() if use_s else 0, Q.data_ptr(), Q.stride(0), nq, D,
                                    0 if dtype == "bf16" else 1, alpha, qb.data_ptr() if use_q else 0, kslot, k,
                                    os_g.ptr(), oi_g.ptr(), _st())
            torch.cuda.synchronize()
            assert rc == 0 and os_g.intact() and oi_g.intact()
            gs, gi = _f64(os_g.t).reshape(nq, k), _np(oi_g.t).reshape(nq, k)
            for q in range(nq):
                ws, wi = R.topk_of_scores(vec[q][None, :], k)
                assert np.array_equal(gi[q], wi[0]), (form, k, q, len(segs[q][0]))
                assert np.array_equal(gs[q], ws[0]), (form, k, q, len(segs[q][0]))


# ================================================================ lzk_tg_gather_fields
@pytest.mark.parametrize("nq,k", [(1, 1), (1, 16), (5, 10), (300, 1), (300, 10), (300, 16)])
def test_gather_fields_gpu(nq, k):
    """``lzk_tg_gather_fields`` through per-query pointers into separately
    allocated columns of different lengths, rows of -1 mixed in; values and
    dtypes of all five outputs, also through ``tenant_ops.gather_fields``."""
    from lazzaro_amd.ops.tenant_ops import gather_fields
    L = _lib.lib()
    rng = np.random.default_rng(nq * 100 + k)
    lens = (1, 3, 40, 257, 1000, 17, 64)
    ten = []
    for n in lens:
        cols = (rng.random(n).astype(np.float32), rng.integers(0, 1 << 30, n).astype(np.int32),
                rng.integers(0, 256, n).astype(np.uint8), rng.integers(0, 256, n).astype(np.uint8),
                rng.integers(-1, 1 << 20, n).astype(np.int32))
        ten.append((cols, tuple(_dev(c) for c in cols)))
    tq = rng.integers(0, len(lens), size=nq)
    rows = np.stack([np.where(rng.random(k) < 0.25, -1, rng.integers(0, lens[t], size=k)) for t in tq]).astype(np.int64)
    rows[0, 0] = lens[tq[0]] - 1  # the last row of a column
    base = _dev(np.array([[ten[t][1][c].data_ptr() for t in tq] for c in range(5)], dtype=np.int64))
    d_rows = _dev(rows)
    outs = [Guarded(nq * k, dt) for dt in (torch.float32, torch.int32, torch.uint8, torch.uint8, torch.int32)]
    rc = L.lzk_tg_gather_fields(d_rows.data_ptr(), nq, k, base.data_ptr(), *[g.ptr() for g in outs], _st())
    torch.cuda.synchronize()
    assert rc == 0 and all(g.intact() for g in outs)
    want = R.gather_fields_ref(rows, [ten[t][0] for t in tq])
    got = gather_fields(d_rows, None, base=base)
    for g, name in zip(outs, ("sal", "acc", "kind", "sup", "shard")):
        assert np.array_equal(_np(g.t).reshape(nq, k), want[name]), name
        assert got[name].dtype == want[name].dtype and np.array_equal(got[name], want[name]), name


# ================================================================ lzk_flat_top1 / lzk_flat_top1_grouped
def run_top1(X, Q):
    L = _lib.lib()
    N, D = X.shape
    nq = Q.shape[0]
    X16, Q16 = _strided16(X, 0), _strided16(Q, 0)
    ws, sc, row = Guarded(nq, torch.int64), Guarded(nq, torch.float32), Guarded(nq, torch.int32)
    rc = L.lzk_flat_top1(X16.data_ptr(), X16.stride(0), N, Q16.data_ptr(), Q16.stride(0), nq, D, ws.ptr(), sc.ptr(),
                         row.ptr(), _st())
    torch.cuda.synchronize()
    assert rc == 0 and ws.intact() and sc.intact() and row.intact()
    return _np(sc.t), _np(row.t).astype(np.int64)


def top1_inputs(N, nq, D):
    """(generic, negative, zero-best) inputs. generic: grid rows with copies of
    query 0 placed 128 apart (the two wave rows of a block) and of query 1
    placed 256 apart (two blocks meeting in the atomicMax), where N allows.
    negative: non-negative rows against non-positive queries, every score <= 0
    and the best ones distinct negatives. zero-best: the same with three
    all-zero rows: the best score is exactly 0, tied."""
    rng = np.random.default_rng(N * 1000 + nq + D)
    X = R.grid_rows(rng, N, D, dup=min(6, N // 4))
    Q = R.grid_queries(rng, nq, D)
    dups = []
    if N > 133:
        R.plant_ties(X, Q[0], [5, 133])
        dups.append((0, 5))
    if N > 263 and nq > 1:
        R.plant_ties(X, Q[1], [263, 7])
        dups.append((1, 7))
    Xn = np.abs(R.grid_rows(rng, N, D, dup=min(6, N // 4)))
    Xn[Xn.sum(1) == 0] = 1.0
    Qn = -np.abs(R.grid_queries(rng, nq, D))
    Qn[Qn.sum(1) == 0] = -1.0
    Xz = Xn.copy()
    zero = sorted({N // 3, N // 2, N - 1})
    Xz[zero] = 0.0
    return (X, Q, dups), (Xn, Qn), (Xz, Qn, zero)


@pytest.mark.parametrize("nq", [1, 255, 256, 257, 600])
@pytest.mark.parametrize("N", [1, 37, 255, 256, 257, 513])
def test_top1_bits_gpu(N, nq):
    """``lzk_flat_top1`` = top1_ref bit for bit: ties to the smaller row within
    a lane, across lane groups, wave rows and blocks; all-negative scores (the
    packed key's order for negative floats decides); a best score of exactly 0."""
    D = 64 if (N + nq) % 2 else 192
    (X, Q, dups), (Xn, Qn), (Xz, Qz, zero) = top1_inputs(N, nq, D)
    gs, gr = run_top1(X, Q)
    ws, wr = R.top1_ref(X, Q)
    assert np.array_equal(gr, wr) and np.array_equal(gs.astype(np.float64), ws)
    for q, r in dups:
        assert wr[q] == r and ws[q] == float(Q[q] @ Q[q])
    gs, gr = run_top1(Xn, Qn)
    ws, wr = R.top1_ref(Xn, Qn)
    assert (ws < 0).all() and (N < 37 or nq < 255 or np.unique(ws).size > 8)
    assert np.array_equal(gr, wr) and np.array_equal(gs.astype(np.float64), ws)
    gs, gr = run_top1(Xz, Qz)
    ws, wr = R.top1_ref(Xz, Qz)
    assert (ws == 0).all() and (wr == zero[0]).all()
    assert np.array_equal(gr, wr) and np.array_equal(gs.astype(np.float64), ws)
    assert np.unique(gs.view(np.int32)).size == 1  # one bit pattern for the tied zero, whichever block won


@pytest.mark.parametrize("D", [64, 192])
@pytest.mark.parametrize("v", [0, 1, 2])
def test_top1_grouped_bits_gpu(v, D):
    """``lzk_flat_top1_grouped``: groups of 1, 255 and 257 positions against
    centroid ranges of 1, 37 and 300 rows (rotated by v), rows read by index;
    generic and all-negative scores; a position no group covers stays (-inf, -1)."""
    L = _lib.lib()
    rng = np.random.default_rng(10 * v + D)
    sizes, ranges = (1, 255, 257), (1, 37, 300)
    groups, c0, p0 = [], 0, 0
    for g in range(3):
        nc = ranges[(g + v) % 3]
        groups.append((c0, nc, p0, sizes[g]))
        c0, p0 = c0 + nc, p0 + sizes[g]
    npos = p0 + 3  # three positions outside every group
    n_data = 700
    for neg in (False, True):
        C = R.grid_rows(rng, c0, D, dup=6)
        X = R.grid_queries(rng, n_data, D)
        if neg:
            C, X = np.abs(C), -np.abs(X)
            C[C.sum(1) == 0] = 1.0
        else:
            C[[40, 300]] = C[38]  # (v = 0: rows 38, 40 and 300 of the 300-row range: a tie across its two tiles)
        qidx = rng.integers(0, n_data, size=npos).astype(np.int32)
        blk = R.grouped_blocks(groups)
        assert int((blk[:, 0] + np.minimum(blk[:, 1], 256)).max()) <= c0
        assert int((blk[:, 2] + np.minimum(blk[:, 3], 256)).max()) <= npos
        C16, X16 = _strided16(C, 8), _strided16(X, 0)
        d_q, d_b = _dev(qidx), _dev(blk)
        ws_g, sc, row = Guarded(npos, torch.int64), Guarded(npos, torch.float32), Guarded(npos, torch.int32)
        rc = L.lzk_flat_top1_grouped(C16.data_ptr(), C16.stride(0), X16.data_ptr(), X16.stride(0), d_q.data_ptr(), npos,
                                     d_b.data_ptr(), int(blk.shape[0]), D, ws_g.ptr(), sc.ptr(), row.ptr(), _st())
        torch.cuda.synchronize()
        assert rc == 0 and ws_g.intact() and sc.intact() and row.intact()
        ws, wr = R.top1_grouped_ref(C, X, qidx, groups)
        assert np.array_equal(_np(row.t).astype(np.int64), wr)
        assert np.array_equal(_f64(sc.t), ws)
        assert (wr[-3:] == -1).all() and (not neg or (ws[:-3] < 0).all())


# ================================================================ Gaussian inputs
GAUSS_CASES = [pytest.param(c, id=f"n{c[0]}-d{c[1]}-k{c[3]}") for c in R.GAUSS_SET_CASES + R.GAUSS_SCORE_CASES]


def _hold(kernel, dec, gs, gi, name):
    bad, worst = dec.check(_f64(gs), _np(gi).astype(np.int64))
    WORST[kernel] = max(WORST.get(kernel, 0.0), worst)
    print(f"[gauss] {kernel} {name}: worst |score - fp64| / bound = {worst:.4f} "
          f"(so far {WORST[kernel]:.4f}); must share {dec.must_share():.4f}, "
          f"decidable {int(dec.decidable.sum())}/{dec.decidable.size}")
    assert not bad, bad[:5]
    assert worst <= 1.0


@functools.lru_cache(maxsize=None)
def _gauss(kernel, case):
    n, D, nq, k, seed = case
    k = 1 if kernel == "top1" else k
    inp, Sc, B = R.gauss_scores(kernel, n, D, nq, seed)
    return inp, R.Decision(Sc, B, k), k


@pytest.mark.parametrize("ch", [None, 3])
@pytest.mark.parametrize("case", GAUSS_CASES)
def test_flat_gauss_gpu(case, ch):
    """The lane path end to end (partial lists + merge), ``2 <q, x> - |x|^2``."""
    (X, Q, bias, _), dec, k = _gauss("flat", case)
    gs, gi = S._flat_topk_lane(_dev(X, torch.bfloat16), _dev(Q, torch.bfloat16), k, R.kslot_of(k), _dev(bias), None,
                               None, 2.0, 0, ch)
    _hold("flat_topk", dec, gs, gi, f"n={case[0]} D={case[1]} chunks={ch}")


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("case", GAUSS_CASES)
def test_segment_gauss_gpu(case, dtype):
    """The serving form ``2 <q, x> - |x|^2 - |q|^2`` of every query over the
    whole matrix, through ``segment_topk_ptrs``."""
    (X, Q, bias, qbias), dec, k = _gauss("seg_" + dtype, case)
    tdt = torch.bfloat16 if dtype == "bf16" else torch.float32
    nq = Q.shape[0]
    dX, dB, dQ = _dev(X, tdt), _dev(bias), _dev(Q, tdt)
    xptr = torch.full((nq,), dX.data_ptr(), dtype=torch.int64, device=DEV)
    bptr = torch.full((nq,), dB.data_ptr(), dtype=torch.int64, device=DEV)
    nrows = torch.full((nq,), X.shape[0], dtype=torch.int32, device=DEV)
    gs, gi = S.segment_topk_ptrs(xptr, nrows, dX.stride(0), dQ, k, bptr=bptr, alpha=2.0, qbias=_dev(qbias))
    _hold("segment_topk_" + dtype, dec, gs, gi, f"n={case[0]} D={case[1]}")


@pytest.mark.parametrize("case", GAUSS_CASES)
def test_top1_gauss_gpu(case):
    (X, Q, _, _), dec, k = _gauss("top1", case)
    gs, gi = S.flat_top1(_dev(X, torch.bfloat16), _dev(Q, torch.bfloat16))
    _hold("flat_top1", dec, gs[:, None], gi[:, None], f"n={case[0]} D={case[1]}")
