"""tests/kernels/_topk_ref.py on its own (CPU tier): every reference against a
naive double loop at tiny sizes, the row-to-list maps against an enumeration of
the kernels' index expressions, the planting helpers (planted rows are the top
K and sit in one list / lane / wave), the CPU tier of the package
(``ops.search._ref_topk``, the CPU branches of ``segment_topk``, ``flat_top1``,
``merge_topk`` and ``gather_fields``) bit for bit against the reference on the
exact grid, and the decidability of the Gaussian cases that
tests/kernels/test_topk_stages_gpu.py runs: by the reference alone, the must
sets fill at least 90 % of the nq * k slots of every committed case.
"""
import numpy as np
import pytest
import torch

from tests.kernels import _topk_ref as R

NEG_INF = float("-inf")


# ---------------------------------------------------------------- naive helpers
def _naive_best(items, k):
    """k times the best of [(score, row)] by (score desc, row asc): a double
    loop, no sort."""
    items = [(s, r) for s, r in items if s != NEG_INF and r >= 0]
    out = []
    for _ in range(k):
        best = None
        for it in items:
            if it in out:
                continue
            if best is None or it[0] > best[0] or (it[0] == best[0] and it[1] < best[1]):
                best = it
        if best is None:
            break
        out.append(best)
    return out + [(NEG_INF, -1)] * (k - len(out))


def _naive_scores(X, Q, bias, rl, ql, alpha):
    out = [[0.0] * len(X) for _ in Q]
    for q in range(len(Q)):
        for r in range(len(X)):
            s = alpha * sum(float(a) * float(b) for a, b in zip(Q[q], X[r]))
            if bias is not None:
                s = NEG_INF if bias[r] == NEG_INF else s + float(bias[r])
            if rl is not None and ql[q] >= 0 and rl[r] != ql[q]:
                s = NEG_INF
            out[q][r] = s
    return out


def _grid(seed, n, D, nq, tomb=True):
    rng = np.random.default_rng(seed)
    X = R.grid_rows(rng, n, D, dup=min(6, n // 4))
    Q = R.grid_queries(rng, nq, D)
    bias = -(X * X).sum(1)
    if tomb and n > 3:
        bias[rng.random(n) < 0.1] = NEG_INF
    return rng, X, Q, bias.astype(np.float32)


# ---------------------------------------------------------------- references vs naive loops
def test_flat_scores_naive():
    rng, X, Q, bias = _grid(1, 23, 8, 5)
    rl = rng.integers(0, 3, size=23).astype(np.int32)
    ql = np.array([0, -1, 2, 7, 1], dtype=np.int32)  # -1: all rows; 7: a label no row carries
    for b, l in ((None, False), (bias, False), (None, True), (bias, True)):
        S = R.flat_scores(X, Q, b, rl if l else None, ql if l else None, 2.0)
        ref = np.array(_naive_scores(X, Q, b, rl if l else None, ql, 2.0))
        assert np.array_equal(S, ref)
    assert (R.flat_scores(X, Q, bias, rl, ql, 2.0)[3] == NEG_INF).all()


def test_chunking_matches_the_launcher():
    """rows_per_chunk rounded up to 128, the count recomputed (launch_flat)."""
    assert R.chunking(1000, 7) == (256, 4)
    assert R.chunking(1000, 3) == (384, 3)
    assert R.chunking(1000, 1) == (1024, 1)
    assert R.chunking(1, 7) == (128, 1)
    assert R.chunking(257, 3) == (128, 3)
    assert R.chunking(129, 7) == (128, 2)
    # lzk_flat_topk_chunks(N, nq, 512): min(ceil(512 / qblocks), tiles), normalised
    assert R.lib_chunks(1000, 1) == 8 and R.lib_chunks(129, 257) == 2 and R.lib_chunks(1, 1) == 1
    assert R.lib_chunks(100000, 129) == R.chunking(100000, 256)[1]
    assert [R.kslot_of(k) for k in (1, 2, 3, 4, 5, 8, 9, 10, 11, 16, 17)] == [1, 2, 4, 4, 8, 8, 10, 10, 16, 16, -1]


@pytest.mark.parametrize("n_chunks,kslot", [(1, 4), (2, 1), (3, 16), (7, 2)])
def test_partial_ref_naive(n_chunks, kslot):
    _, X, Q, bias = _grid(2, 300, 8, 4)
    bias[128:256] = NEG_INF  # a chunk (of the 128-row chunkings) with no live row
    ps, pi, nch = R.partial_ref(X, Q, bias, None, None, 2.0, n_chunks, kslot)
    sc = _naive_scores(X, Q, bias, None, None, 2.0)
    per = -(-300 // n_chunks)
    rpc = -(-per // 128) * 128
    assert nch == -(-300 // rpc) and ps.shape == (4, nch, kslot)
    for q in range(4):
        for c in range(nch):
            want = _naive_best([(sc[q][r], r) for r in range(c * rpc, min(300, (c + 1) * rpc))], kslot)
            assert [(float(a), int(b)) for a, b in zip(ps[q, c], pi[q, c])] == want


def test_merge_refs_naive():
    rng = np.random.default_rng(3)
    nq, nc = 6, 37
    ps = rng.integers(-4, 5, size=(nq, nc)).astype(np.float64)  # many ties
    pi = np.stack([rng.permutation(1000)[:nc] for _ in range(nq)]).astype(np.int64)
    pi[rng.random((nq, nc)) < 0.3] = -1
    ps[rng.random((nq, nc)) < 0.2] = NEG_INF
    ps[5], pi[5] = NEG_INF, -1  # an all-empty query
    off = (1 << 33) + 5
    for kout in (1, 3, 9, 16):
        os_, oi = R.merge_ref(ps, pi, kout, off)
        o64s, o64i = R.merge64_ref(ps, pi + np.where(pi >= 0, 1 << 40, 0), kout)
        for q in range(nq):
            want = _naive_best(list(zip(ps[q].tolist(), pi[q].tolist())), kout)
            assert os_[q].tolist() == [w[0] for w in want]
            assert oi[q].tolist() == [w[1] + off if w[1] >= 0 else -1 for w in want]
            # the 64-bit form keeps a live id whose score is -inf (after every finite score, ids ascending)
            live = [(s, i + (1 << 40)) for s, i in zip(ps[q].tolist(), pi[q].tolist()) if i >= 0]
            fin = _naive_best(live, kout)
            dead = sorted(i for s, i in live if s == NEG_INF)
            want64 = [w for w in fin if w[1] >= 0] + [(NEG_INF, i) for i in dead]
            want64 = (want64 + [(NEG_INF, -1)] * kout)[:kout]
            assert o64s[q].tolist() == [w[0] for w in want64] and o64i[q].tolist() == [w[1] for w in want64]


@pytest.mark.parametrize("n_chunks", [1, 2, 5])
def test_partial_then_merge_is_the_direct_topk(n_chunks):
    """The two-stage form loses nothing: merging the per-chunk lists gives the
    top-k of the whole matrix for every kout <= kslot."""
    _, X, Q, bias = _grid(4, 700, 8, 9)
    S = R.flat_scores(X, Q, bias, None, None, 1.0)
    for kslot, kout in ((4, 3), (8, 5), (10, 9), (16, 16), (1, 1)):
        ps, pi, _ = R.partial_of_scores(S, n_chunks, kslot)
        ms, mi = R.merge_ref(ps, pi, kout, 7)
        ds, di = R.topk_of_scores(S, kout, 7)
        assert np.array_equal(ms, ds) and np.array_equal(mi, di)


def test_segment_ref_naive():
    rng = np.random.default_rng(5)
    D, k = 8, 5
    sizes = [0, 1, 3, 9, 40]
    xs = [R.grid_rows(rng, n, D, dup=min(4, n // 4)) for n in sizes]
    Q = R.grid_queries(rng, len(sizes), D)
    bs = [rng.integers(-9, 10, size=n).astype(np.float64) for n in sizes]
    bs[4][::3] = NEG_INF
    sc = [2.0 ** rng.integers(-2, 1, size=n) for n in sizes]
    qb = rng.integers(-50, 50, size=len(sizes)).astype(np.float64)
    os_, oi = R.segment_ref(xs, Q, k, bs, sc, 2.0, qb)
    for q, n in enumerate(sizes):
        items = []
        for r in range(n):
            dot = sum(float(a) * float(b) for a, b in zip(Q[q], xs[q][r]))
            s = NEG_INF if bs[q][r] == NEG_INF else 2.0 * dot * sc[q][r] + bs[q][r] + qb[q]
            items.append((s, r))
        want = _naive_best(items, k)
        assert os_[q].tolist() == [w[0] for w in want] and oi[q].tolist() == [w[1] for w in want]
    # without bias, scale and query bias
    os2, oi2 = R.segment_ref(xs, Q, 2, None, None, 1.0, None)
    assert oi2[0].tolist() == [-1, -1] and oi2[1].tolist() == [0, -1]
    assert os2[1, 0] == float(Q[1] @ xs[1][0])


def test_top1_refs_naive():
    rng = np.random.default_rng(6)
    X = R.grid_rows(rng, 31, 8, dup=6)
    Q = R.grid_queries(rng, 7, 8)
    s, r = R.top1_ref(X, Q)
    sc = _naive_scores(X, Q, None, None, None, 1.0)
    for q in range(7):
        assert (float(s[q]), int(r[q])) == _naive_best([(sc[q][j], j) for j in range(31)], 1)[0]
    s0, r0 = R.top1_ref(X[:0], Q)
    assert (s0 == NEG_INF).all() and (r0 == -1).all()
    # grouped: positions 0..3 -> centroids 2..6, positions 4..6 -> centroids 10..10
    qidx = np.array([6, 0, 3, 3, 1, 5, 2, 4], dtype=np.int32)
    groups = [(2, 5, 0, 4), (10, 1, 4, 3)]
    gs, gr = R.top1_grouped_ref(X, Q, qidx, groups)
    for c0, nc, p0, np_ in groups:
        for p in range(p0, p0 + np_):
            want = _naive_best([(sc[qidx[p]][j], j) for j in range(c0, c0 + nc)], 1)[0]
            assert (float(gs[p]), int(gr[p])) == want
    assert gs[7] == NEG_INF and gr[7] == -1  # a position no group covers


def test_grouped_blocks_cover_every_pair_once():
    groups = [(0, 1, 0, 1), (1, 37, 1, 255), (38, 300, 256, 257)]
    blk = R.grouped_blocks(groups)
    assert blk.dtype == np.int32 and blk.shape == (1 + 1 + 2 * 2, 4)
    seen = {}
    for c0, nc, p0, np_ in blk.tolist():
        assert nc >= 1 and np_ >= 1
        for c in range(c0, c0 + min(nc, 256)):
            for p in range(p0, p0 + min(np_, 256)):
                seen[(c, p)] = seen.get((c, p), 0) + 1
    want = {(c, p) for c0, nc, p0, np_ in groups for c in range(c0, c0 + nc) for p in range(p0, p0 + np_)}
    assert set(seen) == want and set(seen.values()) == {1}


def test_gather_fields_ref():
    rng = np.random.default_rng(7)
    cols = []
    for n in (3, 9, 1):
        cols.append((rng.random(n).astype(np.float32), rng.integers(0, 99, n).astype(np.int32),
                     rng.integers(0, 3, n).astype(np.uint8), rng.integers(0, 2, n).astype(np.uint8),
                     rng.integers(-1, 8, n).astype(np.int32)))
    rows = np.array([[2, -1, 0], [8, 8, -1], [-1, 0, -1]], dtype=np.int64)
    out = R.gather_fields_ref(rows, cols)
    assert [out[n].dtype for n in ("sal", "acc", "kind", "sup", "shard")] == \
        [np.float32, np.int32, np.uint8, np.uint8, np.int32]
    for q in range(3):
        for j in range(3):
            r = rows[q, j]
            got = tuple(out[n][q, j] for n in ("sal", "acc", "kind", "sup", "shard"))
            assert got == ((0, 0, 0, 0, -1) if r < 0 else tuple(c[r] for c in cols[q]))


# ---------------------------------------------------------------- the row-to-list maps
def test_maps_match_the_kernels_index_expressions():
    # flat_topk_kernel: push(score(rb, cb, e), tile0 + rb * 32 + (e & 3) + 8 * (e >> 2)),
    # tile0 = row_lo + rt * 128 + wrow * 64 + 4 * h, list li = wrow * 2 + h
    seen = set()
    for rt in range(3):
        for wrow in range(2):
            for h in range(2):
                last = -1
                for rb in range(2):
                    for e in range(16):
                        row = 256 + rt * 128 + wrow * 64 + 4 * h + rb * 32 + (e & 3) + 8 * (e >> 2)
                        assert R.flat_list_of(row) == wrow * 2 + h
                        assert row > last  # offered in ascending order: the strict compare keeps the smaller row
                        last = row
                        seen.add(row)
    assert seen == set(range(256, 256 + 384))
    assert sorted(R.flat_rows_in_list(128, 256, 3).tolist()) == \
        [r for r in range(128, 256) if r % 128 >= 64 and (r >> 2) & 1]
    # segment_topk_kernel: for (r = wave * 8 + sub; r < n; r += 32), list in lane sub * 8 of the wave
    seen = set()
    for wave in range(4):
        for sub in range(8):
            for r in range(wave * 8 + sub, 200, 32):
                assert R.seg_lane_of(r) == wave * 8 + sub and R.seg_wave_of(r) == wave
                seen.add(r)
    assert seen == set(range(200))
    # flat_top1_kernel: row = r0 + wr * 128 + i * 16 + 4 * (lane >> 4) + e
    seen = set()
    for blk in range(2):
        for wr in range(2):
            for g in range(4):
                for i in range(8):
                    for e in range(4):
                        row = blk * 256 + wr * 128 + i * 16 + 4 * g + e
                        assert tuple(int(v) for v in R.top1_slot_of(row)) == (blk, wr, g)
                        seen.add(row)
    assert seen == set(range(512))


# ---------------------------------------------------------------- planting
def _l2_bias(X):
    return -(X * X).sum(1)


@pytest.mark.parametrize("form", ["ip", "l2"])
def test_near_copies_fall_strictly(form):
    rng = np.random.default_rng(8)
    q = R.grid_queries(rng, 1, 64)[0]
    P = R.near_copies(q, 16)
    assert (np.abs(P) <= 8).all() and np.array_equal(P[0], q)
    s = P @ q if form == "ip" else 2.0 * (P @ q) + _l2_bias(P)
    assert (np.diff(s) < 0).all()


@pytest.mark.parametrize("kslot", [1, 2, 4, 8, 10, 16])
@pytest.mark.parametrize("form", ["ip", "l2"])
def test_one_list_planting(kslot, form):
    """The kslot best rows of a query all reach ONE of the four lists of one
    chunk -- in a random order -- and are the top kslot."""
    rng = np.random.default_rng(10 + kslot)
    X = R.grid_rows(rng, 1000, 64)
    Q = R.grid_queries(rng, 3, 64)
    rpc, nch = R.chunking(1000, 3)
    planted = []
    for q, (c, li) in enumerate(((0, 0), (1, 3), (2, 2))):
        rows = R.one_list_rows(c * rpc, min(1000, (c + 1) * rpc), li, kslot, rng)
        R.plant(X, Q[q], rows)
        assert (R.flat_list_of(rows) == li).all() and (rows // rpc == c).all()
        planted.append(rows)
    # scored after ALL plantings: a later one must not displace an earlier one
    S = R.flat_scores(X, Q, _l2_bias(X) if form == "l2" else None, None, None, 2.0 if form == "l2" else 1.0)
    for q in range(3):
        assert R.is_top(S[q], planted[q])


@pytest.mark.parametrize("K", [1, 2, 4, 8, 10, 16])
def test_segment_plantings(K):
    """One lane (r % 32 constant: n >= 32 K), one wave, and the planted rows
    are the top K in the planted order."""
    rng = np.random.default_rng(20 + K)
    n, D = 32 * K + 5, 64
    q = R.grid_queries(rng, 1, D)[0]
    for rows, same in ((R.one_lane_rows(n, 13, K, rng), "lane"), (R.one_wave_rows(n, 2, K, rng), "wave")):
        X = R.grid_rows(rng, n, D)
        R.plant(X, q, rows)
        if same == "lane":
            assert (R.seg_lane_of(rows) == 13).all()
        else:
            assert (R.seg_wave_of(rows) == 2).all() and (K < 8 or np.unique(R.seg_lane_of(rows)).size > 1)
        for bias, alpha in ((None, 1.0), (_l2_bias(X), 2.0)):
            s, _ = R.segment_scores(X, q, bias, None, alpha, -float(q @ q))
            assert R.is_top(s, rows)


def test_tie_planting():
    """Copies of the query tie at the top; the reference returns them by row."""
    rng = np.random.default_rng(30)
    X = R.grid_rows(rng, 600, 64)
    Q = R.grid_queries(rng, 2, 64)
    rows = np.array([515, 3, 131, 259, 7])  # across lists (3, 7), chunks / tiles (131, 259, 515)
    R.plant_ties(X, Q[0], rows)
    S = R.flat_scores(X, Q, _l2_bias(X), None, None, 2.0)
    assert R.is_top(S[0], np.sort(rows))
    assert np.unique(S[0][rows]).size == 1
    assert R.flat_list_of(3) != R.flat_list_of(7)
    assert R.top1_slot_of(3)[0] != R.top1_slot_of(259)[0] and R.top1_slot_of(3)[1] != R.top1_slot_of(131)[1]
    assert R.seg_wave_of(3) == R.seg_wave_of(7) and R.seg_lane_of(3) != R.seg_lane_of(7)  # across lanes of a wave
    assert R.seg_lane_of(3) == R.seg_lane_of(259)  # (one lane: 256 rows apart)


# ---------------------------------------------------------------- the CPU tier of the package
@pytest.mark.parametrize("N,nq,D,k", [(1, 3, 64, 4), (129, 5, 64, 1), (300, 9, 128, 10), (1000, 4, 64, 16), (7, 2, 64, 16)])
def test_cpu_ref_topk_equals_reference(N, nq, D, k):
    """``ops.search._ref_topk`` -- the oracle of the older GPU tests -- bit for
    bit on the exact grid: ties, tombstones, labels, an index offset past
    2^31, fewer live rows than k."""
    from lazzaro_amd.ops.search import _ref_topk, flat_topk
    rng, X, Q, bias = _grid(40 + N, N, D, nq)
    rl = rng.integers(0, 3, size=N).astype(np.int32)
    ql = rng.integers(-1, 4, size=nq).astype(np.int32)
    off = (1 << 31) + 11
    Xt, Qt = torch.from_numpy(X).to(torch.bfloat16), torch.from_numpy(Q).to(torch.bfloat16)
    for b, l, alpha in ((None, False, 1.0), (bias, False, 2.0), (None, True, 1.0), (bias, True, 2.0)):
        S = R.flat_scores(X, Q, b, rl if l else None, ql if l else None, alpha)
        ws, wi = R.topk_of_scores(S, k, 0)
        wi = np.where(wi >= 0, wi + off, -1)
        kw = dict(bias=None if b is None else torch.from_numpy(b), row_label=torch.from_numpy(rl) if l else None,
                  q_label=torch.from_numpy(ql) if l else None, alpha=alpha, idx_offset=off)
        for fn in (_ref_topk, flat_topk):
            gs, gi = fn(Xt, Qt, k, **kw)
            assert np.array_equal(gs.numpy().astype(np.float64), ws) and np.array_equal(gi.numpy(), wi)
        # small chunks: the running merge of _ref_topk keeps the order across chunk borders
        gs, gi = _ref_topk(Xt, Qt, k, chunk=64, **kw)
        assert np.array_equal(gs.numpy().astype(np.float64), ws) and np.array_equal(gi.numpy(), wi)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_cpu_segment_topk_equals_reference(dtype):
    from lazzaro_amd.ops.search import segment_topk
    rng = np.random.default_rng(50)
    D = 64
    sizes = [0, 1, 7, 33, 65, 300]
    xs = [R.grid_rows(rng, n, D, dup=min(6, n // 4)) for n in sizes]
    Q = R.grid_queries(rng, len(sizes), D)
    bs = [(-(x * x).sum(1)).astype(np.float32) for x in xs]
    bs[3][::2] = NEG_INF
    bs[4][:] = NEG_INF  # a segment with no live row
    sc = [(2.0 ** rng.integers(-2, 1, size=n)).astype(np.float32) for n in sizes]
    qb = (-(Q * Q).sum(1)).astype(np.float32)
    t = lambda a, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(a)).to(dt)  # noqa: E731
    for k in (1, 3, 5, 16):
        for use_b, use_s, use_q in ((True, True, True), (True, False, True), (False, False, False), (False, True, False)):
            ws, wi = R.segment_ref(xs, Q, k, bs if use_b else None, sc if use_s else None, 2.0,
                                   qb if use_q else None)
            gs, gi = segment_topk([t(x, dtype) for x in xs], t(Q, dtype), k,
                                  biases=[t(b) for b in bs] if use_b else None,
                                  scales=[t(s) for s in sc] if use_s else None, alpha=2.0,
                                  qbias=t(qb) if use_q else None)
            assert np.array_equal(gs.numpy().astype(np.float64), ws) and np.array_equal(gi.numpy(), wi)


def test_cpu_flat_top1_equals_reference():
    from lazzaro_amd.ops.search import flat_top1
    rng = np.random.default_rng(60)
    X = R.grid_rows(rng, 300, 64)
    Q = R.grid_queries(rng, 40, 64)
    X[[5, 133, 261]] = 0.0  # best score exactly 0, tied, for the queries below
    Xn, Qn = np.abs(X), -np.abs(Q)  # every score <= 0
    for Xa, Qa in ((X, Q), (Xn, Qn)):
        ws, wi = R.top1_ref(Xa, Qa)
        gs, gi = flat_top1(torch.from_numpy(Xa).to(torch.bfloat16), torch.from_numpy(Qa).to(torch.bfloat16))
        assert gi.dtype == torch.int32
        assert np.array_equal(gs.numpy().astype(np.float64), ws) and np.array_equal(gi.numpy().astype(np.int64), wi)
    assert (R.top1_ref(Xn, Qn)[0] == 0.0).all() and (R.top1_ref(Xn, Qn)[1] == 5).all()
    s0, i0 = flat_top1(torch.zeros((0, 64), dtype=torch.bfloat16), torch.from_numpy(Q).to(torch.bfloat16))
    assert bool((s0 == NEG_INF).all()) and bool((i0 == -1).all())


def test_cpu_merge_topk_equals_reference():
    from lazzaro_amd.parallel.sharded import merge_topk
    rng = np.random.default_rng(70)
    nq, nc = 9, 65
    ps = rng.integers(-3, 4, size=(nq, nc)).astype(np.float32)
    pi = (np.stack([rng.permutation(5000)[:nc] for _ in range(nq)]).astype(np.int64) << 30) + (1 << 40)
    empty = rng.random((nq, nc)) < 0.3
    ps[empty], pi[empty] = NEG_INF, -1
    for k in (1, 5, 17, 32):
        ws, wi = R.merge64_ref(ps, pi, k)
        gs, gi = merge_topk(torch.from_numpy(ps), torch.from_numpy(pi), k)
        assert np.array_equal(gs.numpy().astype(np.float64), ws) and np.array_equal(gi.numpy(), wi)


def test_cpu_gather_fields_equals_reference():
    from types import SimpleNamespace

    from lazzaro_amd.ops.tenant_ops import gather_fields
    rng = np.random.default_rng(80)
    cols = [(rng.random(n).astype(np.float32), rng.integers(0, 99, n).astype(np.int32),
             rng.integers(0, 3, n).astype(np.uint8), rng.integers(0, 2, n).astype(np.uint8),
             rng.integers(-1, 8, n).astype(np.int32)) for n in (4, 1, 30)]
    rows = np.stack([np.where(rng.random(6) < 0.3, -1, rng.integers(0, len(c[0]), 6)) for c in cols]).astype(np.int64)
    graphs = [SimpleNamespace(sal=c[0], acc=c[1], kind=c[2], sup=c[3], shard=c[4]) for c in cols]
    got = gather_fields(torch.from_numpy(rows), graphs)
    want = R.gather_fields_ref(rows, cols)
    for n in want:
        assert got[n].dtype == want[n].dtype and np.array_equal(got[n], want[n]), n


# ---------------------------------------------------------------- decidability of the Gaussian cases
KERNEL_K = {"flat": None, "seg_bf16": None, "seg_fp32": None, "top1": 1}


@pytest.mark.parametrize("kernel", list(KERNEL_K))
@pytest.mark.parametrize("case", R.GAUSS_SET_CASES)
def test_gauss_cases_are_decidable(kernel, case):
    """By the reference alone: the must sets fill at least 90 % of the nq * k
    slots, so the GPU file's set checks cannot go vacuous. (Observed: D = 64
    every slot for every kernel; D = 128 above 99 %.)"""
    n, D, nq, k, seed = case
    k = KERNEL_K[kernel] or k
    _, S, B = R.gauss_scores(kernel, n, D, nq, seed)
    dec = R.Decision(S, B, k)
    share = dec.must_share()
    print(f"{kernel} n={n} D={D} k={k}: must share {share:.4f}, decidable {int(dec.decidable.sum())}/{nq}")
    assert share >= R.MUST_SHARE
    assert dec.may.sum(1).min() >= k  # the reference rows themselves are always allowed
    assert (np.take_along_axis(dec.may, dec.ref, 1)).all()


def test_decision_check_accepts_the_reference_and_rejects_errors():
    n, D, nq, k, seed = R.GAUSS_SET_CASES[0]
    _, S, B = R.gauss_scores("flat", n, D, nq, seed)
    dec = R.Decision(S, B, k)
    ws, wi = R.topk_of_scores(S, k)
    bad, worst = dec.check(ws, wi)
    assert bad == [] and worst == 0.0
    # a score half a bound off passes, two bounds off does not
    s2 = ws.copy()
    s2[3, 2] += 0.5 * B[3, wi[3, 2]]
    bad, worst = dec.check(s2, wi)
    assert bad == [] and abs(worst - 0.5) < 1e-6
    s2[3, 2] = ws[3, 2] + 2.0 * B[3, wi[3, 2]]
    assert any("score off" in b for b in dec.check(s2, wi)[0])
    # a must row dropped for the (k + 1)-th, a swapped pair of a decidable query, a repeated row, a short list
    q = int(np.nonzero(dec.decidable)[0][0])
    nxt = np.argsort(-S[q], kind="stable")[k]
    i2, s3 = wi.copy(), ws.copy()
    i2[q, k - 1], s3[q, k - 1] = nxt, S[q, nxt]
    assert any("missing" in b for b in dec.check(s3, i2)[0])
    i2, s3 = wi.copy(), ws.copy()
    i2[q, [0, 1]], s3[q, [0, 1]] = wi[q, [1, 0]], ws[q, [1, 0]]
    assert any("order" in b or "decidable" in b for b in dec.check(s3, i2)[0])
    i2 = wi.copy()
    i2[q, 1] = wi[q, 0]
    assert dec.check(ws, i2)[0]
    i2, s3 = wi.copy(), ws.copy()
    i2[q, k - 1], s3[q, k - 1] = -1, NEG_INF
    assert dec.check(s3, i2)[0]


def test_bounds_follow_the_counted_roundings():
    assert R.seg_roundings(64, "bf16") == 14 and R.seg_roundings(2048, "bf16") == 45
    assert R.seg_roundings(32, "fp32") == 11 and R.seg_roundings(2048, "fp32") == 74
    # a whole-row fma chain (D + 4 roundings) bounds the count for every allowed D
    assert all(R.seg_roundings(D, "bf16") <= D + 4 for D in range(64, 2049, 64))
    assert all(R.seg_roundings(D, "fp32") <= D + 4 for D in range(32, 2049, 32))
    x, q = np.array([[1.0, -2.0] + [0.0] * 62]), np.array([3.0, 4.0] + [0.0] * 62)
    s, b = R.segment_scores(x, q, np.array([-5.0]), np.array([0.5]), 2.0, -25.0, "bf16")
    assert s[0] == 2.0 * (-5.0) * 0.5 - 5.0 - 25.0
    assert b[0] == R.gamma(16) * (2.0 * 11.0 * 0.5 + 5.0 + 25.0)
    s, b = R.segment_scores(x, q, np.array([NEG_INF]), None, 2.0, -25.0, "fp32")
    assert s[0] == NEG_INF and b[0] == R.gamma(14) * (2.0 * 11.0 + 25.0)
    assert R.flat_bound(x, q[None], np.array([-5.0]), 2.0)[0, 0] == R.gamma(67) * (22.0 + 5.0)
    assert R.top1_bound(x, q[None])[0, 0] == R.gamma(65) * 11.0
