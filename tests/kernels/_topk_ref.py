"""fp64 references of the oldest search kernels: the lane path of
``ops/search.py flat_topk`` (csrc/kernels/search.hip ``flat_topk_kernel``,
``topk_merge_kernel``, ``topk_merge64_kernel``), the tenant-segment search
(csrc/kernels/segment.hip ``segment_topk_kernel`` and csrc/kernels/tenant.hip
``tg_gather_fields_kernel``) and the k-means assign (csrc/kernels/search256.hip
``flat_top1_kernel``, ``flat_top1_grouped_kernel``, ``top1_decode_kernel``).
Plain numpy; nothing here touches a GPU or the kernel library.
tests/unit/test_topk_ref_cpu.py checks this module on its own and pins the CPU
tier to it, tests/kernels/test_topk_stages_gpu.py holds the kernels against it.

Order. (score descending, row ascending) -- the kernels' ``better()`` --,
missing entries ``(-inf, -1)``: ``order`` of _ivfpq_ref.py. A row whose score
is -inf (tombstone, label mismatch) is never a result.

Exact grid. ``grid_rows`` / ``grid_queries`` of _cand_ref.py: integers in
[-8, 8], alpha 1 or 2, integer biases (``-|x|^2`` or small integers, -inf =
tombstone), power-of-two scales in {1/4, 1/2, 1}, integer query biases. With
D <= 2048 a product is at most 64, a dot product below 2^17, ``|x|^2`` and
``|q|^2`` at most 2^17, a scaled value a multiple of 1/4 below 2^18: every
partial sum in any order is a multiple of 1/4 below 2^20 < 2^22, so bf16 inputs,
fp32 arithmetic and fp64 agree and results are compared bit for bit, ties
included.

Gaussian inputs, the bounds (``gamma(n) = n u / (1 - n u)``, u = 2^-24; a term
that passes through at most n - 1 roundings is off by at most ``gamma(n)`` of
its magnitude). The roundings, counted from the kernels:

* ``flat_topk_kernel`` (bf16 MFMA, the bound of _mt_ref.py's scan): the D
  products are exact in fp32 (8 x 8 bits) and are accumulated in fp32 in some
  order, at most D roundings on a product; then ``alpha * acc`` and ``+ bias``:
  D + 2 roundings, ``flat bound = gamma(D + 3) (|alpha| sum|q x| + |b|)``.
* ``flat_top1_kernel`` / ``flat_top1_grouped_kernel``: the same accumulation
  with neither alpha nor a bias, and the packed key keeps the fp32 bits:
  ``top1 bound = gamma(D + 1) sum|q x|``.
* ``segment_topk_kernel``, bf16 rows (``Piece<u16>``): lane ``part`` of the
  eight that share a row takes the 8-element pieces part, part + 8, ... A
  piece is a chain of 8 fmas from 0 over exact products (the first adds to 0:
  at most 7 roundings on a product), ``a += piece`` per piece (D / 64 pieces
  per lane, the first add is to 0: D / 64 - 1), three shuffle adds, then
  alpha, scale, bias, qbias: at most ``7 + D/64 - 1 + 3 + 4 = D/64 + 13``
  roundings. Counting one fma chain over the whole row (D + 4 roundings) gives
  an upper bound of this for every allowed D (D >= 64) but it is not the count:
  no term ever sees a chain of D fmas, the dot product is split over 8 lanes
  and over pieces. The bound used
  is ``gamma(D/64 + 15) (|alpha scale| sum|q x| + |b| + |qb|)`` (one spare
  rounding beyond the convention's n - 1).
* ``segment_topk_kernel``, fp32 rows (``Piece<float>``): a piece is
  ``fma(v0, q0, fma(v1, q1, fma(v2, q2, v3 * q3)))``: the innermost product is
  rounded once by the multiply and three times by the fmas (4), ``a += piece``
  D / 32 - 1 times, three shuffle adds and the four epilogue operations: at most
  ``D/32 + 10`` roundings, bound ``gamma(D/32 + 12) (...)``. (Contraction of
  ``alpha * a * scale + bias`` by the compiler only removes roundings.)

A non-finite bias adds nothing to a bound: the score is then -inf exactly.

Row-to-list maps (read from the kernels' epilogues, used by the planting
helpers and checked in test_topk_ref_cpu.py against an enumeration of the
kernels' index expressions):

* ``flat_list_of(row)``: ``flat_topk_kernel`` keeps four lists per (query,
  chunk), one per (``wrow``, ``h``). Chunks start at multiples of 128, so with
  ``t = row % 128`` the tile row is ``t = 64 wrow + 32 rb + 8 (e >> 2) + 4 h +
  (e & 3)``: ``wrow = t >> 6``, ``h = (t >> 2) & 1``, list ``2 wrow + h``.
* ``seg_lane_of(r) = r % 32``: ``segment_topk_kernel`` walks ``r = wave * 8 +
  sub, += 32``; the list lives in lane ``sub * 8`` of wave ``(r % 32) // 8``
  (``seg_wave_of``).
* ``top1_slot_of(r)``: ``flat_top1_kernel``: block ``r // 256``, wave row
  ``(r % 256) // 128`` (one ``atomicMax`` each), lane group ``(r % 16) // 4``
  (merged by the two shuffles).
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np

from tests.kernels._cand_ref import grid_queries, grid_rows, to_bf16, unit_rows  # noqa: F401
from tests.kernels._ivfpq_ref import NEG_INF, U_FP32, gamma, order  # noqa: F401  (one definition for all modules)

BM = 128  # rows per tile of flat_topk_kernel; chunks are whole tiles
TOP1_TILE = 256  # rows / queries per block of the top-1 kernels
TARGET_WGS = 512  # ops.search.TARGET_WGS
KSLOTS = (1, 2, 4, 8, 10, 16)


def kslot_of(k: int) -> int:
    """``lzk_flat_topk_kslot``."""
    for s in KSLOTS:
        if k <= s:
            return s
    return -1


# ---------------------------------------------------------------- flat scores
def _fin_abs(b) -> np.ndarray:
    b = np.asarray(b, dtype=np.float64)
    return np.where(np.isfinite(b), np.abs(b), 0.0)


def flat_scores(X, Q, bias=None, row_label=None, q_label=None, alpha: float = 1.0) -> np.ndarray:
    """fp64 ``alpha <q, x> + bias[row]`` [nq, N]; a row whose label differs from
    the query's (query label < 0: all rows) or whose bias is -inf scores -inf."""
    X = np.asarray(X, dtype=np.float64)
    Q = np.asarray(Q, dtype=np.float64)
    s = float(alpha) * (Q @ X.T)
    if bias is not None:
        with np.errstate(invalid="ignore"):
            s = s + np.asarray(bias, dtype=np.float64)[None, :]
        s[:, np.asarray(bias) == NEG_INF] = NEG_INF
    if row_label is not None:
        ql = np.asarray(q_label, dtype=np.int64)[:, None]
        ok = (ql < 0) | (np.asarray(row_label, dtype=np.int64)[None, :] == ql)
        s = np.where(ok, s, NEG_INF)
    return s


def flat_bound(X, Q, bias=None, alpha: float = 1.0) -> np.ndarray:
    """``gamma(D + 3) (|alpha| sum|q x| + |b|)`` [nq, N]."""
    X = np.asarray(X, dtype=np.float64)
    Q = np.asarray(Q, dtype=np.float64)
    mag = abs(float(alpha)) * (np.abs(Q) @ np.abs(X).T)
    if bias is not None:
        mag = mag + _fin_abs(bias)[None, :]
    return gamma(X.shape[1] + 3) * mag


def top1_bound(X, Q) -> np.ndarray:
    """``gamma(D + 1) sum|q x|`` [nq, N]."""
    X = np.asarray(X, dtype=np.float64)
    return gamma(X.shape[1] + 1) * (np.abs(np.asarray(Q, dtype=np.float64)) @ np.abs(X).T)


# ---------------------------------------------------------------- chunks
def chunking(N: int, n_chunks: int) -> Tuple[int, int]:
    """``launch_flat`` / ``_flat_topk_lane``: (rows_per_chunk rounded up to whole
    128-row tiles, the chunk count recomputed from it)."""
    n_chunks = max(int(n_chunks), 1)
    rpc = -(-(-(-N // n_chunks)) // BM) * BM
    return rpc, max(-(-N // rpc), 1)


def lib_chunks(N: int, nq: int, target_wgs: int = TARGET_WGS) -> int:
    """``lzk_flat_topk_chunks``: the library's own choice."""
    nqb = -(-nq // 128)
    n = min(-(-target_wgs // nqb), -(-N // BM))
    return chunking(N, max(n, 1))[1]


def topk_of_scores(S: np.ndarray, k: int, row0: int = 0):
    """Per query the k best columns of S by (score desc, column asc) as (scores
    fp64 [nq, k], rows int64 [nq, k] + row0), (-inf, -1) past the columns that
    are not -inf."""
    nq, n = S.shape
    os_ = np.full((nq, k), NEG_INF)
    oi = np.full((nq, k), -1, dtype=np.int64)
    m = min(k, n)
    if m:
        o = np.argsort(-S, axis=1, kind="stable")[:, :m]  # stable: equal scores keep ascending columns
        s = np.take_along_axis(S, o, 1)
        os_[:, :m] = s
        oi[:, :m] = np.where(s == NEG_INF, -1, o + row0)
    return os_, oi


def partial_of_scores(S: np.ndarray, n_chunks: int, kslot: int):
    """The ``[nq, n_chunks', kslot]`` partial lists of a score matrix (see
    :func:`partial_ref`). Returns (scores fp64, rows int64, n_chunks')."""
    nq, N = S.shape
    rpc, nch = chunking(N, n_chunks)
    ps = np.full((nq, nch, kslot), NEG_INF)
    pi = np.full((nq, nch, kslot), -1, dtype=np.int64)
    for c in range(nch):
        lo, hi = c * rpc, min(N, (c + 1) * rpc)
        ps[:, c], pi[:, c] = topk_of_scores(S[:, lo:hi], kslot, lo)
    return ps, pi, nch


def partial_ref(X, Q, bias, row_label, q_label, alpha, n_chunks: int, kslot: int):
    """``lzk_flat_topk_partial``: for every (query, chunk) the top ``kslot`` of
    the chunk's rows by (score desc, row asc), padded with (-inf, -1)."""
    return partial_of_scores(flat_scores(X, Q, bias, row_label, q_label, alpha), n_chunks, kslot)


# ---------------------------------------------------------------- merges
def _merge(ps, pi, kout: int, drop_neg_inf: bool):
    ps = np.asarray(ps, dtype=np.float64)
    pi = np.asarray(pi, dtype=np.int64)
    nq = ps.shape[0]
    ps, pi = ps.reshape(nq, -1), pi.reshape(nq, -1)
    os_ = np.full((nq, kout), NEG_INF)
    oi = np.full((nq, kout), -1, dtype=np.int64)
    for q in range(nq):
        f = np.nonzero(pi[q] >= 0)[0]
        o = f[order(ps[q][f], pi[q][f])[:kout]]
        os_[q, : o.size] = ps[q][o]
        oi[q, : o.size] = pi[q][o]
    if drop_neg_inf:
        oi[os_ == NEG_INF] = -1
    return os_, oi


def merge_ref(ps, pi, kout: int, idx_offset: int = 0):
    """``lzk_topk_merge``: ps / pi ``[nq, ncand]`` (or ``[nq, chunks, kslot]``);
    entries with row < 0 are ignored, the rest ordered by (score, row); an
    empty slot or a -inf score comes out as row -1 with no offset added."""
    os_, oi = _merge(ps, pi, kout, True)
    return os_, np.where(oi >= 0, oi + int(idx_offset), -1)


def merge64_ref(ps, pi, kout: int):
    """``lzk_topk_merge64`` (and the CPU branch of ``sharded.merge_topk``): the
    same over int64 ids, except that only id < 0 marks an empty slot: an entry
    with id >= 0 and score -inf keeps its id in both tiers (the lists a search
    gathers never hold one: ``flat_topk`` returns -1 with every -inf)."""
    return _merge(ps, pi, kout, False)


# ---------------------------------------------------------------- segments
def seg_roundings(D: int, dtype: str) -> int:
    """Most roundings any term of a ``segment_topk_kernel`` score passes through
    (module docstring)."""
    return D // 64 + 13 if dtype == "bf16" else D // 32 + 10


def segment_scores(x, q, bias=None, scale=None, alpha: float = 1.0, qb: float = 0.0, dtype: str = "bf16"):
    """One segment under one query: fp64 ``alpha <q, x> scale + bias + qb`` [n]
    (-inf where the bias is) and the bound of every entry."""
    x = np.asarray(x, dtype=np.float64)
    q = np.asarray(q, dtype=np.float64)
    sc = np.ones(x.shape[0]) if scale is None else np.asarray(scale, dtype=np.float64)
    s = float(alpha) * (x @ q) * sc
    mag = abs(float(alpha)) * (np.abs(x) @ np.abs(q)) * np.abs(sc)
    if bias is not None:
        with np.errstate(invalid="ignore"):
            s = s + np.asarray(bias, dtype=np.float64)
        mag = mag + _fin_abs(bias)
    s = s + float(qb)
    mag = mag + abs(float(qb))
    if bias is not None:
        s[np.asarray(bias) == NEG_INF] = NEG_INF
    return s, gamma(seg_roundings(x.shape[1], dtype) + 2) * mag


def segment_ref(xs: Sequence, Q, k: int, biases=None, scales=None, alpha: float = 1.0, qbias=None):
    """``lzk_segment_topk``: query q against the rows ``xs[q]`` only; rows are
    local to the segment, (-inf, -1) past the rows that are not -inf."""
    nq = len(xs)
    os_ = np.full((nq, k), NEG_INF)
    oi = np.full((nq, k), -1, dtype=np.int64)
    for q in range(nq):
        if len(xs[q]) == 0:
            continue
        s, _ = segment_scores(xs[q], Q[q], None if biases is None else biases[q],
                              None if scales is None else scales[q], alpha, 0.0 if qbias is None else qbias[q])
        a, b = topk_of_scores(s[None, :], k)
        os_[q], oi[q] = a[0], b[0]
    return os_, oi


def gather_fields_ref(rows, cols):
    """``lzk_tg_gather_fields``: ``rows`` [nq, k] int64, ``cols[q]`` = (sal f32,
    acc i32, kind u8, sup u8, shard i32) of query q's tenant. Plain indexing; a
    row of -1 gives (0, 0, 0, 0, -1)."""
    rows = np.asarray(rows, dtype=np.int64)
    nq, k = rows.shape
    out = {"sal": np.zeros((nq, k), np.float32), "acc": np.zeros((nq, k), np.int32),
           "kind": np.zeros((nq, k), np.uint8), "sup": np.zeros((nq, k), np.uint8),
           "shard": np.full((nq, k), -1, np.int32)}
    for q in range(nq):
        for j in range(k):
            r = int(rows[q, j])
            if r >= 0:
                for n, c in zip(("sal", "acc", "kind", "sup", "shard"), cols[q]):
                    out[n][q, j] = c[r]
    return out


# ---------------------------------------------------------------- top-1
def top1_ref(X, Q):
    """``lzk_flat_top1``: per query (best ``<q, x>`` fp64, its row int64) by
    (score desc, row asc); (-inf, -1) when there are no rows."""
    X = np.asarray(X, dtype=np.float64)
    Q = np.asarray(Q, dtype=np.float64)
    if X.shape[0] == 0:
        return np.full(Q.shape[0], NEG_INF), np.full(Q.shape[0], -1, dtype=np.int64)
    s, i = topk_of_scores(Q @ X.T, 1)
    return s[:, 0], i[:, 0]


def top1_grouped_ref(C, X, qidx, groups):
    """``lzk_flat_top1_grouped``: ``groups`` = (c0, nc, p0, np) per group:
    position p in [p0, p0 + np) is the data row ``X[qidx[p]]`` and is scored
    against the centroid rows ``C[c0 : c0 + nc]`` only. Per position (score,
    centroid row in C) by (score desc, row asc); (-inf, -1) for a position no
    group covers."""
    npos = len(qidx)
    s = np.full(npos, NEG_INF)
    r = np.full(npos, -1, dtype=np.int64)
    for c0, nc, p0, np_ in groups:
        if nc <= 0 or np_ <= 0:
            continue
        gs, gr = top1_ref(np.asarray(C)[c0: c0 + nc], np.asarray(X)[np.asarray(qidx[p0: p0 + np_], dtype=np.int64)])
        s[p0: p0 + np_], r[p0: p0 + np_] = gs, gr + c0
    return s, r


def grouped_blocks(groups, T: int = TOP1_TILE) -> np.ndarray:
    """The block table of ``index/kmeans.py``'s grouped assign: per group one
    {c0, nc, p0, np} entry for every (query tile, centroid tile), the centroid
    tile fastest; nc / np are what is left from the tile's start."""
    out = []
    for c0, nc, p0, np_ in groups:
        for q in range(0, np_, T):
            for r in range(0, nc, T):
                out.append((c0 + r, nc - r, p0 + q, np_ - q))
    return np.array(out, dtype=np.int32).reshape(-1, 4)


# ---------------------------------------------------------------- row-to-list maps
def flat_list_of(row):
    """List (0..3) of ``flat_topk_kernel`` that is offered ``row``."""
    t = np.asarray(row) % BM
    return 2 * (t >> 6) + ((t >> 2) & 1)


def flat_rows_in_list(lo: int, hi: int, li: int) -> np.ndarray:
    r = np.arange(lo, hi)
    return r[flat_list_of(r) == li]


def seg_lane_of(r):
    return np.asarray(r) % 32


def seg_wave_of(r):
    return (np.asarray(r) % 32) // 8


def top1_slot_of(r):
    """(block, wave row, lane group) of ``flat_top1_kernel`` for row r."""
    r = np.asarray(r)
    return r // TOP1_TILE, (r % TOP1_TILE) // 128, (r % 16) // 4


# ---------------------------------------------------------------- planting
def near_copies(q, m: int) -> np.ndarray:
    """m rows near the grid query q: row j is q with its first j non-zero
    coordinates moved one step towards 0. ``<q, row_j>`` and ``2 <q, row_j> -
    |row_j|^2`` both fall strictly with j (by ``|q_d|`` resp. by 1 per moved
    coordinate), and ``row_0 = q`` attains the largest L2-form score any grid
    row can have. Needs m - 1 non-zero coordinates."""
    q = np.asarray(q, dtype=np.float64)
    nz = np.nonzero(q)[0]
    assert nz.size >= m - 1, "query has too few non-zero coordinates to plant m distinct rows"
    out = np.repeat(q[None, :], m, 0)
    for j in range(1, m):
        d = nz[:j]
        out[j, d] = q[d] - np.sign(q[d])
    return out


def plant(X: np.ndarray, q, rows) -> None:
    """Overwrite ``X[rows[j]]`` with ``near_copies(q)[j]``: rows[0] becomes the
    best row of query q, rows[1] the next, ... (for the caller to verify with
    :func:`is_top`; a bias of ``-|x|^2`` has to be recomputed afterwards)."""
    X[np.asarray(rows, dtype=np.int64)] = near_copies(q, len(rows))


def plant_ties(X: np.ndarray, q, rows) -> None:
    """Every row of ``rows`` becomes a copy of the query itself: one exact tie
    at the top of query q that only the row index breaks."""
    X[np.asarray(rows, dtype=np.int64)] = np.asarray(q, dtype=np.float64)[None, :]


def is_top(s: np.ndarray, rows) -> bool:
    """``rows`` are, in this order, the first len(rows) of the score vector s
    by (score desc, row asc)."""
    rows = np.asarray(rows, dtype=np.int64)
    o = order(np.asarray(s, dtype=np.float64), np.arange(len(s)))[: rows.size]
    return bool(np.array_equal(o, rows)) and bool((np.asarray(s)[rows] != NEG_INF).all())


def one_list_rows(lo: int, hi: int, li: int, m: int, rng) -> np.ndarray:
    """m rows of [lo, hi) that all reach list ``li`` of ``flat_topk_kernel``, in
    random order (so the best row is neither the first nor the last offered)."""
    r = flat_rows_in_list(lo, hi, li)
    assert r.size >= m
    return rng.permutation(r[: max(m, min(r.size, 2 * m))])[:m]


def one_lane_rows(n: int, lane: int, m: int, rng) -> np.ndarray:
    """m rows below n with ``r % 32 == lane`` (needs n >= 32 (m - 1) + lane + 1),
    in random order."""
    r = np.arange(lane, n, 32)
    assert r.size >= m
    return rng.permutation(r)[:m]


def one_wave_rows(n: int, wave: int, m: int, rng) -> np.ndarray:
    """m rows below n that wave ``wave`` of ``segment_topk_kernel`` scans, from
    as many of its lanes as there are, in random order."""
    r = np.arange(n)
    r = r[seg_wave_of(r) == wave]
    assert r.size >= m
    return rng.permutation(r)[:m]


# ---------------------------------------------------------------- Gaussian cases
GAUSS_SET_CASES = ((257, 64, 64, 10, 0), (1000, 128, 64, 16, 0))  # n, D, nq, k, seed: set and score checks
GAUSS_SCORE_CASES = ((300, 768, 32, 10, 0),)  # D = 768: per-element score bound only (almost no query is decidable)
MUST_SHARE = 0.9  # the must sets fill at least this share of the nq * k slots of every set case


def gauss_case(n: int, D: int, nq: int, seed: int, dtype: str = "bf16"):
    """Unit-norm rows and queries rounded to ``dtype`` (as fp64 values), the
    L2 serving form ``alpha = 2, bias = -|x|^2, qbias = -|q|^2`` (both fp32),
    every 37th row from row 5 a tombstone. Returns (X, Q, bias, qbias)."""
    rng = np.random.default_rng(1000 * seed + n + D)
    X, Q = unit_rows(rng, n, D), unit_rows(rng, nq, D)
    if dtype == "bf16":
        X, Q = to_bf16(X), to_bf16(Q)
    else:
        X, Q = X.astype(np.float32).astype(np.float64), Q.astype(np.float32).astype(np.float64)
    bias = (-(X * X).sum(1)).astype(np.float32)
    bias[5::37] = NEG_INF
    qbias = (-(Q * Q).sum(1)).astype(np.float32)
    return X, Q, bias, qbias


def gauss_scores(kernel: str, n: int, D: int, nq: int, seed: int):
    """The Gaussian case of one kernel: "flat" (``2 <q, x> - |x|^2``, bf16),
    "seg_bf16" / "seg_fp32" (``2 <q, x> - |x|^2 - |q|^2``) or "top1" (``<q, x>``,
    bf16, no tombstones). Returns (inputs of :func:`gauss_case`, fp64 scores
    [nq, n], bounds [nq, n])."""
    dtype = "fp32" if kernel == "seg_fp32" else "bf16"
    X, Q, bias, qbias = gauss_case(n, D, nq, seed, dtype)
    if kernel == "flat":
        return (X, Q, bias, qbias), flat_scores(X, Q, bias, alpha=2.0), flat_bound(X, Q, bias, 2.0)
    if kernel == "top1":
        return (X, Q, bias, qbias), Q @ X.T, top1_bound(X, Q)
    S = np.empty((nq, n))
    B = np.empty((nq, n))
    for q in range(nq):
        S[q], B[q] = segment_scores(X, Q[q], bias, None, 2.0, qbias[q], dtype)
    return (X, Q, bias, qbias), S, B


class Decision:
    """What a correct fp32 kernel may return for the top k of the score rows
    ``S`` [nq, N] (fp64) given the per-entry bounds ``B``.

    ``ref`` [nq, k]: the fp64 top-k rows (-1 past the live rows). ``must``
    [nq, k] bool: the reference row's score less its bound exceeds every row
    outside the reference top-k plus that row's bound (the largest of them is
    the (k+1)-th up to the spread of the bounds): no rounding can push it out.
    ``may`` [nq, N] bool: the live rows whose score plus bound reaches the
    smallest (score - bound) of the reference top-k: only these can appear.
    ``decidable`` [nq]: every live reference row is a must row and consecutive
    reference rows differ by more than the sum of their bounds: rows and their
    order are forced."""

    def __init__(self, S: np.ndarray, B: np.ndarray, k: int):
        self.S, self.B, self.k = S, B, k
        nq, N = S.shape
        live = S != NEG_INF
        lo = np.where(live, S - B, NEG_INF)
        hi = np.where(live, S + B, NEG_INF)
        self.lo, self.hi = lo, hi
        _, self.ref = topk_of_scores(S, k)
        okr = self.ref >= 0
        rr = np.where(okr, self.ref, 0)
        in_ref = np.zeros((nq, N), dtype=bool)
        in_ref[np.nonzero(okr)[0], self.ref[okr]] = True
        rest = np.where(in_ref, NEG_INF, hi).max(1) if N else np.full(nq, NEG_INF)
        ref_lo = np.where(okr, np.take_along_axis(lo, rr, 1), np.inf) if N else np.full((nq, k), np.inf)
        ref_hi = np.where(okr, np.take_along_axis(hi, rr, 1), NEG_INF) if N else np.full((nq, k), NEG_INF)
        self.must = okr & (ref_lo > rest[:, None])
        self.may = live & (hi >= ref_lo.min(1)[:, None])
        gaps = ~okr[:, 1:] | (ref_lo[:, :-1] > ref_hi[:, 1:])
        self.decidable = (self.must | ~okr).all(1) & gaps.all(1)
        self.n_live = live.sum(1)

    def must_share(self) -> float:
        return float(self.must.sum()) / float(self.must.size)

    def check(self, got_s, got_r) -> Tuple[List[str], float]:
        """Hold returned (scores [nq, k], rows [nq, k]) against the decision.
        Returns (violations, the largest |score - fp64| / bound seen)."""
        S, B, k = self.S, self.B, self.k
        got_s = np.asarray(got_s, dtype=np.float64)
        got_r = np.asarray(got_r, dtype=np.int64)
        bad: List[str] = []
        worst = 0.0
        for q in range(S.shape[0]):
            r = got_r[q]
            m = int(min(k, self.n_live[q]))
            if not ((r[:m] >= 0).all() and (r[m:] == -1).all() and (got_s[q, m:] == NEG_INF).all()):
                bad.append(f"q{q}: {m} live results expected, rows {r.tolist()}")
                continue
            r = r[:m]
            if (r >= S.shape[1]).any() or np.unique(r).size != m:
                bad.append(f"q{q}: rows out of range or repeated {r.tolist()}")
                continue
            err = np.abs(got_s[q, :m] - S[q, r])
            with np.errstate(invalid="ignore", divide="ignore"):
                ratio = np.where(err == 0.0, 0.0, err / B[q, r])
            if m:
                worst = max(worst, float(ratio.max()))
            if (ratio > 1.0).any():
                bad.append(f"q{q}: score off by {float(ratio.max()):.3f} bounds")
            need = self.ref[q][self.must[q]]
            if not np.isin(need, r).all():
                bad.append(f"q{q}: must rows {np.setdiff1d(need, r).tolist()} missing")
            if not self.may[q, r].all():
                bad.append(f"q{q}: rows {r[~self.may[q, r]].tolist()} cannot be in the top {k}")
            if m > 1 and not (self.hi[q, r[:-1]] >= self.lo[q, r[1:]]).all():
                bad.append(f"q{q}: order violated beyond the bounds")
            if self.decidable[q] and not np.array_equal(got_r[q], self.ref[q]):
                bad.append(f"q{q}: decidable, rows {got_r[q].tolist()} != {self.ref[q].tolist()}")
        return bad, worst
