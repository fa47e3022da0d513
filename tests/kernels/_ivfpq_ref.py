"""fp64 references of the IVF-PQ query kernels (csrc/kernels/ivfpq.hip):
``ivfpq_scan_kernel``, ``ivfpq_scan_deep_kernel``, ``ivfpq_scan_thresh_kernel``
and ``rerank_kernel``. Plain numpy; nothing here touches a GPU or the kernel
library (the fp8 decoder goes through ``torch.float8_e4m3fn`` on the CPU).
tests/unit/test_ivfpq_ref_cpu.py checks this module on its own,
tests/kernels/test_ivfpq_scan_gpu.py holds the kernels against it.

Order. Every ranking is (score descending, code row ascending): the kernels'
``better()``. Missing entries are ``(-inf, -1)``.

Exact grid. A scan score is ``base + sum_j LUT[j][code_j]``: M fp32 additions.
With integer ``base`` and LUT entries in [-1024, 1024] every partial sum is an
integer of magnitude at most (M + 1) * 1024 <= 129 * 1024 < 2^24, hence
exactly representable in fp32: the kernel's result has the bits of the fp64
sum whatever the order of the additions. A re-rank score is ``scale * sum_d
v_d q_d`` with integer v_d, q_d in [-8, 8] (exact in bf16, e4m3 and int8):
products are at most 64, every partial sum (fma chain or shuffle tree) is an
integer of at most 768 * 64 < 2^24, and the scale is a power of two -- exact
again. On such inputs the GPU tests compare bits, ties included.

Gaussian inputs, the bound. For any order of summing n - 1 floating-point
terms t_i (n - 2 additions; n - 1 if the accumulator starts from a value that
is itself a term), each rounded with unit round-off u = 2^-24, the computed
sum is ``sum_i t_i (1 + e_i)`` with ``|e_i| <= (1 + u)^(n-1) - 1 <= gamma_n``,
``gamma_n = n u / (1 - n u)`` (Higham, Accuracy and Stability of Numerical
Algorithms, Lemma 3.1 and section 4.2). So ``|computed - exact| <= gamma_n
sum_i |t_i|`` for every order, with n = the number of accumulated terms + 1:

* scans: the M + 1 terms ``base, LUT[0][c_0], ..., LUT[M-1][c_{M-1}]``
  (inputs are fp32, so the terms themselves are exact): ``gamma_{M+2} (|base|
  + sum_j |LUT[j][c_j]|)``;
* re-rank: the D products ``v_d q_d`` (each fma rounds once, the 16-lane
  shuffle tree adds four more roundings to a partial, which stays below the D
  roundings counted) and one more rounding for the multiply by the row scale:
  D + 1 accumulated terms, ``gamma_{D+2} scale sum_d |v_d q_d|``.
"""
from __future__ import annotations

import numpy as np

NEG_INF = float("-inf")
U_FP32 = 2.0 ** -24
LANES, WAVE, LANE_K = 256, 64, 16  # threads per block, lanes per wave, rows a lane keeps in the deep scan
LIST_SIZES = (0, 1, 3, 63, 255, 256, 257, 700)  # the GPU tests' shared list layout
DEEP_LIST = 5120  # 20 rows per lane: the deep scan's per-lane cut at 16 is active


def gamma(n: int) -> float:
    return n * U_FP32 / (1.0 - n * U_FP32)


def order(scores: np.ndarray, rows: np.ndarray) -> np.ndarray:
    """Permutation that sorts by (score desc, row asc)."""
    return np.lexsort((rows, -scores))


def _terms(codes: np.ndarray, lut_q: np.ndarray) -> np.ndarray:
    M = codes.shape[1]
    return np.asarray(lut_q, dtype=np.float64)[np.arange(M)[None, :], codes.astype(np.int64)]


def pq_scores(codes: np.ndarray, lut_q: np.ndarray, base) -> np.ndarray:
    """fp64 ``base + sum_j lut_q[j][codes[r, j]]`` of the code rows ``codes``
    ([rows, M] uint8) under one query's table ``lut_q`` ([M, 256])."""
    return float(base) + _terms(codes, lut_q).sum(1)


def pq_bound(codes: np.ndarray, lut_q: np.ndarray, base) -> np.ndarray:
    """Per row, how far a correct fp32 scan score may be from :func:`pq_scores`."""
    return gamma(codes.shape[1] + 2) * (abs(float(base)) + np.abs(_terms(codes, lut_q)).sum(1))


def pq_scores_fp32_loop(codes: np.ndarray, lut_q: np.ndarray, base) -> np.ndarray:
    """The kernel's arithmetic emulated: fp32 adds in the order j = 0..M-1."""
    s = np.full(codes.shape[0], np.float32(base), dtype=np.float32)
    lq = np.asarray(lut_q, dtype=np.float32)
    for j in range(codes.shape[1]):
        s = (s + lq[j][codes[:, j].astype(np.int64)]).astype(np.float32)
    return s


def _list_rows(list_off, l: int):
    if l < 0:
        return 0, 0
    return int(list_off[l]), int(list_off[l + 1])


def _pad(s: np.ndarray, r: np.ndarray, K: int):
    os_ = np.full(K, NEG_INF)
    oi = np.full(K, -1, dtype=np.int64)
    n = min(K, s.shape[0])
    os_[:n], oi[:n] = s[:n], r[:n]
    return os_, oi


def _list_scores(codes, list_off, probes, coarse, lut, q: int, p: int):
    r0, r1 = _list_rows(list_off, int(probes[q, p]))
    rows = np.arange(r0, r1, dtype=np.int64)
    return pq_scores(codes[r0:r1], lut[q], coarse[q, p]), rows, r0


def scan_ref(codes, list_off, probes, coarse, lut, K: int):
    """``lzk_ivfpq_scan``: per (query, probe) the best K rows of the probed
    list. Returns (scores fp64, rows int64), both [nq, nprobe, K]."""
    nq, nprobe = probes.shape
    S = np.full((nq, nprobe, K), NEG_INF)
    R = np.full((nq, nprobe, K), -1, dtype=np.int64)
    for q in range(nq):
        for p in range(nprobe):
            s, rows, _ = _list_scores(codes, list_off, probes, coarse, lut, q, p)
            o = order(s, rows)[:K]
            S[q, p], R[q, p] = _pad(s[o], rows[o], K)
    return S, R


def deep_ref(codes, list_off, probes, coarse, lut, width: int):
    """``lzk_ivfpq_scan_deep`` with its documented approximation: thread t of
    the block owns rows r0 + t, r0 + t + 256, ... and keeps its best 16; wave
    w = threads 64w..64w+63 emits the best ``width / 4`` rows of the union of
    its lanes' lists. ``width`` = ``lzk_ivfpq_deep_width()``. Returns (scores
    fp64, rows int64), both [nq, nprobe, 4, width / 4] -- flattened, entry
    ``(qp * 4 + w) * (width / 4) + j`` of the kernel's output."""
    nq, nprobe = probes.shape
    W = width // 4
    S = np.full((nq, nprobe, 4, W), NEG_INF)
    R = np.full((nq, nprobe, 4, W), -1, dtype=np.int64)
    for q in range(nq):
        for p in range(nprobe):
            s, rows, r0 = _list_scores(codes, list_off, probes, coarse, lut, q, p)
            thread = (rows - r0) % LANES
            keep = np.zeros(rows.shape[0], dtype=bool)
            for t in np.unique(thread):
                mine = np.nonzero(thread == t)[0]
                keep[mine[order(s[mine], rows[mine])[:LANE_K]]] = True
            for w in range(4):
                sel = np.nonzero(keep & (thread // WAVE == w))[0]
                o = sel[order(s[sel], rows[sel])[:W]]
                S[q, p, w], R[q, p, w] = _pad(s[o], rows[o], W)
    return S, R


def thresh_ref(codes, list_off, probes, coarse, lut, thr):
    """``lzk_ivfpq_scan_thresh``: per query the set of (row, score) over all
    its probed lists with ``score >= thr[q]``, as (rows int64 ascending,
    scores fp64) -- the kernel appends in no particular order."""
    nq, nprobe = probes.shape
    out = []
    for q in range(nq):
        rs, ss = [np.zeros(0, dtype=np.int64)], [np.zeros(0)]
        for p in range(nprobe):
            s, rows, _ = _list_scores(codes, list_off, probes, coarse, lut, q, p)
            take = s >= float(thr[q])
            rs.append(rows[take])
            ss.append(s[take])
        r, s = np.concatenate(rs), np.concatenate(ss)
        o = np.argsort(r, kind="stable")
        out.append((r[o], s[o]))
    return out


def merge_topk(S: np.ndarray, R: np.ndarray, k: int):
    """Top-k by (score desc, row asc) over the last axes of per-probe lists
    ([nq, ...]), -1 rows ignored, padded: what ``lzk_topk_merge`` or a sort of
    the pooled deep candidates makes of them."""
    nq = S.shape[0]
    os_ = np.full((nq, k), NEG_INF)
    oi = np.full((nq, k), -1, dtype=np.int64)
    for q in range(nq):
        s, r = S[q].reshape(-1), R[q].reshape(-1)
        s, r = s[r >= 0], r[r >= 0]
        o = order(s, r)[:k]
        os_[q], oi[q] = _pad(s[o], r[o], k)
    return os_, oi


# ------------------------------------------------------------------ re-rank
FMT_BF16, FMT_FP8, FMT_INT8 = 0, 1, 2


def row_bytes(fmt: int, D: int) -> int:
    return D if fmt else 2 * D


def encode_rows(vals: np.ndarray, fmt: int, ldv: int, pad_byte: int = 0x7F) -> np.ndarray:
    """Raw rows ([n, ldv] uint8) of the kept copy holding ``vals`` ([n, D],
    values the format represents exactly or that are rounded to it). Bytes
    past the row are ``pad_byte`` (0x7f: NaN as e4m3, so a kernel that read
    them would show)."""
    import torch
    n, D = vals.shape
    t = torch.from_numpy(np.ascontiguousarray(vals, dtype=np.float32))
    if fmt == FMT_BF16:
        b = t.to(torch.bfloat16).view(torch.uint8)
    elif fmt == FMT_FP8:
        b = t.to(torch.float8_e4m3fn).view(torch.uint8)
    else:
        b = torch.round(t).clamp_(-127, 127).to(torch.int8).view(torch.uint8)
    raw = np.full((n, ldv), pad_byte, dtype=np.uint8)
    raw[:, : row_bytes(fmt, D)] = b.numpy().reshape(n, -1)
    return raw


def decode_rows(raw: np.ndarray, fmt: int, D: int, vscale=None) -> np.ndarray:
    """fp64 values ([n, D]) of raw rows ([n, ldv] uint8): bf16; fp8 e4m3 x
    row scale; int8 x row scale."""
    import torch
    b = np.ascontiguousarray(raw[:, : row_bytes(fmt, D)])
    if fmt == FMT_BF16:
        v = (b.view(np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    elif fmt == FMT_FP8:
        v = torch.from_numpy(b).view(torch.float8_e4m3fn).to(torch.float64).numpy()
    else:
        v = b.view(np.int8).astype(np.float64)
    if fmt != FMT_BF16:
        v = v * np.asarray(vscale, dtype=np.float64)[:, None]
    return v


def rerank_scores(V64: np.ndarray, rows: np.ndarray, Q: np.ndarray):
    """fp64 ``<Q[q], V64[rows[q, c]]>`` ([nq, R]; -inf where the row is -1)
    and the matching ``sum_d |v_d q_d|``."""
    Q64 = np.asarray(Q, dtype=np.float64)
    v = V64[np.maximum(rows, 0)]  # [nq, R, D]
    s = np.einsum("qrd,qd->qr", v, Q64)
    mag = np.einsum("qrd,qd->qr", np.abs(v), np.abs(Q64))
    return np.where(rows >= 0, s, NEG_INF), np.where(rows >= 0, mag, 0.0)


def rerank_bound(V64, rows, Q) -> np.ndarray:
    """Per candidate, how far a correct fp32 re-rank score may be from
    :func:`rerank_scores` (``V64`` carries the row scale already)."""
    return gamma(V64.shape[1] + 2) * rerank_scores(V64, rows, Q)[1]


def rerank_ref(V64: np.ndarray, rows: np.ndarray, Q: np.ndarray, kout: int):
    """``lzk_rerank`` on decoded values: the top-``kout`` of each query's
    valid (>= 0) rows. Returns (scores fp64, rows int64), both [nq, kout]."""
    s, _ = rerank_scores(V64, rows, Q)
    nq = rows.shape[0]
    os_ = np.full((nq, kout), NEG_INF)
    oi = np.full((nq, kout), -1, dtype=np.int64)
    for q in range(nq):
        ok = rows[q] >= 0
        sq, rq = s[q][ok], rows[q][ok].astype(np.int64)
        o = order(sq, rq)[:kout]
        os_[q], oi[q] = _pad(sq[o], rq[o], kout)
    return os_, oi


def rerank_fp32_emulated(vals: np.ndarray, scale, q: np.ndarray, fmt: int) -> np.ndarray:
    """One query against raw values ([n, D]) as the kernel computes it: 16
    lanes, lane l takes the 16 bytes at ``256 j + 16 l`` of every 256-byte
    step (16 values, 8 as bf16), fp32 accumulation, a 4-step shuffle tree,
    then the row scale. (The fma is emulated as multiply then add: the same
    where the product is exact.)"""
    n, D = vals.shape
    per = 16 if fmt else 8
    v = vals.astype(np.float32).reshape(n, -1, 16, per)
    qq = np.asarray(q, dtype=np.float32).reshape(-1, 16, per)
    acc = np.zeros((n, 16), dtype=np.float32)
    for j in range(v.shape[1]):
        for e in range(per):
            acc = (acc + (v[:, j, :, e] * qq[j, :, e][None, :]).astype(np.float32)).astype(np.float32)
    for o in (8, 4, 2, 1):
        acc = (acc + acc[:, np.arange(16) ^ o]).astype(np.float32)
    return (acc[:, 0] * np.asarray(scale, dtype=np.float32)).astype(np.float32)


# ------------------------------------------------------------------ inputs
HOT = 255       # the planted rows' code byte
RAND_CODES = 240  # random rows draw codes below this
TIERS = 13


def layout(sizes=LIST_SIZES):
    off = np.zeros(len(sizes) + 1, dtype=np.int64)
    off[1:] = np.cumsum(sizes)
    return off


# (tier, offsets in the list): tier t scores Smax - t for every query, so the
# head of a list reads, by rank: two tied rows at distance 1 (straddling K =
# 1), one row, two tied at distance 64 (K = 4), four rows, two tied at
# distance 256 = the same lane (K = 10), four rows, four tied at distances 1,
# 64 and 256 (ranks 16..19: K = 16). Offsets past the end of a list are dropped.
PLAN = ((0, (5, 6)), (1, (100,)), (2, (10, 74)), (3, (20,)), (4, (200,)), (5, (33,)), (6, (150,)),
        (7, (0, 256)), (8, (50,)), (9, (250,)), (10, (60,)), (11, (130,)), (12, (300, 301, 364, 556)))
DEEP_LANE = 7  # of the DEEP_LIST-row list: every row of this lane is planted (20 > 16 rows, all near the top)


def grid_codes(rng, list_off, M: int) -> np.ndarray:
    """Code rows for the exact-grid tests: random bytes below ``RAND_CODES``,
    plus planted rows (all bytes ``HOT`` but byte 0 = ``HOT - tier``) by
    ``PLAN`` in every list, so equal scores sit at row distances 1, 64 and
    256 around every K. A 3-row list gets rows 0 and 1 equal. A list of
    ``DEEP_LIST`` rows also has all 20 rows of lane ``DEEP_LANE`` planted
    (tiers cycling), more good rows than the lane keeps."""
    n = int(list_off[-1])
    codes = rng.integers(0, RAND_CODES, size=(n, M), dtype=np.uint8)

    def plant(r, tier):
        codes[r] = HOT
        codes[r, 0] = HOT - tier
    for l in range(len(list_off) - 1):
        r0, sz = int(list_off[l]), int(list_off[l + 1] - list_off[l])
        for tier, offs in PLAN:
            for o in offs:
                if o < sz:
                    plant(r0 + o, tier)
        if sz == 3:
            codes[r0 + 1] = codes[r0]
        if sz == DEEP_LIST:
            for k in range(sz // LANES):
                plant(r0 + DEEP_LANE + LANES * k, k % TIERS)
    return codes


def grid_lut(rng, nq: int, nprobe: int, M: int):
    """(lut fp32 [nq, M, 256], coarse fp32 [nq, nprobe]): integers in
    [-1024, 1024]. Entries of the random codes stay <= 1000, ``HOT`` is 1024
    in every sub-space and byte ``HOT - t`` of sub-space 0 is 1024 - t, so a
    planted row of tier t scores ``base + 1024 M - t`` and every random row
    at most ``base + 1000 M``: below all tiers."""
    lut = rng.integers(-1024, 1001, size=(nq, M, 256)).astype(np.float32)
    lut[:, :, HOT] = 1024.0
    for t in range(TIERS):
        lut[:, 0, HOT - t] = 1024.0 - t
    coarse = rng.integers(-1024, 1025, size=(nq, nprobe)).astype(np.float32)
    return lut, coarse


def gauss_inputs(rng, list_off, nq: int, nprobe: int, M: int):
    """(codes, lut, coarse): uniform code bytes, standard normal fp32 tables."""
    codes = rng.integers(0, 256, size=(int(list_off[-1]), M), dtype=np.uint8)
    lut = rng.standard_normal((nq, M, 256)).astype(np.float32)
    coarse = rng.standard_normal((nq, nprobe)).astype(np.float32)
    return codes, lut, coarse


def grid_vectors(rng, n: int, D: int, dup: int = 500):
    """(values [n, D] integers in [-8, 8], scales [n] powers of two): rows i
    and i + n // 2 are equal, values and scale, for i < ``dup``."""
    vals = rng.integers(-8, 9, size=(n, D)).astype(np.float32)
    scale = (2.0 ** rng.integers(-3, 4, size=n)).astype(np.float32)
    vals[n // 2: n // 2 + dup] = vals[:dup]
    scale[n // 2: n // 2 + dup] = scale[:dup]
    return vals, scale


def grid_queries(rng, nq: int, D: int) -> np.ndarray:
    return rng.integers(-8, 9, size=(nq, D)).astype(np.float32)
