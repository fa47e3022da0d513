"""Keyword and hybrid search on the device: the BM25 top-k over a tenant's
lexical columns and its fusion with the dense pool (csrc/kernels/lexical.hip),
with their numpy / torch formulations.

Columns (engine/lexicon.py builds them; core/lexical.py defines the terms):
``slots`` [n, W], W in {8, 16, 32} -- a slot is ``(t << 8) | tf``, used slots
first, ascending by the 24-bit term id ``t``, then zeros; held as int32 bit
patterns in torch -- and ``dl`` int32 [n], the row's word count.

BM25 contract. Query ``m`` holds at most 32 distinct terms ``qterms[m]``
(ascending, zeros after) with weights ``w[m]`` (float64, finite; the idf,
computed on the host -- Lexicon.weights). With ``k1``, ``b`` and ``avgdl``
(> 0), in fp64, in this order, no contraction:

    K(r)    = k1 * ((1 - b) + b * (dl[r] / avgdl))
    c(j)    = w[m, t_j] * ((tf_j * (k1 + 1)) / (tf_j + K(r)))   for each used slot j of r whose term is a query term
    s(m, r) = (float)(sum of c(j) in ascending slot order)       rounded once

A row is eligible when ``bias[r]`` is finite and ``s > 0``. ``lex_topk``
returns per query the ``k`` (1 .. 64) eligible rows with the largest ``s``,
ties to the lower row, descending, padded with (-inf, -1). It is plain IEEE
fp64, so the numpy formulation and the oracle reproduce every bit.

Fusion contract (``lex_fuse``). Candidates: the union of a dense pool and a
lexical pool (graph rows; < 0 or >= n: empty). Each scores

    blend = (1 - alpha) * cos(q, v) + alpha * lexn(m, v)
    lexn  = s(m, v) / den[m],  den[m] = (float)((k1 + 1) * (w[m, 0] + w[m, 1] + ...)),  0 when den[m] is 0

``cos`` over the fp32 row and the fp32 query, 0 when either norm is 0. The
``k`` largest blends come back, descending, ties to the lower row, (-inf, -1)
once the candidates run out. ``lexn`` is in [0, 1): tf (k1 + 1) / (tf + K) <
k1 + 1.

Rounding. The kernel's dot products take mmr.hip's order: at most
``LEX_SUM_DEPTH(D) = 4 ceil(D / 64) + 4`` fp32 roundings each. ``lex_tol(D)``
bounds |blend32 - blend64|: L for the dot, L jointly for the two norms, 4 for
the two square roots, the product of the norms and the divide -- the cosine,
of magnitude <= 1 -- then the rounding of s to fp32 (the oracle shares it),
of den, their quotient, ``1 - alpha``, the two products and the sum, every
term of magnitude <= 1: 2 L + 12 units of 2^-24 with room to spare.

Device tensors always take the kernels; CPU tensors take the ``*_ref``
formulations (the CPU tier, and the second formulation the tests hold to the
oracle).
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._dot16 import sum_depth as LEX_SUM_DEPTH  # lex_fuse uses mmr.hip's dot layout (csrc/include/lzk_dot16.h)

NEG_INF = float("-inf")
T_MAX = 32      # lexical.hip LX_T
TILE_Q = 8      # lexical.hip LX_TQ
MAX_K = 64
SLOT_CHOICES = (8, 16, 32)
PAD_TERM = 0xFFFFFFFF


def lex_tol(D: int) -> float:
    """|blend32 - blend64| of lex_fuse (see 'Rounding' above)."""
    return (2 * LEX_SUM_DEPTH(D) + 12) * 2.0 ** -24


_lib.register("lzk_lex_scan_blocks", _lib.I, [_lib.L, _lib.I, _lib.I])
_lib.register("lzk_lex_scan", _lib.I, [_lib.P, _lib.P, _lib.P, _lib.L, _lib.I, _lib.P, _lib.P, _lib.I, _lib.D, _lib.D,
                                       _lib.D, _lib.I, _lib.P, _lib.P, _lib.P])
_lib.register("lzk_lex_fuse", _lib.I, [_lib.P, _lib.L, _lib.L, _lib.P, _lib.L, _lib.I, _lib.I, _lib.P, _lib.P, _lib.I,
                                       _lib.P, _lib.P, _lib.I, _lib.P, _lib.P, _lib.P, _lib.D, _lib.D, _lib.D, _lib.F,
                                       _lib.I, _lib.P, _lib.P, _lib.P])


def _check_terms(qterms, w):
    qt = np.ascontiguousarray(np.asarray(qterms), dtype=np.uint32)
    wv = np.ascontiguousarray(np.asarray(w), dtype=np.float64)
    if qt.ndim == 1:
        qt, wv = qt[None, :], wv[None, :]
    if qt.ndim != 2 or qt.shape != wv.shape or qt.shape[1] > T_MAX:
        raise ValueError(f"qterms and w are [M, T <= {T_MAX}] (got {qt.shape}, {wv.shape})")
    if qt.shape[1] < T_MAX:
        pad = T_MAX - qt.shape[1]
        qt = np.pad(qt, ((0, 0), (0, pad)))
        wv = np.pad(wv, ((0, 0), (0, pad)))
    used = qt > 0
    if (used[:, 1:] & ~used[:, :-1]).any() or (used[:, 1:] & (qt[:, 1:] <= qt[:, :-1])).any():
        raise ValueError("each query's terms are distinct and ascending, zeros after")
    if not np.isfinite(wv).all():
        raise ValueError("the term weights must be finite")
    return qt, np.where(used, wv, 0.0)


def _check_params(k, k1, b, avgdl):
    if not 1 <= int(k) <= MAX_K:
        raise ValueError(f"k must be in 1 .. {MAX_K} (got {k})")
    if not (float(k1) >= 0.0 and np.isfinite(k1)):
        raise ValueError(f"k1 must be >= 0 and finite (got {k1})")
    if not 0.0 <= float(b) <= 1.0:
        raise ValueError(f"b must be in [0, 1] (got {b})")
    if not (float(avgdl) > 0.0 and np.isfinite(avgdl)):
        raise ValueError(f"avgdl must be > 0 (got {avgdl})")


def _check_cols(slots, dl):
    if slots.dim() != 2 or slots.shape[1] not in SLOT_CHOICES or slots.dtype != torch.int32:
        raise ValueError(f"slots is int32 [n, W] with W in {SLOT_CHOICES} (got {tuple(slots.shape)}, {slots.dtype})")
    if dl.dtype != torch.int32 or dl.shape[0] < slots.shape[0]:
        raise ValueError("dl is int32 [n]")


def lexn_den(w, k1: float) -> np.ndarray:
    """``den`` of the fusion, fp32 [M]: (k1 + 1) times the sum of a query's
    weights, added in slot order in fp64 and rounded once."""
    wv = np.asarray(w, dtype=np.float64)
    if wv.ndim == 1:
        wv = wv[None, :]
    tot = np.cumsum(wv, axis=1)[:, -1] if wv.shape[1] else np.zeros(len(wv))
    return ((float(k1) + 1.0) * tot).astype(np.float32)


def tile_tables(qt: np.ndarray, w: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """The merged term table of every tile of 8 queries, as lexical.hip reads
    them: (uint32 [tiles, 256] ascending, 0xffffffff padded, a term listed
    once per query that holds it; float64 [tiles, 256, 8]: the weight of each
    entry's term for each of the tile's queries, 0 where a query lacks it)."""
    M = qt.shape[0]
    tiles = -(-M // TILE_Q)
    qp = np.zeros((tiles * TILE_Q, T_MAX), dtype=np.uint32)
    wp = np.zeros((tiles * TILE_Q, T_MAX), dtype=np.float64)
    qp[:M], wp[:M] = qt, w
    utab = np.sort(np.where(qp == 0, np.uint32(PAD_TERM), qp).reshape(tiles, TILE_Q * T_MAX), axis=1)
    uw = np.zeros((tiles * TILE_Q * T_MAX, TILE_Q), dtype=np.float64)
    # every tile's row is sorted, so (tile, term) keys are sorted over the whole table: one search places all terms
    tile_of = (np.arange(tiles * TILE_Q, dtype=np.uint64) // TILE_Q)[:, None] << np.uint64(32)
    flat = (utab.astype(np.uint64) + (np.arange(tiles, dtype=np.uint64)[:, None] << np.uint64(32))).ravel()
    used = qp != 0
    keys = (qp.astype(np.uint64) + tile_of)[used]
    wk = wp[used]
    qk = np.broadcast_to((np.arange(tiles * TILE_Q) % TILE_Q)[:, None], qp.shape)[used]
    lo, hi = np.searchsorted(flat, keys, "left"), np.searchsorted(flat, keys, "right")
    for d in range(TILE_Q):  # (a term is listed once per query of the tile that holds it)
        at = lo + d
        m = at < hi
        if not m.any():
            break
        uw[at[m], qk[m]] = wk[m]
    uw = uw.reshape(tiles, TILE_Q * T_MAX, TILE_Q)
    return utab, uw


def lex_scores_np(slots_u32: np.ndarray, dl: np.ndarray, qt_m: np.ndarray, w_m: np.ndarray, k1: float, b: float,
                  avgdl: float) -> np.ndarray:
    """``s(m, r)`` of one query over the given rows, fp32 [R] (numpy, the
    contract's order)."""
    R, W = slots_u32.shape
    used = qt_m[qt_m > 0]
    if len(used) == 0 or R == 0:
        return np.zeros(R, dtype=np.float32)
    wu = w_m[: len(used)]
    k1, b, avgdl = float(k1), float(b), float(avgdl)
    t = slots_u32 >> np.uint32(8)
    tf = (slots_u32 & np.uint32(255)).astype(np.float64)
    K = k1 * ((1.0 - b) + b * (dl.astype(np.float64) / avgdl))
    idx = np.minimum(np.searchsorted(used, t), len(used) - 1)
    match = (used[idx] == t) & (slots_u32 != 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        x = (tf * (k1 + 1.0)) / (tf + K[:, None])
    c = np.where(match, wu[idx] * np.where(match, x, 0.0), 0.0)
    s = np.zeros(R, dtype=np.float64)
    for j in range(W):
        s = s + c[:, j]
    return s.astype(np.float32)


def _u32(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def lex_topk_ref(slots: torch.Tensor, dl: torch.Tensor, bias: torch.Tensor, qterms, w, k: int, k1: float = 1.2,
                 b: float = 0.75, avgdl: float = 1.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """numpy formulation of :func:`lex_topk` (tensors of any device are read
    on the host)."""
    qt, wv = _check_terms(qterms, w)
    _check_params(k, k1, b, avgdl)
    _check_cols(slots, dl)
    k = int(k)
    M, n = qt.shape[0], slots.shape[0]
    S, dlv, bv = _u32(slots), dl[:n].cpu().numpy(), bias[:n].detach().cpu().numpy()
    os_ = np.full((M, k), NEG_INF, dtype=np.float32)
    oi = np.full((M, k), -1, dtype=np.int64)
    ok = np.isfinite(bv)
    rows = np.arange(n)
    for m in range(M):
        s = lex_scores_np(S, dlv, qt[m], wv[m], k1, b, avgdl)
        e = rows[ok & (s > 0)]
        o = e[np.lexsort((e, -s[e].astype(np.float64)))][:k]
        os_[m, : len(o)], oi[m, : len(o)] = s[o], o
    dev = slots.device
    return torch.from_numpy(os_).to(dev), torch.from_numpy(oi).to(dev)


def lex_topk(slots: torch.Tensor, dl: torch.Tensor, bias: torch.Tensor, qterms, w, k: int, k1: float = 1.2,
             b: float = 0.75, avgdl: float = 1.0, grid_cap: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """BM25 top-k (lexical.hip lex_scan_kernel + lzk_cand_select_wide):
    ``slots`` int32 [n, W], ``dl`` int32 [n], ``bias`` fp32 [n] on the device;
    ``qterms`` uint32 [M, T <= 32] and ``w`` float64 [M, T] on the host.
    Returns (scores fp32 [M, k], rows int64 [M, k]). ``grid_cap``: the row
    blocks of the scan (0: its own choice; a block strides over the rest).
    Nothing is read back from the device; the tile tables (1 KB + 16 KB per
    tile of 8 queries: 2 MB at M = 1,024) are uploaded from pageable host
    memory on every call, a copy the host waits for."""
    if not slots.is_cuda:
        return lex_topk_ref(slots, dl, bias, qterms, w, k, k1, b, avgdl)
    qt, wv = _check_terms(qterms, w)
    _check_params(k, k1, b, avgdl)
    _check_cols(slots, dl)
    k = int(k)
    dev = slots.device
    M, (n, W) = qt.shape[0], slots.shape
    if M == 0 or n == 0:
        return (torch.full((M, k), NEG_INF, dtype=torch.float32, device=dev),
                torch.full((M, k), -1, dtype=torch.long, device=dev))
    assert slots.is_contiguous() and dl.is_contiguous() and bias.is_contiguous() and bias.shape[0] >= n
    assert bias.dtype == torch.float32
    from .search import cand_select_wide
    utab, uw = tile_tables(qt, wv)
    utab_d = torch.from_numpy(utab.view(np.int32)).to(dev)
    uw_d = torch.from_numpy(uw).to(dev)
    L = _lib.lib()
    nblk = int(L.lzk_lex_scan_blocks(n, M, int(grid_cap)))
    ps = torch.empty((M, nblk * 64), dtype=torch.float32, device=dev)
    pi = torch.empty((M, nblk * 64), dtype=torch.int32, device=dev)
    _lib.check(L.lzk_lex_scan(slots.data_ptr(), dl.data_ptr(), bias.data_ptr(), n, W, utab_d.data_ptr(),
                              uw_d.data_ptr(), M, float(k1), float(b), float(avgdl), nblk, ps.data_ptr(),
                              pi.data_ptr(), _lib.stream_ptr(dev)), "lzk_lex_scan")
    os_, oi, _ = cand_select_wide(None, ps, pi, nblk * 64, k)
    return os_, oi


def _check_fuse(X, Q, dpool, lpool, k, alpha):
    if Q.dim() == 1:
        Q = Q[None, :]
    if lpool.dim() == 1:
        lpool = lpool[None, :]
    if dpool is not None and dpool.dim() == 1:
        dpool = dpool[None, :]
    M, P = lpool.shape
    if not 0.0 <= float(alpha) <= 1.0:
        raise ValueError(f"alpha must be in [0, 1] (got {alpha})")
    if not 1 <= P <= MAX_K or (dpool is not None and tuple(dpool.shape) != (M, P)):
        raise ValueError(f"the pools are [M, P] with P in 1 .. {MAX_K}, of one shape")
    if Q.shape[0] != M or X.dim() != 2 or Q.shape[1] != X.shape[1]:
        raise ValueError(f"shapes do not agree: X {tuple(X.shape)}, Q {tuple(Q.shape)}, pools {tuple(lpool.shape)}")
    return Q, dpool, lpool, M, P


def lex_fuse_ref(X: torch.Tensor, Q: torch.Tensor, dpool: Optional[torch.Tensor], lpool: torch.Tensor,
                 slots: torch.Tensor, dl: torch.Tensor, qterms, w, alpha: float, k: int, k1: float = 1.2,
                 b: float = 0.75, avgdl: float = 1.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """numpy formulation of :func:`lex_fuse`: fp32 cosines and blends."""
    qt, wv = _check_terms(qterms, w)
    _check_params(k, k1, b, avgdl)
    _check_cols(slots, dl)
    Q, dpool, lpool, M, P = _check_fuse(X, Q, dpool, lpool, k, alpha)
    k = int(k)
    n = X.shape[0]
    Xh = X.detach().cpu().numpy().astype(np.float32, copy=False)
    Qh = Q.detach().cpu().to(torch.float32).numpy()
    S, dlv = _u32(slots), dl.cpu().numpy()
    den = lexn_den(wv, k1)
    a = np.float32(alpha)
    os_ = np.full((M, k), NEG_INF, dtype=np.float32)
    oi = np.full((M, k), -1, dtype=np.int64)
    pools = lpool.cpu().numpy() if dpool is None else np.concatenate([dpool.cpu().numpy(), lpool.cpu().numpy()], 1)
    for m in range(M):
        c = np.unique(pools[m][(pools[m] >= 0) & (pools[m] < n)])
        if len(c) == 0:
            continue
        xc, q = Xh[c], Qh[m]
        qn, xn = np.sqrt(np.float32(q @ q)), np.sqrt(np.einsum("cd,cd->c", xc, xc)).astype(np.float32)
        okn = (qn > 0) & (xn > 0)
        cos = np.where(okn, (xc @ q) / np.where(okn, qn * xn, np.float32(1)), np.float32(0)).astype(np.float32)
        s = lex_scores_np(S[c], dlv[c], qt[m], wv[m], k1, b, avgdl)
        lexn = s / den[m] if den[m] > 0 else np.zeros_like(s)
        blend = ((np.float32(1) - a) * cos + a * lexn).astype(np.float32)
        o = np.lexsort((c, -blend.astype(np.float64)))[:k]
        os_[m, : len(o)], oi[m, : len(o)] = blend[o], c[o]
    dev = X.device
    return torch.from_numpy(os_).to(dev), torch.from_numpy(oi).to(dev)


def lex_fuse(X: torch.Tensor, Q: torch.Tensor, dpool: Optional[torch.Tensor], lpool: torch.Tensor,
             slots: torch.Tensor, dl: torch.Tensor, qterms, w, alpha: float, k: int, k1: float = 1.2,
             b: float = 0.75, avgdl: float = 1.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """The fusion (lexical.hip lex_fuse_kernel, one block per query): fp32
    rows ``X`` [n, D] (any row stride), fp32 queries ``Q`` [M, D], ``dpool``
    (or None: no dense pool) and ``lpool`` int64 [M, P <= 64] of graph rows,
    the lexical columns, the queries' terms and weights (host), 1 <= k <= 64.
    Returns (blend fp32 [M, k], rows int64 [M, k]). Nothing is read back
    from the device; the queries' terms, weights and ``den`` (388 bytes a
    query) are uploaded from pageable host memory on every call."""
    if not X.is_cuda:
        return lex_fuse_ref(X, Q, dpool, lpool, slots, dl, qterms, w, alpha, k, k1, b, avgdl)
    qt, wv = _check_terms(qterms, w)
    _check_params(k, k1, b, avgdl)
    _check_cols(slots, dl)
    Q, dpool, lpool, M, P = _check_fuse(X, Q, dpool, lpool, k, alpha)
    k = int(k)
    dev = X.device
    assert X.dtype == torch.float32 and X.stride(1) == 1 and slots.is_contiguous() and dl.is_contiguous()
    assert slots.shape[0] >= X.shape[0] and dl.shape[0] >= X.shape[0]
    D = X.shape[1]
    os_ = torch.empty((M, k), dtype=torch.float32, device=dev)
    oi = torch.empty((M, k), dtype=torch.long, device=dev)
    if M == 0:
        return os_, oi
    Qc = Q.to(dev, torch.float32)
    if Qc.stride(1) != 1:
        Qc = Qc.contiguous()
    lp = lpool.to(dev, torch.long).contiguous()
    dp = None if dpool is None else dpool.to(dev, torch.long).contiguous()
    qt_d = torch.from_numpy(np.where(qt == 0, np.uint32(PAD_TERM), qt).view(np.int32)).to(dev)
    w_d = torch.from_numpy(wv).to(dev)
    den_d = torch.from_numpy(lexn_den(wv, k1)).to(dev)
    L = _lib.lib()
    _lib.check(L.lzk_lex_fuse(X.data_ptr(), X.stride(0) if X.shape[0] > 1 else max(X.stride(0), D), X.shape[0],
                              Qc.data_ptr(), Qc.stride(0) if M > 1 else max(Qc.stride(0), D), M, D, _lib.ptr(dp),
                              lp.data_ptr(), P, slots.data_ptr(), dl.data_ptr(), slots.shape[1], qt_d.data_ptr(),
                              w_d.data_ptr(), den_d.data_ptr(), float(k1), float(b), float(avgdl), float(alpha), k,
                              os_.data_ptr(), oi.data_ptr(), _lib.stream_ptr(dev)), "lzk_lex_fuse")
    return os_, oi
