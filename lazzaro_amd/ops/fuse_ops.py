"""Multi-query search: the pools of a group of sub-queries fused into one
ranked list (csrc/kernels/fuse.hip), with the torch formulation.

The contract. A call carries ``M`` queries cut into ``NG`` groups by
``offsets`` (int64, ``NG + 1`` entries, ascending from 0 to ``M``); group ``g``
is queries ``offsets[g] .. offsets[g + 1] - 1``, 1 .. ``MAX_FUSE_Q`` = 16 of
them. ``pools`` int64 [M, P] (P <= 64) holds each sub-query's pool, graph rows
in rank order; a slot ``< 0`` or ``>= n`` is empty.

* ``rank_j(v)`` is 1 plus the number of non-empty slots before the FIRST
  occurrence of ``v`` in pool ``j``. A later occurrence of the same row is
  ignored for the score but still counts as a slot before the slots after it.
* The candidates are the union of the group's pools (at most 16 x 64 = 1,024
  rows); ``support(v)`` is the number of the group's pools that hold ``v``.
* ``mode="rrf"``: ``score(v) = (float)(sum, in sub-query order over the pools
  that hold v, of (double)w_j / ((double)rrf_k + rank_j(v)))`` -- plain IEEE
  fp64, nothing contracted, rounded once; ``w_j`` an fp32 weight (``>= 0``,
  finite, default 1), ``rrf_k`` fp32 ``> 0``. Rank-only: rows and queries are
  not read. The kernel, :func:`fuse_select_ref` and the tests' oracle agree
  bit for bit.
* ``mode="mean"``: ``score(v) = sum_j wn_j * cos(q_j, v)`` over ALL sub-queries
  of the group, whether or not ``v`` was in that pool (a pool decides
  candidacy, not score). ``wn_j = (float)(w_j / sum w)``, the sum and the
  quotient in fp64 on the host, the sum in sub-query order over the fp32
  weights; a group whose weights sum to 0 raises ValueError. ``cos`` is over
  the fp32 rows and the fp32 query, 0 when either norm is 0; the sum is an
  fp32 ``fmaf`` chain in sub-query order from 0. :func:`fuse_tol` bounds its
  distance from fp64.
* The ``k`` (1 .. 64) largest by the fp32 score come back descending, ties to
  the lower row; beyond the candidate count the padding is ``(-inf, -1,
  support 0)``. A group of one sub-query under ``rrf`` returns its pool in
  pool order (without repeats and holes).

Device tensors always take the kernel; CPU tensors take
:func:`fuse_select_ref` (the CPU tier, and a second formulation the tests hold
to the same oracle).
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._dot16 import cos_or_zero
from ._dot16 import sum_depth as FUSE_SUM_DEPTH  # fuse.hip uses mmr.hip's dot layout (csrc/include/lzk_dot16.h)
from ..core.fuse import MAX_FUSE_Q, MAX_LIMIT, MAX_POOL, QueryFusion

NEG_INF = float("-inf")
MAX_QUERY_FLOATS = 16384  # fuse.hip FUSE_MAX_QF: a group's staged queries, 64 KiB of LDS


def fuse_tol(D: int, G: int) -> float:
    """|score32 - score64| of ``mode="mean"`` for a group of ``G`` sub-queries
    (derived in fuse.hip's header): 2 L(D) + 8 units of 2^-24 for a cosine (as
    ``mmr_tol``: L for the dot, L jointly for the norms, 8 for sqrt, multiply,
    divide) -- the weights are >= 0 and sum to 1, so the cosines' errors do
    not add beyond the largest --, one per ``fmaf`` of the chain, G in all,
    and 2 of slack for the second-order terms. The fp64 score takes the same
    fp32 weights ``wn_j``."""
    return (2 * FUSE_SUM_DEPTH(int(D)) + 8 + int(G) + 2) * 2.0 ** -24


def group_sizes(offsets, M: Optional[int] = None) -> List[int]:
    """The sizes of the groups ``offsets`` cuts (a sequence, an array or a
    CPU tensor). Raises ValueError unless they ascend from 0 (to ``M``)."""
    if torch.is_tensor(offsets):
        offsets = offsets.cpu().tolist()
    off = [int(o) for o in np.asarray(offsets).reshape(-1).tolist()]
    if len(off) < 1 or off[0] != 0 or any(b < a for a, b in zip(off, off[1:])):
        raise ValueError(f"offsets must ascend from 0 (got {off[:8]}{'...' if len(off) > 8 else ''})")
    if M is not None and off[-1] != M:
        raise ValueError(f"offsets end at {off[-1]} but there are {M} queries")
    return [b - a for a, b in zip(off, off[1:])]


def normalised_weights(w32: np.ndarray, sizes: Sequence[int]) -> np.ndarray:
    """``wn_j = (float)(w_j / sum w)`` per group: the fp32 weights summed in
    sub-query order and divided in fp64, rounded once."""
    out = np.empty(len(w32), dtype=np.float32)
    a = 0
    for n in sizes:
        ws = [float(x) for x in w32[a:a + n]]
        tot = 0.0
        for x in ws:
            tot += x
        if not tot > 0.0:
            raise ValueError("the weights of a group sum to 0: a mean needs a positive weight")
        out[a:a + n] = [np.float32(x / tot) for x in ws]
        a += n
    return out


_lib.register("lzk_fuse_select", _lib.I,
              [_lib.P, _lib.L, _lib.L, _lib.P, _lib.L, _lib.I, _lib.I,      # X ldx n Q ldq M D
               _lib.P, _lib.I, _lib.I, _lib.P, _lib.I, _lib.P,              # off NG gmax pools P w
               _lib.I, _lib.F, _lib.I,                                      # mode rrf_k k
               _lib.P, _lib.P, _lib.P, _lib.P, _lib.P])                     # rows scores support ncand stream


def _check(X, Q, offsets, pools, k, fusion, weights):
    fu = QueryFusion.coerce(fusion)
    if fu is None:
        raise ValueError("fuse settings are required")
    if pools.dim() != 2:
        raise ValueError(f"pools must be [M, P] (got {tuple(pools.shape)})")
    M, P = pools.shape
    if not 1 <= P <= MAX_POOL:
        raise ValueError(f"a pool holds 1 .. {MAX_POOL} slots (got {P})")
    sizes = group_sizes(offsets, M)
    k = int(k) if not isinstance(k, bool) and isinstance(k, (int, np.integer)) else k
    fu.check(k, sizes)
    if weights is None:
        flat = fu.group_weights(sizes)
    else:
        if torch.is_tensor(weights):
            weights = weights.cpu().tolist()
        flat = [float(x) for x in np.asarray(weights, dtype=np.float64).reshape(-1).tolist()]
        if len(flat) != M:
            raise ValueError(f"{len(flat)} weights for {M} sub-queries")
        if not all(x >= 0.0 and math.isfinite(x) for x in flat):
            raise ValueError("weights must be finite and >= 0")
    w32 = np.asarray(flat, dtype=np.float32)
    if fu.mode == "mean":
        if X is None or Q is None:
            raise ValueError("mode='mean' needs the rows X and the queries Q")
        if Q.dim() == 1:
            Q = Q[None, :]
        if X.dim() != 2 or Q.dim() != 2 or Q.shape[0] != M or Q.shape[1] != X.shape[1]:
            raise ValueError(f"shapes do not agree: X {tuple(X.shape)}, Q {tuple(Q.shape)}, pools {tuple(pools.shape)}")
        w32 = normalised_weights(w32, sizes)
    return fu, Q, sizes, w32, M, P, k


def fuse_select_ref(X, Q, offsets, pools, k, fusion="rrf", weights=None, n: Optional[int] = None):
    """Torch formulation of :func:`fuse_select` (any device). Per group the
    union is the sorted unique rows, the first occurrences come from an
    all-pairs comparison inside each pool, the ranks from a prefix sum over
    the non-empty slots; ``rrf`` sums in fp64 column by column, ``mean`` in
    fp32. ``rrf`` ignores ``X`` and ``Q`` (``n``: the row count then, default
    ``X.shape[0]``)."""
    fu, Q, sizes, w32, M, P, k = _check(X, Q, offsets, pools, k, fusion, weights)
    dev = pools.device
    n = int(X.shape[0] if n is None else n)
    NG = len(sizes)
    orow = torch.full((NG, k), -1, dtype=torch.long, device=dev)
    oscore = torch.full((NG, k), NEG_INF, dtype=torch.float32, device=dev)
    osup = torch.zeros((NG, k), dtype=torch.int32, device=dev)
    ncand = torch.zeros(NG, dtype=torch.int32, device=dev)
    w = torch.from_numpy(w32).to(dev)
    kk = torch.tensor(float(np.float32(fu.rrf_k)), dtype=torch.float64, device=dev)
    earlier = torch.tril(torch.ones((P, P), dtype=torch.bool, device=dev), -1)  # [s, s'] : s' < s
    pools = pools.to(torch.long)
    a = 0
    for g, G in enumerate(sizes):
        p = pools[a:a + G]
        valid = (p >= 0) & (p < n)
        if not bool(valid.any()):
            a += G
            continue
        seen = torch.cumsum(valid.long(), 1)                                   # the rank of a non-empty slot
        same = (p[:, :, None] == p[:, None, :]) & valid[:, None, :] & earlier  # an equal non-empty slot before it
        first = valid & ~same.any(2)
        U = torch.unique(p[valid])  # (sorted)
        C = U.numel()
        R = torch.zeros((C, G), dtype=torch.long, device=dev)
        jj = torch.arange(G, device=dev)[:, None].expand(G, P)
        R[torch.searchsorted(U, p[first]), jj[first]] = seen[first]
        if fu.mode == "rrf":
            acc = torch.zeros(C, dtype=torch.float64, device=dev)
            for j in range(G):
                r = R[:, j]
                acc = torch.where(r > 0, acc + w[a + j].double() / (kk + r.double()), acc)
            score = acc.float()
        else:
            x = X[U].to(torch.float32)
            xn = x.norm(dim=1)
            score = torch.zeros(C, dtype=torch.float32, device=dev)
            for j in range(G):
                q = Q[a + j].to(dev, torch.float32)
                score = score + w[a + j] * cos_or_zero(x @ q, xn, q.norm().expand(C))
        o = torch.sort(score, descending=True, stable=True).indices[:k]  # (rows ascend: ties to the lower row)
        c = o.numel()
        orow[g, :c], oscore[g, :c], osup[g, :c] = U[o], score[o], (R[o] > 0).sum(1).int()
        ncand[g] = C
        a += G
    return orow, oscore, osup, ncand


def fuse_select(X: Optional[torch.Tensor], Q: Optional[torch.Tensor], offsets, pools: torch.Tensor, k: int,
                fusion="rrf", weights=None, n: Optional[int] = None
                ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Fusion of the groups' pools (fuse.hip lzk_fuse_select; the contract is
    in the module docstring): fp32 rows ``X`` [n, D] (any row stride) and fp32
    queries ``Q`` [M, D] -- read by ``mode="mean"`` only; ``rrf`` takes None
    for both with ``n`` the row count --, ``offsets`` the groups' bounds on
    the host, ``pools`` int64 [M, P], ``fusion`` anything
    ``QueryFusion.coerce`` takes, ``weights`` one per sub-query, flat [M]
    (default: the fusion's per-position weights, else 1). Returns (rows int64
    [NG, k], scores fp32 [NG, k], support int32 [NG, k], ncand int32 [NG]).
    The offsets and weights go up from pinned host memory by asynchronous
    copies and nothing is read back: no host synchronisation."""
    if not pools.is_cuda:
        return fuse_select_ref(X, Q, offsets, pools, k, fusion, weights, n)
    fu, Q, sizes, w32, M, P, k = _check(X, Q, offsets, pools, k, fusion, weights)
    dev = pools.device
    NG = len(sizes)
    mean = fu.mode == "mean"
    D = int(X.shape[1]) if mean else 0
    n = int(X.shape[0] if n is None else n)
    gmax = max(sizes) if sizes else 1
    if mean and gmax * ((D + 3) // 4 * 4) > MAX_QUERY_FLOATS:
        raise ValueError(f"mode='mean' stages a group's queries on chip: {gmax} sub-queries of {D} dimensions exceed "
                         f"{MAX_QUERY_FLOATS} floats (16 sub-queries up to 1,024 dimensions, 8 up to 2,048)")
    if NG == 0:
        return (torch.empty((0, k), dtype=torch.long, device=dev), torch.empty((0, k), dtype=torch.float32, device=dev),
                torch.empty((0, k), dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.int32, device=dev))
    # pinned staging and an asynchronous copy (as filter_ops): the host does not wait for the pool search
    off = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.long).pin_memory().to(dev, non_blocking=True)
    w = torch.from_numpy(w32).pin_memory().to(dev, non_blocking=True)
    Qc = None
    if mean:
        assert X.is_cuda and X.dtype == torch.float32 and X.stride(1) == 1
        Qc = Q.to(dev, torch.float32)
        if Qc.stride(1) != 1:
            Qc = Qc.contiguous()
    return launch(X if mean else None, Qc, off, gmax, pools.to(torch.long).contiguous(), w, fu, k, n)


def launch(X, Qc, off, gmax: int, pools, w, fu: QueryFusion, k: int, n: int):
    """The kernel launch of :func:`fuse_select` over device tensors it has
    validated (``off`` int64 [NG + 1], ``pools`` int64 [M, P] contiguous, ``w``
    fp32 [M] -- normalised per group for ``mean`` --, ``gmax`` the largest
    group); the benchmark times this alone."""
    dev = pools.device
    M, P = pools.shape
    NG = off.numel() - 1
    mean = fu.mode == "mean"
    rows = torch.empty((NG, k), dtype=torch.long, device=dev)
    scores = torch.empty((NG, k), dtype=torch.float32, device=dev)
    support = torch.empty((NG, k), dtype=torch.int32, device=dev)
    ncand = torch.empty(NG, dtype=torch.int32, device=dev)
    xp = xs = qp = qs = D = 0
    if mean:
        D = int(X.shape[1])
        xp, xs = X.data_ptr(), X.stride(0) if n > 1 else max(X.stride(0), D)
        qp, qs = Qc.data_ptr(), Qc.stride(0) if M > 1 else max(Qc.stride(0), D)
    L = _lib.lib()
    _lib.check(L.lzk_fuse_select(xp, xs, n, qp, qs, M, D, off.data_ptr(), NG, gmax, pools.data_ptr(), P, w.data_ptr(),
                                 1 if mean else 0, float(np.float32(fu.rrf_k)), k, rows.data_ptr(), scores.data_ptr(),
                                 support.data_ptr(), ncand.data_ptr(), _lib.stream_ptr(dev)), "lzk_fuse_select")
    return rows, scores, support, ncand
