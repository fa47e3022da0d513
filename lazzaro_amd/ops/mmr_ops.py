"""Diversity-aware selection over a search's candidate pool: greedy
maximal-marginal-relevance picks (csrc/kernels/mmr.hip), with the torch
formulation.

Per query ``q`` and pool ``cand`` (graph rows, -1 or out of range = empty),
step t = 0 .. k-1 picks, among the slots not picked yet, the argmax of

    obj_t(c) = (1 - diversity) * cos(q, c) - diversity * max_{s in S_t} cos(c, s)

(the max is 0 while nothing is picked), ties to the lower graph row. Cosines
are over the fp32 rows and the fp32 query, 0 when either norm is 0.

Device tensors always take the kernel; CPU tensors take ``mmr_select_ref``
(the CPU tier, and a second formulation the tests hold to the same oracle).
"""
from __future__ import annotations

from typing import Tuple

import torch

from . import _lib
from ._dot16 import cos_or_zero
from ._dot16 import sum_depth as MMR_SUM_DEPTH  # L(D) of mmr.hip's 'Summation order' (csrc/include/lzk_dot16.h)

NEG_INF = float("-inf")
MAX_FETCH_K = 64  # mmr.hip MMR_MAX_F: one pool slot per lane of the selecting wave


def mmr_tol(D: int) -> float:
    """|cos32 - cos64| and |obj32 - obj64| of the kernel: L for the dot, L
    jointly for the two norms, 8 units for sqrt, multiply, divide and the
    objective's own roundings."""
    return (2 * MMR_SUM_DEPTH(D) + 8) * 2.0 ** -24


def pool_size(k: int, diversity, fetch_k=None) -> int:
    """The pool a diverse search of ``k`` results selects from: ``fetch_k``,
    by default ``max(16, 2 k)`` -- 16 candidate slots are what the scan
    kernels keep, so ``k <= 8`` leaves the pool search on its fast routes.
    Raises ValueError for arguments the selection does not take."""
    if diversity is None:
        raise ValueError("fetch_k only applies to a diverse search: pass diversity= as well")
    if not 0.0 <= float(diversity) <= 1.0:
        raise ValueError(f"diversity must be in [0, 1] (got {diversity})")
    k = int(k)
    F = max(16, 2 * k) if fetch_k is None else int(fetch_k)
    if fetch_k is None and k <= MAX_FETCH_K:
        F = min(F, MAX_FETCH_K)
    if F > MAX_FETCH_K:
        raise ValueError(f"a diverse search selects from at most {MAX_FETCH_K} candidates (fetch_k={F})")
    if not 1 <= k <= F:
        raise ValueError(f"limit must be in 1 .. fetch_k={F} (got {k})")
    return F


_lib.register("lzk_mmr_select", _lib.I, [_lib.P, _lib.L, _lib.L, _lib.P, _lib.L, _lib.I, _lib.I, _lib.P, _lib.I,
                                         _lib.I, _lib.F, _lib.P, _lib.P, _lib.P])


def _check(X, Q, cand, k, diversity):
    if Q.dim() == 1:
        Q = Q[None, :]
    if cand.dim() == 1:
        cand = cand[None, :]
    M, F = cand.shape
    if not 0.0 <= float(diversity) <= 1.0:
        raise ValueError(f"diversity must be in [0, 1] (got {diversity})")
    if not 1 <= F <= MAX_FETCH_K:
        raise ValueError(f"the pool holds 1 .. {MAX_FETCH_K} candidates per query (got {F})")
    if not 1 <= int(k) <= F:
        raise ValueError(f"k must be in 1 .. the pool size {F} (got {k})")
    if Q.shape[0] != M or X.dim() != 2 or Q.shape[1] != X.shape[1]:
        raise ValueError(f"shapes do not agree: X {tuple(X.shape)}, Q {tuple(Q.shape)}, cand {tuple(cand.shape)}")
    return Q, cand, M, F


def mmr_select_ref(X: torch.Tensor, Q: torch.Tensor, cand: torch.Tensor, k: int, diversity: float,
                   chunk: int = 128) -> Tuple[torch.Tensor, torch.Tensor]:
    """Torch formulation of :func:`mmr_select` (any device), fp32 throughout:
    one [F, F] cosine matrix per query, then k masked argmax steps."""
    Q, cand, M, F = _check(X, Q, cand, k, diversity)
    k = int(k)
    dev = X.device
    n = X.shape[0]
    BIG = 1 << 62
    delta = torch.tensor(float(diversity), dtype=torch.float32, device=dev)
    w = torch.tensor(1.0, dtype=torch.float32, device=dev) - delta
    pick = torch.full((M, k), -1, dtype=torch.int32, device=dev)
    obj = torch.full((M, k), NEG_INF, dtype=torch.float32, device=dev)
    if n == 0:
        return pick, obj
    for m0 in range(0, M, chunk):
        c = cand[m0:m0 + chunk].to(dev).long()
        q = Q[m0:m0 + chunk].to(dev, torch.float32)
        mm = c.shape[0]
        ar = torch.arange(mm, device=dev)
        alive = (c >= 0) & (c < n)
        key = torch.where(alive, c, torch.full_like(c, BIG))
        Xc = X[c.clamp(0, n - 1)].to(torch.float32)             # [mm, F, D]
        nrm = Xc.norm(dim=2)
        rel = cos_or_zero(torch.einsum("md,mfd->mf", q, Xc), q.norm(dim=1)[:, None].expand(-1, F), nrm)
        sim = cos_or_zero(torch.bmm(Xc, Xc.transpose(1, 2)), nrm[:, :, None].expand(-1, -1, F),
                          nrm[:, None, :].expand(-1, F, -1))
        mx = torch.full((mm, F), NEG_INF, dtype=torch.float32, device=dev)
        for t in range(k):
            red = torch.zeros_like(mx) if t == 0 else mx
            o = torch.where(alive, w * rel - delta * torch.where(alive, red, torch.zeros_like(red)),
                            torch.full_like(rel, NEG_INF))
            best = o.max(dim=1).values
            has = alive.any(dim=1)
            # the lowest row among the slots that reach the maximum
            slot = torch.where(alive & (o == best[:, None]), key, torch.full_like(key, BIG)).argmin(dim=1)
            pick[m0:m0 + mm, t] = torch.where(has, slot, torch.full_like(slot, -1)).to(torch.int32)
            obj[m0:m0 + mm, t] = torch.where(has, best, torch.full_like(best, NEG_INF))
            alive[ar[has], slot[has]] = False
            mx = torch.where(has[:, None], torch.maximum(mx, sim[ar, :, slot]), mx)
    return pick, obj


def mmr_select(X: torch.Tensor, Q: torch.Tensor, cand: torch.Tensor, k: int,
               diversity: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """Greedy MMR picks (mmr.hip lzk_mmr_select): fp32 rows ``X`` [n, D]
    (any row stride), fp32 queries ``Q`` [M, D], pools ``cand`` int64 [M, F]
    of graph rows with F <= 64 (< 0 or >= n: an empty slot, never read),
    1 <= k <= F, 0 <= diversity <= 1. Returns (pick int32 [M, k]: the pool
    SLOT of each pick, in pick order, -1 once the pool ran out; obj fp32
    [M, k]: the objective at each pick, -inf for padding). No host
    synchronisation."""
    if not X.is_cuda:
        return mmr_select_ref(X, Q, cand, k, diversity)
    Q, cand, M, F = _check(X, Q, cand, k, diversity)
    k = int(k)
    dev = X.device
    assert X.dtype == torch.float32 and X.stride(1) == 1
    D = X.shape[1]
    Qc = Q.to(dev, torch.float32)
    if Qc.stride(1) != 1:
        Qc = Qc.contiguous()
    cc = cand.to(dev, torch.long).contiguous()
    pick = torch.empty((M, k), dtype=torch.int32, device=dev)
    obj = torch.empty((M, k), dtype=torch.float32, device=dev)
    if M == 0:
        return pick, obj
    L = _lib.lib()
    _lib.check(L.lzk_mmr_select(X.data_ptr(), X.stride(0) if X.shape[0] > 1 else max(X.stride(0), D), X.shape[0],
                                Qc.data_ptr(), Qc.stride(0) if M > 1 else max(Qc.stride(0), D), M, D, cc.data_ptr(),
                                F, k, float(diversity), pick.data_ptr(), obj.data_ptr(), _lib.stream_ptr(dev)),
               "lzk_mmr_select")
    return pick, obj
