"""Filtered store search: the predicate plan and the indexed scan
(csrc/kernels/filter.hip), with their torch formulations.

``filter_plan`` evaluates a :class:`Predicate` -- a ``MemoryFilter`` resolved
against one tenant: type / shard CODES, excluded ROWS -- over the tenant's
node columns and returns ``(bias, rows, count)``: the store bias of the
metric where a row passes and -inf where it does not, the passing rows in
ascending order, and their number. ``gather_topk`` scans only listed rows.

Device tensors always take the kernels; CPU tensors take ``filter_plan_ref``
/ ``gather_topk_ref`` (the CPU tier, and what the GPU tests compare against).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .search import TARGET_WGS, _merge_groups, _ws

NEG_INF = float("-inf")
NODE = 1  # (engine.tenant_graph NODE: the kind of a graph node)

FB_TYPES, FB_SHARDS, FB_MIN_SAL, FB_MAX_SAL, FB_SINCE, FB_UNTIL, FB_ACC_SINCE, FB_MIN_ACC, FB_EXCLUDE = (
    1 << i for i in range(9))

# the columns a plan reads, in the order of the kernel's pointer table
PLAN_COLS = ("sal", "acc", "last", "ts", "shard", "kind", "sup", "stored")


class FilterBounds(C.Structure):
    """The predicate's scalar bounds, passed to the kernel by value
    (filter.hip LzkFilterBounds)."""
    _fields_ = [("since", C.c_double), ("until", C.c_double), ("accessed_since", C.c_double),
                ("min_sal", C.c_float), ("max_sal", C.c_float), ("min_acc", C.c_int), ("sup_mode", C.c_int),
                ("flags", C.c_int), ("n_shard_bits", C.c_int), ("neg_shard_pass", C.c_int), ("l2", C.c_int),
                ("type_mask", C.c_uint * 8)]


_lib.register("lzk_tg_filter_plan_ws", _lib.L, [_lib.L])
_lib.register("lzk_tg_filter_plan", _lib.I, [_lib.P, FilterBounds, _lib.P, _lib.L, _lib.P, _lib.P, _lib.L, _lib.P,
                                             _lib.P, _lib.P])
_lib.register("lzk_gather_topk_chunks", _lib.I, [_lib.I, _lib.I, _lib.I, _lib.I])
_lib.register("lzk_gather_topk_partial", _lib.I, [_lib.P, _lib.L, _lib.I, _lib.P, _lib.I, _lib.P, _lib.L, _lib.I,
                                                  _lib.P, _lib.F, _lib.I, _lib.I, _lib.I, _lib.P, _lib.P, _lib.P])


@dataclass
class Predicate:
    """A ``MemoryFilter`` resolved against one tenant. ``None`` = no test.
    Every predicate also requires ``kind == NODE`` and ``stored == 1``."""
    type_codes: Optional[Sequence[int]] = None   # passing type codes (0..255)
    shard_codes: Optional[Sequence[int]] = None  # passing shard codes (>= 0)
    neg_shard_pass: bool = False                 # rows with shard code < 0 pass the shard test
    min_sal: Optional[float] = None
    max_sal: Optional[float] = None
    since: Optional[float] = None
    until: Optional[float] = None
    accessed_since: Optional[float] = None
    min_acc: Optional[int] = None
    sup_mode: int = -1                           # -1 both, 0 no super-nodes, 1 only super-nodes
    exclude_rows: Optional[Sequence[int]] = None

    def flags(self) -> int:
        f = 0
        for bit, v in ((FB_TYPES, self.type_codes), (FB_SHARDS, self.shard_codes), (FB_MIN_SAL, self.min_sal),
                       (FB_MAX_SAL, self.max_sal), (FB_SINCE, self.since), (FB_UNTIL, self.until),
                       (FB_ACC_SINCE, self.accessed_since), (FB_MIN_ACC, self.min_acc),
                       (FB_EXCLUDE, self.exclude_rows)):
            if v is not None:
                f |= bit
        return f


def _bitmap(bits: Sequence[int], nbits: int) -> np.ndarray:
    """uint32 words with the given bits set (bit b of word b >> 5)."""
    w = np.zeros(max(1, (nbits + 31) // 32), dtype=np.uint32)
    b = np.asarray(list(bits), dtype=np.int64)
    b = b[(b >= 0) & (b < nbits)]
    if b.size:
        np.bitwise_or.at(w, b >> 5, (np.uint32(1) << (b & 31).astype(np.uint32)))
    return w


def _to_dev(a: np.ndarray, dev) -> torch.Tensor:
    t = torch.from_numpy(a.view(np.int32))
    if torch.device(dev).type == "cuda":
        return t.pin_memory().to(dev, non_blocking=True)
    return t


def filter_plan_ref(cols: Dict[str, torch.Tensor], pred: Predicate, sqn: Optional[torch.Tensor], n: int,
                    l2: bool, tcode: Optional[torch.Tensor] = None):
    """Torch formulation of :func:`filter_plan` (any device): the predicate
    by tensor ops, ``torch.where`` for the bias, ``torch.nonzero`` for the
    rows. Returns (bias fp32 [n], rows int32 [count], count int32 [1])."""
    dev = cols["kind"].device
    p = (cols["kind"][:n] == NODE) & (cols["stored"][:n] == 1)
    if pred.sup_mode >= 0:
        p &= (cols["sup"][:n] != 0) == bool(pred.sup_mode)
    if pred.type_codes is not None:
        tab = torch.zeros(256, dtype=torch.bool)
        if len(pred.type_codes):
            tab[torch.as_tensor(sorted(pred.type_codes), dtype=torch.long)] = True
        p &= tab.to(dev)[tcode[:n].long()]
    if pred.shard_codes is not None:
        sh = cols["shard"][:n].long()
        nb = max([int(c) + 1 for c in pred.shard_codes], default=0)
        tab = torch.zeros(nb + 1, dtype=torch.bool)  # (the last entry: codes past the set)
        if len(pred.shard_codes):
            tab[torch.as_tensor(sorted(pred.shard_codes), dtype=torch.long)] = True
        ok = tab.to(dev)[sh.clamp(0, nb)]
        p &= torch.where(sh < 0, torch.full_like(ok, bool(pred.neg_shard_pass)), ok)
    if pred.min_sal is not None:
        p &= cols["sal"][:n] >= torch.tensor(pred.min_sal, dtype=torch.float32)
    if pred.max_sal is not None:
        p &= cols["sal"][:n] <= torch.tensor(pred.max_sal, dtype=torch.float32)
    if pred.since is not None:
        p &= cols["ts"][:n] >= float(pred.since)
    if pred.until is not None:
        p &= cols["ts"][:n] < float(pred.until)
    if pred.accessed_since is not None:
        p &= cols["last"][:n] >= float(pred.accessed_since)
    if pred.min_acc is not None:
        p &= cols["acc"][:n] >= int(pred.min_acc)
    if pred.exclude_rows is not None and len(pred.exclude_rows):
        ex = torch.as_tensor([r for r in pred.exclude_rows if 0 <= r < n], dtype=torch.long)
        hit = torch.zeros(n, dtype=torch.bool, device=dev)
        hit[ex.to(dev)] = True
        p &= ~hit
    ok = torch.zeros(n, dtype=torch.float32, device=dev)
    if l2:
        ok = ok - sqn[:n]
    bias = torch.where(p, ok, torch.full_like(ok, NEG_INF)).contiguous()
    rows = torch.nonzero(p).flatten().to(torch.int32)
    return bias, rows, torch.tensor([rows.numel()], dtype=torch.int32, device=dev)


def filter_plan(cols: Dict[str, torch.Tensor], pred: Predicate, sqn: Optional[torch.Tensor], n: int, l2: bool,
                tcode: Optional[torch.Tensor] = None):
    """The plan of ``pred`` over rows [0, n) (filter.hip lzk_tg_filter_plan):
    (bias fp32 [n], rows int32 [n] of which the first ``count`` are the
    passing rows in ascending order, count int32 [1] on the device). No host
    synchronisation here: the caller reads ``count`` back."""
    dev = cols["kind"].device
    if dev.type != "cuda":
        return filter_plan_ref(cols, pred, sqn, n, l2, tcode)
    n = int(n)
    b = FilterBounds()
    b.flags = pred.flags()
    b.since = float(pred.since or 0.0)
    b.until = float(pred.until or 0.0)
    b.accessed_since = float(pred.accessed_since or 0.0)
    b.min_sal = float(pred.min_sal or 0.0)
    b.max_sal = float(pred.max_sal or 0.0)
    b.min_acc = int(pred.min_acc or 0)
    b.sup_mode = int(pred.sup_mode)
    b.neg_shard_pass = int(bool(pred.neg_shard_pass))
    b.l2 = int(bool(l2))
    shard_bits = excl_bits = None
    if pred.type_codes is not None:
        assert tcode is not None and tcode.dtype == torch.uint8 and tcode.numel() >= n
        for w, v in enumerate(_bitmap(pred.type_codes, 256).tolist()):
            b.type_mask[w] = v
    if pred.shard_codes is not None:
        nb = max([int(c) + 1 for c in pred.shard_codes], default=0)
        b.n_shard_bits = nb
        shard_bits = _to_dev(_bitmap(pred.shard_codes, nb), dev)
    if pred.exclude_rows is not None:
        excl_bits = _to_dev(_bitmap(pred.exclude_rows, n), dev)
        assert excl_bits.numel() * 32 >= n
    for name in PLAN_COLS:
        assert cols[name].numel() >= n and cols[name].is_contiguous()
    assert sqn is None or (sqn.dtype == torch.float32 and sqn.numel() >= n)
    L = _lib.lib()
    bias = torch.empty(n, dtype=torch.float32, device=dev)
    rows = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    ws = torch.empty(int(L.lzk_tg_filter_plan_ws(n)), dtype=torch.int32, device=dev)
    table = (C.c_void_p * 11)(*[cols[c].data_ptr() for c in PLAN_COLS], _lib.ptr(tcode), _lib.ptr(shard_bits),
                              _lib.ptr(excl_bits))
    _lib.check(L.lzk_tg_filter_plan(C.cast(table, C.c_void_p), b, _lib.ptr(sqn), n, bias.data_ptr(), rows.data_ptr(),
                                    int(rows.numel()), count.data_ptr(), ws.data_ptr(), _lib.stream_ptr(dev)),
               "lzk_tg_filter_plan")
    return bias, rows, count


def _pad(s: torch.Tensor, r: torch.Tensor, k: int):
    nq, have = s.shape
    if have < k:
        s = torch.cat([s, torch.full((nq, k - have), NEG_INF, dtype=s.dtype, device=s.device)], 1)
        r = torch.cat([r, torch.full((nq, k - have), -1, dtype=r.dtype, device=r.device)], 1)
    return s, r


def gather_topk_ref(X: torch.Tensor, rows: torch.Tensor, count: int, Q: torch.Tensor, k: int, bias: torch.Tensor,
                    alpha: float = 1.0, chunk: int = 1 << 16) -> Tuple[torch.Tensor, torch.Tensor]:
    """Torch formulation of :func:`gather_topk`: fp32 scores of the listed
    rows, top-k by (score desc, row asc)."""
    nq = Q.shape[0]
    dev = X.device
    best_s = torch.full((nq, 0), NEG_INF, device=dev)
    best_i = torch.zeros((nq, 0), dtype=torch.long, device=dev)
    Qf = Q.float()
    lst = rows[:count].long()
    for c0 in range(0, count, chunk):
        r = lst[c0:c0 + chunk]
        s = alpha * (Qf @ X[r].float().T) + bias[r][None, :]
        cs, ci = torch.cat([best_s, s], 1), torch.cat([best_i, r.expand(nq, -1)], 1)
        # (the list ascends and the kept entries came from earlier rows: stable keeps row order on ties)
        o = torch.sort(cs, dim=1, descending=True, stable=True).indices[:, :k]
        best_s, best_i = torch.gather(cs, 1, o), torch.gather(ci, 1, o)
    best_s, best_i = _pad(best_s, best_i, k)
    return best_s, torch.where(best_s == NEG_INF, torch.full_like(best_i, -1), best_i)


def gather_topk(X: torch.Tensor, rows: torch.Tensor, count: int, Q: torch.Tensor, k: int, bias: torch.Tensor,
                alpha: float = 1.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """Top-k of ``alpha * Q @ X[rows[:count]].T + bias[rows]`` per query, over
    the listed rows only (filter.hip lzk_gather_topk_partial + search.hip
    lzk_topk_merge): fp32 rows ``X`` [n, D], an ascending int32 row list,
    fp32 queries [nq, D], k <= 16. Returns (scores fp32 [nq, k], graph rows
    int64 [nq, k]) by (score desc, row asc); (-inf, -1) past the list."""
    if Q.dim() == 1:
        Q = Q[None, :]
    nq, D = Q.shape
    count = int(count)
    if not X.is_cuda:
        return gather_topk_ref(X, rows, count, Q, k, bias, alpha)
    dev = X.device
    L = _lib.lib()
    kslot = L.lzk_flat_topk_kslot(int(k))
    if kslot < 0:
        raise ValueError(f"gather_topk supports k <= 16 (got {k})")
    if count == 0 or nq == 0:
        return (torch.full((nq, k), NEG_INF, device=dev), torch.full((nq, k), -1, dtype=torch.long, device=dev))
    assert X.dtype == torch.float32 and X.stride(1) == 1 and X.shape[1] == D
    assert rows.dtype == torch.int32 and rows.is_contiguous() and rows.numel() >= count
    assert bias.dtype == torch.float32 and bias.is_contiguous()
    nrows = min(X.shape[0], bias.numel())  # (a graph's columns have spare capacity behind the n rows the bias covers)
    Qc = Q.to(torch.float32).contiguous()
    nch = L.lzk_gather_topk_chunks(count, nq, D, TARGET_WGS)
    part = nq * nch * kslot
    ws = _ws.get(dev, part * 8)
    ps = ws[: part * 4].view(torch.float32)
    pi = ws[part * 4: part * 8].view(torch.int32)
    st = _lib.stream_ptr(dev)
    _lib.check(L.lzk_gather_topk_partial(X.data_ptr(), X.stride(0), nrows, rows.data_ptr(), count, Qc.data_ptr(),
                                         Qc.stride(0), nq, bias.data_ptr(), float(alpha), D, kslot, nch,
                                         ps.data_ptr(), pi.data_ptr(), st), "lzk_gather_topk_partial")
    ncand = nch * kslot
    G = _merge_groups(nq, nch)
    if G > 1:  # few queries, many partial lists: two-level merge (see search._flat_topk_lane)
        os1 = torch.empty((nq * G, kslot), dtype=torch.float32, device=dev)
        oi1 = torch.empty((nq * G, kslot), dtype=torch.long, device=dev)
        _lib.check(L.lzk_topk_merge(ps.data_ptr(), pi.data_ptr(), ncand // G, nq * G, kslot, kslot, 0,
                                    os1.data_ptr(), oi1.data_ptr(), st), "lzk_topk_merge")
        ps, pi, ncand = os1, oi1.to(torch.int32), G * kslot
    os_ = torch.empty((nq, k), dtype=torch.float32, device=dev)
    oi = torch.empty((nq, k), dtype=torch.long, device=dev)
    _lib.check(L.lzk_topk_merge(ps.data_ptr(), pi.data_ptr(), ncand, nq, kslot, int(k), 0, os_.data_ptr(),
                                oi.data_ptr(), st), "lzk_topk_merge")
    return os_, oi
