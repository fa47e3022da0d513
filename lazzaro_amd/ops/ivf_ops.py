"""IVF-PQ index maintenance ops (``csrc/kernels/ivfmaint.hip``).

Device tensors go through the HIP kernels; CPU tensors through the ``*_ref``
torch formulations that compute the same thing on any device (the CPU test
tier and the oracle, not a fallback: ``_lib.lib()`` raises on a GPU box
without the kernel library).
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib

P, I, L = _lib.P, _lib.I, _lib.L

_lib.register("lzk_ivf_mark_count", I, [P, P, P, P, L, L, L, I, P, P, P])
_lib.register("lzk_ivf_spread_rows", I, [P, P, L, P, P, I, L, L, L, P, L, P, L, P, P])


def _st(t: torch.Tensor) -> int:
    return _lib.stream_ptr(t.device)


# ---------------------------------------------------------------- mark + count
def ivf_mark_count(list_of: torch.Tensor, pos: Optional[torch.Tensor], cdead: Optional[torch.Tensor],
                   vdead: Optional[torch.Tensor], nlist: int, ncount: Optional[int] = None
                   ) -> Tuple[torch.Tensor, torch.Tensor]:
    """One pass over the ``n`` code rows: uint8 ``keep[r] = !(cdead[r] |
    vdead[pos[r]])`` (either flag array may be None) and int64 ``cnt[l]`` =
    the kept rows of list ``l`` among the first ``ncount`` rows (default: all;
    the sorted prefix of an index with a pending tail)."""
    n = int(list_of.numel())
    ncount = n if ncount is None else int(ncount)
    if not list_of.is_cuda:
        return ivf_mark_count_ref(list_of, pos, cdead, vdead, nlist, ncount)
    assert list_of.dtype == torch.int32 and list_of.is_contiguous()
    assert vdead is None or (pos is not None and pos.dtype == torch.int64 and pos.is_contiguous()
                             and pos.numel() >= n)
    assert cdead is None or (cdead.dtype == torch.uint8 and cdead.numel() >= n)
    assert vdead is None or vdead.dtype == torch.uint8
    keep = torch.empty(n, dtype=torch.uint8, device=list_of.device)
    cnt = torch.zeros(nlist, dtype=torch.int64, device=list_of.device)
    _lib.check(_lib.lib().lzk_ivf_mark_count(list_of.data_ptr(), _lib.ptr(pos), _lib.ptr(cdead), _lib.ptr(vdead),
                                             int(vdead.numel()) if vdead is not None else 0, n, ncount, int(nlist),
                                             keep.data_ptr(), cnt.data_ptr(), _st(list_of)), "ivf_mark_count")
    return keep, cnt


def ivf_mark_count_ref(list_of, pos, cdead, vdead, nlist: int, ncount: Optional[int] = None):
    """The torch formulation of :func:`ivf_mark_count` (any device)."""
    n = int(list_of.numel())
    ncount = n if ncount is None else int(ncount)
    dead = torch.zeros(n, dtype=torch.bool, device=list_of.device)
    if cdead is not None:
        dead |= cdead[:n] != 0
    if vdead is not None:
        dead |= vdead[pos[:n]] != 0
    keep = (~dead).to(torch.uint8)
    cnt = torch.bincount(list_of[:ncount][keep[:ncount] != 0].long(), minlength=nlist)
    return keep, cnt


# ---------------------------------------------------------------- spread
def ivf_spread_bounds(list_of: torch.Tensor, ins: torch.Tensor, n0: int, first: int, chunk_rows: int) -> np.ndarray:
    """The shift ``ins[list_of[r]]`` at the chunk boundaries first, first +
    chunk_rows, ... and at row n0 - 1 (host int64): what the in-place
    schedule of :func:`ivf_spread_rows` decides by."""
    if n0 <= 0 or first >= n0:
        return np.zeros(1, np.int64)
    idx = list(range(first, n0, chunk_rows)) + [n0 - 1]
    rows = torch.as_tensor(idx, dtype=torch.long).to(list_of.device)
    return ins[list_of[rows].long()].cpu().numpy().astype(np.int64)


def ivf_spread_first(list_of: torch.Tensor, ins: torch.Tensor, n0: int) -> int:
    """The first row of ``[0, n0)`` that moves (n0 when none does)."""
    if n0 <= 0:
        return 0
    moving = ins[list_of[:n0].long()] > 0
    return int(n0 - int(moving.sum()))  # the shift is non-decreasing: the moving rows are a suffix


def ivf_spread_rows(col: torch.Tensor, list_of: torch.Tensor, ins: torch.Tensor, n0: int, first: int,
                    chunk_rows: int, bounds: Optional[np.ndarray] = None, bounce: Optional[torch.Tensor] = None,
                    src: Optional[torch.Tensor] = None) -> Tuple[int, int, int]:
    """Open gaps in a list-sorted column: row ``r`` of ``col[first:n0]`` moves
    up to ``r + ins[list_of[r]]``, in place and in order (ivfmaint.hip
    ivf_spread_rows_kernel; the descending chunk schedule and why it is safe
    are described there). ``list_of`` int32 [n0] sorted, ``ins`` int64
    [nlist + 1] non-decreasing. ``first``: the first row that moves.
    ``bounce``: a uint8 device buffer of at least chunk_rows x row bytes
    (allocated here when missing). ``src``: read the rows from this other
    tensor instead (out of place: the key column itself). The rows between
    the moved runs keep stale bytes -- the caller fills them. Returns (bytes
    moved, chunks written directly, chunks through the bounce buffer). An
    invalid schedule (decreasing shift, destination past ``col``'s rows, small
    bounce buffer) raises before anything is launched. CPU tensors:
    :func:`ivf_spread_rows_ref`."""
    if not col.is_cuda:
        ivf_spread_rows_ref(col, list_of, ins, n0, src=src)
        rb = col[0].numel() * col.element_size() if col.shape[0] else 0
        return (n0 - first) * rb if n0 > first else 0, 0, 0
    assert col.is_contiguous() and list_of.dtype == torch.int32 and ins.dtype == torch.int64
    assert list_of.is_contiguous() and ins.is_contiguous() and list_of.numel() >= n0
    assert src is None or (src.is_contiguous() and src.dtype == col.dtype and src.shape[1:] == col.shape[1:]
                           and src.shape[0] >= n0)
    row_bytes = (col.numel() // col.shape[0]) * col.element_size() if col.shape[0] else 0
    if n0 == 0 or first >= n0 or row_bytes == 0:
        return 0, 0, 0
    if bounds is None:
        bounds = ivf_spread_bounds(list_of, ins, n0, first, chunk_rows)
    bounds = np.ascontiguousarray(bounds, dtype=np.int64)
    assert len(bounds) == (n0 - first + chunk_rows - 1) // chunk_rows + 1
    if src is None:
        need = min(chunk_rows, n0 - first) * row_bytes
        if bounce is None:
            bounce = torch.empty(need, dtype=torch.uint8, device=col.device)
    stats = np.zeros(3, np.int64)
    _lib.check(_lib.lib().lzk_ivf_spread_rows(col.data_ptr(), _lib.ptr(src), row_bytes, list_of.data_ptr(),
                                              ins.data_ptr(), int(ins.numel()) - 1, int(n0), int(first),
                                              int(chunk_rows), bounds.ctypes.data, int(col.shape[0]),
                                              _lib.ptr(bounce) if src is None else None,
                                              int(bounce.numel()) if (src is None and bounce is not None) else 0,
                                              stats.ctypes.data, _st(col)), "ivf_spread_rows")
    return int(stats[0]), int(stats[1]), int(stats[2])


def ivf_spread_rows_ref(col: torch.Tensor, list_of: torch.Tensor, ins: torch.Tensor, n0: int,
                        src: Optional[torch.Tensor] = None) -> None:
    """The torch formulation of :func:`ivf_spread_rows` (out of place: the
    gather makes a second copy of the rows)."""
    if n0 <= 0:
        return
    dst = torch.arange(n0, device=col.device) + ins[list_of[:n0].long()]
    col[dst] = (col if src is None else src)[:n0].clone()


def ivf_tail_slots(tail_lists: torch.Tensor, old_off: torch.Tensor, nlist: int):
    """Where the tail rows go. ``tail_lists``: the lists of the appended rows
    in creation order; ``old_off`` int64 [nlist + 1]: the CSR offsets of the
    sorted part. Returns (order, ins, dest): the stable order of the tail by
    list, ``ins[l]`` = tail rows whose list is < l (int64 [nlist + 1]) and the
    destination of each tail row in that order -- behind the old rows of its
    list, in creation order."""
    order = torch.argsort(tail_lists, stable=True)
    tl = tail_lists[order].long()
    ins = torch.zeros(nlist + 1, dtype=torch.int64, device=tail_lists.device)
    ins[1:] = torch.cumsum(torch.bincount(tl, minlength=nlist), 0)
    dest = old_off[tl + 1] + torch.arange(tl.numel(), device=tl.device)
    return order, ins, dest
