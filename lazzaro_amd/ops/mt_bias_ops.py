"""Options in the served batch: the bias columns of one multi-tenant round in
one launch (csrc/kernels/mtbias.hip ``lzk_mt_bias``) and their torch
formulation.

``DistributedMemoryService`` answers a round of ``search_memories`` requests
of many tenants with one ``segment_topk`` launch that scores
``alpha <q, x_r> + bias[r] + qbias[q]`` with a bias address per query. By their
contracts ``where=`` and ``boost=`` are nothing but a bias column, so a round
with per-request options needs one column per distinct (tenant, filter, boost)
combination -- a *job* -- and nothing else:

    base(r) = job has a filter ? (pass(r) ? (l2 ? 0.0f - sqn[r] : 0.0f) : -inf)
                               : store_bias[r]
    out(r)  = job has a boost  ? (kind[r] == NODE ? base(r) + prior(r) : -inf)
                               : base(r)

``pass`` is the predicate of ops/filter_ops.py (memories only: NODE rows in
the store that pass every test), ``prior`` the fp64 expression of
ops/boost_ops.py. **Contract:** the column of a job equals, bit for bit, what
``TenantGraph._filter_plan(flt, l2).bias`` or ``TenantGraph.boost_bias(boost,
metric, where=flt, now=now)`` returns for that tenant -- the kernel compiles
the same text as filter.hip and boost.hip (csrc/include/lzk_rowpred.h), and the
arithmetic is plain IEEE. The numpy oracle is tests/kernels/_mtbias_ref.py.

:func:`mt_bias` packs the job descriptors, the block prefix and the auxiliary
tables (shard bitmaps, exclusion bitmaps, type-weight tables) into one pinned
staging buffer, issues ONE asynchronous copy and ONE launch on the current
stream, and reads nothing back. The staging buffer is double-buffered behind
an event: ``serve_stream`` keeps two rounds in flight, and a buffer whose copy
may still be pending is never overwritten.

Device tensors always take the kernel; CPU tensors take :func:`mt_bias_ref`
(the CPU tier).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .boost_ops import boost_bias_ref
from .filter_ops import PLAN_COLS, Predicate, _bitmap, filter_plan_ref

MB_FILTER, MB_BOOST = 1, 2

# csrc/kernels/mtbias.hip LzkMtBiasJob, field for field (every field is
# naturally aligned, so the packed layout is the C layout)
_PTRS = ("sal", "acc", "last", "ts", "shard", "kind", "sup", "stored", "tcode", "sqn", "store_bias")
JOB_DTYPE = np.dtype(
    [(p, np.uint64) for p in _PTRS] + [("n", np.int64), ("out_off", np.int64)]
    + [("since", np.float64), ("until", np.float64), ("accessed_since", np.float64),  # LzkFilterBounds
       ("min_sal", np.float32), ("max_sal", np.float32), ("min_acc", np.int32), ("sup_mode", np.int32),
       ("fb_flags", np.int32), ("n_shard_bits", np.int32), ("neg_shard_pass", np.int32), ("l2", np.int32),
       ("type_mask", np.uint32, (8,))]
    + [(w, np.float64) for w in ("w_sal", "w_freq", "w_rec", "scale", "now", "c")]
    + [("shard_off", np.int64), ("excl_off", np.int64), ("tw_off", np.int64), ("clock", np.int32),
       ("flags", np.int32)])
assert JOB_DTYPE.itemsize == 272

_lib.register("lzk_mt_bias_job_bytes", _lib.I, [])
_lib.register("lzk_mt_bias_block_rows", _lib.I, [])
_lib.register("lzk_mt_bias", _lib.I, [_lib.P, _lib.I, _lib.P, _lib.P, _lib.P, _lib.I, _lib.P])

BLOCK_ROWS = 1024  # rows per block (checked against lzk_mt_bias_block_rows on first use)


@dataclass
class MtBiasJob:
    """One (tenant, filter, boost) combination of a round
    (``TenantGraph._mt_bias_job``). ``cols``: the tenant's PLAN_COLS columns;
    ``pred``: the filter resolved against the tenant, None = no filter;
    ``boost``: the settings with ``now`` set, None = no boost; ``tw``: 256
    weights by type code, None = no type weights; ``c``: 2 for L2, else 1.
    ``store_bias``: the base of a job without a filter. The tensors are held,
    so the addresses the kernel reads stay allocated while the job lives."""
    cols: Dict[str, torch.Tensor]
    n: int
    pred: Optional[Predicate] = None
    l2: bool = True
    sqn: Optional[torch.Tensor] = None
    store_bias: Optional[torch.Tensor] = None
    tcode: Optional[torch.Tensor] = None
    boost: Optional[object] = None
    tw: Optional[Sequence[float]] = None
    c: float = 2.0

    @property
    def device(self) -> torch.device:
        return self.cols["kind"].device

    def check(self) -> None:
        """The bounds the kernel relies on: every column it reads holds at
        least ``n`` contiguous rows of the right type."""
        n, dev = self.n, self.device
        want = {"sal": torch.float32, "acc": torch.int32, "last": torch.float64, "ts": torch.float64,
                "shard": torch.int32, "kind": torch.uint8, "sup": torch.uint8, "stored": torch.uint8}
        for name in PLAN_COLS:
            t = self.cols[name]
            assert t.dtype == want[name] and t.numel() >= n and t.is_contiguous() and t.device == dev, name
        p = self.pred
        if p is None:
            b = self.store_bias
            assert b is not None and b.dtype == torch.float32 and b.numel() >= n and b.is_contiguous()
        elif self.l2:
            assert self.sqn is not None and self.sqn.dtype == torch.float32 and self.sqn.numel() >= n \
                and self.sqn.is_contiguous()
        if (p is not None and p.type_codes is not None) or self.tw is not None:
            t = self.tcode
            assert t is not None and t.dtype == torch.uint8 and t.numel() >= n and t.is_contiguous()
        assert self.tw is None or (self.boost is not None and len(self.tw) == 256)


def mt_bias_ref(jobs: Sequence[MtBiasJob]) -> List[torch.Tensor]:
    """Torch formulation of :func:`mt_bias` (any device): one fp32 [n_j]
    column per job, composed from ``filter_plan_ref`` and ``boost_bias_ref``."""
    out = []
    for j in jobs:
        n = int(j.n)
        if n == 0:
            out.append(torch.empty(0, dtype=torch.float32, device=j.device))
            continue
        if j.pred is not None:
            base = filter_plan_ref(j.cols, j.pred, j.sqn, n, j.l2, j.tcode)[0]
        else:
            base = j.store_bias[:n]
        if j.boost is not None:
            b = j.boost
            t = j.cols["last"] if b.clock == "accessed" else j.cols["ts"]
            base = boost_bias_ref(base, j.cols["sal"], j.cols["acc"], t, j.cols["kind"], n, b.salience, b.frequency,
                                  b.recency, b.recency_scale, b.now, j.c, j.tcode if j.tw is not None else None, j.tw)
        out.append(base.contiguous())
    return out


def _offsets(jobs: Sequence[MtBiasJob]) -> Tuple[List[int], int]:
    """Where each job's column starts in the arena (floats, multiples of 4)
    and the arena's length."""
    offs, at = [], 0
    for j in jobs:
        offs.append(at)
        at += (int(j.n) + 3) & ~3
    return offs, at


def _pack(jobs: Sequence[MtBiasJob], offs: Sequence[int]):
    """(records, blk0, aux bytes): the descriptors, the exclusive prefix of
    the jobs' block counts, and the auxiliary tables the records point into
    by byte offset (each table starts at a multiple of 8)."""
    rows = []  # one tuple per job, in JOB_DTYPE's field order: converted in one call, not field by field
    blk0 = np.zeros(len(jobs) + 1, dtype=np.int32)
    aux: List[np.ndarray] = []
    at = 0
    no_mask = (0,) * 8

    def push(a: np.ndarray) -> int:
        nonlocal at
        b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        pad = (-b.size) % 8
        if pad:
            b = np.concatenate([b, np.zeros(pad, np.uint8)])
        aux.append(b)
        at += b.size
        return at - b.size

    for i, j in enumerate(jobs):
        j.check()
        n = int(j.n)
        shard_off = excl_off = tw_off = -1
        flags = 0
        p = j.pred
        if p is not None:
            flags |= MB_FILTER
            mask, nb = no_mask, 0
            if p.type_codes is not None:
                mask = tuple(_bitmap(p.type_codes, 256).tolist())
            if p.shard_codes is not None:
                nb = max([int(c) + 1 for c in p.shard_codes], default=0)
                if nb:
                    shard_off = push(_bitmap(p.shard_codes, nb))
            if p.exclude_rows is not None:
                excl_off = push(_bitmap(p.exclude_rows, n))  # (ceil(n / 32) words: a bit per row)
            fb = (float(p.since or 0.0), float(p.until or 0.0), float(p.accessed_since or 0.0),
                  float(p.min_sal or 0.0), float(p.max_sal or 0.0), int(p.min_acc or 0), int(p.sup_mode), p.flags(),
                  nb, int(bool(p.neg_shard_pass)), int(bool(j.l2)), mask)
        else:
            fb = (0.0, 0.0, 0.0, 0.0, 0.0, 0, -1, 0, 0, 0, 0, no_mask)
        b = j.boost
        if b is not None:
            flags |= MB_BOOST
            w = (b.salience, b.frequency, b.recency, b.recency_scale, b.now, float(j.c))
            clock = 0 if b.clock == "accessed" else 1
            if j.tw is not None:
                tw_off = push(np.asarray(j.tw, dtype=np.float64))
        else:
            w, clock = (0.0,) * 6, 0
        rows.append(tuple(j.cols[name].data_ptr() for name in PLAN_COLS)
                    + (_lib.ptr(j.tcode), _lib.ptr(j.sqn), _lib.ptr(j.store_bias), n, offs[i]) + fb + w
                    + (shard_off, excl_off, tw_off, clock, flags))
        blk0[i + 1] = blk0[i] + (n + BLOCK_ROWS - 1) // BLOCK_ROWS
    rec = np.array(rows, dtype=JOB_DTYPE)
    return rec, blk0, (np.concatenate(aux) if aux else np.zeros(0, np.uint8))


class _Staging:
    """Two pinned staging buffers per device, each behind the event of its
    last copy."""

    def __init__(self):
        self.slots = [[None, None], [None, None]]  # [pinned uint8 tensor, event of its last copy]
        self.turn = 0

    def take(self, nbytes: int):
        s = self.slots[self.turn]
        self.turn ^= 1
        if s[1] is not None:
            s[1].synchronize()  # (done long ago unless three rounds are in flight)
        if s[0] is None or s[0].numel() < nbytes:
            s[0] = torch.empty(max(2 * nbytes, 1 << 16), dtype=torch.uint8, pin_memory=True)
        return s


_staging: Dict[int, _Staging] = {}
_checked = False


def mt_bias(jobs: Sequence[MtBiasJob], keep: Optional[list] = None) -> Tuple[torch.Tensor, List[int]]:
    """The bias columns of ``jobs`` (mtbias.hip ``lzk_mt_bias``): returns
    ``(arena, offsets)`` -- one fp32 device tensor and, per job, where its
    ``n`` floats start in it (a multiple of 4, so ``arena.data_ptr() + 4 *
    offsets[j]`` is 16-byte aligned). One asynchronous copy of the packed
    descriptors and one launch on the current stream; nothing is read back.
    ``keep``: a list that receives the device and staging buffers the launch
    reads, for a caller that must keep them alive past its own scope."""
    global _checked
    jobs = list(jobs)
    offs, total = _offsets(jobs)
    if not jobs:
        return torch.empty(0, dtype=torch.float32), offs
    dev = jobs[0].device
    assert all(j.device == dev for j in jobs)
    if dev.type != "cuda":
        arena = torch.zeros(total, dtype=torch.float32, device=dev)
        for j, o, col in zip(jobs, offs, mt_bias_ref(jobs)):
            arena[o: o + int(j.n)] = col
        return arena, offs
    L = _lib.lib()
    if not _checked:
        assert L.lzk_mt_bias_job_bytes() == JOB_DTYPE.itemsize and L.lzk_mt_bias_block_rows() == BLOCK_ROWS
        _checked = True
    rec, blk0, aux = _pack(jobs, offs)
    jb = rec.nbytes
    bb = (blk0.nbytes + 7) & ~7
    nbytes = jb + bb + aux.size
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    slot = _staging.setdefault(idx, _Staging()).take(nbytes)
    host = slot[0].numpy()
    host[:jb] = rec.view(np.uint8).reshape(-1)
    host[jb: jb + blk0.nbytes] = blk0.view(np.uint8)
    host[jb + bb: nbytes] = aux
    dbuf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    dbuf.copy_(slot[0][:nbytes], non_blocking=True)
    ev = torch.cuda.Event()
    ev.record()
    slot[1] = ev
    arena = torch.empty(max(total, 4), dtype=torch.float32, device=dev)
    base = dbuf.data_ptr()
    assert base % 16 == 0 and arena.data_ptr() % 16 == 0
    _lib.check(L.lzk_mt_bias(base, len(jobs), base + jb, base + jb + bb, arena.data_ptr(), int(blk0[-1]),
                             _lib.stream_ptr(dev)), "lzk_mt_bias")
    if keep is not None:
        keep += [dbuf, slot[0], jobs]
    return arena, offs
