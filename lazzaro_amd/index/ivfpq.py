"""IVF-PQ index (BASELINE config 5).

Memory: ``M`` bytes of PQ code + 20 bytes of list id / position / id per
vector, so one MI355X (288 GB HBM) holds ~3 billion 1024-d vectors at M=64
codes-only, ~200M with an fp8 re-rank copy -- vs 2 KB/vector for bf16 flat
storage. Inner-product metric on unit vectors (cosine).

* train: coarse k-means (``kmeans``: fused MFMA top-1 assign + segmented mean)
  and ``M`` residual sub-quantisers of 256 codewords each
* add:   coarse assign (fused top-1), residual PQ encode (batched GEMM +
         argmax per sub-space), then codes are kept sorted by list (CSR)
* search: coarse probe (top-nprobe centroids), per-query LUT
          ``<q_j, codebook_j[c]>`` (one batched GEMM), HIP ``ivfpq_scan``
          kernel per (query, probed list) with a fused top-k, shared
          ``topk_merge`` kernel; deep lists (re-rank depth > 16) from
          ``ivfpq_scan_deep`` (each wave's best rows per list); optional exact
          re-rank of the candidates against kept bf16/fp8 rows.
* filter: ``filter_rows(allow)`` compacts the code rows whose id passes a mask
          into per-list row lists (ivfpq_filter.hip); ``search`` /
          ``candidate_ids`` with ``allow=`` then scan the passing rows of the
          probed lists only (the ``_f`` scans of ivfpq.hip, one indirection
          per scored row) -- the exact PQ top-k / top-R among passing rows.
* maintain: ``remove(ids)``, ``upsert(ids, x)`` and ``translate_ids(table)``
          delete, rewrite and renumber vectors without a re-train or a
          re-encode of the rest. They only flag rows and append code rows; the
          next search's ``_finalize`` squeezes the flagged rows out in place
          (compact.hip) and merges the appended tail into the CSR order by
          opening gaps in place (ivfmaint.hip) -- O(n) bytes moved, no sort
          and no second code buffer. ``_finalize_ref`` is the torch
          formulation (stable full sort) that the kernel path equals bit for
          bit. Ids are unique among the live vectors.
CPU tensors run a torch reference of the same pipeline (tests).
"""
from __future__ import annotations

import itertools
from typing import Optional, Tuple

import numpy as np
import torch

from ..ops import _lib
from ..ops.search import _ws, flat_topk
from .kmeans import assign as coarse_assign
from .kmeans import kmeans

_lib.register("lzk_ivfpq_scan", _lib.I, [_lib.P, _lib.P, _lib.P, _lib.P, _lib.P, _lib.I, _lib.I, _lib.I, _lib.I,
                                          _lib.P, _lib.P, _lib.P])

_lib.register("lzk_ivfpq_scan_deep", _lib.I, [_lib.P, _lib.P, _lib.P, _lib.P, _lib.P, _lib.I, _lib.I, _lib.I,
                                               _lib.P, _lib.P, _lib.P])
_lib.register("lzk_ivfpq_deep_width", _lib.I, [])
_lib.register("lzk_ivfpq_scan_thresh", _lib.I, [_lib.P, _lib.P, _lib.P, _lib.P, _lib.P, _lib.P, _lib.I, _lib.I,
                                                _lib.I, _lib.I, _lib.P, _lib.P, _lib.P, _lib.P])

_lib.register("lzk_rerank", _lib.I, [_lib.P, _lib.L, _lib.I, _lib.P, _lib.P, _lib.I, _lib.I, _lib.P, _lib.I,
                                      _lib.I, _lib.I, _lib.P, _lib.P, _lib.P])

_lib.register("lzk_ivfpq_scan_f", _lib.I, [_lib.P, _lib.P, _lib.P, _lib.P, _lib.P, _lib.P, _lib.I, _lib.I, _lib.I,
                                            _lib.I, _lib.P, _lib.P, _lib.P])
_lib.register("lzk_ivfpq_scan_deep_f", _lib.I, [_lib.P, _lib.P, _lib.P, _lib.P, _lib.P, _lib.P, _lib.I, _lib.I,
                                                 _lib.I, _lib.P, _lib.P, _lib.P])
_lib.register("lzk_ivfpq_scan_thresh_f", _lib.I, [_lib.P, _lib.P, _lib.P, _lib.P, _lib.P, _lib.P, _lib.P, _lib.I,
                                                   _lib.I, _lib.I, _lib.I, _lib.P, _lib.P, _lib.P, _lib.P])
_lib.register("lzk_ivfpq_filter_rows_ws", _lib.L, [_lib.L])
_lib.register("lzk_ivfpq_filter_rows", _lib.I, [_lib.P, _lib.P, _lib.L, _lib.P, _lib.I, _lib.L, _lib.P, _lib.I,
                                                 _lib.L, _lib.P, _lib.P, _lib.P, _lib.P])

KSLOTS = (1, 4, 10, 16)

# order_gen values: unique over every index of the process, so lists built for
# one index never look current to another (a tenant's rebuilt index)
_GEN = itertools.count(1)

# _finalize on the GPU: flagged rows leave and the appended tail is merged in
# place by the HIP kernels (compact.hip, ivfmaint.hip); MAINT_KERNEL = False:
# the torch formulation the CPU runs (a stable sort of every row)
MAINT_KERNEL = True


def _kslot(k: int) -> int:
    for s in KSLOTS:
        if k <= s:
            return s
    raise ValueError("k <= 16 per IVF-PQ pass")


def _unit(x):
    return x / x.norm(dim=1, keepdim=True).clamp_min(1e-30)


def filtered_nprobe(nprobe: int, nlist: int, n: int, count: int) -> int:
    """Lists to probe when ``count`` of ``n`` rows pass a filter: a filter
    passing 1/s of the rows leaves 1/s of each list, so s times the lists
    keep the number of scanned passing rows level -- capped at ``nlist``."""
    return min(nlist, -(-nprobe * n // max(count, 1)))


class FilteredLists:
    """The code rows of an index that pass a filter, per list: ``rows``
    (int32, ascending code rows, CSR order) and ``off`` (int64 [nlist + 1]
    offsets into ``rows``; ``off[nlist]`` = the number of listed rows). Valid
    while the index's ``order_gen`` equals ``gen``; ``allow`` is the mask they
    were built from (None: not kept, a stale object cannot be rebuilt)."""
    __slots__ = ("rows", "off", "gen", "allow", "max_rows")

    def __init__(self, rows, off, gen, allow=None, max_rows=None):
        self.rows, self.off, self.gen, self.allow, self.max_rows = rows, off, gen, allow, max_rows


class IVFPQIndex:
    def __init__(self, dim: int, nlist: int = 1024, m: int = 64, device=None, keep_vectors=False):
        """keep_vectors: False (codes only, m+20 bytes/vector), True / "bf16"
        (exact re-rank copy, 2*Dp bytes/vector), "int8" or "fp8" (re-rank
        copy with a per-row scale, D+4 bytes/vector -- the layout that fills
        288 GB with ~200M 1024-d vectors and still re-ranks PQ candidates;
        int8's uniform grid is ~3x finer than e4m3 on embedding rows, so it
        is the one to use for recall).

        Storage is preallocated (:meth:`reserve`) and written in place. Code
        rows (``codes``, ``list_of``) are kept sorted by list (CSR) and carry
        ``pos`` = the insertion row of each; the re-rank copy and the ids stay
        in insertion order, so sorting never moves the big vector copy."""
        assert dim % m == 0, "dim must be divisible by m"
        self.dim, self.nlist, self.m, self.dsub = dim, nlist, m, dim // m
        self.device = torch.device(device) if device is not None else torch.device("cpu")
        self.Dp = (dim + 63) // 64 * 64
        self.centroids = None      # fp32 [nlist, dim]
        self.centroids16 = None    # bf16 [nlist, Dp] (GPU assign)
        self.codebooks = None      # fp32 [m, 256, dsub]
        self.keep_vectors = "bf16" if keep_vectors is True else (keep_vectors or False)
        if self.keep_vectors not in (False, "bf16", "fp8", "int8"):
            raise ValueError("keep_vectors must be False, True/'bf16', 'int8' or 'fp8'")
        self.n = 0   # code rows (codes, list_of, pos)
        self.nv = 0  # vector rows (ids, re-rank copy); == n except while changes are pending
        self.cap = 0
        self._sorted_n = 0  # the prefix of the code rows in CSR order, described by list_off
        self._cdead = None  # pending: uint8 per code row / per vector row, 1 = leaves at
        self._vdead = None  # the next _finalize (allocated on first use, dropped there)
        self._nlive = 0
        self.chunk_rows = None  # rows per chunk of the in-place moves (None: rc_chunk_rows)
        self.last_maint = None  # what the last in-place _finalize moved (bytes, direct / bounced chunks)
        z = lambda *s, dt: torch.zeros(s, dtype=dt, device=self.device)  # noqa: E731
        self._codes = z(0, m, dt=torch.uint8)
        self._list = z(0, dt=torch.int32)
        self._pos = z(0, dt=torch.int64)
        self._vids = z(0, dt=torch.int64)
        self._vec = None
        self._vscale = None
        self.list_off = z(nlist + 1, dt=torch.int64)
        self._dirty = False
        # bumps whenever the code rows, their order or their ids may have changed (what FilteredLists depend on)
        self.order_gen = next(_GEN)

    # ------------------------------------------------------------------ storage
    def reserve(self, n: int) -> None:
        """Capacity for ``n`` vectors (grows by copying; call once up front to
        build a large index without reallocations)."""
        if n <= self.cap:
            return
        cap = max(n, int(self.cap * 1.5) + 1)
        k = max(self.n, self.nv)

        def grow(t, shape, dt):
            new = torch.zeros(shape, dtype=dt, device=self.device)
            if t is not None and k:
                new[:k] = t[:k]
            return new
        self._codes = grow(self._codes, (cap, self.m), torch.uint8)
        self._list = grow(self._list, (cap,), torch.int32)
        self._pos = grow(self._pos, (cap,), torch.int64)
        self._vids = grow(self._vids, (cap,), torch.int64)
        if self.keep_vectors == "bf16":
            w = self.Dp if self.device.type == "cuda" else self.dim
            self._vec = grow(self._vec, (cap, w), torch.bfloat16 if self.device.type == "cuda" else torch.float32)
        elif self.keep_vectors in ("fp8", "int8"):
            self._vec = grow(self._vec, (cap, self.dim), torch.uint8)
            self._vscale = grow(self._vscale, (cap,), torch.float32)
        if self._cdead is not None:
            self._cdead = grow(self._cdead, (cap,), torch.uint8)
        if self._vdead is not None:
            self._vdead = grow(self._vdead, (cap,), torch.uint8)
        self.cap = cap

    # views of the live rows (code order) -- and setters for hand-built indexes
    @property
    def codes(self) -> torch.Tensor:
        return self._codes[: self.n]

    @codes.setter
    def codes(self, v: torch.Tensor) -> None:
        self._codes, self.n, self.cap = v.to(self.device), v.shape[0], v.shape[0]
        self._pos = torch.arange(self.n, device=self.device)
        # a hand-built index is in CSR order already (list_off is set beside it)
        self.nv = self._sorted_n = self._nlive = self.n
        self._cdead = self._vdead = None
        self.order_gen = next(_GEN)

    @property
    def list_of(self) -> torch.Tensor:
        return self._list[: self.n]

    @list_of.setter
    def list_of(self, v: torch.Tensor) -> None:
        self._list = v.to(self.device, torch.int32)

    @property
    def ids(self) -> torch.Tensor:
        """ids in code order."""
        return self._vids[self._pos[: self.n]]

    @ids.setter
    def ids(self, v: torch.Tensor) -> None:
        self._vids = v.to(self.device, torch.int64)
        self._pos = torch.arange(v.shape[0], device=self.device)
        self.order_gen = next(_GEN)

    @property
    def vectors(self):
        return None if self._vec is None else self._vec[: self.nv]

    @property
    def vscale(self):
        return None if self._vscale is None else self._vscale[: self.nv]

    # ------------------------------------------------------------------ train
    def _pad(self, x: torch.Tensor) -> torch.Tensor:
        if self.device.type != "cuda":
            return x.float()
        out = torch.zeros((x.shape[0], self.Dp), dtype=torch.bfloat16, device=self.device)
        out[:, : self.dim] = x.to(torch.bfloat16)
        return out

    def train(self, x: torch.Tensor, iters: int = 10, pq_iters: int = 12, seed: int = 0) -> None:
        x = _unit(x.to(self.device).float())
        c32, _, lab = kmeans(self._pad(x), self.nlist, iters=iters, seed=seed)
        self.centroids = c32[:, : self.dim].contiguous()
        self.centroids16 = self._pad(self.centroids)
        res = x - self.centroids[lab.long()]
        self.codebooks = self._train_pq(res, pq_iters, seed)

    def _train_pq(self, res: torch.Tensor, iters: int, seed: int) -> torch.Tensor:
        n = res.shape[0]
        g = torch.Generator(device="cpu").manual_seed(seed + 1)
        sub = res.view(n, self.m, self.dsub).transpose(0, 1).contiguous()  # [m, n, dsub]
        init = torch.randperm(n, generator=g)[:256].to(res.device)
        cb = sub[:, init].clone()  # [m, 256, dsub]
        for _ in range(iters):
            code = self._encode_sub(sub, cb)  # [m, n]
            sums = torch.zeros_like(cb).scatter_add_(1, code[..., None].expand(-1, -1, self.dsub).long(), sub)
            cnt = torch.zeros((self.m, 256), device=res.device).scatter_add_(
                1, code.long(), torch.ones_like(code, dtype=torch.float32))
            upd = sums / cnt.clamp_min(1)[..., None]
            cb = torch.where((cnt > 0)[..., None], upd, cb)
        return cb

    @staticmethod
    def _encode_sub(sub: torch.Tensor, cb: torch.Tensor, chunk: int = 16384) -> torch.Tensor:
        # argmin ||r - c||^2 = argmax (2 r.c - |c|^2), batched over sub-spaces,
        # chunked over rows so the [m, rows, 256] score block stays ~1 GB
        cn = (cb * cb).sum(-1)[:, None, :]
        out = torch.empty(sub.shape[:2], dtype=torch.uint8, device=sub.device)
        for r0 in range(0, sub.shape[1], chunk):
            score = 2.0 * torch.bmm(sub[:, r0:r0 + chunk], cb.transpose(1, 2)) - cn
            out[:, r0:r0 + chunk] = score.argmax(-1).to(torch.uint8)
        return out

    # ------------------------------------------------------------------ add
    def encode(self, x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        x = _unit(x.to(self.device).float())
        if self.device.type == "cuda":
            lab, _ = coarse_assign(self._pad(x), self.centroids16)
        else:
            lab = (x @ self.centroids.T).argmax(1).to(torch.int32)
        res = x - self.centroids[lab.long()]
        sub = res.view(-1, self.m, self.dsub).transpose(0, 1).contiguous()
        codes = self._encode_sub(sub, self.codebooks).T.contiguous()  # [n, m]
        return lab, codes

    def add(self, x: torch.Tensor, ids: Optional[torch.Tensor] = None, batch: int = 1 << 18) -> None:
        n = x.shape[0]
        ids = torch.arange(self.n, self.n + n, dtype=torch.int64) if ids is None else ids.to(torch.int64)
        self._append(x, ids, None, batch)

    def _append(self, x: torch.Tensor, ids: Optional[torch.Tensor], vrows: Optional[torch.Tensor],
                batch: int = 1 << 18) -> None:
        """Encode ``x`` into new code rows at the tail. ``vrows`` None: new
        vector rows with ``ids`` behind the existing ones (``add``); else the
        vector rows (int64, on the device) whose kept copy is overwritten and
        which the new code rows point at (``upsert`` of held ids)."""
        n0, v0 = self.n, self.nv
        n = x.shape[0]
        fresh = vrows is None
        self.reserve(max(n0 + n, v0 + (n if fresh else 0)))
        if fresh:
            self._vids[v0:v0 + n] = ids.to(self.device)
            self._pos[n0:n0 + n] = torch.arange(v0, v0 + n, device=self.device)
        else:
            self._pos[n0:n0 + n] = vrows
        for r0 in range(0, n, batch):
            r1 = min(n, r0 + batch)
            xb = _unit(x[r0:r1].to(self.device).float())
            lab, codes = self.encode(xb)
            self._list[n0 + r0:n0 + r1] = lab
            self._codes[n0 + r0:n0 + r1] = codes
            vr = slice(v0 + r0, v0 + r1) if fresh else vrows[r0:r1]
            if self.keep_vectors == "bf16":
                self._vec[vr] = self._pad(xb) if self.device.type == "cuda" else xb
            elif self.keep_vectors == "fp8":
                from ..ops.encoder_ops import quantize_fp8_rows
                v = xb.to(torch.bfloat16) if self.device.type == "cuda" else xb
                q8, sc = quantize_fp8_rows(v.contiguous())
                self._vec[vr] = q8
                self._vscale[vr] = sc
            elif self.keep_vectors == "int8":
                sc = xb.abs().amax(1).clamp_min(1e-30) / 127.0
                q = torch.round(xb / sc[:, None]).clamp_(-127, 127).to(torch.int8)
                self._vec[vr] = q.view(torch.uint8)
                self._vscale[vr] = sc
        self.n = n0 + n
        if fresh:
            self.nv = v0 + n
            self._nlive += n
        self._dirty = True
        self.order_gen = next(_GEN)

    # ------------------------------------------------------------------ maintain
    def _flags(self, which: str) -> torch.Tensor:
        f = getattr(self, which)
        if f is None:
            f = torch.zeros(max(self.cap, self.n, self.nv), dtype=torch.uint8, device=self.device)
            setattr(self, which, f)
        return f

    def _lookup(self, ids: torch.Tensor, chunk: int = 1 << 24) -> Tuple[torch.Tensor, torch.Tensor]:
        """(vector rows, index into ``ids``) of the live vectors whose id is
        in ``ids`` (int64 on the device, sorted, unique): one elementwise pass
        over the ids column, a binary search per row in the small batch."""
        rows, which = [], []
        m = int(ids.numel())
        for r0 in range(0, self.nv if m else 0, chunk):
            r1 = min(self.nv, r0 + chunk)
            v = self._vids[r0:r1]
            j = torch.searchsorted(ids, v).clamp_(max=m - 1)
            hit = ids[j] == v
            if self._vdead is not None:
                hit &= self._vdead[r0:r1] == 0
            r = torch.nonzero(hit).flatten()
            rows.append(r + r0)
            which.append(j[r])
        if not rows:
            z = torch.zeros(0, dtype=torch.int64, device=self.device)
            return z, z
        return torch.cat(rows), torch.cat(which)

    def remove(self, ids) -> int:
        """Delete the vectors with these ids; ids the index does not hold (or
        no longer holds) are ignored. Lazy: the rows are flagged here and leave
        at the next search. Returns the number of vectors removed."""
        ids = torch.unique(torch.as_tensor(ids, dtype=torch.int64).to(self.device).flatten())
        rows, _ = self._lookup(ids)
        k = int(rows.numel())
        self.order_gen = next(_GEN)
        if k:
            self._flags("_vdead")[rows] = 1
            self._nlive -= k
            self._dirty = True
        return k

    def upsert(self, ids, x: torch.Tensor) -> int:
        """Insert or rewrite: a held id gets its vector re-encoded (its kept
        copy is overwritten in its vector row, its old code row flagged, a new
        code row appended to the tail), an id not held is appended as ``add``
        would. Of a repeated id the last row counts. Returns the number of
        ids that were already held."""
        ids = torch.as_tensor(ids, dtype=torch.int64).to(self.device).flatten()
        assert ids.numel() == x.shape[0]
        self.order_gen = next(_GEN)
        if ids.numel() == 0:
            return 0
        uid, inv = torch.unique(ids, return_inverse=True)
        last = torch.zeros(uid.numel(), dtype=torch.int64, device=self.device)
        last.scatter_reduce_(0, inv, torch.arange(ids.numel(), device=self.device), "amax", include_self=False)
        vrows, j = self._lookup(uid)
        held = torch.zeros(uid.numel(), dtype=torch.bool, device=self.device)
        held[j] = True
        k = int(vrows.numel())
        if k:
            # the code rows (sorted part or tail) that point at these vectors leave
            mark = torch.zeros(self.nv, dtype=torch.uint8, device=self.device)
            mark[vrows] = 1
            cd = self._flags("_cdead")
            cd[: self.n] |= mark[self._pos[: self.n]]
            del mark
            self._append(x.to(self.device)[last[j]], None, vrows)
        new = torch.nonzero(~held).flatten()
        if new.numel():
            self._append(x.to(self.device)[last[new]], uid[new], None)
        return k

    def translate_ids(self, table: torch.Tensor) -> None:
        """Every live id ``i`` becomes ``table[i]``; a negative entry removes
        the vector (a compaction of the caller's id space). ``table``: an
        integer tensor on any device, indexed by the current ids."""
        nv = self.nv
        self.order_gen = next(_GEN)
        if nv == 0:
            return
        t = torch.as_tensor(table).to(self.device, torch.int64).flatten()
        if t.numel() == 0:
            t = torch.full((1,), -1, dtype=torch.int64, device=self.device)
        old = self._vids[:nv]
        new = t[old.clamp(0, int(t.numel()) - 1)]
        live = torch.ones(nv, dtype=torch.bool, device=self.device) if self._vdead is None else self._vdead[:nv] == 0
        gone = live & ((new < 0) | (old < 0) | (old >= t.numel()))
        self._vids[:nv] = torch.where(live & ~gone, new, old)
        k = int(gone.sum())
        if k:
            self._flags("_vdead")[:nv] |= gone.to(torch.uint8)
            self._nlive -= k
            self._dirty = True

    def _finalize_ref(self, chunk: int = 1 << 24) -> None:
        """The torch formulation of :meth:`_finalize` (any device; the CPU
        path and the oracle of the kernel path): the flagged rows are filtered
        out, then the code rows are sorted by list id (CSR) with one stable
        sort and permuted in chunks into one new buffer. The vector rows keep
        their order (``pos`` follows the codes)."""
        n, nv = self.n, self.nv
        self.order_gen = next(_GEN)
        if self._cdead is not None or self._vdead is not None:
            keep = torch.ones(n, dtype=torch.bool, device=self.device)
            if self._cdead is not None:
                keep &= self._cdead[:n] == 0
            if self._vdead is not None:
                keep &= self._vdead[self._pos[:n]] == 0
                vkeep = self._vdead[:nv] == 0
                vremap = torch.cumsum(vkeep, 0) - vkeep.long()
                vi = torch.nonzero(vkeep).flatten()
                nv = int(vi.numel())
                for name in ("_vids", "_vec", "_vscale"):
                    t = getattr(self, name)
                    if t is not None:
                        t[:nv] = t[vi]
            ci = torch.nonzero(keep).flatten()
            n = int(ci.numel())
            self._codes[:n] = self._codes[ci]
            self._list[:n] = self._list[ci]
            p = self._pos[ci]
            self._pos[:n] = vremap[p] if self._vdead is not None else p
            self._cdead = self._vdead = None
            self.n, self.nv = n, nv
        o = torch.argsort(self._list[:n], stable=True)
        codes = torch.empty_like(self._codes)
        for c0 in range(0, n, chunk):
            c1 = min(n, c0 + chunk)
            codes[c0:c1] = self._codes[o[c0:c1]]
        self._codes = codes
        self._list[:n] = self._list[:n][o]
        self._pos[:n] = self._pos[:n][o]
        cnt = torch.bincount(self._list[:n].long(), minlength=self.nlist)
        self.list_off = torch.zeros(self.nlist + 1, dtype=torch.int64, device=self.device)
        self.list_off[1:] = torch.cumsum(cnt, 0)
        self._sorted_n = n
        self._dirty = False

    def _finalize(self, chunk_rows: Optional[int] = None) -> None:
        """Bring the code rows back into CSR order -- amortised over a batch
        of changes. On the GPU (``MAINT_KERNEL``), in place:

        1. flags pending: one pass marks the surviving code rows and counts
           them per list (ivfmaint.hip), the code columns and -- by the vector
           flags -- the vector columns are compacted stably in place
           (compact.hip), ``pos`` follows the vector rows;
        2. a tail smaller than the sorted part: the tail alone is sorted by
           list (O(tail)), the sorted part is spread upwards in place to open
           a gap behind each list (ivfmaint.hip) and the tail rows drop in.

        A first build, or a tail at least as large as the sorted part, takes
        the full stable sort (:meth:`_finalize_ref`), which is also what the
        CPU runs; both leave bit-identical arrays. ``chunk_rows``: rows per
        chunk of the in-place moves (default ``self.chunk_rows``, else
        ops.tenant_ops.rc_chunk_rows)."""
        if not self._dirty:
            return
        self.order_gen = next(_GEN)  # rows are about to move
        if not (self.device.type == "cuda" and MAINT_KERNEL and self._sorted_n > 0):
            return self._finalize_ref()
        from ..ops import ivf_ops as V
        from ..ops import tenant_ops as T
        ch = int(chunk_rows or self.chunk_rows or T.rc_chunk_rows(self.m))
        dev = self.device
        st = self.last_maint = {"bytes_moved": 0, "direct": 0, "bounced": 0}  # of the wide in-place moves

        def tally(r):
            for k, v in zip(("bytes_moved", "direct", "bounced"), r):
                st[k] += v
        if self._cdead is not None or self._vdead is not None:
            n, nv, s0 = self.n, self.nv, self._sorted_n
            assert max(n, nv) < (1 << 31) - 1, "in-place maintenance indexes rows with int32"
            vremap = None
            if self._vdead is not None:
                vkeep = (self._vdead[:nv] == 0).to(torch.uint8)
                vremap = T.rc_remap_of(vkeep)
            keep, cnt = V.ivf_mark_count(self._list[:n], self._pos, self._cdead, self._vdead, self.nlist, s0)
            remap = T.rc_remap_of(keep)
            z = torch.zeros((), dtype=torch.int64, device=dev)
            # (argmin of 0 / 1 flags: the first dead row)
            head = torch.stack([remap[n].long(), remap[s0].long(), keep.argmin(),
                                vremap[nv].long() if vremap is not None else z,
                                vkeep.argmin() if vremap is not None else z])
            m, s1, first, mv, vfirst = (int(v) for v in head.cpu().tolist())
            if vremap is not None and mv < nv:
                wide = [t for t in (self._vec,) if t is not None]
                for t in wide:
                    rb = t.shape[1] * t.element_size()
                    tally(T.rc_move_rows(t, vkeep, vremap, nv, vfirst, int(chunk_rows or self.chunk_rows
                                                                            or T.rc_chunk_rows(rb))))
                T.rc_move_scalars([t for t in (self._vids, self._vscale) if t is not None], vkeep, vremap, nv, mv)
                self.nv = mv
            if m < n:
                tally(T.rc_move_rows(self._codes, keep, remap, n, first, ch))
                T.rc_move_scalars([self._list, self._pos], keep, remap, n, m)
            del keep, remap
            if vremap is not None and mv < nv:
                for c0 in range(0, m, 1 << 22):  # pos follows the vector rows
                    c1 = min(m, c0 + (1 << 22))
                    self._pos[c0:c1] = vremap[self._pos[c0:c1]]
            self.list_off = torch.zeros(self.nlist + 1, dtype=torch.int64, device=dev)
            self.list_off[1:] = torch.cumsum(cnt, 0)
            self.n, self._sorted_n = m, s1
            self._cdead = self._vdead = None
        n, n0 = self.n, self._sorted_n
        tail = n - n0
        if tail and (n0 == 0 or tail >= n0):
            return self._finalize_ref()
        if tail:
            t_codes, t_list, t_pos = self._codes[n0:n].clone(), self._list[n0:n].clone(), self._pos[n0:n].clone()
            order, ins, dest = V.ivf_tail_slots(t_list, self.list_off, self.nlist)
            first = int(self.list_off[int(t_list.min()) + 1])  # the rows of the lists behind the tail's first list
            bounds = V.ivf_spread_bounds(self._list, ins, n0, first, ch)
            bounce = torch.empty(min(ch, max(n0 - first, 0)) * self.m, dtype=torch.uint8, device=dev)
            tally(V.ivf_spread_rows(self._codes, self._list, ins, n0, first, ch, bounds, bounce))
            del bounce
            # the narrow columns through the same kernel, no temporary of their
            # own; the key column last, out of place from a copy of itself
            nb = torch.empty(min(ch, max(n0 - first, 0)) * 8, dtype=torch.uint8, device=dev)
            V.ivf_spread_rows(self._pos, self._list, ins, n0, first, ch, bounds, nb)
            del nb
            if first < n0:
                key = self._list[:n0].clone()
                V.ivf_spread_rows(self._list, key, ins, n0, first, ch, bounds, None, src=key)
                del key
            self._codes[dest] = t_codes[order]
            self._list[dest] = t_list[order]
            self._pos[dest] = t_pos[order]
            self.list_off = self.list_off + ins
        self._sorted_n = n
        self._dirty = False

    def __len__(self) -> int:
        """The live vectors (removed ones leave at once, whatever is pending)."""
        return int(self._nlive)

    def memory_bytes(self) -> int:
        n = self._nlive
        b = n * (self.m + 4 + 8 + 8)  # codes, list id, pos, id
        if self._vec is not None:
            b += n * self._vec.shape[1] * self._vec.element_size()
        return b + (n * 4 if self._vscale is not None else 0)

    # ------------------------------------------------------------------ filter
    def filter_rows(self, allow: torch.Tensor, max_rows: Optional[int] = None, keep_mask: bool = True) -> FilteredLists:
        """The passing code rows of every list (:class:`FilteredLists`).
        ``allow`` is indexed by id: a bool / uint8 tensor (non-zero passes) or
        an fp32 score bias (above -inf passes; a filter plan's bias column as
        it is). An id outside it does not pass -- so ids must be small and
        non-negative, as a TenantGraph's are (ids = rows). ``max_rows``: the
        capacity of the row list (default ``n``, which cannot overflow; a
        caller that knows the passing count may pass it -- were more rows to
        pass, the lists stop at ``max_rows``, nothing is written past it). On
        the GPU three launches and a lower bound per list (ivfpq_filter.hip),
        no host synchronisation; CPU tensors take the torch formulation."""
        self._finalize()
        n = self.n
        a = allow.to(self.device)
        if a.dtype == torch.bool:
            a = a.view(torch.uint8)
        if a.dtype not in (torch.uint8, torch.float32):
            raise TypeError("allow: a bool / uint8 mask or an fp32 bias")
        a = a.flatten().contiguous()
        kind = 1 if a.dtype == torch.float32 else 0
        n_ids = int(a.numel())
        cap = n if max_rows is None else int(max_rows)
        if self.device.type != "cuda":
            if n and n_ids:
                ids = self._vids[self._pos[:n]]
                v = a[ids.clamp(0, n_ids - 1)]
                ok = (ids >= 0) & (ids < n_ids) & ((v > float("-inf")) if kind else (v != 0))
                rows = torch.nonzero(ok).flatten()[:cap]
            else:
                rows = torch.zeros(0, dtype=torch.int64, device=self.device)
            off = torch.searchsorted(rows, self.list_off.contiguous())
            return FilteredLists(rows.to(torch.int32), off.to(torch.int64), self.order_gen,
                                 allow if keep_mask else None, max_rows)
        L = _lib.lib()
        frows = torch.empty(max(cap, 1), dtype=torch.int32, device=self.device)
        foff = torch.empty(self.nlist + 1, dtype=torch.int64, device=self.device)
        ws = torch.empty(max(int(L.lzk_ivfpq_filter_rows_ws(n)), 1), dtype=torch.int32, device=self.device)
        _lib.check(L.lzk_ivfpq_filter_rows(self._pos.data_ptr(), self._vids.data_ptr(), n, a.data_ptr(), kind, n_ids,
                                           self.list_off.data_ptr(), self.nlist, cap, frows.data_ptr(),
                                           foff.data_ptr(), ws.data_ptr(), _lib.stream_ptr(self.device)),
                   "lzk_ivfpq_filter_rows")
        return FilteredLists(frows, foff, self.order_gen, allow if keep_mask else None, max_rows)

    def _lists(self, allow) -> Optional[FilteredLists]:
        """``allow`` of a search as current lists (after ``_finalize``): a
        mask is compacted now; stale lists are rebuilt in place from the mask
        they carry, or refused."""
        if allow is None:
            return None
        if not isinstance(allow, FilteredLists):
            return self.filter_rows(allow)
        if allow.gen != self.order_gen:
            if allow.allow is None:
                raise ValueError("FilteredLists are stale (the index changed since filter_rows) and carry no mask")
            fresh = self.filter_rows(allow.allow, allow.max_rows)
            allow.rows, allow.off, allow.gen = fresh.rows, fresh.off, fresh.gen
        return allow

    # ------------------------------------------------------------------ search
    def search(self, q: torch.Tensor, k: int = 10, nprobe: int = 16, rerank: int = 0, allow=None):
        """Returns (scores fp32 [nq, k], ids int64 [nq, k]). ``rerank`` > 0:
        the best ``rerank`` PQ candidates are re-scored exactly against the
        kept copy (scores then are exact inner products). ``allow`` (a mask
        as :meth:`filter_rows` takes it, or its :class:`FilteredLists`): only
        vectors whose id passes are scanned, ranked and returned."""
        self._finalize()
        fl = self._lists(allow)
        qf = _unit(q.to(self.device).float())
        nq = qf.shape[0]
        nprobe = min(nprobe, self.nlist)
        cs = qf @ self.centroids.T
        coarse, probes = torch.topk(cs, nprobe, dim=1)
        lut = torch.einsum("qmd,mcd->qmc", qf.view(nq, self.m, self.dsub), self.codebooks).contiguous()
        kk = max(k, rerank) if rerank else k
        if self.device.type != "cuda":
            s, rows = self._scan_ref(probes, coarse, lut, kk, fl)
        elif rerank and self._vec is not None and kk > KSLOTS[-1]:
            s, rows = self._scan_candidates(probes.to(torch.int32).contiguous(), coarse.contiguous(), lut, kk, fl)
        elif kk <= KSLOTS[-1]:
            s, rows = self._scan_gpu(probes.to(torch.int32).contiguous(), coarse.contiguous(), lut, kk, fl)
        else:
            s, rows = self._scan_deep(probes.to(torch.int32).contiguous(), coarse.contiguous(), lut, kk, fl)
        if rerank and self._vec is not None:
            vrows = torch.where(rows >= 0, self._pos[rows.clamp_min(0)], torch.full_like(rows, -1))
            if self._rerank_gpu_ok(k) and self._rerank_fits(vrows.shape[1]):
                s, vr = self._rerank_gpu(qf, vrows.contiguous(), k)
            else:
                valid = vrows >= 0
                vv = vrows.clamp_min(0)
                if self._vscale is not None:  # fp8 / int8 copy: dequantise the gathered candidates only
                    dt = torch.int8 if self.keep_vectors == "int8" else torch.float8_e4m3fn
                    v = self._vec[vv].view(dt).float() * self._vscale[vv][..., None]
                else:
                    v = self._vec[vv].float()[..., : self.dim]
                sc = torch.einsum("qd,qkd->qk", qf, v)
                sc = torch.where(valid, sc, torch.full_like(sc, float("-inf")))
                s, o = torch.sort(sc, dim=1, descending=True, stable=True)
                vr = torch.gather(vrows, 1, o)
            s, vr = s[:, :k], vr[:, :k]
            return s, torch.where(vr >= 0, self._vids[vr.clamp_min(0)], torch.full_like(vr, -1))
        s, rows = s[:, :k], rows[:, :k]
        ids = torch.where(rows >= 0, self._vids[self._pos[rows.clamp_min(0)]], torch.full_like(rows, -1))
        return s, ids

    def candidate_ids(self, q: torch.Tensor, R: int, nprobe: int = 16, allow=None) -> torch.Tensor:
        """The ids of the exact PQ top-``R`` rows over the ``nprobe`` probed
        lists per query ([nq, R] int64, -1 padded) -- for a caller that
        re-ranks with its own exact vectors (TenantGraph's fp32 rows).
        ``allow`` as in :meth:`search`: the top-``R`` among passing rows."""
        self._finalize()
        fl = self._lists(allow)
        qf = _unit(q.to(self.device).float())
        nq = qf.shape[0]
        nprobe = min(nprobe, self.nlist)
        coarse, probes = torch.topk(qf @ self.centroids.T, nprobe, dim=1)
        lut = torch.einsum("qmd,mcd->qmc", qf.view(nq, self.m, self.dsub), self.codebooks).contiguous()
        if self.device.type != "cuda":
            _, rows = self._scan_ref(probes, coarse, lut, R, fl)
        elif R <= KSLOTS[-1]:
            _, rows = self._scan_gpu(probes.to(torch.int32).contiguous(), coarse.contiguous(), lut, R, fl)
        else:
            _, rows = self._scan_candidates(probes.to(torch.int32).contiguous(), coarse.contiguous(), lut, R, fl)
        rows = rows.long()
        return torch.where(rows >= 0, self._vids[self._pos[rows.clamp_min(0)]], torch.full_like(rows, -1))

    def _rerank_gpu_ok(self, k: int) -> bool:
        if self.device.type != "cuda" or k > KSLOTS[-1]:
            return False
        w = self._vec.shape[1]
        row_bytes = w if self._vscale is not None else 2 * w
        return row_bytes % 256 == 0

    # rerank_kernel keeps the fp32 query and one fp32 score per candidate in
    # LDS; lzk_rerank refuses more than the CU's 160 KiB
    RERANK_LDS = 160 * 1024

    def _rerank_fits(self, R: int) -> bool:
        """Whether a candidate depth of ``R`` fits the fused re-rank; a deeper
        one goes through the library path of :meth:`search`."""
        return (self._vec.shape[1] + R) * 4 <= self.RERANK_LDS

    def _rerank_gpu(self, qf: torch.Tensor, rows: torch.Tensor, k: int):
        """Fused exact re-rank over the kept copy (csrc/kernels/ivfpq.hip
        rerank_kernel): no dequantised [nq, R, D] intermediate. ``rows`` are
        vector (insertion) rows; returns (scores, vector rows)."""
        nq, R = rows.shape
        fmt = {"fp8": 1, "int8": 2}.get(self.keep_vectors, 0)
        w = self._vec.shape[1]
        Q = torch.zeros((nq, w), dtype=torch.float32, device=self.device)
        Q[:, : qf.shape[1]] = qf
        ks = _kslot(k)
        os_ = torch.empty((nq, k), dtype=torch.float32, device=self.device)
        oi = torch.empty((nq, k), dtype=torch.long, device=self.device)
        ldv = self._vec.stride(0) * self._vec.element_size()
        _lib.check(_lib.lib().lzk_rerank(self._vec.data_ptr(), ldv, fmt, _lib.ptr(self._vscale),
                                         rows.data_ptr(), nq, R, Q.data_ptr(), w, ks, k, os_.data_ptr(),
                                         oi.data_ptr(), _lib.stream_ptr(self.device)), "lzk_rerank")
        return os_, oi

    def _scan_ref(self, probes, coarse, lut, k, fl: Optional[FilteredLists] = None):
        """``fl``: the lists are ``fl.rows[fl.off[l]:fl.off[l + 1]]`` -- here
        and in the three GPU scans below, which then call the ``_f`` kernels."""
        nq = probes.shape[0]
        out_s = torch.full((nq, k), float("-inf"), device=self.device)
        out_r = torch.full((nq, k), -1, dtype=torch.long, device=self.device)
        ar = torch.arange(self.m, device=self.device)
        codes = self.codes
        for qi in range(nq):
            cand_s, cand_r = [], []
            for p in range(probes.shape[1]):
                l = int(probes[qi, p])
                off = self.list_off if fl is None else fl.off
                r0, r1 = int(off[l]), int(off[l + 1])
                if r1 == r0:
                    continue
                rr = torch.arange(r0, r1, device=self.device) if fl is None else fl.rows[r0:r1].long()
                c = codes[rr].long()
                cand_s.append(coarse[qi, p] + lut[qi][ar[None, :], c].sum(1))
                cand_r.append(rr)
            if not cand_s:
                continue
            cs_, cr_ = torch.cat(cand_s), torch.cat(cand_r)
            o = torch.argsort(-cs_, stable=True)[:k]
            out_s[qi, : o.numel()] = cs_[o]
            out_r[qi, : o.numel()] = cr_[o]
        return out_s, out_r

    def _scan_deep(self, probes, coarse, lut, k, fl: Optional[FilteredLists] = None):
        """Deep candidate lists (re-rank depth >> 16): each (query, probed
        list) block emits its waves' best rows (``ivfpq_scan_deep_kernel``,
        4 x 128 per list), then a top-k over the query's nprobe x 512 PQ scores."""
        nq, nprobe = probes.shape
        L = _lib.lib()
        W = L.lzk_ivfpq_deep_width()
        os_ = torch.empty((nq, nprobe * W), dtype=torch.float32, device=self.device)
        oi = torch.empty((nq, nprobe * W), dtype=torch.int32, device=self.device)
        if fl is None:
            _lib.check(L.lzk_ivfpq_scan_deep(self._codes.data_ptr(), self.list_off.data_ptr(), probes.data_ptr(),
                                             coarse.data_ptr(), lut.data_ptr(), nq, nprobe, self.m, os_.data_ptr(),
                                             oi.data_ptr(), _lib.stream_ptr(self.device)), "lzk_ivfpq_scan_deep")
        else:
            _lib.check(L.lzk_ivfpq_scan_deep_f(self._codes.data_ptr(), fl.off.data_ptr(), fl.rows.data_ptr(),
                                               probes.data_ptr(), coarse.data_ptr(), lut.data_ptr(), nq, nprobe,
                                               self.m, os_.data_ptr(), oi.data_ptr(), _lib.stream_ptr(self.device)),
                       "lzk_ivfpq_scan_deep_f")
        kk = min(k, os_.shape[1])
        s, j = torch.topk(os_, kk, dim=1)
        rows = torch.gather(oi, 1, j).long()
        rows = torch.where(torch.isneginf(s), torch.full_like(rows, -1), rows)
        if kk < k:
            s = torch.cat([s, torch.full((nq, k - kk), float("-inf"), device=self.device)], 1)
            rows = torch.cat([rows, torch.full((nq, k - kk), -1, dtype=torch.long, device=self.device)], 1)
        return s, rows

    # threshold-pass buffer: CAND_CAP x the requested depth (at least
    # CAND_MIN): with weak PQ codes a crowded list makes the pooled threshold
    # loose, and everything above it must fit before the PQ top-R is taken
    CAND_CAP = 16
    CAND_MIN = 32768

    def _scan_candidates(self, probes, coarse, lut, R, fl: Optional[FilteredLists] = None):
        """Re-rank candidates: the exact PQ top-R over the probed lists (plus
        ties). Pass 1 (``ivfpq_scan_deep``) pools each list's best rows; the
        R-th best pooled score is a lower bound of the true R-th best; pass 2
        (``ivfpq_scan_thresh``) appends EVERY probed row at or above it, so a
        query whose neighbours crowd into one list still gets all of them.
        Returns (PQ scores, code rows) [nq, R] of the collected rows' PQ
        top-R, -1 padded. With ``fl`` both passes see passing rows only: the
        pooled R-th best passing score bounds the true one from below, and
        the result is the exact PQ top-R among the passing rows."""
        nq, nprobe = probes.shape
        ps, _ = self._scan_deep(probes, coarse, lut, R, fl)
        thr = ps[:, R - 1].contiguous()  # -inf when the pools hold fewer than R rows: take everything
        cap = max(self.CAND_CAP * R, self.CAND_MIN)
        L = _lib.lib()
        cnt = torch.zeros(nq, dtype=torch.int32, device=self.device)
        os_ = torch.empty((nq, cap), dtype=torch.float32, device=self.device)
        oi = torch.empty((nq, cap), dtype=torch.int32, device=self.device)
        if fl is None:
            _lib.check(L.lzk_ivfpq_scan_thresh(self._codes.data_ptr(), self.list_off.data_ptr(), probes.data_ptr(),
                                               coarse.data_ptr(), lut.data_ptr(), thr.data_ptr(), nq, nprobe, self.m,
                                               cap, cnt.data_ptr(), os_.data_ptr(), oi.data_ptr(),
                                               _lib.stream_ptr(self.device)), "lzk_ivfpq_scan_thresh")
        else:
            _lib.check(L.lzk_ivfpq_scan_thresh_f(self._codes.data_ptr(), fl.off.data_ptr(), fl.rows.data_ptr(),
                                                 probes.data_ptr(), coarse.data_ptr(), lut.data_ptr(),
                                                 thr.data_ptr(), nq, nprobe, self.m, cap, cnt.data_ptr(),
                                                 os_.data_ptr(), oi.data_ptr(), _lib.stream_ptr(self.device)),
                       "lzk_ivfpq_scan_thresh_f")
        self.last_candidates = cnt  # per-query count (> cap: overflowed, kept the first cap)
        valid = torch.arange(cap, device=self.device)[None, :] < cnt.clamp(max=cap)[:, None]
        sc = torch.where(valid, os_, torch.full_like(os_, float("-inf")))
        ts, j = torch.topk(sc, min(R, cap), dim=1)
        rows = torch.gather(oi, 1, j).long()
        return ts, torch.where(torch.isneginf(ts), torch.full_like(rows, -1), rows)

    def _scan_gpu(self, probes, coarse, lut, k, fl: Optional[FilteredLists] = None):
        nq, nprobe = probes.shape
        ks = _kslot(k)
        part = nq * nprobe * ks
        ws = _ws.get(self.device, part * 8)
        ps = ws[: part * 4].view(torch.float32)
        pi = ws[part * 4: part * 8].view(torch.int32)
        st = _lib.stream_ptr(self.device)
        L = _lib.lib()
        if fl is None:
            _lib.check(L.lzk_ivfpq_scan(self._codes.data_ptr(), self.list_off.data_ptr(), probes.data_ptr(),
                                        coarse.data_ptr(), lut.data_ptr(), nq, nprobe, self.m, ks, ps.data_ptr(),
                                        pi.data_ptr(), st), "lzk_ivfpq_scan")
        else:
            _lib.check(L.lzk_ivfpq_scan_f(self._codes.data_ptr(), fl.off.data_ptr(), fl.rows.data_ptr(),
                                          probes.data_ptr(), coarse.data_ptr(), lut.data_ptr(), nq, nprobe, self.m,
                                          ks, ps.data_ptr(), pi.data_ptr(), st), "lzk_ivfpq_scan_f")
        os_ = torch.empty((nq, k), dtype=torch.float32, device=self.device)
        oi = torch.empty((nq, k), dtype=torch.long, device=self.device)
        _lib.check(L.lzk_topk_merge(ps.data_ptr(), pi.data_ptr(), nprobe * ks, nq, ks, k, 0, os_.data_ptr(),
                                    oi.data_ptr(), st), "lzk_topk_merge")
        return os_, oi


def recall_at_k(found: torch.Tensor, truth: torch.Tensor) -> float:
    f, t = found.cpu().numpy(), truth.cpu().numpy()
    k = t.shape[1]
    return float(np.mean([len(set(a) & set(b)) / k for a, b in zip(f, t)]))
