"""Boosted store search: the per-row score prior written into a bias column
(csrc/kernels/boost.hip ``lzk_tg_boost_bias``) and its torch formulation.

The contract of ``boost=`` (``core.boost.MemoryBoost``; the fp64 oracle is
tests/kernels/_boost_ref.py):

1. **Prior.** Per row ``r``, in fp64, in exactly this order, no contraction::

       B(r) = ((w_sal * (double)sal[r] + w_freq * fmin(1, (double)acc[r] / 10))
               + w_rec * (1 / (1 + fmax(0, now - t[r]) / scale))) + tw[tcode[r]]

   ``t`` is ``last_accessed`` (clock ``"accessed"``) or ``timestamp``
   (``"created"``); ``tw`` is the weight of the row's type (0 for every row
   when no type weights are given). ``fmin`` / ``fmax`` are IEEE: a NaN clock
   reads as age 0. ``prior(r) = (float)(c * B(r))``, rounded once, with
   ``c = 2`` for ``l2`` and ``c = 1`` for ``ip`` and ``cosine`` -- on unit rows
   and a unit query one unit of boost then trades against one unit of cosine
   under every metric (-|q - x|^2 = 2 cos - 2). A prior that is not finite (a
   NaN or infinite salience, an fp32 overflow) counts as 0, so no NaN ever
   reaches a scan.
2. **Column.** ``out[r] = base[r] + prior(r)``, one fp32 add, where
   ``kind[r] == NODE``; ``-inf`` for every other row; a ``-inf`` base stays
   ``-inf``. ``base`` is the store bias, or under ``where=`` the filter plan's
   bias. A boosted search therefore returns memories only, as every filtered
   search does: ghost rows take no slot and ``node_rows`` changes nothing.
3. **Result.** The ``limit`` rows with the largest ``metric score + prior``
   among all eligible rows, descending, ties to the lower graph row, (-inf,
   -1) once rows run out. The score returned is that sum, exactly what the
   store re-rank computes with the boosted column as its bias: every scan
   stage scores ``alpha <q, x> + bias[row]`` with an arbitrary fp32 bias (the
   threshold sample, the int8 prefilter's quad bound, the bf16 re-score, the
   error margins bound the dot product only), so the column is exact on every
   flat route and through the int8 certificate. ``boost=None`` runs the plain
   code; a boost whose weights are all 0 returns, bit for bit, what
   ``where=MemoryFilter()`` returns.
4. **Composition.** With ``where=``, ``base`` is the plan's bias and its row
   list serves the indexed route unchanged. With ``diversity=`` the pool is
   the boosted search at ``fetch_k``; with ``expand=`` the seeds are the
   boosted search at ``seed_k``; in both the prior only decides the pool or the
   seeds -- MMR's relevance and the expansion's blend stay cosine.

Device tensors always take the kernel; CPU tensors take ``boost_bias_ref``
(the CPU tier). IEEE fp64 makes the kernel, the torch form and the numpy oracle
agree bit for bit on any input.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import torch

from . import _lib

NEG_INF = float("-inf")
NODE = 1  # (engine.tenant_graph NODE: the kind of a graph node)
FLT_MAX = 3.4028234663852886e38

_lib.register("lzk_tg_boost_bias", _lib.I, [_lib.P, _lib.P, _lib.P, _lib.P, _lib.P, _lib.P, _lib.P, _lib.L,
                                            _lib.D, _lib.D, _lib.D, _lib.D, _lib.D, _lib.D, _lib.P, _lib.P])


def metric_scale(metric: str) -> float:
    """``c`` of the contract: 2 for L2 scores, 1 for IP and cosine."""
    return 2.0 if metric == "l2" else 1.0


def boost_bias_ref(base: torch.Tensor, sal: torch.Tensor, acc: torch.Tensor, t: torch.Tensor, kind: torch.Tensor,
                   n: int, w_sal: float, w_freq: float, w_rec: float, scale: float, now: float, c: float,
                   tcode: Optional[torch.Tensor] = None, tw: Optional[Sequence[float]] = None) -> torch.Tensor:
    """Torch formulation of :func:`boost_bias` (any device): the same fp64
    operations in the same order, one tensor op each (nothing to contract)."""
    dev = base.device
    d = torch.float64
    one = torch.ones((), dtype=d, device=dev)
    f = torch.fmin(one, acc[:n].to(d) / torch.tensor(10.0, dtype=d, device=dev))
    age = torch.fmax(torch.zeros((), dtype=d, device=dev), float(now) - t[:n].to(d))
    rec = one / (one + age / torch.tensor(float(scale), dtype=d, device=dev))
    B = (float(w_sal) * sal[:n].to(d) + float(w_freq) * f) + float(w_rec) * rec
    if tw is not None:
        B = B + torch.as_tensor(list(tw), dtype=d).to(dev)[tcode[:n].long()]
    else:
        B = B + 0.0
    p = (float(c) * B).to(torch.float32)
    p = torch.where(p.abs() <= FLT_MAX, p, torch.zeros_like(p))
    out = base[:n] + p
    return torch.where(kind[:n] == NODE, out, torch.full_like(out, NEG_INF)).contiguous()


def boost_bias(base: torch.Tensor, sal: torch.Tensor, acc: torch.Tensor, t: torch.Tensor, kind: torch.Tensor,
               n: int, w_sal: float, w_freq: float, w_rec: float, scale: float, now: float, c: float,
               tcode: Optional[torch.Tensor] = None, tw: Optional[Sequence[float]] = None) -> torch.Tensor:
    """The boosted bias column over rows [0, n) (boost.hip
    ``lzk_tg_boost_bias``): ``base`` fp32 (the store bias or a filter plan's),
    ``sal`` fp32, ``acc`` int32, ``t`` fp64 (the clock column), ``kind`` uint8,
    optionally ``tcode`` uint8 with ``tw``, 256 weights by type code. Returns
    a new fp32 [n] tensor; ``base`` is not written. One launch on the current
    stream, no host synchronisation. The kernel takes 16-byte loads when every
    pointer is aligned for them and 4-byte ones otherwise (a ``base`` that is
    a view starting inside a buffer), with the same result."""
    n = int(n)
    if base.device.type != "cuda":
        return boost_bias_ref(base, sal, acc, t, kind, n, w_sal, w_freq, w_rec, scale, now, c, tcode, tw)
    dev = base.device
    assert base.dtype == torch.float32 and sal.dtype == torch.float32 and acc.dtype == torch.int32
    assert t.dtype == torch.float64 and kind.dtype == torch.uint8
    for col in (base, sal, acc, t, kind):
        assert col.numel() >= n and col.is_contiguous() and col.device == dev
    tab = None
    if tw is not None:
        assert tcode is not None and tcode.dtype == torch.uint8 and tcode.numel() >= n and tcode.is_contiguous()
        assert len(tw) == 256
        tab = (C.c_double * 256)(*[float(w) for w in tw])
    else:
        tcode = None
    out = torch.empty(n, dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().lzk_tg_boost_bias(base.data_ptr(), sal.data_ptr(), acc.data_ptr(), t.data_ptr(),
                                            kind.data_ptr(), _lib.ptr(tcode),
                                            C.cast(tab, C.c_void_p) if tab is not None else None, n,
                                            float(w_sal), float(w_freq), float(w_rec), float(scale), float(now),
                                            float(c), out.data_ptr(), _lib.stream_ptr(dev)), "lzk_tg_boost_bias")
    return out
