"""References of the filtered IVF-PQ kernels: ``lzk_ivfpq_filter_rows``
(csrc/kernels/ivfpq_filter.hip) and the ``_f`` forms of the three scans
(csrc/kernels/ivfpq.hip). Plain numpy on top of ``_ivfpq_ref``; nothing here
touches a GPU or the kernel library.

A filtered scan is the unfiltered one over the compacted code array
``codes[frows]`` with the filtered offsets ``foff`` as its list layout, its
rows mapped back through ``frows``. ``frows`` ascends, so position order in
the compacted array is code-row order: ties still rank (score desc, code row
asc), and the deep scan's thread ownership -- position modulo 256 within the
list -- is that of the compacted list, as the kernel's.
"""
from __future__ import annotations

import numpy as np

from tests.kernels import _ivfpq_ref as R

KIND_U8, KIND_BIAS = 0, 1


def passes(ids: np.ndarray, allow: np.ndarray, allow_kind: int) -> np.ndarray:
    """Per id: inside ``allow`` and its entry passes (uint8: non-zero; fp32
    bias: above -inf)."""
    ids = np.asarray(ids, dtype=np.int64)
    n_ids = allow.shape[0]
    ok = (ids >= 0) & (ids < n_ids)
    if n_ids == 0:
        return ok
    v = allow[np.clip(ids, 0, n_ids - 1)]
    return ok & ((v > -np.inf) if allow_kind == KIND_BIAS else (v != 0))


def filter_rows_ref(pos, vids, allow, allow_kind: int, list_off, max_rows=None):
    """``lzk_ivfpq_filter_rows``: (frows int32 -- the passing code rows in
    ascending order, cut at ``max_rows`` --, foff int64 [nlist + 1] -- the
    number of passing rows below ``list_off[l]``, at most ``max_rows`` --,
    the uncut count)."""
    pos, vids = np.asarray(pos, dtype=np.int64), np.asarray(vids, dtype=np.int64)
    rows = np.nonzero(passes(vids[pos], np.asarray(allow), allow_kind))[0]
    count = rows.shape[0]
    cap = count if max_rows is None else int(max_rows)
    foff = np.minimum(np.searchsorted(rows, np.asarray(list_off, dtype=np.int64), side="left"), cap).astype(np.int64)
    return rows[:cap].astype(np.int32), foff, count


def lists_of_mask(mask: np.ndarray, list_off):
    """(frows, foff) of a boolean mask over the code rows themselves."""
    n = mask.shape[0]
    fr, fo, _ = filter_rows_ref(np.arange(n), np.arange(n), mask.astype(np.uint8), KIND_U8, list_off)
    return fr, fo


def _back(rows: np.ndarray, frows: np.ndarray) -> np.ndarray:
    fr = np.asarray(frows, dtype=np.int64)
    if fr.shape[0] == 0:
        return rows
    return np.where(rows >= 0, fr[np.maximum(rows, 0)], -1)


def scan_f_ref(codes, foff, frows, probes, coarse, lut, K: int):
    S, Rw = R.scan_ref(codes[np.asarray(frows, dtype=np.int64)], foff, probes, coarse, lut, K)
    return S, _back(Rw, frows)


def deep_f_ref(codes, foff, frows, probes, coarse, lut, width: int):
    S, Rw = R.deep_ref(codes[np.asarray(frows, dtype=np.int64)], foff, probes, coarse, lut, width)
    return S, _back(Rw, frows)


def thresh_f_ref(codes, foff, frows, probes, coarse, lut, thr):
    fr = np.asarray(frows, dtype=np.int64)
    return [(fr[r] if r.size else r, s) for r, s in R.thresh_ref(codes[fr], foff, probes, coarse, lut, thr)]
