"""numpy oracle of the bias columns of a served round (``lzk_mt_bias``; the
contract is the docstring of lazzaro_amd/ops/mt_bias_ops.py). Written from
the contract, not from the kernel: plain numpy, one IEEE operation per call,
nothing of the package imported. The prior is tests/kernels/_boost_ref.py's.

    base(r) = job has a filter ? (pass(r) ? (l2 ? 0.0f - sqn[r] : 0.0f) : -inf)
                               : store_bias[r]
    out(r)  = job has a boost  ? (kind[r] == NODE ? base(r) + prior(r) : -inf)
                               : base(r)

``pass(r)``: ``kind == NODE`` and ``stored == 1`` and every test that is set
(``None`` = not set) -- super-node mode, type codes, shard codes (a code < 0
passes iff ``neg_shard_pass``; a code past the set fails), ``min_sal <= sal <=
max_sal`` in fp32, ``since <= ts < until`` and ``last >= accessed_since`` in
fp64, ``acc >= min_acc``, row not excluded. A comparison with a NaN is false,
so a NaN salience fails a salience test.
"""
from __future__ import annotations

import numpy as np

from tests.kernels._boost_ref import boost_column_ref

NEG_INF = float("-inf")
NODE = 1


def pass_ref(cols, n: int, pred) -> np.ndarray:
    """bool [n]. ``cols``: numpy columns sal, acc, last, ts, shard, kind, sup,
    stored, tcode; ``pred``: an object with the fields of
    ``ops.filter_ops.Predicate``."""
    c = {k: np.asarray(v)[:n] for k, v in cols.items() if v is not None}
    p = (c["kind"] == NODE) & (c["stored"] == 1)
    if pred.sup_mode >= 0:
        p &= (c["sup"] != 0) == bool(pred.sup_mode)
    if pred.type_codes is not None:
        p &= np.isin(c["tcode"], np.asarray(sorted(pred.type_codes), dtype=np.int64))
    if pred.shard_codes is not None:
        sh = c["shard"].astype(np.int64)
        inset = np.isin(sh, np.asarray(sorted(pred.shard_codes), dtype=np.int64))
        p &= np.where(sh < 0, bool(pred.neg_shard_pass), inset)
    with np.errstate(invalid="ignore"):
        if pred.min_sal is not None:
            p &= c["sal"].astype(np.float32) >= np.float32(pred.min_sal)
        if pred.max_sal is not None:
            p &= c["sal"].astype(np.float32) <= np.float32(pred.max_sal)
        if pred.since is not None:
            p &= c["ts"] >= np.float64(pred.since)
        if pred.until is not None:
            p &= c["ts"] < np.float64(pred.until)
        if pred.accessed_since is not None:
            p &= c["last"] >= np.float64(pred.accessed_since)
    if pred.min_acc is not None:
        p &= c["acc"] >= int(pred.min_acc)
    if pred.exclude_rows is not None:
        ex = np.zeros(n, dtype=bool)
        rows = [r for r in pred.exclude_rows if 0 <= r < n]
        ex[rows] = True
        p &= ~ex
    return p


def column_ref(cols, n: int, pred=None, l2: bool = True, sqn=None, store_bias=None, boost=None, tw=None,
               c: float = 2.0) -> np.ndarray:
    """fp32 [n]: ``out(r)`` above. ``boost``: an object with ``salience``,
    ``frequency``, ``recency``, ``recency_scale``, ``clock``, ``now``; ``tw``:
    256 weights by type code or None."""
    if pred is not None:
        ok = np.zeros(n, dtype=np.float32)
        if l2:
            ok = (np.float32(0.0) - np.asarray(sqn, dtype=np.float32)[:n]).astype(np.float32)
        base = np.where(pass_ref(cols, n, pred), ok, np.float32(NEG_INF)).astype(np.float32)
    else:
        base = np.asarray(store_bias, dtype=np.float32)[:n].copy()
    if boost is None:
        return base
    t = np.asarray(cols["last" if boost.clock == "accessed" else "ts"])[:n]
    with np.errstate(all="ignore"):
        return boost_column_ref(base, np.asarray(cols["sal"])[:n], np.asarray(cols["acc"])[:n], t,
                                np.asarray(cols["kind"])[:n], boost.now, boost.salience, boost.frequency,
                                boost.recency, boost.recency_scale, c,
                                np.asarray(cols["tcode"])[:n] if tw is not None else None, tw)


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def job_column_ref(job) -> np.ndarray:
    """:func:`column_ref` of an ``ops.mt_bias_ops.MtBiasJob`` (its tensors
    copied to the host)."""
    cols = {k: _np(v) for k, v in job.cols.items()}
    cols["tcode"] = _np(job.tcode)
    return column_ref(cols, int(job.n), job.pred, job.l2, _np(job.sqn), _np(job.store_bias), job.boost, job.tw, job.c)
