"""The int8 threshold sample (ops.search ``sample_topk_i8``, search.hip
``sample_topk_i8_kernel``) against an exact CPU reference: the int64 dot of
the int8 operands, then the scan's two fp32 operations rounded once each,
``p = fl(float(sum) * rs)`` and ``score = fma(alpha * qs, p, bias)``. The
``kslot`` scores per query must be bit-equal to the reference's, the rows equal
((score desc, row asc): the kernel's documented order, so also wherever a
score is not unique in its list), padding (-inf, -1).

Shapes: N = 64 * 293 rows at stride S = 64 (two full 128-row sample tiles plus
a ragged 37), nq = 130 (one full 128-query tile plus 2), Dp = 128 (d = 100,
zero padded) and 768, kslot = 16, with and without bias, one zero query
(qs = 0), each with the default chunking (one tile per chunk) and with all
three tiles in ONE chunk (the double-buffered per-row operands); a store with
fewer sample rows than kslot (N = 64 * 9 + 5: 10 sample rows); S = 1.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from lazzaro_amd.ops import search as S  # noqa: E402

DEV = "cuda"
KSLOT = 16
ALPHA = 2.0
F32, F64 = np.float32, np.float64


def _fma32(a, b, c):
    """fl32(a * b + c) with ONE rounding, for fp32 arrays: the product is exact
    in fp64 (48 bits), the fp64 sum is rounded to odd (TwoSum gives the sign of
    what the sum dropped), and 53 >= 24 + 2 bits make the final rounding to
    fp32 the correct one."""
    prod = a.astype(F64) * b.astype(F64)
    c = np.broadcast_to(c.astype(F64), prod.shape)
    with np.errstate(invalid="ignore", over="ignore"):
        r = prod + c
        bb = r - prod
        e = (prod - (r - bb)) + (c - bb)
        fix = np.isfinite(r) & np.isfinite(e) & (e != 0) & ((r.view(np.int64) & 1) == 0)
        other = np.nextafter(r, np.where(e > 0, np.inf, -np.inf))
    return np.where(fix, other, r).astype(F32)


@functools.lru_cache(maxsize=None)
def _case(N, stride, Dp, d, has_bias):
    """Operands and the reference (scores fp32 [nq, KSLOT], rows [nq, KSLOT])."""
    rng = np.random.default_rng(N * 7 + stride * 3 + Dp + d + int(has_bias))
    nq = 130
    X8 = np.zeros((N, Dp), dtype=np.int8)
    X8[:, :d] = rng.integers(-127, 128, size=(N, d), dtype=np.int8)
    Q8 = np.zeros((nq, Dp), dtype=np.int8)
    Q8[:, :d] = rng.integers(-127, 128, size=(nq, d), dtype=np.int8)
    rs = rng.uniform(0.5, 1.5, N).astype(F32) / F32(127.0)
    qs = rng.uniform(0.5, 1.5, nq).astype(F32) / F32(127.0)
    qs[7] = 0.0  # a zero query
    bias = (-rng.uniform(0.5, 1.5, N)).astype(F32) if has_bias else None
    rows = np.arange(0, N, stride)
    dot = Q8.astype(np.int64) @ X8[rows].astype(np.int64).T  # [nq, ns], exact
    assert np.abs(dot).max() < 2 ** 24
    p = dot.astype(F32) * rs[rows][None, :]                  # fl(float(sum) * rs)
    al = (F32(ALPHA) * qs)[:, None]
    b = bias[rows][None, :] if has_bias else np.zeros((1, rows.size), dtype=F32)
    sc = _fma32(np.broadcast_to(al, p.shape), p, b)
    order = np.argsort(-sc.astype(F64), axis=1, kind="stable")[:, :KSLOT]  # (score desc, row asc)
    e_s = np.take_along_axis(sc, order, 1)
    e_r = rows[order]
    pad = KSLOT - e_s.shape[1]
    if pad > 0:
        e_s = np.concatenate([e_s, np.full((nq, pad), -np.inf, dtype=F32)], 1)
        e_r = np.concatenate([e_r, np.full((nq, pad), -1, dtype=e_r.dtype)], 1)
    return X8, rs, Q8, qs, bias, e_s, e_r


def _run(N, stride, Dp, d, has_bias, n_chunks=None):
    X8, rs, Q8, qs, bias, e_s, e_r = _case(N, stride, Dp, d, has_bias)
    t = lambda a: torch.from_numpy(a).to(DEV) if a is not None else None  # noqa: E731
    s, r = S.sample_topk_i8(t(X8), t(rs), t(Q8), t(qs), KSLOT, stride, bias=t(bias), alpha=ALPHA, n_chunks=n_chunks)
    torch.cuda.synchronize()
    s, r = s.cpu().numpy(), r.cpu().numpy()
    assert s.shape == e_s.shape and s.dtype == F32 and r.dtype == np.int64
    bad = np.flatnonzero((s.view(np.int32) != e_s.view(np.int32)).any(1))
    assert bad.size == 0, (bad[:8], s[bad[:1]], e_s[bad[:1]])
    # rows wherever the score is unique in the query's list ...
    uniq = np.ones_like(e_s, dtype=bool)
    uniq[:, 1:] &= e_s[:, 1:] != e_s[:, :-1]
    uniq[:, :-1] &= e_s[:, :-1] != e_s[:, 1:]
    assert np.array_equal(r[uniq], e_r[uniq])
    # ... and, by the kernel's (score desc, row asc) order, everywhere else too
    assert np.array_equal(r, e_r), np.flatnonzero((r != e_r).any(1))[:8]
    return s, r


@pytest.mark.parametrize("n_chunks", [None, 1])
@pytest.mark.parametrize("has_bias", [False, True])
@pytest.mark.parametrize("Dp,d", [(128, 100), (768, 768)])
def test_sample_scores_are_the_scans_bit_for_bit_gpu(Dp, d, has_bias, n_chunks):
    s, r = _run(64 * 293, 64, Dp, d, has_bias, n_chunks)
    assert (r % 64 == 0).all() and np.isfinite(s).all()
    if not has_bias:  # the zero query: every score 0, the 16 first sample rows
        assert (s[7] == 0).all() and np.array_equal(r[7], 64 * np.arange(KSLOT))


@pytest.mark.parametrize("has_bias", [False, True])
def test_fewer_sample_rows_than_kslot_pads_gpu(has_bias):
    s, r = _run(64 * 9 + 5, 64, 128, 100, has_bias)
    assert (s[:, 10:] == -np.inf).all() and (r[:, 10:] == -1).all() and (r[:, :10] >= 0).all()


@pytest.mark.parametrize("has_bias", [False, True])
def test_stride_one_is_every_row_gpu(has_bias):
    _run(293, 1, 128, 100, has_bias)
