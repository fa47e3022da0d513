"""``flat_topk_i8`` with the int8 threshold sample (``search.I8_SAMPLE``, the
default) against the same search with the bf16 lane-kernel sample (the knob
off) and against ``_ref_topk``: the sample only places the scan threshold, so
(scores, rows) must be IDENTICAL between the two arms -- same re-score kernel,
same select -- on

* 65,536 x 256 random unit rows, 257 queries (the persistent 256 x 256 scan,
  S = 64, speculative threshold on), k = 10, L2 (alpha = 2, bias = -|x|^2);
* the same store, 3 queries (the narrow scan);
* the same store as a lean tenant (``LeanRows``: fp32 rows, no bf16 copy);
* 4,096 x 128 all-equal rows (S = 16; 40 queries with the narrow list capacity
  lowered so that every list overflows, and 130 queries; ties by row).

Against ``_ref_topk`` (fp32 torch matmul of the same bf16 values): both sides
carry fp32 accumulation error <= gamma = (D + 3) 2^-24 (alpha |q| |x| + |b|)
<= 259 * 2^-24 * 3 = 4.7e-5 here, so scores agree within 2 gamma and rows
wherever the reference's scores of ranks 1 .. k + 1 are more than 2 gamma apart
on both sides of the rank (closer pairs may swap). Neighbouring scores near
rank 10 of 65,536 rows are ~sigma / (z * rank) = 0.125 / 40 = 3e-3 apart, so a
gap is under 2 gamma = 9.4e-5 with probability ~3 % and a rank is unsettled
with ~6 %: the comparison must cover at least 85 % of the ranks.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from lazzaro_amd.ops import search as S  # noqa: E402

DEV = "cuda"
K = 10
ALPHA = 2.0


def _unit(gen, n, d):
    v = torch.randn(n, d, device=DEV, generator=gen)
    return (v / v.norm(dim=1, keepdim=True)).to(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def _store(kind):
    gen = torch.Generator(device=DEV).manual_seed(1234)
    if kind == "equal":
        D = 128
        Q16 = _unit(gen, 130, D)
        X16 = Q16[:1].repeat(4096, 1).contiguous()
    else:
        D = 256
        X16 = _unit(gen, 65536, D)
        Q16 = _unit(gen, 257, D)
    bias = -(X16.float() ** 2).sum(1).contiguous()
    X8, rs = S.quantize_i8_rows(X16)
    sumsq = (X16.double() ** 2).sum(0).contiguous()
    smax = rs.max().reshape(1).contiguous()
    xn = float(X16.float().norm(dim=1).max()) + 2.0 ** -7
    return X16, Q16, bias, X8, rs, sumsq, smax, xn


def _search(kind, nq, lean, i8_sample, monkeypatch):
    X16, Q16, bias, X8, rs, sumsq, smax, xn = _store(kind)
    Q16 = Q16[:nq].contiguous()
    N, D = X16.shape
    q8, qs, margin, mr = S.i8_query(Q16, D, sumsq, N, smax, ALPHA, 3.0, xn)
    rows_op = X16
    if lean:
        X32, Q32 = X16.float().contiguous(), Q16.float().contiguous()
        w = ALPHA * 2.0 ** -8 * Q32.norm(dim=1) * xn
        margin, mr = (margin + w).contiguous(), (mr + w).contiguous()
        rows_op = S.LeanRows(X32, D, Q32)
    monkeypatch.setattr(S, "I8_SAMPLE", i8_sample)
    s, r = S.flat_topk_i8(X8, rs, q8, qs, rows_op, Q16, K, bias=bias, alpha=ALPHA, margin=margin, margin_rig=mr)
    torch.cuda.synchronize()
    return s, r


def _both(kind, nq, lean, monkeypatch):
    old = _search(kind, nq, lean, False, monkeypatch)
    new = _search(kind, nq, lean, True, monkeypatch)
    assert torch.equal(new[1], old[1]), torch.nonzero((new[1] != old[1]).any(1)).flatten()[:8]
    assert torch.equal(new[0], old[0])
    return new


def _against_ref(kind, nq, s, r):
    X16, Q16, bias = _store(kind)[:3]
    D = X16.shape[1]
    e_s, e_r = S._ref_topk(X16, Q16[:nq], K + 1, bias, alpha=ALPHA)
    gamma = (D + 3) * 2.0 ** -24 * 3.0
    assert float((s - e_s[:, :K]).abs().max()) <= 2 * gamma
    gap = e_s[:, :-1] - e_s[:, 1:]
    clear = gap > 2 * gamma
    clear[:, 1:] &= clear[:, :-1].clone()  # a rank is settled when the gaps on both its sides are
    print(f"{kind} nq={nq}: {int((~clear).sum())} of {clear.numel()} ranks within 2 gamma of a neighbour")
    assert int((~clear).sum()) <= 0.15 * clear.numel()
    assert torch.equal(r[clear], e_r[:, :K][clear])


def test_wide_batch_identical_to_the_bf16_sample_gpu(monkeypatch):
    s, r = _both("unit", 257, False, monkeypatch)
    _against_ref("unit", 257, s, r)


def test_narrow_batch_identical_gpu(monkeypatch):
    s, r = _both("unit", 3, False, monkeypatch)
    _against_ref("unit", 3, s, r)


def test_lean_tenant_identical_gpu(monkeypatch):
    _both("unit", 257, True, monkeypatch)


@pytest.mark.parametrize("nq", [40, 130])
def test_all_equal_rows_ties_and_overflow_gpu(nq, monkeypatch):
    monkeypatch.setattr(S, "NARROW_CAP", 2048)  # the narrow lists (nq = 40) overflow at 4,096 equal rows
    s, r = _both("equal", nq, False, monkeypatch)
    want = torch.arange(K, device=DEV).expand(nq, -1)
    assert torch.equal(r, want)  # ties resolve by row
