"""The per-element bounds of tests/kernels/_encoder_bounds.py are sound and
sharp, shown without a GPU.

Soundness: fp32 / bf16 emulations of the kernels' arithmetic stay within 1.0 x
the bound -- half of what the GPU tier (test_encoder_elementwise_gpu.py)
allows. Sharpness: small localized corruptions of a correctly rounded result
make ``assert_within`` raise at the GPU tier's 2 x bound.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from tests.kernels._encoder_bounds import (GPU_MARGIN, assert_within, attention_bound, layernorm_bound,
                                           linear_bound, pool_norm_bound, split2_bounds, worst_ratio)

BF = torch.bfloat16


def _linear_inputs(T, N, K, res, seed, gelu=False):
    """The inputs of tests/kernels/test_kernels_gpu.py::test_linear."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, K, generator=g).to(BF)
    w = (torch.randn(N, K, generator=g) * 0.05).to(BF)
    b = torch.randn(N, generator=g)
    r = torch.randn(T, N, generator=g).to(BF) if res else None
    return x, w, b, r


def _emulate_linear(x, w, b, act, r, roundings):
    a = x.float() @ w.float().T + b
    if act == "gelu":
        a = F.gelu(a)
    if r is None:
        return a.to(BF)
    if roundings == 1:
        return (a + r.float()).to(BF)
    return (a.to(BF).float() + r.float()).to(BF)


LINEAR_SHAPES = [(300, 768, 768, "none", False), (257, 3072, 768, "gelu", False), (129, 768, 3072, "none", True),
                 (1000, 384, 384, "gelu", True), (1, 768, 768, "gelu", True), (64, 1000, 384, "gelu", False)]


@pytest.mark.parametrize("T,N,K,act,res", LINEAR_SHAPES)
@pytest.mark.parametrize("roundings", [1, 2])
def test_linear_emulation_within_bound(T, N, K, act, res, roundings):
    x, w, b, r = _linear_inputs(T, N, K, res, seed=T + N + K)
    ref, bound = linear_bound(x, w, b, act, r)
    y = _emulate_linear(x, w, b, act, r, roundings)
    worst = assert_within(y, ref, bound, f"linear emulation {T}x{N}x{K} {act} res={res} roundings={roundings}")
    print(f"SOUNDNESS linear T={T} N={N} K={K} {act} res={res} roundings={roundings}: {worst:.3f}")


@pytest.mark.parametrize("T,N,K,res", [(257, 768, 768, True), (300, 1000, 384, False)])
def test_split2_emulation_within_bound(T, N, K, res):
    x, w, b, r = _linear_inputs(T, N, K, res, seed=7 + T)
    (ra, ba), (rb, bb), (rs, bs) = split2_bounds(x, w, b, r)
    h = K // 2
    ya = _emulate_linear(x[:, :h], w[:, :h], b, "none", r, 2)
    yb = (x[:, h:].float() @ w[:, h:].float().T).to(BF)
    wa = assert_within(ya, ra, ba, "split2 ya")
    wb = assert_within(yb, rb, bb, "split2 yb")
    ws = assert_within(ya.double() + yb.double(), rs, bs, "split2 ya + yb")
    print(f"SOUNDNESS split2 T={T} N={N} K={K} res={res}: ya {wa:.3f} yb {wb:.3f} sum {ws:.3f}")


def _emulate_attention(q, k, v, length):
    """Unnormalised bf16 P for the P V product, fp32 row sum (the kernel)."""
    s = (q.float() @ k[:length].float().T) / math.sqrt(q.shape[1])
    p = torch.exp(s - s.max(dim=1, keepdim=True).values)
    l = p.sum(dim=1, keepdim=True)
    return ((p.to(BF).float() @ v[:length].float()) / l).to(BF)


@pytest.mark.parametrize("S,hd,scale", [(70, 32, 1.0), (130, 64, 1.0), (512, 64, 1.0), (130, 64, 4.0), (512, 32, 4.0)])
def test_attention_emulation_within_bound(S, hd, scale):
    g = torch.Generator().manual_seed(S + hd)
    q = (torch.randn(S, hd, generator=g) * scale).to(BF)
    k = (torch.randn(S, hd, generator=g) * scale).to(BF)
    v = torch.randn(S, hd, generator=g).to(BF)
    for length in (1, 33, S):
        ref, bound = attention_bound(q[:length], k, v, length)
        y = _emulate_attention(q[:length], k, v, length)
        worst = assert_within(y, ref, bound, f"attention emulation S={S} hd={hd} len={length} x{scale}")
        print(f"SOUNDNESS attention S={S} hd={hd} len={length} scale={scale}: {worst:.3f}")


def _emulate_layernorm(x, g, b, eps, r, one_pass):
    v = x.float() + (r.float() if r is not None else 0.0)
    H = v.shape[1]
    mean = v.sum(dim=1, keepdim=True) / H
    if one_pass:
        var = (v * v).sum(dim=1, keepdim=True) / H - mean * mean
    else:
        var = ((v - mean) ** 2).sum(dim=1, keepdim=True) / H
    return ((v - mean) * torch.rsqrt(var + eps) * g + b).to(BF)


@pytest.mark.parametrize("H", [128, 260, 768, 1000, 1024])
@pytest.mark.parametrize("row_mean", [0.0, 8.0, 30.0])
@pytest.mark.parametrize("one_pass", [False, True])
def test_layernorm_emulation_within_bound(H, row_mean, one_pass):
    g_ = torch.Generator().manual_seed(H + int(row_mean))
    rows = 33
    x = (torch.randn(rows, H, generator=g_) + row_mean).to(BF)
    r = torch.randn(rows, H, generator=g_).to(BF)
    g = torch.rand(H, generator=g_) + 0.5
    b = torch.randn(H, generator=g_) + torch.linspace(-1.0, 1.0, H)
    for res in (None, r):
        ref, bound = layernorm_bound(x, g, b, 1e-12, res)
        y = _emulate_layernorm(x, g, b, 1e-12, res, one_pass)
        worst = assert_within(y, ref, bound, f"layernorm emulation H={H} mean={row_mean} one_pass={one_pass}")
        print(f"SOUNDNESS layernorm H={H} mean={row_mean} one_pass={one_pass} res={res is not None}: {worst:.3f}")


@pytest.mark.parametrize("H,S,mode", [(128, 512, "mean"), (768, 130, "mean"), (1024, 33, "mean"), (384, 7, "cls")])
def test_pool_norm_emulation_within_bound(H, S, mode):
    g = torch.Generator().manual_seed(H + S)
    B = 3
    x = torch.randn(B * S, H, generator=g).to(BF)
    lens = torch.tensor([1, S, max(1, S // 2)], dtype=torch.int32)
    ref, bound = pool_norm_bound(x, lens, B, S, mode)
    out = torch.empty(B, H)
    for bb in range(B):
        blk = x[bb * S: bb * S + int(lens[bb])].float()
        if mode == "cls":
            s = blk[0]
        else:
            s = torch.zeros(H)
            for t in range(blk.shape[0]):  # sequential fp32 sum, as the kernel
                s = s + blk[t]
            s = s / blk.shape[0]
        out[bb] = s * (1.0 / torch.sqrt((s * s).sum()))
    worst = assert_within(out, ref, bound, f"pool_norm emulation H={H} S={S} {mode}")
    print(f"SOUNDNESS pool_norm H={H} S={S} {mode}: {worst:.3f}")


# ------------------------------------------------------------------ sharpness
def _rel(a, b):
    """The whole-tensor check of tests/kernels/test_kernels_gpu.py."""
    return ((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-6)).item()


def _add_ulps(t, row, col, n):
    bits = t.view(torch.int16)
    bits[row, col] += n
    return t


def _corruptions(y, x, w, b, r):
    T, N = y.shape
    c = y.clone()
    yield "one element off by 8 bf16 ulps", _add_ulps(c, T // 2, N // 3, 8)
    c = y.clone()
    c[T - 1] = y[T - 2]
    yield "last row replaced by the row above", c
    c = y.clone()
    c[:, N - 8:N - 4] = y[:, N - 4:]
    c[:, N - 4:] = y[:, N - 8:N - 4]
    yield "two adjacent 4-column groups swapped", c
    b0 = b.clone()
    b0[N - 4:] = 0
    yield "bias of the last 4 columns zeroed", _emulate_linear(x, w, b0, "none", r, 1)


# The first four corruptions against the suite's whole-tensor check, measured
# with these inputs (T=300 N=768 K=768 / T=129 N=768 K=3072 + residual; the
# correct result has _rel = 0.0017 / 0.0017):
#   one element off by 8 ulps     0.0017 / 0.0017   passes _rel < 1e-2
#   last row = row above          0.065  / 0.118    caught at these T
#   two 4-column groups swapped   0.172  / 0.139    caught
#   bias of last 4 columns zeroed 0.065  / 0.033    caught
# and limited to one token row, as a mishandled last tile would be (the cases
# "... in the last row only" below):
#   groups swapped, last row only 0.0095 / 0.0107   passes / just caught
#   bias zeroed, last row only    0.0041 / 0.0034   passes
# A whole wrong row costs sqrt(2 / T) of the ratio, so it too passes 1e-2 once
# T is workload-sized (T >= 20000), and a wrong column group passes once N is
# (4 of 3072 columns). Every one of them exceeds 2 x the per-element bound,
# by the factors this test prints (4 to 4000 x the unscaled bound).
@pytest.mark.parametrize("T,N,K,res", [(300, 768, 768, False), (129, 768, 3072, True)])
def test_linear_corruptions_are_caught(T, N, K, res):
    x, w, b, r = _linear_inputs(T, N, K, res, seed=T + N + K)
    ref, bound = linear_bound(x, w, b, "none", r)
    y = _emulate_linear(x, w, b, "none", r, 1)
    assert_within(y, ref, GPU_MARGIN * bound, "uncorrupted")
    print(f"SHARPNESS linear T={T} K={K}: correct result _rel={_rel(y, ref):.4f}")
    cases = list(_corruptions(y, x, w, b, r))
    for name, c in list(cases[2:]):  # the same, confined to the last token row
        one = y.clone()
        one[T - 1] = c[T - 1]
        cases.append((name + " in the last row only", one))
    for name, c in cases:
        with pytest.raises(AssertionError, match="exceed the bound"):
            assert_within(c, ref, GPU_MARGIN * bound, name)
        print(f"SHARPNESS linear T={T} K={K} {name}: _rel={_rel(c, ref):.4f} "
              f"worst ratio to the unscaled bound {worst_ratio(c, ref, bound):.1f}")


def test_attention_unmasked_key_is_caught():
    S, hd, length = 70, 64, 33
    g = torch.Generator().manual_seed(5)
    q = torch.randn(S, hd, generator=g).to(BF)
    k = torch.randn(S, hd, generator=g).to(BF)
    v = torch.randn(S, hd, generator=g).to(BF)
    ref, bound = attention_bound(q[:length], k, v, length)
    assert_within(_emulate_attention(q[:length], k, v, length), ref, GPU_MARGIN * bound, "uncorrupted")
    leaked = _emulate_attention(q[:length], k, v, length + 1)  # one key past len takes part
    with pytest.raises(AssertionError, match="exceed the bound"):
        assert_within(leaked, ref, GPU_MARGIN * bound, "one key past len unmasked")
    print(f"SHARPNESS attention one key past len unmasked: worst ratio {worst_ratio(leaked, ref, bound):.1f}")


def test_layernorm_and_pool_corruptions_are_caught():
    g_ = torch.Generator().manual_seed(3)
    rows, H = 17, 768
    x = torch.randn(rows, H, generator=g_).to(BF)
    g = torch.rand(H, generator=g_) + 0.5
    b = torch.randn(H, generator=g_) + torch.linspace(-1.0, 1.0, H)
    ref, bound = layernorm_bound(x, g, b)
    y = _emulate_layernorm(x, g, b, 1e-12, None, False)
    c = y.clone()
    c[rows - 1] = y[rows - 2]
    with pytest.raises(AssertionError, match="exceed the bound"):
        assert_within(c, ref, GPU_MARGIN * bound, "layernorm last row replaced")
    c = _add_ulps(y.clone(), 5, 700, 8)
    with pytest.raises(AssertionError, match="exceed the bound"):
        assert_within(c, ref, GPU_MARGIN * bound, "layernorm one element off by 8 ulps")
    lens = torch.tensor([5, 9], dtype=torch.int32)
    pref, pbound = pool_norm_bound(x[:16], lens, 2, 8, "mean", cu=torch.tensor([0, 5, 14], dtype=torch.int32))
    wrong, _ = pool_norm_bound(x[:16], lens + 1, 2, 8, "mean", cu=torch.tensor([0, 5, 14], dtype=torch.int32))
    with pytest.raises(AssertionError, match="exceed the bound"):
        assert_within(wrong.float(), pref, GPU_MARGIN * pbound, "pool_norm one row too many")


def test_assert_within_reports_and_requires_finite():
    ref = torch.zeros(4, 6, dtype=torch.float64)
    bound = torch.full((4, 6), 1e-3, dtype=torch.float64)
    y = torch.zeros(4, 6)
    assert assert_within(y, ref, bound, "exact") == 0.0
    y[2, 5] = 0.5
    y[3, 0] = 0.002
    with pytest.raises(AssertionError, match=r"2 of 24 elements exceed the bound; worst ratio 500 at \(row 2, col 5\)"):
        assert_within(y, ref, bound, "two over")
    y[2, 5] = float("nan")
    with pytest.raises(AssertionError, match="non-finite"):
        assert_within(y, ref, bound, "nan")
    y[2, 5] = float("inf")
    with pytest.raises(AssertionError, match="non-finite"):
        assert_within(y, ref, torch.full_like(bound, float("inf")), "inf under an infinite bound")
