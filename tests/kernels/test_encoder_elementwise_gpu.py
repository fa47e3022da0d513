"""Every encoder kernel (csrc/kernels/encoder.hip) against an fp64 reference,
element by element, on every GEMM dispatch path.

Each case checks 100 % of the output at 2 x the derived per-element bound
(tests/kernels/_encoder_bounds.py) and, where the op takes leading dimensions,
runs on sub-views of larger buffers whose untouched part must keep a sentinel
bit pattern. The non-default GEMM variants are reached through the library's
setters, which are restored in a ``finally``. Each test prints the worst ratio
to the unscaled bound it saw (``pytest -s``)."""
import contextlib
import ctypes
import math
import zlib

import pytest
import torch

pytestmark = pytest.mark.gpu

from lazzaro_amd.ops import _lib  # noqa: E402
from lazzaro_amd.ops import encoder_ops as E  # noqa: E402

from ._encoder_bounds import (GPU_MARGIN, assert_within, attention_layer_bound, embed_ln_bound,  # noqa: E402
                              layernorm_bound, linear_bound, pool_norm_bound, split2_bounds)

DEV = "cuda"
BF = torch.bfloat16
SETTERS = ("staging", "gemm_tile", "g256_body", "g256_persist", "g256_tail", "g256_min_n", "g256_min_tiles")


@contextlib.contextmanager
def variant(**settings):
    """Select GEMM dispatch variants (lzk_set_<name>); every setter is back at
    its default (-1) afterwards, also when the body raises."""
    L = _lib.lib()
    fns = {}
    for name in SETTERS:
        fn = getattr(L, "lzk_set_" + name)
        fn.argtypes = [ctypes.c_int]
        fn.restype = None
        fns[name] = fn
    try:
        for name, value in settings.items():
            fns[name](value)
        yield
    finally:
        for fn in fns.values():
            fn(-1)


def _gen(*key):
    return torch.Generator(device=DEV).manual_seed(zlib.crc32(repr(key).encode()))


def _sentinel(rows, cols):
    """A finite bf16 bit pattern (values in [2, 8)) that no kernel output repeats."""
    i = torch.arange(rows * cols, device=DEV, dtype=torch.int64)
    bits = (0x4000 + (i * 7919) % 251).to(torch.int16)
    return bits.view(BF).view(rows, cols)


def _strided(t, ld_extra, col0=8, rows_extra=3):
    """``t`` copied into a column / row sub-view of a larger buffer."""
    rows, cols = t.shape
    buf = torch.zeros((rows + rows_extra, cols + ld_extra), dtype=t.dtype, device=t.device)
    buf += 3  # whatever lies around the operand is finite and not zero
    view = buf[:rows, col0:col0 + cols]
    view.copy_(t)
    assert view.data_ptr() % 16 == 0 and view.stride(0) == cols + ld_extra
    return view


class Out:
    """[rows, cols] bf16 output view inside a sentinel-filled buffer."""

    def __init__(self, rows, cols, ld_extra=8, rows_extra=3):
        self.buf = _sentinel(rows + rows_extra, cols + ld_extra)
        self.want = self.buf.clone()
        self.view = self.buf[:rows, :cols]
        self.outside = torch.ones(self.buf.shape, dtype=torch.bool, device=DEV)
        self.outside[:rows, :cols] = False

    def assert_outside_untouched(self, what):
        same = self.buf.view(torch.int16) == self.want.view(torch.int16)
        bad = (~same) & self.outside
        if bool(bad.any()):
            first = bad.nonzero()[0].tolist()
            raise AssertionError(f"{what}: {int(bad.sum())} elements outside the output were overwritten, "
                                 f"first at buffer (row {first[0]}, col {first[1]})")


class Tally:
    def __init__(self, name):
        self.name, self.worst, self.cases, self.failures = name, 0.0, 0, []

    def run(self, what, fn):
        self.cases += 1
        try:
            self.worst = max(self.worst, fn())
        except AssertionError as e:
            self.failures.append(f"{what}: {e}")

    def finish(self):
        print(f"RATIO {self.name}: worst ratio to the unscaled bound {self.worst:.3f} over {self.cases} cases")
        assert not self.failures, f"{len(self.failures)} of {self.cases} cases failed:\n" + "\n".join(self.failures[:12])


def _linear_inputs(T, N, K, res, g):
    """randn inputs; pre-activations have std ~2.5 plus the bias ramp, so the
    GELU cases cover [-6, 6]; the bias ramp makes a bias shifted by one column
    group visible."""
    x = torch.randn(T, K, device=DEV, generator=g).to(BF)
    w = (torch.randn(N, K, device=DEV, generator=g) * (2.0 / math.sqrt(K))).to(BF)
    b = torch.randn(N, device=DEV, generator=g) + torch.linspace(-2.0, 2.0, N, device=DEV)
    r = torch.randn(T, N, device=DEV, generator=g).to(BF) if res else None
    return x, w, b, r


def _linear_case(T, N, K, act, res, tag):
    what = f"{tag} T={T} N={N} K={K} act={act} res={res}"
    x, w, b, r = _linear_inputs(T, N, K, res, _gen(tag, T, N, K, act, int(res)))
    xs = _strided(x, 8)
    rs = _strided(r, 16) if res else None
    out = Out(T, N)
    y = E.linear(xs, w, b, act=act, residual=rs, out=out.view)
    assert y.data_ptr() == out.view.data_ptr()
    ref, bound = linear_bound(x, w, b, act, r)
    worst = assert_within(out.view, ref, GPU_MARGIN * bound, what) * GPU_MARGIN
    out.assert_outside_untouched(what)
    return worst


ACT_RES = [("none", False), ("none", True), ("gelu", False), ("gelu", True)]


def _sweep(tally, tag, Ts, Ns, K):
    for T in Ts:
        for N in Ns:
            for act, res in ACT_RES:
                tally.run(f"T={T} N={N} {act} res={res}", lambda: _linear_case(T, N, K, act, res, tag))


# ------------------------------------------------------------------ GEMM paths
@pytest.mark.parametrize("K", [128, 384, 3072])
def test_skinny(K):
    """T <= 64, K % 128 == 0: all three NT16 instantiations, N = 1000 leaves
    the last 16-feature block half filled."""
    tally = Tally(f"skinny K={K}")
    with variant():
        _sweep(tally, "skinny", [1, 16, 17, 32, 33, 64], [768, 1000], K)
    tally.finish()


@pytest.mark.parametrize("K", [64, 192, 768])
@pytest.mark.parametrize("staging", [1, 0])
def test_tile128(staging, K):
    """128x128 kernel with LDS-DMA (1) and register (0) staging."""
    tally = Tally(f"128x128 staging={staging} K={K}")
    with variant(gemm_tile=128, staging=staging):
        _sweep(tally, f"t128s{staging}", [1, 65, 127, 128, 129, 300], [4, 132, 768, 772], K)
    tally.finish()


@pytest.mark.parametrize("small_grids", [False, True])
def test_n_not_multiple_of_8_takes_128_route(small_grids):
    """N = 772 with the default tile setting: the 256x256 kernels store 8
    features at a time, so the dispatch must leave N % 8 != 0 to the 128x128
    kernel, also when the grid and N thresholds would admit it."""
    tally = Tally(f"default tile, N=772, small_grids={small_grids}")
    settings = dict(g256_min_tiles=1, g256_min_n=8) if small_grids else {}
    with variant(**settings):
        _sweep(tally, "n772", [65, 300], [772], 768)
        _sweep(tally, "n772", [257], [772], 192)
    tally.finish()


@pytest.mark.parametrize("K", [64, 192, 384, 768])
@pytest.mark.parametrize("body", [0, 1])
def test_tile256(body, K):
    """One-tile 256x256 kernel, four-phase (0) and two-phase (1) main loop,
    KS = 1, odd and even. K = 64 / 192 cannot take the skinny route, so T <=
    64 lands here too."""
    tally = Tally(f"256x256 body={body} K={K}")
    Ts = [65, 255, 256, 257, 300] + ([1, 33, 64] if K % 128 else [])
    with variant(g256_min_tiles=1, g256_min_n=8, g256_body=body):
        _sweep(tally, f"t256b{body}", Ts, [8, 768, 1000], K)
    tally.finish()


@pytest.mark.parametrize("K", [64, 192, 384, 768])
@pytest.mark.parametrize("persist", [1, 2])
def test_persistent256_small(persist, K):
    """Persistent 256x256 kernel, register epilogue (1) and LDS image (2)."""
    tally = Tally(f"persistent256 mode={persist} K={K}")
    Ts = [65, 255, 256, 257, 300] + ([1, 33, 64] if K % 128 else [])
    with variant(g256_min_tiles=1, g256_min_n=8, g256_persist=persist):
        _sweep(tally, f"p256m{persist}", Ts, [8, 768, 1000], K)
    tally.finish()


def _more_tiles_than_cus(N):
    """T with (N / 256) x ceil(T / 256) tiles just above the CU count: one full
    round plus a few tiles, the last token tile 24 rows deep."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n_ft = (N + 255) // 256
    n_tt = cus // n_ft + 1
    assert n_ft * n_tt > cus
    return 256 * (n_tt - 1) + 24, cus, n_ft


@pytest.mark.parametrize("persist", [1, 2])
def test_persistent256_walks_two_tiles(persist):
    """More tiles than CUs (T = 5400, N = 3072 on 256 CUs: 264 tiles): some
    blocks walk two tiles -- the cross-tile prologue and the bias parity."""
    N, K = 3072, 128
    T, cus, n_ft = _more_tiles_than_cus(N)
    tally = Tally(f"persistent256 mode={persist} T={T} ({n_ft * ((T + 255) // 256)} tiles, {cus} CUs)")
    with variant(g256_persist=persist):
        tally.run("gelu+res", lambda: _linear_case(T, N, K, "gelu", True, f"p256big{persist}"))
    tally.finish()


def test_tail_split():
    """lzk_set_g256_tail(100): the 256x256 kernel takes the token rows of the
    whole rounds, the 128x128 kernel the rest; the seam rows are reported
    separately."""
    N, K = 3072, 128
    T, cus, n_ft = _more_tiles_than_cus(N)
    T0 = (cus // n_ft) * 256  # first row of the 128x128 part (5376 on 256 CUs)
    assert 0 < T0 < T
    what = f"tail split T={T} seam={T0}"
    x, w, b, r = _linear_inputs(T, N, K, True, _gen("tail", T))
    xs, rs, out = _strided(x, 8), _strided(r, 16), Out(T, N)
    with variant(g256_tail=100):
        E.linear(xs, w, b, act="gelu", residual=rs, out=out.view)
    ref, bound = linear_bound(x, w, b, "gelu", r)
    seam = slice(T0 - 1, T0 + 1)
    ws = assert_within(out.view[seam], ref[seam], GPU_MARGIN * bound[seam], what + " seam rows") * GPU_MARGIN
    worst = assert_within(out.view, ref, GPU_MARGIN * bound, what) * GPU_MARGIN
    out.assert_outside_untouched(what)
    print(f"RATIO tail split T={T} seam rows {T0 - 1}/{T0}: worst ratio to the unscaled bound {worst:.3f} "
          f"(seam rows {ws:.3f})")


@pytest.mark.parametrize("K", [128, 384, 768])
def test_split2(K):
    """Split-K pair: each half within its own bound, the sum within the sum."""
    tally = Tally(f"split2 K={K}")

    def case(T, N, res):
        what = f"split2 T={T} N={N} K={K} res={res}"
        x, w, b, r = _linear_inputs(T, N, K, res, _gen("split2", T, N, K, int(res)))
        xs = _strided(x, 8)
        rs = _strided(r, 16) if res else None
        ya, yb = E.linear_split2(xs, w, b, residual=rs)
        (ra, ba), (rb, bb), (rsum, bsum) = split2_bounds(x, w, b, r)
        wa = assert_within(ya, ra, GPU_MARGIN * ba, what + " ya")
        wb = assert_within(yb, rb, GPU_MARGIN * bb, what + " yb")
        wsum = assert_within(ya.double() + yb.double(), rsum, GPU_MARGIN * bsum, what + " ya+yb")
        return max(wa, wb, wsum) * GPU_MARGIN

    with variant():
        for T in (1, 257, 300):
            for N in (768, 1000):
                for res in (False, True):
                    tally.run(f"T={T} N={N} res={res}", lambda: case(T, N, res))
    tally.finish()


@pytest.mark.parametrize("K", [128, 384, 768])
def test_fp8(K):
    """linear_fp8 on quantize_fp8_rows outputs; the reference dequantises the
    GPU's own bytes and scales, so only the GEMM and its epilogue are judged."""
    tally = Tally(f"fp8 K={K}")

    def case(T, N, act, res):
        what = f"fp8 T={T} N={N} K={K} act={act} res={res}"
        x, w, b, r = _linear_inputs(T, N, K, res, _gen("fp8", T, N, K, act, int(res)))
        xq, sx = E.quantize_fp8_rows(x)
        wq, sw = E.quantize_fp8_rows(w)
        xqs = _strided(xq, 16, col0=16)
        rs = _strided(r, 16) if res else None
        out = Out(T, N)
        E.linear_fp8(xqs, sx, wq, sw, b, act=act, residual=rs, out=out.view)
        xd = xq.view(torch.float8_e4m3fn).float().double() * sx.double()[:, None]
        wd = wq.view(torch.float8_e4m3fn).float().double() * sw.double()[:, None]
        ref, bound = linear_bound(xd, wd, b, act, r)
        worst = assert_within(out.view, ref, GPU_MARGIN * bound, what) * GPU_MARGIN
        out.assert_outside_untouched(what)
        return worst

    with variant():
        for T in (1, 64, 257, 300):
            for N in (4, 256, 1000):
                for act, res in ACT_RES:
                    tally.run(f"T={T} N={N} {act} res={res}", lambda: case(T, N, act, res))
    tally.finish()


# ------------------------------------------------------------------ attention
def _lens_for(S):
    return sorted({min(v, S) for v in (1, 31, 32, 33, S)})


def _attention_case(hd, heads, S, packed, qk_scale=1.0):
    what = f"attention hd={hd} heads={heads} S={S} packed={packed} x{qk_scale}"
    H = hd * heads
    lens_l = _lens_for(S)
    B = len(lens_l)
    g = _gen("attn", hd, heads, S, int(packed), int(qk_scale))
    lens = torch.tensor(lens_l, dtype=torch.int32, device=DEV)
    cu = None
    rows = B * S
    if packed:
        cu = torch.tensor([0] + list(torch.tensor(lens_l).cumsum(0).tolist()), dtype=torch.int32, device=DEV)
        rows = sum(lens_l)
    qkv = torch.randn(rows, 3 * H, device=DEV, generator=g)
    qkv[:, :2 * H] *= qk_scale
    qkv = qkv.to(BF)
    qs = _strided(qkv, 8)
    out = Out(rows, H)
    o = E.attention(qs, lens, B, S, heads, out=out.view, cu=cu)
    assert o.data_ptr() == out.view.data_ptr()
    ref, bound, valid = attention_layer_bound(qkv, lens, B, S, heads, cu=cu)
    assert bool(torch.isfinite(out.view.float()).all()), what + ": non-finite output"
    worst = assert_within(out.view[valid], ref[valid], GPU_MARGIN * bound[valid], what) * GPU_MARGIN
    out.assert_outside_untouched(what)
    return worst


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("hd,heads", [(32, 2), (32, 12), (64, 2), (64, 12)])
def test_attention(hd, heads, packed):
    tally = Tally(f"attention hd={hd} heads={heads} packed={packed}")
    for S in (1, 31, 32, 33, 64, 65, 130, 512):
        tally.run(f"S={S}", lambda: _attention_case(hd, heads, S, packed))
    tally.finish()


@pytest.mark.parametrize("packed", [False, True])
def test_attention_peaked_softmax(packed):
    """q, k scaled x4: a nearly one-hot softmax whose running maximum moves
    from key block to key block (the accumulator rescale)."""
    tally = Tally(f"attention x4 packed={packed}")
    for hd, S in ((64, 130), (32, 512)):
        tally.run(f"hd={hd} S={S}", lambda: _attention_case(hd, 2, S, packed, qk_scale=4.0))
    tally.finish()


@pytest.mark.parametrize("hd", [32, 64])
def test_attention_padding_rows_cannot_leak(hd):
    """Padded layout: whatever finite values the rows >= len hold, the rows
    < len of the output are bit-identical."""
    heads = 2
    H = hd * heads
    for S in (33, 65, 130):
        lens_l = _lens_for(S)
        B = len(lens_l)
        g = _gen("attnpad", hd, S)
        lens = torch.tensor(lens_l, dtype=torch.int32, device=DEV)
        qkv = torch.randn(B * S, 3 * H, device=DEV, generator=g).to(BF)
        first = E.attention(qkv, lens, B, S, heads).clone()
        pad = torch.arange(S, device=DEV)[None, :] >= lens[:, None]  # [B, S]
        noise = (100.0 * torch.randn(B * S, 3 * H, device=DEV, generator=g)).to(BF)
        qkv2 = torch.where(pad.reshape(-1, 1), noise, qkv)
        assert bool((qkv2[~pad.reshape(-1)] == qkv[~pad.reshape(-1)]).all())
        second = E.attention(qkv2, lens, B, S, heads)
        keep = ~pad.reshape(-1)
        assert torch.equal(first[keep].view(torch.int16), second[keep].view(torch.int16)), \
            f"hd={hd} S={S}: padding rows changed the output of real rows"


# ------------------------------------------------------------------ LayerNorm
def _ln_inputs(rows, H, row_mean, g):
    x = (torch.randn(rows, H, device=DEV, generator=g) + row_mean).to(BF)
    r = torch.randn(rows, H, device=DEV, generator=g).to(BF)
    gamma = torch.rand(H, device=DEV, generator=g) + 0.5
    beta = torch.randn(H, device=DEV, generator=g) + torch.linspace(-1.0, 1.0, H, device=DEV)
    return x, r, gamma, beta


def _ln_case(rows, H, res, row_mean, pad):
    """pad = 8: aligned leading dimensions; pad = 4: multiples of 4 only, which
    rules out 16-B accesses."""
    what = f"layernorm rows={rows} H={H} res={res} mean={row_mean} ld=H+{pad}"
    x, r, gamma, beta = _ln_inputs(rows, H, row_mean, _gen("ln", rows, H, int(res), int(row_mean)))
    xs = _strided(x, pad, col0=0 if pad == 4 else 8)
    rs = _strided(r, pad + 8, col0=8) if res else None
    out = Out(rows, H, ld_extra=pad)
    E.layernorm(xs, gamma, beta, 1e-12, residual=rs, out=out.view)
    ref, bound = layernorm_bound(x, gamma, beta, 1e-12, r if res else None)
    worst = assert_within(out.view, ref, GPU_MARGIN * bound, what) * GPU_MARGIN
    out.assert_outside_untouched(what)
    return worst, out.view.clone()


@pytest.mark.parametrize("H", [128, 256, 260, 512, 516, 768, 1000, 1024])
def test_layernorm(H):
    tally = Tally(f"layernorm H={H}")
    for rows in (1, 15, 16, 17, 33):
        for res in (False, True):
            for row_mean in (0.0, 30.0):
                tally.run(f"rows={rows} res={res} mean={row_mean}",
                          lambda: _ln_case(rows, H, res, row_mean, 8)[0])
    tally.finish()


def _over_one_bf16_ulp(a, b):
    """Elements of two bf16 tensors further apart than one ulp of the larger."""
    a, b = a.double(), b.double()
    big = torch.maximum(a.abs(), b.abs()).clamp_min(2.0 ** -126)
    ulp = torch.exp2(torch.floor(torch.log2(big)) - 7)
    return (a - b).abs() > ulp


LN_ROWS = (1, 15, 16, 17, 33)


@pytest.mark.parametrize("H", [768, 1024])
def test_layernorm_generic_fallback_within_bound(H):
    """H = 768 / 1024 with ld = H + 4 (multiples of 4, not of 8) cannot use
    16-B accesses: they take the 8-B instantiation of layernorm16_kernel. (The
    generic layernorm_kernel<3|4> serves the other H: 516 and 1000 in
    test_layernorm.)"""
    tally = Tally(f"layernorm 8-B aligned rows H={H}")
    for rows in LN_ROWS:
        for res in (False, True):
            for row_mean in (0.0, 30.0):
                tally.run(f"rows={rows} res={res} mean={row_mean}",
                          lambda: _ln_case(rows, H, res, row_mean, 4)[0])
    tally.finish()


@pytest.mark.parametrize("row_mean", [0.0, 30.0])
@pytest.mark.parametrize("H", [768, 1024])
def test_layernorm_generic_fallback_agrees(H, row_mean):
    """H = 768 / 1024 with aligned leading dimensions (16-B accesses) and with
    ld = H + 4 (8-B accesses) on the same inputs: within one bf16 ulp of each
    other, and in fact bit-identical, since both run layernorm16_kernel's
    lane mapping and summation order.

    Before that, ld = H + 4 fell back to layernorm_kernel<3|4>, whose
    different fp32 summation order moved the mean of a row of mean 30 by
    ~2e-6: outputs where g z cancels against b (results of ~2e-4) came out 2
    to 3 ulps apart in 3 of 20 cases (0.000160217 vs 0.000163078, fp64
    0.000161378), so a row's result depended on how its buffer was aligned."""
    failures, differing = [], []
    for rows in LN_ROWS:
        for res in (False, True):
            _, y16 = _ln_case(rows, H, res, row_mean, 8)
            _, yg = _ln_case(rows, H, res, row_mean, 4)
            over = _over_one_bf16_ulp(y16, yg)
            n_diff = int((y16.view(torch.int16) != yg.view(torch.int16)).sum())
            print(f"AGREE layernorm H={H} rows={rows} res={res} mean={row_mean}: {n_diff} of {over.numel()} "
                  f"elements differ, {int(over.sum())} by more than one ulp")
            for i, j in over.nonzero().tolist()[:4]:
                failures.append(f"rows={rows} res={res} ({i},{j}): {float(y16[i, j]):.9g} vs {float(yg[i, j]):.9g}")
            if n_diff:
                differing.append(f"rows={rows} res={res}: {n_diff} elements")
    assert not failures, "more than one bf16 ulp apart:\n" + "\n".join(failures)
    assert not differing, "same arithmetic, yet not bit-identical:\n" + "\n".join(differing)


@pytest.mark.parametrize("H", [128, 384, 768, 1024])
def test_embed_ln(H):
    V, max_pos, S = 1000, 64, 7
    tally = Tally(f"embed_ln H={H}")
    g = _gen("embed", H)
    wemb = torch.randn(V, H, device=DEV, generator=g).to(BF)
    pemb = torch.randn(max_pos, H, device=DEV, generator=g).to(BF)
    temb = torch.randn(2, H, device=DEV, generator=g).to(BF)
    gamma = torch.rand(H, device=DEV, generator=g) + 0.5
    beta = torch.randn(H, device=DEV, generator=g) + torch.linspace(-1.0, 1.0, H, device=DEV)

    def case(T, with_pos):
        what = f"embed_ln T={T} H={H} pos={with_pos}"
        ids = torch.randint(0, V, (T,), device=DEV, generator=g, dtype=torch.int32)
        ids[0] = 0
        ids[-1] = V - 1
        pos = None
        if with_pos:
            pos = torch.randint(0, max_pos, (T,), device=DEV, generator=g, dtype=torch.int32)
            pos[-1] = 0
            pos[0] = max_pos - 1
        y = E.embed_ln(ids, S, wemb, pemb, temb, gamma, beta, 1e-12, pos=pos)
        ref, bound = embed_ln_bound(ids, S, wemb, pemb, temb, gamma, beta, 1e-12, pos=pos)
        return assert_within(y, ref, GPU_MARGIN * bound, what) * GPU_MARGIN

    for T in (1, 5, 333):
        for with_pos in (False, True):
            tally.run(f"T={T} pos={with_pos}", lambda: case(T, with_pos))
    tally.finish()


@pytest.mark.parametrize("H", [128, 384, 768, 1024])
def test_pool_norm(H):
    tally = Tally(f"pool_norm H={H}")

    def case(S, mode, packed, width):
        what = f"pool_norm H={H} S={S} {mode} packed={packed} width={width}"
        lens_l = [1, S, min(7, S)]
        B = len(lens_l)
        g = _gen("pool", H, S, mode, int(packed))
        lens = torch.tensor(lens_l, dtype=torch.int32, device=DEV)
        cu = None
        rows = B * S
        if packed:
            cu = torch.tensor([0] + list(torch.tensor(lens_l).cumsum(0).tolist()), dtype=torch.int32, device=DEV)
            rows = sum(lens_l)
        x = torch.randn(rows, H, device=DEV, generator=g).to(BF)
        o32, o16 = E.pool_norm(x, lens, B, S, mode, out16_width=width, cu=cu)
        ref, bound = pool_norm_bound(x, lens, B, S, mode, cu=cu)
        worst = assert_within(o32, ref, GPU_MARGIN * bound, what) * GPU_MARGIN
        norms = o32.double().norm(dim=1)
        assert bool(((norms - 1.0).abs() <= 1e-5).all()), f"{what}: norms {norms.tolist()}"
        assert o16.shape == (B, width)
        assert torch.equal(o16[:, :H].view(torch.int16), o32.to(BF).view(torch.int16)), f"{what}: bf16 copy"
        assert bool((o16[:, H:].view(torch.int16) == 0).all()), f"{what}: padding columns not zero"
        return worst

    for S in ((33, 512) if H == 384 else (33,)):
        for mode in ("mean", "cls"):
            for packed in (False, True):
                for width in (H, H + 24):
                    tally.run(f"S={S} {mode} packed={packed} width={width}",
                              lambda: case(S, mode, packed, width))
    tally.finish()


def test_setters_are_back_at_their_defaults():
    """variant() restores every setter when its body raises, so a failing case
    above cannot leave a non-default GEMM variant selected: after a raise, a
    shape that only the default dispatch sends to the skinny kernel is still
    bit-identical to a run before any setter was touched."""
    x, w, b, _ = _linear_inputs(33, 768, 384, False, _gen("defaults"))
    before = E.linear(x, w, b)
    with pytest.raises(RuntimeError):
        with variant(gemm_tile=128, staging=0, g256_min_tiles=1, g256_min_n=8, g256_persist=1, g256_tail=100,
                     g256_body=0):
            raise RuntimeError("mid-test failure")
    after = E.linear(x, w, b)
    assert torch.equal(before.view(torch.int16), after.view(torch.int16))
