"""Per-element error bounds for the encoder kernels (csrc/kernels/encoder.hip).

Every helper takes an op's bf16 / fp32 inputs, computes the op in fp64 on the
inputs' device (pure torch: nothing here imports the kernel library) and
returns ``(ref, bound)``: the fp64 result and, per element, how far a correct
kernel may be from it. ``u = 2**-8`` is the unit round-off of bf16 (8
significant bits, round to nearest), ``2**-24`` that of fp32.

Margin. The GPU tests assert ``|y - ref| <= 2 * bound`` (``GPU_MARGIN``). The
bounds below model the roundings a kernel is documented to make; the factor 2
covers what they do not model: the order in which an MFMA accumulates, the
hardware ``exp2`` / ``rsqrt`` / reciprocal approximations and the rounding of
the fp32 scores before the softmax. The CPU tier
(tests/unit/test_encoder_bounds_cpu.py) shows that fp32 / bf16 emulations of
the kernels stay within 1.0 x bound and that corrupting four elements exceeds
2 x bound many times over, so the factor hides nothing.
"""
from __future__ import annotations

import math

import torch

U_BF16 = 2.0 ** -8
U_FP32 = 2.0 ** -24
GELU_ABS = 1e-4  # polynomial GELU of encoder.hip: |error| < 1e-4 (its header comment)
GPU_MARGIN = 2.0


def _f64(t):
    return None if t is None else t.to(torch.float64)


def gelu64(z: torch.Tensor) -> torch.Tensor:
    return 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))


def linear_bound(x, w, b, act: str = "none", residual=None):
    """``ref = act(x w^T + b) + r`` and its bound.

    Let ``a = act(x w^T + b)`` and ``mag = |x| |w|^T + |b|`` in fp64, K the
    inner dimension.

      bound = u (|a| + |ref|) + K 2^-24 mag + (1e-4 if gelu)

    * ``u |ref|`` is the final rounding of the stored bf16. ``u |a|`` is the
      rounding of ``a`` to bf16 *before* the residual is added: the 256x256
      and fp8 epilogues pass ``a`` through a bf16 LDS image and add the
      residual to that (two roundings); the 128x128, skinny and persistent
      register epilogues round once and simply do not use this term.
    * ``K 2^-24 mag``: the products of two bf16 (or two e4m3) numbers are exact
      in fp32, so the pre-activation differs from the fp64 one only by the K
      additions (and the bias add), each at most 2^-24 of a partial sum that
      is itself at most ``mag`` -- the classic worst case for any summation
      order. Real sums err like sqrt(K), so the term is far from binding. GELU
      has slope in [-0.13, 1.13]; the term is kept as stated and the 0.13 K
      2^-24 mag that the slope could add lies far inside the margin.
    * GELU is a polynomial with a documented absolute error below 1e-4.

    ``x`` / ``w`` may be any float dtype: for the fp8 GEMM pass the
    dequantised operands (``q * scale``), so that only the GEMM is judged.
    """
    x64, w64, b64, r64 = _f64(x), _f64(w), _f64(b), _f64(residual)
    K = x64.shape[1]
    z = x64 @ w64.T + b64
    a = gelu64(z) if act == "gelu" else z
    ref = a if r64 is None else a + r64
    mag = x64.abs() @ w64.abs().T + b64.abs()
    bound = U_BF16 * (a.abs() + ref.abs()) + K * U_FP32 * mag
    if act == "gelu":
        bound = bound + GELU_ABS
    return ref, bound


def split2_bounds(x, w, b, residual=None):
    """Split-K pair (``linear_split2``): ``ya = x[:, :K/2] w[:, :K/2]^T + b + r``
    and ``yb = x[:, K/2:] w[:, K/2:]^T``, each bounded as in
    :func:`linear_bound` with its own K range (K/2 additions, its own ``mag``;
    yb has no bias and no residual). The consumer adds the halves in fp32, so
    ``ya + yb`` is compared with the full product: by the triangle inequality
    its bound is the sum of the two.

    Returns ``(ref_a, bound_a), (ref_b, bound_b), (ref_sum, bound_sum)``.
    """
    h = x.shape[1] // 2
    ra, ba = linear_bound(x[:, :h], w[:, :h], b, "none", residual)
    rb, bb = linear_bound(x[:, h:], w[:, h:], torch.zeros_like(b), "none", None)
    x64, w64 = _f64(x), _f64(w)
    full = x64 @ w64.T + _f64(b)
    if residual is not None:
        full = full + _f64(residual)
    return (ra, ba), (rb, bb), (full, ba + bb)


def attention_bound(q, k, v, length: int):
    """One head of one sequence: q ``[Sq, hd]``, k / v ``[Sk, hd]``; keys at or
    past ``length`` are masked. ``P = softmax(q k^T / sqrt(hd))`` over the
    unmasked keys and ``o = P V`` in fp64.

      bound = u (P |V|) + u |o| + 1e-6

    The kernel keeps the unnormalised ``p_j = exp2(s_j - m)`` in fp32, sums
    them in fp32 for the denominator ``l`` and rounds each to bf16 only as the
    operand of the P V MFMA: ``o' = sum_j p_j (1 + d_j) v_j / l`` with ``|d_j|
    <= u``, so ``|o' - o| <= u sum_j P_j |v_j|`` -- the first term. Rescaling
    the accumulator when the running maximum moves multiplies numerator and
    denominator alike. ``u |o|`` is the rounding of the stored bf16. ``1e-6``
    absorbs the fp32 roundings (scores, ``l``, the accumulation), which are
    relative 2^-24-sized effects on values of order one.
    """
    q64, k64, v64 = _f64(q), _f64(k[..., :length, :]), _f64(v[..., :length, :])  # leading dims: heads
    s = (q64 @ k64.transpose(-1, -2)) / math.sqrt(q64.shape[-1])
    P = torch.softmax(s, dim=-1)
    o = P @ v64
    bound = U_BF16 * (P @ v64.abs()) + U_BF16 * o.abs() + 1e-6
    return o, bound


def attention_layer_bound(qkv, lens, B: int, S: int, nheads: int, cu=None):
    """:func:`attention_bound` for every sequence and head of a ``[rows, 3H]``
    (q | k | v) buffer, padded (sequence b = rows ``[b S, b S + S)``) or packed
    (``cu``: rows ``[cu[b], cu[b] + len)``). Returns ``ref, bound, valid`` of
    shape ``[rows, H]``; ``valid`` marks the rows ``< len`` (the only rows the
    op defines), everywhere else ref = 0 and bound = inf."""
    rows = qkv.shape[0]
    H = qkv.shape[1] // 3
    hd = H // nheads
    ref = torch.zeros((rows, H), dtype=torch.float64, device=qkv.device)
    bound = torch.full((rows, H), float("inf"), dtype=torch.float64, device=qkv.device)
    valid = torch.zeros((rows,), dtype=torch.bool, device=qkv.device)
    lens_l = [int(v) for v in lens.tolist()]
    cu_l = None if cu is None else [int(v) for v in cu.tolist()]
    for b in range(B):
        L = lens_l[b]
        r0 = cu_l[b] if cu_l is not None else b * S
        blk = qkv[r0:r0 + L]
        valid[r0:r0 + L] = True
        q, k, v = (blk[:, i * H:(i + 1) * H].reshape(L, nheads, hd).transpose(0, 1) for i in range(3))
        o, bd = attention_bound(q, k, v, L)  # [heads, L, hd]
        ref[r0:r0 + L] = o.transpose(0, 1).reshape(L, H)
        bound[r0:r0 + L] = bd.transpose(0, 1).reshape(L, H)
    return ref, bound, valid


def _ln_bound(v64, g, b, eps):
    g64, b64 = _f64(g), _f64(b)
    mean = v64.mean(dim=1, keepdim=True)
    var = ((v64 - mean) ** 2).mean(dim=1, keepdim=True)
    z = (v64 - mean) / torch.sqrt(var + eps)
    ref = g64 * z + b64
    bound = U_BF16 * ref.abs() + 1e-4 * (g64.abs() * z.abs() + b64.abs())
    return ref, bound


def layernorm_bound(x, g, b, eps: float = 1e-12, residual=None):
    """``ref = g z + b`` with ``z = (v - mean) / sqrt(var + eps)``, ``v = x + r``.

      bound = u |ref| + 1e-4 (|g| |z| + |b|)

    ``u |ref|`` is the rounding of the stored bf16. The second term covers
    fp32 statistics over H <= 1024 features: a sum of H fp32 terms carries a
    relative error of at most H 2^-24 = 6e-5, so the mean, the variance
    (two-pass, or one-pass ``E[v^2] - mean^2`` for rows whose mean is up to
    ~30 standard deviations) and ``rsqrt`` move ``z`` by a relative 1e-4 at
    most, and the multiply-add with g and b adds 2^-24 of each term.
    """
    v = _f64(x) if residual is None else _f64(x) + _f64(residual)
    return _ln_bound(v, g, b, eps)


def embed_ln_bound(ids, S: int, wemb, pemb, temb, g, b, eps: float = 1e-12, pos=None):
    """``LN(word[ids] + position[p] + type[0])`` with ``p = t % S`` or the given
    ``pos``: the sum of three bf16 numbers in fp32 is within 2 * 2^-24 of the
    fp64 sum, so the LayerNorm bound (:func:`layernorm_bound`) applies as is."""
    T = ids.numel()
    p = (torch.arange(T, device=ids.device) % S) if pos is None else pos.long()
    v = _f64(wemb)[ids.long()] + _f64(pemb)[p] + _f64(temb)[0]
    return _ln_bound(v, g, b, eps)


def pool_norm_bound(x, lens, B: int, S: int, mode: str = "mean", cu=None):
    """``ref = s / |s|`` (fp32 output) with ``s`` the mean of the first ``len``
    rows of a sequence (``mode="mean"``) or its first row (``"cls"``).

    The kernel adds the ``len <= 512`` bf16 values of a column one after the
    other in fp32: ``|ds_c| <= e_c = len 2^-24 m_c`` with ``m_c`` the mean of
    ``|x|`` over those rows (len - 1 additions and the division, each 2^-24 of
    a partial sum of at most ``len m_c``); for CLS ``e = 0``. Then, with ``n =
    |s|``:

      d(s_c / n) <= e_c / n + |ref_c| (|e| / n + 16 2^-24)

    -- the column's own error, the error of the norm caused by all columns
    (``|d n| <= |e|``), and the fp32 arithmetic of the normalisation: the
    squares and their sum (at most 4 + 6 + 3 additions of non-negative terms
    per partial: 14 roundings of ``n^2``, so 7 of ``n``), the square root, the
    reciprocal (2), and the final product (1), rounded up to 16.
    """
    H = x.shape[1]
    x64 = _f64(x)
    lens_l = [max(1, int(v)) for v in lens.tolist()]
    cu_l = None if cu is None else [int(v) for v in cu.tolist()]
    ref = torch.empty((B, H), dtype=torch.float64, device=x.device)
    bound = torch.empty((B, H), dtype=torch.float64, device=x.device)
    for bb in range(B):
        L = lens_l[bb]
        r0 = cu_l[bb] if cu_l is not None else bb * S
        if mode == "cls":
            s = x64[r0]
            e = torch.zeros_like(s)
        else:
            blk = x64[r0:r0 + L]
            s = blk.mean(dim=0)
            e = L * U_FP32 * blk.abs().mean(dim=0)
        n = s.norm().clamp_min(1e-12)
        ref[bb] = s / n
        bound[bb] = e / n + ref[bb].abs() * (e.norm() / n + 16 * U_FP32)
    return ref, bound


def worst_ratio(y, ref, bound) -> float:
    """max |y - ref| / bound over all elements (0 / 0 counts as 0)."""
    err = (_f64(y) - ref).abs()
    ratio = torch.where(err > 0, err / bound, torch.zeros_like(err))
    return float(ratio.max()) if ratio.numel() else 0.0


def assert_within(y, ref, bound, what: str) -> float:
    """Every element of ``y`` is finite and within ``bound`` of ``ref``; no
    element is exempt. Returns the worst ratio ``|y - ref| / bound``; on
    failure reports it, its (row, col) and how many elements are over."""
    assert tuple(y.shape) == tuple(ref.shape) == tuple(bound.shape), \
        f"{what}: shapes {tuple(y.shape)} {tuple(ref.shape)} {tuple(bound.shape)}"
    y64 = _f64(y)
    finite = torch.isfinite(y64)
    if not bool(finite.all()):
        bad = (~finite).nonzero()
        raise AssertionError(f"{what}: {bad.shape[0]} non-finite elements, first at {tuple(bad[0].tolist())}")
    err = (y64 - ref).abs()
    over = err > bound
    ratio = torch.where(err > 0, err / bound, torch.zeros_like(err))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    n_over = int(over.sum())
    if n_over:
        flat = int(ratio.reshape(-1).argmax())
        cols = ratio.shape[-1] if ratio.dim() > 1 else 1
        row, col = divmod(flat, cols)
        raise AssertionError(
            f"{what}: {n_over} of {ratio.numel()} elements exceed the bound; worst ratio {worst:.3g} at "
            f"(row {row}, col {col}): got {float(y64.reshape(-1)[flat]):.9g}, ref {float(ref.reshape(-1)[flat]):.9g}, "
            f"bound {float(bound.reshape(-1)[flat]):.3g}")
    return worst
