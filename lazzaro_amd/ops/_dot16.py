"""The arithmetic of csrc/include/lzk_dot16.h restated once for the ops that
bound or mirror it (mmr_ops, expand_ops, fuse_ops, lex_ops): the rounding depth
of the 16-lanes-per-row dot product and the cosine that is 0 when either norm
is 0."""
from __future__ import annotations

import torch


def sum_depth(D: int) -> int:
    """L(D) = 4 ceil(D / 64) + 4: the fp32 roundings one dot product of the
    kernels passes through (lzk_dot16.h): a lane's chain of fmas over its share
    of the dimensions -- 4 per float4 it owns, ceil(D / 4 / 16) of them at
    most; the scalar path's ceil(D / 16) is never longer -- and the 4 shuffle
    adds."""
    return 4 * -(-int(D) // 64) + 4


def cos_or_zero(dot, na, nb):
    """``dot / (na * nb)`` elementwise, 0 where either norm is 0 (lzk_cos)."""
    ok = (na > 0) & (nb > 0)
    return torch.where(ok, dot / torch.where(ok, na * nb, torch.ones_like(dot)), torch.zeros_like(dot))
