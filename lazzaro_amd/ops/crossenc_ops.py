"""Cross-encoder re-ranking of a search's pool: the pair assembly, the
embedding and the classification head around the encoder layers
(csrc/kernels/crossenc.hip), with the torch formulations.

The contract. A call carries ``M`` queries with a pool of ``P <= 64`` graph
rows each, ``rows`` int64 [M, P] in the first-stage order; a slot ``< 0`` or
``>= n`` is empty. ``B = M * P <= 65,536`` pairs per call (models/
cross_encoder.py chunks the queries).

1. **Tokens.** A text's body pieces are ``Tokenizer.encode(text, n + 2)[1:-1]``
   (:func:`body_pieces`). A query keeps its first ``MAX_QUERY_TOKENS`` = 64:
   ``qtok`` int32 [M, 64], ``qlen`` int32 [M]. A memory keeps its first ``L``
   (32 / 64 / 128): the token column ``tok`` [n, L] of 16-bit patterns and
   ``dlen`` int32 [n] (engine/token_column.py). The vocabulary is at most
   65,536.
2. **Pair.** Slot ``(m, j)`` with row ``r >= 0``: ``ql = qlen[m]``, ``dl =
   min(dlen[r], max_pos - 3 - ql)``; the sequence is ``[CLS] q_1..q_ql [SEP]
   d_1..d_dl [SEP]``, token types 0 through the first ``[SEP]`` and 1 after
   it, positions ``0 .. ql + dl + 2`` -- HF's pair encoding with
   ``token_type_ids``. An empty slot is ``[CLS] [SEP] [SEP]`` (types 0, 0, 1):
   every sequence is non-empty, and the empty slot's logit is discarded.
   :func:`ce_lens` gives ``lens`` int32 [B], their exclusive prefix ``cu``
   int32 [B + 1] and ``stat = (T, S_max)``; :func:`ce_embed_ln` writes
   ``LN(word[id] + position[p] + type[t])`` as bf16 row ``cu[b] + p``, summed
   and normalised exactly as ``encoder_ops.embed_ln`` does.
3. **Score.** The encoder layers run over the packed tokens, the last one past
   its attention on the CLS rows only; ``pooled = tanh(Wp h_cls + bp)`` and
   ``logit = <wc, pooled> + bc``. :func:`ce_head_select` takes the pooler's
   dense output (bf16, before the tanh), applies ``tanhf`` and the fp32 dot;
   :func:`ce_head_tol` bounds the logit's distance from fp64 given that bf16
   input. The logit is the score: nothing of the first stage is blended in.
4. **Result.** The ``k`` largest logits come back descending, ties to the
   lower row, ``(-inf, -1)`` once the pool's real rows run out, with
   ``logits`` fp32 [M, P] in pool order, ``-inf`` in empty slots.

Device tensors always take the kernels; CPU tensors take the ``*_ref``
formulations (the CPU tier, and a second formulation the tests hold to the
same fp64 oracle).
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib
from ..core.crossenc import DOC_TOKEN_CHOICES, MAX_POOL, MAX_QUERY_TOKENS, MAX_VOCAB

NEG_INF = float("-inf")
MAX_PAIRS = 65536  # crossenc.hip CE_MAX_B: pairs per call

# rows M P qlen dlen n L max_pos | lens cu stat stream
_lib.register("lzk_ce_lens", _lib.I, [_lib.P, _lib.I, _lib.I, _lib.P, _lib.P, _lib.L, _lib.I, _lib.I,
                                      _lib.P, _lib.P, _lib.P, _lib.P])
# rows M P n qtok qlen tok dlen | L max_pos cu T cls sep vocab | word pos type g b H eps | Y oid opos otype stream
_lib.register("lzk_ce_embed_ln", _lib.I, [_lib.P, _lib.I, _lib.I, _lib.L, _lib.P, _lib.P, _lib.P, _lib.P,
                                          _lib.I, _lib.I, _lib.P, _lib.I, _lib.I, _lib.I, _lib.I,
                                          _lib.P, _lib.P, _lib.P, _lib.P, _lib.P, _lib.I, _lib.F,
                                          _lib.P, _lib.P, _lib.P, _lib.P, _lib.P])
# X ldx H rows M P n | wc bc k scores rows logits stream
_lib.register("lzk_ce_head_select", _lib.I, [_lib.P, _lib.L, _lib.I, _lib.P, _lib.I, _lib.I, _lib.L,
                                             _lib.P, _lib.P, _lib.I, _lib.P, _lib.P, _lib.P, _lib.P])


def ce_head_tol(H: int, wsum: float = 1.0, bias: float = 0.0) -> float:
    """|logit32 - logit64| given the bf16 pooler output (derived in
    crossenc.hip's header), with ``wsum = sum |wc_i|`` and ``bias = bc``:
    4 units of 2^-24 of ``wsum`` for ``tanhf`` (2 ulp stated, counted twice),
    H + 4 for the fused multiply-adds and the folds -- each rounds a partial
    sum of magnitude at most ``wsum``, in any order --, one for the bias add
    on a number of magnitude at most ``wsum + |bias|``."""
    return (int(H) + 9) * (float(wsum) + abs(float(bias))) * 2.0 ** -24


# ------------------------------------------------------------------ tokens
def body_pieces(tokenizer, texts, n: int) -> Tuple[np.ndarray, np.ndarray]:
    """The first ``n`` body pieces of every text -- ``tokenizer.encode(text, n
    + 2)[1:-1]`` -- as (ids int32 [len(texts), n] zero padded, lens int32)."""
    texts = ["" if t is None else str(t) for t in texts]
    out = np.zeros((len(texts), n), dtype=np.int32)
    lens = np.zeros(len(texts), dtype=np.int32)
    if not texts:
        return out, lens
    ids, ln = tokenizer.encode_batch(texts, n + 2)
    ids, ln = np.asarray(ids, dtype=np.int32), np.asarray(ln, dtype=np.int32)
    lens[:] = np.clip(ln - 2, 0, n)
    w = min(n, max(ids.shape[1] - 1, 0))
    out[:, :w] = ids[:, 1:1 + w]
    out[np.arange(n)[None, :] >= lens[:, None]] = 0  # (the closing [SEP] and the padding)
    return out, lens


def as_query_tokens(query_tokens, tokenizer=None) -> Tuple[np.ndarray, np.ndarray]:
    """The queries' tokens on the host, (ids int32 [M, 64], lens int32 [M]):
    from texts (through ``tokenizer``) or from ``(ids [M, <= 64], lens)``."""
    if query_tokens is None:
        raise ValueError("a re-ranked search needs the queries' text: pass query_tokens=")
    if isinstance(query_tokens, str):
        query_tokens = [query_tokens]
    if isinstance(query_tokens, tuple) and len(query_tokens) == 2 and not isinstance(query_tokens[0], str):
        ids, lens = query_tokens
        ids = np.asarray(ids.cpu() if torch.is_tensor(ids) else ids).astype(np.int64)
        lens = np.asarray(lens.cpu() if torch.is_tensor(lens) else lens).astype(np.int64).reshape(-1)
        if ids.ndim == 1:
            ids = ids[None, :]
        if ids.ndim != 2 or ids.shape[1] > MAX_QUERY_TOKENS or ids.shape[0] != lens.shape[0]:
            raise ValueError(f"query_tokens ids must be [M, <= {MAX_QUERY_TOKENS}] with one length per row "
                             f"(got {ids.shape}, {lens.shape})")
        if lens.size and (lens.min() < 0 or lens.max() > ids.shape[1]):
            raise ValueError("query_tokens lengths must lie in 0 .. the ids' width")
        if ids.size and (ids.min() < 0 or ids.max() >= MAX_VOCAB):
            raise ValueError(f"query_tokens ids must lie in 0 .. {MAX_VOCAB - 1}")
        out = np.zeros((ids.shape[0], MAX_QUERY_TOKENS), dtype=np.int32)
        out[:, :ids.shape[1]] = ids
        out[np.arange(MAX_QUERY_TOKENS)[None, :] >= lens[:, None]] = 0
        return out, lens.astype(np.int32)
    texts = list(query_tokens)
    if not all(isinstance(t, str) for t in texts):
        raise ValueError("query_tokens must be texts, or (ids, lens)")
    if tokenizer is None:
        raise ValueError("query texts need the re-ranker's tokenizer")
    return body_pieces(tokenizer, texts, MAX_QUERY_TOKENS)


# ------------------------------------------------------------------ checks
def _check_pairs(rows, qlen, dlen, max_pos: int, L: int):
    if rows.dim() != 2:
        raise ValueError(f"rows must be [M, P] (got {tuple(rows.shape)})")
    M, P = rows.shape
    if not 1 <= P <= MAX_POOL:
        raise ValueError(f"a pool holds 1 .. {MAX_POOL} slots (got {P})")
    if M * P > MAX_PAIRS:
        raise ValueError(f"{M} x {P} pairs in one call: at most {MAX_PAIRS}")
    if qlen.numel() != M:
        raise ValueError(f"{M} pools but {qlen.numel()} query lengths")
    if int(L) not in DOC_TOKEN_CHOICES:
        raise ValueError(f"L must be one of {DOC_TOKEN_CHOICES} (got {L})")
    if int(max_pos) < 4:
        raise ValueError(f"max_pos must be >= 4 (got {max_pos})")
    return M, P, int(dlen.numel())


def _pair_parts(rows, qlen, dlen, max_pos: int, L: int):
    """(valid, ql, dl) [M, P] of the pair rule."""
    M, P = rows.shape
    n = dlen.numel()
    rows = rows.to(torch.long)
    valid = (rows >= 0) & (rows < n)
    ql = qlen.to(torch.long).clamp(0, min(MAX_QUERY_TOKENS, max_pos - 3))[:, None].expand(M, P)
    if n:
        d = dlen.to(torch.long)[rows.clamp(0, n - 1)]
    else:
        d = torch.zeros_like(rows)
    dl = torch.minimum(d.clamp_max(L), max_pos - 3 - ql).clamp_min(0)
    zero = torch.zeros_like(rows)
    return valid, torch.where(valid, ql, zero), torch.where(valid, dl, zero)


# ------------------------------------------------------------------ lens
def ce_lens_ref(rows, qlen, dlen, max_pos: int, L: int):
    """Torch formulation of :func:`ce_lens` (any device)."""
    M, P, n = _check_pairs(rows, qlen, dlen, max_pos, L)
    _, ql, dl = _pair_parts(rows, qlen, dlen, max_pos, L)
    lens = (ql + dl + 3).reshape(-1)
    cu = torch.cat([torch.zeros(1, dtype=torch.long, device=rows.device), torch.cumsum(lens, 0)])
    stat = torch.stack([cu[-1], lens.max() if lens.numel() else cu[-1]])
    return lens.to(torch.int32), cu.to(torch.int32), stat.to(torch.int32)


def ce_lens(rows: torch.Tensor, qlen: torch.Tensor, dlen: torch.Tensor, max_pos: int, L: int):
    """(lens int32 [B], cu int32 [B + 1], stat int32 [2] = (T, S_max)) of the
    pairs of ``rows`` int64 [M, P], ``qlen`` int32 [M], ``dlen`` int32 [n]
    (crossenc.hip ce_lens_kernel). Nothing is read back here."""
    M, P, n = _check_pairs(rows, qlen, dlen, max_pos, L)
    if not rows.is_cuda or M == 0:
        return ce_lens_ref(rows, qlen, dlen, max_pos, L)
    dev = rows.device
    assert rows.dtype == torch.long and rows.is_contiguous() and qlen.dtype == torch.int32 and dlen.dtype == torch.int32
    B = M * P
    lens = torch.empty(B, dtype=torch.int32, device=dev)
    cu = torch.empty(B + 1, dtype=torch.int32, device=dev)
    stat = torch.empty(2, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().lzk_ce_lens(rows.data_ptr(), M, P, qlen.data_ptr(), _lib.ptr(dlen) if n else 0, n, int(L),
                                      int(max_pos), lens.data_ptr(), cu.data_ptr(), stat.data_ptr(),
                                      _lib.stream_ptr(dev)), "lzk_ce_lens")
    return lens, cu, stat


# ------------------------------------------------------------------ embed
def pair_tokens_ref(rows, qtok, qlen, tok, dlen, max_pos: int, L: int, cls_id: int, sep_id: int, vocab: int):
    """(ids, positions, types) int32 [T] of the packed pairs, vectorised."""
    M, P, n = _check_pairs(rows, qlen, dlen, max_pos, L)
    dev = rows.device
    _, ql, dl = _pair_parts(rows, qlen, dlen, max_pos, L)
    ql, dl = ql.reshape(-1), dl.reshape(-1)
    lens = ql + dl + 3
    B = M * P
    cu = torch.cat([torch.zeros(1, dtype=torch.long, device=dev), torch.cumsum(lens, 0)])
    seq = torch.repeat_interleave(torch.arange(B, device=dev), lens)
    p = torch.arange(int(cu[-1]), device=dev) - cu[seq]
    qt, dt, ln = ql[seq], dl[seq], lens[seq]
    qid = qtok.to(torch.long)[seq // P, (p - 1).clamp(0, MAX_QUERY_TOKENS - 1)]
    if n:
        r = rows.to(torch.long).reshape(-1)[seq].clamp(0, n - 1)
        did = tok.to(torch.long)[r, (p - qt - 2).clamp(0, L - 1)] & 0xFFFF
    else:
        did = torch.zeros_like(p)
    cls = torch.full_like(p, int(cls_id))
    sep = torch.full_like(p, int(sep_id))
    ids = torch.where(p == 0, cls, torch.where(p <= qt, qid, torch.where((p == qt + 1) | (p == ln - 1), sep, did)))
    ids = ids.clamp(0, int(vocab) - 1)
    types = (p > qt + 1)
    return ids.to(torch.int32), p.to(torch.int32), types.to(torch.int32)


def ce_embed_ln_ref(rows, qtok, qlen, tok, dlen, cu, T, max_pos, L, cls_id, sep_id, wemb, pemb, temb, g, b,
                    eps: float = 1e-12, debug: bool = False):
    """Torch formulation of :func:`ce_embed_ln` (any device)."""
    ids, pos, types = pair_tokens_ref(rows, qtok, qlen, tok, dlen, max_pos, L, cls_id, sep_id, wemb.shape[0])
    H = wemb.shape[1]
    v = wemb[ids.long()].float() + pemb[pos.long()].float() + temb[types.long()].float()
    y = F.layer_norm(v, (H,), g.float(), b.float(), eps).to(wemb.dtype)
    return (y, ids, pos, types) if debug else y


def ce_embed_ln(rows, qtok, qlen, tok, dlen, cu, T: int, max_pos: int, L: int, cls_id: int, sep_id: int,
                wemb, pemb, temb, g, b, eps: float = 1e-12, debug: bool = False):
    """bf16 [T, H]: the pairs of ``rows`` assembled, embedded and normalised
    (crossenc.hip ce_embed_ln_kernel; ``cu`` from :func:`ce_lens`, ``T`` its
    last entry as read back by the caller). ``qtok`` int32 [M, 64], ``tok``
    int16 [n, L]. ``debug``: also the (ids, positions, types) int32 [T] the
    kernel resolved."""
    M, P, n = _check_pairs(rows, qlen, dlen, max_pos, L)
    vocab, H = wemb.shape
    if vocab > MAX_VOCAB:
        raise ValueError(f"the token column stores 16-bit ids: vocabulary {vocab} exceeds {MAX_VOCAB}")
    if not rows.is_cuda or M == 0:
        return ce_embed_ln_ref(rows, qtok, qlen, tok, dlen, cu, T, max_pos, L, cls_id, sep_id, wemb, pemb, temb, g, b,
                               eps, debug)
    dev = rows.device
    assert rows.dtype == torch.long and rows.is_contiguous()
    assert qtok.dtype == torch.int32 and qtok.is_contiguous() and tuple(qtok.shape) == (M, MAX_QUERY_TOKENS)
    assert tok.dtype == torch.int16 and tok.is_contiguous() and tok.shape[1] == L and tok.shape[0] >= n
    assert wemb.dtype == torch.bfloat16 and wemb.is_contiguous() and pemb.is_contiguous() and temb.is_contiguous()
    assert pemb.shape[0] >= max_pos and temb.shape[0] >= 2 and cu.numel() == M * P + 1
    T = int(T)
    y = torch.empty((T, H), dtype=torch.bfloat16, device=dev)
    dbg = [torch.empty(T, dtype=torch.int32, device=dev) for _ in range(3)] if debug else [None] * 3
    rc = _lib.lib().lzk_ce_embed_ln(rows.data_ptr(), M, P, n, qtok.data_ptr(), qlen.data_ptr(), tok.data_ptr(),
                                    dlen.data_ptr(), int(L), int(max_pos), cu.data_ptr(), T, int(cls_id), int(sep_id),
                                    int(vocab), wemb.data_ptr(), pemb.data_ptr(), temb.data_ptr(), g.data_ptr(),
                                    b.data_ptr(), H, float(eps), y.data_ptr(), _lib.ptr(dbg[0]), _lib.ptr(dbg[1]),
                                    _lib.ptr(dbg[2]), _lib.stream_ptr(dev))
    _lib.check(rc, "lzk_ce_embed_ln")
    return (y, *dbg) if debug else y


# ------------------------------------------------------------------ head
def select_ref(logits, rows, k: int):
    """The ``k`` largest ``logits`` [M, P] descending, ties to the lower row;
    (-inf, -1) where a slot's logit is -inf."""
    rows = rows.to(torch.long)
    big = torch.full_like(rows, torch.iinfo(torch.long).max)
    o1 = torch.argsort(torch.where(logits > NEG_INF, rows, big), dim=1, stable=True)
    o2 = torch.argsort(torch.gather(logits, 1, o1), dim=1, descending=True, stable=True)
    o = torch.gather(o1, 1, o2)[:, :k]
    s = torch.gather(logits, 1, o)
    r = torch.where(s > NEG_INF, torch.gather(rows, 1, o), torch.full_like(o, -1))
    return s, r


def ce_head_select_ref(pooled, rows, cls_w, cls_b, k: int, n: int):
    """Torch formulation of :func:`ce_head_select` (any device)."""
    M, P = rows.shape
    rows = rows.to(torch.long)
    lg = torch.tanh(pooled.float()) @ cls_w.float().reshape(-1) + cls_b.float().reshape(-1)[0]
    valid = (rows >= 0) & (rows < n)
    logits = torch.where(valid, lg.view(M, P), torch.full((M, P), NEG_INF, device=rows.device))
    s, r = select_ref(logits, rows, k)
    return s, r, logits


def ce_head_select(pooled: torch.Tensor, rows: torch.Tensor, cls_w: torch.Tensor, cls_b: torch.Tensor, k: int,
                   n: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(scores fp32 [M, k], rows int64 [M, k], logits fp32 [M, P]) from the
    pooler's dense output ``pooled`` [M * P, H] (bf16 on the device, before
    its tanh), the pool ``rows`` int64 [M, P], ``cls_w`` fp32 [H] and
    ``cls_b`` fp32 [1] (crossenc.hip ce_head_select_kernel). No host
    synchronisation."""
    if rows.dim() != 2:
        raise ValueError(f"rows must be [M, P] (got {tuple(rows.shape)})")
    M, P = rows.shape
    k = int(k)
    if not 1 <= P <= MAX_POOL or not 1 <= k <= P:
        raise ValueError(f"a pool holds 1 .. {MAX_POOL} slots and returns 1 .. P of them (P={P}, k={k})")
    if pooled.shape[0] != M * P:
        raise ValueError(f"{M * P} pairs but {pooled.shape[0]} pooled rows")
    if not rows.is_cuda or M == 0:
        return ce_head_select_ref(pooled, rows, cls_w, cls_b, k, n)
    dev = rows.device
    H = pooled.shape[1]
    assert pooled.dtype == torch.bfloat16 and pooled.stride(1) == 1
    assert rows.dtype == torch.long and rows.is_contiguous()
    assert cls_w.dtype == cls_b.dtype == torch.float32 and cls_w.numel() == H and cls_w.is_contiguous()
    scores = torch.empty((M, k), dtype=torch.float32, device=dev)
    out = torch.empty((M, k), dtype=torch.long, device=dev)
    logits = torch.empty((M, P), dtype=torch.float32, device=dev)
    ldx = pooled.stride(0) if M * P > 1 else max(pooled.stride(0), H)
    rc = _lib.lib().lzk_ce_head_select(pooled.data_ptr(), ldx, H, rows.data_ptr(), M, P, int(n), cls_w.data_ptr(),
                                       cls_b.data_ptr(), k, scores.data_ptr(), out.data_ptr(), logits.data_ptr(),
                                       _lib.stream_ptr(dev))
    _lib.check(rc, "lzk_ce_head_select")
    return scores, out, logits
