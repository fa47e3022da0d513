"""fp64 oracle of the cross-encoder re-ranker (lazzaro_amd/ops/crossenc_ops.py
holds the contract): the pair assembly, the BERT forward with token types, the
pooler and classifier, and the selection -- numpy / torch in fp64, nothing here
imports the kernel library. Also the shared recipes of the CPU and GPU tests.
"""
from __future__ import annotations

import math
from typing import Dict, NamedTuple

import numpy as np
import torch

MAX_QUERY_TOKENS = 64
CLS, SEP = 101, 102


class Pairs(NamedTuple):
    lens: np.ndarray    # int32 [B]
    cu: np.ndarray      # int32 [B + 1]
    ids: np.ndarray     # int32 [T]
    pos: np.ndarray     # int32 [T]
    types: np.ndarray   # int32 [T]
    T: int
    S_max: int


def pair_assembly(rows, qtok, qlen, tok, dlen, max_pos: int, L: int, cls_id: int = CLS, sep_id: int = SEP) -> Pairs:
    """The contract's pair rule, one slice-built sequence per slot. ``rows``
    [M, P] (a slot < 0 or >= n is empty), ``qtok`` [M, 64], ``qlen`` [M],
    ``tok`` [n, L] (16-bit patterns in any integer dtype), ``dlen`` [n]."""
    rows = np.asarray(rows, dtype=np.int64)
    M, P = rows.shape
    n = len(dlen)
    tok = np.asarray(tok).astype(np.int64) & 0xFFFF
    seqs, typs = [], []
    for m in range(M):
        for j in range(P):
            r = int(rows[m, j])
            if r < 0 or r >= n:
                seqs.append([cls_id, sep_id, sep_id])
                typs.append([0, 0, 1])
                continue
            ql = int(qlen[m])
            dl = min(int(dlen[r]), L, max_pos - 3 - ql)
            assert 0 <= ql <= MAX_QUERY_TOKENS and dl >= 0
            q = [int(x) for x in qtok[m, :ql]]
            d = [int(x) for x in tok[r, :dl]]
            seqs.append([cls_id] + q + [sep_id] + d + [sep_id])
            typs.append([0] * (ql + 2) + [1] * (dl + 1))
    lens = np.asarray([len(s) for s in seqs], dtype=np.int32)
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ids = np.asarray([x for s in seqs for x in s], dtype=np.int32)
    pos = np.asarray([p for s in seqs for p in range(len(s))], dtype=np.int32)
    types = np.asarray([x for t in typs for x in t], dtype=np.int32)
    return Pairs(lens, cu, ids, pos, types, int(cu[-1]), int(lens.max()) if len(lens) else 0)


def _f64(t):
    return t.detach().to("cpu", torch.float64)


def params64(p: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """A CrossEncoder's parameters (``.p``) in fp64 on the host."""
    return {k: _f64(v) for k, v in p.items()}


def _ln(v, g, b, eps):
    mean = v.mean(dim=-1, keepdim=True)
    var = ((v - mean) ** 2).mean(dim=-1, keepdim=True)
    return g * (v - mean) / torch.sqrt(var + eps) + b


def gelu64(z):
    return 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))


def embed64(p, ids, pos, types, eps):
    ids, pos, types = (torch.as_tensor(np.asarray(a), dtype=torch.long) for a in (ids, pos, types))
    v = p["word"][ids] + p["pos"][pos] + p["type"][types]
    return v, _ln(v, p["emb_g"], p["emb_b"], eps)


def forward64(p, cfg, pairs: Pairs):
    """(logits fp64 [B], pooler dense output before its tanh fp64 [B, H]) of
    the packed sequences: plain BERT, one sequence at a time."""
    H, nh = cfg.hidden, cfg.heads
    hd = H // nh
    _, x = embed64(p, pairs.ids, pairs.pos, pairs.types, cfg.eps)
    cls = []
    for b in range(len(pairs.lens)):
        h = x[int(pairs.cu[b]):int(pairs.cu[b + 1])]
        S = h.shape[0]
        for i in range(cfg.layers):
            qkv = h @ p[f"{i}.wqkv"].T + p[f"{i}.bqkv"]
            q, k, v = (qkv[:, j * H:(j + 1) * H].reshape(S, nh, hd).transpose(0, 1) for j in range(3))
            a = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(hd), dim=-1) @ v
            ctx = a.transpose(0, 1).reshape(S, H)
            h = _ln(ctx @ p[f"{i}.wo"].T + p[f"{i}.bo"] + h, p[f"{i}.ln1_g"], p[f"{i}.ln1_b"], cfg.eps)
            f = gelu64(h @ p[f"{i}.w1"].T + p[f"{i}.b1"])
            h = _ln(f @ p[f"{i}.w2"].T + p[f"{i}.b2"] + h, p[f"{i}.ln2_g"], p[f"{i}.ln2_b"], cfg.eps)
        cls.append(h[0])
    hc = torch.stack(cls)
    dense = hc @ p["pool_w"].T + p["pool_b"]
    return head64(dense, p["cls_w"], p["cls_b"]), dense


def head64(dense, cls_w, cls_b):
    """logit = <wc, tanh(dense)> + bc in fp64 (a row-wise sum, not a matmul:
    equal rows give equal bits wherever they stand in the batch)."""
    return (torch.tanh(_f64(dense)) * _f64(cls_w).reshape(1, -1)).sum(dim=1) + _f64(cls_b).reshape(-1)[0]


def pool_logits(logits, rows, n: int):
    """[M, P] in pool order, -inf in the empty slots."""
    rows = np.asarray(rows, dtype=np.int64)
    lg = np.asarray(logits, dtype=np.float64).reshape(rows.shape).copy()
    lg[(rows < 0) | (rows >= n)] = -np.inf
    return lg


def select(logits, rows, k: int):
    """The ``k`` largest logits per query, descending, ties to the lower
    row; (-inf, -1) once the real rows run out. ``logits`` [M, P] with -inf
    in the empty slots. Returns (scores float64 [M, k], rows int64 [M, k])."""
    rows = np.asarray(rows, dtype=np.int64)
    logits = np.asarray(logits, dtype=np.float64)
    M, P = rows.shape
    s = np.full((M, k), -np.inf)
    r = np.full((M, k), -1, dtype=np.int64)
    for m in range(M):
        live = [(-(logits[m, j] + 0.0), int(rows[m, j])) for j in range(P) if logits[m, j] > -np.inf]
        live.sort()
        for i, (neg, row) in enumerate(live[:k]):
            s[m, i], r[m, i] = -neg, row
    return s, r


# ------------------------------------------------------------------ recipes
def lens_case(B: int, L: int = 64, max_pos: int = 128, seed: int = 0):
    """(rows [M, P], qlen [M], dlen [n]) with ``M * P == B`` whose first slots
    hold, as far as B reaches: an empty slot; ``ql = 0``; ``dlen = 0``; a
    memory longer than L; and ``ql = 64`` with ``dlen = 64`` (the ``max_pos``
    truncation, ``dl = 61`` at max_pos 128). The rest is random."""
    rng = np.random.default_rng(seed + B)
    P = 5 if B % 5 == 0 else 1
    M = B // P
    n = 50
    dlen = rng.integers(1, L + 1, size=n).astype(np.int32)
    dlen[0], dlen[1], dlen[2] = 0, L + 70, 64
    qlen = rng.integers(1, MAX_QUERY_TOKENS + 1, size=M).astype(np.int32)
    rows = rng.integers(0, n, size=(M, P)).astype(np.int64)
    rows[rng.random((M, P)) < 0.1] = -1
    if M >= 6:
        qlen[0], qlen[1], qlen[2] = 0, 64, 10
        rows[0, 0], rows[1, 0], rows[2, 0], rows[3, 0], rows[4, 0] = 7, 2, -1, 0, 1
        rows[5, 0] = n + 3  # past the column: empty
    elif B == 5:
        qlen[0] = 64
        rows[0] = [-1, 2, 0, 1, 9]
    else:
        qlen[0] = 64
        rows[0, 0] = 2
    return rows, qlen, dlen


def token_case(M: int, P: int, n: int, L: int, vocab: int, seed: int = 0, max_pos: int = 128):
    """Random pools with every kind of slot, queries' and memories' tokens:
    (rows, qtok, qlen, tok int16 patterns, dlen)."""
    rng = np.random.default_rng(seed)
    qcap = min(MAX_QUERY_TOKENS, max_pos - 3)
    qlen = rng.integers(0, qcap + 1, size=M).astype(np.int32)
    qlen[0] = qcap
    if M > 1:
        qlen[1] = 0
    qtok = rng.integers(1000, vocab, size=(M, MAX_QUERY_TOKENS)).astype(np.int32)
    qtok[np.arange(MAX_QUERY_TOKENS)[None, :] >= qlen[:, None]] = 0
    dlen = rng.integers(0, L + 1, size=n).astype(np.int32)
    dlen[0], dlen[1] = 0, L
    tok = rng.integers(1000, vocab, size=(n, L)).astype(np.int64)
    tok[np.arange(L)[None, :] >= dlen[:, None]] = 0
    rows = np.stack([rng.permutation(n)[:P] for _ in range(M)]).astype(np.int64)
    rows[rng.random((M, P)) < 0.15] = -1
    rows[0, 0], rows[0, P - 1] = 1, 0  # the full memory under the longest query, and the empty one
    rows[M - 1, 0] = -1
    return rows, qtok, qlen, tok.astype(np.uint16).view(np.int16), dlen


# (H, M, P, k, what): the head's cases -- ties from duplicated pooler rows, empty slots, limit = 1, limit = P, P = 64
HEAD_CASES = [(128, 3, 5, 1, "ties"), (128, 3, 5, 5, "ties"), (384, 4, 16, 7, "ties"), (1024, 2, 64, 64, "ties"),
              (384, 2, 64, 16, "plain"),
              # the shared wave sort (lzk_topk64.h) with a nearly empty and a full 64-entry block, a prefix of 4 returned
              (128, 3, 5, 4, "ties"), (1024, 2, 64, 4, "ties")]


def head_case(H: int, M: int, P: int, what: str, seed: int = 0):
    """(dense bf16 [M * P, H], rows [M, P], wc fp32 [H], bc fp32 [1], n). The
    pooler outputs are spread so that distinct rows' fp64 logits lie far
    further apart than the head's tolerance (the CPU tier checks it); under ``ties`` slots 1 and 3 of
    every query repeat slot 0's pooler row (equal logits, bit for bit), and
    slot 2 is empty."""
    g = torch.Generator().manual_seed(seed + H + P)
    n = 4 * P + 7
    wc = (torch.randn(H, generator=g) * 0.05).float()
    # slot j's row is level_j * sign(wc) plus noise: its logit is close to sum |wc| * tanh(level_j), and the
    # P levels (in a random slot order) are spread evenly over tanh's range
    level = torch.stack([torch.atanh(-0.9 + 1.8 * (torch.randperm(P, generator=g) + 0.5) / P) for _ in range(M)])
    dense = level.reshape(-1, 1) * torch.sign(wc)[None, :] + 0.05 * torch.randn(M * P, H, generator=g)
    dense = dense.to(torch.bfloat16)
    bc = torch.tensor([0.03125 + 0.001], dtype=torch.float32)
    rows = torch.stack([torch.randperm(n, generator=g)[:P] for _ in range(M)]).long()
    if what == "ties":
        d = dense.view(M, P, H)
        d[:, 1] = d[:, 0]
        if P > 3:
            d[:, 3] = d[:, 0]
        rows[:, 2] = -1
        rows[M - 1, P - 1] = n + 1  # past the rows: empty too
    return dense, rows, wc, bc, n
