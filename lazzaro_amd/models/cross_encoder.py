"""BERT cross-encoder for re-ranking (``rerank=``): a sentence encoder's
parameters plus the pooler and a one-label classifier, HF
``BertForSequenceClassification`` (``cross-encoder/ms-marco-MiniLM-L-6-v2`` has
exactly the shape of the ``minilm-l6`` config).

The forward runs over device-prepared packed pairs -- ``ops.crossenc_ops``
assembles and embeds them on the device, nothing is packed on the host -- with
the encoder's own ops unchanged (``E.linear``, ``E.attention(cu=)``,
``E.layernorm``), the last layer past its attention on the CLS rows only, the
pooler's dense as one more ``E.linear``, and the tanh, the classifier and the
selection in one kernel (``ce_head_select``). bf16 on the device; the CPU tier
takes fp32 parameters through the same code.

Host synchronisation: ONE 8-byte read-back of ``stat = (T, S_max)`` per chunk,
to size the packed forward.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np
import torch

from ..core.crossenc import DEFAULT_DOC_TOKENS, MAX_QUERY_TOKENS, MAX_VOCAB, check_doc_tokens
from ..ops import crossenc_ops as X
from ..ops import encoder_ops as E
from .encoder import SentenceEncoder, _to_dev, get_config

# Tokens per chunk of queries (an upper bound known on the host: sum over the
# chunk of P * (3 + ql_m + L)). The largest activation of a layer is the FFN's,
# T * ffn * 2 bytes in bf16: 262,144 tokens are 0.75 GiB at ffn = 1536
# (minilm-l6), 1.5 GiB at 3072 and 2 GiB at 4096 -- beside T * 3H * 2 for the
# QKV and three T * H * 2 buffers, under 4 GiB in all at every config here.
CE_TOKEN_BUDGET = 262144


class CrossEncoder:
    """Weights + the pair forward. Without ``weights`` everything is
    random-init from ``seed`` with std 0.02, the encoder as ``SentenceEncoder``
    does and the pooler and classifier after it."""

    CLS_LAST = True  # False: the full last layer, then the CLS rows (A/B and tests)

    def __init__(self, config, device=None, weights: Optional[str] = None, vocab_file: Optional[str] = None,
                 seed: int = 0, dtype=None):
        self.cfg = get_config(config) if isinstance(config, str) else config
        if self.cfg.vocab > MAX_VOCAB:
            raise ValueError(f"the token column stores 16-bit ids: vocabulary {self.cfg.vocab} exceeds {MAX_VOCAB}")
        self.device = torch.device(device) if device is not None else torch.device("cpu")
        if dtype is None:
            dtype = torch.bfloat16 if self.device.type == "cuda" else torch.float32
        if self.device.type == "cuda" and dtype != torch.bfloat16:
            raise ValueError("the cross-encoder runs in bf16 on the device")
        self.dtype = dtype
        self.enc = SentenceEncoder(self.cfg, device=self.device, seed=seed, dtype=dtype)
        self.p = self.enc.p
        H = self.cfg.hidden
        g = torch.Generator(device="cpu").manual_seed(seed + 1)
        self.p["pool_w"] = (torch.randn(H, H, generator=g) * 0.02).to(self.device, dtype)
        self.p["pool_b"] = (torch.randn(H, generator=g) * 0.02).to(self.device, torch.float32)
        self.p["cls_w"] = (torch.randn(H, generator=g) * 0.02).to(self.device, torch.float32)
        self.p["cls_b"] = (torch.randn(1, generator=g) * 0.02).to(self.device, torch.float32)
        if weights:
            self.load_safetensors(weights)
        self.vocab_file = vocab_file
        self._tok = None
        self._special = None

    # --------------------------------------------------------------- weights
    def load_safetensors(self, path: str) -> None:
        """HF ``BertForSequenceClassification`` naming: ``bert.*``,
        ``bert.pooler.dense.{weight,bias}``, ``classifier.{weight,bias}`` with
        one label."""
        from safetensors.torch import load_file
        sd = load_file(path)
        for k in ("bert.pooler.dense.weight", "bert.pooler.dense.bias", "classifier.weight", "classifier.bias"):
            if k not in sd:
                raise ValueError(f"{path} holds no {k}: not a BertForSequenceClassification checkpoint")
        if sd["classifier.weight"].shape[0] != 1:
            raise ValueError(f"the classifier has {sd['classifier.weight'].shape[0]} labels: a re-ranker has one")
        self.enc.load_safetensors(path)
        dev = self.device
        self.p["pool_w"] = sd["bert.pooler.dense.weight"].to(dev, self.dtype).contiguous()
        self.p["pool_b"] = sd["bert.pooler.dense.bias"].float().to(dev)
        self.p["cls_w"] = sd["classifier.weight"].float().reshape(-1).to(dev).contiguous()
        self.p["cls_b"] = sd["classifier.bias"].float().reshape(1).to(dev)

    # --------------------------------------------------------------- tokens
    @property
    def tokenizer(self):
        if self._tok is None:
            from ..core.embedders import Tokenizer
            self._tok = Tokenizer(self.vocab_file, vocab_size=self.cfg.vocab)
        return self._tok

    @property
    def special_ids(self) -> Tuple[int, int]:
        """([CLS], [SEP]) of the tokenizer."""
        if self._special is None:
            both = self.tokenizer.encode("", 2)
            self._special = (int(both[0]), int(both[-1]))
        return self._special

    # --------------------------------------------------------------- forward
    def pooled(self, rows, qtok, qlen, tok, dlen, L: int, special=None, stat=None):
        """The pooler's dense output (before its tanh) [M * P, H] of the pairs
        of ``rows`` int64 [M, P] -- every tensor on the encoder's device."""
        c, p = self.cfg, self.p
        cls_id, sep_id = special if special is not None else self.special_ids
        M, P = rows.shape
        B = M * P
        lens, cu, st = X.ce_lens(rows, qlen, dlen, c.max_pos, L)
        T, S = (int(v) for v in (st.cpu().tolist() if stat is None else stat))  # the one read-back: sizes the forward
        x = X.ce_embed_ln(rows, qtok, qlen, tok, dlen, cu, T, c.max_pos, L, cls_id, sep_id, p["word"], p["pos"],
                          p["type"], p["emb_g"], p["emb_b"], c.eps)
        x = self.layers(x, lens, cu, B, S)
        return E.linear(x, p["pool_w"], p["pool_b"])

    def layers(self, x, lens, cu, B: int, S: int):
        """Every transformer layer over the packed tokens ``x`` [T, H];
        returns the CLS rows' last states [B, H]."""
        c, p = self.cfg, self.p
        first = cu[:-1].long()
        for i in range(c.layers):
            qkv = E.linear(x, p[f"{i}.wqkv"], p[f"{i}.bqkv"])
            ctx = E.attention(qkv, lens, B, S, c.heads, cu=cu)
            if self.CLS_LAST and i == c.layers - 1:
                ctx, x = ctx.index_select(0, first), x.index_select(0, first)
            x = E.layernorm(E.linear(ctx, p[f"{i}.wo"], p[f"{i}.bo"], residual=x), p[f"{i}.ln1_g"], p[f"{i}.ln1_b"],
                            c.eps)
            hdn = E.linear(x, p[f"{i}.w1"], p[f"{i}.b1"], act="gelu")
            x = E.layernorm(E.linear(hdn, p[f"{i}.w2"], p[f"{i}.b2"], residual=x), p[f"{i}.ln2_g"], p[f"{i}.ln2_b"],
                            c.eps)
        return x if self.CLS_LAST else x.index_select(0, first)

    @staticmethod
    def chunks(qlen: np.ndarray, P: int, L: int, budget: int = CE_TOKEN_BUDGET) -> List[Tuple[int, int]]:
        """[a, b) ranges of queries whose pairs hold at most ``budget`` tokens
        (by the host's bound ``P * (3 + ql_m + L)``) and at most 65,536 pairs;
        a range always holds one query at least."""
        out, a, tot = [], 0, 0
        for m, ql in enumerate(np.asarray(qlen).tolist()):
            t = P * (3 + int(ql) + L)
            if m > a and (tot + t > budget or (m - a + 1) * P > X.MAX_PAIRS):
                out.append((a, m))
                a, tot = m, 0
            tot += t
        if len(qlen) > a:
            out.append((a, len(qlen)))
        return out

    def rerank(self, rows, qtok, qlen, tok, dlen, k: int, L: int = DEFAULT_DOC_TOKENS, n: Optional[int] = None):
        """(scores fp32 [M, k], rows int64 [M, k], logits fp32 [M, P]) of the
        pools ``rows`` int64 [M, P] (on the device); ``qtok`` / ``qlen`` the
        queries' tokens on the HOST (numpy int32 [M, 64] / [M]); ``tok`` /
        ``dlen`` the token column on the device."""
        L = check_doc_tokens(int(L))
        M, P = rows.shape
        dev = rows.device
        n = int(dlen.numel() if n is None else n)
        qtok, qlen = np.ascontiguousarray(qtok, dtype=np.int32), np.ascontiguousarray(qlen, dtype=np.int32)
        if qtok.shape != (M, MAX_QUERY_TOKENS) or qlen.shape != (M,):
            raise ValueError(f"{M} pools but query tokens {qtok.shape} / lengths {qlen.shape}")
        rows = rows.to(torch.long).contiguous()
        qt_d, ql_d = _to_dev(torch.from_numpy(qtok), dev), _to_dev(torch.from_numpy(qlen), dev)
        outs = []
        for a, b in self.chunks(qlen, P, L):
            r = rows[a:b]
            pooled = self.pooled(r, qt_d[a:b], ql_d[a:b], tok, dlen[:n], L)
            outs.append(X.ce_head_select(pooled, r, self.p["cls_w"], self.p["cls_b"], k, n))
        if not outs:
            return (torch.empty((0, k), dtype=torch.float32, device=dev),
                    torch.empty((0, k), dtype=torch.long, device=dev),
                    torch.empty((0, P), dtype=torch.float32, device=dev))
        if len(outs) == 1:
            return outs[0]
        return tuple(torch.cat([o[i] for o in outs]) for i in range(3))

    def flops(self, tokens: int) -> float:
        return self.enc.flops(tokens)
