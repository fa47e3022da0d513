"""The token column of a tenant: every memory's first ``L`` body pieces on
the device, read by the cross-encoder re-ranker (``TenantGraph.token_column()``;
ops/crossenc_ops.py holds the contract).

A derived structure, exactly as engine/lexicon.py: not a NODE_COLS column,
never persisted, built on the first re-ranked search. A tenant that never
passes ``rerank=`` pays nothing.

Device columns. ``tok`` [cap, L] (16-bit id patterns held as int16) and
``dlen`` int32 [cap]: ``n * (2 L + 4)`` bytes. Rows [covered, g.n) are
tokenised and appended by the next :meth:`sync`; a row whose content was
rewritten (``_content_rewritten``) is tokenised again there; a change of
``row_epoch`` (compaction) drops everything and the next use rebuilds, and so
does another ``L`` or tokenizer (``TenantGraph.token_column`` makes a new
column then). Tokenising is host work (the native WordPiece tokenizer).
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from ..core.crossenc import MAX_VOCAB, check_doc_tokens
from ..ops.crossenc_ops import body_pieces


class TokenColumn:
    def __init__(self, g, tokenizer, L: int, vocab: int):
        if int(vocab) > MAX_VOCAB:
            raise ValueError(f"the token column stores 16-bit ids: vocabulary {vocab} exceeds {MAX_VOCAB}")
        self.g = g
        self.tokenizer = tokenizer
        self.L = check_doc_tokens(int(L))
        self.builds = 0
        self._reset()

    def _reset(self) -> None:
        self.tok: Optional[torch.Tensor] = None
        self.dlen: Optional[torch.Tensor] = None
        self.covered = 0
        self.epoch = -1
        self.dirty: Optional[list] = None

    # ---- upkeep
    def rewritten(self, r: int) -> None:
        if self.tok is not None and r < self.covered:
            if self.dirty is None:
                self.dirty = []
            self.dirty.append(int(r))

    def _pieces(self, rows):
        col = self.g.content
        if isinstance(rows, range) and rows.step == 1:
            texts = list(col[rows.start:rows.stop])
        else:
            texts = [col[r] for r in rows]
        ids, lens = body_pieces(self.tokenizer, texts, self.L)
        dev = self.g.device
        return (torch.from_numpy(ids.astype(np.uint16).view(np.int16)).to(dev), torch.from_numpy(lens).to(dev))

    def sync(self) -> "TokenColumn":
        """Bring the columns up to the tenant's rows [0, g.n)."""
        g = self.g
        n = g.n
        dev = g.device
        if self.tok is None or self.epoch != g.row_epoch or self.covered > n:
            self._reset()
            self.epoch = g.row_epoch
            self.builds += 1
        rows_cap = max(g.cap, n, 1)
        if self.tok is None or self.tok.shape[0] < n:
            tok = torch.zeros((rows_cap, self.L), dtype=torch.int16, device=dev)
            dlen = torch.zeros(rows_cap, dtype=torch.int32, device=dev)
            if self.tok is not None and self.covered:
                tok[: self.covered] = self.tok[: self.covered]
                dlen[: self.covered] = self.dlen[: self.covered]
            self.tok, self.dlen = tok, dlen
        a = self.covered
        if self.dirty:
            rows = sorted(set(r for r in self.dirty if r < a))
            if rows:
                ix = torch.as_tensor(rows, dtype=torch.long, device=dev)
                self.tok[ix], self.dlen[ix] = self._pieces(rows)
        self.dirty = None
        if a < n:
            self.tok[a:n], self.dlen[a:n] = self._pieces(range(a, n))
            self.covered = n
        return self

    def nbytes(self) -> int:
        return self.covered * (2 * self.L + 4)

    def state(self):
        """The covered rows on the host (tests): ids uint16 [covered, L], dlen."""
        c = self.covered
        return self.tok[:c].cpu().numpy().view(np.uint16), self.dlen[:c].cpu().numpy()
