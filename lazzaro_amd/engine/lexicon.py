"""The lexicon of a tenant: the lexical index keyword search reads
(``TenantGraph.lexicon()``; core/lexical.py defines the terms, ops/lex_ops.py
the scores).

A derived structure, like the type-code column: not a NODE_COLS column, not
persisted, built on the first lexical search. A tenant that never passes
``lexical=`` pays nothing.

Device columns. ``slots`` [cap, W] (uint32 bit patterns held as int32) and
``dl`` int32 [cap]. Rows [covered, g.n) are tokenised and appended by the next
:meth:`sync`; a row whose content was rewritten (``_content_rewritten``) is
tokenised again there; a change of ``row_epoch`` (compaction) drops everything
and the next use rebuilds.

Host side, over the covered rows: the document-frequency table (sorted term
ids + counts), ``N`` = the rows with ``dl > 0`` and ``sum_dl``. Limit: an
evicted row keeps counting in all three (and keeps its slots; its bias is -inf,
so it is never returned) until the next rebuild. Re-tokenising a rewritten
row reads its old slots back from the device (one small copy, a host
synchronisation, only when rows were rewritten).
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from ..core.lexical import DEFAULT_SLOTS, SLOT_CHOICES, as_query_terms, lex_terms


class Lexicon:
    def __init__(self, g, slots: int = DEFAULT_SLOTS):
        if int(slots) not in SLOT_CHOICES:
            raise ValueError(f"lexical_slots must be one of {SLOT_CHOICES} (got {slots})")
        self.g = g
        self.W = int(slots)
        self.builds = 0
        self._reset()

    def _reset(self) -> None:
        self.slots: Optional[torch.Tensor] = None
        self.dl: Optional[torch.Tensor] = None
        self.covered = 0
        self.epoch = -1
        self.dirty: Optional[list] = None
        self.df_terms = np.zeros(0, dtype=np.uint32)
        self.df_counts = np.zeros(0, dtype=np.int64)
        self.N = 0
        self.sum_dl = 0

    # ---- upkeep
    def rewritten(self, r: int) -> None:
        if self.slots is not None and r < self.covered:
            if self.dirty is None:
                self.dirty = []
            self.dirty.append(int(r))

    def _texts(self, rows) -> list:
        col = self.g.content
        if isinstance(rows, range) and rows.step == 1:
            return list(col[rows.start:rows.stop])
        return [col[r] for r in rows]

    def _df_add(self, slots_u32: np.ndarray, sign: int) -> None:
        t = (slots_u32[slots_u32 != 0] >> np.uint32(8)).astype(np.uint32)
        if t.size == 0:
            return
        u, c = np.unique(t, return_counts=True)
        terms = np.concatenate([self.df_terms, u])
        counts = np.concatenate([self.df_counts, sign * c.astype(np.int64)])
        terms, inv = np.unique(terms, return_inverse=True)
        tot = np.zeros(len(terms), dtype=np.int64)
        np.add.at(tot, inv, counts)
        keep = tot > 0
        self.df_terms, self.df_counts = terms[keep], tot[keep]

    def sync(self) -> "Lexicon":
        """Bring the columns and the host statistics up to the tenant's rows
        [0, g.n)."""
        g = self.g
        n = g.n
        dev = g.device
        if self.slots is None or self.epoch != g.row_epoch or self.covered > n:
            self._reset()
            self.epoch = g.row_epoch
            self.builds += 1
        rows_cap = max(g.cap, n, 1)
        if self.slots is None or self.slots.shape[0] < n:
            slots = torch.zeros((rows_cap, self.W), dtype=torch.int32, device=dev)
            dl = torch.zeros(rows_cap, dtype=torch.int32, device=dev)
            if self.slots is not None and self.covered:
                slots[: self.covered] = self.slots[: self.covered]
                dl[: self.covered] = self.dl[: self.covered]
            self.slots, self.dl = slots, dl
        a = self.covered
        if self.dirty:
            rows = sorted(set(r for r in self.dirty if r < a))
            if rows:
                ix = torch.as_tensor(rows, dtype=torch.long, device=dev)
                old_s = self.slots[ix].cpu().numpy().view(np.uint32)
                old_dl = self.dl[ix].cpu().numpy()
                new_s, new_dl = lex_terms(self._texts(rows), self.W)
                self._df_add(old_s, -1)
                self._df_add(new_s, +1)
                self.N += int((new_dl > 0).sum()) - int((old_dl > 0).sum())
                self.sum_dl += int(new_dl.astype(np.int64).sum()) - int(old_dl.astype(np.int64).sum())
                self.slots[ix] = torch.from_numpy(np.ascontiguousarray(new_s).view(np.int32)).to(dev)
                self.dl[ix] = torch.from_numpy(np.ascontiguousarray(new_dl)).to(dev)
        self.dirty = None
        if a < n:
            s, d = lex_terms(self._texts(range(a, n)), self.W)
            self.slots[a:n] = torch.from_numpy(np.ascontiguousarray(s).view(np.int32)).to(dev)
            self.dl[a:n] = torch.from_numpy(np.ascontiguousarray(d)).to(dev)
            self._df_add(s, +1)
            self.N += int((d > 0).sum())
            self.sum_dl += int(d.astype(np.int64).sum())
            self.covered = n
        return self

    # ---- statistics the scores take
    @property
    def avgdl(self) -> float:
        """``sum_dl / N`` in fp64 (1 for a lexicon without words: no row can match then)."""
        return float(self.sum_dl) / float(self.N) if self.N > 0 else 1.0

    def df(self, qterms) -> np.ndarray:
        qt = np.asarray(qterms, dtype=np.uint32)
        if len(self.df_terms) == 0:
            return np.zeros(qt.shape, dtype=np.int64)
        i = np.minimum(np.searchsorted(self.df_terms, qt), len(self.df_terms) - 1)
        return np.where(self.df_terms[i] == qt, self.df_counts[i], 0)

    def weights(self, qterms) -> np.ndarray:
        """float64 [M, T]: ``idf(t) = log1p((N - df + 0.5) / (df + 0.5))`` of
        every query term, 0 for an unused slot."""
        qt = np.asarray(qterms, dtype=np.uint32)
        if qt.ndim == 1:
            qt = qt[None, :]
        df = self.df(qt).astype(np.float64)
        w = np.log1p((float(self.N) - df + 0.5) / (df + 0.5))
        return np.where(qt > 0, w, 0.0)

    def query(self, texts_or_terms):
        """(qterms uint32 [M, 32], weights float64 [M, 32]) of a batch of
        query texts (or of term-id rows)."""
        qt = as_query_terms(texts_or_terms)
        return qt, self.weights(qt)

    def state(self):
        """The whole lexicon on the host (tests): slots, dl, df terms and
        counts, N, sum_dl."""
        c = self.covered
        return (self.slots[:c].cpu().numpy().view(np.uint32), self.dl[:c].cpu().numpy(), self.df_terms.copy(),
                self.df_counts.copy(), self.N, self.sum_dl)
