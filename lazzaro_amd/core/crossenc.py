"""Settings of a cross-encoder re-ranked search, ``rerank=``.

The search of the other options runs at ``limit = pool``; every (query,
memory) pair of the pool is read as ONE sequence by a BERT cross-encoder
(models/cross_encoder.py) whose classification logit is the score, and the
``limit`` largest logits come back. ops/crossenc_ops.py holds the contract in
full.
"""
from __future__ import annotations

import numbers
from dataclasses import dataclass, fields
from typing import Any, Dict, Optional, Union

MAX_POOL = 64            # crossenc.hip CE_MAX_P: a pool is one search of at most 64 results
DEFAULT_POOL = 16
MAX_QUERY_TOKENS = 64    # crossenc.hip CE_MAX_Q: body pieces kept of a query
DOC_TOKEN_CHOICES = (32, 64, 128)  # L: body pieces kept of a memory (rerank_doc_tokens)
DEFAULT_DOC_TOKENS = 64
MAX_VOCAB = 65536        # the token column stores 16-bit ids


def check_doc_tokens(L) -> int:
    if isinstance(L, bool) or not isinstance(L, int) or L not in DOC_TOKEN_CHOICES:
        raise ValueError(f"rerank_doc_tokens must be one of {DOC_TOKEN_CHOICES} (got {L!r})")
    return int(L)


@dataclass(frozen=True)
class CrossRerank:
    pool: int = DEFAULT_POOL

    def __post_init__(self):
        v = self.pool
        if isinstance(v, bool) or not isinstance(v, int):
            if isinstance(v, float) and v.is_integer():
                v = int(v)
            else:
                raise ValueError(f"pool must be an integer (got {v!r})")
        object.__setattr__(self, "pool", int(v))
        if not 1 <= self.pool <= MAX_POOL:
            raise ValueError(f"pool must be in 1 .. {MAX_POOL} (got {self.pool})")

    def to_dict(self) -> Dict[str, Any]:
        return {f.name: getattr(self, f.name) for f in fields(self)}

    @classmethod
    def coerce(cls, rerank: Union[None, bool, int, "CrossRerank", Dict[str, Any]]) -> Optional["CrossRerank"]:
        """``rerank`` as given to a search: settings, a dict of their fields,
        an int (the pool), True (the defaults), or None / False (off)."""
        if rerank is None or rerank is False or isinstance(rerank, cls):
            return rerank or None
        if rerank is True:
            return cls()
        if isinstance(rerank, int):
            return cls(pool=rerank)
        if isinstance(rerank, dict):
            unknown = set(rerank) - {f.name for f in fields(cls)}
            if unknown:
                raise ValueError(f"unknown rerank field(s): {sorted(unknown)}")
            return cls(**rerank)
        raise ValueError("rerank must be True, an int (the pool), a dict or a CrossRerank, not "
                         f"{type(rerank).__name__}")

    def check_limit(self, limit) -> None:
        """Raises ValueError, before any work, unless ``1 <= limit <= pool``."""
        if isinstance(limit, bool) or not isinstance(limit, numbers.Integral) or limit < 1:
            raise ValueError(f"a re-ranked search returns 1 .. {MAX_POOL} results (limit={limit!r})")
        if limit > self.pool:
            raise ValueError(f"rerank pool {self.pool} is below the limit {limit}: pool must be in limit .. {MAX_POOL}")
