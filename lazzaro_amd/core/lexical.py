"""Keyword and hybrid search, ``lexical=``: the terms of a text and the
settings of a search.

Words. A text's words are the tokens of the runtime tokenizer's basic split
(``Tokenizer::basic_split``: control characters removed, CJK ideographs
isolated, NFD with combining marks dropped and lower-casing, split on
whitespace and on every Unicode punctuation mark) that hold at least one
alphanumeric code point. No stemming, no stop list.

Term id. 24 bits: ``h`` = FNV-1a 32 over the word's UTF-8 bytes (offset
2166136261, prime 16777619), ``t = (h ^ (h >> 24)) & 0xFFFFFF``, 0 mapped to
1. Two words with the same ``t`` are the same term: that is the contract.

Row of slots. The distinct terms of a text in order of first appearance, the
first ``W`` kept; ``tf`` = a kept term's occurrences, saturated at 255; a slot
is ``(t << 8) | tf``; used slots first, ascending by ``t``, then zeros. ``dl``
is the number of words (those of dropped terms included), clipped at 65,535.

Query. At most ``T_MAX = 32`` distinct terms, the first 32 by appearance,
ascending, zeros after; ``tf`` is ignored.

``lex_terms`` is the native function (``_lzrt.lex_terms``) where the runtime
is built and ``terms_py`` -- the same definition on ``unicodedata`` -- where
it is not; the tests hold the two to each other.
"""
from __future__ import annotations

import math
import unicodedata
from dataclasses import dataclass, fields
from typing import Any, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

T_MAX = 32            # query terms kept per query
SLOT_CHOICES = (8, 16, 32)
DEFAULT_SLOTS = 16
MAX_POOL = 64         # lexical.hip: the fused candidates of one query are two pools of at most 64
DEFAULT_POOL = 16     # CAND_SLOTS: the dense pool stays on the fast candidate routes
MAX_DL = 65535
FNV_OFFSET = 2166136261
FNV_PRIME = 16777619


def term_id(word: str) -> int:
    h = FNV_OFFSET
    for c in word.encode("utf-8"):
        h = ((h ^ c) * FNV_PRIME) & 0xFFFFFFFF
    t = (h ^ (h >> 24)) & 0xFFFFFF
    return t or 1


def _is_cjk(c: int) -> bool:
    return (0x4E00 <= c <= 0x9FFF or 0x3400 <= c <= 0x4DBF or 0x20000 <= c <= 0x2A6DF or 0x2A700 <= c <= 0x2B73F
            or 0x2B740 <= c <= 0x2B81F or 0x2B820 <= c <= 0x2CEAF or 0xF900 <= c <= 0xFAFF or 0x2F800 <= c <= 0x2FA1F)


def _is_space(ch: str) -> bool:
    return ch in " \t\n\r\u2028\u2029" or unicodedata.category(ch) == "Zs"


def _is_punct(ch: str) -> bool:
    c = ord(ch)
    if 33 <= c <= 47 or 58 <= c <= 64 or 91 <= c <= 96 or 123 <= c <= 126:
        return True
    return c >= 0x80 and unicodedata.category(ch).startswith("P")


def split_py(text: str) -> List[str]:
    """The basic split (csrc/runtime/tokenizer.cpp ``basic_split``, uncased)
    on ``unicodedata``: every token, punctuation marks included."""
    out: List[str] = []
    cur: List[str] = []

    def flush():
        if cur:
            out.append("".join(cur))
            cur.clear()

    def emit(ch: str):
        if _is_space(ch):
            flush()
        elif _is_punct(ch):
            flush()
            out.append(ch)
        else:
            cur.append(ch)

    for ch in text:
        c = ord(ch)
        if c == 0 or c == 0xFFFD or 0xD800 <= c <= 0xDFFF:
            continue
        if ch not in "\t\n\r" and unicodedata.category(ch) in ("Cc", "Cf", "Co"):
            continue
        if _is_space(ch):
            flush()
        elif _is_cjk(c):
            flush()
            out.append(ch)
        elif c < 0x80:
            emit(ch.lower())
        elif c >= 0x10000:  # (the runtime's fold table covers the BMP)
            emit(ch)
        else:
            t = "".join(x for x in unicodedata.normalize("NFD", ch) if unicodedata.category(x) != "Mn").lower()
            for x in t:
                emit(x)
    flush()
    return out


def words_py(text: str) -> List[str]:
    """The words of ``text``: the tokens with an alphanumeric code point."""
    return [w for w in split_py(text) if any(ch.isalnum() for ch in w)]


def terms_py(texts: Sequence[str], slots: int) -> Tuple[np.ndarray, np.ndarray]:
    """(uint32 [n, slots], int32 [n]): the rows of slots and ``dl`` of
    ``texts``, in pure Python."""
    W = int(slots)
    if not 1 <= W <= 64:
        raise ValueError(f"slots must be in 1 .. 64 (got {slots})")
    out = np.zeros((len(texts), W), dtype=np.uint32)
    dl = np.zeros(len(texts), dtype=np.int32)
    for i, text in enumerate(texts):
        kept: Dict[int, int] = {}
        n = 0
        for w in words_py(text):
            n += 1
            t = term_id(w)
            if t in kept:
                kept[t] = min(255, kept[t] + 1)
            elif len(kept) < W:
                kept[t] = 1
        for j, t in enumerate(sorted(kept)):
            out[i, j] = (t << 8) | kept[t]
        dl[i] = min(n, MAX_DL)
    return out, dl


def _native():
    try:
        from .._lib import _lzrt  # type: ignore
    except ImportError:  # pragma: no cover - the runtime ships with the package build
        return None
    return getattr(_lzrt, "lex_terms", None)


def lex_terms(texts: Sequence[str], slots: int) -> Tuple[np.ndarray, np.ndarray]:
    """Rows of slots and ``dl`` of ``texts`` (the native runtime; ``terms_py``
    where it is not built)."""
    fn = _native()
    texts = texts if isinstance(texts, list) else list(texts)
    if fn is None:
        return terms_py(texts, slots)
    return fn(texts, int(slots))


def query_terms(texts: Sequence[str]) -> np.ndarray:
    """uint32 [M, T_MAX]: each query's terms, ascending, zeros after."""
    if isinstance(texts, str):
        texts = [texts]
    return np.ascontiguousarray(lex_terms(texts, T_MAX)[0] >> np.uint32(8))


def as_query_terms(q) -> np.ndarray:
    """``q`` -- a text, a list of texts or an integer array [M, T <= T_MAX] of
    term ids -- as uint32 [M, T_MAX]: used terms first, ascending and
    distinct, zeros after."""
    if isinstance(q, str) or (isinstance(q, (list, tuple)) and all(isinstance(x, str) for x in q)):
        return query_terms(q)
    a = np.asarray(q.cpu() if hasattr(q, "cpu") else q)
    if a.dtype == np.uint32 and a.ndim == 2 and a.shape[1] == T_MAX and a.max(initial=0) <= 0xFFFFFF:
        u = a > 0  # already in form (what query_terms returns): nothing to do
        if not (u[:, 1:] & ~u[:, :-1]).any() and not (u[:, 1:] & (a[:, 1:] <= a[:, :-1])).any():
            return np.ascontiguousarray(a)
    if a.dtype.kind not in "iu":
        raise ValueError("query terms are texts or an integer array of term ids")
    if a.ndim == 1:
        a = a[None, :]
    if a.ndim != 2 or a.shape[1] > T_MAX:
        raise ValueError(f"query terms are [M, T] with T <= {T_MAX} (got {a.shape})")
    a = a.astype(np.int64)
    if ((a < 0) | (a > 0xFFFFFF)).any():
        raise ValueError("term ids are 24 bits")
    out = np.zeros((a.shape[0], T_MAX), dtype=np.uint32)
    for m in range(a.shape[0]):
        u = np.unique(a[m][a[m] > 0])
        out[m, : len(u)] = u
    return out


@dataclass(frozen=True)
class LexicalSearch:
    """Settings of ``lexical=``: a result scores ``(1 - alpha) * cos(q, v) +
    alpha * lexn(q, v)`` over the union of the ``pool`` nearest rows and the
    ``pool`` best rows by BM25 (``k1``, ``b``); ops/lex_ops.py holds the
    contract in full."""
    alpha: float
    pool: int = DEFAULT_POOL
    k1: float = 1.2
    b: float = 0.75

    def __post_init__(self):
        for name in ("alpha", "k1", "b"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float, np.floating, np.integer)):
                raise ValueError(f"{name} must be a number (got {v!r})")
            object.__setattr__(self, name, float(v))
        p = self.pool
        if isinstance(p, bool) or not isinstance(p, (int, np.integer)):
            if isinstance(p, float) and p.is_integer():
                p = int(p)
            else:
                raise ValueError(f"pool must be an integer (got {p!r})")
        object.__setattr__(self, "pool", int(p))
        if not 0.0 <= self.alpha <= 1.0:
            raise ValueError(f"alpha must be in [0, 1] (got {self.alpha})")
        if not 1 <= self.pool <= MAX_POOL:
            raise ValueError(f"pool must be in 1 .. {MAX_POOL} (got {self.pool})")
        if not (self.k1 >= 0.0 and math.isfinite(self.k1)):
            raise ValueError(f"k1 must be >= 0 and finite (got {self.k1})")
        if not 0.0 <= self.b <= 1.0:
            raise ValueError(f"b must be in [0, 1] (got {self.b})")

    def check_limit(self, limit: int) -> "LexicalSearch":
        if not 1 <= int(limit) <= self.pool:
            raise ValueError(f"limit must be in 1 .. pool={self.pool} (got {limit})")
        return self

    def to_dict(self) -> Dict[str, Any]:
        return {f.name: getattr(self, f.name) for f in fields(self)}

    @classmethod
    def coerce(cls, lexical: Union[None, float, "LexicalSearch", Dict[str, Any]]) -> Optional["LexicalSearch"]:
        """``lexical`` as given to a search: settings, a dict of their fields,
        a number (``alpha``) or None."""
        if lexical is None or isinstance(lexical, cls):
            return lexical
        if isinstance(lexical, bool):
            raise ValueError("lexical must be a LexicalSearch, a dict, a number in [0, 1] or None, not bool")
        if isinstance(lexical, (int, float, np.floating, np.integer)):
            return cls(alpha=float(lexical))
        if isinstance(lexical, dict):
            unknown = set(lexical) - {f.name for f in fields(cls)}
            if unknown:
                raise ValueError(f"unknown lexical field(s): {sorted(unknown)}")
            if "alpha" not in lexical:
                raise ValueError("lexical needs alpha")
            return cls(**lexical)
        raise ValueError(f"lexical must be a LexicalSearch, a dict, a number in [0, 1] or None, "
                         f"not {type(lexical).__name__}")
