"""Settings of a multi-query search, ``fuse=``.

A group of 1 .. 16 sub-queries (the user's sentence, a rewritten question, a
hypothetical answer ...) returns ONE ranked list. Every sub-query is searched
with the inner options at ``limit = pool``; the union of the group's pools is
scored by ``mode`` and the ``limit`` best come back:

* ``"rrf"``: reciprocal rank fusion, ``sum_j w_j / (rrf_k + rank_j(v))`` over
  the pools that hold ``v`` (rank-only: no rows, no metric);
* ``"mean"``: the weighted mean cosine ``sum_j wn_j cos(q_j, v)`` over ALL
  sub-queries, whether or not ``v`` was in that pool.

``weights``: one per position in the group (default 1 each, ``>= 0``, finite);
ops/fuse_ops.py holds the contract in full.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, fields
from typing import Any, Dict, Optional, Sequence, Tuple, Union

MODES = ("rrf", "mean")
MAX_FUSE_Q = 16   # fuse.hip FUSE_MAX_Q: sub-queries per group
MAX_POOL = 64     # fuse.hip FUSE_MAX_P: a pool is one search of at most 64 results
MAX_LIMIT = 64


def check_weights(weights, what: str = "weights") -> Tuple[float, ...]:
    """``weights`` as a tuple of finite floats ``>= 0``."""
    if isinstance(weights, (str, bytes)) or not hasattr(weights, "__iter__"):
        raise ValueError(f"{what} must be a sequence of numbers (got {weights!r})")
    out = []
    for w in weights:
        if isinstance(w, bool) or not isinstance(w, (int, float)):
            raise ValueError(f"{what} must be numbers (got {w!r})")
        w = float(w)
        if not (w >= 0.0 and math.isfinite(w)):
            raise ValueError(f"{what} must be finite and >= 0 (got {w})")
        out.append(w)
    return tuple(out)


@dataclass(frozen=True)
class QueryFusion:
    mode: str = "rrf"
    pool: int = 16
    rrf_k: float = 60.0
    weights: Optional[Tuple[float, ...]] = None

    def __post_init__(self):
        if self.mode not in MODES:
            raise ValueError(f"mode must be one of {MODES} (got {self.mode!r})")
        v = self.pool
        if isinstance(v, bool) or not isinstance(v, int):
            if isinstance(v, float) and v.is_integer():
                v = int(v)
            else:
                raise ValueError(f"pool must be an integer (got {v!r})")
        object.__setattr__(self, "pool", int(v))
        if not 1 <= self.pool <= MAX_POOL:
            raise ValueError(f"pool must be in 1 .. {MAX_POOL} (got {self.pool})")
        k = self.rrf_k
        if isinstance(k, bool) or not isinstance(k, (int, float)):
            raise ValueError(f"rrf_k must be a number (got {k!r})")
        object.__setattr__(self, "rrf_k", float(k))
        if not (self.rrf_k > 0.0 and math.isfinite(self.rrf_k)):
            raise ValueError(f"rrf_k must be finite and > 0 (got {self.rrf_k})")
        if self.weights is not None:
            object.__setattr__(self, "weights", check_weights(self.weights))

    def to_dict(self) -> Dict[str, Any]:
        return {f.name: getattr(self, f.name) for f in fields(self)}

    @classmethod
    def coerce(cls, fuse: Union[None, str, "QueryFusion", Dict[str, Any]]) -> Optional["QueryFusion"]:
        """``fuse`` as given to a search: settings, a dict of their fields,
        ``"rrf"`` / ``"mean"`` or None."""
        if fuse is None or isinstance(fuse, cls):
            return fuse
        if isinstance(fuse, str):
            return cls(mode=fuse)
        if isinstance(fuse, dict):
            unknown = set(fuse) - {f.name for f in fields(cls)}
            if unknown:
                raise ValueError(f"unknown fuse field(s): {sorted(unknown)}")
            return cls(**fuse)
        raise ValueError(f"fuse must be a QueryFusion, a dict, 'rrf' or 'mean', not {type(fuse).__name__}")

    def check(self, limit, group_sizes: Sequence[int]) -> None:
        """Raises ValueError, before any work, for a ``limit`` outside 1 ..
        64, an empty group, a group above 16 sub-queries, or ``weights`` whose
        length is not every group's."""
        if isinstance(limit, bool) or not isinstance(limit, int) or not 1 <= limit <= MAX_LIMIT:
            raise ValueError(f"a fused search returns 1 .. {MAX_LIMIT} results (limit={limit!r})")
        for i, n in enumerate(group_sizes):
            if n < 1:
                raise ValueError(f"group {i} is empty: a group holds 1 .. {MAX_FUSE_Q} sub-queries")
            if n > MAX_FUSE_Q:
                raise ValueError(f"group {i} holds {n} sub-queries: at most {MAX_FUSE_Q}")
            if self.weights is not None and len(self.weights) != n:
                raise ValueError(f"{len(self.weights)} weights for group {i} of {n} sub-queries: weights= of a "
                                 "QueryFusion apply per position and need equal group sizes")

    def group_weights(self, group_sizes: Sequence[int], weights=None):
        """The weight of every sub-query of the call, flat, as a list of
        floats: ``weights`` (one sequence per group) when given, else this
        record's per-position weights, else 1. Raises ValueError for lengths
        that do not fit, and -- ``mode="mean"`` -- a group whose weights sum
        to 0."""
        if weights is not None:
            weights = list(weights)
            if len(weights) != len(group_sizes):
                raise ValueError(f"weights= for {len(weights)} groups, but {len(group_sizes)} groups")
            per = [check_weights(w, f"weights[{i}]") for i, w in enumerate(weights)]
            for i, (w, n) in enumerate(zip(per, group_sizes)):
                if len(w) != n:
                    raise ValueError(f"{len(w)} weights for group {i} of {n} sub-queries")
        elif self.weights is not None:
            per = [self.weights] * len(group_sizes)
        else:
            per = [(1.0,) * n for n in group_sizes]
        if self.mode == "mean":
            for i, w in enumerate(per):
                if not math.fsum(w) > 0.0:
                    raise ValueError(f"the weights of group {i} sum to 0: a mean needs a positive weight")
        return [x for w in per for x in w]
