"""Settings of an associative (graph-expanded) search, ``expand=``.

The nearest ``seed_k`` memories are the seeds; ``hops`` times, every candidate
found so far follows the first ``fanout`` links of weight ``>= min_weight``
that lead to a searchable memory, handing on its activation damped by
``decay`` and the link's weight; every candidate is then scored
``(1 - graph_weight) * cos(q, v) + graph_weight * activation(v)``
(ops/expand_ops.py holds the contract in full).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, fields
from typing import Any, Dict, Optional, Union

MAX_HOPS = 3
MAX_FANOUT = 16
MAX_SEED_K = 16   # CAND_SLOTS: the seed search stays on the fast candidate routes
MAX_POOL = 1024   # expand.hip EXP_MAX_POOL: the candidate table of one query
MAX_LIMIT = 64


@dataclass(frozen=True)
class GraphExpand:
    hops: int = 1
    fanout: int = 8
    seed_k: int = 16
    min_weight: float = 0.3   # the reference's neighbour cut (neighbor_boost)
    decay: float = 0.85
    graph_weight: float = 0.5

    def __post_init__(self):
        for name in ("hops", "fanout", "seed_k"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, int):
                if isinstance(v, float) and v.is_integer():
                    v = int(v)
                else:
                    raise ValueError(f"{name} must be an integer (got {v!r})")
            object.__setattr__(self, name, int(v))
        for name in ("min_weight", "decay", "graph_weight"):
            object.__setattr__(self, name, float(getattr(self, name)))
        if not 1 <= self.hops <= MAX_HOPS:
            raise ValueError(f"hops must be in 1 .. {MAX_HOPS} (got {self.hops})")
        if not 1 <= self.fanout <= MAX_FANOUT:
            raise ValueError(f"fanout must be in 1 .. {MAX_FANOUT} (got {self.fanout})")
        if not 1 <= self.seed_k <= MAX_SEED_K:
            raise ValueError(f"seed_k must be in 1 .. {MAX_SEED_K} (got {self.seed_k})")
        if not (self.min_weight >= 0.0 and math.isfinite(self.min_weight)):
            raise ValueError(f"min_weight must be >= 0 (got {self.min_weight})")
        if not 0.0 < self.decay <= 1.0:
            raise ValueError(f"decay must be in (0, 1] (got {self.decay})")
        if not 0.0 <= self.graph_weight <= 1.0:
            raise ValueError(f"graph_weight must be in [0, 1] (got {self.graph_weight})")
        if self.pool > MAX_POOL:
            raise ValueError(f"seed_k * (1 + fanout) ** hops = {self.pool} exceeds the candidate table of {MAX_POOL}: "
                             "lower hops, fanout or seed_k")

    @property
    def pool(self) -> int:
        """Upper bound of the candidate count of one query."""
        return self.seed_k * (1 + self.fanout) ** self.hops

    def to_dict(self) -> Dict[str, Any]:
        return {f.name: getattr(self, f.name) for f in fields(self)}

    @classmethod
    def coerce(cls, expand: Union[None, int, "GraphExpand", Dict[str, Any]]) -> Optional["GraphExpand"]:
        """``expand`` as given to a search: settings, a dict of their fields,
        an int (the hop count) or None."""
        if expand is None or isinstance(expand, cls):
            return expand
        if isinstance(expand, bool):
            raise TypeError("expand must be a GraphExpand, a dict, an int or None, not bool")
        if isinstance(expand, int):
            return cls(hops=expand)
        if isinstance(expand, dict):
            unknown = set(expand) - {f.name for f in fields(cls)}
            if unknown:
                raise ValueError(f"unknown expand field(s): {sorted(unknown)}")
            return cls(**expand)
        raise TypeError(f"expand must be a GraphExpand, a dict, an int or None, not {type(expand).__name__}")
