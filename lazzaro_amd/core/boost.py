"""Settings of a boosted search, ``boost=``.

A boosted search ranks by ``metric score + prior``: every memory's salience,
use and recency (and a weight per node type) add to its score BEFORE the
``limit`` best are chosen, so a memory that wins under the combined score is
found wherever its distance alone would have ranked it
(ops/boost_ops.py holds the contract in full).
"""
from __future__ import annotations

import math
import time
from dataclasses import dataclass, fields, replace
from typing import Any, Dict, Optional, Tuple, Union

MAX_BOOST = 4.0  # salience + frequency + recency + max(type_weights): the prior stays of the order of a cosine
CLOCKS = ("accessed", "created")
# the reference's eviction importance (0.5 sal + 0.3 min(1, acc / 10) + 0.2 / (1 + days)): the bare-float form
IMPORTANCE = {"salience": 0.5, "frequency": 0.3, "recency": 0.2}
_clock = time.time  # what ``now=None`` reads


@dataclass(frozen=True)
class MemoryBoost:
    """``salience``, ``frequency``, ``recency`` (each ``>= 0``): the weights of
    ``salience[r]``, ``min(1, access_count[r] / 10)`` and
    ``1 / (1 + max(0, now - t[r]) / recency_scale)``; ``clock``: ``t`` is
    ``last_accessed`` (``"accessed"``) or ``timestamp`` (``"created"``);
    ``type_weights``: node type -> weight added for rows of that type (a type
    the tenant never saw adds nothing); ``now``: None = ``time.time()``, read
    once per search call."""
    salience: float = 0.0
    frequency: float = 0.0
    recency: float = 0.0
    recency_scale: float = 86400.0
    clock: str = "accessed"
    type_weights: Optional[Dict[str, float]] = None
    now: Optional[float] = None

    def __post_init__(self):
        for name in ("salience", "frequency", "recency"):
            v = self._num(name, getattr(self, name))
            if not (v >= 0.0 and math.isfinite(v)):
                raise ValueError(f"{name} must be a finite weight >= 0 (got {v!r})")
            object.__setattr__(self, name, v)
        sc = self._num("recency_scale", self.recency_scale)
        if not (sc > 0.0 and math.isfinite(sc)):
            raise ValueError(f"recency_scale must be finite and > 0 seconds (got {sc!r})")
        object.__setattr__(self, "recency_scale", sc)
        if self.clock not in CLOCKS:
            raise ValueError(f"clock must be one of {CLOCKS} (got {self.clock!r})")
        tw = self.type_weights
        top = 0.0
        if tw is not None:
            if not isinstance(tw, dict):
                raise ValueError(f"type_weights must be a dict of type name -> weight (got {type(tw).__name__})")
            clean = {}
            for t, w in tw.items():
                w = self._num(f"type_weights[{t!r}]", w)
                if not (w >= 0.0 and math.isfinite(w)):
                    raise ValueError(f"type_weights[{t!r}] must be a finite weight >= 0 (got {w!r})")
                clean[str(t)] = w
            top = max(clean.values(), default=0.0)
            object.__setattr__(self, "type_weights", clean)
        if self.now is not None:
            now = self._num("now", self.now)
            if not math.isfinite(now):
                raise ValueError(f"now must be finite (got {now!r})")
            object.__setattr__(self, "now", now)
        total = self.salience + self.frequency + self.recency + top
        if total > MAX_BOOST:
            raise ValueError(f"salience + frequency + recency + max(type_weights) = {total} exceeds {MAX_BOOST}")

    @staticmethod
    def _num(name: str, v) -> float:
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            raise ValueError(f"{name} must be a number (got {v!r})")
        return float(v)

    @property
    def is_zero(self) -> bool:
        """No weight set: the prior is 0 for every memory."""
        return not (self.salience or self.frequency or self.recency or any((self.type_weights or {}).values()))

    def at(self, now: Optional[float] = None) -> "MemoryBoost":
        """These settings with ``now`` fixed: its own ``now`` if set, else the
        given one, else ``time.time()``."""
        if self.now is not None:
            return self
        return replace(self, now=float(_clock() if now is None else now))

    def key(self) -> Tuple:
        """Hashable identity of the settings (equal settings, equal keys)."""
        return tuple(tuple(sorted(v.items())) if isinstance(v, dict) else v
                     for v in (getattr(self, f.name) for f in fields(self)))

    def __hash__(self):
        return hash(self.key())

    def to_dict(self) -> Dict[str, Any]:
        return {f.name: (dict(v) if isinstance(v, dict) else v)
                for f, v in ((f, getattr(self, f.name)) for f in fields(self))}

    @classmethod
    def coerce(cls, boost: Union[None, float, "MemoryBoost", Dict[str, Any]]) -> Optional["MemoryBoost"]:
        """``boost`` as given to a search: settings, a dict of their fields, a
        number ``w`` (``w`` times the reference's importance: salience 0.5 w,
        frequency 0.3 w, recency 0.2 w over days since the last access) or
        None."""
        if boost is None or isinstance(boost, cls):
            return boost
        if isinstance(boost, bool):
            raise TypeError("boost must be a MemoryBoost, a dict, a number or None, not bool")
        if isinstance(boost, (int, float)):
            w = float(boost)
            if not (w >= 0.0 and math.isfinite(w)):
                raise ValueError(f"boost must be a finite weight >= 0 (got {w!r})")
            return cls(**{name: share * w for name, share in IMPORTANCE.items()})
        if isinstance(boost, dict):
            unknown = set(boost) - {f.name for f in fields(cls)}
            if unknown:
                raise ValueError(f"unknown boost field(s): {sorted(unknown)}")
            return cls(**boost)
        raise TypeError(f"boost must be a MemoryBoost, a dict, a number or None, not {type(boost).__name__}")
