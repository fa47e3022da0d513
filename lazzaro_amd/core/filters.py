"""``MemoryFilter``: the ``where`` clause of a memory search.

A filter restricts ``search_memories`` (and the store / graph searches under
it) to the nodes whose metadata passes every given test; the tests are
evaluated on the device over the tenant's HBM columns
(``TenantGraph.store_search(..., where=)``, csrc/kernels/filter.hip). All
fields are optional; an empty filter still restricts the search to memories
(graph nodes that are in the store), so ghost rows take no result slot.
"""
from __future__ import annotations

from dataclasses import dataclass, fields
from typing import Any, Collection, Dict, Optional, Tuple, Union

MAX_EXCLUDE_IDS = 4096

_SETS = ("types", "shard_keys", "exclude_ids")
_FLOATS = ("min_salience", "max_salience", "since", "until", "accessed_since")


@dataclass(frozen=True)
class MemoryFilter:
    """A row passes iff

    * ``types``: its ``Node.type`` is in the set;
    * ``shard_keys``: its ``Node.shard_key`` is in the set (a name the tenant
      has never seen matches nothing);
    * ``min_salience`` / ``max_salience``: ``min <= salience <= max`` (fp32);
    * ``since`` / ``until``: ``since <= timestamp < until`` (float64);
    * ``accessed_since``: ``last_accessed >= accessed_since``;
    * ``min_access_count``: ``access_count >= min_access_count``;
    * ``super_nodes``: ``None`` both, ``True`` only super-nodes, ``False`` none;
    * ``exclude_ids``: its id is not in the set (unknown ids are ignored; at
      most ``MAX_EXCLUDE_IDS``).
    """
    types: Optional[Collection[str]] = None
    shard_keys: Optional[Collection[str]] = None
    min_salience: Optional[float] = None
    max_salience: Optional[float] = None
    since: Optional[float] = None
    until: Optional[float] = None
    accessed_since: Optional[float] = None
    min_access_count: Optional[int] = None
    super_nodes: Optional[bool] = None
    exclude_ids: Optional[Collection[str]] = None

    def __post_init__(self):
        for name in _SETS:
            v = getattr(self, name)
            if v is not None:
                if isinstance(v, str):
                    v = (v,)
                object.__setattr__(self, name, frozenset(str(x) for x in v))
        for name in _FLOATS:
            v = getattr(self, name)
            if v is not None:
                object.__setattr__(self, name, float(v))
        if self.min_access_count is not None:
            object.__setattr__(self, "min_access_count", int(self.min_access_count))
        if self.super_nodes is not None:
            object.__setattr__(self, "super_nodes", bool(self.super_nodes))
        if self.exclude_ids is not None and len(self.exclude_ids) > MAX_EXCLUDE_IDS:
            raise ValueError(f"exclude_ids holds {len(self.exclude_ids)} ids; at most {MAX_EXCLUDE_IDS}")

    def key(self) -> Tuple:
        """Hashable identity of the filter (equal filters, equal keys)."""
        return tuple(tuple(sorted(v)) if isinstance(v, frozenset) else v
                     for v in (getattr(self, f.name) for f in fields(self)))

    def to_dict(self) -> Dict[str, Any]:
        """The fields that are set, sets as sorted lists (JSON-ready)."""
        out = {}
        for f in fields(self):
            v = getattr(self, f.name)
            if v is not None:
                out[f.name] = sorted(v) if isinstance(v, frozenset) else v
        return out

    @classmethod
    def from_dict(cls, d: Dict[str, Any]) -> "MemoryFilter":
        known = {f.name for f in fields(cls)}
        bad = sorted(set(d) - known)
        if bad:
            raise ValueError(f"unknown filter field(s): {', '.join(bad)}")
        return cls(**d)

    @classmethod
    def coerce(cls, where: Union[None, "MemoryFilter", Dict[str, Any]]) -> Optional["MemoryFilter"]:
        """``where`` as given to a search: a filter, a dict of its fields, or None."""
        if where is None or isinstance(where, cls):
            return where
        if isinstance(where, dict):
            return cls.from_dict(where)
        raise TypeError(f"where must be a MemoryFilter, a dict or None, not {type(where).__name__}")
