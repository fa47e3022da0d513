"""The options of a memory search as one record: ``where=``, ``diversity=`` /
``fetch_k=``, ``expand=``, ``boost=``, ``lexical=`` and ``rerank=`` are coerced and checked
against each other and the ``limit`` once, in :meth:`SearchSpec.of`; every
layer below the public signatures takes the spec. The queries' texts / terms
of a lexical search, and the texts / tokens of a re-ranked one, are per call
and travel beside it."""
from __future__ import annotations

from dataclasses import dataclass, fields
from typing import Any, Dict, Optional

from .boost import MemoryBoost
from .crossenc import CrossRerank
from .expand import GraphExpand
from .filters import MemoryFilter
from .lexical import LexicalSearch


def _first_set(options: Dict[str, Any]) -> Optional[str]:
    return next((name for name, v in options.items() if v is not None), None)


@dataclass(frozen=True)
class SearchSpec:
    where: Optional[MemoryFilter] = None
    diversity: Optional[float] = None
    fetch_k: Optional[int] = None
    expand: Optional[GraphExpand] = None
    boost: Optional[MemoryBoost] = None  # (``now`` is set)
    lexical: Optional[LexicalSearch] = None
    rerank: Optional[CrossRerank] = None

    @classmethod
    def of(cls, limit, where=None, diversity=None, fetch_k=None, expand=None, boost=None,
           lexical=None, rerank=None) -> Optional["SearchSpec"]:
        """The options as given to a search (each in any form its ``coerce``
        takes), validated before any work; None: the plain search. A boost's
        ``now`` is fixed here, once per call. Idempotent: the fields of a
        spec give an equal spec, and read the clock no second time."""
        if where is None and diversity is None and fetch_k is None and expand is None and boost is None \
                and lexical is None and (rerank is None or rerank is False):
            return None
        rerank = CrossRerank.coerce(rerank)
        if rerank is not None:
            if diversity is not None or fetch_k is not None:
                raise NotImplementedError("rerank= does not compose with diversity=: two final selectors")
            rerank.check_limit(limit)
            limit = rerank.pool  # the search of the other options runs at limit = pool
        where = MemoryFilter.coerce(where)
        lexical = LexicalSearch.coerce(lexical)
        if lexical is not None and (expand is not None or boost is not None):
            raise NotImplementedError("lexical= does not compose with expand= or boost=")
        pool = None
        if diversity is not None or fetch_k is not None:
            from ..ops.mmr_ops import pool_size
            pool = pool_size(limit, diversity, fetch_k)
            diversity = float(diversity)
        if lexical is not None:
            lexical.check_limit(pool or limit)  # (the fused search is the pool search of a diverse one)
        if boost is not None:
            boost = MemoryBoost.coerce(boost).at()
        if expand is not None:
            from ..ops.expand_ops import pool_bound
            expand = GraphExpand.coerce(expand)
            pool_bound(expand, limit if diversity is None else None)  # (with diversity= the expansion returns the pool)
        return cls(where, diversity, fetch_k, expand, boost, lexical, rerank)

    @property
    def needs_text(self) -> bool:
        """Whether the search reads the queries' texts (lexical, rerank)."""
        return self.lexical is not None or self.rerank is not None

    def kwargs(self, **texts) -> Dict[str, Any]:
        """The options that are set, as the keyword arguments of a public
        search; ``texts`` (``query_text=`` / ``query_texts=``) join them for a
        lexical or a re-ranked search."""
        kw = {f.name: v for f, v in ((f, getattr(self, f.name)) for f in fields(self)) if v is not None}
        return dict(kw, **texts) if self.needs_text else kw

    def as_dict(self) -> Dict[str, Any]:
        """The options that are set in a JSON-able normal form (what a served
        request carries between ranks): every settings record as the dict of
        its fields, sets as sorted lists. ``SearchSpec.of(limit,
        **json.loads(json.dumps(spec.as_dict())))`` is an equal spec."""
        return {name: (v.to_dict() if hasattr(v, "to_dict") else v) for name, v in self.kwargs().items()}

    @property
    def bias_only(self) -> bool:
        """Only ``where`` and / or ``boost`` are set: the search is the plain
        scan under another bias column (ops/mt_bias_ops.py)."""
        return (self.diversity is None and self.fetch_k is None and self.expand is None and self.lexical is None
                and self.rerank is None)

    def only(self, *names: str) -> Optional["SearchSpec"]:
        """The spec of an inner search that keeps the options ``names``."""
        kept = {name: getattr(self, name) for name in names}
        return None if _first_set(kept) is None else SearchSpec(**kept)

    def needs(self, what: str):
        """Raises: the search cannot run without ``what`` (the tenant's graph)."""
        raise NotImplementedError(f"a search with {_first_set(self.kwargs())}= needs {what}")

    @staticmethod
    def refuse(surface: str, **options) -> None:
        """Raises if any of ``options`` is set: ``surface`` takes none of them."""
        name = _first_set(options)
        if name is not None:
            raise NotImplementedError(f"{surface} does not take {name}=; search each tenant with it "
                                      "(MemorySystem.search_memories)")
