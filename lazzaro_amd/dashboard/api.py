"""Web dashboard (reference ``src/lazzaro/dashboard/api.py:12-139``).

Same FastAPI routes and JSON shapes: ``GET /``, ``/api/stats``, ``/api/users``,
``POST /api/users/switch``, ``/api/insights``, ``/api/export``, ``/api/graph``,
``/api/profile``, ``POST /api/consolidate``; served on port 5299. The page is
self-contained (no CDN scripts, renders offline) and polls every 30 s.
Extra: ``GET /api/search?q=&limit=`` (on-device vector search) and
``GET /api/engine`` (device / kernel-library status).
"""
from __future__ import annotations

import os
from typing import List, Optional

from fastapi import FastAPI, Query, Request
from fastapi.responses import HTMLResponse

app = FastAPI(title="Lazzaro MI355X Memory Dashboard")
_ms = None
_HERE = os.path.dirname(os.path.abspath(__file__))


def set_memory_system(ms) -> None:
    global _ms
    _ms = ms


@app.get("/", response_class=HTMLResponse)
async def get_dashboard(request: Request):
    with open(os.path.join(_HERE, "templates", "index.html"), encoding="utf-8") as f:
        return HTMLResponse(f.read())


@app.get("/api/stats")
async def get_stats():
    if not _ms:
        return {"error": "Memory system not initialized"}
    _ms.check_for_updates()
    s = _ms.get_stats()
    s["user_id"] = _ms.user_id
    return s


@app.get("/api/users")
async def get_users():
    return _ms.get_all_users() if _ms else []


@app.post("/api/users/switch")
async def switch_user(request: Request):
    if not _ms:
        return {"error": "Memory system not initialized"}
    data = await request.json()
    uid = data.get("user_id")
    if not uid:
        return {"error": "User ID required"}
    _ms.switch_user(uid)
    return {"status": "success", "user_id": _ms.user_id}


@app.get("/api/insights")
async def get_insights():
    if not _ms:
        return {"error": "Memory system not initialized"}
    return {"insights": _ms.get_insights()}


@app.get("/api/export")
async def export_observations(format: str = "markdown"):
    if not _ms:
        return {"error": "Memory system not initialized"}
    return {"content": _ms.export_observations(format=format)}


@app.get("/api/graph")
async def get_graph():
    if not _ms:
        return {"nodes": [], "links": []}
    _ms.check_for_updates()
    return _ms.graph_json()


@app.get("/api/profile")
async def get_profile():
    if not _ms:
        return {}
    _ms.check_for_updates()
    with _ms._graph_lock:
        return _ms.profile.to_dict()


@app.post("/api/consolidate")
async def consolidate():
    if not _ms:
        return {"error": "Memory system not initialized"}
    return {"status": _ms.run_consolidation()}


def _csv(v: Optional[str]):
    return [x for x in v.split(",") if x] if v is not None else None


@app.get("/api/search")
async def search(q: str, limit: int = 5, types: Optional[str] = None, shard_keys: Optional[str] = None,
                 min_salience: Optional[float] = None, max_salience: Optional[float] = None,
                 since: Optional[float] = None, until: Optional[float] = None,
                 accessed_since: Optional[float] = None, min_access_count: Optional[int] = None,
                 super_nodes: Optional[bool] = None, exclude_ids: Optional[str] = None,
                 diversity: Optional[float] = None, fetch_k: Optional[int] = None,
                 hops: Optional[int] = None, fanout: Optional[int] = None, graph_weight: Optional[float] = None,
                 boost: Optional[float] = None, boost_recency_scale: Optional[float] = None,
                 lexical: Optional[float] = None, lexical_pool: Optional[int] = None,
                 rerank: Optional[bool] = None, rerank_pool: Optional[int] = None,
                 also: Optional[List[str]] = Query(None), fuse: Optional[str] = None):
    """``MemoryFilter`` fields as optional query parameters (the set-valued
    ones comma separated); none given: the unfiltered search. ``diversity``
    (0 .. 1) and ``fetch_k``: results picked for diversity from the
    ``fetch_k`` nearest (``MemorySystem.search_memories``). ``hops``,
    ``fanout``, ``graph_weight``: any of them given makes it an associative
    search along the memories' links (``expand=``, core/expand.py; the others
    keep their defaults). ``boost`` (a weight ``w``): the results are ranked
    by closeness plus ``w`` times each memory's importance -- salience 0.5 w,
    use 0.3 w, recency 0.2 w (``boost=``, core/boost.py);
    ``boost_recency_scale``: the recency term's scale in seconds (default one
    day; given alone it changes nothing). ``lexical`` (``alpha`` in 0 .. 1):
    keyword and hybrid search over the memories' words (``lexical=``,
    core/lexical.py); ``lexical_pool``: its candidate pool (default 16; given
    alone it changes nothing). ``rerank`` (true): the pool of the other
    options is re-scored by the store's cross-encoder (``rerank=``,
    core/crossenc.py); ``rerank_pool``: its pool (default 16; given alone it
    changes nothing). ``also`` (repeatable): further sub-queries --
    ``q`` and every ``also`` form one group whose pools are fused into one
    list (``MemorySystem.search_memories_fused``, core/fuse.py) by ``fuse``
    (``rrf``, the default, or ``mean``); without ``also`` nothing changes.
    ``diversity`` / ``fetch_k`` / ``rerank`` do not apply to a fused search."""
    if not _ms:
        return []
    where = {k: v for k, v in (("types", _csv(types)), ("shard_keys", _csv(shard_keys)),
                               ("min_salience", min_salience), ("max_salience", max_salience), ("since", since),
                               ("until", until), ("accessed_since", accessed_since),
                               ("min_access_count", min_access_count), ("super_nodes", super_nodes),
                               ("exclude_ids", _csv(exclude_ids))) if v is not None}
    expand = {k: v for k, v in (("hops", hops), ("fanout", fanout), ("graph_weight", graph_weight)) if v is not None}
    if boost is not None:
        from ..core.boost import MemoryBoost
        boost = MemoryBoost.coerce(float(boost)).to_dict()
        if boost_recency_scale is not None:
            boost["recency_scale"] = boost_recency_scale
    if lexical is not None:
        lexical = {"alpha": lexical}
        if lexical_pool is not None:
            lexical["pool"] = lexical_pool
    rr = ({"pool": rerank_pool} if rerank_pool is not None else True) if rerank else None
    if also:
        if diversity is not None or fetch_k is not None:
            raise ValueError("diversity= / fetch_k= do not apply to a fused search (also=)")
        if rr is not None:
            raise ValueError("rerank= does not apply to a fused search (also=)")
        hits = _ms.search_memories_fused([q] + list(also), limit=limit, fuse=fuse or "rrf", where=where or None,
                                         expand=expand or None, boost=boost, lexical=lexical)
        return [{"id": n.id, "content": n.content, "salience": n.salience, "shard": n.shard_key} for n in hits]
    # (an option that is None is an option not given)
    hits = _ms.search_memories(q, limit=limit, where=where or None, diversity=diversity, fetch_k=fetch_k,
                               expand=expand or None, boost=boost, lexical=lexical, rerank=rr)
    return [{"id": n.id, "content": n.content, "salience": n.salience, "shard": n.shard_key} for n in hits]


@app.get("/api/engine")
async def engine():
    import torch

    from ..ops import _lib

    dev = str(getattr(_ms, "_device", None)) if _ms else None
    return {"device": dev, "hip_available": torch.cuda.is_available(), "kernel_library": _lib.available(),
            "store": type(_ms.store).__name__ if _ms else None}


def entry_point(host: str = "0.0.0.0", port: int = 5299, ms: Optional[object] = None) -> None:
    import uvicorn

    if ms is None:
        from ..core.memory_system import MemorySystem

        ms = MemorySystem(load_from_disk=True)
    set_memory_system(ms)
    print(f"🚀 Starting Lazzaro MI355X Dashboard on http://localhost:{port}")
    uvicorn.run(app, host=host, port=port)


if __name__ == "__main__":
    entry_point()
