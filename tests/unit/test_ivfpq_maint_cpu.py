"""IVF-PQ maintenance in place (``IVFPQIndex.remove / upsert / translate_ids``)
and what the tenant graph and the arena do with it: evicted rows leave the
lists, rewrites and compactions keep the index. CPU tier: the torch
formulation (``_finalize_ref``), compared against filters written out here."""
import pytest
import torch

import lazzaro_amd.core  # noqa: F401  (before engine.views: the package's import order)
from lazzaro_amd.index.ivfpq import IVFPQIndex

from .test_compact_rows import reclaimable

F = torch.nn.functional


def _data(n, d, seed, clusters=8, noise=0.3):
    g = torch.Generator().manual_seed(seed)
    c = F.normalize(torch.randn(clusters, d, generator=g), dim=1)
    lab = torch.randint(0, clusters, (n,), generator=g)
    return F.normalize(c[lab] + noise * torch.randn(n, d, generator=g), dim=1)


def _built(keep, n=2000, d=32, seed=0):
    x = _data(n, d, seed)
    idx = IVFPQIndex(d, nlist=8, m=8, device="cpu", keep_vectors=keep)
    idx.train(x, iters=4, pq_iters=4)
    idx.add(x, ids=torch.arange(n) + 100)
    idx._finalize()
    return idx, x


def _arrays(idx):
    out = {"codes": idx.codes.clone(), "list_of": idx.list_of.clone(), "pos": idx._pos[: idx.n].clone(),
           "vids": idx._vids[: idx.nv].clone(), "list_off": idx.list_off.clone()}
    if idx.vectors is not None:
        out["vectors"] = idx.vectors.clone()
    if idx.vscale is not None:
        out["vscale"] = idx.vscale.clone()
    return out


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), k


def _from_arrays(src, arr):
    """An index with ``src``'s quantisers holding exactly ``arr``, through the setters."""
    o = IVFPQIndex(src.dim, nlist=src.nlist, m=src.m, device="cpu", keep_vectors=src.keep_vectors)
    o.centroids, o.codebooks = src.centroids, src.codebooks
    o.codes, o.list_of, o.list_off = arr["codes"].clone(), arr["list_of"].clone(), arr["list_off"].clone()
    o.ids = arr["vids"].clone()
    o._pos = arr["pos"].clone()
    if "vectors" in arr:
        o._vec = arr["vectors"].clone()
    if "vscale" in arr:
        o._vscale = arr["vscale"].clone()
    return o


def _filtered(arr, gone_ids, nlist):
    """The arrays with the vectors of ``gone_ids`` filtered out, written out by hand."""
    vkeep = ~torch.isin(arr["vids"], gone_ids)
    vremap = torch.cumsum(vkeep, 0) - 1
    ckeep = vkeep[arr["pos"]]
    out = {"codes": arr["codes"][ckeep], "list_of": arr["list_of"][ckeep], "pos": vremap[arr["pos"][ckeep]],
           "vids": arr["vids"][vkeep]}
    off = torch.zeros(nlist + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(torch.bincount(out["list_of"].long(), minlength=nlist), 0)
    out["list_off"] = off
    for k in ("vectors", "vscale"):
        if k in arr:
            out[k] = arr[k][vkeep]
    return out


# ---------------------------------------------------------------- the index
@pytest.mark.parametrize("keep", [False, "int8"])
def test_remove(keep):
    idx, x = _built(keep)
    n = 2000
    before = _arrays(idx)
    g = torch.Generator().manual_seed(1)
    whole = int(torch.bincount(idx.list_of.long(), minlength=8).argmax())  # every id of one whole list
    in_list = idx.ids[idx.list_of == whole]
    rnd = torch.randperm(n, generator=g)[:300] + 100
    gone = torch.unique(torch.cat([rnd, in_list]))
    cent = idx.centroids
    asked = torch.cat([rnd, in_list, torch.tensor([5, 99, 10_000]), rnd[:7]])  # + never added + a repeat
    assert idx.remove(asked) == gone.numel()
    assert idx.remove(rnd[:50]) == 0  # already removed
    live = n - gone.numel()
    assert len(idx) == live
    per = 8 + 4 + 8 + 8 + ((32 + 4) if keep else 0)
    assert idx.memory_bytes() == live * per
    q = torch.cat([x[:20], x[(in_list[:5] - 100)]])
    s, ids = idx.search(q, 10, nprobe=8, rerank=16 if keep else 0)
    want = _filtered(before, gone, 8)
    _same(_arrays(idx), want)
    assert idx.n == idx.nv == live and idx._cdead is None and idx._vdead is None
    assert int(idx.list_off[whole + 1] - idx.list_off[whole]) == 0
    assert not torch.isin(ids, gone).any() and idx.centroids is cent
    twin = _from_arrays(idx, want)
    s2, ids2 = twin.search(q, 10, nprobe=8, rerank=16 if keep else 0)
    assert torch.equal(s, s2) and torch.equal(ids, ids2)
    # 100 more rows: the merged index is the stable full sort of (survivors, new rows)
    y = _data(100, 32, 7)
    idx.add(y, ids=torch.arange(100) + 50_000)
    lab, codes = idx.encode(y)
    s, ids = idx.search(q, 10, nprobe=8)
    al = torch.cat([want["list_of"], lab])
    o = torch.argsort(al, stable=True)
    assert torch.equal(idx.list_of, al[o]) and torch.equal(idx.codes, torch.cat([want["codes"], codes])[o])
    assert torch.equal(idx._pos[: idx.n], torch.cat([want["pos"], torch.arange(live, live + 100)])[o])
    assert torch.equal(idx._vids[: idx.nv], torch.cat([want["vids"], torch.arange(100) + 50_000]))
    assert len(idx) == live + 100 and not torch.isin(ids, gone).any()


def test_upsert():
    idx, x = _built("int8")
    n = 2000
    lists = idx.list_of.clone()
    ids0 = idx.ids.clone()
    # a held id moves to another cluster: the vector of a row of a different list
    a = int(ids0[0])
    other = int(ids0[torch.nonzero(lists != lists[0]).flatten()[0]])
    new_vec = F.normalize(x[other - 100] + 0.01 * torch.randn(32, generator=torch.Generator().manual_seed(3)), dim=0)
    old_vec = x[a - 100].clone()
    fresh = _data(3, 32, 11)
    k = idx.upsert(torch.tensor([a, 70_000, 70_001, 70_002]), torch.cat([new_vec[None], fresh]))
    assert k == 1 and len(idx) == n + 3
    assert idx.n == n + 4 and idx.nv == n + 3  # the old code row is only flagged until the next search
    s, ids = idx.search(torch.stack([new_vec, old_vec]), 5, nprobe=8, rerank=32)
    assert idx.n == idx.nv == n + 3
    assert int(ids[0, 0]) == a and a not in ids[1].tolist()
    # the re-rank score is the new vector's (int8 copy of it)
    sc = new_vec.abs().max() / 127.0
    deq = torch.round(new_vec / sc).clamp(-127, 127) * sc
    assert abs(float(s[0, 0]) - float(new_vec @ deq)) < 1e-5
    all_ids = idx.ids
    assert all_ids.numel() == torch.unique(all_ids).numel() == n + 3  # one code row per live id
    # ids not held behave as add
    ref, _ = _built("int8")
    ref.add(fresh, ids=torch.tensor([70_000, 70_001, 70_002]))
    ref._finalize()
    sel = torch.isin(idx.ids, torch.tensor([70_000, 70_001, 70_002]))
    sel_r = torch.isin(ref.ids, torch.tensor([70_000, 70_001, 70_002]))
    assert torch.equal(idx.codes[sel], ref.codes[sel_r]) and torch.equal(idx.list_of[sel], ref.list_of[sel_r])
    # upsert twice before a search: still one row, the last vector
    idx.upsert(torch.tensor([a]), old_vec[None])
    idx.upsert(torch.tensor([a, a]), torch.stack([old_vec, new_vec]))
    _, ids = idx.search(new_vec[None], 1, nprobe=8, rerank=32)
    assert int(ids[0, 0]) == a and int((idx.ids == a).sum()) == 1 and len(idx) == n + 3


def test_translate_ids():
    idx, x = _built(False)
    n = 2000
    idx.remove(torch.arange(100, 150))  # pending removals: their ids are not translated back to life
    g = torch.Generator().manual_seed(5)
    keep = torch.rand(n + 100, generator=g) < 0.7
    remap = torch.cumsum(keep, 0) - 1
    table = torch.where(keep, remap, torch.full_like(remap, -1)).to(torch.int32)
    old_live = torch.arange(150, n + 100)
    idx.translate_ids(table)
    want = remap[old_live[keep[old_live]]]
    assert len(idx) == want.numel()
    idx._finalize()
    assert torch.equal(torch.sort(idx.ids).values, want) and torch.equal(idx._vids[: idx.nv], want)
    # the vectors still answer to their new ids
    r = int(old_live[keep[old_live]][10])
    _, ids = idx.search(x[r - 100][None], 1, nprobe=8)
    assert int(ids[0, 0]) == int(remap[r])


# ---------------------------------------------------------------- through the tenant graph
def _clustered(n=6000, d=32, C=4, seed=0):
    g0 = torch.Generator().manual_seed(seed)
    cen = F.normalize(torch.randn(C, d, generator=g0), dim=1)
    X = F.normalize(cen.repeat_interleave(n // C, 0) + 0.3 * torch.randn(n, d, generator=g0), dim=1)
    return X, g0


def _system(tmp_path, name, d=32):
    from lazzaro_amd.core.memory_system import MemorySystem
    from lazzaro_amd.core.providers import HashEmbedder, LocalLLM
    return MemorySystem(llm_provider=LocalLLM(), embedding_provider=HashEmbedder(dim=d), enable_async=False,
                        load_from_disk=False, db_dir=str(tmp_path / name), index="ivfpq",
                        index_params={"nlist": 16, "nprobe": 16, "pq_m": 8, "ivf_min_rows": 1000})


def _recall(rows, truth):
    return sum(len(set(a) & set(b)) for a, b in zip(rows, truth)) / sum(len(t) for t in truth)


def test_evicted_rows_leave_the_lists(tmp_path):
    """Evicting more near neighbours of a query than the candidate depth
    (1,200 > 1,024) must not cost the query its true neighbours: the dead
    rows leave the index's lists, the index itself stays (no re-train)."""
    X, g0 = _clustered()
    ms = _system(tmp_path, "a")
    g = ms.graph
    g.add_nodes([f"m{i}" for i in range(len(X))], [f"c{i}" for i in range(len(X))], X, shard=g.shard_id("w"),
                stored=True)
    q = X[:1] + 0.01 * torch.randn(1, 32, generator=g0)
    g.store_search(q, 5, "l2")
    idx, cent = g._ann, g._ann.centroids
    near = torch.topk(-torch.cdist(q, X)[0], 1200).indices
    g.remove_nodes(near.tolist(), unstore=True)
    _, rows = g.store_search(q, 5, "l2")
    assert g._ann is idx and idx.centroids is cent and g.ann_rebuilds == 0 and g.ann_removed == 1200
    cand = idx.candidate_ids(q, 1024, 16)
    assert not torch.isin(cand, near).any()
    alive = torch.ones(len(X), dtype=torch.bool)
    alive[near] = False
    live = torch.nonzero(alive).flatten()
    truth = live[torch.topk(-torch.cdist(q, X[live])[0], 5).indices].tolist()
    # what a rebuild would give: a second graph built from the survivors only
    ms2 = _system(tmp_path, "b")
    g2 = ms2.graph
    g2.add_nodes([f"m{i}" for i in live.tolist()], ["c"] * len(live), X[live], shard=g2.shard_id("w"), stored=True)
    _, rows2 = g2.store_search(q, 5, "l2")
    r_m = _recall([rows[0].tolist()], [truth])
    r_b = _recall([live[rows2[0]].tolist()], [truth])
    assert r_m >= r_b - 0.05, f"recall@5 maintained {r_m} vs rebuilt {r_b}"
    assert ms.get_stats()["engine"]["ann_removed"] == 1200
    ms.close(), ms2.close()


def test_deleted_rows_leave_the_arena_index(tmp_path):
    """HBMStore(index="ivfpq") / ArenaIVF: more deleted near neighbours than
    ``candidates`` (256) -- the search still fills ``limit`` and agrees with
    the flat store on the top hit."""
    from lazzaro_amd.core.vector_store import HBMStore
    st = HBMStore(db_dir=str(tmp_path / "ivf"), device="cpu", metric="cosine", index="ivfpq",
                  nlist=16, nprobe=16, pq_m=8, ivf_min_rows=1000)
    flat = HBMStore(db_dir=str(tmp_path / "flat"), device="cpu", metric="cosine")
    X, g0 = _clustered(n=4000)
    x = X.numpy()
    rows = [{"id": f"m{i}", "content": "c", "embedding": v.tolist()} for i, v in enumerate(x)]
    st.add_nodes(rows, user_id="big")
    flat.add_nodes(rows, user_id="big")
    q = (X[0] + 0.01 * torch.randn(32, generator=g0)).tolist()
    st.search_nodes(q, user_id="big", limit=5)
    ivf = st._arena("big").ivf
    idx = ivf.idx
    assert ivf.candidates < 400
    near = torch.topk(X @ F.normalize(torch.tensor(q), dim=0), 400).indices.tolist()
    dead = [f"m{i}" for i in near]
    st.delete_nodes(dead, user_id="big")
    flat.delete_nodes(dead, user_id="big")
    got = st.search_nodes(q, user_id="big", limit=5)
    want = flat.search_nodes(q, user_id="big", limit=5)
    assert ivf.idx is idx and len(idx) == 4000 - 400
    assert len(got) == 5 and got[0] == want[0] and not set(got) & set(dead)


def _graph_with_index(device="cpu", n=3000, d=32):
    from lazzaro_amd.engine.tenant_graph import TenantGraph
    X, g0 = _clustered(n=n, d=d, seed=2)
    g = TenantGraph(device=device, dim=d, capacity=64)
    g.ann_cfg = {"nlist": 16, "nprobe": 16, "m": 8, "min_rows": 1000, "rerank": 1024}
    g.add_nodes([f"m{i}" for i in range(n)], [f"c{i}" for i in range(n)], X, shard=g.shard_id("w"), stored=True)
    g.take_dirty_rows(), g.take_dirty_edges(), g.take_deleted()
    return g, X, g0


def test_compaction_keeps_the_index():
    """compact() renumbers the index's ids instead of throwing it away: by
    id, the searches equal a twin graph that was never compacted."""
    g, X, g0 = _graph_with_index()
    t, _, _ = _graph_with_index()
    q = X[::300] + 0.01 * torch.randn(10, 32, generator=g0)
    vic = list(range(1, 3000, 3))
    fresh = F.normalize(X[5:45] + 0.05 * torch.randn(40, 32, generator=g0), dim=1)
    for h in (g, t):
        h.store_search(q, 5, "l2")
        h.remove_nodes(vic, drop_edges=True, unstore=True)
        h.take_dirty_rows(), h.take_dirty_edges(), h.take_deleted()
    idx = g._ann
    assert reclaimable(g).sum() == len(vic)
    out = g.compact()
    assert out["reclaimed"] == len(vic)
    for h in (g, t):
        h.add_nodes([f"f{i}" for i in range(40)], ["f"] * 40, fresh, shard=h.shard_id("w"), stored=True)
    s1, r1 = g.store_search(q, 5, "l2")
    s2, r2 = t.store_search(q, 5, "l2")
    assert g._ann is idx and g.ann_rebuilds == 0 and g._ann_covered == g.n == 3000 - len(vic) + 40
    assert len(idx) == g.n
    ids1 = [[g.ids[r] for r in row] for row in r1.tolist()]
    ids2 = [[t.ids[r] for r in row] for row in r2.tolist()]
    assert ids1 == ids2 and torch.equal(s1, s2)


def test_rewritten_embedding_is_upserted():
    """set_embedding on an indexed row, and an id added again: no rebuild,
    and the row is found at its new vector."""
    g, X, g0 = _graph_with_index()
    q = X[:1]
    g.store_search(q, 3, "l2")
    idx, cent = g._ann, g._ann.centroids
    far = X[2999].clone()  # another cluster
    g.set_embedding(0, far.tolist())
    g.add_nodes(["m7"], ["again"], X[2990:2991] * 1.0, shard=g.shard_id("w"), stored=True)
    _, rows = g.store_search(torch.stack([far, X[2990]]), 3, "l2")
    assert g._ann is idx and idx.centroids is cent and g.ann_rebuilds == 0 and g.ann_upserts == 2
    assert 0 in rows[0].tolist() and 7 in rows[1].tolist()
    _, rows = g.store_search(torch.stack([X[0], X[7]]), 3, "l2")
    assert 0 not in rows[0].tolist() and 7 not in rows[1].tolist()
    assert len(idx) == g.n == g._ann_covered
