"""IVF-PQ maintenance on an MI355X (csrc/kernels/ivfmaint.hip,
IVFPQIndex._finalize): the in-place spread against the stable-argsort
formulation, the mark / count pass against bincount, the whole index against
``_finalize_ref`` on the CPU -- bit for bit, the kernels only move bytes --
its peak memory, and the tenant graph keeping its index through evictions, a
compaction and appends."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from lazzaro_amd.index import ivfpq as IV  # noqa: E402
from lazzaro_amd.index.ivfpq import IVFPQIndex  # noqa: E402
from lazzaro_amd.ops import ivf_ops as V  # noqa: E402
from lazzaro_amd.utils.faults import KernelError  # noqa: E402

DEV = torch.device("cuda")
NLIST = 64
EMPTY = (5, 17)  # lists without main rows


def main_lists(n0: int, gen) -> torch.Tensor:
    ok = torch.tensor([l for l in range(NLIST) if l not in EMPTY])
    lists = ok[torch.randint(0, ok.numel(), (n0,), generator=gen)]
    if n0:
        lists[0], lists[-1] = 0, NLIST - 1  # rows in the first and in the last list
    return torch.sort(lists).values.to(torch.int32)


def tails(n0: int, gen):
    rnd = lambda t: torch.randint(0, NLIST, (t,), generator=gen).to(torch.int32)  # noqa: E731
    f = lambda t, l: torch.full((t,), l, dtype=torch.int32)  # noqa: E731
    return {"one": rnd(1), "64": rnd(64), "third": rnd(max(1, n0 // 3)), "all_list0": f(100, 0),
            "all_last": f(100, NLIST - 1), "no_main_rows": f(70, EMPTY[0]),
            "empty_main_lists": torch.tensor(list(EMPTY) * 20, dtype=torch.int32)}


@pytest.mark.parametrize("row_bytes", [8, 16, 48, 64, 96, 4, 6])
def test_spread_rows_matches_stable_argsort(row_bytes):
    """16-byte lanes (16, 48, 64, 96), 4-byte (8, 4) and 1-byte (6) rows;
    chunks of 64 / 1024 rows (many chunks) and n0 (one). The merged column
    must be the stable argsort by list of (main rows, tail rows)."""
    gen = torch.Generator().manual_seed(row_bytes)
    for n0 in (0, 1, 257, 70_001):
        lists = main_lists(n0, gen)
        X = torch.randint(0, 256, (n0, row_bytes), dtype=torch.uint8, generator=gen)
        off = torch.zeros(NLIST + 1, dtype=torch.int64)
        off[1:] = torch.cumsum(torch.bincount(lists.long(), minlength=NLIST), 0)
        for name, tl in tails(n0, gen).items():
            t = tl.numel()
            Y = torch.randint(0, 256, (t, row_bytes), dtype=torch.uint8, generator=gen)
            o = torch.argsort(torch.cat([lists, tl]), stable=True)
            want = torch.cat([X, Y])[o]
            order, ins, dest = V.ivf_tail_slots(tl.to(DEV), off.to(DEV), NLIST)
            l_d = lists.to(DEV)
            first = V.ivf_spread_first(l_d, ins, n0)
            # the stats case also starts below the first moving row, so that one chunk
            # holds rows that stay (the end of list 0) AND rows that move (not on a chunk boundary)
            low = min(first, 0 if int(off[1]) % 64 else 1)
            for chunk in (64, 1024, max(n0, 1)):
                for f0 in ((first, low) if name == "all_list0" else (first,)):
                    col = torch.zeros((n0 + t, row_bytes), dtype=torch.uint8, device=DEV)
                    col[:n0] = X.to(DEV)
                    moved, direct, bounced = V.ivf_spread_rows(col, l_d, ins, n0, f0, chunk)
                    col[dest] = Y.to(DEV)[order]
                    assert torch.equal(col.cpu(), want), (n0, name, chunk, f0)
                    if name == "all_last":  # nothing moves
                        assert (moved, direct, bounced) == (0, 0, 0)
                    if name == "all_list0" and f0 == low and chunk == 64 and n0 > 257:
                        # the chunk that holds the end of list 0 lands on its own rows, the rest jump 100 > 64 rows
                        assert direct >= 1 and bounced >= 1, (direct, bounced)
                    if name == "all_list0" and f0 == first and chunk == 64 and n0 > 257:
                        assert direct >= 1 and bounced == 0 and moved == (n0 - first) * row_bytes
        # the torch formulation gives the same rows
        if n0:
            tl = tails(n0, gen)["third"]
            order, ins, dest = V.ivf_tail_slots(tl, off, NLIST)
            col = torch.cat([X, torch.zeros((tl.numel(), row_bytes), dtype=torch.uint8)])
            V.ivf_spread_rows_ref(col, lists, ins, n0)
            col2 = torch.cat([X, torch.zeros((tl.numel(), row_bytes), dtype=torch.uint8)]).to(DEV)
            V.ivf_spread_rows(col2, lists.to(DEV), ins.to(DEV), n0, V.ivf_spread_first(lists, ins, n0), 1024)
            moved = torch.ones(n0 + tl.numel(), dtype=torch.bool)
            moved[dest] = False  # the gaps keep stale bytes
            assert torch.equal(col[moved], col2.cpu()[moved])


def test_spread_rows_out_of_place_key_column():
    gen = torch.Generator().manual_seed(3)
    n0 = 5000
    lists = main_lists(n0, gen)
    tl = tails(n0, gen)["third"]
    off = torch.zeros(NLIST + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(torch.bincount(lists.long(), minlength=NLIST), 0)
    order, ins, dest = V.ivf_tail_slots(tl.to(DEV), off.to(DEV), NLIST)
    col = torch.cat([lists, torch.zeros_like(tl)]).to(DEV)
    key = lists.to(DEV)
    first = V.ivf_spread_first(key, ins, n0)
    _, direct, bounced = V.ivf_spread_rows(col, key, ins, n0, first, 64, src=key)
    col[dest] = tl.to(DEV)[order]
    assert bounced == 0 and direct > 0
    assert torch.equal(col.cpu(), torch.sort(torch.cat([lists, tl]), stable=True).values)


def test_spread_rows_rejects_invalid_schedules():
    """A decreasing shift and a destination past the column: an error, and
    nothing launched (the column keeps its bytes)."""
    gen = torch.Generator().manual_seed(4)
    n0 = 1000
    lists = main_lists(n0, gen).to(DEV)
    X = torch.randint(0, 256, (n0 + 50, 16), dtype=torch.uint8, generator=gen)
    col = X.to(DEV)
    ins = torch.arange(NLIST, -1, -1, dtype=torch.int64, device=DEV)  # decreasing
    with pytest.raises(KernelError):
        V.ivf_spread_rows(col, lists, ins, n0, 0, 64)
    ins = torch.zeros(NLIST + 1, dtype=torch.int64, device=DEV)
    ins[1:] = 51  # row n0 - 1 would land on row n0 + 50: one past the column
    with pytest.raises(KernelError):
        V.ivf_spread_rows(col, lists, ins, n0, 0, 64)
    ins[1:] = 30
    with pytest.raises(KernelError):  # chunks that overlap themselves, and a bounce buffer of half a chunk
        V.ivf_spread_rows(col, lists, ins, n0, 0, 64, bounce=torch.empty(32 * 16, dtype=torch.uint8, device=DEV))
    torch.cuda.synchronize()
    assert torch.equal(col.cpu(), X)


def test_mark_count_matches_bincount():
    gen = torch.Generator().manual_seed(5)
    n = 70_001
    # lists of length 0 (EMPTY), 1 (list 1) and > 64
    ok = torch.tensor([l for l in range(NLIST) if l not in EMPTY + (1,)])
    lists = ok[torch.randint(0, ok.numel(), (n - 1,), generator=gen)]
    lists = torch.sort(torch.cat([lists, torch.tensor([1])])).values.to(torch.int32)
    cnt_all = torch.bincount(lists.long(), minlength=NLIST)
    assert int(cnt_all[1]) == 1 and int(cnt_all[EMPTY[0]]) == 0 and int(cnt_all.max()) > 64
    pos = torch.randperm(n, generator=gen)
    cdead = (torch.rand(n, generator=gen) < 0.3).to(torch.uint8)
    vdead = (torch.rand(n, generator=gen) < 0.3).to(torch.uint8)
    for cd, vd in ((cdead, vdead), (None, vdead), (cdead, None), (None, None)):
        for ncount in (n, 40_000):
            keep, cnt = V.ivf_mark_count(lists.to(DEV), pos.to(DEV), cd.to(DEV) if cd is not None else None,
                                         vd.to(DEV) if vd is not None else None, NLIST, ncount)
            dead = torch.zeros(n, dtype=torch.bool)
            if cd is not None:
                dead |= cd.bool()
            if vd is not None:
                dead |= vd[pos].bool()
            assert torch.equal(keep.cpu(), (~dead).to(torch.uint8))
            want = torch.bincount(lists[:ncount][~dead[:ncount]].long(), minlength=NLIST)
            assert torch.equal(cnt.cpu(), want)
            k2, c2 = V.ivf_mark_count_ref(lists, pos, cd, vd, NLIST, ncount)
            assert torch.equal(k2, keep.cpu()) and torch.equal(c2, want)


# ---------------------------------------------------------------- the whole index
STATE = ("_codes", "_list", "_pos", "_vids", "_vec", "_vscale", "_cdead", "_vdead", "list_off", "centroids",
         "codebooks")


def cpu_copy(idx: IVFPQIndex) -> IVFPQIndex:
    """The index with its pending state, on the CPU."""
    o = IVFPQIndex(idx.dim, nlist=idx.nlist, m=idx.m, device="cpu", keep_vectors=idx.keep_vectors)
    for name in STATE:
        t = getattr(idx, name)
        setattr(o, name, None if t is None else t.cpu().clone())
    for name in ("n", "nv", "cap", "_sorted_n", "_nlive", "_dirty"):
        setattr(o, name, getattr(idx, name))
    return o


def arrays(idx: IVFPQIndex) -> dict:
    out = {"codes": idx.codes, "list_of": idx.list_of, "pos": idx._pos[: idx.n], "vids": idx._vids[: idx.n],
           "list_off": idx.list_off}
    if idx._vec is not None:
        out.update(vectors=idx.vectors, vscale=idx.vscale)
    return {k: v.cpu() for k, v in out.items()}


def hand_built(n, d, m, nlist, keep, dev, seed=0) -> IVFPQIndex:
    """Codes, lists and ids through the setters, random quantisers: no training."""
    gen = torch.Generator().manual_seed(seed)
    idx = IVFPQIndex(d, nlist=nlist, m=m, device=dev, keep_vectors=keep)
    idx.centroids = torch.nn.functional.normalize(torch.randn(nlist, d, generator=gen), dim=1).to(dev)
    if torch.device(dev).type == "cuda":
        idx.centroids16 = idx._pad(idx.centroids)
    idx.codebooks = (0.1 * torch.randn(m, 256, d // m, generator=gen)).to(dev)
    lists = torch.sort(torch.randint(0, nlist, (n,), generator=gen)).values
    idx.codes = torch.randint(0, 256, (n, m), dtype=torch.uint8, generator=gen)
    idx.list_of = lists
    idx.ids = torch.arange(n)
    off = torch.zeros(nlist + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(torch.bincount(lists, minlength=nlist), 0)
    idx.list_off = off.to(dev)
    if keep:
        idx._vec = torch.randint(0, 256, (n, d), dtype=torch.uint8, generator=gen).to(dev)
        idx._vscale = (torch.rand(n, generator=gen) / 127.0).to(dev)
    return idx


@pytest.mark.parametrize("kernel", [True, False])
@pytest.mark.parametrize("keep", [False, "int8"])
def test_index_rounds_match_finalize_ref(monkeypatch, kernel, keep):
    """Three rounds of interleaved remove / add / upsert / translate_ids: after
    each, every array equals ``_finalize_ref`` run on a CPU copy of the pending
    state, and the searches of the two are bit-equal."""
    monkeypatch.setattr(IV, "MAINT_KERNEL", kernel)
    n, d, m, nlist = 50_000, 64, 16, 64
    gen = torch.Generator().manual_seed(9)
    idx = hand_built(n, d, m, nlist, keep, DEV)
    idx.reserve(80_000)
    idx.chunk_rows = 4096  # several chunks per move
    next_id = n
    q = torch.randn(16, d, generator=gen)
    for rnd in range(3):
        live = idx._vids[: idx.nv][(idx._vdead[: idx.nv] == 0) if idx._vdead is not None else slice(None)].cpu()
        gone = live[torch.randperm(live.numel(), generator=gen)[:2000]]
        assert idx.remove(torch.cat([gone, torch.tensor([next_id + 7, -3])])) == 2000
        idx.add(torch.randn(1500, d, generator=gen), ids=torch.arange(next_id, next_id + 1500))
        next_id += 1500
        live = live[~torch.isin(live, gone)]
        held = live[torch.randperm(live.numel(), generator=gen)[:300]]
        up = torch.cat([held, torch.arange(next_id, next_id + 200)])
        assert idx.upsert(up, torch.randn(500, d, generator=gen)) == 300
        next_id += 200
        if rnd == 1:
            km = torch.rand(next_id, generator=gen) < 0.9
            table = torch.where(km, torch.cumsum(km, 0) - 1, torch.full((next_id,), -1, dtype=torch.long))
            idx.translate_ids(table.to(DEV))
            next_id = int(km.sum())
            idx.remove(torch.arange(40, 60))  # a removal after the renumbering, in the new ids
        ref = cpu_copy(idx)
        ref._finalize_ref()
        base = idx._codes.data_ptr()
        idx._finalize()
        assert idx._codes.data_ptr() == base or not kernel  # in place: no second code buffer
        a, b = arrays(idx), arrays(ref)
        assert idx.n == idx.nv == ref.n == ref.nv == len(idx) == len(ref)
        for k in b:
            assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), (rnd, k)
        twin = hand_built(1, d, m, nlist, keep, DEV)
        twin.centroids, twin.codebooks = idx.centroids, idx.codebooks
        twin.codes, twin.list_of, twin.list_off = b["codes"], b["list_of"], b["list_off"].to(DEV)
        twin.ids = b["vids"]
        twin._pos = b["pos"].to(DEV)
        if keep:
            twin._vec, twin._vscale = b["vectors"].to(DEV), b["vscale"].to(DEV)
        s1, i1 = idx.search(q, 10, nprobe=8)
        s2, i2 = twin.search(q, 10, nprobe=8)
        assert torch.equal(s1, s2) and torch.equal(i1, i2)
        assert torch.unique(idx.ids).numel() == idx.n


def test_finalize_peak_memory():
    """2M x 64-byte codes: a finalize after 1,000 appends and 1,000 removals
    stays under 32 B/row of temporaries (12 narrow columns, 4 remap, 2 flags,
    per column kind, + the 8 MiB bounce buffer and the tail) -- the full
    sort's second code buffer alone is 64 B/row."""
    n, m = 2_000_000, 64
    gen = torch.Generator(device="cuda").manual_seed(0)
    idx = IVFPQIndex(64, nlist=1024, m=m, device=DEV)
    idx.centroids = torch.nn.functional.normalize(torch.randn(1024, 64, device=DEV, generator=gen), dim=1)
    idx.centroids16 = idx._pad(idx.centroids)
    idx.codebooks = 0.1 * torch.randn(m, 256, 1, device=DEV, generator=gen)
    lists = torch.sort(torch.randint(0, 1024, (n,), device=DEV, generator=gen)).values
    idx.codes = torch.randint(0, 256, (n, m), dtype=torch.uint8, device=DEV, generator=gen)
    idx.list_of = lists
    idx.ids = torch.arange(n, device=DEV)
    idx.list_off = torch.zeros(1025, dtype=torch.int64, device=DEV)
    idx.list_off[1:] = torch.cumsum(torch.bincount(lists, minlength=1024), 0)
    idx.chunk_rows = (8 << 20) // m
    idx.add(torch.randn(1000, 64, device=DEV, generator=gen), ids=torch.arange(n, n + 1000))
    assert idx.remove(torch.randint(0, n, (1000,), device=DEV, generator=gen).unique()) > 900
    want_lists = torch.sort(idx._list[: idx.n][idx._vdead[idx._pos[: idx.n]] == 0]).values
    del lists
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    idx._finalize()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert peak < n * m // 2, f"{peak / n:.1f} B/row of temporaries"
    assert torch.equal(idx.list_of, want_lists) and idx.n == idx.nv == len(idx)


# ---------------------------------------------------------------- through the tenant graph
def _recall(rows, truth):
    return sum(len(set(a) & set(b)) for a, b in zip(rows, truth)) / sum(len(t) for t in truth)


def test_tenant_graph_keeps_its_index_gpu():
    """200,000 x 128 clustered rows: 5,000 evicted (among them the 1,200
    nearest of 8 queries -- more than the 1,024 candidates), compacted, 2,000
    fresh rows. The index is never rebuilt, no dead row is a candidate, and
    recall@10 against the exact truth over the live rows is within 0.05 of a
    twin graph rebuilt from the live rows."""
    from lazzaro_amd.engine.tenant_graph import TenantGraph
    g0 = torch.Generator(device="cuda").manual_seed(0)
    C, per, d = 400, 500, 128
    F = torch.nn.functional
    cen = F.normalize(torch.randn(C, d, device=DEV, generator=g0), dim=1)
    X = F.normalize(cen.repeat_interleave(per, 0) + 0.5 * torch.randn(C * per, d, device=DEV, generator=g0) / d ** 0.5,
                    dim=1)
    N = len(X)
    cfg = {"nlist": 512, "nprobe": 16, "m": 32, "min_rows": 100_000}
    q = F.normalize(X[:1] + 0.3 * torch.randn(8, d, device=DEV, generator=g0) / d ** 0.5, dim=1)  # 8 near one row

    def graph(ids, rows):
        g = TenantGraph(device="cuda", dim=d, capacity=N + 4096)
        g.ann_cfg = dict(cfg)
        g.add_nodes(ids, [""] * len(ids), rows, shard=g.shard_id("w"), stored=True)
        g.take_dirty_rows(), g.take_dirty_edges(), g.take_deleted()
        return g
    g = graph([f"m{i}" for i in range(N)], X)
    g.store_search(q, 10, "l2")
    idx, cent = g._ann, g._ann.centroids
    near = torch.unique(torch.topk(-torch.cdist(q, X), 1200, dim=1).indices)
    assert near.numel() < 4000  # the queries are neighbours: their 1,200 nearest overlap
    rest = torch.ones(N, dtype=torch.bool, device=DEV)
    rest[near] = False
    rest = torch.nonzero(rest).flatten()
    vic = torch.cat([near, rest[torch.randperm(rest.numel(), device=DEV, generator=g0)[: 5000 - near.numel()]]])
    vic = torch.sort(vic).values
    assert vic.numel() == 5000
    g.remove_nodes(vic.cpu().tolist(), drop_edges=True, unstore=True)
    g.take_dirty_rows(), g.take_dirty_edges(), g.take_deleted()
    g.store_search(q, 10, "l2")  # the dead rows leave the lists here ...
    out = g.compact()            # ... and the survivors are renumbered here
    assert out["reclaimed"] == vic.numel()
    fresh = F.normalize(cen[:20].repeat_interleave(100, 0) + 0.5 * torch.randn(2000, d, device=DEV, generator=g0)
                        / d ** 0.5, dim=1)
    g.add_nodes([f"f{i}" for i in range(2000)], [""] * 2000, fresh, shard=g.shard_id("w"), stored=True)
    _, rows = g.store_search(q, 10, "l2")
    assert g._ann is idx and idx.centroids is cent and g.ann_rebuilds == 0 and g._ann_covered == g.n
    assert g.ann_removed == vic.numel() and len(idx) == g.n == N - vic.numel() + 2000
    alive = torch.ones(N, dtype=torch.bool, device=DEV)
    alive[vic] = False
    live = torch.cat([X[alive], fresh])
    live_ids = [f"m{i}" for i in torch.nonzero(alive).flatten().cpu().tolist()] + [f"f{i}" for i in range(2000)]
    assert list(g.ids[: g.n]) == live_ids  # every row of the graph is live: no candidate can be a dead row
    cand = idx.candidate_ids(q, 1024, 16)
    assert int(cand.max()) < g.n and torch.unique(idx.ids).numel() == g.n
    truth = torch.topk(-torch.cdist(q, live), 10, dim=1).indices.cpu().tolist()
    t = graph(live_ids, live)  # the rebuild: trained on the live rows only
    _, rows_t = t.store_search(q, 10, "l2")
    r_m, r_b = _recall(rows.cpu().tolist(), truth), _recall(rows_t.cpu().tolist(), truth)
    assert r_m >= r_b - 0.05, f"recall@10 maintained {r_m} vs rebuilt {r_b}"
