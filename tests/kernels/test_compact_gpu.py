"""Row reclamation on an MI355X (csrc/kernels/compact.hip, TenantGraph.compact):
the in-place chunked row move against ``X[keep]``, the mark / remap kernels
against their torch formulation, and the twin differentials of
tests/unit/test_compact_rows.py on the GPU -- kernel path == torch
formulation == CPU graph, bit for bit (a compaction only moves bytes)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from lazzaro_amd.engine import tenant_graph as TG  # noqa: E402
from lazzaro_amd.engine.tenant_graph import LOWP_MIN_ROWS, NODE, TenantGraph  # noqa: E402
from lazzaro_amd.ops import tenant_ops as T  # noqa: E402
from tests.unit.test_compact_rows import (NOW, assert_same_answers, assert_same_state, assert_twins, build_graph,  # noqa: E402
                                          by_id, conversations, edges_by_id, ids_of, reclaimable, run_sequential,
                                          system)

N = 1000


def keep_patterns(n: int, chunk: int):
    rng = np.random.default_rng(7)
    k = {"none_dead": np.ones(n, bool), "all_dead": np.zeros(n, bool), "row0_dead": np.ones(n, bool),
         "last_dead": np.ones(n, bool), "alternating": np.arange(n) % 2 == 0, "third": rng.random(n) >= 1 / 3}
    k["row0_dead"][0] = False
    k["last_dead"][-1] = False
    run = np.ones(n, bool)  # a dead run longer than a chunk, live rows after it: the direct path
    run[3:3 + min(chunk + 17, n - 200)] = False
    k["long_dead_run"] = run
    return k


@pytest.mark.parametrize("row_bytes", [3072, 192, 200, 128, 4])
def test_move_rows_matches_gather(row_bytes):
    """Row widths: d = 768 fp32, 16-byte lanes narrower than a wave, the 4-byte
    path (200), int8 at Dp = 128, one word. Chunks of 64 / 256 rows (many
    chunks) and 4096 (one). The tail [n_new, n) is not compared."""
    dev = torch.device("cuda")
    gen = torch.Generator().manual_seed(row_bytes)
    X = torch.randint(0, 256, (N, row_bytes), dtype=torch.uint8, generator=gen)
    for chunk in (64, 256, 4096):
        for name, kp in keep_patterns(N, chunk).items():
            keep = torch.from_numpy(kp.astype(np.uint8)).to(dev)
            remap = T.rc_remap_of(keep)
            m = int(kp.sum())
            assert int(remap[N]) == m
            first = int(np.argmin(kp)) if m < N else N
            col = X.to(dev).clone()
            moved, direct, bounced = T.rc_move_rows(col, keep, remap, N, first, chunk)
            want = X[torch.from_numpy(kp)]
            assert torch.equal(col[:m].cpu(), want), (name, chunk)
            assert moved == (m - first) * row_bytes if m > first else moved == 0, (name, chunk)
            if name == "row0_dead":  # every chunk lands on its own source rows
                assert direct == 0 and bounced == (N + chunk - 1) // chunk
            if name == "long_dead_run" and chunk < 4096:
                assert direct > 0
            if name in ("none_dead", "all_dead"):
                assert direct == bounced == 0
    # the torch formulation gives the same rows
    col = X.to(dev).clone()
    kp = keep_patterns(N, 64)["third"]
    assert T.rc_move_rows_ref(col, torch.from_numpy(kp.astype(np.uint8)).to(dev), N) == int(kp.sum())
    assert torch.equal(col[:int(kp.sum())].cpu(), X[torch.from_numpy(kp)])


def test_move_scalars_matches_gather():
    dev = torch.device("cuda")
    gen = torch.Generator().manual_seed(3)
    kp = keep_patterns(N, 64)["third"]
    keep = torch.from_numpy(kp.astype(np.uint8)).to(dev)
    remap = T.rc_remap_of(keep)
    m = int(kp.sum())
    dts = [torch.uint8, torch.int32, torch.float32, torch.float64] * 5  # 20 columns: two launches
    src = [torch.randint(0, 200, (N,), generator=gen).to(dt) for dt in dts]
    cols = [s.to(dev).clone() for s in src]
    T.rc_move_scalars(cols, keep, remap, N, m)
    for s, c in zip(src, cols):
        assert torch.equal(c[:m].cpu(), s[torch.from_numpy(kp)])


def test_mark_and_remap_match_reference():
    """Random flags, edges and parents (chains of ghost parents among them):
    the kernels against the torch formulation on the CPU."""
    n, ne = 5000, 1500
    gen = torch.Generator().manual_seed(11)
    kind = (torch.rand(n, generator=gen) < 0.3).to(torch.uint8) + 2 * (torch.rand(n, generator=gen) < 0.5).to(torch.uint8)
    kind = torch.where(kind == 3, torch.ones_like(kind), kind)
    stored = (torch.rand(n, generator=gen) < 0.02).to(torch.uint8)
    dirty = (torch.rand(n, generator=gen) < 0.02).to(torch.uint8)
    parent = torch.where(torch.rand(n, generator=gen) < 0.4, torch.randint(0, n, (n,), generator=gen),
                         torch.full((n,), -1)).to(torch.int32)
    src = torch.randint(0, n, (ne,), generator=gen).to(torch.int32)
    dst = torch.randint(0, n, (ne,), generator=gen).to(torch.int32)
    want = T.rc_mark_ref(kind, stored, dirty, parent, src, dst)
    base = ((kind == 1) | (stored != 0) | (dirty != 0)).to(torch.uint8)
    base[src.long()] = 1
    base[dst.long()] = 1
    assert int(want.sum()) > int(base.sum())  # parents (and theirs) were added
    d = lambda t: t.cuda()  # noqa: E731
    got = T.rc_mark(d(kind), d(stored), d(dirty), d(parent), d(src), d(dst))
    assert torch.equal(got.cpu(), want) and 0 < int(want.sum()) < n
    z = torch.zeros(0, dtype=torch.int32)
    assert torch.equal(T.rc_mark(d(kind), d(stored), d(dirty), d(parent), d(z), d(z)).cpu(),
                       T.rc_mark_ref(kind, stored, dirty, parent, z, z))
    remap = T.rc_remap_of(want)
    m = int(remap[n])
    idx = torch.nonzero(want).flatten()
    ps, pd, pp = src.clone(), dst.clone(), parent[idx].clone()
    T.rc_remap_ref(ps, pd, pp, remap)
    gs, gd, gp = d(src), d(dst), d(parent[idx].contiguous())
    T.rc_remap(gs, gd, gp, d(remap))
    assert torch.equal(gs.cpu(), ps) and torch.equal(gd.cpu(), pd) and torch.equal(gp.cpu(), pp)
    assert int(ps.max()) < m and int(pp.max()) < m and torch.equal(idx[ps.long()], src.long())


def test_twin_differential_gpu(monkeypatch):
    """8,192 rows x 768, 64 queries: M * n clears KERNEL_MIN_WORK // 16, so the
    store search runs the MFMA flat_topk + store_rerank path. Kernel
    compaction == torch formulation == never compacted, bit for bit, scores
    included -- with one exception that is not the compaction's: at 64
    queries ``cos_topk`` takes the exact path, a float64 GEMM over all rows,
    and the BLAS behind it picks its summation order by the matrix SHAPE.
    Measured on an MI355X: the same 64 x 768 queries against the 8,195 rows
    and against the 5,993 kept rows differ in 272,567 of 383,552 products by
    at most 3.9e-16, while against the same kept rows gathered from the
    uncompacted graph (same shape, other addresses) they differ in none. So
    the 64-query cos_topk scores are compared bit for bit between the two
    compacted graphs (same shape), and against the uncompacted twin by ids;
    768 queries take cos_topk's kernel path (scan + float64 re-rank kernel,
    arithmetic local to a row), where the scores are bit-equal to the
    uncompacted twin's too."""
    n, d = 8192, 768
    assert 64 * n >= TG.KERNEL_MIN_WORK // 16
    A, B_on, B_off = (build_graph("cuda", n=n, d=d, n_edges=4000) for _ in range(3))
    C = build_graph("cpu", n=n, d=d, n_edges=4000)
    gone = {A.ids[r] for r in np.nonzero(reclaimable(A))[0]}
    assert len(gone) > n // 4
    out_on = B_on.compact(chunk_rows=1024)  # several chunks, bounced ones and direct ones
    monkeypatch.setattr(TG, "COMPACT_KERNEL", False)
    out_off = B_off.compact()
    monkeypatch.setattr(TG, "COMPACT_KERNEL", True)
    out_c = C.compact()
    for k in ("rows_before", "rows_after", "reclaimed", "ghosts_kept", "epoch"):
        assert out_on[k] == out_off[k] == out_c[k], k
    assert out_on["reclaimed"] == len(gone)
    assert_twins(A, B_on, gone)
    assert_twins(A, B_off, gone)
    # the CPU graph: same ids in the same order, same edges, same columns (emb32 is the input, bit for bit)
    assert C.ids[:C.n] == B_on.ids[:B_on.n] and edges_by_id(C) == edges_by_id(B_on)
    sc, sg = by_id(C), by_id(B_on)
    for i, v in sc.items():
        for c in ("sal", "acc", "last", "ts", "shard", "kind", "sup", "has_emb", "stored", "dirty", "parent",
                  "children", "content", "type", "emb32"):
            assert v[c] == sg[i][c], (i, c)
    assert_same_answers(B_on, B_off, nq=64, nq_cos=768)
    assert_same_answers(A, B_off, nq=64, nq_cos=768, gemm_scores=False)
    assert_same_answers(A, B_on, nq=64, nq_cos=768, gemm_scores=False, evict_to=4000)
    vo = B_off.evict(4000, now=NOW)
    assert len(vo) > 0 and B_off.ids[:B_off.n] == B_on.ids[:B_on.n]
    assert torch.equal(B_off.kind[:B_off.n], B_on.kind[:B_on.n])


def test_prefetch_handle_and_guards_gpu():
    n, d, M = 8192, 128, 512
    g = build_graph("cuda", n=n, d=d, n_edges=40000)
    rng = np.random.default_rng(5)
    live = torch.nonzero((g.kind[:g.n] == NODE) & (g.sup[:g.n] == 0)).flatten()
    pick = live[torch.from_numpy(rng.integers(0, live.numel(), M)).cuda()]
    Q = g.emb32[pick] + 0.05 * torch.randn(M, d, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    lab = g.shard[pick].cpu()
    mask = (g.kind[:g.n] == NODE) & (g.sup[:g.n] == 0)
    assert g.dual_prefetch_ok(M, 8)
    h = g.cos_topk_prefetch(Q, mask, lab, 0.5, torch.cuda.Stream())
    assert h["epoch"] == 0
    # an open incremental-components window refuses
    assert g.cc_begin(np.zeros(0, np.int64), 0.5, 0.99, 4)
    with pytest.raises(RuntimeError):
        g.compact()
    g.cc_end()
    tok = g.segment_begin(0.0, None, 0)
    with pytest.raises(RuntimeError):
        g.compact()
    g.segment_end(tok, [])
    assert g.compact()["reclaimed"] > 0
    mask = (g.kind[:g.n] == NODE) & (g.sup[:g.n] == 0)
    (sa, ra), (sb, rb) = g.cos_topk_finish(h, 8, mask)  # epoch mismatch: the lists are discarded
    (fa, fra), (fb, frb) = g.cos_topk(Q, 8, mask, dual_label=lab, min_score=0.5)
    assert torch.equal(ra, fra) and torch.equal(rb, frb) and torch.equal(sa, fa) and torch.equal(sb, fb)
    assert int((ra >= 0).sum()) >= M  # (each query finds at least the row it was made from)


def test_int8_narrow_search_after_compaction():
    """LOWP_MIN_ROWS + 4,096 unit rows at d = 128 (int8 copy at Dp = 128), a
    random quarter removed and unstored; 8 queries take the narrow,
    worst-case-certified int8 regime on the uncompacted twin."""
    n, d = LOWP_MIN_ROWS + 4096, 128
    dev = torch.device("cuda")
    ids = [f"n{i}" for i in range(n)]
    X = torch.randn(n, d, device=dev, generator=torch.Generator("cuda").manual_seed(2))
    X /= X.norm(dim=1, keepdim=True)
    vic = torch.nonzero(torch.rand(n, generator=torch.Generator().manual_seed(4)) < 0.25).flatten().tolist()

    def make():
        g = TenantGraph(device=dev, dim=d, capacity=n)
        g.add_nodes(ids, [""] * n, X, shard=g.shard_id("all"), sal=0.5, stored=True, now=NOW, want_rows=False)
        g.take_dirty_rows()
        g.remove_nodes(vic, drop_edges=False, unstore=True)
        g.take_deleted()
        return g
    A, B = make(), make()
    assert A.emb8 is not None and A.emb8.dtype == torch.int8 and A.unit_rows()
    out = B.compact()
    assert out["reclaimed"] == len(vic) and B.n == n - len(vic)
    Q = X[torch.as_tensor(vic[:4] + [r + 1 for r in vic[:4]], device=dev)] + 0.02 * torch.randn(
        8, d, device=dev, generator=torch.Generator("cuda").manual_seed(9))
    (sa, ra), (sb, rb) = A.store_search(Q, 5, "l2"), B.store_search(Q, 5, "l2")
    assert ids_of(A, ra) == ids_of(B, rb) and torch.equal(sa, sb)
    assert int((ra >= 0).sum()) == 40


def test_continue_after_compaction_gpu(tmp_path, monkeypatch):
    """The consolidate_batch continuation with the native segment applier
    (lazy node decay: the per-row stamps and the removal bitmap after a move)."""
    import time as _time

    from lazzaro_amd.core import consolidation as C
    from lazzaro_amd.engine import native_apply as NA
    monkeypatch.setattr(_time, "time", lambda: NOW)
    monkeypatch.setattr(C.ConsolidationMixin, "NATIVE_APPLY", True)
    monkeypatch.setattr(NA, "LAZY_NODE_DECAY", True)
    runs = []
    orig = C.ConsolidationMixin._native_run

    def counted(self, segs, *a, **k):
        runs.append(len(segs))
        return orig(self, segs, *a, **k)
    monkeypatch.setattr(C.ConsolidationMixin, "_native_run", counted)
    k = 12
    convs = conversations(3 * k)
    a, b = system(tmp_path / "a", "cuda"), system(tmp_path / "b", "cuda")
    for ms in (a, b):
        ms.consolidate_batch(convs[:k], now=NOW)
    out = b.compact_memory()
    assert out["reclaimed"] > 0 and sum(runs) > 0
    assert_same_state(a, b)
    for part in (convs[k:2 * k], convs[2 * k:]):
        sa, sb = a.consolidate_batch(part, now=NOW), b.consolidate_batch(part, now=NOW)
        assert sa == sb and sa["evicted"] > 0
        assert_same_state(a, b)
        assert b.compact_memory(shrink=True)["reclaimed"] > 0
    c = system(tmp_path / "c", "cpu")  # and the CPU run of the same script, never compacted
    for part in (convs[:k], convs[k:2 * k], convs[2 * k:]):
        c.consolidate_batch(part, now=NOW)
    sc, sb = ms_ids(c), ms_ids(b)
    assert sc == sb


def ms_ids(ms):
    g = ms.graph
    kind = g.kind[:g.n].cpu().numpy()
    return [g.ids[r] for r in np.nonzero(kind == NODE)[0]], sorted((s, d) for s, d, *_ in edges_by_id(g))
