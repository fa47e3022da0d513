"""Filtered IVF-PQ search on the CPU tier: the numpy reference of the filtered
kernels (tests/kernels/_ivfpq_filter_ref.py) checked by hand, ``filtered_nprobe``,
``IVFPQIndex.filter_rows`` / ``search(allow=)`` in their torch formulation,
``order_gen`` and stale lists, and the opt-in TenantGraph route against the
flat filtered search, bit for bit (tests/kernels/_filtered_tenant.py)."""
import numpy as np
import pytest
import torch

from lazzaro_amd.index.ivfpq import FilteredLists, IVFPQIndex, filtered_nprobe
from tests.kernels import _filtered_tenant as T
from tests.kernels import _ivfpq_filter_ref as FR
from tests.kernels import _ivfpq_ref as R

NEG = float("-inf")


# ------------------------------------------------------------------ the reference, by hand
def test_filter_rows_ref_by_hand():
    # code rows 0..6 in lists [0,2) [2,2) [2,5) [5,7); code row r holds vector pos[r] whose id is vids[pos[r]]
    pos = np.array([3, 0, 6, 1, 5, 2, 4])
    vids = np.array([4, -1, 9, 0, 2, 1, 3])  # ids of the code rows: 0, 4, 3, -1, 1, 9, 2
    off = np.array([0, 2, 2, 5, 7])
    allow = np.array([1, 0, 7, 1, 1], dtype=np.uint8)  # ids 0, 2, 3, 4 pass; 1 fails; -1 and 9 are outside
    fr, fo, cnt = FR.filter_rows_ref(pos, vids, allow, FR.KIND_U8, off)
    assert fr.dtype == np.int32 and fo.dtype == np.int64
    assert fr.tolist() == [0, 1, 2, 6] and fo.tolist() == [0, 2, 2, 3, 4] and cnt == 4
    bias = np.array([0.0, NEG, -3.5, 1.0, -0.0], dtype=np.float32)  # the same ids as a bias: 0.0 and negatives pass
    fr2, fo2, _ = FR.filter_rows_ref(pos, vids, bias, FR.KIND_BIAS, off)
    assert fr2.tolist() == fr.tolist() and fo2.tolist() == fo.tolist()
    fr3, fo3, cnt3 = FR.filter_rows_ref(pos, vids, allow, FR.KIND_U8, off, max_rows=3)  # overflow: cut and clamped
    assert fr3.tolist() == [0, 1, 2] and fo3.tolist() == [0, 2, 2, 3, 3] and cnt3 == 4
    fr4, fo4, _ = FR.filter_rows_ref(pos, vids, np.zeros(0, dtype=np.uint8), FR.KIND_U8, off)
    assert fr4.size == 0 and fo4.tolist() == [0, 0, 0, 0, 0]


def test_filtered_scan_refs_by_hand():
    # M = 1: the score of a row is base + lut[0][code]; list 0 = rows 0..4, list 1 = rows 5..6
    codes = np.array([[5], [9], [9], [1], [7], [3], [9]], dtype=np.uint8)
    lut = np.arange(256, dtype=np.float32)[None, None, :]
    off = np.array([0, 5, 7])
    probes = np.array([[0, 1, -1]], dtype=np.int32)
    coarse = np.array([[0.0, 100.0, 0.0]], dtype=np.float32)
    mask = np.array([1, 0, 1, 1, 1, 0, 1], dtype=bool)  # row 1 (the lower of the tied 9s) and row 5 fail
    fr, fo = FR.lists_of_mask(mask, off)
    assert fr.tolist() == [0, 2, 3, 4, 6] and fo.tolist() == [0, 4, 5]
    S, Rw = FR.scan_f_ref(codes, fo, fr, probes, coarse, lut, 3)
    assert Rw[0].tolist() == [[2, 4, 0], [6, -1, -1], [-1, -1, -1]]  # code rows, not positions
    assert S[0, 0].tolist() == [9.0, 7.0, 5.0] and S[0, 1].tolist() == [109.0, NEG, NEG]
    W = 8
    SD, RD = FR.deep_f_ref(codes, fo, fr, probes, coarse, lut, W)
    assert RD[0, 0, 0].tolist() == [2, 4] and RD[0, 0, 1].tolist() == [-1, -1]  # 4 positions: all in wave 0
    (rows, scores), = FR.thresh_f_ref(codes, fo, fr, probes, coarse, lut, np.array([7.0]))
    assert rows.tolist() == [2, 4, 6] and scores.tolist() == [9.0, 7.0, 109.0]
    # all-pass lists are the unfiltered scan
    fr, fo = FR.lists_of_mask(np.ones(7, dtype=bool), off)
    a, b = FR.scan_f_ref(codes, fo, fr, probes, coarse, lut, 3), R.scan_ref(codes, off, probes, coarse, lut, 3)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_filtered_nprobe_edges():
    assert filtered_nprobe(16, 4096, 1 << 21, 1 << 21) == 16      # count = n: the unfiltered probe count
    assert filtered_nprobe(16, 4096, 1 << 21, 1 << 20) == 32      # half the rows pass: twice the lists
    assert filtered_nprobe(16, 4096, 1000, 3) == 4096             # ceil(16 * 1000 / 3) = 5334 > nlist
    assert filtered_nprobe(16, 4096, 1000, 300) == 54             # ceil(53.33)
    assert filtered_nprobe(16, 4096, 1 << 21, 1) == 4096          # count = 1: the nlist cap
    assert filtered_nprobe(16, 1 << 30, 1000, 1) == 16000         # count = 1, uncapped: nprobe * n
    assert filtered_nprobe(64, 32, 100, 100) == 32                # nprobe above nlist


# ------------------------------------------------------------------ IVFPQIndex on CPU
def _index(n=3000, d=32, seed=0, nlist=8, m=8):
    g = torch.Generator().manual_seed(seed)
    cen = torch.nn.functional.normalize(torch.randn(12, d, generator=g), dim=1)
    x = torch.nn.functional.normalize(cen[torch.randint(0, 12, (n,), generator=g)]
                                      + 0.3 * torch.randn(n, d, generator=g) / d ** 0.5, dim=1)
    idx = IVFPQIndex(d, nlist=nlist, m=m, device="cpu")
    idx.train(x, iters=3, pq_iters=3)
    idx.add(x)
    return idx, x, g


@pytest.fixture(scope="module")
def cpu_index():
    return _index()


def test_filter_rows_cpu_equals_reference(cpu_index):
    idx, x, g = cpu_index
    n = len(x)
    mask = torch.rand(n + 50, generator=g) < 0.3
    mask = mask[: n - 100]  # ids >= n - 100 are outside the mask: they fail
    fl = idx.filter_rows(mask)
    pos, vids, off = idx._pos[: idx.n].numpy(), idx._vids.numpy(), idx.list_off.numpy()
    fr, fo, cnt = FR.filter_rows_ref(pos, vids, mask.numpy().astype(np.uint8), FR.KIND_U8, off)
    assert fl.rows.dtype == torch.int32 and fl.off.dtype == torch.int64 and fl.gen == idx.order_gen
    assert np.array_equal(fl.rows.numpy(), fr) and np.array_equal(fl.off.numpy(), fo) and cnt == int(mask.sum())
    bias = torch.where(mask, torch.randn(mask.numel(), generator=g), torch.tensor(NEG))
    fb = idx.filter_rows(bias)
    assert torch.equal(fb.rows, fl.rows) and torch.equal(fb.off, fl.off)
    cut = idx.filter_rows(mask, max_rows=cnt // 2)
    fr, fo, _ = FR.filter_rows_ref(pos, vids, mask.numpy().astype(np.uint8), FR.KIND_U8, off, cnt // 2)
    assert np.array_equal(cut.rows.numpy(), fr) and np.array_equal(cut.off.numpy(), fo) and fo.max() == cnt // 2
    with pytest.raises(TypeError):
        idx.filter_rows(mask.long())


@pytest.mark.parametrize("k", (1, 10, 40))
def test_search_allow_is_the_full_ranking_minus_failing_ids(cpu_index, k):
    idx, x, g = cpu_index
    n = len(x)
    q = x[[5, 700, 2222]] + 0.05 * torch.randn(3, x.shape[1], generator=torch.Generator().manual_seed(k))
    mask = torch.rand(n, generator=torch.Generator().manual_seed(9)) < 0.25
    full_s, full_i = idx.search(q, k=n, nprobe=3)  # every row of the probed lists, ranked
    s, i = idx.search(q, k=k, nprobe=3, allow=mask)
    for a in range(3):
        keep = (full_i[a] >= 0) & mask[full_i[a].clamp_min(0)]
        want_i, want_s = full_i[a][keep][:k], full_s[a][keep][:k]
        assert want_i.numel() == k
        assert torch.equal(i[a], want_i) and torch.equal(s[a], want_s)
    # the same through prebuilt lists, candidate_ids, and a mask nobody passes
    fl = idx.filter_rows(mask)
    s2, i2 = idx.search(q, k=k, nprobe=3, allow=fl)
    assert torch.equal(s2, s) and torch.equal(i2, i)
    assert torch.equal(idx.candidate_ids(q, k, 3, allow=fl), i)
    s0, i0 = idx.search(q, k=k, nprobe=3, allow=torch.zeros(n, dtype=torch.bool))
    assert bool((i0 == -1).all()) and bool(torch.isneginf(s0).all())
    s1, i1 = idx.search(q, k=k, nprobe=3)  # allow=None: today's code
    assert torch.equal(i1, full_i[:, :k]) and torch.equal(s1, full_s[:, :k])


def test_order_gen_bumps_on_every_mutator():
    idx, x, g = _index(n=600, seed=3)
    seen = [idx.order_gen]

    def bumped(what):
        assert idx.order_gen not in seen, what
        assert idx.order_gen > seen[-1], what
        seen.append(idx.order_gen)
    idx._finalize()
    bumped("_finalize after add")
    idx._finalize()
    assert idx.order_gen == seen[-1]  # nothing pending: nothing moved
    idx.add(x[:5], ids=torch.arange(600, 605))
    bumped("add / _append")
    idx._finalize()
    bumped("_finalize of a tail")
    assert idx.remove([1, 2, 3]) == 3
    bumped("remove")
    idx.upsert(torch.tensor([7, 900]), x[:2])
    bumped("upsert")
    idx.translate_ids(torch.arange(2000))
    bumped("translate_ids")
    idx.search(x[:1], k=3, nprobe=2)
    bumped("the search's _finalize")
    idx.search(x[:1], k=3, nprobe=2)
    assert idx.order_gen == seen[-1]  # a search of a clean index leaves it
    idx.ids = idx._vids[: idx.nv].clone()
    bumped("ids setter")
    idx.codes = idx.codes.clone()
    bumped("codes setter")
    other, _, _ = _index(n=600, seed=3)
    assert other.order_gen not in seen  # generations are not shared between indexes


def test_stale_lists_are_rebuilt_or_rejected():
    idx, x, g = _index(n=800, seed=4)
    mask = torch.rand(900, generator=g) < 0.5
    q = x[:2]
    fl = idx.filter_rows(mask)
    bare = idx.filter_rows(mask, keep_mask=False)
    assert isinstance(fl, FilteredLists) and fl.allow is mask and bare.allow is None
    gone = torch.nonzero(mask[:800]).flatten()[:50]
    idx.remove(gone)
    idx.add(x[:30], ids=torch.arange(800, 830))
    assert fl.gen != idx.order_gen
    want = idx.search(q, k=10, nprobe=8, allow=mask)
    got = idx.search(q, k=10, nprobe=8, allow=fl)  # rebuilt from the mask it carries, in place
    assert fl.gen == idx.order_gen and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert not set(got[1].flatten().tolist()) & set(gone.tolist())
    assert torch.equal(fl.rows, idx.filter_rows(mask).rows)
    with pytest.raises(ValueError, match="stale"):
        idx.search(q, k=10, nprobe=8, allow=bare)
    with pytest.raises(ValueError, match="stale"):
        idx.candidate_ids(q, 10, 8, allow=bare)


# ------------------------------------------------------------------ TenantGraph on CPU
def test_tenant_graph_filtered_route_equals_flat_cpu(monkeypatch):
    from lazzaro_amd.engine import tenant_graph as TG
    monkeypatch.setattr(TG, "FILTER_SPARSE_MAX_ROWS", 0)
    steps = []
    for step, g, (s1, r1), t, (s2, r2) in T.run("cpu"):
        steps.append(step)
        assert g.filtered_ann == len(steps) and t.filtered_ann == 0, step  # the switch off: never the index route
        assert g.filtered_sparse == 0 and g._ann is not None and t._ann is None
        assert torch.equal(r1, r2), step
        assert torch.equal(s1.view(torch.int32), s2.view(torch.int32)), step
        assert bool((r1 >= 0).all()) and bool((g.sal[r1.flatten()] >= 0.5).all())
        assert 512 <= g._filter_plan(TG_filter(), True).count <= 1024
        assert T.N / g._filter_plan(TG_filter(), True).count <= TG.FILTER_ANN_MAX_SCALE
    assert steps == ["first", "evicted", "rewritten"]
    assert g.ann_rebuilds == 0 and g.ann_upserts == 40 and g.ann_removed > 0
    # the lists are cached on the plan: a second search of the same state builds nothing
    plan = g._filter_plan(TG_filter(), True)
    fl = plan.ann_lists
    assert fl is not None and fl.gen == g._ann.order_gen
    g.store_search(torch.zeros(T.D) + 0.125, T.K, "l2", where=T.WHERE)
    assert g._filter_plan(TG_filter(), True).ann_lists is fl and g.filtered_ann == 4


def TG_filter():
    from lazzaro_amd.core.filters import MemoryFilter
    return MemoryFilter.coerce(T.WHERE)


def test_route_conditions(monkeypatch):
    """Outside its conditions the route is not taken: a filter passing fewer
    than 1 / FILTER_ANN_MAX_SCALE of the rows, a tenant below ``min_rows``."""
    from lazzaro_amd.engine import tenant_graph as TG
    monkeypatch.setattr(TG, "FILTER_SPARSE_MAX_ROWS", 0)
    gen = torch.Generator().manual_seed(1)
    X = T.grid_rows(T.N, gen)
    sal = torch.full((T.N,), 0.1)
    sal[: T.N // 8 - 1] = 0.9  # n / count just above 8
    g = T.make_graph("cpu", True, X, sal)
    g.store_search(X[:1], 5, "l2", where=T.WHERE)
    assert g.filtered_ann == 0 and g._ann is None
    monkeypatch.setattr(TG, "FILTER_ANN_MAX_SCALE", 9)
    g.store_search(X[:1], 5, "l2", where=T.WHERE)
    assert g.filtered_ann == 1
    g.ann_cfg["min_rows"] = T.N + 1
    g.store_search(X[:1], 5, "l2", where=T.WHERE)
    assert g.filtered_ann == 1


def test_public_switch_defaults_off(tmp_path):
    from lazzaro_amd.config import MemoryConfig
    from lazzaro_amd.core.vector_store import HBMStore

    class G:
        ann_cfg = None
    assert MemoryConfig().ivf_filtered is False
    for kw, want in (({}, False), ({"ivf_filtered": True}, True)):
        st = HBMStore(db_dir=str(tmp_path / f"s{int(want)}"), device="cpu", index="ivfpq", **kw)
        g = G()
        st.attach("u", g)
        assert g.ann_cfg["filtered"] is want and "filtered" not in st.ivf_params
    st = HBMStore(db_dir=str(tmp_path / "flat"), device="cpu", ivf_filtered=True)
    g = G()
    st.attach("u", g)
    assert g.ann_cfg is None  # index="flat": no index, whatever the switch says
