"""Multi-query fusion on the device (csrc/kernels/fuse.hip) against the fp64
oracle tests/kernels/_fuse_ref.py: ``rrf`` bit for bit -- rows, scores,
support and ``ncand`` --, ``mean`` under the oracle's two rules,
``store_search_fused`` end to end, and the batch against the per-group call."""
import functools

import numpy as np
import pytest
import torch

from lazzaro_amd.ops.fuse_ops import fuse_select
from tests.kernels import _fuse_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _case(D, P, G, NG, independent=False):
    return R.recipe(D, P, G, NG, independent=independent)


@functools.lru_cache(maxsize=None)
def _rrf_refs(D, P, G, NG, independent=False):
    X, _, off, pools = _case(D, P, G, NG, independent)
    return R.fuse64(off, pools, X.shape[0], "rrf", 60.0)


@functools.lru_cache(maxsize=None)
def _mean_refs(D, P, G, NG, independent=False):
    X, Q, off, pools = _case(D, P, G, NG, independent)
    return R.fuse64(off, pools, X.shape[0], "mean", X=X, Q=Q)


def _np(out):
    return [t.cpu().numpy() for t in out]


_ids5 = [f"D{c[0]}-P{c[1]}-G{c[2]}-k{c[3]}" for c in R.FULL_ORDER_CASES]


# ---- rrf: equality
@pytest.mark.parametrize("D,P,G,k,NG", R.FULL_ORDER_CASES, ids=_ids5)
def test_rrf_equals_the_oracle(D, P, G, k, NG):
    X, _, off, pools = _case(D, P, G, NG)
    out = fuse_select(None, None, off, _dev(pools), k, "rrf", n=X.shape[0])
    assert out[0].dtype == torch.long and out[1].dtype == torch.float32 and out[2].dtype == out[3].dtype == torch.int32
    R.check_rrf(_rrf_refs(D, P, G, NG), k, *_np(out))


@pytest.mark.parametrize("D,P,G,k,NG,independent", R.WIDE_CASES, ids=["perturbed", "independent"])
def test_rrf_k64_over_sixteen_pools(D, P, G, k, NG, independent):
    X, _, off, pools = _case(D, P, G, NG, independent)
    out = fuse_select(None, None, off, _dev(pools), k, "rrf", n=X.shape[0])
    R.check_rrf(_rrf_refs(D, P, G, NG, independent), k, *_np(out))


def test_rrf_mixed_groups_holes_repeats_and_weights():
    """Group sizes 1, 2, 3 and 16 in one launch; -1 holes mid-list, rows >= n,
    a row repeated inside a pool, an all-empty pool and an all-empty group;
    unequal weights with zeros among them; an ``rrf_k`` that is no integer;
    k = 1, k = 64 and k above the union size."""
    X, _, _, pools = _case(64, 16, 4, 128)
    n = X.shape[0]
    off = [0, 1, 3, 6, 22]
    pools = R.mangle(pools[:22], n, seed=2)
    pools[3:6] = -1
    w = np.random.default_rng(5).uniform(0.0, 3.0, 22).astype(np.float32)
    w[[0, 7, 8]] = 0.0
    assert (pools[11] == -1).all() and (pools >= n).any() and (pools[6:, 4] == -1).any()
    for k in (1, 10, 64):
        for weights in (None, w):
            refs = R.fuse64(off, pools, n, "rrf", 12.25, weights)
            out = _np(fuse_select(None, None, off, _dev(pools), k, {"rrf_k": 12.25}, weights, n=n))
            R.check_rrf(refs, k, *out)
        assert out[3].tolist()[2] == 0 and (out[0][2] == -1).all() and (out[2][2] == 0).all()
        assert k < 64 or ((out[0][:3, -1] == -1).all() and out[0][3, -1] >= 0)  # (unions of 1 .. 3 pools of 16: padding)
    assert max(ref.support.max() for ref in refs if ref.rows.size) > 2


def test_rrf_one_slot_pools_and_the_full_table():
    # P = 1
    X, _, off, pools = _case(64, 16, 4, 128)
    n = X.shape[0]
    p1 = np.ascontiguousarray(pools[:, :1])
    R.check_rrf(R.fuse64(off, p1, n, "rrf", 60.0), 4, *_np(fuse_select(None, None, off, _dev(p1), 4, "rrf", n=n)))
    # 16 disjoint pools of 64: exactly 1,024 candidates, the full table; a second group beside it
    rng = np.random.default_rng(3)
    full = rng.permutation(4096)[:1024].reshape(16, 64).astype(np.int64)
    both = np.concatenate([full, full[::-1]])
    w = rng.uniform(0.5, 1.5, 32).astype(np.float32)
    for k in (64, 7):
        refs = R.fuse64([0, 16, 32], both, 4096, "rrf", 60.0, w)
        out = _np(fuse_select(None, None, [0, 16, 32], _dev(both), k, "rrf", w, n=4096))
        R.check_rrf(refs, k, *out)
        assert out[3].tolist() == [1024, 1024]


# ---- the shared tournament and row table (csrc/include/lzk_topk64.h, lzk_rowset.h) at their smallest shapes
@pytest.mark.parametrize("mode", ["rrf", "mean"])
def test_three_blocks_one_block_ties_and_colliding_rows(mode):
    """n = 1,024 (the first 256 rows collide nowhere in the hash), D = 64, k =
    64. Group 0: three disjoint pools of 64, so 192
    candidates in three 64-entry blocks -- the third has no partner in the
    tournament's first round. Group 1: one pool of 16 with a row listed twice:
    15 candidates in a single block. Rows a < b open pools 0 and 1 and collide
    in the table's 11-bit hash; rows u < v hold one embedding, the best for
    every sub-query, so ``mean`` ties them bit for bit; under ``rrf`` the
    three pools tie rank by rank. Ties go to the lower row."""
    n, D, k = 1024, 64, 64
    rng = np.random.default_rng(11)
    h = ((np.arange(n, dtype=np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(21)
    a, b = next((int(np.flatnonzero(h[:j] == h[j])[0]), j) for j in range(n) if (h[:j] == h[j]).any())
    u, v = [r for r in range(n) if r not in (a, b)][:2]
    rest = rng.permutation([r for r in range(n) if r not in (a, b, u, v)])
    p3 = np.concatenate([[a, u], rest[:62], [b, v], rest[62:124], rest[124:188]]).reshape(3, 64).astype(np.int64)
    p1 = np.full((1, 64), -1, dtype=np.int64)
    p1[0, :16] = np.concatenate([[b, a], rest[188:201], [b]])
    pools = np.concatenate([p3, p1])
    off = [0, 3, 4]
    base = rng.standard_normal(D)
    X = rng.standard_normal((n, D))
    X[u] = X[v] = 3.0 * base
    X = (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)
    Q = (base + 0.3 * rng.standard_normal((4, D))).astype(np.float32)
    assert np.unique(p3).size == 192 and np.array_equal(X[u], X[v])
    if mode == "rrf":
        out = _np(fuse_select(None, None, off, _dev(pools), k, "rrf", n=n))
        R.check_rrf(R.fuse64(off, pools, n, "rrf", 60.0), k, *out)
        assert out[0][0, :6].tolist() == sorted([a, b, int(p3[2, 0])]) + sorted([u, v, int(p3[2, 1])])
    else:
        out = _np(fuse_select(_dev(X), _dev(Q), off, _dev(pools), k, "mean"))
        R.check_mean(R.fuse64(off, pools, n, "mean", X=X, Q=Q), k, *out, D)
        assert out[0][0, :2].tolist() == [u, v] and out[1][0, 0].view(np.uint32) == out[1][0, 1].view(np.uint32)
    rows = out[0]
    assert out[3].tolist() == [192, 15] and (rows[1, 15:] == -1).all()
    # colliding rows: one entry each (group 1 returns all it has; group 0 ranks both first under rrf)
    assert all((rows[g] == r).sum() == 1 for g in ((0, 1) if mode == "rrf" else (1,)) for r in (a, b))


# ---- mean: the two rules
@pytest.mark.parametrize("D,P,G,k,NG", R.FULL_ORDER_CASES, ids=_ids5)
def test_mean_holds_the_two_rules(D, P, G, k, NG):
    """D = 64 and 768 take the vector loads, D = 100 the scalar ones, D = 2048 fills 16 KiB of LDS a query."""
    X, Q, off, pools = _case(D, P, G, NG)
    out = _np(fuse_select(_dev(X), _dev(Q), off, _dev(pools), k, "mean"))
    left = R.check_mean(_mean_refs(D, P, G, NG), k, *out, D, full_order=True)
    print(f"D={D} P={P} G={G} k={k}: {left} of {NG} groups left out of the exact-order rule")


@pytest.mark.parametrize("D,P,G,k,NG,independent", R.WIDE_CASES, ids=["perturbed", "independent"])
def test_mean_k64_over_sixteen_pools(D, P, G, k, NG, independent):
    X, Q, off, pools = _case(D, P, G, NG, independent)
    out = _np(fuse_select(_dev(X), _dev(Q), off, _dev(pools), k, "mean"))
    left = R.check_mean(_mean_refs(D, P, G, NG, independent), k, *out, D)
    print(f"independent={independent}: {left} of {NG} groups with a gap inside the first {k + 1}, "
          f"ncand mean {out[3].mean():.0f} max {out[3].max()}")
    if independent:
        assert out[3].mean() > 800


def test_mean_strided_rows_misaligned_rows_weights_and_a_zero_query():
    X, Q, _, pools = _case(64, 16, 4, 128)
    n, D = X.shape
    off = [0, 1, 3, 6, 22]
    M = 22
    pools = R.mangle(pools[:M], n, seed=4)
    Q = Q[:M].copy()
    Q[4] = 0.0  # cosine 0 with every row
    w = np.random.default_rng(6).uniform(0.0, 3.0, M).astype(np.float32)
    w[[1, 7]] = 0.0  # (no group's weights sum to 0)
    refs = R.fuse64(off, pools, n, "mean", weights=w, X=X, Q=Q)
    wide = torch.zeros((n, D + 8), device=DEV)
    wide[:, :D] = _dev(X)
    flat = torch.zeros(n * D + 1, device=DEV)
    flat[1:] = _dev(X).reshape(-1)
    shifted = flat[1:].view(n, D)
    assert shifted.data_ptr() % 16 == 4 and wide[:, :D].stride(0) == D + 8
    for Xd in (_dev(X), wide[:, :D], shifted):
        for k in (10, 64):
            out = _np(fuse_select(Xd, _dev(Q), off, _dev(pools), k, "mean", w))
            R.check_mean(refs, k, *out, D)
    assert np.isfinite(out[1][out[0] >= 0]).all()


def test_mean_at_the_lds_cap():
    """8 sub-queries of 2,048 dimensions fill the 64 KiB of staged queries; 9 raise."""
    X, Q, off, pools = R.recipe(2048, 16, 8, 4, n=512, seed=7)
    refs = R.fuse64(off, pools, 512, "mean", X=X, Q=Q)
    out = _np(fuse_select(_dev(X), _dev(Q), off, _dev(pools), 16, "mean"))
    R.check_mean(refs, 16, *out, 2048)
    X9, Q9, off9, pools9 = R.recipe(2048, 16, 9, 1, n=512, seed=7)
    with pytest.raises(ValueError):
        fuse_select(_dev(X9), _dev(Q9), off9, _dev(pools9), 16, "mean")
    # rrf reads no query: 9 and 16 sub-queries are fine whatever the width
    R.check_rrf(R.fuse64(off9, pools9, 512, "rrf", 60.0), 16,
                *_np(fuse_select(None, None, off9, _dev(pools9), 16, "rrf", n=512)))


# ---- end to end
def _tenant():
    from lazzaro_amd.engine.tenant_graph import TenantGraph
    from tests.kernels._lex_ref import e2e_inputs
    X, texts, sal, _, _ = e2e_inputs()
    n, D = X.shape
    g = TenantGraph(device=DEV, dim=D, capacity=n + 8)
    g.add_nodes([f"m{i}" for i in range(n)], texts, torch.from_numpy(X), shard=g.shard_id("w"),
                sal=torch.from_numpy(sal), stored=True)
    return g, X, sal


@pytest.mark.parametrize("mode", ["rrf", "mean"])
def test_store_search_fused_end_to_end(mode):
    from lazzaro_amd.core.boost import MemoryBoost
    g, X, sal = _tenant()
    n, D = X.shape
    rng = np.random.default_rng(8)
    off = np.asarray([0, 1, 4, 8, 24])
    base = X[rng.integers(0, n, 4)]
    Q = np.concatenate([np.repeat(base[i:i + 1], c, 0) for i, c in enumerate(np.diff(off))])
    Q = (Q + 0.4 * rng.standard_normal(Q.shape) / np.sqrt(D)).astype(np.float32)
    Qd = _dev(Q)
    boost = MemoryBoost.coerce(1.5).at(1000.0)
    for kw in ({}, {"where": {"min_salience": 0.5}}, {"where": {"min_salience": 0.5}, "boost": boost}):
        for metric in ("l2", "cosine"):
            _, pools = g.store_search(Qd, 16, metric, node_rows=True, **kw)
            s, r, sup = g.store_search_fused(Qd, off, 10, metric, mode, **kw)
            refs = R.fuse64(off, pools.cpu().numpy(), n, mode, 60.0, X=X, Q=Q)
            nc = np.asarray([ref.rows.size for ref in refs])
            if mode == "rrf":
                R.check_rrf(refs, 10, r.cpu().numpy(), s.cpu().numpy(), sup.cpu().numpy(), nc)
            else:
                R.check_mean(refs, 10, r.cpu().numpy(), s.cpu().numpy(), sup.cpu().numpy(), nc, D)
            rows = r.cpu().numpy()
            assert (rows >= 0).all()
            if kw:
                assert (sal[rows] >= 0.5).all()  # a row the filter rejects never appears
            assert g.search_ids_fused(Qd, off, 10, metric, mode, **kw) == [[f"m{x}" for x in row] for row in rows]
    assert g.fused_searches == 12 and g.fused_groups == 48


def test_memory_system_batch_equals_the_per_group_call(tmp_path):
    from lazzaro_amd.core.memory_system import MemorySystem
    from lazzaro_amd.core.providers import HashEmbedder, LocalLLM
    from tests.kernels._lex_ref import e2e_inputs
    _, texts, sal, _, _ = e2e_inputs()
    ms = MemorySystem(llm_provider=LocalLLM(), embedding_provider=HashEmbedder(dim=64), enable_async=False,
                      load_from_disk=False, db_dir=str(tmp_path / "db"), device=DEV)
    try:
        g = ms.graph
        emb = np.asarray([ms._get_embedding(t) for t in texts], dtype=np.float32)
        g.add_nodes([f"m{i}" for i in range(len(texts))], texts, torch.from_numpy(emb), shard=g.shard_id("w"),
                    sal=torch.from_numpy(sal), stored=True)
        groups = [[texts[5], texts[17] + " garden", texts[40]], [texts[9]], texts[100:108]]
        for kw in (dict(fuse="rrf"), dict(fuse="mean"), dict(fuse="rrf", where={"min_salience": 0.3}),
                   dict(fuse={"mode": "mean", "pool": 8}, boost=0.5)):
            batch = ms.search_memories_fused_batch(groups, limit=6, **kw)
            single = [ms.search_memories_fused(grp, limit=6, **kw) for grp in groups]
            assert [[n.id for n in b] for b in batch] == [[n.id for n in s] for s in single]
            assert all(len(b) == 6 for b in batch)
        assert [n.id for n in ms.search_memories_fused([texts[9]], limit=6)] == \
            [n.id for n in ms.search_memories(texts[9], limit=6)]
        e = ms.get_stats()["engine"]
        assert e["fused_searches"] == 17 and e["fused_groups"] == 25
    finally:
        ms.close()
