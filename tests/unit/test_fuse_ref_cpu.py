"""The multi-query fusion on the CPU tier: the fp64 oracle
(tests/kernels/_fuse_ref.py) against a brute-force loop, the torch formulation
``fuse_select_ref`` against the oracle -- ``rrf`` for equality, ``mean`` by the
two rules and the ``fuse_tol`` bound --, and the shares that make the GPU
cases decidable."""
import functools

import numpy as np
import pytest
import torch

from lazzaro_amd.core.fuse import QueryFusion
from lazzaro_amd.ops.fuse_ops import fuse_select, fuse_select_ref, fuse_tol, group_sizes
from tests.kernels import _fuse_ref as R


@functools.lru_cache(maxsize=None)
def _case(D, P, G, NG, independent=False):
    return R.recipe(D, P, G, NG, independent=independent)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _brute(offsets, pools, n, rrf_k, w):
    """RRF with no helper of the oracle: per group and row, scan every pool."""
    off = [int(o) for o in offsets]
    out = []
    for g in range(len(off) - 1):
        js = range(off[g], off[g + 1])
        cand = sorted({int(r) for j in js for r in pools[j] if 0 <= r < n})
        res = []
        for v in cand:
            acc, sup = 0.0, 0
            for j in js:
                live = [int(r) for r in pools[j] if 0 <= r < n]
                if v in live:
                    acc = acc + float(np.float32(w[j])) / (float(np.float32(rrf_k)) + (live.index(v) + 1))
                    sup += 1
            res.append((-float(np.float32(acc)), v, sup))
        out.append(sorted(res))
    return out


def test_oracle_equals_a_brute_force_loop():
    X, Q, off, pools = R.recipe(64, 16, 4, 16, n=512, seed=3)
    pools = R.mangle(pools, 512, seed=1)
    w = np.random.default_rng(0).uniform(0, 2, pools.shape[0]).astype(np.float32)
    w[5] = 0.0
    refs = R.fuse64(off, pools, 512, "rrf", 7.5, w)
    brute = _brute(off, pools, 512, 7.5, w)
    assert any(ref.rows.size == 0 or (ref.support > 1).any() for ref in refs)
    for ref, b in zip(refs, brute):
        o = ref.order
        assert [v for _, v, _ in b] == ref.rows[o].tolist()
        assert [s for _, _, s in b] == ref.support[o].tolist()
        assert np.array_equal(np.asarray([-s for s, _, _ in b], dtype=np.float32), ref.score[o])


def test_rank_rules():
    """A later occurrence is ignored for the score but counts as a slot; holes and rows >= n count as nothing."""
    n = 10
    assert R.ranks_of([3, -1, 3, 12, 5, 3, 7], n) == {3: 1, 5: 3, 7: 5}
    pools = np.asarray([[3, -1, 3, 12, 5, 3, 7], [7, 5, -1, -1, -1, -1, -1]], dtype=np.int64)
    for fn in (lambda: R.expected(R.fuse64([0, 2], pools, n, "rrf", 60.0), 6),
               lambda: [t.numpy() for t in fuse_select_ref(None, None, [0, 2], _t(pools), 6, "rrf", n=n)]):
        rows, scores, support, ncand = fn()
        assert ncand.tolist() == [3] and rows[0].tolist() == [5, 7, 3, -1, -1, -1]
        assert support[0].tolist() == [2, 2, 1, 0, 0, 0]
        want = [np.float32(1 / 63.0 + 1 / 62.0), np.float32(1 / 65.0 + 1 / 61.0), np.float32(1 / 61.0)]
        assert scores[0, :3].tolist() == want and np.isneginf(scores[0, 3:]).all()


@pytest.mark.parametrize("D,P,G,k,NG", R.FULL_ORDER_CASES, ids=[f"D{c[0]}-P{c[1]}-G{c[2]}-k{c[3]}" for c in
                                                             R.FULL_ORDER_CASES])
def test_full_order_cases(D, P, G, k, NG):
    X, Q, off, pools = _case(D, P, G, NG)
    n = X.shape[0]
    # rrf: equality
    refs = R.fuse64(off, pools, n, "rrf", 60.0)
    R.check_rrf(refs, k, *[t.numpy() for t in fuse_select_ref(None, None, off, _t(pools), k, "rrf", n=n)])
    # mean: the two rules, and the shares that make the case decide something
    refs = R.fuse64(off, pools, n, "mean", X=X, Q=Q)
    rows, scores, support, ncand = fuse_select(_t(X), _t(Q), off, _t(pools), k, "mean")  # (CPU tensors: the formulation)
    left = R.check_mean(refs, k, rows.numpy(), scores.numpy(), support.numpy(), ncand.numpy(), D, full_order=True)
    share = R.shared_share(refs)
    print(f"D={D} P={P} G={G} k={k} NG={NG}: {left} groups with a gap inside the first k + 1, "
          f"{share:.0%} of union rows in more than one pool, mean ncand {ncand.float().mean():.0f}")
    assert left <= R.CAP * NG
    assert share >= 0.25, "the pools barely overlap: the union rule is hardly exercised"
    assert share <= 0.80 and int(ncand.max()) > P, "the pools nearly coincide: the union rule is hardly exercised"


def test_rrf_ties_occur():
    """Equal fp32 RRF scores inside the first k + 1 -- the tie rule decides rows there."""
    tied = 0
    for D, P, G, k, NG in R.FULL_ORDER_CASES[:4]:
        X, Q, off, pools = _case(D, P, G, NG)
        tied += len(R.rrf_tie_groups(R.fuse64(off, pools, X.shape[0], "rrf", 60.0), k))
    assert tied >= 10


@pytest.mark.parametrize("D,P,G,k,NG,independent", R.WIDE_CASES, ids=["perturbed", "independent"])
def test_wide_cases(D, P, G, k, NG, independent):
    X, Q, off, pools = _case(D, P, G, NG, independent)
    n = X.shape[0]
    refs = R.fuse64(off, pools, n, "rrf", 60.0)
    R.check_rrf(refs, k, *[t.numpy() for t in fuse_select_ref(None, None, off, _t(pools), k, "rrf", n=n)])
    refs = R.fuse64(off, pools, n, "mean", X=X, Q=Q)
    out = [t.numpy() for t in fuse_select_ref(_t(X), _t(Q), off, _t(pools), k, "mean")]
    left = R.check_mean(refs, k, *out, D)
    print(f"independent={independent}: {left} of {NG} groups with a gap inside the first {k + 1}, "
          f"mean ncand {out[3].mean():.0f}, max {out[3].max()}")
    if independent:
        assert out[3].mean() > 800  # nearly disjoint pools: the table close to full


def test_mixed_groups_weights_and_edges():
    X, Q, _, pools = _case(64, 16, 4, 128)
    n = X.shape[0]
    off = [0, 1, 3, 6, 22]
    M = 22
    pools = R.mangle(pools[:M], n, seed=2)
    pools[3:6] = -1  # an all-empty group
    rng = np.random.default_rng(5)
    w = rng.uniform(0.0, 3.0, M).astype(np.float32)
    w[[0, 7, 8]] = 0.0
    for k in (1, 10, 64):
        refs = R.fuse64(off, pools, n, "rrf", 12.25, w)
        out = fuse_select_ref(None, None, off, _t(pools), k, {"mode": "rrf", "rrf_k": 12.25}, w, n=n)
        R.check_rrf(refs, k, *[t.numpy() for t in out])
        assert refs[2].rows.size == 0 and int(out[3][2]) == 0 and (out[0][2] == -1).all()
        refs = R.fuse64(off, pools, n, "mean", weights=np.where(w == 0, 1, w), X=X, Q=Q[:M])
        out = fuse_select_ref(_t(X), _t(Q[:M]), off, _t(pools), k, "mean", np.where(w == 0, 1, w))
        R.check_mean(refs, k, *[t.numpy() for t in out], 64)
    # a singleton group under rrf returns its pool in pool order, without holes and repeats
    rows = fuse_select_ref(None, None, off, _t(pools), 16, "rrf", n=n)[0][0].tolist()
    seen = []
    for r in pools[0].tolist():
        if 0 <= r < n and r not in seen:
            seen.append(r)
    assert [r for r in rows if r >= 0] == seen


def test_fuse_tol_bounds_the_formulation():
    """|score32 - score64| <= fuse_tol over every candidate of every group, on data made to stress it: D = 2048."""
    for D, P, G, NG in ((2048, 16, 8, 8), (100, 16, 16, 8)):
        X, Q, off, pools = R.recipe(D, P, G, NG, n=512, seed=9)
        w = np.random.default_rng(1).uniform(0.1, 2.0, G * NG).astype(np.float32)
        refs = R.fuse64(off, pools, 512, "mean", weights=w, X=X, Q=Q)
        rows, scores, _, _ = fuse_select_ref(_t(X), _t(Q), off, _t(pools), 64, "mean", w)
        worst = 0.0
        for g, ref in enumerate(refs):
            got = rows[g].numpy()
            live = got >= 0
            pos = np.searchsorted(ref.rows, got[live])
            worst = max(worst, float(np.abs(scores[g].numpy()[live].astype(np.float64) - ref.score[pos]).max()))
        print(f"D={D} G={G}: worst |score32 - score64| = {worst / 2 ** -24:.2f} units of 2^-24, "
              f"tol {fuse_tol(D, G) / 2 ** -24:.0f}")
        assert worst <= fuse_tol(D, G)
    assert fuse_tol(768, 4) == (2 * (4 * 12 + 4) + 8 + 4 + 2) * 2.0 ** -24


def test_a_zero_query_scores_zero():
    X, Q, off, pools = R.recipe(64, 16, 3, 4, n=256, seed=2)
    Q = Q.copy()
    Q[1] = 0.0
    refs = R.fuse64(off, pools, 256, "mean", X=X, Q=Q)
    out = fuse_select_ref(_t(X), _t(Q), off, _t(pools), 10, "mean")
    R.check_mean(refs, 10, *[t.numpy() for t in out], 64)
    assert np.isfinite(out[1].numpy()).all()


def test_settings_and_validation():
    assert QueryFusion.coerce("mean") == QueryFusion(mode="mean") and QueryFusion.coerce(None) is None
    assert QueryFusion.coerce({"pool": 32.0, "weights": [1, 2]}) == QueryFusion(pool=32, weights=(1.0, 2.0))
    fu = QueryFusion()
    assert (fu.mode, fu.pool, fu.rrf_k, fu.weights) == ("rrf", 16, 60.0, None)
    for bad in ("max", {"mode": "rrf", "k": 3}, {"pool": 0}, {"pool": 65}, {"pool": 2.5}, {"rrf_k": 0}, {"rrf_k": -1.0},
                {"rrf_k": float("inf")}, {"weights": [1.0, -1.0]}, {"weights": [float("nan")]}, {"weights": "12"},
                {"pool": True}, 3):
        with pytest.raises(ValueError):
            QueryFusion.coerce(bad)
    for limit, sizes in ((0, [2]), (65, [2]), (5, [0]), (5, [2, 17]), (True, [2]), (2.5, [2])):
        with pytest.raises(ValueError):
            fu.check(limit, sizes)
    fu.check(64, [1, 16])
    with pytest.raises(ValueError):
        QueryFusion(weights=(1.0, 2.0)).check(5, [2, 3])
    assert QueryFusion(weights=(1.0, 2.0)).group_weights([2, 2]) == [1.0, 2.0, 1.0, 2.0]
    assert fu.group_weights([1, 2], [[3], [0, 1]]) == [3.0, 0.0, 1.0]
    for sizes, w in (([2], [[1.0]]), ([2], [[1.0, 2.0], [1.0]]), ([1], [[-1.0]])):
        with pytest.raises(ValueError):
            fu.group_weights(sizes, w)
    with pytest.raises(ValueError):
        QueryFusion(mode="mean").group_weights([2], [[0.0, 0.0]])
    assert fu.group_weights([2], [[0.0, 0.0]]) == [0.0, 0.0]  # (rrf: every score 0, the rows by number)
    assert group_sizes([0, 1, 3], 3) == [1, 2]
    for off, M in (([1, 3], 3), ([0, 3, 2], 2), ([0, 2], 3), ([], 0)):
        with pytest.raises(ValueError):
            group_sizes(off, M)
    pools = torch.zeros((3, 4), dtype=torch.long)
    with pytest.raises(ValueError):
        fuse_select_ref(None, None, [0, 3], pools, 5, "mean", n=8)  # mean needs rows and queries
    with pytest.raises(ValueError):
        fuse_select_ref(None, None, [0, 3], torch.zeros((3, 65), dtype=torch.long), 5, "rrf", n=8)
    with pytest.raises(ValueError):
        fuse_select_ref(None, None, [0, 3], pools, 5, "rrf", [1.0, 2.0], n=8)
