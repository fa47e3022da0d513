"""The fp64 MMR oracle (tests/kernels/_mmr_ref.py) against a brute-force
enumeration, the share of queries the oracle's exact-pick rule leaves out at
the shapes the GPU tests use, and the torch formulation ``mmr_select_ref``
against the oracle."""
import numpy as np
import pytest
import torch

from lazzaro_amd.ops.mmr_ops import MMR_SUM_DEPTH, mmr_select, mmr_select_ref, mmr_tol
from tests.kernels._mmr_ref import CAP, check_against_ref, check_rule1, mmr_greedy64, recipe

SHAPES = [(768, 16, 10), (768, 64, 10), (1024, 64, 16), (20, 16, 5), (30, 17, 17), (1536, 16, 5)]


def _ref(X, Q, cand, k, delta):
    p, o = mmr_select_ref(torch.from_numpy(X), torch.from_numpy(Q), torch.from_numpy(cand), k, delta)
    return p.numpy(), o.numpy()


def _cos(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    na, nb = np.sqrt(a @ a), np.sqrt(b @ b)
    return float(a @ b / (na * nb)) if na > 0 and nb > 0 else 0.0


def test_summation_depth_covers_both_paths():
    for D in (1, 4, 20, 30, 64, 65, 768, 1024, 1536):
        lane_f4 = 4 * -(-(-(-D // 4)) // 16)  # fmas of the busiest lane, float4 path
        lane_sc = -(-D // 16)                 # scalar path
        assert MMR_SUM_DEPTH(D) >= max(lane_f4, lane_sc) + 4
    assert mmr_tol(768) == (2 * MMR_SUM_DEPTH(768) + 8) * 2.0 ** -24 and MMR_SUM_DEPTH(768) == 52


def test_oracle_equals_brute_force_on_a_tiny_pool():
    rng = np.random.default_rng(5)
    n, D, F, k = 12, 7, 5, 5
    X = rng.standard_normal((n, D)).astype(np.float32)
    Q = rng.standard_normal((6, D)).astype(np.float32)
    cand = np.stack([rng.permutation(n)[:F] for _ in range(6)]).astype(np.int64)
    cand[2, 3] = -1
    cand[4, :] = [3, -1, 40, -1, 9]  # (40: out of range)
    for delta in (0.0, 0.3, 0.7, 1.0):
        pick, obj, gap = mmr_greedy64(X, Q, cand, k, delta)
        d = float(np.float32(delta))
        for m in range(6):
            left = [f for f in range(F) if 0 <= cand[m, f] < n]
            S, want, wobj, wgap = [], [], [], np.inf
            while left and len(want) < k:
                o = {f: (1.0 - d) * _cos(Q[m], X[cand[m, f]])
                     - d * (max(_cos(X[cand[m, f]], X[cand[m, s]]) for s in S) if S else 0.0) for f in left}
                best = max(o.values())
                f = min((f for f in left if o[f] == best), key=lambda f: cand[m, f])
                if len(left) > 1:
                    wgap = min(wgap, best - max(v for g, v in o.items() if g != f))
                want.append(f), wobj.append(best), S.append(f), left.remove(f)
            pad = k - len(want)
            assert pick[m].tolist() == want + [-1] * pad
            np.testing.assert_allclose(obj[m, :len(want)], wobj, rtol=0, atol=1e-14)
            assert np.isneginf(obj[m, len(want):]).all()
            assert gap[m] == pytest.approx(wgap, abs=1e-14) if np.isfinite(wgap) else np.isinf(gap[m])


@pytest.mark.parametrize("D,F,k", SHAPES, ids=[f"D{d}-F{f}-k{k}" for d, f, k in SHAPES])
def test_cap_holds_for_the_recipe_and_the_torch_ref_passes(D, F, k):
    X, Q, cand = recipe(D, F)
    assert np.abs(np.linalg.norm(X.astype(np.float64), axis=1) - 1).max() < 1e-6 and (np.abs(X) > 0).mean() > 0.99
    for delta in (0.3, 0.7):
        gap = mmr_greedy64(X, Q, cand, k, delta)[2]
        left_out = int((gap <= 2 * mmr_tol(D)).sum())
        print(f"D={D} F={F} k={k} delta={delta}: {left_out} of {len(gap)} left out of the exact-pick rule")
        assert left_out <= CAP * len(gap)
        pick, obj = _ref(X, Q, cand, k, delta)
        assert check_against_ref(X, Q, cand, k, delta, pick, obj) == left_out


def test_cpu_tensors_take_the_torch_formulation():
    X, Q, cand = recipe(20, 16, M=8, n=256)
    a = mmr_select(torch.from_numpy(X), torch.from_numpy(Q), torch.from_numpy(cand), 5, 0.4)
    b = _ref(X, Q, cand, 5, 0.4)
    assert a[0].dtype == torch.int32 and a[1].dtype == torch.float32
    assert np.array_equal(a[0].numpy(), b[0]) and np.array_equal(a[1].numpy(), b[1])


def test_delta_zero_is_descending_cosine_and_delta_one_ignores_relevance():
    X, Q, cand = recipe(30, 17, M=16, n=512, seed=3)
    X = X * np.linspace(0.5, 2.0, len(X), dtype=np.float32)[:, None]  # (cosine, not the dot, must decide)
    F = cand.shape[1]
    pick, obj = _ref(X, Q, cand, F, 0.0)
    check_against_ref(X, Q, cand, F, 0.0, pick, obj)
    for m in range(len(Q)):
        c = np.array([_cos(Q[m], X[r]) for r in cand[m]])
        assert pick[m].tolist() == np.argsort(-c, kind="stable").tolist()
        np.testing.assert_allclose(obj[m], c[pick[m]], rtol=0, atol=mmr_tol(30))
    # delta = 1: the first pick is the lowest row (every objective is 0); from then on
    # the objective is minus the largest cosine to the picks, whatever the query
    p1, o1 = _ref(X, Q, cand, 6, 1.0)
    p2, o2 = _ref(X, np.roll(Q, 1, axis=0), cand, 6, 1.0)
    check_against_ref(X, Q, cand, 6, 1.0, p1, o1, gap_from=1)  # (step 0 ties everywhere, exactly)
    assert np.array_equal(p1, p2) and np.array_equal(o1, o2)
    assert (p1[:, 0] == cand.argmin(1)).all() and (o1[:, 0] == 0).all()


def test_zero_query_zero_row_and_ties():
    D = 8
    X = np.zeros((6, D), dtype=np.float32)
    X[0, 0] = 1.0
    X[1, 1] = 2.0
    X[2, 1] = 2.0          # row 2 == row 1
    X[4, :2] = (3.0, 4.0)  # row 3 and row 5 stay zero
    cand = np.array([[5, 4, 2, 1, 0, 3]], dtype=np.int64)
    # a zero query: every relevance is 0, so the lowest row goes first
    pick, obj = _ref(X, np.zeros((1, D), np.float32), cand, 6, 0.5)
    check_rule1(X, np.zeros((1, D), np.float32), cand, 6, 0.5, pick, obj)  # (ties by construction)
    assert cand[0, pick[0, 0]] == 0 and obj[0, 0] == 0.0
    # a zero row has cosine 0 to the query and to every pick
    q = np.zeros((1, D), np.float32)
    q[0, 1] = 1.0
    pick, obj = _ref(X, q, cand, 6, 0.5)
    check_rule1(X, q, cand, 6, 0.5, pick, obj)
    rows = cand[0, pick[0]].tolist()
    assert rows[0] == 1  # rows 1 and 2 tie at cosine 1: the lower row
    # then: row 4 (0.5 * 0.8 - 0.5 * 0.8 = 0), rows 0, 3, 5 (0 - 0) all tie at 0 -> row 0; row 2 is at 0.5 - 0.5 = 0 too
    assert rows[1] == 0 and obj[0, 1] == 0.0
    assert sorted(rows) == [0, 1, 2, 3, 4, 5]
    for bad in (dict(k=7), dict(k=0), dict(diversity=1.5), dict(diversity=-0.1)):
        kw = dict(k=3, diversity=0.5)
        kw.update(bad)
        with pytest.raises(ValueError):
            mmr_select_ref(torch.from_numpy(X), torch.from_numpy(q), torch.from_numpy(cand), **kw)
    with pytest.raises(ValueError):
        mmr_select_ref(torch.from_numpy(X), torch.zeros(1, D), torch.zeros((1, 65), dtype=torch.long), 3, 0.5)
