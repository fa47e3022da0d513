"""fp64 oracle of the diversity-aware (MMR) selection and the two rules a
result is held to (ops/mmr_ops.py, csrc/kernels/mmr.hip).

The oracle takes the fp32 inputs cast to float64, computes every norm and
cosine in float64 and breaks ties to the lower graph row. ``check_against_ref``
holds a result to

1. every query, no exceptions: replaying the result's own prefix in fp64, each
   pick's fp64 objective is within ``2 tol(D)`` of that step's maximum and the
   returned objective within ``tol(D)`` of it; picks are distinct, valid and
   never an empty slot; padding appears exactly when the pool runs out;
2. queries whose fp64 gap between the best and the second-best objective
   exceeds ``2 tol(D)`` at every step: the picks equal the fp64 greedy picks.
   At most ``CAP`` (10 %) of the queries may fall outside this rule; the
   helper asserts that itself. Inputs that tie by construction (a zero query,
   identical rows) sit in a batch large enough to stay under it, or are held
   to rule 1 alone (``check_rule1``) with their picks asserted by the test.

``tol(D)`` is ``mmr_ops.mmr_tol``: the kernel's stated summation depth.
"""
import numpy as np

from lazzaro_amd.ops.mmr_ops import mmr_tol

CAP = 0.10


def cos64(X, Q, cand):
    """(valid [M, F], rel [M, F], sim [M, F, F]) in float64; empty slots read
    as zero rows. cos is 0 when either norm is 0."""
    X = np.asarray(X)
    Q = np.asarray(Q, dtype=np.float64)
    cand = np.asarray(cand, dtype=np.int64)
    n = X.shape[0]
    valid = (cand >= 0) & (cand < n)
    Xc = np.where(valid[:, :, None], X[np.clip(cand, 0, max(n - 1, 0))].astype(np.float64), 0.0) if n else \
        np.zeros(cand.shape + (Q.shape[1],))
    nrm = np.sqrt((Xc * Xc).sum(2))
    qn = np.sqrt((Q * Q).sum(1))

    def div(dot, den):
        ok = den > 0
        return np.where(ok, dot / np.where(ok, den, 1.0), 0.0)

    rel = div(np.matmul(Xc, Q[:, :, None])[:, :, 0], qn[:, None] * nrm)
    sim = div(np.matmul(Xc, Xc.transpose(0, 2, 1)), nrm[:, :, None] * nrm[:, None, :])
    return valid, rel, sim


def _weights(delta):
    d = float(np.float32(delta))  # (the kernel is handed the fp32 value)
    return 1.0 - d, d


def _objective(rel, sim, alive, picked, w, d):
    """fp64 objective of every slot of one query given the picked slots
    (-inf where not alive)."""
    red = sim[:, picked].max(1) if picked else 0.0
    return np.where(alive, w * rel - d * red, -np.inf)


def _argmax_low_row(o, rows):
    """The slot of the maximum; among equal objectives the lower graph row
    (the lower slot if a row is listed twice)."""
    c = np.flatnonzero(o == o.max())
    return int(c[np.argsort(rows[c], kind="stable")[0]])


def mmr_greedy64(X, Q, cand, k, delta, pre=None, gap_from=0):
    """fp64 greedy picks. Returns (pick int64 [M, k] pool slots, -1 padding;
    obj float64 [M, k], -inf padding; gap float64 [M]: the smallest gap
    between the best and the second-best objective over the steps taken,
    +inf where no step had two candidates). ``gap_from``: the first step
    whose gap counts -- 1 for delta = 1, where every objective of step 0 is
    exactly 0 in any precision and the row rule alone decides."""
    cand = np.asarray(cand, dtype=np.int64)
    valid, rel, sim = pre if pre is not None else cos64(X, Q, cand)
    M, F = cand.shape
    w, d = _weights(delta)
    pick = np.full((M, k), -1, dtype=np.int64)
    obj = np.full((M, k), -np.inf)
    gap = np.full(M, np.inf)
    for m in range(M):
        alive = valid[m].copy()
        picked = []
        for t in range(k):
            if not alive.any():
                break
            o = _objective(rel[m], sim[m], alive, picked, w, d)
            s = _argmax_low_row(o, cand[m])
            if alive.sum() > 1 and t >= gap_from:
                rest = o.copy()
                rest[s] = -np.inf
                gap[m] = min(gap[m], o[s] - rest.max())
            pick[m, t], obj[m, t] = s, o[s]
            alive[s] = False
            picked.append(s)
    return pick, obj, gap


def check_rule1(X, Q, cand, k, delta, pick, obj, pre=None):
    """Rule 1 of the module docstring, for every query of (pick, obj) -- int
    [M, k] pool slots and fp32 [M, k] objectives."""
    X = np.asarray(X)
    cand = np.asarray(cand, dtype=np.int64)
    pick = np.asarray(pick, dtype=np.int64)
    obj = np.asarray(obj, dtype=np.float64)
    M, F = cand.shape
    tol = mmr_tol(X.shape[1])
    assert pick.shape == (M, k) and obj.shape == (M, k)
    valid, rel, sim = pre if pre is not None else cos64(X, Q, cand)
    w, d = _weights(delta)
    for m in range(M):
        alive = valid[m].copy()
        picked = []
        for t in range(k):
            s = int(pick[m, t])
            if not alive.any():
                assert (pick[m, t:] == -1).all() and np.isneginf(obj[m, t:]).all(), (m, t, pick[m], obj[m])
                break
            assert 0 <= s < F, f"query {m} step {t}: padding while {int(alive.sum())} candidates remain"
            assert alive[s], f"query {m} step {t}: slot {s} is empty or already picked"
            o = _objective(rel[m], sim[m], alive, picked, w, d)
            assert o[s] >= o.max() - 2 * tol, f"query {m} step {t}: picked {o[s]!r}, best {o.max()!r}, tol {tol!r}"
            assert abs(obj[m, t] - o[s]) <= tol, f"query {m} step {t}: obj {obj[m, t]!r} vs fp64 {o[s]!r}, tol {tol!r}"
            alive[s] = False
            picked.append(s)


def check_against_ref(X, Q, cand, k, delta, pick, obj, gap_from=0):
    """Hold (pick, obj) to both rules of the module docstring. Returns the
    number of queries left out of rule 2 (asserted <= CAP of them).
    ``gap_from``: see :func:`mmr_greedy64`."""
    cand = np.asarray(cand, dtype=np.int64)
    pick = np.asarray(pick, dtype=np.int64)
    M = cand.shape[0]
    tol = mmr_tol(np.asarray(X).shape[1])
    pre = cos64(X, Q, cand)
    check_rule1(X, Q, cand, k, delta, pick, obj, pre)
    rp, _, gap = mmr_greedy64(X, Q, cand, k, delta, pre, gap_from)
    clear = gap > 2 * tol
    left_out = int((~clear).sum())
    assert left_out <= CAP * M, f"{left_out} of {M} queries have an fp64 gap within 2 tol: the case decides too little"
    bad = [m for m in np.flatnonzero(clear) if not np.array_equal(pick[m], rp[m])]
    assert not bad, f"queries {bad[:8]} differ from the fp64 greedy picks: {pick[bad[0]]} vs {rp[bad[0]]}"
    return left_out


def recipe(D, F, M=128, n=2048, seed=0, rank=8):
    """Rank-8 Gaussian data embedded in R^D by a random orthonormal basis and
    unit-normalised (every coordinate dense; cosine gaps those of 8
    dimensions), M queries of the same kind, and the fp64 L2 top-F of the n
    rows as pools, nearest first. Returns (X fp32 [n, D], Q fp32 [M, D],
    cand int64 [M, F])."""
    rng = np.random.default_rng(seed)
    B = np.linalg.qr(rng.standard_normal((D, rank)))[0].T          # [rank, D], orthonormal rows
    X = rng.standard_normal((n, rank)) @ B
    Q = rng.standard_normal((M, rank)) @ B
    X = (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)
    Q = (Q / np.linalg.norm(Q, axis=1, keepdims=True)).astype(np.float32)
    X64, Q64 = X.astype(np.float64), Q.astype(np.float64)
    s = 2.0 * Q64 @ X64.T - (X64 * X64).sum(1)[None, :]            # -|q - x|^2 + |q|^2
    cand = np.argsort(-s, axis=1, kind="stable")[:, :F].astype(np.int64)
    return X, Q, cand
