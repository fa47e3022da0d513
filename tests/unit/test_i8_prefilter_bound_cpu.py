"""The quad bound of the int8 scan's tiered prefilter (search256.hip, OPT bit
6), modelled in numpy float32 operation by operation as the kernel rounds:

    score[e] = fma(al, fl(float(v[e]) * rs[e]), b[e])          e = 0..3
    u        = fma(al, fl(float(max(v[0..3], 0)) * max_e rs[e]), max_e b[e])

For al > 0 and rs >= 0 the bound u must reach every score of its quad, bit for
bit (no tolerance): the scan drops a quad whose u is below the threshold, and
the set of appended records has to stay the one of the float epilogue.
"""
import numpy as np

N_QUADS = 200_000
LIM = (1 << 24) - 1  # |int32 sum| of a D <= 1024 int8 dot product stays below 2^24


def fma32(a, b, c):
    """Correctly rounded float32 fma(a, b, c) of float32 arrays: the product is
    exact in float64, the sum is rounded to odd in float64 (TwoSum gives the
    rounding error's sign), and 53 >= 2 * 24 + 2 bits make the final rounding
    to float32 the single rounding of the exact a * b + c."""
    a, b, c = (np.asarray(x, dtype=np.float32).astype(np.float64) for x in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        bits = s.view(np.int64).copy()
        fix = np.isfinite(s) & np.isfinite(err) & (err != 0) & ((bits & 1) == 0)
        grow = (err > 0) == (s > 0)  # the exact sum lies further from zero than s
        bits = np.where(fix, np.where(grow, bits + 1, bits - 1), bits)
        return bits.view(np.float64).astype(np.float32)


def scores(al, v, rs, b):
    p = (v.astype(np.float32) * rs).astype(np.float32)  # the conversion is exact below 2^24
    return fma32(al[:, None], p, b)


def bound(al, v, rs, b):
    m = np.maximum(v.max(axis=1), 0)
    R = rs.max(axis=1)
    B = b.max(axis=1)
    return fma32(al, (m.astype(np.float32) * R).astype(np.float32), B)


def draw(seed=0, n=N_QUADS):
    g = np.random.default_rng(seed)
    kind = g.integers(0, 6, size=n)
    v = np.empty((n, 4), dtype=np.int64)
    v[:] = g.integers(-LIM, LIM + 1, size=(n, 4))
    small = kind == 1  # sums of unit vectors: a few thousand either side of zero
    v[small] = g.integers(-4000, 4001, size=(int(small.sum()), 4))
    neg = kind == 2  # every sum negative (queries = -rows)
    v[neg] = -np.abs(v[neg]) - 1
    v[neg] = np.maximum(v[neg], -LIM)
    ext = kind == 3  # the extremes and zero
    v[ext] = g.choice(np.array([-LIM, LIM, 0, -1, 1]), size=(int(ext.sum()), 4))
    zero = kind == 4
    v[zero] = 0
    v = v.astype(np.int32)
    # scales: log-uniform over 1e-6..1 inside ONE quad, some of them zero (zero rows)
    rs = np.exp(g.uniform(np.log(1e-6), 0.0, size=(n, 4))).astype(np.float32)
    near = g.random(n) < 0.3  # neighbouring rows of real embeddings: a few percent apart
    base = np.exp(g.uniform(np.log(1e-6), 0.0, size=n)).astype(np.float32)
    rs[near] = (base[near, None] * g.uniform(0.97, 1.03, size=(int(near.sum()), 4))).astype(np.float32)
    rs[g.random((n, 4)) < 0.1] = 0.0
    rs[:64] = 0.0  # whole quads of zero rows
    # biases: mixed sign, some -inf (removed rows), some quads all -inf, some all zero (no bias)
    b = g.normal(0.0, 1.0, size=(n, 4)).astype(np.float32)
    b[g.random((n, 4)) < 0.15] = -np.inf
    b[64:128] = -np.inf
    b[g.random(n) < 0.2] = 0.0
    al = np.exp(g.uniform(np.log(1e-5), np.log(8.0), size=n)).astype(np.float32)  # alpha * query scale > 0
    return al, v, rs, b


def test_fma32_model_is_a_single_rounding():
    # cases where a float64 sum rounded again to float32 (double rounding) goes wrong
    a = np.float32(1.0 + 2.0 ** -23)
    got = fma32([a], [a], [np.float32(-1.0)])
    exact = (1.0 + 2.0 ** -23) ** 2 - 1.0  # 2^-22 + 2^-46: exact in float64
    assert got[0] == np.float32(exact)
    # a tie in float32 that the product's low bits break upwards
    one = np.float32(1.0)
    tie = fma32([np.float32(2.0 ** -24)], [np.float32(1.0 + 2.0 ** -23)], [one])
    assert tie[0] == np.float32(1.0 + 2.0 ** -23)
    assert fma32([one], [one], [np.float32(-np.inf)])[0] == -np.inf
    assert fma32([np.float32(0.0)], [one], [np.float32(0.0)])[0] == 0.0


def test_quad_bound_reaches_every_score():
    al, v, rs, b = draw()
    assert len(al) >= 100_000
    sc = scores(al, v, rs, b)
    u = bound(al, v, rs, b)
    assert not np.isnan(u).any() and not np.isnan(sc).any()
    assert (u[:, None] >= sc).all()
    # the data holds what it claims to
    assert (v < 0).any() and (v == 0).any() and (v == LIM).any() and (v == -LIM).any()
    nz = np.where(rs > 0, rs, np.inf).min(axis=1)
    assert (rs.max(axis=1) / nz > 1e4).any() and (rs == 0).any()
    assert (b > 0).any() and (b < 0).any() and np.isneginf(b).any()
    assert np.isneginf(u).any()  # an all -inf quad is bounded by -inf, not by NaN


def test_threshold_at_a_score_keeps_its_quad():
    """The kernel's tests `u >= t - 1e-6 |t|` (quad, column) must hold for a
    threshold set exactly to one of the quad's scores -- that score is
    appended by the per-score pass (score >= t), so its quad may not be
    skipped; t = +inf skips (NaN compare), t = -inf keeps."""
    al, v, rs, b = draw(seed=1)
    sc = scores(al, v, rs, b)
    u = bound(al, v, rs, b)
    for e in range(4):
        t = sc[:, e]
        fin = np.isfinite(t)
        with np.errstate(invalid="ignore"):
            tcut = (t - (np.float32(1e-6) * np.abs(t)).astype(np.float32)).astype(np.float32)
            keep = u >= tcut
        assert keep[fin].all()
    with np.errstate(invalid="ignore"):
        inf = np.full_like(u, np.inf)
        assert not (u >= inf - np.float32(1e-6) * np.abs(inf)).any()
        assert (u >= -inf - np.float32(1e-6) * np.abs(inf)).all()


def test_bound_is_tight_for_equal_scales():
    """With one scale and one bias in the quad and a non-negative largest sum
    the bound IS the largest score: the filter loses nothing to the model."""
    al, v, rs, b = draw(seed=2, n=20_000)
    rs[:] = rs[:, :1]
    b = np.where(np.isneginf(b[:, :1]), np.float32(0.0), b[:, :1]) * np.ones((1, 4), dtype=np.float32)
    sc = scores(al, v, rs, b)
    u = bound(al, v, rs, b)
    pos = v.max(axis=1) >= 0
    assert pos.sum() > 1000
    assert (u[pos] == sc[pos].max(axis=1)).all()
