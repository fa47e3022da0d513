"""The references of the certified int8 store search's stages
(tests/kernels/_cand_ref.py) on their own, on any machine: each reference
against an independent formulation, fp32 emulations of the re-score kernels
inside ``score_bound`` -- and the property the search's exactness claim rests
on: the worst-case margin of TenantGraph._i8_query bounds |int8 scan score -
bf16 score| for every (query, row), adversarial rows included.
"""
import numpy as np
import pytest
import torch

from lazzaro_amd.ops import search as S
from tests.kernels import _cand_ref as R

NEG_INF = float("-inf")


# ---------------------------------------------------------------- select
@pytest.mark.parametrize("kout", [1, 4, 10])
def test_select_ref_against_stable_sort_chain(kout):
    rng = np.random.default_rng(11 + kout)
    nq, cap = 9, 40
    cs = rng.integers(-3, 4, size=(nq, cap)).astype(np.float64)  # many ties
    cs[rng.random((nq, cap)) < 0.2] = NEG_INF
    cs[7] = NEG_INF
    ci = np.stack([rng.permutation(1000)[:cap] for _ in range(nq)]).astype(np.int64)
    cnt = np.array([0, 1, kout - 1, kout, 17, cap, cap + 5, 3, 12 | R.CNT_OVF], dtype=np.int64)
    need = np.array([0, 2, 0, kout, 18, cap + 1, 0, 3, 1], dtype=np.int64)
    off = (1 << 33) + 5
    s, r, ovf = R.select_ref(cnt, cs, ci, cap, kout, off, need)
    for q in range(nq):
        n = min(int(cnt[q]) & R.CNT_MASK, cap)
        ts, ti = torch.from_numpy(cs[q, :n].copy()), torch.from_numpy(ci[q, :n].copy())
        o = torch.sort(ti, stable=True).indices  # rows ascending, then a stable sort by score descending
        ts, ti = ts[o], ti[o]
        o = torch.sort(ts, descending=True, stable=True).indices[:kout]
        es = torch.full((kout,), NEG_INF, dtype=torch.float64)
        ei = torch.full((kout,), -1, dtype=torch.long)
        es[: o.numel()] = ts[o]
        ei[: o.numel()] = torch.where(ts[o] == NEG_INF, torch.full_like(ti[o], -1), ti[o] + off)
        assert np.array_equal(s[q], es.numpy()) and np.array_equal(r[q], ei.numpy()), q
        assert int(ovf[q]) == int(cnt[q] > cap or cnt[q] < need[q])
    assert ovf.tolist() == [0, 1, 0, 0, 1, 1, 1, 0, 1]  # bit 30 alone makes the last one overflow
    assert np.array_equal(R.select_ref(cnt, cs, ci, cap, kout)[2], (cnt > cap).astype(np.int32))


# ---------------------------------------------------------------- thresholds
@pytest.mark.parametrize("has_m,has_r", [(True, True), (True, False), (False, True), (False, False)])
def test_thr_prep_ref_against_the_torch_chain(has_m, has_r):
    """The three lines of flat_topk_i8 that lzk_thr_prep replaced: tau =
    _margin(ts[:, col]); thr = tau - margin; cert = _cert_tau(thr, margin_rig)."""
    rng = np.random.default_rng(3)
    fm = R.FLT_MAX
    special = [np.inf, -np.inf, np.nan, fm, -fm, 0.0, 1e-42, -1e-42, 1.0, -1.0, 3e38, -3e38]
    t = np.concatenate([np.array(special), rng.standard_normal(300) * 10.0 ** rng.integers(-6, 7, size=300)])
    nq = t.size
    ts = rng.standard_normal((nq, 5)).astype(np.float32)
    ts[:, 3] = t.astype(np.float32)
    m = np.abs(rng.standard_normal(nq)).astype(np.float32) if has_m else None
    mr = (np.abs(rng.standard_normal(nq)) * 1.5).astype(np.float32) if has_r else None
    thr, cert = R.thr_prep_ref(ts, 3, m, mr)
    tt = torch.from_numpy(ts)
    tau = S._margin(tt[:, 3])
    e_thr = (tau - torch.from_numpy(m)).contiguous() if has_m else tau
    e_cert = S._cert_tau(e_thr, torch.from_numpy(mr) if has_r else None)
    assert thr.dtype == np.float32 and cert.dtype == np.float32
    assert np.array_equal(thr.view(np.int32), e_thr.numpy().view(np.int32))
    assert np.array_equal(cert.view(np.int32), e_cert.numpy().view(np.int32))
    assert not np.isnan(thr).any() and not np.isnan(cert).any()
    assert thr[2] == NEG_INF and cert[2] == NEG_INF  # a nan sample: no threshold, certified without a count


# ---------------------------------------------------------------- exact scores, the bound
@pytest.mark.parametrize("D", [4, 252, 256, 260, 768, 2048])
@pytest.mark.parametrize("bf16", [True, False])
def test_fp32_rescore_emulations_inside_score_bound(D, bf16):
    rng = np.random.default_rng(100 + D)
    X = R.unit_rows(rng, 64, D)
    q = R.unit_rows(rng, 1, D)[0]
    if bf16:
        X, q = R.to_bf16(X), R.to_bf16(q)
    else:
        X, q = X.astype(np.float32).astype(np.float64), q.astype(np.float32).astype(np.float64)
    bias = -(X.astype(np.float32) ** 2).sum(1).astype(np.float32)
    rows = np.arange(64)
    for alpha, b in ((1.0, None), (2.0, bias)):
        ref, bound = R.score_ref(X, q, rows, b, alpha)
        for emu in (R.rescore_wave_fp32, R.rescore16_fp32):
            got = emu(X, q, b, alpha).astype(np.float64)
            assert (np.abs(got - ref) <= 1.0 * bound).all(), (emu.__name__, float((np.abs(got - ref) / bound).max()))
        # sanity of the pair: four corrupted elements leave the bound many times over
        Xc = X.copy()
        Xc[:, :4] += np.sign(q[:4])[None, :]
        bad = R.rescore_wave_fp32(Xc, q, b, alpha).astype(np.float64)
        assert np.abs(q[:4]).sum() > 0.02
        assert (np.abs(bad - ref) > 20.0 * bound).all()


def test_grid_inputs_rescore_exactly_in_fp32():
    rng = np.random.default_rng(5)
    X, Q = R.grid_rows(rng, 40, 2048), R.grid_queries(rng, 1, 2048)
    bias = rng.integers(-64, 65, size=40).astype(np.float64)
    ref, _ = R.score_ref(X, Q[0], np.arange(40), bias, 2.0)
    assert np.abs(ref).max() < 2.0 ** 24
    for emu in (R.rescore_wave_fp32, R.rescore16_fp32):
        assert np.array_equal(emu(X, Q[0], bias, 2.0).astype(np.float64), ref)
    assert np.array_equal(X[39], X[0]) and ref[39] - bias[39] == ref[0] - bias[0]  # planted duplicate rows tie


def test_cut_and_rescore_ref_edges():
    c, b = R.cut_ref(np.array([NEG_INF, 5.0, 5.0]), np.array([0.5, 0.5, 0.5]), 2.0)
    assert c[0] == NEG_INF and b[0] == 0.0
    assert abs(c[1] - (4.5 - 2 * R.C_2E4 - 6 * R.C_1E6)) < 1e-15
    c, _ = R.cut_ref(np.array([NEG_INF, 5.0]), np.array([0.5, 0.5]), 1.0, floor=7.0)
    assert c.tolist() == [6.5, 6.5]
    # re-score: an entry at the cut, at the floor and at tau is kept / kept / a hit
    X = np.array([[1.0, 0, 0, 0], [2.0, 0, 0, 0], [3.0, 0, 0, 0], [4.0, 0, 0, 0]])
    Q = np.array([[1.0, 0, 0, 0]])
    cs = np.array([[10.0, 9.0, 10.0, 11.0, np.nan]])
    ci = np.array([[0, 1, 2, 3, 0]])
    out = R.rescore_ref(X, Q, None, 1.0, [4], cs, ci, 5, cut=[10.0], floor=3.0, tau=[3.0], k_need=2, need_val=9)
    assert out["cs"][0, :4].tolist() == [NEG_INF, NEG_INF, 3.0, 4.0] and np.isnan(out["cs"][0, 4])
    assert out["hits"][0] == 2 and out["need"][0] == 0
    out = R.rescore_ref(X, Q, None, 1.0, [4], cs, ci, 5, cut=[10.0], floor=3.0, tau=[3.5], k_need=2, need_val=9)
    assert out["hits"][0] == 1 and out["need"][0] == 9
    out = R.rescore_ref(X, Q, None, 1.0, [4], cs, ci, 5, tau=[NEG_INF], k_need=2, need_val=9)
    assert out["need"][0] == 0 and out["cs"][0, :4].tolist() == [1.0, 2.0, 3.0, 4.0]


def test_gather_ref_counts_and_overflow_flag():
    recs = np.zeros((2, 4, 4), dtype=np.int32)
    recs[0, :3] = [[0, 5, 1, 1], [1, 6, 2, 3], [-1, 7, 3, 1]]
    recs[1, :4] = [[0, 8, 4, 2], [2, 9, 5, 1], [0, 1, 6, 1], [0, 2, 7, 1]]
    (c1, f1), (c2, f2) = R.gather_ref(recs, [3, 4], 4, 2, True)
    assert c1.tolist() == [3, 1] and f1[0] == [(1, 6), (2, 7), (5, 1)] and c2.tolist() == [1, 1]
    (c1, f1), = R.gather_ref(recs, [3, 9], 4, 2, False)
    assert c1.tolist() == [3 | R.CNT_OVF, 1 | R.CNT_OVF]


# ---------------------------------------------------------------- the margin of _i8_query
def test_margin_rig_ref_against_the_torch_branch():
    from lazzaro_amd.engine import tenant_graph as TG
    torch.manual_seed(0)
    g = TG.TenantGraph(device="cpu", dim=100)
    X = torch.randn(300, 100)
    X /= X.norm(dim=1, keepdim=True)
    g.add_nodes([f"n{i}" for i in range(300)], [""] * 300, X, shard=g.shard_id("default"), stored=True)
    # a CPU tenant keeps no int8 copy: the largest row scale its GPU twin would have recorded
    g._rs8_max = S.quantize_i8_rows(X.to(torch.bfloat16))[1].max()
    Q = torch.randn(6, 100)
    Q[0] = 0.0
    q16 = g._q16(Q / Q.norm(dim=1, keepdim=True).clamp_min(1e-30))
    assert not (g.on_gpu and TG.I8_QUERY_KERNEL)  # the torch branch
    q8, qs, _, mr = g._i8_query(q16, 2.0)
    xn = 1.0 + g.max_norm_dev + 2.0 ** -7
    ref = R.margin_rig_ref(q16.float().numpy(), g.dim, float(g._rs8_max), 2.0, xn, q8.numpy(), qs.numpy())
    assert np.allclose(mr.double().numpy(), ref, rtol=1e-5, atol=0.0)
    r8, rs = R.quantize_i8_ref(q16.float().numpy())  # and the reference's own quantiser
    assert np.array_equal(r8, q8.numpy()) and np.array_equal(rs, qs.numpy())


def _adversarial_rows(rng, q16, eta, d, Dp, xn):
    """Rows of norm <= xn after bf16 rounding, [n, Dp] fp64 (bf16 values)."""
    nq = q16.shape[0]
    rows = [R.unit_rows(rng, 200, d)]
    for s in (1.0, -1.0):
        rows.append(s * eta[:, :d])          # x ~ the query's own rounding error
        rows.append(s * np.sign(q16[:, :d]))  # x ~ sign(q): the row error term's direction
        rows.append(s * (eta[:, :d] / np.maximum(np.linalg.norm(eta[:, :d], axis=1, keepdims=True), 1e-30)
                         + 0.3 * np.sign(q16[:, :d]) / np.sqrt(d)))
    dom = 0.02 * rng.standard_normal((24, d))  # one dominant element: a large row scale
    dom[np.arange(24), rng.integers(0, d, size=24)] = rng.choice([-1.0, 1.0], size=24)
    rows.append(dom)
    X = np.concatenate(rows, 0)
    nrm = np.linalg.norm(X, axis=1, keepdims=True)
    X = np.where(nrm > 0, X * (xn * (1.0 - 2.0 ** -7) / np.maximum(nrm, 1e-300)), 0.0)
    X = np.concatenate([X, q16[:, :d], np.zeros((1, d))], 0)  # rows equal to the queries (norm 1), a zero row
    out = np.zeros((X.shape[0], Dp))
    out[:, :d] = R.to_bf16(X)
    assert np.linalg.norm(out, axis=1).max() <= xn
    plain = np.ones(out.shape[0], dtype=bool)
    plain[200 + 6 * nq: 200 + 6 * nq + 24] = False  # all but the dominant-element rows
    return out, plain


# Largest observed |s8 - s16| / margin_rig per (d, xn): the maximum over alpha in
# {1, 2}, all queries and the three roundings of the bf16 score; "all rows /
# without the dominant-element rows" (the second set has the smaller smax).
# Measured with the seeds below -- observations, not thresholds: the assertion
# is <= 1.
#   d     xn = 1 + 2^-7    xn = 1.5         xn = 4
#   100   0.254 / 0.382    0.234 / 0.431    0.210 / 0.399
#   384   0.141 / 0.431    0.137 / 0.386    0.149 / 0.426
#   768   0.104 / 0.381    0.106 / 0.425    0.105 / 0.381
#   1024  0.091 / 0.356    0.093 / 0.373    0.100 / 0.399
@pytest.mark.parametrize("xn", [1.0 + 2.0 ** -7, 1.5, 4.0])
@pytest.mark.parametrize("alpha", [1.0, 2.0])
@pytest.mark.parametrize("d", [100, 384, 768, 1024])
def test_worst_case_margin_bounds_the_int8_error(d, alpha, xn):
    """|int8 scan score (fp32) - bf16 score (fp32)| <= margin_rig for every
    (query, row): Gaussian rows and the adversarial constructions, rows of norm
    up to xn, smax = the largest row scale. alpha = 2 carries the L2 bias
    -|x|^2, whose fp32 add rounds at magnitude xn^2."""
    rng = np.random.default_rng(1000 * d + int(alpha) + int(64 * xn))
    Dp = (d + 127) // 128 * 128
    q = np.zeros((9, Dp))
    q[:8, :d] = R.to_bf16(R.unit_rows(rng, 8, d))  # q[8]: a zero query
    q8t, qst = S.quantize_i8_rows(torch.from_numpy(q).float())
    q8, qs = q8t.numpy(), qst.numpy()
    eta = q8.astype(np.float64) * qs.astype(np.float64)[:, None] - q
    X, plain = _adversarial_rows(rng, q, eta, d, Dp, xn)
    x8t, rst = S.quantize_i8_rows(torch.from_numpy(X).float())
    x8, rs = x8t.numpy(), rst.numpy()
    assert float(rs[-1]) == 0.0 and float(qs[8]) == 0.0
    assert float(rs[~plain].min()) > 2.0 * float(rs[plain].max())  # the dominant rows do set smax
    bias = -(X.astype(np.float32) ** 2).sum(1).astype(np.float32) if alpha == 2.0 else None
    # the scan's score, rounded as the scan rounds: al = alpha qs; al * (float(v) * rs) + bias in fp32
    f = np.float32
    v = (q8.astype(np.float64) @ x8.astype(np.float64).T).astype(f)
    al = (f(alpha) * qs).astype(f)
    s8 = (al[:, None] * (v * rs[None, :]).astype(f)).astype(f)
    if bias is not None:
        s8 = (s8 + bias[None, :]).astype(f)
    worst = [0.0, 0.0]
    for qi in range(9):
        ref, _ = R.score_ref(X, q[qi], np.arange(X.shape[0]), bias, alpha)
        for s16 in (ref.astype(f), R.rescore_wave_fp32(X, q[qi], bias, alpha), R.rescore16_fp32(X, q[qi], bias, alpha)):
            err = np.abs(s8[qi].astype(np.float64) - s16.astype(np.float64))
            # the whole row set, and the set without its dominant-element rows: a smaller smax, a tighter bound
            for j, rows in enumerate((np.ones_like(plain), plain)):
                mr = R.margin_rig_ref(q, d, float(rs[rows].max()), alpha, xn, q8, qs)[qi]
                worst[j] = max(worst[j], float((err[rows] / mr).max()))
                assert (err[rows] <= mr).all(), (qi, j, float((err[rows] / mr).max()))
    print(f"margin ratio d={d} alpha={alpha} xn={xn:.4f}: all rows {worst[0]:.3f}, without dominant rows {worst[1]:.3f}")
