"""tests/kernels/_wide_ref.py on its own, and the CPU side of the wide-k
search: the threshold rule against an exact tail sum, the reference against a
brute-force loop, the ``wide_k`` plumbing, the CPU tier of the two new ops, and
the proof that every Gaussian case of tests/kernels/test_widek_gpu.py is
decidable (no query of it is ever left out of a comparison)."""
from fractions import Fraction
from math import comb

import numpy as np
import pytest
import torch

from lazzaro_amd.ops import search as S
from tests.kernels import _cand_ref as C
from tests.kernels import _wide_ref as W


# ---------------------------------------------------------------- threshold rule
def _exact_tail(k, S_, j):
    p = Fraction(1, S_)
    return sum(Fraction(comb(k, i)) * p ** i * (1 - p) ** (k - i) for i in range(j, k + 1))


@pytest.mark.parametrize("S_", [1, 2, 16, 40, 64, 256])
def test_threshold_rule_against_the_exact_tail(S_):
    for k in (17, 18, 30, 31, 40, 47, 48, 63, 64):
        for j in (1, 3, 5, 9, 16):
            assert abs(W.binom_tail(k, 1.0 / S_, j) - float(_exact_tail(k, S_, j))) <= 1e-12
        j = W.spec_j(k, S_)
        assert j == S.wide_spec_j(k, S_)  # the library's rule is the reference's
        ok = [t for t in range(1, 17) if _exact_tail(k, S_, t) <= Fraction(1, 10000)]
        assert j == (ok[0] if ok else 16)
        if ok and j > 1:
            assert _exact_tail(k, S_, j - 1) > Fraction(1, 10000)


def test_the_documented_table_at_stride_64():
    got = {k: S.wide_spec_j(k, 64) for k in range(17, 65)}
    want = {k: 5 if k <= 30 else 6 if k <= 47 else 7 for k in range(17, 65)}
    assert got == want
    assert "j = 5" in S.flat_topk_i8_wide.__doc__ and "j = 7" in S.flat_topk_i8_wide.__doc__


# ---------------------------------------------------------------- the reference itself
def _brute_topk(s, k):
    """Selection by repeated scan: the best remaining (score, then lower row)."""
    left = [(float(v), r) for r, v in enumerate(s) if v != W.NEG_INF]
    out = []
    while left and len(out) < k:
        b = left[0]
        for e in left[1:]:
            if e[0] > b[0] or (e[0] == b[0] and e[1] < b[1]):
                b = e
        left.remove(b)
        out.append(b)
    return out


def test_topk_ref_against_a_brute_force_loop():
    rng = np.random.default_rng(3)
    X = C.grid_rows(rng, 90, 64)          # integers: exact ties, planted duplicate rows
    Q = C.grid_queries(rng, 4, 64)
    bias = -(X * X).sum(1)
    bias[[3, 50]] = W.NEG_INF
    for k in (17, 64):
        s, r = W.topk_ref(X, Q, k, bias, 2.0, idx_offset=5)
        full = W.scores64(X, Q, bias, 2.0)
        for q in range(4):
            want = _brute_topk(full[q], k)
            assert r[q].tolist() == [w[1] + 5 for w in want] and s[q].tolist() == [w[0] for w in want]
    bias[10:] = W.NEG_INF                 # 9 live rows (0 .. 9 without row 3): padding
    s, r = W.topk_ref(X, Q, 17, bias, 2.0)
    assert (r[:, 9:] == -1).all() and (s[:, 9:] == W.NEG_INF).all() and (r[:, :9] >= 0).all()


def test_contract_ref_is_the_rerank_of_the_bf16_top64():
    rng = np.random.default_rng(4)
    X = C.unit_rows(rng, 300, 32).astype(np.float32)
    Q = C.unit_rows(rng, 3, 32).astype(np.float32) * 1.7
    for metric in ("l2", "ip", "cosine"):
        bias = W.l2_bias(X) if metric == "l2" else np.zeros(300, np.float32)
        bias[7] = W.NEG_INF
        s, r = W.contract_ref(X, Q, bias, metric, 20)
        full = W.store_scores64(X, Q, bias, metric)
        Qn = Q / np.linalg.norm(Q, axis=1, keepdims=True) if metric == "cosine" else Q
        _, c64 = W.topk_ref(C.to_bf16(X), C.to_bf16(Qn.astype(np.float32)), 64, bias, 2.0 if metric == "l2" else 1.0)
        for q in range(3):
            want = sorted(c64[q].tolist(), key=lambda i: (-full[q, i], i))[:20]
            assert r[q].tolist() == want and 7 not in want
            assert np.array_equal(s[q], full[q, want])
        # with kc >= the live rows the contract is the exact fp32-precision search
        s2, r2 = W.contract_ref(X, Q, bias, metric, 20, kc=300)
        assert np.array_equal(r2, W.topk_of(full, 20)[1])


def test_wide_bound_counts_the_kernels_roundings():
    assert W.wide_roundings(128) == 21 and W.wide_roundings(768) == 101
    X = np.array([[1.0, -2.0] * 4]); Q = np.array([[0.5, 3.0] * 4])
    b = W.wide_bound(X, Q, np.array([-4.0]), 2.0)
    assert np.isclose(b[0, 0], W.gamma(8 // 8 + 6) * (2.0 * 4 * 6.5 + 4.0))
    assert W.wide_bound(X, Q, np.array([W.NEG_INF]), 2.0)[0, 0] == W.gamma(7) * 52.0


# ---------------------------------------------------------------- decidable Gaussian cases
@pytest.mark.parametrize("name", sorted(W.GAUSS_CASES))
def test_every_gaussian_gpu_case_is_decidable(name):
    N, D, nq, k, roundings = W.GAUSS_CASES[name]
    X, Q, bias, Sc, B = W.gauss_case(name)
    assert X.shape == (N, D) and Q.shape == (nq, D) and np.array_equal(X, C.to_bf16(X))
    assert np.array_equal(bias, W.l2_bias(X))
    assert np.array_equal(B, W.wide_bound(X, Q, bias, W.ALPHA, roundings))
    s, r = W.topk_of(Sc, k + 1)
    assert (r >= 0).all()
    b = np.take_along_axis(B, r, 1)
    gap = s[:, :-1] - s[:, 1:]
    assert (gap > 2.0 * np.maximum(b[:, :-1], b[:, 1:])).all()  # ranks 1 .. k + 1, every query: nothing skipped


# ---------------------------------------------------------------- CPU tier of the ops
def test_cpu_tier_of_both_ops_is_ref_topk():
    gen = torch.Generator().manual_seed(5)
    X16 = torch.nn.functional.normalize(torch.randn(500, 128, generator=gen), dim=1).to(torch.bfloat16)
    Q16 = torch.nn.functional.normalize(torch.randn(4, 128, generator=gen), dim=1).to(torch.bfloat16)
    bias = -(X16.float() ** 2).sum(1)
    bias[11] = float("-inf")
    X8, rs = S.quantize_i8_rows(X16)
    Q8, qs = S.quantize_i8_rows(Q16)
    for k in (17, 64):
        e_s, e_r = S._ref_topk(X16, Q16, k, bias, None, None, 2.0, 0)
        a_s, a_r = S.flat_topk_wide(X16, Q16, k, bias=bias, alpha=2.0)
        b_s, b_r = S.flat_topk_i8_wide(X8, rs, Q8, qs, X16, Q16, k, bias=bias, alpha=2.0)
        for s_, r_ in ((a_s, a_r), (b_s, b_r)):
            assert torch.equal(r_, e_r) and torch.equal(s_, e_s)
        w_s, w_r = W.topk_ref(X16.float().numpy(), Q16.float().numpy(), k, bias.numpy(), 2.0)
        assert (a_r.numpy() == w_r).mean() > 0.98  # (fp32 matmul against fp64: a near tie may swap)
    with pytest.raises(AssertionError):
        S.flat_topk_i8_wide(X8, rs, Q8, qs, X16, Q16, 16, bias=bias, alpha=2.0)
    with pytest.raises(AssertionError):
        S.flat_topk_i8_wide(X8, rs, Q8, qs, X16, Q16, 65, bias=bias, alpha=2.0)


# ---------------------------------------------------------------- plumbing
def test_wide_k_plumbing(tmp_path):
    from lazzaro_amd.config import MemoryConfig
    from lazzaro_amd.core.memory_system import MemorySystem
    from lazzaro_amd.core.providers import HashEmbedder, LocalLLM
    from lazzaro_amd.core.vector_store import HBMStore
    from lazzaro_amd.engine.tenant_graph import TenantGraph

    assert MemoryConfig().wide_k is False and TenantGraph.wide_k is False
    assert MemoryConfig.from_env(wide_k=True).wide_k is True

    class G:
        wide_k = False
        ann_cfg = None
    for kw, want in (({}, False), ({"wide_k": True}, True)):
        st = HBMStore(db_dir=str(tmp_path / f"s{int(want)}"), device="cpu", **kw)
        g = G()
        st.attach("u", g)
        assert g.wide_k is want and st.wide_k is want
    for params, want in ((None, False), ({"wide_k": True}, True)):
        m = MemorySystem(llm_provider=LocalLLM(), embedding_provider=HashEmbedder(dim=32), enable_async=False,
                         load_from_disk=False, db_dir=str(tmp_path / f"m{int(want)}"), device="cpu",
                         index_params=params)
        try:
            assert m.graph.wide_k is want
            assert m.get_stats()["engine"]["wide_searches"] == 0
        finally:
            m.close()


def test_cpu_tenant_is_identical_with_the_flag_on_and_off():
    from lazzaro_amd.engine.tenant_graph import TenantGraph
    gen = torch.Generator().manual_seed(6)
    X = torch.nn.functional.normalize(torch.randn(700, 48, generator=gen), dim=1)
    Q = torch.nn.functional.normalize(torch.randn(5, 48, generator=gen), dim=1)
    g = TenantGraph(device="cpu", dim=48, capacity=1024)
    g.add_nodes([f"m{i}" for i in range(700)], ["c"] * 700, X, shard=g.shard_id("w"), stored=True)
    off = g.store_search(Q, 40, "l2")
    g.wide_k = True
    on = g.store_search(Q, 40, "l2")
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])
    assert g.wide_searches == 0  # a CPU tenant never takes the route
    e_s, e_r = W.topk_of(W.store_scores64(X.numpy(), Q.numpy(), W.l2_bias(X.numpy()), "l2"), 40)
    assert (on[1].numpy() == e_r).mean() > 0.98
