"""Keyword and hybrid search on the device (csrc/kernels/lexical.hip) against
the fp64 oracle tests/kernels/_lex_ref.py: the BM25 scan and its merge bit for
bit, the fusion under the oracle's two rules, ``store_search(lexical=)`` end
to end, and ``lexical=None`` against the plain call."""
import functools

import numpy as np
import pytest
import torch

from lazzaro_amd.ops.lex_ops import lex_fuse, lex_topk
from tests.kernels import _lex_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
K1, B = 1.2, 0.75


def _dev(a):
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _scan_case(n, M, T, W):
    """The columns, queries, weights and fp32 oracle scores of a case (computed once)."""
    slots, dl, bias = R.columns(n, W, seed=n % 7)
    qt = R.queries(M, T, seed=M)
    df, N, avgdl = R.stats(slots, dl)
    w = R.weights(qt, df, N)
    return slots, dl, bias, qt, w, avgdl, R.scores(slots, dl, qt, w, K1, B, avgdl)


@pytest.mark.parametrize("n,M,T,W,k,cap", R.SCAN_CASES,
                         ids=[f"n{n}-M{M}-T{T}-W{W}-k{k}-cap{c}" for n, M, T, W, k, c in R.SCAN_CASES])
def test_scan_and_merge_equal_the_oracle(n, M, T, W, k, cap):
    slots, dl, bias, qt, w, avgdl, sc = _scan_case(n, M, T, W)
    ws, wr = R.topk(sc, bias, k)
    s, r = lex_topk(_dev(slots), _dev(dl), _dev(bias), qt, w, k, K1, B, avgdl, grid_cap=cap)
    assert s.dtype == torch.float32 and r.dtype == torch.long and s.shape == r.shape == (M, k)
    assert np.array_equal(r.cpu().numpy(), wr), (r.cpu().numpy()[:2], wr[:2])
    assert np.array_equal(s.cpu().numpy(), ws)
    if n > 1000 and M > 4:  # the case means what it says: a k above the matches, the term every row holds, ties
        live = (wr >= 0).sum(1)
        assert live.min() == 0 and live.max() == k
        assert (np.isfinite(bias) & (sc > 0)).sum(1).max() > n // 2


def test_other_k_and_parameters_on_one_case():
    n, M, T, W = 4097, 9, 32, 32
    slots, dl, bias, qt, w, avgdl, _ = _scan_case(n, M, T, W)
    d = _dev(slots), _dev(dl), _dev(bias)
    for k1, b in ((0.0, 0.0), (2.0, 1.0), (0.9, 0.4)):
        sc = R.scores(slots, dl, qt, w, k1, b, avgdl)
        for k in (1, 16):
            ws, wr = R.topk(sc, bias, k)
            s, r = lex_topk(*d, qt, w, k, k1, b, avgdl, grid_cap=3)
            assert np.array_equal(r.cpu().numpy(), wr) and np.array_equal(s.cpu().numpy(), ws), (k1, b, k)
    # identical rows: the lower row first, at one score
    s, r = lex_topk(*d, qt, w, 64, K1, B, avgdl)
    s, r = s.cpu().numpy(), r.cpu().numpy()
    pairs = [(a, c) for m in range(M) for a, c in zip(r[m], r[m][1:]) if a >= 0 and c == a + 1
             and np.array_equal(slots[a], slots[c]) and dl[a] == dl[c]]
    assert pairs, "no identical neighbours among the results: the case does not test the tie order"


@functools.lru_cache(maxsize=None)
def _fuse_case(n, D, M, P):
    return R.fuse_inputs(n, D, M, P)


@pytest.mark.parametrize("n,D,M,P,k,alpha", R.FUSE_CASES,
                         ids=[f"n{n}-D{D}-M{M}-P{P}-k{k}-a{a}" for n, D, M, P, k, a in R.FUSE_CASES])
def test_fuse_holds_the_two_rules(n, D, M, P, k, alpha):
    I = _fuse_case(n, D, M, P)
    dp = None if alpha == 1.0 else I["dpool"]
    s, r = lex_fuse(_dev(I["X"]), _dev(I["Q"]), None if dp is None else _dev(dp), _dev(I["lpool"]), _dev(I["slots"]),
                    _dev(I["dl"]), I["qt"], I["w"], alpha, k, K1, B, I["avgdl"])
    assert s.dtype == torch.float32 and r.dtype == torch.long
    left = R.check_fused(I["X"], I["Q"], dp, I["lpool"], I["slots"], I["dl"], I["qt"], I["w"], alpha, K1, B,
                         I["avgdl"], k, s.cpu().numpy(), r.cpu().numpy())
    print(f"n={n} D={D} M={M} P={P} k={k} alpha={alpha}: {left} of {M} left out of the exact-order rule")
    if dp is not None:  # the case means what it says: overlapping and disjoint pools, empty slots in either
        both = [len(set(a[a >= 0]) & set(c[c >= 0])) for a, c in zip(dp, I["lpool"])]
        assert max(both) > 0 and min(both) == 0
        assert (dp < 0).any() and (I["lpool"] < 0).any() and (dp >= n).any()


def test_fuse_scalar_path_and_strided_rows():
    """D % 4 != 0 takes the scalar loads; a row stride above D the strided ones."""
    I = R.fuse_inputs(63, 30, 8, 16, seed=3)
    X = torch.zeros((63, 40), device=DEV)
    X[:, :30] = _dev(I["X"])
    for Xd in (_dev(I["X"]), X[:, :30]):
        s, r = lex_fuse(Xd, _dev(I["Q"]), _dev(I["dpool"]), _dev(I["lpool"]), _dev(I["slots"]), _dev(I["dl"]),
                        I["qt"], I["w"], 0.3, 10, K1, B, I["avgdl"])
        R.check_fused(I["X"], I["Q"], I["dpool"], I["lpool"], I["slots"], I["dl"], I["qt"], I["w"], 0.3, K1, B,
                      I["avgdl"], 10, s.cpu().numpy(), r.cpu().numpy())


def _tenant(W=16):
    from lazzaro_amd.engine.tenant_graph import TenantGraph
    X, texts, sal, _, _ = R.e2e_inputs()
    n, D = X.shape
    g = TenantGraph(device=DEV, dim=D, capacity=n + 8)
    g.lexical_slots = W
    g.add_nodes([f"m{i}" for i in range(n)], texts, torch.from_numpy(X), shard=g.shard_id("w"),
                sal=torch.from_numpy(sal), stored=True)
    return g, X, texts, sal


@pytest.mark.parametrize("where", [None, {"min_salience": 0.5}], ids=["all", "where"])
def test_store_search_end_to_end(where):
    from lazzaro_amd.core.lexical import query_terms, terms_py
    g, X, texts, sal = _tenant()
    n = g.n
    _, _, _, queries, Q = R.e2e_inputs()
    slots, dl = terms_py(texts, 16)
    ok = sal >= 0.5 if where else np.ones(n, dtype=bool)
    bias = np.where(ok, 0.0, -np.inf).astype(np.float32)
    qt = query_terms(queries)
    df, N, avgdl = R.stats(slots, dl)
    w = R.weights(qt, df, N)
    # the lexical leg alone
    sc = R.scores(slots, dl, qt, w, K1, B, avgdl)
    ws, wr = R.topk(sc, bias, 16)
    s, r = g.lexical_topk(queries, 16, where=where)
    assert np.array_equal(r.cpu().numpy(), wr) and np.array_equal(s.cpu().numpy(), ws)
    assert (wr[3] == -1).all() and (123 in wr[0]) == bool(ok[123])
    # fused: the oracle over the pools the engine's own dense search returns
    Qd = torch.from_numpy(Q).to(DEV)
    _, dpool = g.store_search(Qd, 16, "cosine", True, where)
    for alpha in (0.3, 1.0):
        s, r = g.store_search(Qd, 10, "cosine", where=where, lexical=alpha, query_terms=queries)
        dp = None if alpha == 1.0 else dpool.cpu().numpy()
        R.check_fused(X, Q, dp, wr, slots, dl, qt, w, alpha, K1, B, avgdl, 10, s.cpu().numpy(), r.cpu().numpy())
        rows = r.cpu().numpy()
        assert ok[rows[rows >= 0]].all()
        if ok[123] and alpha == 1.0:
            assert rows[0, 0] == 123
    assert 123 not in g.store_search(Qd, 10, "cosine", where=where)[1][0].tolist()


def test_lexical_none_is_the_plain_call():
    g, X, _, _ = _tenant()
    Q = torch.from_numpy(X[:5] + 0.01).to(DEV)
    for metric in ("l2", "cosine"):
        for kw in ({}, {"where": {"min_salience": 0.3}}, {"node_rows": True}):
            a = g.store_search(Q, 10, metric, **kw)
            b = g.store_search(Q, 10, metric, lexical=None, query_terms=None, **kw)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert g._lexicon is None and g.lexical_searches == 0


def test_lexical_topk_after_a_compaction():
    """Rows leave, the survivors slide down, the epoch moves: the next lexical
    search rebuilds the lexicon over the rows as they now lie."""
    from lazzaro_amd.core.lexical import query_terms, terms_py
    g, X, texts, _ = _tenant()
    _, _, _, queries, _ = R.e2e_inputs()
    g.lexical_topk(queries, 16)  # the lexicon of the rows as inserted
    assert g._lexicon.builds == 1 and g._lexicon.covered == g.n == len(texts)
    gone = sorted(set(range(3, len(texts), 7)) | {122})
    g.remove_nodes(gone, drop_edges=True, unstore=True)
    g.take_dirty_rows(), g.take_dirty_edges(), g.take_deleted()
    out = g.compact()
    assert out["reclaimed"] == len(gone) and g.row_epoch == 1 and g.n == len(texts) - len(gone)
    kept = [r for r in range(len(texts)) if r not in set(gone)]
    assert [g.ids[i] for i in range(g.n)] == [f"m{r}" for r in kept]
    slots, dl = terms_py([texts[r] for r in kept], 16)
    qt = query_terms(queries)
    df, N, avgdl = R.stats(slots, dl)
    w = R.weights(qt, df, N)
    ws, wr = R.topk(R.scores(slots, dl, qt, w, K1, B, avgdl), np.zeros(len(kept), dtype=np.float32), 16)
    s, r = g.lexical_topk(queries, 16)
    assert g._lexicon.builds == 2 and g._lexicon.covered == g.n
    assert np.array_equal(r.cpu().numpy(), wr) and np.array_equal(s.cpu().numpy(), ws)
    assert kept[int(wr[0, 0])] == 123 and int(wr[0, 0]) < 123  # the memory that holds the token, at its new row
