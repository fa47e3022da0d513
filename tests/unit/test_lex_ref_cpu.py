"""Keyword search on the CPU tier: the oracle tests/kernels/_lex_ref.py against
a naive BM25 over Python dicts of words, the numpy formulations of
ops/lex_ops.py against the oracle bit for bit, the native terms against
``terms_py``, the FNV constants, ``Lexicon.weights`` and the decidability cap
of the GPU test's cases."""
import math
from collections import Counter

import numpy as np
import pytest
import torch

from lazzaro_amd.core import lexical as LX
from lazzaro_amd.ops import lex_ops as L
from tests.kernels import _lex_ref as R

K1, B = 1.2, 0.75

TEXTS = [
    "Ticket LZ-4812 was closed by Müller; again LZ-4812!",
    "",
    "...!!! --- ???",
    "東京タワー is 333m tall — café CAFÉ café",
    "한국어 test line\x0bx €5 ½ ² İstanbul ǅ",
    "tabs\tand\nnewlines\r\nand separators nbsp",
    "x " * 300 + " ".join(f"w{i}" for i in range(40)),
    " ".join(f"t{i}" for i in range(50)) + " t3 t3 t49 t49",
    "emoji 🙂 and math 𝔘𝔫𝔦 ∑ symbols ©",
    "snake_case camelCase kebab-case dotted.name v1.2.3 0xDEADBEEF",
]


def test_fnv_constants_on_known_words():
    # FNV-1a 32 of "a", "foobar" and "hello" (the published test vectors), folded to 24 bits
    for word, h in (("a", 0xE40C292C), ("foobar", 0xBF9CF968), ("hello", 0x4F9F2CAB)):
        want = (h ^ (h >> 24)) & 0xFFFFFF
        assert LX.term_id(word) == want
        got, dl = LX.lex_terms([word], 8)
        assert int(got[0, 0]) == (want << 8) | 1 and dl[0] == 1 and not got[0, 1:].any()
    assert LX.FNV_OFFSET == 2166136261 and LX.FNV_PRIME == 16777619


def test_native_terms_equal_terms_py():
    from lazzaro_amd._lib import _lzrt
    for W in LX.SLOT_CHOICES + (LX.T_MAX,):
        a, da = _lzrt.lex_terms(TEXTS, W)
        b, db = LX.terms_py(TEXTS, W)
        assert a.dtype == np.uint32 and da.dtype == np.int32 and a.shape == (len(TEXTS), W)
        assert np.array_equal(a, b) and np.array_equal(da, db), W
    s, dl = LX.terms_py(TEXTS, 16)
    assert dl[1] == 0 and dl[2] == 0 and not s[1].any() and not s[2].any()  # empty, punctuation only
    assert LX.words_py(TEXTS[0]) == ["ticket", "lz", "4812", "was", "closed", "by", "muller", "again", "lz", "4812"]
    assert LX.words_py(TEXTS[3])[:3] == ["東", "京", "タワー"] and LX.words_py(TEXTS[3])[-3:] == ["cafe"] * 3
    # a term repeated more than 255 times saturates; dl counts every word
    x = LX.term_id("x")
    row = {int(v) >> 8: int(v) & 255 for v in s[6] if v}
    assert row[x] == 255 and dl[6] == 340 and len(row) == 16
    # more than W distinct terms: the first W by appearance, ascending; later occurrences of a dropped term are words
    first = sorted(LX.term_id(f"t{i}") for i in range(16))
    assert [int(v) >> 8 for v in s[7]] == first and dl[7] == 54
    assert {int(v) >> 8: int(v) & 255 for v in s[7]}[LX.term_id("t3")] == 3
    assert (np.diff((s >> 8).astype(np.int64), axis=1)[(s[:, 1:] != 0)] > 0).all()
    # the query form: 32 terms at most, ascending, tf dropped
    q = LX.query_terms([TEXTS[7], "LZ-4812 lz"])
    assert q.shape == (2, 32) and (q[0] > 0).all() and (np.diff(q[0].astype(np.int64)) > 0).all()
    assert sorted(q[1][q[1] > 0].tolist()) == sorted({LX.term_id("lz"), LX.term_id("4812")})
    assert np.array_equal(LX.as_query_terms(q), q) and np.array_equal(LX.as_query_terms([[5, 3, 3, 0]])[0, :3], [3, 5, 0])


def _naive_bm25(docs, query_words, k1, b):
    """BM25 over Python dicts of words (the textbook form; fp64, its own order)."""
    N = sum(1 for d in docs if d)
    avgdl = sum(len(d) for d in docs) / N
    df = Counter(w for d in docs for w in set(d))
    out = []
    for d in docs:
        tf = Counter(d)
        s = 0.0
        for w in sorted(set(query_words), key=LX.term_id):
            if tf[w]:
                idf = math.log1p((N - df[w] + 0.5) / (df[w] + 0.5))
                s += idf * tf[w] * (k1 + 1) / (tf[w] + k1 * (1 - b + b * len(d) / avgdl))
        out.append(s)
    return np.asarray(out)


def test_oracle_against_naive_bm25_over_words():
    rng = np.random.default_rng(3)
    vocab = [f"w{i}" for i in range(60)]
    docs = [list(rng.choice(vocab, size=int(rng.integers(0, 14)))) for _ in range(200)]
    queries = [list(rng.choice(vocab, size=int(rng.integers(1, 6)))) for _ in range(12)]
    assert len({LX.term_id(w) for w in vocab}) == len(vocab)  # (no collision in this vocabulary)
    slots, dl = LX.terms_py([" ".join(d) for d in docs], 16)  # (at most 13 distinct words: nothing is dropped)
    qt = LX.query_terms([" ".join(q) for q in queries])
    df, N, avgdl = R.stats(slots, dl)
    w = R.weights(qt, df, N)
    sc = R.scores(slots, dl, qt, w, K1, B, avgdl)
    for m, q in enumerate(queries):
        want = _naive_bm25(docs, q, K1, B)
        assert np.allclose(sc[m], want, rtol=1e-6, atol=1e-9)  # (fp32 rounding of s; another association of K)
    # top-k: descending, ties to the lower row, only positive scores
    s, r = R.topk(sc, np.zeros(len(docs), dtype=np.float32), 64)
    for m in range(len(queries)):
        live = r[m] >= 0
        assert (sc[m][r[m][live]] > 0).all() and live.sum() == min(64, (sc[m] > 0).sum())
        key = list(zip(-s[m][live].astype(np.float64), r[m][live]))
        assert key == sorted(key)


def _t(a):
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a)


@pytest.mark.parametrize("n,M,T,W,k,cap", R.SCAN_CASES[:5])
def test_lex_topk_ref_equals_the_oracle(n, M, T, W, k, cap):
    slots, dl, bias = R.columns(n, W, seed=n % 7)
    qt = R.queries(M, T, seed=M)
    df, N, avgdl = R.stats(slots, dl)
    w = R.weights(qt, df, N)
    ws, wr = R.topk(R.scores(slots, dl, qt, w, K1, B, avgdl), bias, k)
    s, r = L.lex_topk(_t(slots), _t(dl), _t(bias), qt, w, k, K1, B, avgdl)  # (CPU tensors: lex_topk_ref)
    assert np.array_equal(r.numpy(), wr) and np.array_equal(s.numpy(), ws)
    # the tables the kernel reads carry the same terms and weights
    utab, uw = L.tile_tables(*L._check_terms(qt, w))
    for m in range(M):
        t, q = divmod(m, L.TILE_Q)
        for j, term in enumerate(qt[m]):
            if term:
                at = np.flatnonzero(utab[t] == term)
                assert at.size and (uw[t, at, q] == w[m, j]).all()
        assert set(utab[t][uw[t, :, q] != 0].tolist()) <= set(qt[m].tolist())  # (and no other term weighs)


def test_fuse_ref_and_decidability_cap_of_the_gpu_cases():
    for n, D, M, P, k, alpha in R.FUSE_CASES:
        I = R.fuse_inputs(n, D, M, P)
        dp = None if alpha == 1.0 else I["dpool"]
        cb = R.blends64(I["X"], I["Q"], dp, I["lpool"], I["slots"], I["dl"], I["qt"], I["w"], alpha, K1, B, I["avgdl"])
        assert R.undecidable(cb, k, D) <= R.CAP * M, (n, D, M, P, k, alpha)
        if D == 768 and P == 16:
            continue  # (one case per shape is enough for the numpy formulation)
        s, r = L.lex_fuse(_t(I["X"]), _t(I["Q"]), None if dp is None else _t(dp), _t(I["lpool"]), _t(I["slots"]),
                          _t(I["dl"]), I["qt"], I["w"], alpha, k, K1, B, I["avgdl"])
        R.check_fused(I["X"], I["Q"], dp, I["lpool"], I["slots"], I["dl"], I["qt"], I["w"], alpha, K1, B, I["avgdl"],
                      k, s.numpy(), r.numpy())
    # the end-to-end tenant of the GPU test: every query decidable (4 queries: the cap allows none)
    X, texts, sal, queries, Q = R.e2e_inputs()
    slots, dl = LX.terms_py(texts, 16)
    qt = LX.query_terms(queries)
    df, N, avgdl = R.stats(slots, dl)
    w = R.weights(qt, df, N)
    for ok in (np.ones(len(texts), bool), sal >= 0.5):
        bias = np.where(ok, 0.0, -np.inf).astype(np.float32)
        _, lp = R.topk(R.scores(slots, dl, qt, w, K1, B, avgdl), bias, 16)
        cos = np.where(ok[None, :], Q.astype(np.float64) @ X.astype(np.float64).T, -np.inf)
        dpool = np.argsort(-cos, axis=1, kind="stable")[:, :16]
        for alpha, dp in ((0.3, dpool), (1.0, None)):
            cb = R.blends64(X, Q, dp, lp, slots, dl, qt, w, alpha, K1, B, avgdl)
            assert R.undecidable(cb, 10, X.shape[1]) == 0


def test_lexicon_weights_against_the_formula():
    from lazzaro_amd.engine.tenant_graph import TenantGraph
    X, texts, sal, queries, _ = R.e2e_inputs()
    g = TenantGraph(device="cpu", dim=X.shape[1])
    g.add_nodes([f"m{i}" for i in range(len(texts))], texts, torch.from_numpy(X), shard=g.shard_id("w"), stored=True)
    lx = g.lexicon()
    slots, dl = LX.terms_py(texts, 16)
    df, N, avgdl = R.stats(slots, dl)
    assert lx.N == N and lx.avgdl == avgdl and lx.covered == len(texts)
    assert dict(zip(lx.df_terms.tolist(), lx.df_counts.tolist())) == df
    qt, w = lx.query(queries + ["zzz unknown", ""])
    assert w.dtype == np.float64 and w.shape == qt.shape == (6, 32)
    for m in range(6):
        for j in range(32):
            t = int(qt[m, j])
            want = math.log1p((N - df.get(t, 0) + 0.5) / (df.get(t, 0) + 0.5)) if t else 0.0
            assert w[m, j] == pytest.approx(want, rel=1e-15, abs=0)
    assert np.array_equal(w, R.weights(qt, df, N))
    assert (w[5] == 0).all() and (w[4][qt[4] > 0] == math.log1p((N + 0.5) / 0.5)).all()
    assert L.lex_tol(768) == (2 * (4 * 12 + 4) + 12) * 2.0 ** -24 and L.LEX_SUM_DEPTH(30) == 8
