"""Cross-encoder re-ranking on the device (csrc/kernels/crossenc.hip) against
the fp64 oracle tests/kernels/_crossenc_ref.py: ``ce_lens_kernel`` exactly,
``ce_embed_ln_kernel``'s tokens exactly and its rows within the embedding +
LayerNorm bound (and bit for bit against ``E.embed_ln`` when the type rows are
equal), ``ce_head_select_kernel``'s logits within ``2 x ce_head_tol`` and its
selection exactly, and ``store_search(rerank=)`` end to end against the CPU
fp32 tier (which tests/unit/test_crossenc_ref_cpu.py pins to HuggingFace)."""
import functools

import numpy as np
import pytest
import torch

from lazzaro_amd.models.cross_encoder import CrossEncoder
from lazzaro_amd.ops import crossenc_ops as X
from lazzaro_amd.ops import encoder_ops as E
from tests.kernels import _crossenc_ref as R
from tests.kernels import _encoder_bounds as EB

pytestmark = pytest.mark.gpu
DEV = "cuda"
VOCAB, MAX_POS = 4096, 128

# |logit(device, bf16) - logit(CPU tier, fp32 over the same bf16-rounded weights)|, random-init weights. Not
# derivable (bf16 roundings pass through every layer), so: the largest deviation measured on an MI355X over
# this file's end-to-end cases, times 4 because it moves with the weight seed.
#   tiny (2 layers, H 128): measured 7.04e-4 (plain and lexical; where: 4.82e-4), logit spread 1.7e-3
#   minilm-l6 (6 layers, H 384): measured 4.52e-3, logit spread 1.8e-2
# Random-init logits lie close together, so these are large beside their spread; they are the size the token
# states' bf16 error gives (test_encoder_parity_gpu.py accepts 2e-2 relative per token at minilm-l6): about
# 1e-2 per element of h_cls, times |Wp| ~ 0.02 sqrt(H) into the pooler, times sum-in-quadrature of wc again.
E2E_TOL = {"tiny": 4 * 7.04e-4, "minilm-l6": 4 * 4.52e-3}


def _dev(a):
    return (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(DEV)


# ---------------------------------------------------------------- ce_lens_kernel
@pytest.mark.parametrize("B", [1, 5, 1025])
def test_lens_equal_the_oracle(B):
    rows, qlen, dlen = R.lens_case(B)
    pairs = R.pair_assembly(rows, np.zeros((len(qlen), 64), np.int32), qlen, np.zeros((len(dlen), 64), np.int16), dlen,
                            MAX_POS, 64)
    lens, cu, stat = X.ce_lens(_dev(rows), _dev(qlen), _dev(dlen), MAX_POS, 64)
    assert lens.is_cuda and lens.dtype == cu.dtype == stat.dtype == torch.int32
    assert lens.cpu().tolist() == pairs.lens.tolist()
    assert cu.cpu().tolist() == pairs.cu.tolist()
    assert stat.cpu().tolist() == [pairs.T, pairs.S_max]
    if B == 1:  # ql = 64 with dlen = 64: the max_pos truncation
        assert pairs.lens.tolist() == [64 + 61 + 3]


# ---------------------------------------------------------------- ce_embed_ln_kernel
@functools.lru_cache(maxsize=None)
def _tables(H):
    g = torch.Generator().manual_seed(H)
    bf = torch.bfloat16
    return dict(word=(torch.randn(VOCAB, H, generator=g) * 0.05).to(bf),
                pos=(torch.randn(MAX_POS, H, generator=g) * 0.05).to(bf),
                type=(torch.randn(2, H, generator=g) * 0.05).to(bf), emb_g=1.0 + 0.1 * torch.randn(H, generator=g),
                emb_b=0.02 * torch.randn(H, generator=g))


@pytest.mark.parametrize("H,L", [(128, 32), (384, 64), (1024, 128)])
def test_embed_tokens_equal_and_rows_within_the_bound(H, L):
    t = _tables(H)
    rows, qtok, qlen, tok, dlen = R.token_case(5, 7, 30, L, VOCAB, seed=H, max_pos=MAX_POS)
    pairs = R.pair_assembly(rows, qtok, qlen, tok, dlen, MAX_POS, L)
    d = {k: _dev(v) for k, v in t.items()}
    args = (_dev(rows), _dev(qtok), _dev(qlen), _dev(tok), _dev(dlen))
    lens, cu, stat = X.ce_lens(args[0], args[2], args[4], MAX_POS, L)
    assert stat.cpu().tolist() == [pairs.T, pairs.S_max] and cu.cpu().tolist() == pairs.cu.tolist()
    y, ids, pos, types = X.ce_embed_ln(*args, cu, pairs.T, MAX_POS, L, R.CLS, R.SEP, d["word"], d["pos"], d["type"],
                                       d["emb_g"], d["emb_b"], 1e-12, debug=True)
    assert y.dtype == torch.bfloat16 and tuple(y.shape) == (pairs.T, H)
    assert ids.cpu().tolist() == pairs.ids.tolist() and pos.cpu().tolist() == pairs.pos.tolist()
    assert types.cpu().tolist() == pairs.types.tolist()
    v, _ = R.embed64({k: a.double() for k, a in t.items()}, pairs.ids, pairs.pos, pairs.types, 1e-12)
    ref, bound = EB._ln_bound(v, t["emb_g"], t["emb_b"], 1e-12)
    EB.assert_within(y.cpu(), ref, EB.GPU_MARGIN * bound, f"ce_embed_ln H={H}")
    # without the debug outputs: the same rows
    y2 = X.ce_embed_ln(*args, cu, pairs.T, MAX_POS, L, R.CLS, R.SEP, d["word"], d["pos"], d["type"], d["emb_g"],
                       d["emb_b"], 1e-12)
    assert torch.equal(y2, y)
    # both type rows equal: bit for bit E.embed_ln over the host-assembled ids and positions
    same = d["type"][:1].repeat(2, 1).contiguous()
    y3 = X.ce_embed_ln(*args, cu, pairs.T, MAX_POS, L, R.CLS, R.SEP, d["word"], d["pos"], same, d["emb_g"], d["emb_b"],
                       1e-12)
    y4 = E.embed_ln(_dev(pairs.ids), pairs.S_max, d["word"], d["pos"], same, d["emb_g"], d["emb_b"], 1e-12,
                    pos=_dev(pairs.pos))
    assert torch.equal(y3, y4) and not torch.equal(y3, y)


# ---------------------------------------------------------------- ce_head_select_kernel
@pytest.mark.parametrize("H,M,P,k,what", R.HEAD_CASES)
def test_head_logits_and_selection(H, M, P, k, what):
    dense, rows, wc, bc, n = R.head_case(H, M, P, what)
    want = R.pool_logits(R.head64(dense, wc, bc).numpy(), rows.numpy(), n)
    tol = X.ce_head_tol(H, float(wc.double().abs().sum()), float(bc[0]))
    s, r, lg = X.ce_head_select(_dev(dense), _dev(rows), _dev(wc), _dev(bc), k, n)
    assert s.dtype == lg.dtype == torch.float32 and r.dtype == torch.long and tuple(lg.shape) == (M, P)
    got = lg.cpu().double().numpy()
    assert np.array_equal(np.isinf(got), np.isinf(want)) and (got[np.isinf(got)] < 0).all()
    live = ~np.isinf(want)
    worst = np.abs(got[live] - want[live]).max()
    print(f"head H={H} P={P}: worst |logit - fp64| = {worst:.3g}, tol = {tol:.3g}")
    assert worst <= 2 * tol
    # the selection: the oracle's over the device's own logits -- and, the cases being decidable
    # (test_crossenc_ref_cpu.py), over the fp64 logits too
    ws, wr = R.select(got, rows.numpy(), k)
    assert np.array_equal(r.cpu().numpy(), wr) and np.array_equal(s.cpu().double().numpy(), ws)
    assert np.array_equal(r.cpu().numpy(), R.select(want, rows.numpy(), k)[1])
    if what == "ties":
        assert (got[:, 0] == got[:, 1]).all()  # duplicated pooler rows: equal bits


def test_head_limit_one_of_one_and_a_strided_input():
    dense, rows, wc, bc, n = R.head_case(128, 3, 5, "plain")
    wide = torch.zeros((15, 136), dtype=torch.bfloat16, device=DEV)
    wide[:, :128] = _dev(dense)
    a = X.ce_head_select(_dev(dense), _dev(rows), _dev(wc), _dev(bc), 2, n)
    b = X.ce_head_select(wide[:, :128], _dev(rows), _dev(wc), _dev(bc), 2, n)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    s, r, lg = X.ce_head_select(_dev(dense[:1]), _dev(rows[:1, :1]), _dev(wc), _dev(bc), 1, n)
    assert r.cpu().tolist() == [[int(rows[0, 0])]] and float(s[0, 0]) == float(a[2][0, 0]) == float(lg[0, 0])


# ---------------------------------------------------------------- end to end
WORDS = ["alpha", "beta", "gamma", "router", "kernel", "memory", "garden", "violin", "harbor", "lantern", "orchid",
         "quartz", "ticket", "billing", "invoice", "sunrise"]
QUERIES = ["which violin does the orchid garden prefer?", "router kernel memory", ""]


def _cpu_tier(ce):
    """The CPU fp32 tier over the device's own (bf16-rounded) parameters."""
    cpu = CrossEncoder(ce.cfg, device="cpu", dtype=torch.float32)
    for k, v in ce.p.items():
        cpu.p[k] = v.detach().cpu().float()
    return cpu


@functools.lru_cache(maxsize=None)
def _tenant():
    from lazzaro_amd.engine.tenant_graph import TenantGraph
    n, D = 40, 64
    rng = np.random.default_rng(5)
    texts = [" ".join(rng.choice(WORDS, size=int(rng.integers(1, 12)))) for _ in range(n)]
    texts[7] = " ".join(WORDS * 9)  # longer than L
    Xr = rng.standard_normal((n, D)).astype(np.float32)
    Xr /= np.linalg.norm(Xr, axis=1, keepdims=True)
    g = TenantGraph(device=DEV, dim=D, capacity=n + 8)
    g.add_nodes([f"m{i}" for i in range(n)], texts, torch.from_numpy(Xr), shard=g.shard_id("w"),
                types=["preference" if i % 2 == 0 else "semantic" for i in range(n)],
                sal=torch.linspace(0.05, 0.95, n), stored=True)
    g.reranker = CrossEncoder("tiny", device=DEV)
    Q = (Xr[[3, 17, 30]] + 0.3 * rng.standard_normal((3, D)) / np.sqrt(D)).astype(np.float32)
    return g, _dev(Q), _cpu_tier(g.reranker)


@pytest.mark.parametrize("inner", [{}, {"where": {"types": ["preference"]}}, {"lexical": 0.5}],
                         ids=["plain", "where", "lexical"])
def test_store_search_rerank_end_to_end(inner):
    g, Q, cpu = _tenant()
    M, P, k = 3, 5, 3
    terms = {"query_terms": QUERIES} if "lexical" in inner else {}
    s, r, lg = g.store_search_rerank(Q, k, "l2", rerank=P, query_tokens=QUERIES, **inner, **terms)
    assert s.is_cuda and tuple(s.shape) == tuple(r.shape) == (M, k) and tuple(lg.shape) == (M, P)
    # the pool is the inner options' own search
    _, pool = g.store_search(Q, P, "l2", node_rows=True, **inner, **terms)
    assert torch.equal(torch.isinf(lg), pool < 0) and (pool >= 0).any()
    # the rows: the oracle's selection over the returned logits
    got = lg.cpu().double().numpy()
    ws, wr = R.select(got, pool.cpu().numpy(), k)
    assert np.array_equal(r.cpu().numpy(), wr) and np.array_equal(s.cpu().double().numpy(), ws)
    s2, r2 = g.store_search(Q, k, "l2", rerank=P, query_tokens=QUERIES, **inner, **terms)
    assert torch.equal(r2, r) and torch.equal(s2, s)
    # the logits: the CPU fp32 tier over the same pool and the same token column
    col = g.token_column()
    qtok, qlen = X.as_query_tokens(QUERIES, g.reranker.tokenizer)
    _, _, want = cpu.rerank(pool.cpu(), qtok, qlen, col.tok.cpu(), col.dlen.cpu(), k, col.L, g.n)
    want = want.double().numpy()
    live = ~np.isinf(want)
    worst = np.abs(got[live] - want[live]).max()
    print(f"end to end (tiny, {list(inner) or 'plain'}): worst |logit - CPU tier| = {worst:.3g}, "
          f"logit spread {np.ptp(want[live]):.3g}")
    assert worst <= E2E_TOL["tiny"]
    assert int(col.dlen[7]) == col.L and int(qlen[2]) == 0


def test_minilm_l6_against_the_cpu_tier():
    ce = CrossEncoder("minilm-l6", device=DEV)
    cpu = _cpu_tier(ce)
    L = 64
    rows, qtok, qlen, tok, dlen = R.token_case(2, 4, 12, L, ce.cfg.vocab, seed=1, max_pos=ce.cfg.max_pos)
    s, r, lg = ce.rerank(_dev(rows), qtok, qlen, _dev(tok), _dev(dlen), 3, L)
    _, _, want = cpu.rerank(torch.from_numpy(rows), qtok, qlen, torch.from_numpy(tok), torch.from_numpy(dlen), 3, L)
    got, want = lg.cpu().double().numpy(), want.double().numpy()
    assert np.array_equal(np.isinf(got), np.isinf(want))
    live = ~np.isinf(want)
    worst = np.abs(got[live] - want[live]).max()
    print(f"end to end (minilm-l6): worst |logit - CPU tier| = {worst:.3g}, logit spread {np.ptp(want[live]):.3g}")
    assert worst <= E2E_TOL["minilm-l6"]
    ws, wr = R.select(got, rows, 3)
    assert np.array_equal(r.cpu().numpy(), wr) and np.array_equal(s.cpu().double().numpy(), ws)


def test_chunked_queries_equal_one_call(monkeypatch):
    """A token budget that cuts the batch into one query per chunk gives the
    pools and shapes of one call; a GEMM of another height may sum in another
    order, so the logits agree within twice the end-to-end tolerance (each
    lies within one of the CPU tier)."""
    import lazzaro_amd.models.cross_encoder as cemod
    g, Q, _ = _tenant()
    a = g.store_search_rerank(Q, 3, "l2", rerank=5, query_tokens=QUERIES)
    real = cemod.CrossEncoder.chunks
    seen = []
    monkeypatch.setattr(cemod.CrossEncoder, "chunks",
                        staticmethod(lambda qlen, P, L, budget=0: seen.append(real(qlen, P, L, 1)) or seen[-1]))
    b = g.store_search_rerank(Q, 3, "l2", rerank=5, query_tokens=QUERIES)
    assert seen == [[(0, 1), (1, 2), (2, 3)]]
    assert all(x.shape == y.shape and x.dtype == y.dtype for x, y in zip(a, b))
    assert torch.equal(torch.isinf(a[2]), torch.isinf(b[2]))
    live = ~torch.isinf(a[2])
    assert float((a[2][live] - b[2][live]).abs().max()) <= 2 * E2E_TOL["tiny"]
    ws, wr = R.select(b[2].cpu().double().numpy(), g.store_search(Q, 5, "l2", node_rows=True)[1].cpu().numpy(), 3)
    assert np.array_equal(b[1].cpu().numpy(), wr)
