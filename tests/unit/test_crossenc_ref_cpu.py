"""The cross-encoder re-ranker's oracle and CPU tier (no GPU): the oracle's
pair assembly against a per-token loop, its forward against HuggingFace's
``BertForSequenceClassification`` fed ``token_type_ids`` (through the new
safetensors loader), the torch formulations against the oracle, the head's
tolerance against an fp32 emulation of the kernel's order, and the
decidability of the cases the GPU tests run."""
import numpy as np
import pytest
import torch

from lazzaro_amd.models.cross_encoder import CE_TOKEN_BUDGET, CrossEncoder
from lazzaro_amd.models.encoder import get_config
from lazzaro_amd.ops import crossenc_ops as X
from tests.kernels import _crossenc_ref as R
from tests.kernels import _encoder_bounds as EB

CFG = get_config("tiny")
L = 32


def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t if dtype is None else t.to(dtype)


def _case(M=3, P=4, n=12, seed=0, L_=L):
    return R.token_case(M, P, n, L_, CFG.vocab, seed, CFG.max_pos)


# ---------------------------------------------------------------- the oracle itself
def test_pair_assembly_against_a_per_token_loop():
    rows, qtok, qlen, tok, dlen = _case(M=4, P=5, n=14, seed=3)
    pairs = R.pair_assembly(rows, qtok, qlen, tok, dlen, CFG.max_pos, L)
    u = tok.view(np.uint16)
    ids, pos, types, lens = [], [], [], []
    for m in range(rows.shape[0]):
        for j in range(rows.shape[1]):
            r = rows[m, j]
            ql = int(qlen[m]) if r >= 0 else 0
            dl = min(int(dlen[r]), CFG.max_pos - 3 - ql) if r >= 0 else 0
            n_tok = ql + dl + 3
            lens.append(n_tok)
            for p in range(n_tok):
                if p == 0:
                    ids.append(R.CLS)
                elif p <= ql:
                    ids.append(int(qtok[m, p - 1]))
                elif p == ql + 1 or p == n_tok - 1:
                    ids.append(R.SEP)
                else:
                    ids.append(int(u[r, p - ql - 2]))
                pos.append(p)
                types.append(0 if p <= ql + 1 else 1)
    assert pairs.lens.tolist() == lens and pairs.T == sum(lens) and pairs.S_max == max(lens)
    assert pairs.cu.tolist() == np.concatenate([[0], np.cumsum(lens)]).tolist()
    assert pairs.ids.tolist() == ids and pairs.pos.tolist() == pos and pairs.types.tolist() == types
    # the recipe holds what it promises: the truncation, an empty query, an empty and a full memory, empty slots
    assert qlen[0] == 64 and qlen[1] == 0 and dlen[0] == 0 and dlen[1] == L and (rows < 0).any()
    assert pairs.lens[0] == 64 + min(L, CFG.max_pos - 3 - 64) + 3 and 3 in lens


def _hf_classifier(path, seed=0):
    transformers = pytest.importorskip("transformers")
    pytest.importorskip("safetensors")
    from safetensors.torch import save_file
    c = CFG
    cfg = transformers.BertConfig(vocab_size=c.vocab, hidden_size=c.hidden, num_hidden_layers=c.layers,
                                  num_attention_heads=c.heads, intermediate_size=c.ffn,
                                  max_position_embeddings=c.max_pos, hidden_act="gelu", layer_norm_eps=c.eps,
                                  type_vocab_size=2, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
                                  num_labels=1)
    torch.manual_seed(seed)
    m = transformers.BertForSequenceClassification(cfg).eval()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():  # every bias and LayerNorm randomised, as test_encoder_parity's hf_bert does
        for n, p in m.named_parameters():
            if n.endswith("LayerNorm.weight"):
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
            elif n.endswith("bias"):
                p.copy_(0.02 * torch.randn(p.shape, generator=g))
    save_file({k: v.contiguous() for k, v in m.state_dict().items()}, path)
    return m


def test_forward_matches_hf_sequence_classification(tmp_path):
    path = str(tmp_path / "ce.safetensors")
    hf = _hf_classifier(path).double()
    ce = CrossEncoder("tiny", device="cpu", weights=path, dtype=torch.float32)
    rows, qtok, qlen, tok, dlen = _case(M=2, P=3, n=10, seed=5)
    pairs = R.pair_assembly(rows, qtok, qlen, tok, dlen, CFG.max_pos, L)
    B, S = len(pairs.lens), pairs.S_max
    ids = torch.zeros((B, S), dtype=torch.long)
    tt = torch.zeros((B, S), dtype=torch.long)
    mask = torch.zeros((B, S), dtype=torch.long)
    for b in range(B):
        a, e = int(pairs.cu[b]), int(pairs.cu[b + 1])
        ids[b, :e - a], tt[b, :e - a], mask[b, :e - a] = _t(pairs.ids[a:e]).long(), _t(pairs.types[a:e]).long(), 1
    with torch.no_grad():
        want = hf(input_ids=ids, attention_mask=mask, token_type_ids=tt).logits.reshape(-1)
    got, _ = R.forward64(R.params64(ce.p), CFG, pairs)
    assert float((got - want).abs().max()) < 1e-9 and float(want.std()) > 1e-3  # both fp64
    # and the CPU tier through the public forward (fp32: see test_cpu_tier_against_the_oracle for the bound)
    s, r, lg = ce.rerank(_t(rows), qtok, qlen, _t(tok), _t(dlen), 3, L)
    live = rows.reshape(-1) >= 0
    assert float((lg.reshape(-1).double()[_t(live)] - want[_t(live)]).abs().max()) < 1e-4


def test_loader_rejects_a_checkpoint_without_a_one_label_head(tmp_path):
    from safetensors.torch import save_file
    path = str(tmp_path / "plain.safetensors")
    save_file({"bert.embeddings.word_embeddings.weight": torch.zeros(4, 4)}, path)
    with pytest.raises(ValueError, match="BertForSequenceClassification"):
        CrossEncoder("tiny", device="cpu", weights=path)


# ---------------------------------------------------------------- the torch formulations
def test_lens_and_tokens_equal_the_oracle():
    for B in (1, 5, 1025):
        rows, qlen, dlen = R.lens_case(B)
        n = len(dlen)
        tok = np.zeros((n, 64), dtype=np.int16)
        pairs = R.pair_assembly(rows, np.zeros((len(qlen), 64), np.int32), qlen, tok, dlen, 128, 64)
        lens, cu, stat = X.ce_lens(_t(rows), _t(qlen), _t(dlen), 128, 64)
        assert lens.dtype == cu.dtype == stat.dtype == torch.int32
        assert lens.tolist() == pairs.lens.tolist() and cu.tolist() == pairs.cu.tolist()
        assert stat.tolist() == [pairs.T, pairs.S_max]
    rows, qtok, qlen, tok, dlen = _case(M=4, P=5, n=14, seed=3)
    pairs = R.pair_assembly(rows, qtok, qlen, tok, dlen, CFG.max_pos, L)
    ids, pos, types = X.pair_tokens_ref(_t(rows), _t(qtok), _t(qlen), _t(tok), _t(dlen), CFG.max_pos, L, R.CLS, R.SEP,
                                        CFG.vocab)
    assert ids.tolist() == pairs.ids.tolist() and pos.tolist() == pairs.pos.tolist()
    assert types.tolist() == pairs.types.tolist()


def test_embed_formulation_within_the_layernorm_bound():
    ce = CrossEncoder("tiny", device="cpu", dtype=torch.float32, seed=2)
    p = ce.p
    p["emb_g"] = 1.0 + 0.1 * torch.randn(CFG.hidden, generator=torch.Generator().manual_seed(1))
    p["emb_b"] = 0.02 * torch.randn(CFG.hidden, generator=torch.Generator().manual_seed(2))
    rows, qtok, qlen, tok, dlen = _case(seed=7)
    pairs = R.pair_assembly(rows, qtok, qlen, tok, dlen, CFG.max_pos, L)
    y, ids, pos, types = X.ce_embed_ln(_t(rows), _t(qtok), _t(qlen), _t(tok), _t(dlen), _t(pairs.cu), pairs.T,
                                       CFG.max_pos, L, R.CLS, R.SEP, p["word"], p["pos"], p["type"], p["emb_g"],
                                       p["emb_b"], CFG.eps, debug=True)
    assert ids.tolist() == pairs.ids.tolist() and types.tolist() == pairs.types.tolist()
    v, _ = R.embed64(R.params64(p), pairs.ids, pairs.pos, pairs.types, CFG.eps)
    ref, bound = EB._ln_bound(v, p["emb_g"], p["emb_b"], CFG.eps)
    EB.assert_within(y, ref, bound, "ce_embed_ln (CPU)")
    # the type row matters: with the types flipped the rows leave the bound
    y2 = X.ce_embed_ln_ref(_t(rows), _t(qtok), _t(qlen), _t(tok), _t(dlen), None, pairs.T, CFG.max_pos, L, R.CLS,
                           R.SEP, p["word"], p["pos"], p["type"].flip(0), p["emb_g"], p["emb_b"], CFG.eps)
    assert EB.worst_ratio(y2, ref, bound) > 2.0


# fp32 against fp64 through two layers: every GEMM sums K <= 256 products of O(1) activations (LayerNorm
# output) and |w| ~ 0.02 weights, so each adds at most K 2^-24 |x|.|w| ~ 256 * 6e-8 * 3 ~ 5e-5 in the worst
# case and a square root of that in practice; LayerNorm renormalises, and the logit weighs the pooled
# vector by sum |wc| ~ 2. 1e-4 absolute on the logit covers the worst case of the last stage and is three
# orders of magnitude below the logits' spread here.
CPU_TIER_TOL = 1e-4


def test_cpu_tier_against_the_oracle():
    ce = CrossEncoder("tiny", device="cpu", dtype=torch.float32, seed=4)
    rows, qtok, qlen, tok, dlen = _case(M=3, P=4, n=12, seed=9)
    n = len(dlen)
    pairs = R.pair_assembly(rows, qtok, qlen, tok, dlen, CFG.max_pos, L)
    want, _ = R.forward64(R.params64(ce.p), CFG, pairs)
    want = R.pool_logits(want.numpy(), rows, n)
    for cls_last in (True, False):
        ce.CLS_LAST = cls_last
        s, r, lg = ce.rerank(_t(rows), qtok, qlen, _t(tok), _t(dlen), 3, L)
        got = lg.double().numpy()
        assert np.array_equal(np.isinf(got), np.isinf(want))
        live = ~np.isinf(want)
        assert np.abs(got[live] - want[live]).max() <= CPU_TIER_TOL
        # the selection: the oracle's over the tier's own logits
        ws, wr = R.select(got, rows, 3)
        assert np.array_equal(r.numpy(), wr) and np.array_equal(s.double().numpy(), ws)
    assert (rows[-1] < 0).any() and lg[-1, 0] == float("-inf")


def test_selection_ties_go_to_the_lower_row_and_padding():
    logits = torch.tensor([[0.5, 0.25, 0.5, float("-inf"), 0.5], [float("-inf")] * 5, [1.0, -1.0, 0.0, 0.0, -0.0]])
    rows = torch.tensor([[9, 3, 4, -1, 7], [-1, -1, -1, -1, -1], [5, 4, 3, 2, 1]])
    s, r = X.select_ref(logits, rows, 5)
    ws, wr = R.select(logits.numpy(), rows.numpy(), 5)
    assert r.tolist() == wr.tolist() == [[4, 7, 9, 3, -1], [-1] * 5, [5, 1, 2, 3, 4]]
    assert np.array_equal(s.double().numpy(), ws)


def test_chunks_respect_the_token_budget_and_the_pair_limit():
    qlen = np.full(3000, 64, dtype=np.int32)
    ch = CrossEncoder.chunks(qlen, 64, 128)
    assert ch[0][0] == 0 and ch[-1][1] == 3000 and all(a[1] == b[0] for a, b in zip(ch, ch[1:]))
    assert all((b - a) * 64 * (3 + 64 + 128) <= CE_TOKEN_BUDGET and (b - a) * 64 <= X.MAX_PAIRS for a, b in ch)
    assert CrossEncoder.chunks(qlen[:1], 64, 128, budget=10) == [(0, 1)]  # one query at least
    assert CrossEncoder.chunks(qlen[:0], 16, 64) == []


# ---------------------------------------------------------------- the head's tolerance
def _head_emulation(dense, wc, bc):
    """crossenc.hip's order in fp32: lane ``part`` of 16 takes the float4
    indices d4 == part (mod 16) ascending, one fma each (emulated as a
    rounded product and a rounded add: no further from fp64 than two
    roundings where the kernel makes one), folds by xor 8, 4, 2, 1."""
    x = np.tanh(dense.float().numpy().astype(np.float64)).astype(np.float32)
    w = wc.numpy()
    H = x.shape[1]
    out = np.zeros(x.shape[0], dtype=np.float32)
    for b in range(x.shape[0]):
        part = np.zeros(16, dtype=np.float32)
        for lane in range(16):
            acc = np.float32(0)
            for d4 in range(lane, H // 4, 16):
                for u in range(4):
                    acc = np.float32(acc + np.float32(w[4 * d4 + u] * x[b, 4 * d4 + u]))
            part[lane] = acc
        for o in (8, 4, 2, 1):
            part = (part + part[np.arange(16) ^ o]).astype(np.float32)
        out[b] = np.float32(part[0] + bc.numpy()[0])
    return out


@pytest.mark.parametrize("H", [128, 384, 1024])
def test_head_tolerance_holds_for_an_fp32_emulation_and_catches_a_corrupted_element(H):
    dense, rows, wc, bc, n = R.head_case(H, 2, 5, "plain")
    want = R.head64(dense, wc, bc).numpy()
    tol = X.ce_head_tol(H, float(wc.double().abs().sum()), float(bc[0]))
    assert np.abs(_head_emulation(dense, wc, bc).astype(np.float64) - want).max() <= tol
    # the torch formulation sums in another order: the same bound
    _, _, lg = X.ce_head_select(dense.float(), rows, wc, bc, 1, n)
    assert np.abs(lg.reshape(-1).double().numpy() - want).max() <= tol
    bad = dense.clone()
    i = int(wc.abs().argmax())
    bad[0, i] = bad[0, i] + (1.0 if float(bad[0, i]) < 0 else -1.0)  # one element of one pooler row
    err = np.abs(_head_emulation(bad, wc, bc).astype(np.float64) - want)
    assert err[0] > 2 * tol and err[1:].max() <= tol


@pytest.mark.parametrize("H,M,P,k,what", R.HEAD_CASES)
def test_head_cases_are_decidable(H, M, P, k, what):
    """The GPU test compares the device's rows with the fp64 selection: any
    two distinct logits of a query lie more than 4 x the tolerance apart (2 x
    for each, the GPU test's margin), and the duplicated pooler rows give
    equal logits, so the order is decided by the contract alone."""
    dense, rows, wc, bc, n = R.head_case(H, M, P, what)
    tol = X.ce_head_tol(H, float(wc.double().abs().sum()), float(bc[0]))
    lg = R.pool_logits(R.head64(dense, wc, bc).numpy(), rows.numpy(), n)
    for m in range(M):
        live = np.sort(lg[m][~np.isinf(lg[m])])
        gaps = np.diff(live)
        assert ((gaps == 0) | (gaps > 4 * tol)).all()
        if what == "ties":
            assert lg[m, 0] == lg[m, 1] == lg[m, 3] and np.isinf(lg[m, 2]) and (gaps == 0).sum() == 2
    if what == "ties":
        assert np.isinf(lg[M - 1, P - 1])
