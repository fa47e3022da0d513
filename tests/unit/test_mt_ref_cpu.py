"""tests/kernels/_mt_ref.py on its own (no GPU): ``global_ref`` against a
brute-force double loop, ``rerank_ref``'s per-slot contract, ``MtTiles`` (device
"cpu") against the reference's tile content, and the proof that the Gaussian
inputs of tests/kernels/test_mtscan_gpu.py meet the "at most 1 query in 20
undecidable" condition -- evaluated from the reference alone, for exactly the
seeds and shapes the GPU test runs."""
import numpy as np
import pytest

from tests.kernels import _mt_ref as R

NEG_INF = float("-inf")


def _tiny(seed, family):
    rng = np.random.default_rng(seed)
    counts = [5, 0, 1, 9, 3]
    slots = [7, 2, 11, 0, 4]
    ts = R.make_tenants(rng, [c for c in counts if c], [s for c, s in zip(counts, slots) if c], 8, family)
    ts.insert(1, R.Tenant(2, np.zeros((0, 8), np.float32), np.zeros(0, np.float32), np.zeros(0, np.uint8)))
    # rows that matter at this size: a ghost, a free unstored row, an unstored node
    ts[0].kind[1] = R.GHOST
    ts[0].bias[1] = R.l2_bias(ts[0].X[1:2])[0]
    ts[3].bias[2] = NEG_INF
    ts[3].kind[2] = R.FREE
    ts[3].bias[4] = NEG_INF
    Q = (R.grid_queries(rng, 6, 8) if family == "grid" else R.unit_rows(rng, 6, 8)).astype(np.float32)
    if family == "grid":
        Q[0] = ts[0].X[1]  # a query on the ghost: the ghost is its nearest stored row
    return ts, Q


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("family", ["grid", "gauss"])
@pytest.mark.parametrize("k", [1, 3, 16])
def test_global_ref_matches_double_loop(k, family, metric):
    ts, Q = _tiny(3, family)
    S, K, _ = R.Table(ts).global_ref(Q, k, metric)
    for q in range(Q.shape[0]):
        merged = []
        for t in ts:
            own = []
            for r in range(len(t.bias)):
                if t.bias[r] == NEG_INF:
                    continue
                dot = sum(float(Q[q, d]) * float(t.X[r, d]) for d in range(8))
                s = dot + float(t.bias[r])
                if metric == "l2":
                    s = 2.0 * dot + float(t.bias[r]) - sum(float(v) ** 2 for v in Q[q])
                own.append((-s, r))
            own.sort()
            merged += [(ms, (t.slot << 32) | r) for ms, r in own[:k] if t.kind[r] == R.NODE]
        merged.sort()
        merged = merged[:k]
        assert K[q, : len(merged)].tolist() == [m[1] for m in merged]
        assert np.allclose(S[q, : len(merged)], [-m[0] for m in merged], rtol=1e-12, atol=1e-12)
        assert (K[q, len(merged):] == -1).all() and (S[q, len(merged):] == NEG_INF).all()
    if family == "grid" and k == 1:
        assert K[0, 0] >= 0 and K[0, 0] != (7 << 32) | 1  # the ghost's slot is filled from elsewhere


def test_rerank_ref_contract():
    """Ranks by (score desc, key asc) whatever the tile order; a non-node among
    the first k is (-inf, -1) in place and flags the query; holes, -inf rows
    and slots past the live count are (-inf, -1)."""
    ts, Q = _tiny(5, "grid")
    tab = R.Table(ts, sort=False)
    assert tab.t_slot.tolist() == [7, 11, 0, 4]  # list order kept, the zero-row tenant has no tile
    ghost_c = 0 * 256 + 1
    uns_c = 2 * 256 + 2
    cand = np.array([[ghost_c, -1, 2 * 256 + 0, uns_c, 3 * 256 + 1, 1 * 256 + 0, -1, -1]] * Q.shape[0])
    S, K, _, ghost = tab.rerank_ref(Q, cand, 4, "l2")
    ex, _ = tab.exact(Q, "l2")
    for q in range(Q.shape[0]):
        live = [c for c in cand[q] if c >= 0 and ex[q][tab.flat_of_cid([c])[0]] != NEG_INF]
        assert uns_c not in live and ghost_c in live
        f = tab.flat_of_cid(np.array(live))
        o = sorted(range(len(live)), key=lambda j: (-ex[q][f[j]], tab.key[f[j]]))[:4]
        for rank, j in enumerate(o):
            if tab.kind[f[j]] != R.NODE:
                assert K[q, rank] == -1 and S[q, rank] == NEG_INF
            else:
                assert K[q, rank] == tab.key[f[j]] and S[q, rank] == ex[q][f[j]]
        assert (K[q, len(o):] == -1).all() and (S[q, len(o):] == NEG_INF).all()
        assert bool(ghost[q]) == any(tab.kind[f[j]] != R.NODE for j in o)
    # query 0 sits on the ghost (7, 1); its planted copy (4, 1) ties and has the smaller key
    assert ghost[0] and K[0, 0] == (4 << 32) | 1 and K[0, 1] == -1 and S[0, 0] == 0.0
    S, K, _, _ = tab.rerank_ref(Q, np.full((Q.shape[0], 5), -1), 3, "ip")
    assert (K == -1).all() and (S == NEG_INF).all()


def test_cand_ref_membership():
    ts, Q = _tiny(8, "grid")
    tab = R.Table(ts)
    s, _ = tab.scan(Q, 2.0, 64)
    lists = tab.cand_ref(Q, 2.0, np.full(Q.shape[0], NEG_INF), 64)
    for ids, sc in lists:
        assert ids.size == int(tab.stored.sum()) and np.isfinite(sc).all()
    assert all(ids.size == 0 for ids, _ in tab.cand_ref(Q, 2.0, np.full(Q.shape[0], np.inf), 64))
    thr = np.sort(s[:, tab.stored], axis=1)[:, -3]
    for q, (ids, sc) in enumerate(tab.cand_ref(Q, 2.0, thr, 64)):
        assert ids.size >= 3 and (sc >= thr[q]).all() and ids.size == int((s[q][tab.stored] >= thr[q]).sum())


def test_mt_tiles_match_reference_layout():
    """MtTiles from an unsorted slot list with a zero-row tenant: tiles in
    ascending slot order, addresses, counts and the sample as the reference
    lays them out."""
    from lazzaro_amd.ops.search import MtTiles
    rng = np.random.default_rng(2)
    counts = [700, 1, 0, 257, 64, 256, 65]
    slots = np.array([9, 4, 6, 30, 2, 17, 1], np.int64)
    ld = 72
    ts = [R.Tenant(int(s), np.zeros((n, 64), np.float32), np.zeros(n, np.float32), np.ones(n, np.uint8))
          for n, s in zip(counts, slots)]
    e16 = (np.arange(len(counts), dtype=np.int64) + 1) << 24
    bias = e16 + (1 << 23)
    t = MtTiles(slots, np.array(counts), e16, bias, ld, "cpu")
    tab = R.Table(ts)
    assert t.n_tiles == tab.n_tiles and t.rows == tab.N
    assert t.slot.tolist() == tab.t_slot.tolist() == sorted(tab.t_slot.tolist())
    assert t.row0.tolist() == tab.t_row0.tolist() and t.n.tolist() == tab.t_n.tolist()
    base = {int(s): (int(e), int(b)) for s, e, b in zip(slots, e16, bias)}
    assert t.x.tolist() == [base[int(s)][0] + int(r0) * ld * 2 for s, r0 in zip(tab.t_slot, tab.t_row0)]
    assert t.b.tolist() == [base[int(s)][1] + int(r0) * 4 for s, r0 in zip(tab.t_slot, tab.t_row0)]
    s_tile, s_row, _, _ = tab.sample_ref(ld)
    assert t.n_sample == s_tile.size
    assert t.s_tile.tolist() == s_tile.tolist() and t.s_row.tolist() == s_row.tolist()
    # candidate-id order is key order
    assert (np.diff(tab.key[np.argsort(tab.cid)]) > 0).all()


@pytest.mark.parametrize("D,norm,k", [(64, 1.0, 6), (64, 1.0, 10), (768, 1.0, 6), (768, 1.0, 10),
                                      (64, 4.0, 10), (768, 4.0, 10)])
def test_gpu_gaussian_inputs_are_decidable(D, norm, k):
    """The inputs of test_mtscan_gpu.py::test_mt_topk_gauss_gpu: at most 1 query
    in 20 is undecidable (a condition on the inputs, shown here from the
    reference alone)."""
    ts, Q = R.e2e_gauss(D, norm)
    dec = R.Table(ts).decidable(Q, k, "l2", D)
    print("decidable", int(dec.sum()), "of", dec.size)
    assert (~dec).sum() * 20 <= dec.size


def test_margin_table_is_covered_by_its_sample():
    """The threshold-margin table of the GPU test: for at least every second
    query the 16th best row of the sample is the 16th best row of the whole table --
    the sampled threshold is then the score of a row the candidate pass must
    keep, and nothing but the margin allows for the two kernels' rounding."""
    for D, norm in ((64, 4.0), (768, 4.0), (768, 1.0)):
        ts, Q = R.margin_gauss(D, norm)
        tab = R.Table(ts)
        s_tile, s_row, _, sb = tab.sample_ref(D)
        assert int(np.isfinite(sb).sum()) > R.KC
        sample = tab.t_flat0[s_tile] + s_row
        sample = sample[tab.stored[sample]]
        f = np.nonzero(tab.stored)[0]
        sn, _ = tab.scan(Q, 2.0, D)
        hit = 0
        for q in range(Q.shape[0]):
            kth = f[R.order(sn[q][f], tab.key[f])[R.KC - 1]]
            kth_s = sample[R.order(sn[q][sample], tab.key[sample])[R.KC - 1]]
            hit += int(kth == kth_s)
        print("sample 16th == table 16th for", hit, "of", Q.shape[0])
        assert hit * 2 >= Q.shape[0]
