"""``lzk_mmr_select`` (csrc/kernels/mmr.hip) against the fp64 oracle of
tests/kernels/_mmr_ref.py, at the smallest shapes where each part of the
kernel can go wrong, and ``store_search(..., diversity=)`` end to end on a
GPU tenant."""
import functools

import numpy as np
import pytest
import torch

from lazzaro_amd.ops.mmr_ops import mmr_select
from tests.kernels._mmr_ref import check_against_ref, check_rule1, recipe

pytestmark = pytest.mark.gpu
DEV = "cuda"


@functools.lru_cache(maxsize=None)
def _case(D, F, M=128, n=2048, seed=0):
    return recipe(D, F, M=M, n=n, seed=seed)


def _select(X, Q, cand, k, delta):
    """``X``: a numpy array, or a tensor already laid out on the device."""
    Xd = X if torch.is_tensor(X) else torch.from_numpy(X).to(DEV)
    pick, obj = mmr_select(Xd, torch.from_numpy(Q).to(DEV), torch.from_numpy(cand).to(DEV), k, delta)
    assert pick.dtype == torch.int32 and obj.dtype == torch.float32 and pick.shape == obj.shape == (len(Q), k)
    return pick.cpu().numpy(), obj.cpu().numpy()


SHAPES = [(20, 16, 5),      # float4 path, 5 of the 16 lanes of a group loaded
          (30, 17, 17),     # scalar path; a second row for one group; every slot picked
          (768, 16, 10), (768, 64, 10), (1024, 64, 16), (1536, 16, 5)]


@pytest.mark.parametrize("delta", [0.3, 0.7])
@pytest.mark.parametrize("D,F,k", SHAPES, ids=[f"D{d}-F{f}-k{k}" for d, f, k in SHAPES])
def test_recipe_shapes(D, F, k, delta):
    X, Q, cand = _case(D, F)
    pick, obj = _select(X, Q, cand, k, delta)
    left = check_against_ref(X, Q, cand, k, delta, pick, obj)
    print(f"D={D} F={F} k={k} delta={delta}: {left} of {len(Q)} left out of the exact-pick rule")


@pytest.mark.parametrize("M", [1, 3, 130])
@pytest.mark.parametrize("F", [1, 5, 16, 17, 64])
def test_pool_sizes_batches_and_deltas(F, M):
    D = 30 if F in (5, 17) else 20
    X, Q, cand = _case(D, F, M=130, n=512, seed=7)
    Q, cand = Q[:M], cand[:M]
    for k in sorted({1, min(10, F), F}):
        for delta in (0.0, 0.3, 0.7, 1.0):
            pick, obj = _select(X, Q, cand, k, delta)
            # (delta = 1: every objective of step 0 is exactly 0, the lowest row goes first)
            check_against_ref(X, Q, cand, k, delta, pick, obj, gap_from=1 if delta == 1.0 else 0)
            if delta == 1.0:
                assert (pick[:, 0] == cand.argmin(1)).all() and (obj[:, 0] == 0).all()


def test_strided_and_misaligned_rows():
    D, F, k, delta = 768, 16, 10, 0.7
    X, Q, cand = _case(D, F)
    n = len(X)
    base = _select(X, Q, cand, k, delta)
    check_against_ref(X, Q, cand, k, delta, *base)
    Xt = torch.from_numpy(X)
    # ldx > D, still 16-byte rows: the float4 path again, bit for bit
    wide = torch.full((n, D + 8), 7.0, device=DEV)
    wide[:, :D] = Xt.to(DEV)
    got = _select(wide[:, :D], Q, cand, k, delta)
    assert np.array_equal(got[0], base[0]) and np.array_equal(got[1].view(np.int32), base[1].view(np.int32))
    # an odd row stride, and a base 4 bytes off a 16-byte boundary: the scalar path at D % 4 == 0
    odd = torch.full((n, D + 3), 7.0, device=DEV)
    odd[:, :D] = Xt.to(DEV)
    flat = torch.full((n * D + 1,), 7.0, device=DEV)
    off = flat[1:].view(n, D)
    off.copy_(Xt)
    assert off.data_ptr() % 16 == 4
    a = _select(odd[:, :D], Q, cand, k, delta)
    b = _select(off, Q, cand, k, delta)
    check_against_ref(X, Q, cand, k, delta, *a)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32))


def test_empty_slots_and_rows_out_of_range():
    D, F, k = 20, 16, 10
    X, Q, cand = _case(D, F, M=32, n=512, seed=3)
    n = len(X)
    cand = cand.copy()
    cand[0, :] = -1                       # nothing to pick
    cand[1, [3, 7]] = -1                  # holes in the middle
    cand[2, 6:] = -1                      # 6 candidates for 10 picks
    cand[3, [0, 2]] = [n + 5, 1 << 40]    # rows the graph does not have: empty, never read
    cand[4, [1, 15]] = [-7, n]
    for delta in (0.3, 0.7):
        pick, obj = _select(X, Q, cand, k, delta)
        check_against_ref(X, Q, cand, k, delta, pick, obj)
        assert (pick[0] == -1).all() and np.isneginf(obj[0]).all()
        assert (pick[2, :6] >= 0).all() and (pick[2, 6:] == -1).all() and np.isneginf(obj[2, 6:]).all()
        assert not np.isin(pick[1], [3, 7]).any() and not np.isin(pick[3], [0, 2]).any()
        assert not np.isin(pick[4], [1, 15]).any()


def test_non_unit_rows_zero_row_zero_query():
    D, F, k = 30, 17, 17
    X, Q, cand = _case(D, F, M=32, n=512, seed=5)
    X = X * np.linspace(0.25, 4.0, len(X), dtype=np.float32)[:, None]
    Q = Q * np.linspace(0.5, 3.0, len(Q), dtype=np.float32)[:, None]
    zr = int(cand[1, 0])
    X[zr] = 0.0                           # the nearest row of query 1 (and whoever else lists it)
    Q[9] = 0.0                            # every relevance 0: the lowest row goes first
    for delta in (0.3, 0.7):
        pick, obj = _select(X, Q, cand, k, delta)
        check_against_ref(X, Q, cand, k, delta, pick, obj)  # (query 9 ties at step 0: within the cap)
        assert pick[9, 0] == cand[9].argmin() and obj[9, 0] == 0.0
        assert np.isfinite(obj).all()


def test_identical_rows_tie_to_the_lower_row_bit_for_bit():
    D, F = 768, 16
    X, Q, cand = _case(D, F, M=32)
    n = len(X)
    v = X[cand[0, 0]]
    X = np.concatenate([X, v[None], v[None], v[None]])        # the same vector at rows n, n + 1, n + 2
    cand = cand.copy()
    cand[0, :3] = [n + 2, n + 1, n]                           # listed in descending row order
    # delta = 0: the three lead, lowest row first, with objectives equal as bits
    pick, obj = _select(X, Q, cand, F, 0.0)
    check_against_ref(X, Q, cand, F, 0.0, pick, obj)          # (query 0 ties: within the cap)
    assert pick[0, :3].tolist() == [2, 1, 0]
    assert len(set(obj[0, :3].view(np.int32).tolist())) == 1
    # delta = 0.3: row n leads; the two others fall behind, stay adjacent, n + 1 before n + 2
    pick, obj = _select(X, Q, cand, F, 0.3)
    check_against_ref(X, Q, cand, F, 0.3, pick, obj)
    order = pick[0].tolist()
    assert order[0] == 2
    at = order.index(1)
    assert at > 1 and order[at + 1] == 0
    assert obj[0, at].view(np.int32) == obj[0, at + 1].view(np.int32)


def test_invalid_arguments_are_refused():
    from lazzaro_amd.ops import _lib
    L = _lib.lib()
    X = torch.zeros((8, 16), device=DEV)
    Q = torch.zeros((2, 16), device=DEV)
    cand = torch.zeros((2, 64), dtype=torch.long, device=DEV)
    pick = torch.full((2, 64), -5, dtype=torch.int32, device=DEV)
    obj = torch.zeros((2, 64), device=DEV)
    INVALID = 1  # hipErrorInvalidValue

    def call(ldx=16, n=8, ldq=16, M=2, D=16, F=16, k=4, delta=0.5):
        return L.lzk_mmr_select(X.data_ptr(), ldx, n, Q.data_ptr(), ldq, M, D, cand.data_ptr(), F, k, delta,
                                pick.data_ptr(), obj.data_ptr(), _lib.stream_ptr(X.device))
    for bad in (dict(F=65), dict(F=0), dict(k=17), dict(k=0), dict(D=0), dict(D=-4), dict(D=8200, ldx=8200, ldq=8200),
                dict(delta=1.5), dict(delta=-0.5), dict(delta=float("nan")), dict(n=1 << 31), dict(ldx=8), dict(M=-1)):
        assert call(**bad) == INVALID, bad
    torch.cuda.synchronize()
    assert (pick == -5).all()  # nothing was launched
    assert call() == 0 and call(M=0) == 0
    torch.cuda.synchronize()
    assert (pick.view(-1)[:8] >= 0).all()
    for kw in (dict(k=65), dict(k=0), dict(diversity=2.0)):
        a = dict(k=4, diversity=0.5)
        a.update(kw)
        with pytest.raises(ValueError):
            mmr_select(X, Q, cand, **a)
    with pytest.raises(ValueError):
        mmr_select(X, Q, torch.zeros((2, 65), dtype=torch.long, device=DEV), 4, 0.5)


def test_store_search_with_diversity_on_a_gpu_tenant():
    from lazzaro_amd.engine.tenant_graph import TenantGraph
    N, D, k = 4096, 96, 5
    gen = torch.Generator().manual_seed(21)
    X = torch.nn.functional.normalize(torch.randn(N, D, generator=gen), dim=1)
    g = TenantGraph(device=DEV, dim=D, capacity=N + 64)
    g.add_nodes([f"m{i}" for i in range(N)], [f"c{i}" for i in range(N)], X, shard=g.shard_id("w"),
                types=["preference" if i % 3 == 0 else "semantic" for i in range(N)], stored=True)
    g.take_dirty_rows(), g.take_dirty_edges(), g.take_deleted()
    Qall = torch.nn.functional.normalize(X[:64] + 0.5 * torch.randn(64, D, generator=gen), dim=1).to(DEV)
    n0 = g.mmr_searches
    runs = 0
    for M in (1, 64):       # (64 x 4096: the kernel scan route at fetch_k = 16; 1: the exact store)
        Q = Qall[:M]
        for F in (16, 40):  # (40 > 16 candidate slots: the pool search's wide routes)
            for where in (None, {"types": ["preference"]}):
                ps, pr = g.store_search(Q, F, "l2", where=where)
                s, r = g.store_search(Q, k, "l2", where=where, diversity=0.5, fetch_k=F)
                runs += 1
                pick, obj = mmr_select(g.emb32[: g.n], Q, pr, k, 0.5)
                assert (pick >= 0).all()
                p = pick.long()
                assert torch.equal(r, torch.gather(pr, 1, p))
                assert torch.equal(s.view(torch.int32), torch.gather(ps, 1, p).view(torch.int32))  # bit-equal
                if where is not None:
                    assert (r % 3 == 0).all()
                check_rule1(X.numpy(), Q.cpu().numpy(), pr.cpu().numpy(), k, 0.5, pick.cpu().numpy(),
                            obj.cpu().numpy())
    assert g.mmr_searches - n0 == runs
    # the default pool, and ids in pick order
    s, r = g.store_search(Qall[:3], k, "l2", diversity=0.5)
    assert g.search_ids(Qall[:3], k, "l2", diversity=0.5) == [[f"m{i}" for i in row] for row in r.tolist()]
