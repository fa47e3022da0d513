"""fp64 reference of the cross-tenant tile-table search
(csrc/kernels/mtscan.hip: ``mt_sample_kernel``, ``mt_cand_kernel``,
``mt_rerank_kernel``; driven by ops/search.py ``mt_topk`` and
parallel/routing.py ``_global_small``). Plain numpy; nothing here touches a
GPU or the kernel library. tests/unit/test_mt_ref_cpu.py checks this module on
its own, tests/kernels/test_mtscan_gpu.py and the route test of
test_service_gpu.py hold the kernels and the routes against it.

Tenants. A list of :class:`Tenant` (slot, fp32 rows [n, D], store bias [n]
with -inf = "not stored", kind bytes [n] with 1 = live node). :class:`Table`
lays them out as the tile table does -- tile t = up to 256 consecutive rows of
one tenant, zero-row tenants have no tile, candidate id = tile * 256 + row in
tile, key = slot << 32 | row -- without looking at ``MtTiles``. ``sort=True``
(the route's contract) orders the tenants by slot, so that candidate-id order
is key order; ``sort=False`` keeps the list order (a hand-built table).

Order. (score descending, key ascending), missing entries ``(-inf, -1)``:
``order`` of _ivfpq_ref.py.

Exact grid. ``grid_rows`` / ``grid_queries`` of _cand_ref.py: integers in
[-8, 8], bias ``-|x|^2`` (an integer), alpha 2 or 1. With D <= 1024 a product
is at most 64, ``|x|^2`` and ``|q|^2`` at most 65536 and every partial sum of
``2 <q, x> + b - |q|^2`` in any order an integer below 4 * 65536 < 2^24: bf16,
fp32 and fp64 agree and results are compared bit for bit, ties included.

Gaussian inputs, the bounds (``gamma(n) = n u / (1 - n u)``, u = 2^-24, see
_ivfpq_ref.py: a term that passes through at most n - 1 roundings is off by at
most ``gamma(n)`` of its magnitude).

* scan (``mt_cand_kernel``, and the sampled threshold's lane kernel):
  ``alpha * sum_d q_d x_d + b`` over the bf16 values, Dp products (exact in
  fp32: 8 x 8 bits) accumulated in fp32 in some order -- at most Dp roundings
  on a product --, the multiply by alpha and the bias add: Dp + 2 roundings,
  ``scan bound = gamma(Dp + 3) (|alpha| sum |q_d x_d| + |b|)``.
* re-rank (``mt_rerank_kernel``): ``2 acc + b - qq``. A product of ``acc``
  passes through its lane's fma chain (D / 4 roundings at most) and two
  shuffle adds, then ``2 acc + b`` (one rounding, the doubling is exact) and
  the subtraction: at most D + 2. A square of ``qq`` passes through a chain of
  ceil(D / 64) fmas, the six adds of the wave sum and the subtraction: at most
  D + 3 for every D >= 1. The bias is rounded twice. Hence ``re-rank bound =
  gamma(D + 4) (2 sum |q_d x_d| + |b| + sum q_d^2)`` for L2; the inner-product
  metric has neither the doubling nor the ``qq`` term: ``gamma(D + 4) (sum
  |q_d x_d| + |b|)``.

A non-finite bias adds nothing to a bound: the score is then -inf exactly.
"""
from __future__ import annotations

from typing import List, NamedTuple, Sequence

import numpy as np

from tests.kernels._cand_ref import grid_queries, grid_rows, to_bf16, unit_rows  # noqa: F401
from tests.kernels._ivfpq_ref import NEG_INF, U_FP32, gamma, order  # noqa: F401  (one definition for all modules)

MT_TILE = 256
MT_STRIDE = 64  # the threshold sample: rows 0, 64, 128, 192 of every tile
NODE, GHOST, FREE = 1, 2, 0  # kind bytes: live node; a removed row (any byte but 1); a free row
KC = 16  # candidates mt_topk re-ranks


class Tenant(NamedTuple):
    slot: int
    X: np.ndarray  # fp32 [n, D]
    bias: np.ndarray  # fp32 [n]; -inf: the row is not in the store
    kind: np.ndarray  # uint8 [n]


def l2_bias(X: np.ndarray) -> np.ndarray:
    """The L2 store bias ``-|x|^2`` of fp32 rows, rounded to fp32."""
    return (-(np.asarray(X, dtype=np.float64) ** 2).sum(1)).astype(np.float32)


class Table:
    """The logical content of the tile table of ``tenants`` and the flat row
    arrays (table order: tenant after tenant, rows ascending) every reference
    below works on."""

    def __init__(self, tenants: Sequence[Tenant], sort: bool = True):
        ts = [t for t in tenants if len(t.bias) > 0]
        if sort:
            ts = sorted(ts, key=lambda t: t.slot)
        self.tenants: List[Tenant] = ts
        t_slot, t_row0, t_n, t_ten, t_flat0 = [], [], [], [], []
        self.ten_flat0 = []
        flat = 0
        for j, t in enumerate(ts):
            n = len(t.bias)
            self.ten_flat0.append(flat)
            for r0 in range(0, n, MT_TILE):
                t_slot.append(t.slot)
                t_row0.append(r0)
                t_n.append(min(MT_TILE, n - r0))
                t_ten.append(j)
                t_flat0.append(flat + r0)
            flat += n
        self.N = flat
        self.t_slot = np.array(t_slot, dtype=np.int64)
        self.t_row0 = np.array(t_row0, dtype=np.int64)
        self.t_n = np.array(t_n, dtype=np.int64)
        self.t_ten = np.array(t_ten, dtype=np.int64)
        self.t_flat0 = np.array(t_flat0, dtype=np.int64)
        self.n_tiles = len(t_slot)
        D = ts[0].X.shape[1] if ts else 0
        self.D = D
        self.X = np.concatenate([np.asarray(t.X, dtype=np.float32) for t in ts]).astype(np.float64) if ts \
            else np.zeros((0, 0))
        self.X16 = to_bf16(self.X)
        self.bias = np.concatenate([np.asarray(t.bias, dtype=np.float32) for t in ts]).astype(np.float64) if ts \
            else np.zeros(0)
        self.kind = np.concatenate([np.asarray(t.kind, dtype=np.uint8) for t in ts]) if ts else np.zeros(0, np.uint8)
        self.row = np.concatenate([np.arange(len(t.bias), dtype=np.int64) for t in ts]) if ts else np.zeros(0, np.int64)
        self.slot = np.concatenate([np.full(len(t.bias), t.slot, dtype=np.int64) for t in ts]) if ts \
            else np.zeros(0, np.int64)
        self.key = (self.slot << 32) | self.row
        # candidate id of every flat row: its tile * 256 + its row in the tile
        tile_of = np.repeat(np.arange(self.n_tiles, dtype=np.int64), self.t_n)
        self.cid = tile_of * MT_TILE + (self.row - self.t_row0[tile_of])
        self.stored = self.bias != NEG_INF
        self._fin_bias = np.where(np.isfinite(self.bias), np.abs(self.bias), 0.0)

    # ------------------------------------------------------------ id maps
    def flat_of_cid(self, cid) -> np.ndarray:
        """Flat row of candidate ids (which must name rows inside their tile's
        count)."""
        cid = np.asarray(cid, dtype=np.int64)
        t, r = cid >> 8, cid & 255
        assert ((t >= 0) & (t < self.n_tiles)).all() and (r < self.t_n[t]).all()
        return self.t_flat0[t] + r

    # ------------------------------------------------------------ sample
    def sample_ref(self, Dp: int):
        """``lzk_mt_sample``: (tile, row in tile) of every sample row -- rows 0,
        64, 128, 192 of every tile below its count, tile after tile --, the bf16
        values [ns, Dp] (zero padding past D) and the biases [ns]."""
        s_tile, s_row = [], []
        for t in range(self.n_tiles):
            for r in range(0, int(self.t_n[t]), MT_STRIDE):
                s_tile.append(t)
                s_row.append(r)
        s_tile, s_row = np.array(s_tile, dtype=np.int64), np.array(s_row, dtype=np.int64)
        f = self.t_flat0[s_tile] + s_row if s_tile.size else np.zeros(0, np.int64)
        rows = np.zeros((f.size, Dp))
        rows[:, : self.D] = self.X16[f]
        return s_tile, s_row, rows, self.bias[f]

    # ------------------------------------------------------------ scores
    def scan(self, Q, alpha: float, Dp: int):
        """fp64 ``alpha <bf16(q), bf16(x)> + bias`` [nq, N] (exact: bf16
        products and their sums are exact in fp64 at these sizes) and the scan
        bound of every entry."""
        q = to_bf16(np.asarray(Q, dtype=np.float64))
        with np.errstate(invalid="ignore"):
            s = float(alpha) * (q @ self.X16.T) + self.bias[None, :]
        mag = abs(float(alpha)) * (np.abs(q) @ np.abs(self.X16).T) + self._fin_bias[None, :]
        return s, gamma(Dp + 3) * mag

    def exact(self, Q, metric: str):
        """fp64 store score from the fp32 rows, ``2 <q, x> + b - |q|^2`` (l2) or
        ``<q, x> + b`` (ip), [nq, N], and the re-rank bound of every entry."""
        q = np.asarray(Q, dtype=np.float32).astype(np.float64)
        dot = q @ self.X.T
        adot = np.abs(q) @ np.abs(self.X).T
        qq = (q * q).sum(1)[:, None]
        with np.errstate(invalid="ignore"):
            if metric == "l2":
                s = 2.0 * dot + self.bias[None, :] - qq
                mag = 2.0 * adot + self._fin_bias[None, :] + qq
            else:
                s = dot + self.bias[None, :]
                mag = adot + self._fin_bias[None, :]
        return s, gamma(self.D + 4) * mag

    # ------------------------------------------------------------ candidates
    def cand_ref(self, Q, alpha: float, thr, Dp: int):
        """``lzk_mt_cand``: per query the (candidate id, fp64 scan score) of
        every row with score >= thr[q]; rows past a tile's count do not exist
        here and rows whose score is -inf are never members. Returns a list of
        (ids int64 ascending, scores fp64)."""
        s, _ = self.scan(Q, alpha, Dp)
        out = []
        for q in range(s.shape[0]):
            m = (s[q] >= float(thr[q])) & (s[q] != NEG_INF)
            ids = self.cid[m]
            o = np.argsort(ids)
            out.append((ids[o], s[q][m][o]))
        return out

    def top_cand(self, Q, alpha: float, Dp: int, kc: int = KC) -> np.ndarray:
        """The kc best stored rows of every query by (scan score desc, key asc)
        as candidate ids [nq, kc], -1 past the stored rows: what the candidate
        pass and ``cand_select`` hand to the re-rank when no accumulation error
        exists (the exact grid)."""
        s, _ = self.scan(Q, alpha, Dp)
        out = np.full((s.shape[0], kc), -1, dtype=np.int64)
        for q in range(s.shape[0]):
            f = np.nonzero(s[q] != NEG_INF)[0]
            if f.size > kc:  # (only rows at or above the kc-th best value can rank: ties included)
                f = f[s[q][f] >= np.partition(s[q][f], f.size - kc)[f.size - kc]]
            o = f[order(s[q][f], self.key[f])[:kc]]
            out[q, : o.size] = self.cid[o]
        return out

    # ------------------------------------------------------------ re-rank
    def rerank_ref(self, Q, cand, k: int, metric: str):
        """``lzk_mt_rerank``: ``cand`` [M, C] candidate ids (-1 = none, an id at
        most once per list). The live entries (id >= 0, score != -inf) are
        ordered by (fp64 score desc, key asc); the first k ranks are written,
        a rank whose row is not a live node as (-inf, -1) in place; slots past
        the live count are (-inf, -1). Returns (scores fp64 [M, k], keys int64
        [M, k], bound [M, k] -- the re-rank bound of each written score, 0 where
        none --, ghost [M] bool: a non-node row took one of the k ranks)."""
        cand = np.asarray(cand, dtype=np.int64)
        M = cand.shape[0]
        S = np.full((M, k), NEG_INF)
        K = np.full((M, k), -1, dtype=np.int64)
        B = np.zeros((M, k))
        ghost = np.zeros(M, dtype=bool)
        sc, bd = self.exact(Q, metric)
        for q in range(M):
            v = cand[q][cand[q] >= 0]
            assert np.unique(v).size == v.size
            f = self.flat_of_cid(v)
            f = f[sc[q][f] != NEG_INF]
            o = f[order(sc[q][f], self.key[f])[:k]]
            node = self.kind[o] == NODE
            n = o.size
            S[q, :n] = np.where(node, sc[q][o], NEG_INF)
            K[q, :n] = np.where(node, self.key[o], -1)
            B[q, :n] = np.where(node, bd[q][o], 0.0)
            ghost[q] = bool((~node).any())
        return S, K, B, ghost

    # ------------------------------------------------------------ the route
    def global_ref(self, Q, k: int, metric: str = "l2"):
        """The contract of the global search over these tenants: per tenant the
        top-k of its stored rows (finite bias) by (score desc, row asc), the
        non-nodes among them dropped, the rest merged by (score desc, key asc).
        Returns (scores fp64 [nq, k], keys int64 [nq, k], bound [nq, k])."""
        sc, bd = self.exact(Q, metric)
        nq = sc.shape[0]
        cs, ck, cb = [np.full((nq, k), NEG_INF)], [np.full((nq, k), -1, dtype=np.int64)], [np.zeros((nq, k))]
        for j, t in enumerate(self.tenants):
            a, n = self.ten_flat0[j], len(t.bias)
            s = sc[:, a: a + n]
            o = np.argsort(-s, axis=1, kind="stable")[:, :k]  # (score desc, row asc); -inf (not stored) last
            ts = np.take_along_axis(s, o, 1)
            ok = (ts != NEG_INF) & (self.kind[a + o] == NODE)
            cs.append(np.where(ok, ts, NEG_INF))
            ck.append(np.where(ok, self.key[a + o], -1))
            cb.append(np.where(ok, np.take_along_axis(bd[:, a: a + n], o, 1), 0.0))
        cs, ck, cb = np.concatenate(cs, 1), np.concatenate(ck, 1), np.concatenate(cb, 1)
        S = np.full((nq, k), NEG_INF)
        K = np.full((nq, k), -1, dtype=np.int64)
        B = np.zeros((nq, k))
        for q in range(nq):
            f = np.nonzero(ck[q] >= 0)[0]
            o = f[order(cs[q][f], ck[q][f])[:k]]
            S[q, : o.size], K[q, : o.size], B[q, : o.size] = cs[q][o], ck[q][o], cb[q][o]
        return S, K, B

    # ------------------------------------------------------------ decidability
    def decidable(self, Q, k: int, metric: str, Dp: int, kc: int = KC):
        """Per query: every row of the fp64 top-k (stored rows, exact scores)
        beats the (kc + 1)-th best bf16-input scan score by more than twice the
        scan bound (the largest of the query's entries), so neither bf16
        rounding of the inputs nor the accumulation order can push it out of
        the kc candidates. A table of at most kc stored rows decides every
        query. Returns bool [nq]."""
        alpha = 2.0 if metric == "l2" else 1.0
        ex, _ = self.exact(Q, metric)
        sn, bn = self.scan(Q, alpha, Dp)
        out = np.ones(ex.shape[0], dtype=bool)
        f = np.nonzero(self.stored)[0]
        if f.size <= kc:
            return out
        for q in range(ex.shape[0]):
            top = f[order(ex[q][f], self.key[f])[:k]]
            s17 = np.sort(sn[q][f])[::-1][kc]
            out[q] = bool((sn[q][top] - 2.0 * bn[q][f].max() > s17).all())
        return out


# ---------------------------------------------------------------- input builders
ROW_COUNTS = (1, 63, 64, 65, 255, 256, 257, 700)


def make_tenants(rng, counts, slots, D: int, family: str, norm: float = 1.0, ghosts: bool = True,
                 unstore_samples: bool = False) -> List[Tenant]:
    """Tenants of ``counts`` rows at ``slots``. family "grid": integer rows,
    bias ``-|x|^2``, rows planted as duplicates of the first tenant's rows (so
    exact ties cross tenants); "gauss": rows of norm ``norm``. About one row in
    16 is not stored (bias -inf); with ``ghosts`` about one stored row in 12 is
    a ghost (kind 2) and one unstored row in 2 is free (kind 0).
    ``unstore_samples``: every threshold-sample row (0, 64, 128, 192 of a
    tile) is not stored."""
    out = []
    first = None
    for n, slot in zip(counts, slots):
        if family == "grid":
            X = grid_rows(rng, n, D, dup=min(6, n // 4)).astype(np.float32)
            if first is not None and n > 1:
                m = min(n, len(first), 5)
                X[n - m:] = first[:m]  # the same rows in another tenant: ties that only the key breaks
            elif first is None:
                first = X.copy()
        else:
            X = unit_rows(rng, n, D, norm).astype(np.float32)
        b = l2_bias(X)
        kind = np.full(n, NODE, dtype=np.uint8)
        if n > 1:
            uns = rng.random(n) < 1.0 / 16
            if unstore_samples:
                uns[(np.arange(n) % MT_TILE) % MT_STRIDE == 0] = True
            b[uns] = NEG_INF
            if ghosts:
                kind[uns & (rng.random(n) < 0.5)] = FREE
                kind[~uns & (rng.random(n) < 1.0 / 12)] = GHOST
        out.append(Tenant(int(slot), X, b, kind))
    return out


def e2e_counts() -> List[int]:
    """The end-to-end tests' tenant sizes: 40 tenants cycling through
    ROW_COUNTS, six more of 700 rows and six one-row tenants (12511 rows)."""
    return [ROW_COUNTS[j % len(ROW_COUNTS)] for j in range(40)] + [700] * 6 + [1] * 6


def e2e_slots(rng, n: int) -> np.ndarray:
    """n distinct slots below 3 n in random order: unsorted, with gaps."""
    return rng.permutation(3 * n)[:n].astype(np.int64)


def e2e_gauss(D: int, norm: float, nq: int = 60):
    """The Gaussian end-to-end case of (D, norm): tenants without ghosts and the
    queries (norm 1). One definition for test_mt_ref_cpu.py, which proves the
    undecidable-query cap on it, and test_mtscan_gpu.py, which runs it."""
    rng = np.random.default_rng(7000 + D + int(10 * norm))
    counts = e2e_counts()
    tenants = make_tenants(rng, counts, e2e_slots(rng, len(counts)), D, "gauss", norm=norm, ghosts=False)
    Q = unit_rows(rng, nq, D).astype(np.float32)
    return tenants, Q


def margin_gauss(D: int, norm: float, nq: int = 120):
    """A table its threshold sample covers almost completely (96 one-row
    tenants -- row 0 of every tile is a sample row -- and two of 2 rows): for
    most queries the sample's 16th best IS the table's 16th best, so only the
    threshold's accumulation-order margin keeps that row in the list."""
    rng = np.random.default_rng(9000 + D + int(10 * norm))
    counts = [1] * 96 + [2, 2]
    tenants = make_tenants(rng, counts, e2e_slots(rng, len(counts)), D, "gauss", norm=norm, ghosts=False)
    Q = unit_rows(rng, nq, D).astype(np.float32)
    return tenants, Q
