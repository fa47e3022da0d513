"""Associative (graph-expanded) selection: the links of a search's nearest rows
are walked, everything reached is scored, the best ``limit`` come back
(csrc/kernels/expand.hip), with the torch formulation.

The contract, per query ``q`` with seeds ``s`` (graph rows, -1 or out of
range = empty, duplicates one entry) and settings ``core.expand.GraphExpand``:

* ``act_0(s) = max(cos(q, s), 0)``. Every cosine is over the fp32 rows and the
  fp32 query and is 0 when either norm is 0.
* Hops h = 1 .. ``hops`` in Jacobi order: the sources of hop h are the
  candidates present at its start, each with ``act_{h-1}``. A source with
  ``sup != 0`` does not expand. A source walks its visible arcs
  ``off[u] .. off[u+1]`` in CSR order and takes the first ``fanout`` that
  qualify: ``w[e] >= min_weight`` (fp32), ``kind[v] == NODE``, ``bias[v]``
  finite. Each taken arc proposes ``t = act_{h-1}(u) * (decay * min(w[e], 1))``
  (two fp32 roundings) and ``act_h(v) = max(act_{h-1}(v), proposals to v)``.
  A row is 0 before it is reached, and every candidate expands whatever its
  activation: the candidate set never depends on a floating-point value.
* ``score(v) = (1 - graph_weight) * cos(q, v) + graph_weight * act_H(v)``; the
  ``limit`` largest in descending order, ties to the lower row, ``(-inf, -1)``
  beyond the candidate count.
* ``via(v)``: -1 when ``act_H(v)`` is the activation the row started with --
  its seed activation, or the 0 of a row that was reached -- which wins a tie
  against a proposal; otherwise the source row of the largest proposal over
  all hops, ties to the lower source row.

Device tensors always take the kernel; CPU tensors take ``expand_select_ref``
(the CPU tier, and a second formulation the tests hold to the same oracle).
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib
from ._dot16 import cos_or_zero
from ._dot16 import sum_depth as EXPAND_SUM_DEPTH  # expand.hip uses mmr.hip's dot layout (csrc/include/lzk_dot16.h)

NEG_INF = float("-inf")
NODE = 1  # (engine.tenant_graph NODE: the kind of a graph node)
MAX_D = 2048  # expand.hip EXP_MAX_D: the query shares the block's LDS with the candidate table


def expand_tol(D: int, hops: int) -> float:
    """|score32 - score64| of the kernel: 2 L(D) + 8 units for a cosine (as
    ``mmr_tol``: L for the dot, L jointly for the norms, 8 for sqrt, multiply,
    divide), 2 roundings per hop on the activation (its factors are <= 1, so
    the seed cosine's error does not grow), 6 for the blend (1 - graph_weight,
    the two products, the sum, with slack for the first applying to both
    terms). The blend's weights sum to 1, so the two terms' errors do not add
    beyond the larger."""
    return (2 * EXPAND_SUM_DEPTH(D) + 8 + 2 * int(hops) + 6) * 2.0 ** -24


def pool_bound(spec, limit: Optional[int] = None) -> int:
    """The most candidates one query of ``spec`` (anything
    ``GraphExpand.coerce`` takes) can reach: ``seed_k * (1 + fanout) ** hops``.
    Raises ValueError for settings, or a ``limit``, the selection does not
    take."""
    from ..core.expand import MAX_LIMIT, GraphExpand
    sp = GraphExpand.coerce(spec)
    if sp is None:
        raise ValueError("expand settings are required")
    if limit is not None and not 1 <= int(limit) <= MAX_LIMIT:
        raise ValueError(f"an expanded search returns 1 .. {MAX_LIMIT} results (limit={limit})")
    return sp.pool


_lib.register("lzk_expand_select", _lib.I,
              [_lib.P, _lib.L, _lib.L, _lib.P, _lib.L, _lib.I, _lib.I,      # X ldx n Q ldq M D
               _lib.P, _lib.I, _lib.P, _lib.P, _lib.P, _lib.L,              # seeds S off adj eid na
               _lib.P, _lib.L, _lib.P, _lib.P, _lib.P,                      # w ne kind sup bias
               _lib.I, _lib.I, _lib.F, _lib.F, _lib.F, _lib.I,              # hops fanout min_w decay gamma limit
               _lib.P, _lib.P, _lib.P, _lib.P, _lib.P])                     # rows scores via ncand stream


def _check(X, Q, seeds, csr, w, kind, sup, bias, spec, limit):
    from ..core.expand import GraphExpand
    sp = GraphExpand.coerce(spec)
    pool_bound(sp, limit)
    if Q.dim() == 1:
        Q = Q[None, :]
    if seeds.dim() == 1:
        seeds = seeds[None, :]
    M, S = seeds.shape
    if not 1 <= S <= sp.seed_k:
        raise ValueError(f"1 .. seed_k={sp.seed_k} seeds per query (got {S})")
    n = X.shape[0]
    if Q.shape[0] != M or X.dim() != 2 or Q.shape[1] != X.shape[1]:
        raise ValueError(f"shapes do not agree: X {tuple(X.shape)}, Q {tuple(Q.shape)}, seeds {tuple(seeds.shape)}")
    off, adj, eid = csr
    if off.numel() != n + 1 or adj.numel() != eid.numel() or min(kind.numel(), sup.numel(), bias.numel()) < n:
        raise ValueError("the CSR and the row columns do not cover the rows of X")
    return sp, Q, seeds, M, S


def expand_select_ref(X, Q, seeds, csr, w, kind, sup, bias, spec, limit):
    """Torch formulation of :func:`expand_select` (any device), fp32
    throughout. Per query the candidate table is a sorted row list; a hop
    flattens its sources' CSR segments, ranks the qualifying arcs of each
    segment by a prefix sum and merges the proposals into the table by three
    stable sorts (via, activation, row)."""
    sp, Q, seeds, M, S = _check(X, Q, seeds, csr, w, kind, sup, bias, spec, limit)
    limit = int(limit)
    dev = X.device
    n, D = X.shape
    off, adj, eid = (t.to(dev) for t in csr)
    w32 = w.to(dev, torch.float32)
    f32 = lambda v: torch.tensor(float(v), dtype=torch.float32, device=dev)  # noqa: E731
    min_w, decay, gamma = f32(sp.min_weight), f32(sp.decay), f32(sp.graph_weight)
    w1 = f32(1.0) - gamma
    target_ok = (kind[:n].to(dev) == NODE) & torch.isfinite(bias[:n].to(dev))
    no_expand = sup[:n].to(dev) != 0
    orow = torch.full((M, limit), -1, dtype=torch.long, device=dev)
    oscore = torch.full((M, limit), NEG_INF, dtype=torch.float32, device=dev)
    ovia = torch.full((M, limit), -1, dtype=torch.long, device=dev)
    ncand = torch.zeros(M, dtype=torch.int32, device=dev)
    Qf = Q.to(dev, torch.float32)
    qn = Qf.norm(dim=1)
    OWN = -1

    def cos_rows(m, rows):
        x = X[rows].to(torch.float32)
        return cos_or_zero(x @ Qf[m], x.norm(dim=1), qn[m].expand(rows.numel()))

    for m in range(M):
        s = seeds[m].to(dev).long()
        rows = torch.unique(s[(s >= 0) & (s < n)])  # (sorted)
        if rows.numel() == 0:
            continue
        act = cos_rows(m, rows).clamp_min(0.0) + 0.0  # (+0.0: no negative zero)
        via = torch.full_like(rows, OWN)
        for _ in range(sp.hops):
            src = ~no_expand[rows]
            u, au = rows[src], act[src]
            start = off[u]
            deg = (off[u + 1] - start).clamp_min(0)
            tot = int(deg.sum())
            if tot == 0:
                continue
            seg = torch.repeat_interleave(torch.arange(u.numel(), device=dev), deg)
            first = torch.cumsum(deg, 0) - deg                      # each segment's first flat index
            pos = torch.arange(tot, device=dev) - first[seg] + start[seg]
            v, e = adj[pos].long(), eid[pos].long()
            we = w32[e]
            ok = (we >= min_w) & target_ok[v]
            before = torch.cumsum(ok.long(), 0) - ok.long()          # qualifying arcs before this one
            take = ok & (before - before[first.clamp_max(tot - 1)][seg] < sp.fanout)
            v, t, pu = v[take], (au[seg] * (decay * we.clamp_max(1.0)))[take], u[seg][take]
            # records: the table's own, the proposals, and (0, own) for every target
            r_all = torch.cat([rows, v, v])
            a_all = torch.cat([act, t, torch.zeros_like(t)])
            v_all = torch.cat([via, pu, torch.full_like(pu, OWN)])
            o = torch.sort(v_all, stable=True).indices              # own (-1) first, then the lower source
            o = o[torch.sort(a_all[o], descending=True, stable=True).indices]
            o = o[torch.sort(r_all[o], stable=True).indices]
            r_s = r_all[o]
            head = torch.ones_like(r_s, dtype=torch.bool)
            head[1:] = r_s[1:] != r_s[:-1]
            rows, act, via = r_s[head], a_all[o][head], v_all[o][head]
        c = cos_rows(m, rows)
        score = w1 * c + gamma * act
        o = torch.sort(score, descending=True, stable=True).indices[:limit]  # (rows ascend: ties to the lower row)
        k = o.numel()
        orow[m, :k], oscore[m, :k], ovia[m, :k] = rows[o], score[o], via[o]
        ncand[m] = rows.numel()
    return orow, oscore, ovia, ncand


def expand_select(X: torch.Tensor, Q: torch.Tensor, seeds: torch.Tensor, csr, w: torch.Tensor, kind: torch.Tensor,
                  sup: torch.Tensor, bias: torch.Tensor, spec, limit: int
                  ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Graph-expanded selection (expand.hip lzk_expand_select; the contract is
    in the module docstring): fp32 rows ``X`` [n, D] (any row stride), fp32
    queries ``Q`` [M, D], ``seeds`` int64 [M, S] graph rows with S <= seed_k,
    ``csr`` = (off int64 [n + 1], adj int32, eid int32) the visible-arc CSR,
    ``w`` fp32 edge weights, ``kind`` / ``sup`` uint8 and ``bias`` fp32 row
    columns, ``spec`` the settings, ``limit`` <= 64. Returns (rows int64
    [M, limit], scores fp32 [M, limit], via int64 [M, limit], ncand int32
    [M]). No host synchronisation."""
    if not X.is_cuda:
        return expand_select_ref(X, Q, seeds, csr, w, kind, sup, bias, spec, limit)
    sp, Q, seeds, M, S = _check(X, Q, seeds, csr, w, kind, sup, bias, spec, limit)
    limit = int(limit)
    dev = X.device
    n, D = X.shape
    if D > MAX_D:
        raise ValueError(f"an expanded search takes rows of at most {MAX_D} dimensions (got {D})")
    off, adj, eid = csr
    assert X.dtype == torch.float32 and X.stride(1) == 1
    assert off.dtype == torch.int64 and adj.dtype == torch.int32 and eid.dtype == torch.int32
    assert w.dtype == torch.float32 and kind.dtype == torch.uint8 and sup.dtype == torch.uint8
    assert bias.dtype == torch.float32
    assert all(t.is_cuda and t.is_contiguous() for t in (off, adj, eid, w, kind, sup, bias))
    Qc = Q.to(dev, torch.float32)
    if Qc.stride(1) != 1:
        Qc = Qc.contiguous()
    sc = seeds.to(dev, torch.long).contiguous()
    rows = torch.empty((M, limit), dtype=torch.long, device=dev)
    scores = torch.empty((M, limit), dtype=torch.float32, device=dev)
    via = torch.empty((M, limit), dtype=torch.long, device=dev)
    ncand = torch.empty(M, dtype=torch.int32, device=dev)
    if M == 0:
        return rows, scores, via, ncand
    L = _lib.lib()
    _lib.check(L.lzk_expand_select(X.data_ptr(), X.stride(0) if n > 1 else max(X.stride(0), D), n,
                                   Qc.data_ptr(), Qc.stride(0) if M > 1 else max(Qc.stride(0), D), M, D,
                                   sc.data_ptr(), S, off.data_ptr(), _lib.ptr(adj), _lib.ptr(eid), adj.numel(),
                                   _lib.ptr(w), w.numel(), kind.data_ptr(), sup.data_ptr(), bias.data_ptr(),
                                   sp.hops, sp.fanout, sp.min_weight, sp.decay, sp.graph_weight, limit,
                                   rows.data_ptr(), scores.data_ptr(), via.data_ptr(), ncand.data_ptr(),
                                   _lib.stream_ptr(dev)), "lzk_expand_select")
    return rows, scores, via, ncand
