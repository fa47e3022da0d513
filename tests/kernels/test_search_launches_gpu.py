"""The device work of the store search entry points (ops.search), pinned
launch by launch: the launchers each call reaches, their order and every
scalar argument (caps, grids, slots, strides, ranks, alpha) equal the traces in
``tests/golden/search_launches.json``, recorded on one MI355X before the host
side was folded into one staged pipeline. A host-side refactor of the path may
not add, drop, reorder or resize a launch.

The recorder swaps the functions of ``_lib.lib()`` for wrappers during one
call and notes ``(name, [arguments declared I, L, F or D in _lib._SIGS])``;
pointers are dropped, and functions without any pointer argument (not even a
stream: the host-side sizing queries) are not launches and are left alone.
Names and order are compared on every device, the scalars when the device has
the recorded number of CUs (grids and record capacities follow it).

Every call's result is also held against ``_ref_topk`` on the bf16 operands,
rows exactly. Stores: N = 16,384 seeded unit rows (sample stride S = 64, the
speculative threshold on), repaired on the host until the fp64 scores of the
ranks that decide a result lie more than GAP apart -- GAP = 4 D 2^-24 |q| |x|,
twice the worst fp32 accumulation error of two scores, so the rows are the
same for any summation order.

``python -m tests.kernels.test_search_launches_gpu OUT.json`` writes the traces
of the tree it runs in.

Observed on one MI355X: the 21 cases, their stores and references included,
take under 5 s together.
"""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from lazzaro_amd.ops import _lib  # noqa: E402
from lazzaro_amd.ops import search as S  # noqa: E402

DEV = "cuda"
N = 16384
GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden", "search_launches.json")
FLOOR = 0.5
FP8_SCALE = 64.0
# e4m3 keeps 3 mantissa bits (relative rounding error 2^-4 per element, the
# scaled values far above its subnormals): |<q8, x8> / scale^2 - <q, x>| <=
# (2 * 2^-4 + 2^-8) |q| |x| = 0.129 |q| |x|, norms <= 1 + 2^-7
FP8_MARGIN = 0.14
_SCALAR = {_lib.I: int, _lib.L: int, _lib.F: float, _lib.D: float}


class Recorder:
    """Context: every launcher of the kernel library appends its name and
    scalar arguments to ``trace`` and then runs."""

    def __init__(self):
        self.trace = []

    def __enter__(self):
        L = _lib.lib()
        self._saved = {}
        for name, (_, argtypes) in list(_lib._SIGS.items()):
            fn = getattr(L, name, None)
            if fn is None or _lib.P not in argtypes:
                continue
            self._saved[name] = fn
            setattr(L, name, self._wrap(name, fn, argtypes))
        return self

    def _wrap(self, name, fn, argtypes):
        def launch(*args):
            self.trace.append([name, [_SCALAR[t](a) for a, t in zip(args, argtypes) if t in _SCALAR]])
            return fn(*args)
        return launch

    def __exit__(self, *exc):
        L = _lib.lib()
        for name, fn in self._saved.items():
            setattr(L, name, fn)
        return False


def _bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).double().numpy()


def _unit(rng, n, d):
    a = rng.standard_normal((n, d))
    return _bf16(a / np.linalg.norm(a, axis=1, keepdims=True))


def _gap(d):
    return 4.0 * d * 2.0 ** -24 * (1.0 + 2.0 ** -7) ** 2


@functools.lru_cache(maxsize=None)
def _store(d, nq, kmax):
    """(X, Q, row labels, query labels) on the host, bf16 values as fp64: unit
    rows; the first four queries lean on rows 1000 .. 1003 of their own label
    (scores near 0.95: the entries a floor of 0.5 keeps). Rows are replaced
    until ranks 1 .. kmax + 1 of every query, over all rows and over the rows
    of its label, are more than GAP apart."""
    rng = np.random.default_rng(1000 * d + nq)
    X, Q = _unit(rng, N, d), _unit(rng, nq, d)
    rl, ql = (np.arange(N) % 4).astype(np.int32), (np.arange(nq) % 4).astype(np.int32)
    lean = range(min(4, nq))
    for q in lean:
        Q[q] = _bf16((0.95 * X[1000 + q] + 0.3 * _unit(rng, 1, d)[0])[None, :])[0]
        Q[q] = _bf16((Q[q] / np.linalg.norm(Q[q]))[None, :])[0]
    keep = {1000 + q for q in lean}
    other = torch.from_numpy(rl[None, :] != ql[:, None])
    for _ in range(60):
        s = torch.from_numpy(Q @ X.T)
        victims = set()
        for sc in (s, s.masked_fill(other, float("-inf"))):
            ts, tr = sc.topk(kmax + 1, dim=1)
            bad = (ts[:, :-1] - ts[:, 1:]) <= _gap(d)
            for q, i in bad.nonzero().tolist():
                lo, hi = int(tr[q, i + 1]), int(tr[q, i])
                victims.add(lo if lo not in keep else hi)
        victims -= keep
        if not victims:
            return X, Q, rl, ql
        v = sorted(victims)
        X[v] = _unit(rng, len(v), d)
    raise AssertionError("the store did not settle")


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(dtype) if dtype is not None else t).to(DEV)


def _blk_nq():
    """The smallest batch for which the bf16 candidate scan of N rows takes
    the block-record branch (lzk_cand_grid > 0: as many 256 x 256 tiles as
    CUs)."""
    L = _lib.lib()
    return next(nq for nq in range(1, 1 << 16, 256) if L.lzk_cand_grid(N, nq, 0) > 0)


class _I8:
    """The operands of the int8 entry points the way TenantGraph drives them:
    rigorous margins from ``i8_query`` (smax = the largest row scale, xn = the
    largest row norm + 2^-7), widened by 2^-8 |q| |x| for lean rows."""

    def __init__(self, nq, lean=False):
        X, Q, rl, ql = _store(128, 130, 64)
        Q = Q[:nq]
        self.X16, self.Q16 = _dev(X, torch.bfloat16), _dev(Q, torch.bfloat16)
        self.rl, self.ql = _dev(rl), _dev(ql[:nq])
        self.X8, self.rs = S.quantize_i8_rows(self.X16)
        norms = np.linalg.norm(X, axis=1)
        sumsq = (self.X16.double() ** 2).sum(0).contiguous()
        smax = self.rs.max().reshape(1).contiguous()
        self.q8, self.qs, _, self.mr = S.i8_query(self.Q16, 128, sumsq, N, smax, 1.0, 3.0,
                                                  float(norms.max()) + 2.0 ** -7)
        self.rows = self.X16
        if lean:
            X32, Q32 = self.X16.float().contiguous(), self.Q16.float().contiguous()
            self.mr = (self.mr + 2.0 ** -8 * Q32.norm(dim=1) * float(norms.max())).contiguous()
            self.rows = S.LeanRows(X32, 128, Q32)
        torch.cuda.synchronize()

    def ref(self, k, labels=False):
        return S._ref_topk(self.X16, self.Q16, k, None, self.rl if labels else None, self.ql if labels else None)


def _bf(nq):
    X, Q, rl, ql = _store(64, nq, 10)
    return _dev(X, torch.bfloat16), _dev(Q, torch.bfloat16), _dev(rl), _dev(ql)


def _i8(nq, lean, i8_sample):
    o = _I8(nq, lean)

    def call():
        S.I8_SAMPLE = i8_sample
        return [S.flat_topk_i8(o.X8, o.rs, o.q8, o.qs, o.rows, o.Q16, 10, margin=o.mr, margin_rig=o.mr)]
    return call, lambda: [o.ref(10)], 128, None


def _i8_wide(nq, k):
    o = _I8(nq)
    return (lambda: [S.flat_topk_i8_wide(o.X8, o.rs, o.q8, o.qs, o.X16, o.Q16, k, margin=o.mr, margin_rig=o.mr)],
            lambda: [o.ref(k)], 128, None)


def _dual_i8(floor):
    o = _I8(130)

    def call():
        stats = []
        out = S.flat_topk_dual_i8(o.X8, o.rs, o.q8, o.qs, o.X16, o.Q16, 10, row_label=o.rl, q_label=o.ql,
                                  margin=o.mr, margin_rig=o.mr, floor=floor, stats=stats)
        assert len(stats) == 3 and stats[2] == max(2048, 16 * 10 * 64)  # two (flags, lengths) pairs and the capacity
        return list(out)
    return call, lambda: [o.ref(10), o.ref(10, True)], 128, floor


def _fp8():
    o = _I8(130)
    X8, Q8 = S.quantize_e4m3(o.X16, FP8_SCALE), S.quantize_e4m3(o.Q16, FP8_SCALE)
    margin = torch.full((130,), FP8_MARGIN, device=DEV)
    return (lambda: [S.flat_topk_fp8(X8, Q8, FP8_SCALE * FP8_SCALE, o.X16, o.Q16, 10, margin=margin)],
            lambda: [o.ref(10)], 128, None)


def _cand(nq, dual):
    X16, Q16, rl, ql = _bf(nq)

    def call():
        S.SEARCH_MODE = "cand"
        if dual:
            return list(S.flat_topk_dual(X16, Q16, 10, row_label=rl, q_label=ql))
        return [S.flat_topk(X16, Q16, 10)]
    return call, lambda: [S._ref_topk(X16, Q16, 10)] + ([S._ref_topk(X16, Q16, 10, None, rl, ql)] if dual else []), 64, None


def _lane1():
    X16, Q16, _, _ = _bf(8)
    Q1 = Q16[:1].contiguous()
    nch = _lib.lib().lzk_flat_topk_chunks(N, 1, S.TARGET_WGS)
    assert S._merge_groups(1, nch) > 1  # the two-level merge
    return (lambda: [S._flat_topk_lane(X16, Q1, 10, 10, None, None, None, 1.0, 0, None)],
            lambda: [S._ref_topk(X16, Q1, 10)], 64, None)


def _sample1(stride=4):
    o = _I8(1)
    nch = _lib.lib().lzk_flat_topk_chunks(N // stride, 1, S.TARGET_WGS)
    assert S._merge_groups(1, nch) > 1  # the two-level merge (a 1/64 sample of this store has two chunks only)

    def ref():
        # the scan's own score of the sampled rows, bit for bit (no bias: one product)
        dot = (o.X8[::stride].cpu().long() @ o.q8.cpu().long().T).T.float()
        sc = o.qs.cpu()[:, None] * (dot * o.rs[::stride].cpu()[None, :])
        order = torch.argsort(-sc, dim=1, stable=True)[:, :16]
        return [(torch.gather(sc, 1, order).to(DEV), (order * stride).to(DEV))]
    return lambda: [S.sample_topk_i8(o.X8, o.rs, o.q8, o.qs, 16, stride)], ref, 128, "i8"


def _cases():
    """name -> builder of (call, reference, D, floor | "i8" | None)."""
    c = {}
    for nq in (8, 130):
        for lean in (False, True):
            for smp in (True, False):
                c[f"i8-nq{nq}-{'lean' if lean else 'bf16'}-{'i8sample' if smp else 'lanesample'}"] = \
                    functools.partial(_i8, nq, lean, smp)
        for k in (20, 64):
            c[f"i8wide-k{k}-nq{nq}"] = functools.partial(_i8_wide, nq, k)
    c["duali8"] = functools.partial(_dual_i8, None)
    c["duali8-floor"] = functools.partial(_dual_i8, FLOOR)
    c["fp8"] = _fp8
    for nq in ("8", "blk"):
        c[f"cand-nq{nq}"] = lambda nq=nq: _cand(8 if nq == "8" else _blk_nq(), False)
        c[f"canddual-nq{nq}"] = lambda nq=nq: _cand(8 if nq == "8" else _blk_nq(), True)
    c["lane-nq1"] = _lane1
    c["samplei8-nq1"] = _sample1
    return c


CASES = _cases()
_KNOBS = ("I8_SAMPLE", "SEARCH_MODE")


def run_case(name):
    """Run one case under the recorder; its results are checked against the
    reference. Returns the trace."""
    call, ref, d, mode = CASES[name]()
    saved = {k: getattr(S, k) for k in _KNOBS}
    try:
        with Recorder() as rec:
            got = call()
    finally:
        for k, v in saved.items():
            setattr(S, k, v)
    torch.cuda.synchronize()
    want = ref()
    assert len(got) == len(want)
    for (s, r), (es, er) in zip(got, want):
        if mode == "i8":
            assert torch.equal(r, er) and torch.equal(s, es), name
            continue
        if mode is None:
            assert torch.equal(r, er), (name, (r != er).any(1).nonzero().flatten()[:8])
            assert bool(((s - es).abs() <= _gap(d)).all()), name
            continue
        keep = es >= mode + 1e-3  # a floor: the entries above it, and below it such an entry or an empty slot
        assert bool(keep[:4, 0].all())
        assert torch.equal(r[keep], er[keep]) and bool(((s[keep] - es[keep]).abs() <= _gap(d)).all()), name
        assert bool(((r[~keep] == er[~keep]) | (r[~keep] == -1)).all()), name
    return rec.trace


def _cus():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


@functools.lru_cache(maxsize=None)
def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_recorder_restores_the_library_gpu():
    L = _lib.lib()
    before = L.lzk_cand_gather
    with Recorder() as rec:
        assert L.lzk_cand_gather is not before
        assert L.lzk_flat_topk_kslot(10) == 10 and rec.trace == []  # a sizing query: no launch
    assert L.lzk_cand_gather is before


def test_every_case_is_recorded_gpu():
    assert sorted(_golden()["traces"]) == sorted(CASES)
    assert _golden()["blk_nq"] == _blk_nq() or _golden()["multi_processor_count"] != _cus()


@pytest.mark.parametrize("name", sorted(CASES))
def test_launch_trace_gpu(name):
    g = _golden()
    want = g["traces"][name]
    got = run_case(name)
    assert [n for n, _ in got] == [n for n, _ in want]
    if _cus() == g["multi_processor_count"]:
        for (n, a), (_, e) in zip(got, want):
            assert a == e, (n, a, e)


if __name__ == "__main__":
    out = {"multi_processor_count": _cus(), "blk_nq": _blk_nq(), "traces": {n: run_case(n) for n in sorted(CASES)}}
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
    print("recorded", len(out["traces"]), "cases on", out["multi_processor_count"], "CUs, blk_nq", out["blk_nq"])
