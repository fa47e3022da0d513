"""``lzk_mt_bias`` (csrc/kernels/mtbias.hip) on the GPU: the bias columns of a
served round, ONE launch over every job of tests/kernels/_mtbias_cases.py plus
the hand-made ones below, compared for equality -- the contract is plain IEEE
arithmetic, so there is no tolerance -- with

1. the numpy oracle tests/kernels/_mtbias_ref.py, written from the contract;
2. the column the tenant's own code builds (``TenantGraph._filter_plan(...)
   .bias`` / ``TenantGraph.boost_bias(...)``: filter.hip and boost.hip).
"""
import dataclasses

import numpy as np
import pytest
import torch

from tests.kernels import _mtbias_cases as C
from tests.kernels._mtbias_ref import job_column_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def launch():
    """(cases, jobs, arena, offsets) of the one launch every test reads."""
    from lazzaro_amd.ops.mt_bias_ops import mt_bias
    cs, graphs = C.cases("cuda")
    jobs = [g._mt_bias_job(flt, boost, metric) for _, g, flt, boost, metric in cs]
    # a column that is a view one element into its buffer: the job's pointers
    # no longer allow 16-byte loads, the result must not change
    views = []
    for i, shift in ((2, "store_bias"), (3, "sal"), (1, "sqn")):
        for k in range(len(cs) - 1, -1, -1):
            label, g, flt, boost, metric = cs[k]
            has = {"store_bias": flt is None, "sal": boost is not None and flt is not None,
                   "sqn": flt is not None and boost is None and metric == "l2"}[shift]
            if g.n == C.SIZES[-i] and has:
                break
        else:
            raise AssertionError(shift)
        j = jobs[k]
        src = j.cols["sal"] if shift == "sal" else getattr(j, shift)
        buf = torch.cat([torch.zeros(1, dtype=src.dtype, device=src.device), src[: j.n]])
        assert buf.data_ptr() % 16 == 0 and buf[1:].data_ptr() % 16 == 4
        if shift == "sal":
            vj = dataclasses.replace(j, cols=dict(j.cols, sal=buf[1:]))
        else:
            vj = dataclasses.replace(j, **{shift: buf[1:]})
        views.append((f"{label} [{shift} one element in]", k, vj))
    all_jobs = jobs + [v[2] for v in views]
    arena, offs = mt_bias(all_jobs)
    torch.cuda.synchronize()
    return cs, jobs, views, all_jobs, arena.cpu().numpy(), offs


def _col(arena, offs, jobs, i):
    return arena[offs[i]: offs[i] + int(jobs[i].n)]


def test_the_layout_of_the_arena(launch):
    cs, jobs, views, all_jobs, arena, offs = launch
    assert 40 <= len(cs) <= 60 and sorted({g.n for _, g, *_ in cs}) == sorted(C.SIZES)
    at = 0
    for j, o in zip(all_jobs, offs):
        assert o == at and o % 4 == 0
        at += (int(j.n) + 3) & ~3
    kinds = {(flt is not None, boost is not None) for _, _, flt, boost, _ in cs}
    assert kinds == {(True, False), (False, True), (True, True)}


def test_every_column_equals_the_oracle(launch):
    cs, jobs, views, all_jobs, arena, offs = launch
    finite = masked = 0
    for i, ((label, *_), job) in enumerate(zip(cs, jobs)):
        got, want = _col(arena, offs, all_jobs, i), job_column_ref(job)
        assert got.shape == want.shape, label
        bad = np.nonzero(got.view(np.int32) != want.view(np.int32))[0]
        assert bad.size == 0, (label, bad[:8].tolist(), got[bad[:4]].tolist(), want[bad[:4]].tolist())
        assert not np.isnan(got).any(), label
        finite += int(np.isfinite(want).sum())
        masked += int(np.isneginf(want).sum())
    assert finite > 5000 and masked > 5000  # rows pass and rows are masked: the comparison is not vacuous


def test_the_cases_the_columns_must_show(launch):
    """What the issue lists, looked up in the launch's own output."""
    cs, jobs, views, all_jobs, arena, offs = launch
    by = {label: i for i, (label, *_) in enumerate(cs)}
    # a type the tenant never saw passes nothing
    never = [i for i, (label, *_) in enumerate(cs) if "never_seen" in label and jobs[i].boost is None]
    assert never and all(np.isneginf(_col(arena, offs, all_jobs, i)).all() for i in never)
    # the NaN salience (row 2) and the overflowing prior (row 1) of a boost-only job: prior 0, the base comes through
    seen = 0
    for i, (label, g, flt, boost, metric) in enumerate(cs):
        if flt is None and boost is C.OVERFLOW and g.n > 2:
            col, base = _col(arena, offs, all_jobs, i), jobs[i].store_bias.cpu().numpy()
            kind = jobs[i].cols["kind"][: g.n].cpu().numpy()
            for r in (1, 2):
                if kind[r] == 1:
                    assert col[r] == base[r], (label, r)
                    seen += 1
    assert seen >= 2
    # one filter on two tenants whose type dictionaries assign different codes to the same names
    a, b = by["n257 types shared"], by["n1023 types shared"]
    ga, gb = cs[a][1], cs[b][1]
    assert ga.type_code["t0"] != gb.type_code["t0"] and {ga.type_code["t0"], gb.type_code["t0"]} == {0, 254}
    assert sorted(jobs[a].pred.type_codes) != sorted(jobs[b].pred.type_codes)
    for i, g in ((a, ga), (b, gb)):
        col = _col(arena, offs, all_jobs, i)
        ok = np.isfinite(col)
        assert ok.any() and {g.types[r] for r in np.nonzero(ok)[0]} <= {"t0", "t31", "t32", "t254"}
        assert {31, 32} <= set(jobs[i].pred.type_codes) or {254 - 31, 254 - 32} <= set(jobs[i].pred.type_codes)
    # two jobs on one tenant with different filters differ
    same = [i for i, (label, g, flt, boost, _) in enumerate(cs) if g is ga and flt is not None and boost is None]
    assert len(same) >= 2
    assert not np.array_equal(_col(arena, offs, all_jobs, same[0]), _col(arena, offs, all_jobs, same[1]))
    # excluded rows 31, 32 and n - 1 are masked
    hit = 0
    for i, (label, g, flt, boost, _) in enumerate(cs):
        if flt is not None and flt.exclude_ids and g.n > 32:
            col = _col(arena, offs, all_jobs, i)
            assert np.isneginf(col[[0, 31, 32, g.n - 1]]).all(), label
            hit += 1
    assert hit >= 1


def test_a_shifted_column_takes_the_4_byte_path_with_the_same_result(launch):
    cs, jobs, views, all_jobs, arena, offs = launch
    assert len(views) == 3
    for v, (label, k, vj) in enumerate(views):
        got = _col(arena, offs, all_jobs, len(jobs) + v)
        want = _col(arena, offs, all_jobs, k)
        assert got.size > 1000 and np.array_equal(got.view(np.int32), want.view(np.int32)), label
        assert np.array_equal(got.view(np.int32), job_column_ref(vj).view(np.int32)), label


def test_every_column_equals_the_tenants_own(launch):
    """The second reference: the per-tenant column of the existing code."""
    cs, jobs, views, all_jobs, arena, offs = launch
    for i, (label, g, flt, boost, metric) in enumerate(cs):
        if g.n == 0:
            assert _col(arena, offs, all_jobs, i).size == 0
            continue
        ref = g.boost_bias(boost, metric, where=flt) if boost is not None else g._filter_plan(flt, metric == "l2").bias
        got = _col(arena, offs, all_jobs, i)
        assert np.array_equal(got.view(np.int32), ref.cpu().numpy().view(np.int32)), label
