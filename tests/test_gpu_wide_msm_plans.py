"""dr_wide_msm on the GPU in the upper half of its plan (msm_plan.hpp: plan_wide_msm), bit for bit against the closed forms of
wide_msm_cases.py: window widths 9 and 10 (H = 256, and H = 512 where every lane of wave_msm_sort owns two bins and the reduction has 64
chunks per set), 8, 16 and 64 index groups, and sizes that are no multiple of their group count, so that every group bound is a ceiling
that differs from the floor.  cases.PLANS lists the sizes and what each is for; test_wide_msm_plan_cpu.py proves on the host which plans
and bucket lists they make.  Every family call follows a random MSM of the same size on the same context.  Then sizes in descending
order and other pipelines in between on the one context, whose scratch (counts, offsets, sorted, perm, buckets, partial, winsum) all of
them share, and one call per suite through the raw C ABI under the suite's second curve id."""
import ctypes
import os
import sys

import pytest

from oracle import coracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import te_msm_cases  # noqa: E402
import wide_msm_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu


def _check(ctx, name, family, n):
    case = cases.build(name, family, n)
    got = ctx.wide_msm(name, *case.packed())
    assert got == case.expected(), case.name
    return got


@pytest.mark.parametrize("name,family,n", cases.plan_keys(), ids=lambda v: str(v))
def test_family_equals_the_closed_form(ctx, name, family, n):
    before = cases.ladder_case(name, n, "before-" + family)
    ctx.wide_msm(name, *before.packed())
    got = _check(ctx, name, family, n)
    if family == "cancel-identity":
        assert got == cases.SUITES[name].identity


@pytest.mark.parametrize("name", cases.NAMES)
def test_descending_sizes_on_one_context(ctx, name):
    """after a call of 16 index groups and 512 buckets per set, the small calls run over the counts, lists, buckets and chunk sums that it
    left beyond what they write themselves"""
    for family, n in (("equal", 65539), ("ladder", 256), ("lengths", 16387), ("ladder", 1031)):
        _check(ctx, name, family, n)


def test_shared_scratch_serves_other_pipelines_between_wide_calls(ctx, srs_bytes):
    """counts, offsets, sorted, perm, buckets, partial and winsum are one scratch for dr_wide_msm, dr_te_msm and dr_g1_msm: each step has
    its own expectation"""
    _check(ctx, "p521", "equal", 65539)
    _check(ctx, "ed448", "ladder", 256)
    te = te_msm_cases.case("bsn-equal-1030")
    raw = ctx.bsn_msm(coracle.te_pack(te.points), b"".join(k.to_bytes(32, "little") for k in te.scalars), te.curve)
    assert te.curve == te_msm_cases.BANDERSNATCH and raw == coracle.te_pack([coracle.te_msm(te.points, te.reduced)])
    m = 600
    srs = ctx.srs_load(srs_bytes[: 96 * m])
    sc = b"".join(k.to_bytes(32, "little") for k in te_msm_cases.seeded("wide-msm-g1", m, coracle.FR_P))
    le = b"".join(srs_bytes[96 * i : 96 * i + 48][::-1] + srs_bytes[96 * i + 48 : 96 * i + 96][::-1] for i in range(m))
    g1 = coracle.g1_msm_raw(le, sc, m)
    assert ctx.g1_msm(srs, sc) == g1[:48][::-1] + g1[48:][::-1]
    srs.close()
    _check(ctx, "p384", "ladder", 4103)
    _check(ctx, "p521", "equal", 65539)


@pytest.mark.parametrize("name,curve", (("ed448", 20), ("curve448", 22), ("p521", 24), ("p384", 26)))
def test_second_curve_id_through_the_c_abi(ctx, name, curve):
    """the _NU id of each suite at 16387 terms (test_gpu_wide_msm.py's test_refusals calls both ids at 256)"""
    from dot_ring_amd import _native

    case = cases.build(name, "ladder", 16387)
    pts, ks = case.packed()
    out = ctypes.create_string_buffer(136)
    assert _native.lib().dr_wide_msm(ctx.handle, curve, pts, ks, case.n, out) == 0
    want = case.expected()
    assert out.raw[: len(want)] == want and out.raw[len(want) :] == bytes(136 - len(want))
