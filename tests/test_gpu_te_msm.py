"""GPU: the twisted Edwards Pippenger (te_msm_pippenger: k_te_msm_accumulate, k_te_msm_accumulate_heavy, k_te_msm_reduce, k_te_msm_fold)
on the input families of te_msm_cases.py, bit for bit against the oracle.  test_te_msm_plan_cpu.py proves on the CPU, from the library's
own plan and recoder, that these very inputs make bucket lists longer than TE_HEAVY_BUCKET (the wave kernel), lists of exactly 64 and 65
entries (the hand-over between the two accumulate kernels), lists whose lanes hold the identity or equal sums, and entries in the last
bucket of every full-width window.

Every family call follows, on the same context, a random MSM of the same size and curve that is checked too: `buckets` and `partial`
then hold foreign points, and a bucket that neither kernel wrote cannot pass for a result."""
import os
import sys
from types import SimpleNamespace

import pytest

from oracle import coracle
from oracle.pyref import bandersnatch as bsn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sw_ref  # noqa: E402
import te_msm_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu


def _by_point(case):
    """scalars summed per distinct point, mod the order"""
    total = {}
    for pt, k in zip(case.points, case.reduced):
        total[pt] = (total.get(pt, 0) + k) % case.order
    return total


def _want_raw(case, aggregate=False):
    """the 64 bytes dr_te_msm must return"""
    if case.curve == cases.BANDERSNATCH:
        if aggregate:
            total = _by_point(case)
            return coracle.te_pack([coracle.te_msm(list(total), list(total.values()))])
        return coracle.te_pack([coracle.te_msm(case.points, case.reduced)])
    if case.curve == cases.JUBJUB:
        with bsn.using(bsn.JUBJUB):
            acc = bsn.IDENTITY
            for pt, k in _by_point(case).items():
                acc = bsn._te_add_ref(acc, bsn.mul(pt, k))
        return coracle.te_pack([acc])
    acc = None
    for pt, k in _by_point(case).items():
        if pt is not None:
            acc = sw_ref.add(acc, sw_ref.mul(k, pt))
    return sw_ref.raw(acc)


def _run(ctx, case):
    if case.curve == cases.BANDERSNATCH_SW:
        raw_p = b"".join(sw_ref.raw(p) for p in case.points)
    else:
        raw_p = coracle.te_pack(case.points)
    return ctx.bsn_msm(raw_p, b"".join(k.to_bytes(32, "little") for k in case.scalars), case.curve)


def _closed_form_equal(case):
    """k * sum P_i, the sum taken over the pool with each point's multiplicity"""
    count = {}
    for pt in case.points:
        count[pt] = count.get(pt, 0) + 1
    k = case.reduced[0]
    if case.curve == cases.BANDERSNATCH:
        return coracle.te_pack([coracle.te_mul(coracle.te_msm(list(count), list(count.values())), k)])
    if case.curve == cases.JUBJUB:
        with bsn.using(bsn.JUBJUB):
            acc = bsn.IDENTITY
            for pt, c in count.items():
                acc = bsn._te_add_ref(acc, bsn.mul_py(pt, c))
            return coracle.te_pack([bsn.mul(acc, k)])
    acc = None
    for pt, c in count.items():
        acc = sw_ref.add(acc, sw_ref.mul(c, pt))
    return sw_ref.raw(sw_ref.mul(k, acc))


@pytest.mark.parametrize("name", cases.NAMES)
def test_te_msm_family_matches_oracle(ctx, name):
    case = cases.case(name)
    before = cases.random_case(case.curve, case.n)
    assert _run(ctx, before) == _want_raw(before, aggregate=True)
    got = _run(ctx, case)
    assert got == _want_raw(case)
    if "-equal-" in name:
        assert len(set(case.reduced)) == 1 and got == _closed_form_equal(case)


def test_te_msm_equal_through_the_reference_seam(ctx):
    """the equal family through the shim of the reference's msm_pippenger_signed_native_cy (bandersnatch_te.pyx:257): point objects,
    scalars centred into (-n/2, n/2], both return forms"""
    from dot_ring_amd.shims import bandersnatch_te_hip as te

    case = cases.case("bsn-equal-1030")
    order = case.order
    centred = [k - order if k > order // 2 else k for k in case.reduced]
    objs = [SimpleNamespace(x=p[0], y=p[1]) for p in case.points]
    want = coracle.te_msm(case.points, case.reduced)
    assert coracle.te_pack([want]) == _closed_form_equal(case)
    assert te.msm_pippenger_signed_native_cy(objs, centred, bsn.A, bsn.D, bsn.P, window_bits=8, affine=True) == want
    x, y, z, t = te.msm_pippenger_signed_native_cy(objs, centred, bsn.A, bsn.D, bsn.P, 8)
    zi = pow(z, -1, bsn.P)
    assert (x * zi % bsn.P, y * zi % bsn.P) == want and t * z % bsn.P == x * y % bsn.P


def test_shared_scratch_serves_a_g1_msm_after_heavy_te_lists(ctx, srs_bytes):
    """`sorted`, `counts`, `offsets` and `perm` are one scratch for every pipeline of the context: after a family full of heavy lists a KZG
    commitment of 600 coefficients (dr_g1_msm) still gives the oracle's bytes, and the family gives its own again afterwards"""
    case = cases.case("bsn-equal-65536")
    want = _closed_form_equal(case)
    assert _run(ctx, case) == want
    m = 600
    srs = ctx.srs_load(srs_bytes[: 96 * m])
    sc = b"".join(k.to_bytes(32, "little") for k in cases.seeded("te-msm-g1", m, coracle.FR_P))
    le = b"".join(srs_bytes[96 * i : 96 * i + 48][::-1] + srs_bytes[96 * i + 48 : 96 * i + 96][::-1] for i in range(m))
    g1 = coracle.g1_msm_raw(le, sc, m)
    assert ctx.g1_msm(srs, sc) == g1[:48][::-1] + g1[48:][::-1]
    srs.close()
    assert _run(ctx, cases.case("bsn-lengths-low")) == _want_raw(cases.case("bsn-lengths-low"))
    assert _run(ctx, case) == want
