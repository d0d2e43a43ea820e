"""The bucket method under dr_te_msm (Ed25519, Baby JubJub, P-256, secp256k1, Curve25519) and dr_blsg1_msm (BLS12-381's E(Fq)) on the
GPU (csrc/wave_msm.hip.h, csrc/capi_wide_msm.hpp, csrc/narrow_law.hpp), bit for bit against closed forms of the big-integer restatements.
Sizes: NARROW_PIP_FROM (the smallest plan), 1031, 4103, 16387 and 65539 (window widths 7 - 10; 1, 2, 4, 8 and 16 index groups, none
dividing its size).  The families are narrow_msm_cases.py's (test_narrow_msm_cpu.py proves on the host which bucket lists they make).
Every family call follows a random MSM of the same size on the same context, so stale scratch cannot pass for a result.  Then the alias
ids, the hand-over at the threshold, the launch names on either side of it, dr_blsg1_msm against the loop it replaces, calls that share
the MSM workspaces, the refusals, point_type.msm and the batch verifiers."""
import ctypes
import dataclasses
import os
import sys
from functools import lru_cache

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import narrow_msm_cases as cases  # noqa: E402
import wide_msm_cases  # noqa: E402

pytestmark = pytest.mark.gpu
NATIVE = tuple(n for n in cases.NAMES if cases.SUITES[n].cv is not None)
# the launches of one bucket call, and the msm_groups kernel it replaces
STAGES = {
    "ed25519": (["k_ed_msm_prepare", "k_ed_msm_sort", "k_ed_msm_accumulate", "k_ed_msm_reduce", "k_ed_msm_fold"], "k_ed_msm_groups"),
    "bjj": (["k_bjj_msm_prepare", "k_bjj_msm_sort", "k_bjj_msm_accumulate", "k_bjj_msm_reduce", "k_bjj_msm_fold"], "k_bjj_msm_groups"),
    "p256": (["k_p256_msm_prepare", "k_p256_msm_sort", "k_p256_msm_accumulate", "k_p256_msm_reduce", "k_p256_msm_fold"], "k_p256_msm_groups"),
    "secp256k1": (["k_secp256k1_msm_prepare", "k_secp256k1_msm_sort", "k_secp256k1_msm_accumulate", "k_secp256k1_msm_reduce", "k_secp256k1_msm_fold"],
                  "k_secp256k1_msm_groups"),
    "curve25519": (["k_c25519_msm_prepare", "k_ed_msm_sort", "k_ed_msm_accumulate", "k_ed_msm_reduce", "k_ed_msm_fold"], "k_c25519_msm_groups"),
}


def msm(ctx, name, pts, ks, cv=None):
    s = cases.SUITES[name]
    return ctx.blsg1_msm(pts, ks) if s.cv is None else ctx.bsn_msm(pts, ks, cv or s.cv)


@lru_cache(maxsize=None)
def _before(name, n):
    return cases.ladder_case(name, n, "before").packed()


@pytest.mark.parametrize("name,family,n", cases.plan_keys())
def test_family_equals_the_closed_form(ctx, name, family, n):
    msm(ctx, name, *_before(name, n))
    case = cases.build(name, family, n)
    got = msm(ctx, name, *case.packed())
    assert got == case.expected()
    if family == "cancel-identity":
        assert got == cases.SUITES[name].identity


@pytest.mark.parametrize("name", NATIVE)
def test_alias_ids_take_the_same_path(ctx, name):
    s = cases.SUITES[name]
    case = cases.ladder_case(name, cases.FROM, "alias")
    for cv in s.aliases:
        assert msm(ctx, name, *case.packed(), cv=cv) == case.expected()
    assert s.aliases or name == "bjj"


def test_blsg1_nu_id(ctx):
    from dot_ring_amd import _native

    case = cases.ladder_case("blsg1", cases.FROM, "alias")
    pts, ks = case.packed()
    out = ctypes.create_string_buffer(96)
    assert _native.lib().dr_blsg1_msm(ctx.handle, _native.CURVE_BLS12_381_G1_NU, pts, ks, cases.FROM, out) == 0 and out.raw == case.expected()
    assert _native.lib().dr_blsg1_msm(ctx.handle, 3, pts, ks, cases.FROM, out) == -1
    assert ctx.blsg1_msm(b"", b"") == bytes(96)


@pytest.mark.parametrize("name", cases.NAMES)
def test_hand_over_at_the_threshold(ctx, name):
    """FROM - 1 terms go through msm_groups, FROM terms through the buckets: the same ladder, each equal to its closed form, and the
    longer one the shorter one plus its last term"""
    s = cases.SUITES[name]
    full = cases.ladder_case(name, cases.FROM)
    below = cases.Case(name, "ladder-below", cases.FROM - 1, full.terms[:-1])
    got_below, got_full = msm(ctx, name, *below.packed()), msm(ctx, name, *full.packed())
    assert got_below == below.expected() and got_full == full.expected()
    half = s.fe
    pt = lambda b: s.o if b == s.identity else (int.from_bytes(b[:half], "little"), int.from_bytes(b[half:], "little"))
    _, v, k = full.terms[-1]
    assert s.raw(s.ref.add(pt(got_below), s.ref.mul(s.red(k) % s.order, cases.ladder(name)[v]))) == got_full


def _launches(ctx, names, call):
    ctx.prof_enable(True)
    try:
        ctx.prof_reset()
        call()
        return {k: ctx.prof_get(k)[1] for k in names}
    finally:
        ctx.prof_enable(False)


@pytest.mark.parametrize("name", NATIVE)
def test_launch_names_on_either_side_of_the_threshold(ctx, name):
    """at the threshold the curve's stage kernels run and its msm_groups kernel does not; at 256 terms the launches are the two
    msm_groups the recorded surface has"""
    stages, groups = STAGES[name]
    at = cases.ladder_case(name, cases.FROM, "launch")
    got = _launches(ctx, stages + [groups, "k_size_sort"], lambda: msm(ctx, name, *at.packed()))
    assert got == {**{k: 1 for k in stages}, groups: 0, "k_size_sort": 1}
    small = cases.Case(name, "launch-256", 256, at.terms[:256])
    got = _launches(ctx, stages + [groups, "k_size_sort"], lambda: msm(ctx, name, *small.packed()))
    assert got == {**{k: 0 for k in stages}, groups: 2, "k_size_sort": 0}


def test_blsg1_msm_exists_and_equals_the_loop_it_replaces(ctx):
    """300 terms: dr_blsg1_msm (the buckets) against msm_groups in chunks of 64 and their partial sums, as Bls12381G1Point.msm looped"""
    from dot_ring_amd import _native

    assert "dr_blsg1_msm" in _native.EXPORTED_SYMBOLS and hasattr(_native.lib(), "dr_blsg1_msm")
    case = cases.ladder_case("blsg1", 300, "loop")
    pts, ks = case.packed()
    parts = ctx.blsg1_msm_groups(pts + bytes(96 * 20), ks + bytes(32 * 20), 64)
    old = ctx.blsg1_msm_groups(parts, (1).to_bytes(32, "little") * 5, 5)
    stages = ["k_blsg1_msm_prepare", "k_blsg1_msm_sort", "k_blsg1_msm_accumulate", "k_blsg1_msm_reduce", "k_blsg1_msm_fold", "k_blsg1_msm_groups"]
    got = {}
    counts = _launches(ctx, stages, lambda: got.setdefault("out", ctx.blsg1_msm(pts, ks)))
    assert got["out"] == old == case.expected()
    assert counts == {**{k: 1 for k in stages[:-1]}, "k_blsg1_msm_groups": 0}
    few = cases.Case("blsg1", "few", 100, case.terms[:100])
    counts = _launches(ctx, stages, lambda: got.setdefault("few", ctx.blsg1_msm(*few.packed())))
    assert got["few"] == few.expected() and counts == {**{k: 0 for k in stages[:-1]}, "k_blsg1_msm_groups": 2}


@pytest.mark.parametrize("name", ("ed25519", "blsg1"))
def test_a_small_call_after_a_large_one(ctx, name):
    big = cases.ladder_case(name, 65539, "state")
    assert msm(ctx, name, *big.packed()) == big.expected()
    small = cases.build(name, "edges", cases.FROM)
    assert msm(ctx, name, *small.packed()) == small.expected()
    tiny = cases.Case(name, "tiny", 3, small.terms[:3])
    assert msm(ctx, name, *tiny.packed()) == tiny.expected()


def test_between_a_wide_call_and_a_bandersnatch_call(ctx):
    """the MSM workspaces are shared: dr_wide_msm on P-384 (1031 terms), dr_te_msm on secp256k1 and Ed25519, dr_te_msm on Bandersnatch
    (300 terms, its own Pippenger), and the narrow call again"""
    from dot_ring_amd import curve

    wide = wide_msm_cases.ladder_case("p384", 1031, "shared")
    k1, ed = cases.build("secp256k1", "lengths", cases.FROM), cases.build("ed25519", "cancel-mixed", cases.FROM)
    g = curve.Bandersnatch.point_type.generator_point()
    rng = cases._rng("bandersnatch")
    ks = [rng.getrandbits(250) for _ in range(300)]
    bsn_pts, bsn_ks = curve.pack_points([g] * 300), b"".join(k.to_bytes(32, "little") for k in ks)
    bsn_want = ctx.bsn_scalar_mul_batch(curve.pack_points([g]), (sum(ks) % curve._N).to_bytes(32, "little"))
    for _ in range(2):
        assert ctx.wide_msm("p384", *wide.packed()) == wide.expected()
        assert msm(ctx, "secp256k1", *k1.packed()) == k1.expected()
        assert ctx.bsn_msm(bsn_pts, bsn_ks) == bsn_want
        assert msm(ctx, "ed25519", *ed.packed()) == ed.expected()


@pytest.mark.parametrize("name", cases.NAMES)
def test_refusals(ctx, name):
    """at the threshold and at 100 terms: null points, scalars and out, and a coordinate = p, with msm_groups' strings"""
    from dot_ring_amd import _native

    s = cases.SUITES[name]
    lib = _native.lib()
    pts, ks = cases.ladder_case(name, cases.FROM, "refuse").packed()
    out = ctypes.create_string_buffer(96)
    call = (lambda p, k, n, o: lib.dr_blsg1_msm(ctx.handle, _native.CURVE_BLS12_381_G1, p, k, n, o)) if s.cv is None else \
        (lambda p, k, n, o: lib.dr_te_msm(ctx.handle, s.cv, p, k, n, o))
    for n in (cases.FROM, 100):
        for args in ((None, ks, n, out), (pts, None, n, out), (pts, ks, n, None)):
            assert call(*args) == -1 and _native.last_error() == "null buffer"
        bad = bytearray(pts)
        bad[s.fe * 3 : s.fe * 4] = s.ref.P.to_bytes(s.fe, "little")            # y of the second point = p: not canonical
        assert call(bytes(bad), ks, n, out) == -1 and _native.last_error() == "point coordinate is not a canonical field element"
        assert call(pts, ks, n, out) == 0
    if s.cv is not None:
        assert call(pts, ks, 1 << 31, out) == -1 and _native.last_error() == "batch too large"
        assert ctx.bsn_msm(b"", b"", s.cv) == s.identity


def _curves():
    import dot_ring_amd as d

    return {"ed25519": d.Ed25519, "bjj": d.BabyJubJub, "p256": d.P256, "secp256k1": d.Secp256k1, "curve25519": d.Curve25519, "blsg1": d.BLS12_381_G1}


@pytest.mark.parametrize("name", cases.NAMES)
def test_point_type_msm_of_twice_the_threshold(name):
    pt_type = _curves()[name].point_type
    n = 2 * cases.FROM
    case = cases.ladder_case(name, n, "python")
    lad = cases.ladder(name)
    got = pt_type.msm([pt_type(*lad[i]) for i in range(n)], case.scalars)
    s = cases.SUITES[name]
    want = case.expected()
    assert isinstance(got, pt_type) and (int(got.x), int(got.y)) == (int.from_bytes(want[: s.fe], "little"), int.from_bytes(want[s.fe :], "little"))


@pytest.mark.parametrize("name", NATIVE)
def test_batch_verify_takes_the_bucket_path(name):
    """5 B (+ 2) terms with B = 103 proofs: at least twice the threshold.  True for honest proofs, false after one s is changed"""
    import dot_ring_amd as d

    cv = _curves()[name]
    B = -(-2 * cases.FROM // 5)
    sks = [bytes([i + 1]) * 32 for i in range(B)]
    alphas = [b"narrow msm %d" % i for i in range(B)]
    ads = [b"ad %d" % (i % 3) for i in range(B)]
    pks = [cv.public_key_from_secret(sk) for sk in sks]
    order = cases.SUITES[name].order
    thin = d.ThinVRF[cv].prove_batch(alphas, sks, ads)
    assert d.ThinVRF[cv].batch_verify(thin, pks, alphas, ads) is True
    thin[37] = dataclasses.replace(thin[37], s=(thin[37].s + 1) % order)
    assert d.ThinVRF[cv].batch_verify(thin, pks, alphas, ads) is False
    ped = d.PedersenVRF[cv].prove_batch(alphas, sks, ads)
    assert d.PedersenVRF[cv].batch_verify(ped, alphas, ads) is True
    ped[11] = dataclasses.replace(ped[11], s=(ped[11].s + 1) % order)
    assert d.PedersenVRF[cv].batch_verify(ped, alphas, ads) is False
