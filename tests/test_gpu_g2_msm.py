"""Sums of scalar multiples on BLS12-381's E(Fq2) on the GPU: dr_blsg2_msm (csrc/kernels_g2_msm.hip.h: wave_msm.hip.h's bucket method
over G2hCurve, csrc/g2_law.hpp on the host) and dr_blsg2_msm_groups (k_blsg2_msm_groups), bit for bit against closed forms of the
big-integer restatement, and what Bls12381G2Point builds on them: msm and the classmethods scalar_mul_batch, msm_groups and
valid_points.  The families are g2_msm_cases.py's (test_g2_msm_cpu.py proves on the host which bucket
lists they make): the threshold with all six, 1031 (two uneven index groups), 4103 (width 8, four groups) and 16387 (width 9, eight
groups).  Every family call follows a random MSM of the same size on the same context, so stale scratch cannot pass for a result."""
import ctypes
import os
import random
import sys
from functools import lru_cache

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bls12_381_g2_ref as g2  # noqa: E402
import g2_msm_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu
STAGES = ["k_blsg2_msm_prepare", "k_blsg2_msm_sort", "k_blsg2_msm_accumulate", "k_blsg2_msm_reduce", "k_blsg2_msm_fold"]
GROUPS = "k_blsg2_msm_groups"


@lru_cache(maxsize=None)
def _before(n):
    return cases.ladder_case(cases.NAME, n, "before").packed()


@pytest.mark.parametrize("family,n", cases.plan_keys())
def test_family_equals_the_closed_form(ctx, family, n):
    ctx.blsg2_msm(*_before(n))
    case = cases.build(cases.NAME, family, n)
    got = ctx.blsg2_msm(*case.packed())
    assert got == case.expected()
    if family == "cancel-identity":
        assert got == bytes(192)


def _launches(ctx, names, call):
    ctx.prof_enable(True)
    try:
        ctx.prof_reset()
        call()
        return {k: ctx.prof_get(k)[1] for k in names}
    finally:
        ctx.prof_enable(False)


def test_hand_over_at_the_threshold(ctx):
    """FROM - 1 terms go through msm_groups' kernel, FROM terms through the buckets: the same ladder, each equal to its closed form, the
    longer one the shorter one plus its last term, and the launches on either side are the ones the header names"""
    full = cases.ladder_case(cases.NAME, cases.FROM)
    below = cases.Case(cases.NAME, "ladder-below", cases.FROM - 1, full.terms[:-1])
    got = {}
    counts = _launches(ctx, STAGES + [GROUPS], lambda: got.setdefault("below", ctx.blsg2_msm(*below.packed())))
    chunks = (1 if (cases.FROM - 1) // 64 else 0) + (1 if (cases.FROM - 1) % 64 else 0)
    assert counts == {**{k: 0 for k in STAGES}, GROUPS: chunks} and got["below"] == below.expected()
    counts = _launches(ctx, STAGES + [GROUPS], lambda: got.setdefault("full", ctx.blsg2_msm(*full.packed())))
    assert counts == {**{k: 1 for k in STAGES}, GROUPS: 0} and got["full"] == full.expected()
    _, v, k = full.terms[-1]
    assert cases.raw(g2.add(cases.point_of(got["below"]), g2.mul(k % g2.R_ORDER, cases.ladder(cases.NAME)[v]))) == got["full"]


def test_either_curve_id_and_no_terms(ctx):
    from dot_ring_amd import _native

    case = cases.ladder_case(cases.NAME, cases.FROM, "alias")
    assert ctx.blsg2_msm(*case.packed(), curve=_native.CURVE_BLS12_381_G2_NU) == case.expected() == ctx.blsg2_msm(*case.packed())
    assert ctx.blsg2_msm(b"", b"") == bytes(192)
    few = cases.Case(cases.NAME, "few", 3, cases.build(cases.NAME, "edges", cases.FROM).terms[1:4])
    assert ctx.blsg2_msm(*few.packed()) == few.expected()


# ---------------------------------------------------------------- dr_blsg2_msm_groups
E_ORDER = cases.ORDER_E
EDGE_SCALARS = (0, g2.R_ORDER, E_ORDER - 1, 1 << 767, (1 << 768) - 1)
GROUP_SHAPES = ((64, 1), (64, 2), (3, 22), (2, 33), (1, 65))       # a wave exactly, two workgroups, a tail (66 and 65 lanes)


def _group_terms(m, groups):
    """(kind, ladder index, scalar) per term: the edge scalars and full 768-bit ones over ladder points, one repeated point, the
    identity and the point outside G2; where there is more than one group the LAST one is (P, -P) pairs under one scalar each (m odd:
    and the identity)"""
    rng = random.Random(f"g2-msm-groups/{m}/{groups}")
    terms = []
    for i in range(m * groups):
        k = EDGE_SCALARS[(i // 3) % 5] if i % 3 == 0 else rng.getrandbits(768)
        kind = "special" if i % 7 == 3 else "id" if i % 11 == 5 else "m"
        terms.append((kind, 5 if i % 13 == 2 else i % 48, k))
    last = []
    for j in range(m // 2):
        k = rng.getrandbits(768)
        last += [("m", j, k), ("neg", j, k)]
    if m % 2:
        last.append(("id", 0, rng.getrandbits(768)))
    if groups > 1:
        terms[m * (groups - 1) :] = last
    if m == 1:
        terms[1], terms[2] = ("m", 3, 0), ("m", 4, g2.R_ORDER)        # 0 P and r P for P in G2: the identity both
    return terms


def _group_sum(terms):
    total = sum(k * (cases.LADDER_A + v) * (1 if kind == "m" else -1) for kind, v, k in terms if kind in ("m", "neg")) % g2.R_ORDER
    out = g2.mul(total, g2.G)
    outside = sum(k for kind, _, k in terms if kind == "special") % E_ORDER
    return g2.add(out, g2.mul(outside, cases.SPECIAL)) if outside else out


@pytest.mark.parametrize("m,groups", GROUP_SHAPES)
def test_msm_groups_equal_the_restatement(ctx, m, groups):
    lad = cases.ladder(cases.NAME)
    terms = _group_terms(m, groups)
    kinds = {kind for kind, _, _ in terms}
    assert len(terms) == m * groups and {"m", "id", "special"} <= kinds and set(EDGE_SCALARS) <= {k for _, _, k in terms}
    raw_of = {"m": lambda v: cases.raw(lad[v]), "neg": lambda v: cases.raw(g2.neg(lad[v])), "id": lambda v: bytes(192),
              "special": lambda v: cases.raw(cases.SPECIAL)}
    pts = b"".join(raw_of[kind](v) for kind, v, _ in terms)
    ks = b"".join(k.to_bytes(96, "little") for _, _, k in terms)
    got = ctx.blsg2_msm_groups(pts, ks, m)
    want = [cases.raw(_group_sum(terms[g * m : (g + 1) * m])) for g in range(groups)]
    assert [got[192 * g : 192 * g + 192] for g in range(groups)] == want
    assert groups == 1 or want[-1] == bytes(192)
    assert m > 1 or want[1] == want[2] == bytes(192)
    assert ctx.blsg2_msm_groups(b"", b"", m) == b""


# ---------------------------------------------------------------- refusals
def test_refusals_leave_the_context_usable(ctx):
    from dot_ring_amd import _native

    lib = _native.lib()
    case = cases.ladder_case(cases.NAME, cases.FROM, "refuse")
    pts, ks = case.packed()
    out = ctypes.create_string_buffer(192)
    msm = lambda p, k, n, o, cv=_native.CURVE_BLS12_381_G2: lib.dr_blsg2_msm(ctx.handle, cv, p, k, n, o)
    for cv in (0, 3, 15, 16, 19, -1):
        assert msm(pts, ks, cases.FROM, out, cv) == -1 and "DR_CURVE_BLS12_381_G2" in _native.last_error()
    bad = bytearray(pts)
    bad[48 * 7 : 48 * 8] = g2.P.to_bytes(48, "little")                        # y.c1 of the second point = p: not canonical
    for n in (cases.FROM, 100):
        for args in ((None, ks, n, out), (pts, None, n, out), (pts, ks, n, None)):
            assert msm(*args) == -1 and _native.last_error() == "null buffer"
        assert msm(bytes(bad), ks, n, out) == -1 and _native.last_error() == "point coordinate is not a canonical field element"
        assert msm(pts, ks, n, out) == 0
    assert msm(pts, ks, 1 << 28, out) == -1 and _native.last_error() == "batch too large"
    wide = b"".join(k.to_bytes(96, "little") for k in case.scalars[:64])
    outs = ctypes.create_string_buffer(192 * 64)
    groups = lambda p, k, g, m, o: lib.dr_blsg2_msm_groups(ctx.handle, p, k, g, m, o)
    for m in (0, 65):
        assert groups(pts, wide, 1, m, outs) == -1 and _native.last_error() == "group size must be in 1..64"
    for args in ((None, wide, 2, 32, outs), (pts, None, 2, 32, outs), (pts, wide, 2, 32, None)):
        assert groups(*args) == -1 and _native.last_error() == "null buffer"
    assert groups(bytes(bad), wide, 2, 32, outs) == -1 and _native.last_error() == "point coordinate is not a canonical field element"
    assert groups(pts, wide, 1 << 28, 1, outs) == -1 and _native.last_error() == "batch too large"
    assert groups(pts, wide, 0, 32, None) == 0
    assert groups(pts, wide, 2, 32, outs) == 0
    assert ctx.blsg2_msm(pts, ks) == case.expected()


# ---------------------------------------------------------------- calls that share the context's workspaces
def test_a_small_call_after_a_large_one(ctx):
    big = cases.ladder_case(cases.NAME, 4103, "state")
    assert ctx.blsg2_msm(*big.packed()) == big.expected()
    small = cases.Case(cases.NAME, "small", 64, cases.build(cases.NAME, "edges", cases.FROM).terms[:64])
    assert ctx.blsg2_msm(*small.packed()) == small.expected()


def test_between_a_g1_call_and_a_bandersnatch_call(ctx):
    """dr_blsg1_msm of 257 terms (the same stage templates over E(Fq)) and Bandersnatch's own Pippenger between two G2 calls"""
    import narrow_msm_cases
    from dot_ring_amd import curve

    first, second = cases.build(cases.NAME, "lengths", cases.FROM), cases.build(cases.NAME, "edges", 1031)
    g1 = narrow_msm_cases.ladder_case("blsg1", 257, "shared")
    g = curve.Bandersnatch.point_type.generator_point()
    rng = random.Random("g2-msm/bandersnatch")
    ks = [rng.getrandbits(250) for _ in range(300)]
    bsn_pts, bsn_ks = curve.pack_points([g] * 300), b"".join(k.to_bytes(32, "little") for k in ks)
    bsn_want = ctx.bsn_scalar_mul_batch(curve.pack_points([g]), (sum(ks) % curve._N).to_bytes(32, "little"))
    for _ in range(2):
        assert ctx.blsg2_msm(*first.packed()) == first.expected()
        assert ctx.blsg1_msm(*g1.packed()) == g1.expected()
        assert ctx.bsn_msm(bsn_pts, bsn_ks) == bsn_want
        assert ctx.blsg2_msm(*second.packed()) == second.expected()


# ---------------------------------------------------------------- the point class
def _pt_type():
    import dot_ring_amd as d

    return d.BLS12_381_G2.point_type


def _obj(pt):
    t = _pt_type()
    return t.identity() if pt is None else t(*pt)


def _ref(pt):
    return None if pt.is_identity() else ((pt.x.re, pt.x.im), (pt.y.re, pt.y.im))


def test_point_type_msm_of_twice_the_threshold():
    n = 2 * cases.FROM
    case = cases.ladder_case(cases.NAME, n, "python")
    lad = cases.ladder(cases.NAME)
    got = _pt_type().msm([_obj(lad[i]) for i in range(n)], case.scalars)
    assert isinstance(got, _pt_type()) and cases.raw(_ref(got)) == case.expected()


def test_point_type_msm_with_wide_and_negative_scalars():
    """300 terms, scalars -5 and 2^770 + 12345 among them: both are reduced mod h2 r and split in three, so 304 terms take the buckets"""
    lad = cases.ladder(cases.NAME)
    rng = random.Random("g2-msm/python-wide")
    ks = [rng.getrandbits(256) for _ in range(300)]
    ks[17], ks[211] = -5, (1 << 770) + 12345
    pts = [_obj(lad[i]) for i in range(300)]
    pts[42] = _obj(cases.SPECIAL)
    got = _pt_type().msm(pts, ks)
    total = sum(k * (cases.LADDER_A + i) for i, k in enumerate(ks) if i != 42) % g2.R_ORDER
    assert _ref(got) == g2.add(g2.mul(total, g2.G), g2.mul(ks[42], cases.SPECIAL))
    few = _pt_type().msm(pts[15:20], ks[15:20])
    assert _ref(few) == g2.mul(sum(k * (cases.LADDER_A + i) for i, k in zip(range(15, 20), ks[15:20])) % g2.R_ORDER, g2.G)


def test_point_type_msm_of_nothing_and_of_unequal_lengths():
    t = _pt_type()
    assert t.msm([], []).is_identity()
    with pytest.raises(ValueError, match="same length"):
        t.msm([t.generator_point()], [1, 2])
    assert t.msm([t.generator_point(), t.identity()], [0, 5]).is_identity()


def test_batch_classmethods_of_the_point_type():
    """scalar_mul_batch and msm_groups as classmethods of Bls12381G2Point (the module-level helpers keep their recorded behaviour on
    this type: tests/golden/point_surface_*.json)"""
    t = _pt_type()
    hashed = g2.encode_to_curve_ro(b"g2 batch helpers")
    base = [g2.G, hashed, cases.SPECIAL, None, cases.SPECIAL]
    ks = [5, -7, (1 << 769) + 3, g2.R_ORDER, g2.R_ORDER + 1]
    got = t.scalar_mul_batch([_obj(p) for p in base], ks)
    assert [_ref(p) for p in got] == [g2.mul(k, p) for k, p in zip(ks, base)]
    assert t.scalar_mul_batch([], []) == [] and t.msm_groups([], [], 2) == []
    with pytest.raises(ValueError, match="same length"):
        t.scalar_mul_batch([t.generator_point()], [1, 2])
    # groups of 2 through dr_blsg2_msm_groups, 96-byte scalars as they are where they fit
    pts = [g2.G, hashed, cases.SPECIAL, g2.neg(cases.SPECIAL), None, g2.G]
    ks = [3, (1 << 700) + 9, -2, -2, 11, (1 << 768) + 1]
    got = t.msm_groups([_obj(p) for p in pts], ks, 2)
    want = [g2.add(g2.mul(ks[i], pts[i]), g2.mul(ks[i + 1], pts[i + 1])) for i in (0, 2, 4)]
    assert [_ref(p) for p in got] == want and want[1] is None
    # groups of more than 64: one msm each
    lad = cases.ladder(cases.NAME)
    rng = random.Random("g2-msm/groups-of-65")
    ks = [rng.getrandbits(256) for _ in range(130)]
    got = t.msm_groups([_obj(lad[i]) for i in range(130)], ks, 65)
    want = [g2.mul(sum(k * (cases.LADDER_A + i) for i, k in zip(range(a, a + 65), ks[a : a + 65])) % g2.R_ORDER, g2.G) for a in (0, 65)]
    assert [_ref(p) for p in got] == want


def test_valid_points_is_the_reference_s_valid_point():
    hashed = g2.encode_to_curve_ro(b"g2 valid points")
    r_special = g2.mul(g2.R_ORDER, cases.SPECIAL)
    assert r_special is not None and g2.on_curve(r_special)
    pts = [_obj(p) for p in (g2.G, hashed, cases.SPECIAL, None, r_special)]
    assert _pt_type().valid_points(pts) == [True, True, False, False, False]
    assert [_pt_type().valid_points([p])[0] for p in pts[:3]] == [True, True, False] and _pt_type().valid_points([]) == []
    # the reference's own two conditions on the same points, by the restatement
    c = pow(g2.H_EFF, -1, g2.R_ORDER)
    for p, want in zip((g2.G, hashed, cases.SPECIAL, r_special), (True, True, False, False)):
        cleared = g2.mul(g2.H_EFF, p)
        assert (cleared is not None and g2.mul(c, cleared) == p) is want
