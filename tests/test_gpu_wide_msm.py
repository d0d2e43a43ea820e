"""dr_wide_msm on the GPU (csrc/wave_msm.hip.h, csrc/capi_wide_msm.hpp): ONE MSM on P-384, P-521, Ed448 and Curve448 through
ctx.wide_msm, bit for bit against closed forms of the big-integer restatements.  Sizes WIDE_PIP_FROM, 1030 and 4100: one index group,
two, and the second window width.  The families are wide_msm_cases.py's (test_wide_msm_plan_cpu.py proves on the host which bucket lists
they make): distinct ladder points under full-width scalars; one scalar for every term (the wave walk); lists of exactly 64 and 65; pairs
that cancel and points that repeat, once with the identity as the total in each suite's spelling; the edge scalars, identity points among
the inputs and, on Ed448 and Curve448, the small-order point under scalars of n and more.  Every family call follows a random MSM of the
same size on the same context, so stale scratch cannot pass for a result.  Then the hand-over at WIDE_PIP_FROM, the agreement with
dr_<suite>_msm_groups folded on the host, the refusals, n = 0, point_type.msm and the batch verifiers of 64 proofs (320 terms)."""
import ctypes
import dataclasses
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wide_msm_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", cases.SIZES)
@pytest.mark.parametrize("family", cases.FAMILIES)
@pytest.mark.parametrize("name", cases.NAMES)
def test_family_equals_the_closed_form(ctx, name, family, n):
    before = cases.ladder_case(name, n, "before-" + family)
    ctx.wide_msm(name, *before.packed())
    case = cases.case(name, family, n)
    got = ctx.wide_msm(name, *case.packed())
    assert got == case.expected()
    if family == "cancel-identity":
        assert got == cases.SUITES[name].identity


@pytest.mark.parametrize("name", cases.NAMES)
def test_hand_over_at_the_threshold(ctx, name):
    """FROM - 1 terms go through msm_groups in chunks (three of 64 and one of 63), FROM terms through the buckets: the same ladder"""
    full = cases.ladder_case(name, cases.FROM)
    below = cases.Case(name, "ladder-below", cases.FROM - 1, full.terms[:-1])
    assert ctx.wide_msm(name, *below.packed()) == below.expected()
    assert ctx.wide_msm(name, *full.packed()) == full.expected()


@pytest.mark.parametrize("name", cases.NAMES)
def test_bucket_result_equals_msm_groups_folded_on_the_host(ctx, name):
    s = cases.SUITES[name]
    case = cases.ladder_case(name, 256, "against-groups")
    pts, ks = case.packed()
    parts = getattr(ctx, f"{name}_msm_groups")(pts, ks, 64)
    step = len(s.identity)
    acc = getattr(s.ref, "O", None)
    for i in range(0, len(parts), step):
        blob = parts[i : i + step]
        half = step // 2
        pt = None if blob == s.identity and name != "ed448" else (int.from_bytes(blob[:half], "little"), int.from_bytes(blob[half:], "little"))
        acc = s.ref.add(acc, pt)
    assert ctx.wide_msm(name, pts, ks) == s.raw(acc) == case.expected()


@pytest.mark.parametrize("name", cases.NAMES)
def test_no_terms_give_the_identity(ctx, name):
    assert ctx.wide_msm(name, b"", b"") == cases.SUITES[name].identity


def _call(ctx, curve, pts, ks, n, out_len=136):
    from dot_ring_amd import _native

    out = ctypes.create_string_buffer(out_len)
    return _native.lib().dr_wide_msm(ctx.handle, curve, pts, ks, n, out), out


def test_refusals(ctx):
    from dot_ring_amd import _native

    invalid = -1
    wide = set(range(19, 27))                                  # Ed448, Curve448, P-521, P-384: RO and NU each
    case = cases.ladder_case("p384", 256)
    pts, ks = case.packed()
    for curve in list(range(-1, 19)) + [27, 28, 100]:
        assert curve not in wide
        assert _call(ctx, curve, pts, ks, 256)[0] == invalid, curve
    for name, (ro, nu) in {"ed448": (19, 20), "curve448": (21, 22), "p521": (23, 24), "p384": (25, 26)}.items():
        c = cases.ladder_case(name, 256)
        p, k = c.packed()
        for curve in (ro, nu):
            rc, out = _call(ctx, curve, p, k, 256)
            assert rc == 0 and out.raw[: len(c.expected())] == c.expected()
        for n in (256, 100):                                   # both paths check their buffers
            assert _call(ctx, ro, None, k, n)[0] == invalid and _call(ctx, ro, p, None, n)[0] == invalid
            assert _native.lib().dr_wide_msm(ctx.handle, ro, p, k, n, None) == invalid
        s = cases.SUITES[name]
        half = len(s.identity) // 2
        modulus = s.ref.P
        for n in (256, 100):
            bad = bytearray(p)
            bad[half * 3 : half * 4] = modulus.to_bytes(half, "little")          # y of the second point = p: not canonical
            assert _call(ctx, ro, bytes(bad), k, n)[0] == invalid
            with pytest.raises(ValueError, match="canonical"):
                ctx.wide_msm(name, bytes(bad[: n * 2 * half]), k[: n * s.nbytes])
    p, k = cases.ladder_case("p521", 256).packed()
    for n in (256, 100):
        big = bytearray(k)
        big[68 * 5 : 68 * 6] = (1 << 521).to_bytes(68, "little")
        assert _call(ctx, 23, p, bytes(big), n)[0] == invalid
        with pytest.raises(ValueError, match="2\\^521"):
            ctx.wide_msm("p521", p[: n * 136], bytes(big[: n * 68]))
    with pytest.raises(ValueError):
        ctx.wide_msm("blsg1", b"", b"")
    with pytest.raises(ValueError):
        ctx.wide_msm("p384", pts, ks[:-48])


def _curves():
    import dot_ring_amd as d

    return {"p384": d.P384, "p521": d.P521, "ed448": d.Ed448, "curve448": d.Curve448}


@pytest.mark.parametrize("name", cases.NAMES)
def test_point_type_msm_of_300_terms(name):
    pt_type = _curves()[name].point_type
    case = cases.ladder_case(name, 300, "python")
    lad = cases.ladder(name)
    got = pt_type.msm([pt_type(*lad[i]) for i in range(300)], case.scalars)
    assert isinstance(got, pt_type) and pt_type._pack([got]) == case.expected()


@pytest.mark.parametrize("name", cases.NAMES)
def test_batch_verify_of_64_proofs_takes_the_bucket_path(name):
    """5 x 64 = 320 terms: above WIDE_PIP_FROM.  True for honest proofs, false after one s is changed"""
    import dot_ring_amd as d

    cv = _curves()[name]
    assert 5 * 64 >= cases.FROM
    sks = [bytes([i + 1]) * 32 for i in range(64)]
    alphas = [b"wide msm %d" % i for i in range(64)]
    ads = [b"ad %d" % (i % 3) for i in range(64)]
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
