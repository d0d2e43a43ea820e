"""CPU: the BLS12_381_G2 suites without a GPU — the big-integer restatement (tests/bls12_381_g2_ref.py) against RFC 9380's vector files
as the reference ships them (tests/golden/h2c/bls12_381_G2_{ro,nu}.json), the library's host hash_to_field against both, every limb
constant of csrc/fq2_28.hip.h and csrc/kernels_g2_h2c.hip.h recomputed from its integer, the clearing by psi against h_eff, the
unreachable kernel of the isogeny, the Python Fp2 and point class, the public names and the refusals.

Three strings of the NU file are no 96-digit hexadecimal field elements (97 characters each): Q0.x.re of the second record and P.y.re of
the fourth begin with a space, Q0.y.im of the third ends with a line feed.  They are listed by position; the test asserts that each of
them is malformed, that every other string is well-formed (96 digits, after `0x` in the RO file), and compares the three after
stripping the white space — so nothing is left unchecked and the list cannot widen silently."""
import json
import os
import random
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bls12_381_g2_ref as g2  # noqa: E402

import dot_ring_amd as d  # noqa: E402
from dot_ring_amd import _native  # noqa: E402
from dot_ring_amd.curve import Bls12381G2Point, Fp2  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = g2.P
R392 = 1 << 392
LENGTHS = (0, 1, 55, 56, 64, 119, 120, 517)
# (file, index of the vector, point, coordinate, component): the malformed strings
MALFORMED = {("nu", 1, "Q0", "x", "re"), ("nu", 2, "Q0", "y", "im"), ("nu", 3, "P", "y", "re")}
WELL_FORMED = {"ro": re.compile(r"0x[0-9a-f]{96}\Z"), "nu": re.compile(r"[0-9a-f]{96}\Z")}
VARIANTS = (("ro", g2.DST_RO, 2, _native.CURVE_BLS12_381_G2), ("nu", g2.DST_NU, 1, _native.CURVE_BLS12_381_G2_NU))


def vectors(name):
    with open(os.path.join(ROOT, "tests", "golden", "h2c", f"bls12_381_G2_{name}.json")) as f:
        return json.load(f)


def vector_us(vec):
    return [(int(u["re"], 16), int(u["im"], 16)) for u in vec["u"]]


def test_restatement_reproduces_the_vector_files():
    seen_malformed = set()
    for name, dst, count, _ in VARIANTS:
        doc = vectors(name)
        assert doc["dst"].encode() == dst and [len(v["msg"]) for v in doc["vectors"]] == [0, 3, 16, 133, 517]
        for idx, vec in enumerate(doc["vectors"]):
            msg = vec["msg"].encode()
            us = g2.hash_to_field(msg, count, dst)
            assert len(vec["u"]) == count and ("Q1" in vec) == (count == 2) and "Q" not in vec
            for u, rec in zip(us, vec["u"]):
                assert all(WELL_FORMED[name].match(rec[c]) for c in ("re", "im")) and (int(rec["re"], 16), int(rec["im"], 16)) == u
            images = {f"Q{j}": g2.map_to_curve(u) for j, u in enumerate(us)}
            images["P"] = g2.map_sum(us, True)
            for key, pt in images.items():
                assert g2.on_curve(pt)
                for coord, val in zip("xy", pt):
                    for comp, part in zip(("re", "im"), val):
                        text = vec[key][coord][comp]
                        if (name, idx, key, coord, comp) in MALFORMED:
                            assert not WELL_FORMED[name].match(text) and len(text) == 97
                            seen_malformed.add((name, idx, key, coord, comp))
                            text = text.strip()
                        assert WELL_FORMED[name].match(text) and int(text, 16) == part, (name, idx, key, coord, comp)
            assert (g2.encode_to_curve_ro if count == 2 else g2.encode_to_curve_nu)(msg) == images["P"]
            assert g2.in_g2(images["P"]) and g2.clear_cofactor(g2.map_sum(us, False)) == images["P"]
    assert seen_malformed == MALFORMED


def test_restatement_group_order_and_clearing():
    """G.3's clearing equals [h_eff] on random points of E(Fq2), on a point of [r] E and on the identity; #E(Fq2) = h2 r"""
    assert g2.on_curve(g2.G) and g2.in_g2(g2.G)
    assert g2.H_EFF.bit_length() == 636 and bin(g2.H_EFF).count("1") == 305 and g2.H_EFF % g2.H2 == 0
    assert (g2.H2 * g2.R_ORDER).bit_length() == 762
    assert g2.BLS_Z_ABS.bit_length() == 64 and bin(g2.BLS_Z_ABS).count("1") == 6       # 63 doublings and 5 additions a walk
    rng = random.Random(2381)
    for _ in range(6):
        q = g2.map_to_curve((rng.randrange(P), rng.randrange(P)))
        assert g2.on_curve(q) and g2.mul(g2.R_ORDER, q) is not None                     # outside G2
        assert g2.mul(g2.H2 * g2.R_ORDER, q) is None
        cleared = g2.clear_cofactor_psi(q)
        assert cleared == g2.clear_cofactor(q) and g2.in_g2(cleared)
        assert g2.on_curve(g2.psi(q)) and g2.psi2(q) == g2.psi(g2.psi(q))
    torsion = g2.mul(g2.R_ORDER, g2.map_to_curve((3, 5)))                               # in the cofactor part [r] E
    assert torsion is not None and g2.clear_cofactor_psi(torsion) is None and g2.clear_cofactor(torsion) is None
    assert g2.clear_cofactor_psi(None) is None
    q = g2.map_to_curve((1, 0))
    assert g2.add(q, g2.neg(q)) is None and g2.add(q, q) == g2.mul(2, q) and g2.mul(-3, q) == g2.neg(g2.mul(3, q))
    # the psi constants as appendix G.3 states them
    assert g2.f2_mul(g2.PSI_CX, g2.f2_pow((1, 1), (P - 1) // 3)) == g2.ONE
    assert g2.f2_mul(g2.PSI_CY, g2.f2_pow((1, 1), (P - 1) // 2)) == g2.ONE
    assert g2.PSI2_K * pow(2, (P - 1) // 3, P) % P == 1


def test_kernel_of_the_isogeny_is_unreachable():
    """The x of a point of the isogeny's kernel is a root of the x denominator; both its roots and the remaining root of the y denominator
    lie in Fq2 (they coincide: the kernel of a 3-isogeny is {O, K, -K}), and g(x) = x^3 + A' x + B' is a non-square there, so it is the x
    of no point of E'(Fq2): no input of the map has an image with Z = 0, and no test reaches the kernels' ok = 0.  Also: -1 / Z is a
    non-square, so tv1 = Z^2 u^4 + Z u^2 vanishes for u = 0 alone, and g is a square at the exceptional x1 = B' / (Z A')."""
    k0, k1 = g2.ISO_XDEN
    root_disc = g2.f2_sqrt(g2.f2_sub(g2.f2_sqr(k1), g2.f2_mul((4, 0), k0)))
    assert root_disc is not None                                                        # the roots are in Fq2
    half = g2.f2_inv((2, 0))
    r1 = g2.f2_mul(g2.f2_sub(root_disc, k1), half)
    r2 = g2.f2_mul(g2.f2_sub(g2.f2_neg(root_disc), k1), half)
    r3 = g2.f2_sub(g2.f2_sub(g2.f2_neg(g2.ISO_YDEN[2]), r1), r2)                        # the y denominator's roots sum to -k_(4,2)
    for r in (r1, r2, r3):
        assert g2._poly(g2.ISO_YDEN, r, True) == g2.ZERO and not g2.f2_is_square(g2.iso_rhs(r))
    assert g2._poly(g2.ISO_XDEN, r1, True) == g2.ZERO and g2._poly(g2.ISO_XDEN, r2, True) == g2.ZERO
    assert not g2.f2_is_square(g2.f2_neg(g2.f2_inv(g2.SSWU_Z)))
    assert g2.f2_is_square(g2.iso_rhs(g2.f2_mul(g2.ISO_B, g2.f2_inv(g2.f2_mul(g2.SSWU_Z, g2.ISO_A)))))
    assert g2.on_curve(g2.map_to_curve(g2.ZERO))


def test_native_hash_to_field_matches_vectors_and_restatement():
    """dr_blsg2_hash_to_field_batch is host code: it loads and runs without a GPU"""
    rng = random.Random(2381)
    pack = lambda u: u[0].to_bytes(48, "little") + u[1].to_bytes(48, "little")  # noqa: E731
    for name, dst, count, variant in VARIANTS:
        doc = vectors(name)
        got = _native.blsg2_hash_to_field_batch(variant, [vec["msg"].encode() for vec in doc["vectors"]])
        assert got == b"".join(pack(u) for vec in doc["vectors"] for u in vector_us(vec))
        msgs, salts = [], []
        for length in LENGTHS:
            for salt_len in (0, 32):
                msgs.append(bytes(rng.randrange(256) for _ in range(length)))
                salts.append(bytes(rng.randrange(256) for _ in range(salt_len)))
        want = b"".join(pack(u) for m, s in zip(msgs, salts) for u in g2.hash_to_field(s + m, count, dst))
        assert _native.blsg2_hash_to_field_batch(variant, [s + m for m, s in zip(msgs, salts)]) == want
        point_type = (d.BLS12_381_G2_RO if count == 2 else d.BLS12_381_G2_NU).point_type
        assert point_type.hash_to_field_pairs(msgs, salts) == want
        assert _native.blsg2_hash_to_field_batch(variant, []) == b""
    for variant in (_native.CURVE_SECP256K1, _native.CURVE_BLS12_381_G1, _native.CURVE_BLS12_381_G1_NU, 12, 19, -1):
        with pytest.raises(ValueError):
            _native.blsg2_hash_to_field_batch(variant, [b"abc"])
    for variant in (_native.CURVE_BLS12_381_G2, _native.CURVE_BLS12_381_G2_NU):          # and the G1 call refuses the G2 ids
        with pytest.raises(ValueError):
            _native.blsg1_hash_to_field_batch(variant, [b"abc"])


def _text(name):
    with open(os.path.join(ROOT, "dot_ring_amd", "csrc", name)) as f:
        return f.read()


def _limbs_value(words):
    assert len(words) == 14 and all(0 <= w < 1 << 28 for w in words)
    return sum(w << (28 * i) for i, w in enumerate(words))


def _words(text, pattern):
    m = re.search(pattern, text, re.S)
    assert m, pattern
    return [int(w.rstrip("u"), 16) for w in re.findall(r"0x[0-9a-f]+u", m.group(1))]


def _fq(text, name):
    return _limbs_value(_words(text, r"\b" + name + r"\[14\] = \{(.*?)\};"))


def _fq2(text, name):
    words = _words(text, r"\b" + name + r"\[2\]\[14\] = \{(.*?)\};")
    assert len(words) == 28
    return _limbs_value(words[:14]), _limbs_value(words[14:])


def test_every_limb_constant_of_the_two_headers():
    mont = lambda v: v % P * R392 % P  # noqa: E731
    mont2 = lambda a: (mont(a[0]), mont(a[1]))  # noqa: E731
    field, kern = _text("fq2_28.hip.h"), _text("kernels_g2_h2c.hip.h")
    assert _fq(field, "INV2") == mont(pow(2, -1, P))
    # A' = 240 i and B' = 1012 (1 + i) act through these two, Z = -(2 + i), and sqrt(-5) with 5 = norm(Z)
    assert _fq(kern, "K240") == mont(240) and g2.ISO_A == (0, 240)
    assert _fq(kern, "K1012") == mont(1012) and g2.ISO_B == (1012, 1012)
    assert _fq2(kern, "Z") == mont2(g2.SSWU_Z) and g2.f2_norm(g2.SSWU_Z) == 5
    root = _fq(kern, "SQRT_NEG5") * pow(R392, -1, P) % P
    assert root * root % P == P - 5
    names = 0
    for prefix, coeffs in (("XN", g2.ISO_XNUM), ("XD", g2.ISO_XDEN), ("YN", g2.ISO_YNUM), ("YD", g2.ISO_YDEN)):
        for j, c in enumerate(coeffs):
            assert _fq2(kern, f"{prefix}{j}") == mont2(c), (prefix, j)
            names += 1
        assert not re.search(r"\b%s%d\[2\]" % (prefix, len(coeffs)), kern)               # the monic leading 1 is not a table entry
    assert names == 13
    assert _fq2(kern, "PSI_CX") == mont2(g2.PSI_CX) and _fq2(kern, "PSI_CY") == mont2(g2.PSI_CY) and _fq(kern, "PSI2_K") == mont(g2.PSI2_K)
    # b3 = 12 (1 + i) is made of additions (no constant); b = 4 (1 + i) takes fq28.hip.h's FOUR twice; the offsets are plain multiples of p
    fq, g1h = _text("fq28.hip.h"), _text("kernels_g1_h2c.hip.h")
    assert _fq(fq, "FOUR") == mont(4) and g2.CURVE_B == (4, 4) and _fq(fq, "P") == P and _fq(fq, "ONE") == R392 % P
    assert _fq(g1h, "P18") == 18 * P and "G1hConsts::P18" in kern and "Fq28Params::P" in field
    b3 = g2.f2_mul((3, 0), g2.CURVE_B)
    assert b3 == (12, 12) and g2.f2_mul(b3, (5, 7)) == (12 * (5 - 7) % P, 12 * (5 + 7) % P)    # what mul_b3's two sums compute
    # the public scalars of the fixed walks, as 32-bit words
    scalar = lambda name, n: sum(w << (32 * i) for i, w in enumerate(_words(kern, name + r"\[%d\] = \{(.*?)\};" % n)))  # noqa: E731
    assert scalar("G2H_Z_ABS", 2) == g2.BLS_Z_ABS and scalar("G2H_R", 8) == g2.R_ORDER and g2.R_ORDER.bit_length() == 255
    assert "G2H_Z_ABS, 63)" in kern and "G2H_R, 254)" in kern                            # top bits of the two walks
    # the chain of (p - 3) / 4 is kernels_g1_h2c.hip.h's, shared as it is (test_bls12_381_g1_cpu.py recomputes it)
    assert '#include "kernels_g1_h2c.hip.h"' in field and "g1h_pow_p34" in field and "__global__" not in g1h


def test_fp2_class():
    rng = random.Random(7)
    rand = lambda: (rng.randrange(P), rng.randrange(P))  # noqa: E731
    for _ in range(20):
        a, b = rand(), rand()
        fa, fb = Fp2(*a, P), Fp2(*b, P)
        assert (fa + fb).to_tuple() == g2.f2_add(a, b) and (fa - fb).to_tuple() == g2.f2_sub(a, b)
        assert (fa * fb).to_tuple() == g2.f2_mul(a, b) and (-fa).to_tuple() == g2.f2_neg(a)
        assert fa.inv().to_tuple() == g2.f2_inv(a) and (fa / fb) * fb == fa and fa ** 3 == fa * fa * fa
        assert fa.is_square() == g2.f2_is_square(a) and fa.sgn0() == g2.f2_sgn0(a)
        assert (fa.re, fa.im, fa.p) == (a[0], a[1], P)
        sq = fa * fa
        root = sq.sqrt()
        assert root is not None and root * root == sq
        assert (fa.sqrt() is None) == (not fa.is_square())
        assert 2 * fa == fa + fa and fa + 1 == Fp2(a[0] + 1, a[1], P) and 1 - fa == -(fa - 1) and (1 / fa) * fa == 1
    for real in (0, 1, 4, 5, P - 1, P - 4):                                              # im = 0: the root is (r, 0) or (0, r)
        root = Fp2(real, 0, P).sqrt()
        assert root * root == real and (root.re == 0 or root.im == 0)
    for a, want in (((0, 0), 0), ((1, 0), 1), ((0, 1), 1), ((2, 1), 0), ((0, 2), 0), ((P - 1, 0), 0)):
        assert Fp2(*a, P).sgn0() == want == g2.f2_sgn0(a)
    assert Fp2(3, 0, P) == 3 and Fp2(3, 1, P) != 3 and Fp2(3, 1, P) != Fp2(3, 1, 7) and Fp2(0, 0, P).is_zero()
    with pytest.raises(ValueError):
        Fp2(1, 1, P) + Fp2(1, 1, 7)
    with pytest.raises(ZeroDivisionError):
        Fp2(0, 0, P).inv()


def test_point_class_host_law_names_and_refusals():
    assert d.BLS12_381_G2 is d.BLS12_381_G2_RO and d.BLS12_381_G2_NU is not d.BLS12_381_G2_RO
    for name in ("BLS12_381_G2", "BLS12_381_G2_RO", "BLS12_381_G2_NU"):
        assert name in d.__all__
    assert (_native.CURVE_BLS12_381_G2, _native.CURVE_BLS12_381_G2_NU) == (17, 18)
    for cv, e2c, curve_id in ((d.BLS12_381_G2_RO, "sswu", 17), (d.BLS12_381_G2_NU, "sswu_nu", 18)):
        params = cv.curve.params
        assert cv.name == ("BLS12_381_G2_RO" if curve_id == 17 else "BLS12_381_G2_NU")
        assert params.curve_id == curve_id and params.e2c == e2c and params.suite_id == b"BLS12381G2_XMD:SHA-256_SSWU_RO_"
        assert params.field_modulus == P and params.subgroup_order == g2.R_ORDER and params.cofactor == g2.H_EFF
        assert tuple(c.to_tuple() for c in params.generator) == g2.G and cv.point_type._COFACTOR == g2.H2
        assert params.encoding.point_len == 32 and params.encoding.challenge_len == 32
        assert issubclass(cv.point_type, Bls12381G2Point)
    point_type = d.BLS12_381_G2.point_type
    gen = point_type.generator_point()
    q_ref = g2.map_to_curve((5, 9))
    q = point_type(*q_ref)                                                               # (re, im) tuples are accepted
    assert q == point_type(Fp2(*q_ref[0], P), Fp2(*q_ref[1], P)) and isinstance(q.x, Fp2)
    assert gen.is_on_curve() and not gen.is_identity() and point_type.identity().is_identity() and point_type.identity().is_on_curve()
    as_ref = lambda pt: None if pt.is_identity() else (pt.x.to_tuple(), pt.y.to_tuple())  # noqa: E731
    assert as_ref(gen + q) == g2.add(g2.G, q_ref) and as_ref(q + q) == g2.add(q_ref, q_ref) and as_ref(-q) == g2.neg(q_ref)
    assert (q - q).is_identity() and q + point_type.identity() == q and point_type.identity() + q == q and as_ref(gen - q) == g2.add(g2.G, g2.neg(q_ref))
    assert d.BLS12_381_G2_NU.point_type(*q_ref) == q                                     # one curve, two variants
    with pytest.raises(ValueError):
        point_type((1, 1), (1, 1))                                                       # not on the curve
    with pytest.raises(ValueError):
        point_type(Fp2(1, 1, 7), Fp2(1, 1, 7))                                           # the wrong field
    with pytest.raises(ValueError):
        point_type((1, 1), None)
    for bad in (1, [1, 2], (1, 2, 3), "x"):
        with pytest.raises(TypeError):
            point_type(bad, bad)
    for other in (d.BLS12_381_G1.point_type.generator_point(), 5, None):
        with pytest.raises(TypeError):
            gen + other
        with pytest.raises(TypeError):
            gen - other
    with pytest.raises(NotImplementedError):
        gen.point_to_string()
    with pytest.raises(NotImplementedError):
        point_type.string_to_point(b"\x00")
    for cv in (d.BLS12_381_G2_RO, d.BLS12_381_G2_NU):
        for scheme in (d.TinyVRF, d.ThinVRF, d.PedersenVRF, d.RingVRF):
            with pytest.raises(ValueError, match="no point codec"):
                scheme[cv]
        with pytest.raises(ValueError):
            d.RingProofParams(cv=cv)
    assert d.TinyVRF[d.Secp256k1].cv is d.Secp256k1                                      # the other suites bind as before
