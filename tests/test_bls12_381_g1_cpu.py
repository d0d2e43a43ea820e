"""CPU: the BLS12_381_G1 suites without a GPU — the big-integer restatement (tests/bls12_381_g1_ref.py) against RFC 9380's vector files
as the reference ships them (tests/golden/h2c/bls12_381_G1_{ro,nu}.json), the library's host hash_to_field against both, every limb
constant of csrc/kernels_g1_h2c.hip.h recomputed from its integer, the public names, the Python codec and the VRF refusals.

Five strings of the two files are no 96-digit hexadecimal field elements: in the RO file Q1.x of the 133-byte message (97 digits) and
Q0.y, Q1.x and Q1.y of the 517-byte message (97, 95 and 95 digits), in the NU file Q.y of the empty message (96 characters, one of them
a space where the restatement has the digit c).  The reference's own test reads `P` only.  Those five are skipped by position; the
test asserts that each of them is malformed and that every other string is 96 hexadecimal digits, so the skip cannot widen silently."""
import json
import os
import random
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bls12_381_g1_ref as g1  # noqa: E402

import dot_ring_amd as d  # noqa: E402
from dot_ring_amd import _native  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = g1.P
R392 = 1 << 392
LENGTHS = (0, 1, 55, 56, 64, 119, 120, 517)
# (file, index of the vector, point, coordinate): the malformed strings
MALFORMED = {("ro", 3, "Q1", "x"), ("ro", 4, "Q0", "y"), ("ro", 4, "Q1", "x"), ("ro", 4, "Q1", "y"), ("nu", 0, "Q", "y")}
WELL_FORMED = re.compile(r"[0-9a-f]{96}\Z")


def vectors(name):
    with open(os.path.join(ROOT, "tests", "golden", "h2c", f"bls12_381_G1_{name}.json")) as f:
        return json.load(f)


VARIANTS = (("ro", g1.DST_RO, 2, _native.CURVE_BLS12_381_G1), ("nu", g1.DST_NU, 1, _native.CURVE_BLS12_381_G1_NU))


def test_restatement_reproduces_the_vector_files():
    seen_malformed = set()
    for name, dst, count, _ in VARIANTS:
        doc = vectors(name)
        assert doc["dst"].encode() == dst and len(doc["vectors"]) == 5
        for idx, vec in enumerate(doc["vectors"]):
            msg = vec["msg"].encode()
            us = g1.hash_to_field(msg, count, dst)
            assert [int(u, 16) for u in vec["u"]] == us
            images = {"Q0": g1.map_to_curve(us[0]), "Q1": g1.map_to_curve(us[1])} if count == 2 else {"Q": g1.map_to_curve(us[0])}
            for key, pt in images.items():
                assert g1.on_curve(pt)
                for coord, val in zip("xy", pt):
                    text = vec[key][coord]
                    if (name, idx, key, coord) in MALFORMED:
                        assert not WELL_FORMED.match(text)
                        seen_malformed.add((name, idx, key, coord))
                        continue
                    assert WELL_FORMED.match(text) and int(text, 16) == val, (name, idx, key, coord)
            want = (int(vec["P"]["x"], 16), int(vec["P"]["y"], 16))
            assert WELL_FORMED.match(vec["P"]["x"]) and WELL_FORMED.match(vec["P"]["y"])
            assert g1.map_sum(us, True) == want
            assert (g1.encode_to_curve_ro if count == 2 else g1.encode_to_curve_nu)(msg) == want
            assert g1.valid_point(want)
    assert seen_malformed == MALFORMED


def test_restatement_group_and_codec():
    assert g1.on_curve(g1.G) and g1.valid_point(g1.G) and g1.mul(g1.R_ORDER, g1.G) is None
    assert g1.H_EFF.bit_length() == 64 and bin(g1.H_EFF).count("1") == 7           # 63 doublings and 6 additions
    q = g1.map_to_curve(5)                                                        # a point of E(Fq) outside G1
    assert g1.on_curve(q) and not g1.valid_point(q) and g1.mul(g1.R_ORDER, q) is not None
    assert g1.mul(g1.H * g1.R_ORDER, q) is None and g1.valid_point(g1.clear_cofactor(q))
    assert g1.add(q, g1.neg(q)) is None and g1.add(q, q) == g1.mul(2, q) and g1.mul(-3, q) == g1.neg(g1.mul(3, q))
    # the tv1 = 0 branch of the map: u = 0 and u^2 = -1 / Z
    s = g1.sqrt(-pow(g1.SSWU_Z, -1, P) % P)
    assert s is not None and (g1.SSWU_Z * g1.SSWU_Z * pow(s, 4, P) + g1.SSWU_Z * s * s) % P == 0
    for u in (0, s, P - s):
        assert g1.on_curve(g1.map_to_curve(u))
    for pt in (g1.G, q, g1.neg(q)):
        for compressed in (True, False):
            enc = g1.sec1_encode(pt, compressed)
            assert len(enc) == (49 if compressed else 97) and g1.sec1_decode(enc) == pt
        hybrid = bytes([6 + (pt[1] & 1)]) + g1.sec1_encode(pt, False)[1:]
        assert g1.sec1_decode(hybrid) == pt
        assert g1.sec1_decode(bytes([7 - (pt[1] & 1)]) + hybrid[1:]) == "bad"
    assert g1.sec1_encode(None) == b"\x00" and g1.sec1_decode(b"\x00") is None
    assert g1.sec1_decode(b"\x02" + P.to_bytes(48, "big")) == "bad" and g1.sec1_decode(b"\x05" + bytes(48)) == "bad"
    assert g1.sec1_decode(b"") == "bad" and g1.sec1_decode(b"\x00\x00") == "bad" and g1.sec1_decode(b"\x02" + bytes(47)) == "bad"


def test_kernel_inputs_of_the_isogeny():
    """KERNEL_US: the SSWU image is a point of E' whose x is a root of both monic denominators, and the restatement raises there"""
    xs = set()
    for u in g1.KERNEL_US:
        assert 0 < u < P
        x, y = g1.sswu(u)
        assert (y * y - (x ** 3 + g1.ISO_A * x + g1.ISO_B)) % P == 0
        assert g1._poly(g1.ISO_XDEN, x, True) == 0 and g1._poly(g1.ISO_YDEN, x, True) == 0
        with pytest.raises(ValueError):
            g1.map_to_curve(u)
        xs.add(x)
    assert len(xs) >= 2                                                           # more than one point of the kernel is reached


def test_native_hash_to_field_matches_vectors_and_restatement():
    """dr_blsg1_hash_to_field_batch is host code: it loads and runs without a GPU"""
    rng = random.Random(381)
    for name, dst, count, variant in VARIANTS:
        doc = vectors(name)
        got = _native.blsg1_hash_to_field_batch(variant, [vec["msg"].encode() for vec in doc["vectors"]])
        assert got == b"".join(int(u, 16).to_bytes(48, "little") for vec in doc["vectors"] for u in vec["u"])
        msgs, salts = [], []
        for length in LENGTHS:
            for salt_len in (0, 32):
                msgs.append(bytes(rng.randrange(256) for _ in range(length)))
                salts.append(bytes(rng.randrange(256) for _ in range(salt_len)))
        want = b"".join(u.to_bytes(48, "little") for m, s in zip(msgs, salts) for u in g1.hash_to_field(s + m, count, dst))
        assert _native.blsg1_hash_to_field_batch(variant, [s + m for m, s in zip(msgs, salts)]) == want
        point_type = (d.BLS12_381_G1_RO if count == 2 else d.BLS12_381_G1_NU).point_type
        assert point_type.hash_to_field_pairs(msgs, salts) == want
        assert _native.blsg1_hash_to_field_batch(variant, []) == b""
    for variant in (_native.CURVE_SECP256K1, _native.CURVE_CURVE25519_NU, 12, 17, -1):
        with pytest.raises(ValueError):
            _native.blsg1_hash_to_field_batch(variant, [b"abc"])


def _header():
    with open(os.path.join(ROOT, "dot_ring_amd", "csrc", "kernels_g1_h2c.hip.h")) as f:
        return f.read()


def _limbs_value(words):
    assert len(words) == 14 and all(0 <= w < 1 << 28 for w in words)
    return sum(w << (28 * i) for i, w in enumerate(words))


def _array(text, name):
    m = re.search(r"\b" + name + r"\[14\] = \{(.*?)\};", text, re.S)
    return _limbs_value([int(w.rstrip("u"), 16) for w in re.findall(r"0x[0-9a-f]+u", m.group(1))])


def _table(text, name, rows):
    m = re.search(r"\b" + name + r"\[%d\]\[14\] = \{(.*?)\};" % rows, text, re.S)
    words = [int(w.rstrip("u"), 16) for w in re.findall(r"0x[0-9a-f]+u", m.group(1))]
    assert len(words) == 14 * rows
    return [_limbs_value(words[14 * i : 14 * i + 14]) for i in range(rows)]


def test_every_limb_constant_of_the_description():
    text = _header()
    mont = lambda v: v * R392 % P  # noqa: E731
    assert _array(text, "A") == mont(g1.ISO_A) and _array(text, "B") == mont(g1.ISO_B) and _array(text, "Z") == mont(g1.SSWU_Z)
    root = _array(text, "SQRT_NEG_Z") * pow(R392, -1, P) % P
    assert root * root % P == -g1.SSWU_Z % P
    assert _array(text, "P18") == 18 * P                                          # a plain multiple of p, no Montgomery factor
    for name, coeffs in (("G1H_XN", g1.ISO_XNUM), ("G1H_XD", g1.ISO_XDEN), ("G1H_YN", g1.ISO_YNUM), ("G1H_YD", g1.ISO_YDEN)):
        assert _table(text, name, len(coeffs)) == [mont(c) for c in coeffs], name
    assert len(g1.ISO_XNUM) + len(g1.ISO_XDEN) + len(g1.ISO_YNUM) + len(g1.ISO_YDEN) == 53
    # the R-forms the description takes from fq28.hip.h
    with open(os.path.join(ROOT, "dot_ring_amd", "csrc", "fq28.hip.h")) as f:
        fq = f.read()
    assert _array(fq, "P") == P and _array(fq, "ONE") == R392 % P and _array(fq, "R2") == R392 * R392 % P and _array(fq, "FOUR") == mont(4)
    # the addition chain: x^3, then per entry c: c >> 2 squarings and a product with x^(2 (c & 3) + 1); G1H_POW_TAIL squarings
    chain = [int(v) for v in re.search(r"G1H_POW_CHAIN\[105\] = \{(.*?)\};", text, re.S).group(1).split(",")]
    first, tail = (int(v) for v in re.search(r"G1H_POW_FIRST = (\d+), G1H_POW_TAIL = (\d+);", text).groups())
    exponent = first
    for c in chain:
        assert 0 < c >> 2 < 64
        exponent = (exponent << (c >> 2)) + 2 * (c & 3) + 1
    assert len(chain) == 105 and first == 3 and exponent << tail == (P - 3) // 4 and P % 4 == 3
    # the public scalars of the fixed chains, as 32-bit words
    words = lambda name, n: [int(w.rstrip("u"), 16) for w in re.findall(r"0x[0-9a-f]+u", re.search(name + r"\[%d\] = \{(.*?)\};" % n, text).group(1))]  # noqa: E731
    assert sum(w << (32 * i) for i, w in enumerate(words("G1H_H_EFF", 2))) == g1.H_EFF
    assert sum(w << (32 * i) for i, w in enumerate(words("G1H_R", 8))) == g1.R_ORDER and g1.R_ORDER.bit_length() == 255


def test_public_names():
    assert d.BLS12_381_G1 is d.BLS12_381_G1_RO and d.BLS12_381_G1_NU is not d.BLS12_381_G1_RO
    for name in ("BLS12_381_G1", "BLS12_381_G1_RO", "BLS12_381_G1_NU"):
        assert name in d.__all__
    assert d.BLS12_381_G1_RO.name == "BLS12_381_G1_RO" and d.BLS12_381_G1_NU.name == "BLS12_381_G1_NU"
    for cv, e2c, curve_id in ((d.BLS12_381_G1_RO, "sswu", 15), (d.BLS12_381_G1_NU, "sswu_nu", 16)):
        params = cv.curve.params
        assert params.curve_id == curve_id and params.e2c == e2c and params.suite_id == b"BLS12381G1_XMD:SHA-256_SSWU_RO_"
        assert params.field_modulus == P and params.subgroup_order == g1.R_ORDER and params.cofactor == g1.H_EFF
        assert tuple(params.generator) == g1.G and cv.point_type._COFACTOR == g1.H
        assert params.encoding.point_len == 32 and params.encoding.challenge_len == 48       # the reference's own (contradictory) figures
    assert (_native.CURVE_BLS12_381_G1, _native.CURVE_BLS12_381_G1_NU) == (15, 16)


def test_python_codec_round_trips_without_a_kernel():
    """identity, uncompressed and hybrid strings are host code; compressed ones go through the decode kernel (test_gpu_bls12_381_g1.py)"""
    point_type = d.BLS12_381_G1.point_type
    gen = point_type.generator_point()
    q = point_type(*g1.map_to_curve(5))
    assert gen.is_on_curve() and not gen.is_identity() and point_type.identity().is_identity()
    assert point_type.identity().point_to_string() == b"\x00" and point_type.string_to_point(b"\x00").is_identity()
    for pt in (gen, q, -q):
        assert pt.point_to_string() == g1.sec1_encode((pt.x, pt.y)) and len(pt.point_to_string()) == 49
        full = pt.point_to_string(compressed=False)
        assert full == g1.sec1_encode((pt.x, pt.y), False) and point_type.string_to_point(full) == pt
        assert point_type.string_to_point(full.hex()) == pt
        assert point_type.string_to_point(bytes([6 + pt.y % 2]) + full[1:]) == pt
        with pytest.raises(ValueError):
            point_type.string_to_point(bytes([7 - pt.y % 2]) + full[1:])
    assert gen + q == point_type(*g1.add(g1.G, (q.x, q.y))) and q - q == point_type.identity() and q.double() == q + q
    for bad in (b"", b"\x00\x00", b"\x02" + bytes(47), b"\x04" + bytes(95), b"\x05" + bytes(48), b"\x04" + bytes(96),
                b"\x02" + P.to_bytes(48, "big"), b"\x04" + P.to_bytes(48, "big") + bytes(48), b"\x04" + bytes(48) + P.to_bytes(48, "big")):
        with pytest.raises(ValueError):
            point_type.string_to_point(bad)
    with pytest.raises(ValueError):
        point_type(1, 1)


def test_vrf_classes_and_ring_params_refuse():
    for cv in (d.BLS12_381_G1_RO, d.BLS12_381_G1_NU):
        for scheme in (d.TinyVRF, d.ThinVRF, d.PedersenVRF, d.RingVRF):
            with pytest.raises(ValueError, match="point length for this curve is 32 while its points encode to 49 bytes"):
                scheme[cv]
        with pytest.raises(ValueError):
            d.RingProofParams(cv=cv)
    assert d.TinyVRF[d.Secp256k1].cv is d.Secp256k1                                # the other suites bind as before
