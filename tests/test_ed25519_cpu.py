"""Ed25519 without a GPU: the big-integer restatement (ed25519_ref.py) against the suite's 8 vector files field by field, the
codec's sign rule, the decoding rules (non-canonical y, x = 0 with the sign bit, torsion points) through the Python point type,
and the public names."""
import glob
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ed25519_ref as r  # noqa: E402

import dot_ring_amd as d  # noqa: E402
from dot_ring_amd import _native  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILES = sorted(glob.glob(os.path.join(GOLDEN, "*", "ed25519_sha*_tai_*.json")))
FIELDS = {"pedersen": ("gamma", "proof_pk_com", "proof_r", "proof_ok", "proof_s", "proof_sb"), "thin": ("gamma", "proof_r", "proof_s"),
          "tiny": ("gamma", "proof_c", "proof_s"), "ietf": ("gamma", "proof_c", "proof_s")}


def _kind(path):
    return next(k for k in FIELDS if k in os.path.basename(path))


def test_eight_vector_files():
    assert len(FILES) == 8


@pytest.mark.parametrize("path", FILES, ids=lambda p: "/".join(p.split(os.sep)[-2:]))
def test_restatement_reproduces_vectors(path):
    kind = _kind(path)
    for v in json.load(open(path)):
        hx = lambda k: bytes.fromhex(v[k])  # noqa: E731
        sk, al, ad = hx("sk"), hx("alpha"), hx("ad")
        x = r.le(sk) % r.N
        assert r.encode(r.mul(x, r.G)) == hx("pk")
        h, _ = r.encode_to_curve(al)
        assert r.encode(h) == hx("h")
        gamma = r.mul(x, h)
        assert r.encode(gamma) == hx("gamma")
        assert r.point_to_hash(gamma).hex() == v["beta"][:64]
        if kind == "pedersen":
            proof, b = r.pedersen_prove(sk, al, ad)
            assert b == r.le(hx("blinding"))
        else:
            proof = r.ietf_prove(sk, al, ad, thin=kind == "thin")
        assert proof == b"".join(hx(f) for f in FIELDS[kind])


def test_base_point_encoding():
    assert r.encode(r.G).hex() == "58" + "66" * 31
    assert d.Ed25519.point_type.generator_point().point_to_string() == r.encode(r.G)


def test_sign_rule_is_the_references_not_parity():
    # the reference's bit is x > p - x; RFC 8032's is the parity of x.  In ark-vrf's Tiny file they differ for 3 of the 7 public keys.
    vs = json.load(open(os.path.join(GOLDEN, "ark-vrf", "ed25519_sha-512_tai_tiny.json")))
    P = d.Ed25519.point_type
    differ = 0
    for v in vs:
        pt = r.decode(bytes.fromhex(v["pk"]))
        assert r.encode(pt).hex() == v["pk"]
        assert P.string_to_point(bytes.fromhex(v["pk"])).point_to_string().hex() == v["pk"]
        differ += r.encode_parity(pt) != r.encode(pt)
    assert differ == 3


@pytest.mark.parametrize("k", range(19))
def test_non_canonical_y_rejected(k):
    enc = (r.P + k).to_bytes(32, "little")            # the 19 values of [p, 2^255)
    assert r.decode(enc, check=False) is None
    with pytest.raises(ValueError):
        d.Ed25519.point_type.string_to_point(enc)


@pytest.mark.parametrize("y", [1, r.P - 1])
def test_x_zero_with_sign_bit(y):
    # both candidates are 0, so the sign bit is ignored; (0, 1) and (0, -1) are accepted by the codec (the constructor takes both)
    P = d.Ed25519.point_type
    for sign in (0, 0x80):
        enc = bytearray(y.to_bytes(32, "little"))
        enc[31] |= sign
        pt = P.string_to_point(bytes(enc))
        assert (pt.x, pt.y) == (0, y) == r.decode(bytes(enc), check=False)
        assert r.decode(bytes(enc)) is None            # but neither is a valid prime-order point
    assert P.string_to_point(bytes(r.encode((0, y)))).point_to_string() == r.encode((0, y))


def test_torsion_points():
    tp = r.torsion_points()
    assert len(set(tp)) == 8 and all(r.on_curve(t) and r.mul(8, t) == r.O for t in tp)
    P = d.Ed25519.point_type
    for t in tp:
        enc = r.encode(t)
        assert r.decode(enc, check=False) == t and r.decode(enc) is None
        pt = P.string_to_point(enc)
        assert (pt.x, pt.y) == t
        # a prime-order point plus torsion decodes, and fails the subgroup check unless the torsion part is trivial
        q = r.add(r.mul(77, r.G), t)
        assert (r.decode(r.encode(q)) is None) == (t != r.O)


def test_public_names_and_parameters():
    assert d.Ed25519 is d.Ed25519_TAI
    assert "Ed25519" in d.__all__ and "Ed25519_TAI" in d.__all__
    sp = d.Ed25519.curve.params
    assert sp.suite_id == b"Ed25519-SHA512-TAI-v1" and sp.field_modulus == r.P and sp.subgroup_order == r.N and sp.cofactor == 8
    assert sp.curve_id == _native.CURVE_ED25519 == 3 and sp.e2c == "tai" and sp.encoding.point_len == 32
    assert tuple(sp.generator) == r.G and tuple(sp.auxiliary_points.blinding_base) == r.BLINDING


def test_point_type_uses_its_own_field():
    P = d.Ed25519.point_type
    a, b = P(*r.mul(5, r.G)), P(*r.mul(9, r.G))
    assert ((a + b).x, (a + b).y) == r.add(r.mul(5, r.G), r.mul(9, r.G))
    assert (a.double().x, a.double().y) == r.mul(10, r.G)
    assert (-a).x == -a.x % r.P
    with pytest.raises(ValueError):
        P(r.P, 1)
    assert d.Ed25519.curve.mod_sqrt(4) in (2, r.P - 2)
    with pytest.raises(ValueError):
        d.Ed25519.curve.mod_sqrt(2)                     # 2 is not a square mod 2^255 - 19
    # a coordinate above the BLS12-381 scalar field is still a valid Ed25519 coordinate
    pt = next(r.mul(k, r.G) for k in range(1, 200) if max(r.mul(k, r.G)) > d.Bandersnatch.curve.params.field_modulus)
    assert P(*pt).point_to_string() == r.encode(pt)


def test_ring_params_refuse_ed25519():
    with pytest.raises(ValueError, match="ring proofs require auxiliary point accumulator_base"):
        d.RingProofParams(cv=d.Ed25519)
