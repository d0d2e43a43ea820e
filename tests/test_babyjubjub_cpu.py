"""Baby JubJub without a GPU: the big-integer restatement (babyjubjub_ref.py) against the suite's 8 vector files field by field, the
curve's constants, the codec's sign rule, the decoding rules (non-canonical y, bit 254, x = 0 with the sign bit, torsion points)
through the Python point type, the try-and-increment mask, the public names and the refusal of ring proofs."""
import glob
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import babyjubjub_ref as r  # noqa: E402

import dot_ring_amd as d  # noqa: E402
from dot_ring_amd import _native  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILES = sorted(glob.glob(os.path.join(GOLDEN, "*", "baby*jubjub_sha*_tai_*.json")))
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


def test_curve_constants():
    assert r.P.bit_length() == 254 and r.N.bit_length() == 251
    assert (r.P - 1) % (1 << 28) == 0 and ((r.P - 1) >> 28) % 2 == 1
    assert not r.is_square(r.D)                 # d a non-residue, a = 1 a square: the unified addition is complete
    assert r.is_square(r.A)
    assert not r.is_square(r.NONRESIDUE) and all(r.is_square(z) for z in range(1, r.NONRESIDUE))
    assert (-pow(r.P, -1, 1 << 29)) % (1 << 29) == 0x0FFFFFFF
    for pt in (r.G, r.BLINDING, r.ACCUMULATOR, r.PADDING):
        assert r.on_curve(pt) and r.mul(r.N, pt) == r.O and pt != r.O
    assert (2**256 - 1) // r.N == 42


def test_sqrt_tonelli_shanks():
    c = pow(r.NONRESIDUE, r.Q, r.P)
    for k in range(29):                        # the 2-Sylow elements of every order 2^(28 - k)
        v = pow(c, 1 << k, r.P)
        root = r.sqrt(v)
        assert (root is not None) == (k > 0)
        if root is not None:
            assert root * root % r.P == v
    assert r.sqrt(0) == 0 and r.sqrt(r.P - 1) is not None   # -1 is a square: p = 1 mod 4
    assert d.BabyJubJub.curve.mod_sqrt(r.P - 1) ** 2 % r.P == r.P - 1
    with pytest.raises(ValueError):
        d.BabyJubJub.curve.mod_sqrt(r.NONRESIDUE)


def test_sign_rule_is_x_greater_than_minus_x():
    vs = json.load(open(os.path.join(GOLDEN, "ark-vrf", "baby-jubjub_sha-512_tai_tiny.json")))
    P = d.BabyJubJub.point_type
    differ = 0
    for v in vs:
        pt = r.decode(bytes.fromhex(v["pk"]))
        assert r.encode(pt).hex() == v["pk"]
        assert P.string_to_point(bytes.fromhex(v["pk"])).point_to_string().hex() == v["pk"]
        differ += (pt[0] & 1) != (pt[0] > r.P - pt[0])
    assert differ > 0                           # the parity of x would encode some of them differently


@pytest.mark.parametrize("y", [r.P, r.P + 1, r.P + 12345, 2**254 - 1, 2**254, 2**254 + 5, 2**255 - 1])
def test_non_canonical_y_and_bit_254_rejected(y):
    enc = y.to_bytes(32, "little")
    assert r.decode(enc, check=False) is None
    with pytest.raises(ValueError):
        d.BabyJubJub.point_type.string_to_point(enc)


def test_bit_254_set_on_a_valid_point_rejected():
    enc = bytearray(r.encode(r.G))
    enc[31] |= 0x40
    assert r.decode(bytes(enc), check=False) is None
    with pytest.raises(ValueError):
        d.BabyJubJub.point_type.string_to_point(bytes(enc))


@pytest.mark.parametrize("y", [1, r.P - 1])
def test_x_zero_with_sign_bit(y):
    P = d.BabyJubJub.point_type
    for sign in (0, 0x80):
        enc = bytearray(y.to_bytes(32, "little"))
        enc[31] |= sign
        pt = P.string_to_point(bytes(enc))
        assert (pt.x, pt.y) == (0, y) == r.decode(bytes(enc), check=False)
        assert r.decode(bytes(enc)) is None     # neither is a valid prime-order point


def test_torsion_points():
    tp = r.torsion_points()
    assert len(set(tp)) == 8 and all(r.on_curve(t) and r.mul(8, t) == r.O for t in tp)
    P = d.BabyJubJub.point_type
    for t in tp:
        enc = r.encode(t)
        assert r.decode(enc, check=False) == t and r.decode(enc) is None
        pt = P.string_to_point(enc)
        assert (pt.x, pt.y) == t
        q = r.add(r.mul(77, r.G), t)
        assert (r.decode(r.encode(q)) is None) == (t != r.O)


@pytest.mark.parametrize("i,masked,unmasked", [(5, 1, 2), (6, 0, 9), (2901, 18, 18)])
def test_try_and_increment_mask(i, masked, unmasked):
    alpha = i.to_bytes(4, "little")
    pt, ctr = r.encode_to_curve(alpha)
    raw_pt, raw_ctr = r.encode_to_curve(alpha, masked=False)
    assert (ctr, raw_ctr) == (masked, unmasked)
    assert (pt == raw_pt) == (i == 2901)
    assert ctr < 20 and (i != 2901 or ctr >= 12)    # 2901: the third launch of the [0,4), [4,12), [12,20) schedule


def test_public_names_and_parameters():
    assert "BabyJubJub" in d.__all__
    sp = d.BabyJubJub.curve.params
    assert sp.suite_id == b"BabyJubJub-SHA512-TAI-v1" and sp.field_modulus == r.P and sp.subgroup_order == r.N and sp.cofactor == 8
    assert sp.curve_id == _native.CURVE_BABYJUBJUB == 5 and sp.e2c == "tai" and sp.encoding.point_len == 32
    assert sp.a == 1 and sp.d == r.D and not sp.xof
    aux = sp.auxiliary_points
    assert tuple(sp.generator) == r.G and tuple(aux.blinding_base) == r.BLINDING
    assert tuple(aux.accumulator_base) == r.ACCUMULATOR and tuple(aux.padding_point) == r.PADDING
    assert d.BabyJubJub.point_type.generator_point().point_to_string() == r.encode(r.G)


def test_point_type_group_law():
    P = d.BabyJubJub.point_type
    a, b = P(*r.mul(5, r.G)), P(*r.mul(9, r.G))
    assert ((a + b).x, (a + b).y) == r.add(r.mul(5, r.G), r.mul(9, r.G))
    assert (a.double().x, a.double().y) == r.mul(10, r.G)
    assert ((a - b).x, (a - b).y) == r.add(r.mul(5, r.G), r.neg(r.mul(9, r.G)))
    assert (-a).x == -a.x % r.P
    with pytest.raises(ValueError):
        P(r.P, 1)
    with pytest.raises(ValueError):
        P(1, 1)                                  # not on the curve
    for t in r.torsion_points():
        q = P(*t)
        assert ((q + a).x, (q + a).y) == r.add(t, r.mul(5, r.G))


def test_ring_params_refuse_babyjubjub():
    with pytest.raises(ValueError, match="BabyJubJub ring proofs require a primitive 2048-th root of unity"):
        d.RingProofParams(cv=d.BabyJubJub)
