"""P-256 without a GPU: the big-integer restatement (p256_ref.py) against the suite's 9 vector files field by field, the library's
SHA-256 against hashlib, the codec's rules (flag bits, infinity, x >= p, no root, canonical strings that start with 0x02 / 0x03) and
the reference's SEC1 fallback through the Python point type, and the public names."""
import glob
import hashlib
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import p256_ref as r  # noqa: E402

import dot_ring_amd as d  # noqa: E402
from dot_ring_amd import _native  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILES = sorted(glob.glob(os.path.join(GOLDEN, "*", "secp256r1_sha*_tai_*.json")))
FIELDS = {"pedersen": ("gamma", "proof_pk_com", "proof_r", "proof_ok", "proof_s", "proof_sb"), "thin": ("gamma", "proof_r", "proof_s"),
          "tiny": ("gamma", "proof_c", "proof_s"), "ietf": ("gamma", "proof_c", "proof_s")}
# alpha = LE32(i) whose hash-to-curve candidate decodes only through the SEC1 fallback, with the counter it stops at
FALLBACK_ALPHAS = [(240, 0), (967, 0), (1184, 0), (987, 3)]


def _kind(path):
    return next(k for k in FIELDS if k in os.path.basename(path))


def _pt(enc):
    return d.P256.point_type.string_to_point(enc)


def test_nine_vector_files():
    assert len(FILES) == 9


@pytest.mark.parametrize("path", FILES, ids=lambda p: "/".join(p.split(os.sep)[-2:]))
def test_restatement_reproduces_vectors(path):
    kind = _kind(path)
    for v in json.load(open(path)):
        hx = lambda k: bytes.fromhex(v[k])  # noqa: E731
        sk, al, ad = hx("sk"), hx("alpha"), hx("ad")
        x = r.le(sk) % r.N
        assert r.encode(r.mul(x, r.G)) == hx("pk")
        h, _, _ = r.encode_to_curve(al)
        assert r.encode(h) == hx("h")
        gamma = r.mul(x, h)
        assert r.encode(gamma) == hx("gamma")
        assert r.point_to_hash(gamma).hex() == v["beta"][:64]
        if kind == "pedersen":
            proof, b = r.pedersen_prove(sk, al, ad)
            assert b == r.le(hx("blinding"))
            assert len(proof) == 196
        else:
            proof = r.ietf_prove(sk, al, ad, thin=kind == "thin")
            assert len(proof) == (98 if kind == "thin" else 81)
        assert proof == b"".join(hx(f) for f in FIELDS[kind])


@pytest.mark.parametrize("length", [0, 1, 55, 56, 63, 64, 65, 119, 120, 128, 1000, 5000])
def test_host_sha256(length):
    data = bytes((7 * i + length) & 0xFF for i in range(length))
    assert _native.host_hash(4, data, 32) == hashlib.sha256(data).digest()


def test_flag_bits_rejected():
    enc = r.encode(r.mul(5, r.G))
    for bit in range(6):
        bad = enc[:32] + bytes([enc[32] | (1 << bit)])
        assert r.decode(bad, check=False) == "bad"
        with pytest.raises(ValueError):
            _pt(bad)


def test_infinity_encodings():
    P = d.P256.point_type
    assert P.identity().point_to_string() == bytes(32) + b"\x40"
    assert _pt(bytes(32) + b"\x40").is_identity() and r.decode(bytes(32) + b"\x40", check=False) is None
    assert r.decode(bytes(32) + b"\x40") == "bad"                 # dec_point refuses the identity
    for bad in (bytes(32) + b"\xc0", b"\x01" + bytes(31) + b"\x40", bytes(31) + b"\x05" + b"\x40"):
        assert r.decode(bad, check=False) == "bad"
        with pytest.raises(ValueError):
            _pt(bad)


@pytest.mark.parametrize("k", [0, 1, 5, 2**200, 2**256 - r.P - 1])
def test_x_not_below_p_rejected(k):
    enc = (r.P + k).to_bytes(32, "little") + b"\x00"
    assert r.decode(enc, check=False) == "bad"
    with pytest.raises(ValueError):
        _pt(enc)


def test_non_residue_rejected():
    xs = [x for x in range(4, 80) if r.sqrt(r.rhs(x)) is None]        # (x = 2, 3 would start with a SEC1 marker byte)
    assert len(xs) > 10
    for x in xs:
        for flag in (0, 0x80):
            enc = x.to_bytes(32, "little") + bytes([flag])
            assert r.decode(enc, check=False) == "bad"
            with pytest.raises(ValueError):
                _pt(enc)


def test_flag_is_larger_root_not_parity():
    P = d.P256.point_type
    differ = 0
    for k in range(1, 40):
        pt = r.mul(k, r.G)
        enc = r.encode(pt)
        assert P(*pt).point_to_string() == enc
        q = _pt(enc)
        assert (q.x, q.y) == pt
        differ += (pt[1] & 1) != (enc[32] >> 7)
    assert 0 < differ < 39


def test_canonical_strings_starting_with_sec1_markers():
    # canonical encodings whose first byte is 0x02 / 0x03 decode canonically (the fallback is only reached on failure)
    P = d.P256.point_type
    seen = 0
    for k in range(1, 6000):
        pt = r.mul(k, r.G) if k < 3 else None
        x = k * 0x1000193 % r.P
        x = (x & ~0xFF) | (2 + k % 2)
        ys = r.sqrt(r.rhs(x))
        if ys is None:
            continue
        pt = (x, max(ys, r.P - ys) if k % 3 else min(ys, r.P - ys))
        enc = r.encode(pt)
        assert enc[0] in (2, 3)
        assert r.decode(enc, check=False) == pt and not r.decoded_by_fallback(enc)
        q = _pt(enc)
        assert (q.x, q.y) == pt
        seen += 1
        if seen == 20:
            break
    assert seen == 20


def test_sec1_fallback_strings():
    P = d.P256.point_type
    found = 0
    for k in range(1, 400):
        pt = r.mul(k, r.G)
        enc = bytes([2 + (pt[1] & 1)]) + pt[0].to_bytes(32, "big")
        if not r.decoded_by_fallback(enc):
            continue                                              # (some of them read canonically as another point)
        assert r.decode(enc) == pt
        q = P.string_to_point(enc)
        assert (q.x, q.y) == pt
        found += 1
    assert found > 100
    # a fallback string whose big-endian x is not below p fails both ways
    bad = b"\x02" + b"\xff" * 32
    assert r.decode(bad, check=False) == "bad"
    with pytest.raises(ValueError):
        P.string_to_point(bad)


@pytest.mark.parametrize("i,counter", FALLBACK_ALPHAS)
def test_fallback_alphas(i, counter):
    alpha = i.to_bytes(4, "little")
    pt, ctr, by_fallback = r.encode_to_curve(alpha)
    assert (ctr, by_fallback) == (counter, True)
    cand = r.tai_candidate(alpha, ctr)
    assert cand[0] in (2, 3) and cand[32] == 0x80
    q = d.P256.point_type.string_to_point(cand)
    assert (q.x, q.y) == pt
    # the first fallback alpha below 1000 at counter 0
    assert min(j for j, c in FALLBACK_ALPHAS if c == 0) == 240


def test_public_names_and_parameters():
    assert d.P256 is d.P256_TAI
    assert "P256" in d.__all__ and "P256_TAI" in d.__all__
    sp = d.P256.curve.params
    assert sp.suite_id == b"Secp256r1-SHA256-TAI-v1" and sp.field_modulus == r.P and sp.subgroup_order == r.N and sp.cofactor == 1
    assert sp.curve_id == _native.CURVE_P256 == 4 and sp.e2c == "tai" and sp.encoding.point_len == 33 and sp.hash_fn is hashlib.sha256
    assert tuple(sp.generator) == r.G and tuple(sp.auxiliary_points.blinding_base) == r.BLINDING
    assert r.on_curve(r.G) and r.on_curve(r.BLINDING) and r.mul(r.N, r.G) is None
    assert _native.xof_kind(sp.hash_fn) == 2 and _native.xof_kind(hashlib.sha512) == 0 and _native.xof_kind(hashlib.shake_128) == 1
    assert _native.vrf_suite(sp.suite_id, sp.hash_fn, bytes(64), bytes(64), 4).xof == 2
    assert _native.vrf_suite(b"x", True, bytes(64), bytes(64)).xof == 1 and _native.vrf_suite(b"x", False, bytes(64), bytes(64)).xof == 0


def test_point_type_group_law():
    P = d.P256.point_type
    a, b = P(*r.mul(5, r.G)), P(*r.mul(9, r.G))
    assert ((a + b).x, (a + b).y) == r.mul(14, r.G)
    assert (a.double().x, a.double().y) == r.mul(10, r.G)
    assert (a + (-a)).is_identity() and (a - a).is_identity() and (a + P.identity()) == a
    with pytest.raises(ValueError):
        P(r.P, 1)
    with pytest.raises(ValueError):
        P(1, 1)
    assert d.P256.curve.valid_point(a) and not d.P256.curve.valid_point(P.identity())
    assert d.P256.curve.mod_sqrt(4) in (2, r.P - 2)


def test_ring_params_refuse_p256():
    with pytest.raises(ValueError, match="ring proofs require a Twisted Edwards curve"):
        d.RingProofParams(cv=d.P256)
