"""The RFC 9380 variants of P-256 and Ed25519 (P256_RO / P256_NU / Ed25519_RO / Ed25519_NU) without a GPU: the big-integer restatement
(h2c_ref.py) against the hash-to-curve vectors and the public keys the reference holds; its generic VRF layer against the reference's
P-256 and Ed25519 try-and-increment proof files byte for byte — which is what entitles it to judge the proofs of the new variants, for
which the reference holds none; the library's hash_to_field for curves 8 - 11 (a host routine: no context); names, codec and the ABI
header."""
import glob
import hashlib
import json
import os
import random
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ed25519_ref as ed  # noqa: E402
import h2c_ref as h  # noqa: E402
import p256_ref as p256  # noqa: E402

import dot_ring_amd as d  # noqa: E402
from dot_ring_amd import _native  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
TAI_FILES = sorted(glob.glob(os.path.join(GOLDEN, "*", "secp256r1_sha*_tai_*.json")) + glob.glob(os.path.join(GOLDEN, "*", "ed25519_sha*_tai_*.json")))
FIELDS = {"pedersen": ("gamma", "proof_pk_com", "proof_r", "proof_ok", "proof_s", "proof_sb"), "thin": ("gamma", "proof_r", "proof_s"),
          "tiny": ("gamma", "proof_c", "proof_s"), "ietf": ("gamma", "proof_c", "proof_s")}
# name of the vector file -> (hash_to_field, one image, encode_to_curve, DST, elements per message)
MAPS = {
    "p256_ro": (h.p256_hash_to_field, h.p256_map_to_curve, h.p256_encode_to_curve_ro, h.P256_DST_RO, 2),
    "p256_nu": (h.p256_hash_to_field, h.p256_map_to_curve, h.p256_encode_to_curve_nu, h.P256_DST_NU, 1),
    "ed25519_ro": (h.ed_hash_to_field, h.ed_map_to_curve, h.ed_encode_to_curve_ro, h.ED_DST_RO, 2),
    "ed25519_nu": (h.ed_hash_to_field, h.ed_map_to_curve, h.ed_encode_to_curve_nu, h.ED_DST_NU, 1),
}
VARIANTS = {"p256_ro": "P256_RO", "p256_nu": "P256_NU", "ed25519_ro": "Ed25519_RO", "ed25519_nu": "Ed25519_NU"}


def h2c_file(name):
    return json.load(open(os.path.join(GOLDEN, "h2c", f"{name}.json")))


def base_vectors(curve):
    return json.load(open(os.path.join(GOLDEN, "base", f"{curve}_base_vectors.json")))


def _xy(v):
    return int(v["x"], 16), int(v["y"], 16)


# ---------------------------------------------------------------- 1. the restatement against what the reference holds
@pytest.mark.parametrize("name", sorted(MAPS))
def test_restatement_reproduces_hash_to_curve_vectors(name):
    hash_to_field, image, encode_to_curve, dst, count = MAPS[name]
    doc = h2c_file(name)
    assert doc["dst"].encode() == dst and len(doc["vectors"]) == 5
    for v in doc["vectors"]:
        msg = v["msg"].encode()
        us = hash_to_field(msg, count, dst)
        assert us == [int(u, 16) for u in v["u"]]
        if count == 2:
            assert image(us[0]) == _xy(v["Q0"]) and image(us[1]) == _xy(v["Q1"])
        else:
            assert image(us[0]) == _xy(v["Q"])
        assert encode_to_curve(msg) == _xy(v["P"])


def test_restatement_reproduces_public_keys():
    recs = base_vectors("p256")
    assert len(recs) == 5
    for v in recs:
        pk = p256.mul(p256.le(bytes.fromhex(v["sk"])) % p256.N, p256.G)
        assert h.p256_sec1_encode(pk).hex() == v["pk"] and h.p256_sec1_decode(bytes.fromhex(v["pk"])) == pk
    # Ed25519's file holds secret keys, inputs and additional data; its pk fields are empty (asserted, so that a refreshed file is noticed)
    recs = base_vectors("ed25519")
    assert len(recs) == 5 and all(v["pk"] == "" for v in recs)
    for v in recs:
        pk = ed.mul(ed.le(bytes.fromhex(v["sk"])) % ed.N, ed.G)
        assert ed.decode(ed.encode(pk)) == pk


def test_restatement_constants():
    p, q = p256.P, ed.P
    # Z = -10 is not a square mod p256 and -Z is (the map's sqrt(-Z) exists); Z = 2 is not a square mod 2^255 - 19
    assert pow(h.P256_Z % p, (p - 1) // 2, p) == p - 1 and pow(-h.P256_Z, (p - 1) // 2, p) == 1
    assert pow(h.ELL2_Z, (q - 1) // 2, q) == q - 1
    k = h.SQRT_NEG_A_MINUS_2
    assert k * k % q == -(h.MONT_A + 2) % q
    for u in (1, 2, 5, q - 1, p - 1):
        assert p256.on_curve(h.p256_map_to_curve(u % p))
        pt = h.ed_map_to_curve(u % q)
        assert ed.on_curve(pt) and ed.mul(ed.N, h.ed_clear_cofactor(pt)) == ed.O
    with pytest.raises(ValueError):          # the image of 0 on curve25519 is (0, 0)-like: v = 0, the reference's inverse fails
        h.ed_map_to_curve(0)


# ---------------------------------------------------------------- 2. the generic VRF layer against the reference's proof files
@pytest.mark.parametrize("path", TAI_FILES, ids=lambda p: "/".join(p.split(os.sep)[-2:]))
def test_generic_vrf_layer_reproduces_tai_vectors(path):
    kind = next(k for k in FIELDS if k in os.path.basename(path))
    is_ed = os.path.basename(path).startswith("ed25519")
    suite = h.ED25519_TAI if is_ed else h.P256_TAI
    pl = 32 if is_ed else 33
    recs = json.load(open(path))
    assert recs
    for v in recs:
        hx = lambda k: bytes.fromhex(v[k])  # noqa: E731
        sk, al, ad = hx("sk"), hx("alpha"), hx("ad")
        if kind == "pedersen":
            proof, b = suite.pedersen_prove(sk, al, ad)
            assert b == int.from_bytes(hx("blinding"), "little") and len(proof) == 4 * pl + 64
        else:
            proof = suite.ietf_prove(sk, al, ad, thin=kind == "thin")
            assert len(proof) == (2 * pl + 32 if kind == "thin" else pl + 48)
        assert proof == b"".join(hx(f) for f in FIELDS[kind])


def test_tai_vector_files_present():
    assert len([p for p in TAI_FILES if "secp256r1" in p]) == 9 and len([p for p in TAI_FILES if "ed25519" in p]) == 8


# ---------------------------------------------------------------- 3. the library's hash_to_field (host only)
def _variant(name):
    return getattr(d, VARIANTS[name])


@pytest.mark.parametrize("name", sorted(MAPS))
def test_hash_to_field_batch_vectors(name):
    vs = h2c_file(name)["vectors"]
    count = MAPS[name][4]
    got = _native.hash_to_field_batch(_variant(name).point_type._suite_struct(), [v["msg"].encode() for v in vs])
    assert len(got) == 32 * count * len(vs)
    assert got == b"".join(int(u, 16).to_bytes(32, "little") for v in vs for u in v["u"])


@pytest.mark.parametrize("name", sorted(MAPS))
def test_hash_to_field_batch_random_messages(name):
    rng = random.Random(0x9380)
    msgs = [rng.randbytes(rng.randrange(0, 301)) for _ in range(198)] + [b"", rng.randbytes(300)]
    salts = [rng.randbytes(rng.randrange(0, 40)) for _ in msgs]
    salts[-2] = b""                                   # the empty message, unsalted: nothing at all to absorb
    data = [s + m for s, m in zip(salts, msgs)]
    hash_to_field, _, _, dst, count = MAPS[name]
    cv = _variant(name)
    got = _native.hash_to_field_batch(cv.point_type._suite_struct(), data)
    want = b"".join(u.to_bytes(32, "little") for m in data for u in hash_to_field(m, count, dst))
    assert got == want
    assert cv.point_type.hash_to_field_pairs(msgs, salts) == want


# ---------------------------------------------------------------- 4. names, parameters, codec, refusals (no GPU)
def test_public_names():
    assert {"P256_RO", "P256_NU", "Ed25519_RO", "Ed25519_NU"} <= set(d.__all__)
    assert d.P256 is d.P256_TAI and d.Ed25519 is d.Ed25519_TAI
    assert len({id(v) for v in (d.P256_TAI, d.P256_RO, d.P256_NU, d.Ed25519_TAI, d.Ed25519_RO, d.Ed25519_NU)}) == 6
    for cv, cid, e2c in ((d.P256_RO, 8, "sswu"), (d.P256_NU, 9, "sswu_nu")):
        sp = cv.curve.params
        assert sp.suite_id == p256.SUITE_ID and sp.field_modulus == p256.P and sp.subgroup_order == p256.N and sp.cofactor == 1
        assert sp.curve_id == cid and sp.e2c == e2c and sp.encoding.point_len == 33 and sp.hash_fn is hashlib.sha256
        assert sp.generator == p256.G and sp.auxiliary_points.blinding_base == p256.BLINDING
        assert cv.point_type._CV == cid and cv.point_type.curve is cv.curve and cv.name == ("P256_RO" if cid == 8 else "P256_NU")
    for cv, cid, e2c in ((d.Ed25519_RO, 10, "ell2"), (d.Ed25519_NU, 11, "ell2_nu")):
        sp = cv.curve.params
        assert sp.suite_id == ed.SUITE_ID and sp.field_modulus == ed.P and sp.subgroup_order == ed.N and sp.cofactor == 8
        assert sp.curve_id == cid and sp.e2c == e2c and sp.encoding.point_len == 32 and sp.hash_fn is hashlib.sha512
        assert sp.generator == ed.G and sp.auxiliary_points.blinding_base == ed.BLINDING
        assert cv.point_type._CV == cid and cv.point_type.curve is cv.curve
    assert d.P256_TAI.curve.params.curve_id == 4 and d.Ed25519_TAI.curve.params.curve_id == 3
    assert (_native.CURVE_P256_RO, _native.CURVE_P256_NU, _native.CURVE_ED25519_RO, _native.CURVE_ED25519_NU) == (8, 9, 10, 11)
    assert [_native.curve_point_len(c) for c in (8, 9, 10, 11)] == [33, 33, 32, 32]


def test_abi_header_declares_the_new_calls():
    text = open(os.path.join(HERE, "..", "include", "dotring_hip.h")).read()
    for name, value in (("DR_CURVE_P256_RO", 8), ("DR_CURVE_P256_NU", 9), ("DR_CURVE_ED25519_RO", 10), ("DR_CURVE_ED25519_NU", 11)):
        assert re.search(rf"\b{name} = {value}\b", text)
    for call in ("dr_p256_map_to_curve", "dr_ed25519_map_to_curve"):
        assert re.search(rf"DR_API int {call}\(dr_ctx \*ctx, const uint8_t \*us", text)
        assert call in _native.EXPORTED_SYMBOLS and hasattr(_native.lib(), call)


def test_p256_sec1_codec_python():
    ro, tai = d.P256_RO.point_type, d.P256_TAI.point_type
    for k in (1, 2, 3, 7, p256.N - 1):
        pt = p256.mul(k, p256.G)
        enc = h.p256_sec1_encode(pt)
        q = ro.string_to_point(enc)
        assert (q.x, q.y) == pt and q.point_to_string() == enc and ro.string_to_point(enc.hex()) == q
        assert ro.string_to_point(q.point_to_string(compressed=False)) == q
        # the try-and-increment variant keeps its own form, and neither reads the other's as its own
        t = tai(*pt).point_to_string()
        assert t == p256.encode(pt) and t != enc
        if t[0] not in (2, 3):
            with pytest.raises(ValueError):
                ro.string_to_point(t)
        else:
            assert h.p256_sec1_decode(t) == "bad" or ro.string_to_point(t) != q
    assert ro.identity().point_to_string() == b"\x00" and ro.string_to_point(b"\x00").is_identity()
    x = 1
    while p256.sqrt(p256.rhs(x)) is not None:
        x += 1
    g = p256.G
    for bad in (b"", b"\x00\x00", b"\x02" + p256.P.to_bytes(32, "big"), b"\x03" + x.to_bytes(32, "big"), b"\x02" + bytes(31),
                b"\x05" + g[0].to_bytes(32, "big"), b"\x04" + g[0].to_bytes(32, "big"),
                b"\x04" + g[0].to_bytes(32, "big") + (g[1] + 1).to_bytes(32, "big"), bytes(32) + b"\x40"):
        with pytest.raises(ValueError):
            ro.string_to_point(bad)


def test_ed25519_variants_keep_the_codec_and_map_on_the_host():
    for cv in (d.Ed25519_RO, d.Ed25519_NU):
        pt_cls = cv.point_type
        for k in (1, 2, 9):
            pt = ed.mul(k, ed.G)
            q = pt_cls.string_to_point(ed.encode(pt))
            assert (q.x, q.y) == pt and q.point_to_string() == ed.encode(pt)
        for v in h2c_file("ed25519_nu")["vectors"]:
            q = pt_cls.map_to_curve(int(v["u"][0], 16))
            assert (q.x, q.y) == _xy(v["Q"])
        with pytest.raises(ValueError):
            pt_cls.map_to_curve(0)


def test_ring_params_refuse_the_variants():
    for cv in (d.P256_RO, d.P256_NU, d.Ed25519_RO, d.Ed25519_NU):
        with pytest.raises(ValueError):
            d.RingProofParams(cv=cv)


def test_load_suite_wants_the_suites_hash():
    le = lambda pt: pt[0].to_bytes(32, "little") + pt[1].to_bytes(32, "little")  # noqa: E731
    for cv, wrong in ((d.P256_RO, hashlib.sha512), (d.P256_NU, hashlib.sha512), (d.Ed25519_RO, hashlib.sha256), (d.Ed25519_NU, hashlib.shake_128)):
        sp = cv.curve.params
        bad = _native.vrf_suite(sp.suite_id, wrong, le(sp.generator), le(sp.auxiliary_points.blinding_base), sp.curve_id)
        with pytest.raises(Exception):
            _native.hash_to_field_batch(bad, [b"abc"])
