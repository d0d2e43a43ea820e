"""secp256k1 without a GPU: the big-integer restatement (secp256k1_ref.py) against the hash-to-curve vectors and the public keys the
reference holds; its curve-generic VRF layer, given P-256's constants, codec and try-and-increment (p256_ref.py), against the reference's
P-256 vector files byte for byte — which is what entitles it to judge secp256k1 proofs, for which the reference holds none; the library's
hash_to_field for curves 6 and 7 (a host routine: no context) against the vectors and the restatement; the codec and the public names."""
import glob
import hashlib
import json
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import p256_ref  # noqa: E402
import secp256k1_ref as r  # noqa: E402

import dot_ring_amd as d  # noqa: E402
from dot_ring_amd import _native  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
P256_FILES = sorted(glob.glob(os.path.join(GOLDEN, "*", "secp256r1_sha*_tai_*.json")))
FIELDS = {"pedersen": ("gamma", "proof_pk_com", "proof_r", "proof_ok", "proof_s", "proof_sb"), "thin": ("gamma", "proof_r", "proof_s"),
          "tiny": ("gamma", "proof_c", "proof_s"), "ietf": ("gamma", "proof_c", "proof_s")}


def h2c_vectors(variant):
    return json.load(open(os.path.join(GOLDEN, "h2c", f"secp256k1_{variant}.json")))["vectors"]


def base_vectors():
    return json.load(open(os.path.join(GOLDEN, "base", "secp256k1_base_vectors.json")))


def _xy(v):
    return int(v["x"], 16), int(v["y"], 16)


# ---------------------------------------------------------------- 1. the restatement against what the reference holds
def test_restatement_reproduces_hash_to_curve_vectors():
    ro, nu = h2c_vectors("ro"), h2c_vectors("nu")
    assert len(ro) == 5 and len(nu) == 5
    for v in ro:
        msg = v["msg"].encode()
        us = r.hash_to_field(msg, 2, r.DST_RO)
        assert us == [int(u, 16) for u in v["u"]]
        assert r.map_to_curve(us[0]) == _xy(v["Q0"]) and r.map_to_curve(us[1]) == _xy(v["Q1"])
        assert r.encode_to_curve_ro(msg) == _xy(v["P"])
    for v in nu:
        msg = v["msg"].encode()
        us = r.hash_to_field(msg, 1, r.DST_NU)
        assert us == [int(u, 16) for u in v["u"]]
        assert r.map_to_curve(us[0]) == _xy(v["Q"])
        assert r.encode_to_curve_nu(msg) == _xy(v["P"])


def test_restatement_reproduces_public_keys():
    recs = base_vectors()
    assert len(recs) == 5
    for v in recs:
        pk = r.mul(r.le(bytes.fromhex(v["sk"])) % r.N, r.G)
        assert r.encode(pk).hex() == v["pk"] and r.decode(bytes.fromhex(v["pk"])) == pk


def test_restatement_constants():
    assert r.on_curve(r.G) and r.on_curve(r.BLINDING) and r.mul(r.N, r.G) is None
    assert pow(-r.Z % r.P, (r.P - 1) // 2, r.P) == 1 and pow(r.Z % r.P, (r.P - 1) // 2, r.P) == r.P - 1
    # the images of E' land on secp256k1, and the map is a homomorphism (checked on E' = y^2 = x^3 + A' x + B')
    a, _ = r.sswu(5)
    b, _ = r.sswu(6)
    assert (a[1] ** 2 - (a[0] ** 3 + r.ISO_A * a[0] + r.ISO_B)) % r.P == 0
    assert r.on_curve(r.iso_map(a))
    assert r.iso_map(r.sw_add(a, b, r.ISO_A, r.P)) == r.add(r.iso_map(a), r.iso_map(b))


# ---------------------------------------------------------------- 2. the generic VRF layer against the P-256 vectors
def _p256_suite():
    return r.Suite(p256_ref.SUITE_ID, p256_ref.N, p256_ref.G, p256_ref.BLINDING, p256_ref.add, p256_ref.encode,
                   lambda data: p256_ref.encode_to_curve(data)[0])


@pytest.mark.parametrize("path", P256_FILES, ids=lambda p: "/".join(p.split(os.sep)[-2:]))
def test_generic_vrf_layer_reproduces_p256_vectors(path):
    kind = next(k for k in FIELDS if k in os.path.basename(path))
    suite = _p256_suite()
    for v in json.load(open(path)):
        hx = lambda k: bytes.fromhex(v[k])  # noqa: E731
        sk, al, ad = hx("sk"), hx("alpha"), hx("ad")
        gamma = suite.mul(r.le(sk), suite.e2c(al))
        assert suite.point_to_hash(gamma).hex() == v["beta"][:64]
        if kind == "pedersen":
            proof, b = suite.pedersen_prove(sk, al, ad)
            assert b == r.le(hx("blinding")) and len(proof) == 196
        else:
            proof = suite.ietf_prove(sk, al, ad, thin=kind == "thin")
            assert len(proof) == (98 if kind == "thin" else 81)
        assert proof == b"".join(hx(f) for f in FIELDS[kind])


def test_p256_vector_files_present():
    assert len(P256_FILES) == 9


# ---------------------------------------------------------------- 3. the library's hash_to_field (host only)
def _suite_struct(cv):
    return cv.point_type._suite_struct()


def test_hash_to_field_batch_vectors():
    for variant, cv, count in (("ro", d.Secp256k1_RO, 2), ("nu", d.Secp256k1_NU, 1)):
        vs = h2c_vectors(variant)
        got = _native.hash_to_field_batch(_suite_struct(cv), [v["msg"].encode() for v in vs])
        assert len(got) == 32 * count * len(vs)
        want = b"".join(int(u, 16).to_bytes(32, "little") for v in vs for u in v["u"])
        assert got == want


def test_hash_to_field_batch_random_messages():
    rng = random.Random(0x5ec9)
    msgs = [rng.randbytes(rng.randrange(0, 301)) for _ in range(198)] + [b"", rng.randbytes(300)]
    salts = [rng.randbytes(rng.randrange(0, 40)) for _ in msgs]
    data = [s + m for s, m in zip(salts, msgs)]
    assert {0, 300} <= {len(m) for m in msgs}
    for cv, count, dst in ((d.Secp256k1_RO, 2, r.DST_RO), (d.Secp256k1_NU, 1, r.DST_NU)):
        got = _native.hash_to_field_batch(_suite_struct(cv), data)
        want = b"".join(u.to_bytes(32, "little") for m in data for u in r.hash_to_field(m, count, dst))
        assert got == want
        assert cv.point_type.hash_to_field_pairs(msgs, salts) == want


# ---------------------------------------------------------------- codec, names, refusals (no GPU)
def test_public_names():
    assert d.Secp256k1 is d.Secp256k1_RO and d.Secp256k1_NU is not d.Secp256k1_RO
    assert {"Secp256k1", "Secp256k1_RO", "Secp256k1_NU"} <= set(d.__all__)
    for cv, cid, e2c in ((d.Secp256k1_RO, 6, "sswu"), (d.Secp256k1_NU, 7, "sswu_nu")):
        sp = cv.curve.params
        assert sp.suite_id == r.SUITE_ID and sp.field_modulus == r.P and sp.subgroup_order == r.N and sp.cofactor == 1
        assert sp.curve_id == cid and sp.e2c == e2c and sp.encoding.point_len == 33 and sp.hash_fn is hashlib.sha256
        assert sp.generator == r.G and sp.auxiliary_points.blinding_base == r.BLINDING
        assert sp.auxiliary_points.accumulator_base is None and sp.auxiliary_points.padding_point is None
        assert cv.point_type._CV == cid and cv.point_type.curve is cv.curve
    assert _native.CURVE_SECP256K1 == 6 and _native.CURVE_SECP256K1_NU == 7
    assert _native.curve_point_len(6) == _native.curve_point_len(7) == _native.curve_point_len(4) == 33 and _native.curve_point_len(3) == 32


def test_codec_python():
    pt_cls = d.Secp256k1.point_type
    for k in (1, 2, 3, 7, r.N - 1):
        pt = r.mul(k, r.G)
        enc = r.encode(pt)
        q = pt_cls.string_to_point(enc)
        assert (q.x, q.y) == pt and q.point_to_string() == enc and pt_cls.string_to_point(enc.hex()) == q
        assert pt_cls.string_to_point(q.point_to_string(compressed=False)) == q
    assert pt_cls.identity().point_to_string() == b"\x00" and pt_cls.string_to_point(b"\x00").is_identity()
    x = 1
    while r.sqrt(r.rhs(x)) is not None:
        x += 1
    for bad in (b"", b"\x00\x00", b"\x02" + r.P.to_bytes(32, "big"), b"\x03" + x.to_bytes(32, "big"), b"\x02" + bytes(31),
                b"\x05" + r.G[0].to_bytes(32, "big"), b"\x04" + r.G[0].to_bytes(32, "big"),
                b"\x04" + r.G[0].to_bytes(32, "big") + (r.G[1] + 1).to_bytes(32, "big")):
        assert r.decode(bad) == "bad" or bad[:1] == b"\x00"
        with pytest.raises(ValueError):
            pt_cls.string_to_point(bad)


def test_host_group_law_python():
    pt_cls = d.Secp256k1.point_type
    g = pt_cls.generator_point()
    a, b = g + g, g.double().double()
    assert (a.x, a.y) == r.mul(2, r.G) and (b.x, b.y) == r.mul(4, r.G) and ((a + b).x, (a + b).y) == r.mul(6, r.G)
    assert (g - g).is_identity() and (g + pt_cls.identity()) == g and (-g).y == r.P - r.G[1]
    assert d.Secp256k1.curve.valid_point(a) and not d.Secp256k1.curve.valid_point(pt_cls.identity())
    assert d.Secp256k1.point(r.G) == g and d.Secp256k1.point(g) is g
    with pytest.raises(ValueError):
        pt_cls(1, 1)


def test_ring_params_refuse_secp256k1():
    for cv in (d.Secp256k1, d.Secp256k1_NU):
        with pytest.raises(ValueError):
            d.RingProofParams(cv=cv)


def test_load_suite_wants_sha256():
    sp = d.Secp256k1.curve.params
    le = lambda pt: pt[0].to_bytes(32, "little") + pt[1].to_bytes(32, "little")  # noqa: E731
    bad = _native.vrf_suite(sp.suite_id, hashlib.sha512, le(sp.generator), le(sp.auxiliary_points.blinding_base), sp.curve_id)
    with pytest.raises(Exception):
        _native.hash_to_field_batch(bad, [b"abc"])
