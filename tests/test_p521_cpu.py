"""P521_RO / P521_NU without a GPU: the big-integer restatement (p521_ref.py) against the strings of the reference's two RFC 9380 vector
files and the five public keys of its base file, the facts the kernels rely on (the order, the map's exceptional inputs, the points
that do and do not exist), the host build of fp521.hip.h, p521_law.hip.h and sswu.hip.h's map under -fsanitize=undefined against
integers (every field operation at the extreme limb images of its contract, every pair of a set of points with the exceptional ones in
it, the map, the scalar recoding), the library's host hash_to_field, the Python point type on the host, names, ids and exports, and the
pin of the restatement's VRF layer on the reference's P-256 proof files.

The tests of the checker alone pass without the feature: test_restatement_reproduces_the_vector_files,
test_restatement_reproduces_the_public_keys, test_facts_the_kernels_rely_on, test_width_suite_reproduces_the_p256_files and
test_restatement_vrf_layer_is_self_consistent.  The others need dot_ring_amd.P521*, dr_p521_* or csrc/fp521.hip.h."""
import glob
import json
import os
import random
import re
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import p256_ref as p256  # noqa: E402
import p521_ref as r  # noqa: E402

import dot_ring_amd as d  # noqa: E402
from dot_ring_amd import _native  # noqa: E402
from dot_ring_amd.vrf.codec import point_len, scalar_len  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dot_ring_amd", "csrc")
P, N = r.P, r.N
HEX132 = re.compile(r"^[0-9a-f]{132}$")
# the two records of the two files that are no points of the curve (the restatement's images of the same u are): p521_ro.json, vector
# 1's Q1, whose x string lacks one hexadecimal digit, and vector 3's Q0, whose y string does
NOT_A_POINT = {("p521_ro.json", 1, "Q1"), ("p521_ro.json", 3, "Q0")}
X0 = (0, r.sqrt(r.B))


def _vectors(golden_dir, name):
    with open(os.path.join(golden_dir, "h2c", name)) as f:
        return json.load(f)


def _base(golden_dir):
    with open(os.path.join(golden_dir, "base", "p521_base_vectors.json")) as f:
        return json.load(f)


# ---------------------------------------------------------------- the restatement against the reference's data
def test_restatement_reproduces_the_vector_files(golden_dir):
    matched_u = matched_p = 0
    shown = set()
    for name, nu in (("p521_ro.json", False), ("p521_nu.json", True)):
        doc = _vectors(golden_dir, name)
        dst = doc["dst"].encode()
        assert dst == (r.DST_NU if nu else r.DST_RO) and len(dst) == 44 and doc["suite"].encode() == dst[len(b"QUUX-V01-CS02-with-"):]
        assert len(doc["vectors"]) == 5
        for index, v in enumerate(doc["vectors"]):
            us = r.hash_to_field(v["msg"].encode(), 1 if nu else 2, dst)
            assert [int(u, 16) for u in v["u"]] == us and all(HEX132.match(u) for u in v["u"])       # every u, no exception
            matched_u += 1
            images = [r.map_to_curve(u) for u in us]
            for key, image in zip(("Q",) if nu else ("Q0", "Q1"), images):
                recorded = (int(v[key]["x"], 16), int(v[key]["y"], 16))
                if (name, index, key) in NOT_A_POINT:
                    # shown, not skipped: the record is on no curve point, one of its strings is a digit short, the image is a point
                    assert not r.on_curve(recorded) and r.on_curve(image)
                    assert sorted((len(v[key]["x"]), len(v[key]["y"]))) == [131, 132]
                    shown.add((name, index, key))
                else:
                    assert recorded == image                                # (as integers: one string carries a leading blank)
            total = None
            for image in images:
                total = r.add(total, image)
            assert total == (int(v["P"]["x"], 16), int(v["P"]["y"], 16))                              # every P, no exception
            matched_p += 1
    assert matched_u == 10 and matched_p == 10 and shown == NOT_A_POINT


def test_restatement_reproduces_the_public_keys(golden_dir):
    recs = _base(golden_dir)
    assert len(recs) == 5 and {len(v["sk"]) // 2 for v in recs} == {74, 60}
    for v in recs:
        assert r.public_key(bytes.fromhex(v["sk"])).hex() == v["pk"] and len(v["pk"]) == 134
        assert v["h"] == v["gamma"] == v["proof_c"] == v["proof_s"] == ""       # the reference holds no P-521 proof bytes


def test_facts_the_kernels_rely_on():
    assert P == 2**521 - 1 and P % 4 == 3 and N.bit_length() == 521 and N < P
    assert r.on_curve(r.G) and r.mul(N, r.G) is None and r.mul(N - 1, r.G) == r.neg(r.G) and r.BLINDING == r.G
    assert 2 * r.HALF % P == 1 and 2**532 % P == 2**11
    # the map's exceptional branch: Z u^2 = -1 iff u = +-1/2; all three inputs land on x1 = B / (Z A), a point
    x1 = r.B * pow(r.Z * r.A % P, -1, P) % P
    for u in (0, r.HALF, r.HALF - 1):
        assert (r.Z * r.Z * pow(u, 4, P) + r.Z * u * u) % P == 0
        assert r.map_to_curve(u)[0] == x1 and r.on_curve(r.map_to_curve(u))
    assert (P - r.HALF) % P == r.HALF - 1
    for u in (1, 2, P - 1, 12345):
        assert (r.Z * r.Z * pow(u, 4, P) + r.Z * u * u) % P != 0
        assert r.map_to_curve(P - u) == r.neg(r.map_to_curve(u))                 # so (u, p - u) cancels
    # Z = -4 is a non-square and -Z = 4 has the root 2
    assert pow(r.Z % P, (P - 1) // 2, P) == P - 1
    # no point with y = 0 (odd order): x^3 - 3 x + b has no root that is a point of order 2 — n is odd
    assert N % 2 == 1
    assert r.on_curve(X0) and r.sqrt(r.B) is not None                            # x = 0 is on the curve: b is a square
    assert [r.sqrt(r.rhs(x)) for x in (3, 5, 7, 9)] == [None] * 4                # on no point
    assert r.encode(None) == b"\x00" and r.decode(b"\x00") == "bad" and r.decode(bytes(67)) == "bad"
    assert r.TINY_LEN == 149 and r.THIN_LEN == 200 and r.PEDERSEN_LEN == 400
    assert r.RO.scalar_len == 66 and r.RO.nonce_len == 82 == (521 + 128 + 7) // 8
    for chunk, value in ((0, 0), (P, 0), (P + 1, 1), (2 * P, 0), (2**784 - 1, (2**784 - 1) % P)):
        assert r.reduce_be98(chunk.to_bytes(98, "big")) == value


# ---------------------------------------------------------------- the restatement's VRF layer
P256_FILES = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "*", "secp256r1_sha*_tai_*.json")))
FIELDS = {"pedersen": ("gamma", "proof_pk_com", "proof_r", "proof_ok", "proof_s", "proof_sb"), "thin": ("gamma", "proof_r", "proof_s"),
          "tiny": ("gamma", "proof_c", "proof_s"), "ietf": ("gamma", "proof_c", "proof_s")}


def test_width_suite_reproduces_the_p256_files():
    """p521_ref.WidthSuite with P-256's constants (a 256-bit order: 32-byte scalars, a 48-byte nonce squeeze) against the proof bytes the
    reference recorded for P-256"""
    suite = r.WidthSuite(p256.SUITE_ID, p256.N, p256.G, p256.BLINDING, p256.add, p256.encode, lambda data: p256.encode_to_curve(data)[0],
                         __import__("hashlib").sha256)
    assert suite.scalar_len == 32 and suite.nonce_len == 48 and len(P256_FILES) == 9
    for path in P256_FILES:
        kind = next(k for k in FIELDS if k in os.path.basename(path))
        for v in json.load(open(path))[:2]:
            hx = lambda k: bytes.fromhex(v[k])  # noqa: E731
            sk, al, ad = hx("sk"), hx("alpha"), hx("ad")
            proof = suite.pedersen_prove(sk, al, ad)[0] if kind == "pedersen" else suite.ietf_prove(sk, al, ad, thin=kind == "thin")
            assert proof == b"".join(hx(f) for f in FIELDS[kind])


def test_restatement_vrf_layer_is_self_consistent(golden_dir):
    v = _base(golden_dir)[1]
    sk, alpha, ad = bytes.fromhex(v["sk"]), bytes.fromhex(v["alpha"]), bytes.fromhex(v["ad"])
    pk = r.public_key(sk)
    for suite in (r.RO, r.NU):
        tiny, thin = suite.ietf_prove(sk, alpha, ad), suite.ietf_prove(sk, alpha, ad, thin=True)
        ped, _ = suite.pedersen_prove(sk, alpha, ad)
        assert (len(tiny), len(thin), len(ped)) == (149, 200, 400)
        assert r.ietf_verify(suite, pk, tiny, alpha, ad) and r.ietf_verify(suite, pk, thin, alpha, ad, thin=True)
        assert r.pedersen_verify(suite, ped, alpha, ad)
        assert not r.ietf_verify(suite, pk, tiny, alpha + b"x", ad) and not r.pedersen_verify(suite, ped, alpha, ad + b"x")
    assert r.RO.ietf_prove(sk, alpha, ad) != r.NU.ietf_prove(sk, alpha, ad)


# ---------------------------------------------------------------- the host build of the device headers
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("p521") / "p521_host_check"
    # (-std=c++20: divstep28.hip.h shifts negative values left, which is defined from C++20 on; signed overflow stays undefined)
    subprocess.run(["g++", "-O2", "-std=c++20", "-fsanitize=undefined", "-fno-sanitize-recover", "-I", CSRC,
                    os.path.join(ROOT, "tests", "native", "p521_host_check.cpp"), "-o", str(out)], check=True)
    return str(out)


def _run(exe, lines):
    run = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]                        # (a column overflow aborts the program)
    rows = run.stdout.strip().splitlines()
    assert len(rows) == len(lines)
    return [row.split() for row in rows]


def _hx(v):
    return "%x" % v


def _pt(pt):
    return "0 0" if pt is None else _hx(pt[0]) + " " + _hx(pt[1])


def test_host_field_at_the_limb_bounds_of_the_contract(exe):
    pairs = r.contract_pairs(random.Random(1))
    rows = _run(exe, ["field " + " ".join(map(str, a)) + " " + " ".join(map(str, b)) for a, b in pairs])
    for (a, b), row in zip(pairs, rows):
        got, flags = [int(x, 16) for x in row[:12]], [int(x) for x in row[12:]]
        e = r.field_expectations(a, b)
        assert got[:10] == [e["mul"], e["sqr"], e["add"], e["sub"], e["neg"], e["a"], e["small4"], e["smallneg"], e["inv"], e["inv"]], (a, b)
        assert got[11] == e["a"]
        assert flags == [int(e["square"]), e["odd"], int(e["zero"]), int(e["equal"]), 1, 1]
        if e["square"]:
            assert got[10] * got[10] % P == e["a"]
    values = {tuple(image): value for image, value in r.SPELLED}
    for (a, _), row in zip(pairs, rows):                                  # limbs that spell p, p + 1, 2^521 pack as 0, 1, 1
        if tuple(a) in values:
            assert int(row[11], 16) == values[tuple(a)]
    rows = _run(exe, ["words " + _hx(v) for v in (0, 1, P - 1, P, P + 1, 2**521, 2**532 - 1)])
    assert [(int(a, 16), b) for a, b in rows] == [(0, "1"), (1, "1"), (P - 1, "1"), (0, "0"), (1, "0"), (1, "0"), ((2**532 - 1) % P, "0")]


def test_host_group_law_on_every_pair(exe):
    rng = random.Random(2)
    pts = [None, r.G, r.neg(r.G), r.add(r.G, r.G), X0] + [r.mul(rng.randrange(1, N), r.G) for _ in range(4)]
    lines, want = [], []
    for p1 in pts:
        lines.append("dbl " + _pt(p1))
        want.append(r.add(p1, p1))
        for p2 in pts:                                                    # P + P through add and P + (-P) are among them
            lines.append("add " + _pt(p1) + " " + _pt(p2))
            want.append(r.add(p1, p2))
            lines.append("sub " + _pt(p1) + " " + _pt(p2))
            want.append(r.add(p1, r.neg(p2)))
    rows = _run(exe, lines)
    assert [(int(x, 16), int(y, 16)) for x, y in rows] == [(0, 0) if pt is None else pt for pt in want]


def test_host_map(exe):
    rng = random.Random(3)
    us = [0, 1, P - 1, r.HALF, r.HALF - 1] + [rng.randrange(P) for _ in range(5)]
    rows = _run(exe, ["map " + _hx(u) for u in us])
    assert [(int(x, 16), int(y, 16)) for x, y in rows] == [r.map_to_curve(u) for u in us]


def test_host_scalar_recoding(exe):
    rng = random.Random(4)
    ks = [0, 1, N - 1, N, 2**521 - 1, int("7" * 130, 16) + (1 << 520), int("8" * 130, 16), rng.randrange(2**521)]
    for k, row in zip(ks, _run(exe, ["recode " + _hx(k) for k in ks])):
        digits = [int(x) for x in row]
        assert len(digits) == 136 and all(-8 <= x <= 7 for x in digits) and digits[131:] == [0] * 5
        assert sum(x * 16**i for i, x in enumerate(digits[:131])) == k    # 131 windows and nothing leaves the top one


# ---------------------------------------------------------------- the library on the host
def test_host_hash_to_field_equals_the_restatement(golden_dir):
    msgs = [b"", b"abc", b"a" * 129, bytes(range(200))]
    for cid, per, dst in ((_native.CURVE_P521_RO, 2, r.DST_RO), (_native.CURVE_P521_NU, 1, r.DST_NU)):
        out = _native.p521_hash_to_field_batch(cid, msgs)
        assert out == b"".join(u.to_bytes(68, "little") for m in msgs for u in r.hash_to_field(m, per, dst))
    doc = _vectors(golden_dir, "p521_ro.json")
    out = _native.p521_hash_to_field_batch(_native.CURVE_P521_RO, [v["msg"].encode() for v in doc["vectors"]])
    assert out == b"".join(int(u, 16).to_bytes(68, "little") for v in doc["vectors"] for u in v["u"])
    pt = d.P521.point_type
    assert pt.hash_to_field_pairs([b"abc"], [b"s"]) == b"".join(u.to_bytes(68, "little") for u in r.hash_to_field(b"sabc", 2, r.DST_RO))
    for cid in (19, 21, 15, 4):
        with pytest.raises(ValueError, match="DR_CURVE_P521_RO or DR_CURVE_P521_NU"):
            _native.p521_hash_to_field_batch(cid, [b"a"])
    for other in (_native.ed448_hash_to_field_batch, _native.curve448_hash_to_field_batch, _native.blsg1_hash_to_field_batch):
        with pytest.raises(ValueError):
            other(_native.CURVE_P521_RO, [b"a"])


def test_98_byte_reduction_through_the_host_check():
    """the reduction of the library's hash_to_field on chunks that spell 0, p, p + 1, 2 p and 2^784 - 1, in a stand-alone program"""
    src = r'''
#include <cstdio>
#include "hosth2c.hpp"
int main() {
    unsigned char in[98], out[68];
    for (;;) {
        for (int i = 0; i < 98; i++) { unsigned v; if (std::scanf("%2x", &v) != 1) return 0; in[i] = (unsigned char)v; }
        drh::fp521_reduce_be98(in, out);
        for (int i = 67; i >= 0; i--) std::printf("%02x", out[i]);
        std::printf("\n");
    }
}
'''
    import tempfile

    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "reduce.cpp"), "w") as f:
            f.write(src)
        subprocess.run(["g++", "-O2", "-std=c++17", "-fsanitize=undefined", "-fno-sanitize-recover", "-I", CSRC, os.path.join(tmp, "reduce.cpp"),
                        "-o", os.path.join(tmp, "reduce"), "-pthread"], check=True)
        rng = random.Random(5)
        chunks = [0, P, P + 1, 2 * P, 2**784 - 1, 2**521, (P << 262) + P, 2**783] + [rng.randrange(2**784) for _ in range(8)]
        run = subprocess.run([os.path.join(tmp, "reduce")], input="\n".join(c.to_bytes(98, "big").hex() for c in chunks) + "\n",
                             capture_output=True, text=True)
        assert run.returncode == 0, run.stderr[-2000:]
        assert [int(row, 16) for row in run.stdout.split()] == [c % P for c in chunks]


def test_point_type_on_the_host():
    pt = d.P521.point_type
    assert pt._WIDE and pt._SUITE == "p521" and pt._P == P and pt._N == N and pt._SW_A == -3 and pt._SW_B == r.B and pt._H == 1
    g = pt.generator_point()
    assert (g.x, g.y) == r.G and g.is_on_curve() and not g.is_identity()
    assert g.point_to_string() == r.encode(r.G) and len(g.point_to_string()) == 67
    assert pt.string_to_point(r.encode(r.neg(r.G))) == -g and pt.string_to_point(g.point_to_string(compressed=False)) == g
    assert pt.identity().point_to_string() == b"\x00" and pt.string_to_point(b"\x00").is_identity()
    two = g + g
    assert (two.x, two.y) == r.add(r.G, r.G) and (g - g).is_identity() and g.double() == two and g.clear_cofactor() is g
    assert pt.string_to_point(r.encode(X0)) == pt(*X0)
    for bad, text in ((b"\x02" + P.to_bytes(66, "big"), "not in field"), (b"\x02" + (3).to_bytes(66, "big"), "Invalid point encoding"),
                      (b"\x05" + bytes(66), "prefix"), (b"\x02" + bytes(32), "length"), (b"", "Empty")):
        with pytest.raises(ValueError, match=text):
            pt.string_to_point(bad)
    with pytest.raises(ValueError):
        pt(1, 1)
    with pytest.raises(ValueError):
        pt(P, 0)
    pts = [g, pt.identity(), two]
    packed = pt._pack(pts)
    assert packed == r.raw(r.G) + bytes(136) + r.raw(r.add(r.G, r.G)) and pt._unpack(packed) == pts
    assert pt._scalars([0, 1, N, N + 5, -1, 2**600]) == b"".join(k.to_bytes(68, "little") for k in (0, 1, 0, 5, N - 1, 2**600 % N))
    assert g != d.P256.point_type.generator_point()
    assert d.P521_NU.point_type.generator_point() == g                           # the variants of one curve compare and add


def test_names_ids_exports_and_lengths():
    assert d.P521 is d.P521_RO and d.P521_NU is not d.P521_RO
    for name in ("P521", "P521_RO", "P521_NU"):
        assert hasattr(d, name) and name not in d.__all__                        # Curve448's convention: the recorded surface pins __all__
    assert (_native.CURVE_P521_RO, _native.CURVE_P521_NU) == (23, 24)
    for cv, cid, e2c in ((d.P521_RO, 23, "sswu"), (d.P521_NU, 24, "sswu_nu")):
        sp = cv.curve.params
        assert sp.curve_id == cid and sp.e2c == e2c and sp.suite_id == b"P521_XMD:SHA-512_SSWU_RO_" and sp.cofactor == 1
        assert sp.hash_fn().name == "sha512" and sp.generator == r.G and sp.auxiliary_points.blinding_base == r.G
        assert sp.encoding.point_len == 67 and sp.encoding.challenge_len == 32 and sp.encoding.endian == "little"
        assert sp.field_modulus == P and sp.subgroup_order == N
        assert point_len(cv) == 67 and scalar_len(cv) == 66
        assert d.PedersenVRF[cv].proof_len() == 400
        with pytest.raises(ValueError, match="Twisted Edwards"):
            d.RingVRF[cv]
        with pytest.raises(ValueError, match="Twisted Edwards"):
            d.RingProofParams(cv=cv)
        for scheme in (d.TinyVRF, d.ThinVRF, d.PedersenVRF):
            assert scheme[cv].cv is cv
    w = _native._WIDE["p521"]
    assert (w.elem, w.point, w.scalar, w.enc, w.limbs, w.records, w.nu, w.flagged) == (68, 136, 68, 67, 76, 11, 24, "decode_points")
    names = ["dr_p521_hash_to_field_batch", "dr_p521_map_to_curve", "dr_p521_encode_to_curve_batch", "dr_p521_scalar_mul_batch",
             "dr_p521_msm_groups", "dr_p521_decode_points", "dr_p521_field_selftest", "dr_p521_law_selftest"]
    lib = _native.lib()
    for name in names:
        assert name in _native.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert sorted(s for s in _native.EXPORTED_SYMBOLS if s.startswith("dr_p521")) == sorted(names)
    with open(os.path.join(ROOT, "include", "dotring_hip.h")) as f:
        header = f.read()
    declared = re.findall(r"DR_API\s+[\w\s\*]+?\b(dr_\w+)\s*\(", header)
    assert sorted(declared) == sorted(_native.EXPORTED_SYMBOLS)
    assert "enum { DR_CURVE_P521_RO = 23, DR_CURVE_P521_NU = 24 };" in header
    for call in ("map_to_curve", "encode_to_curve_batch", "scalar_mul_batch", "msm_groups", "decode_points", "field_selftest"):
        assert callable(getattr(_native.Context, "p521_" + call))
