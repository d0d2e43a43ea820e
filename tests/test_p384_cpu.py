"""P384_RO / P384_NU without a GPU: the big-integer restatement (p384_ref.py) against every record of the reference's two RFC 9380 vector
files and the five public keys of its base file, the facts the kernels rely on (the radix identity of the Montgomery step, the order, the
map's exceptional inputs, the points that do and do not exist), the host build of fp384.hip.h, p384_law.hip.h and sswu.hip.h's map under
-fsanitize=undefined against integers (every field operation at the extreme limb images of its contract, both inversions, the fused
pair of products, every pair of a set of points with the exceptional ones in it, the map, the scalar recoding), the library's host
hash_to_field, its 72-byte reduction and its SHA-384 in a second sanitized program, the Python point type on the host, and names, ids
and exports.

The tests of the checker alone pass without the feature: test_restatement_reproduces_the_vector_files,
test_restatement_reproduces_the_public_keys, test_facts_the_kernels_rely_on and test_restatement_vrf_layer_is_self_consistent.  The
others need dot_ring_amd.P384*, dr_p384_*, csrc/fp384.hip.h or hosth2c.hpp's fp384_reduce_be72 and fail on the parent."""
import hashlib
import json
import os
import random
import re
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import p384_ref as r  # noqa: E402

import dot_ring_amd as d  # noqa: E402
from dot_ring_amd import _native  # noqa: E402
from dot_ring_amd.vrf.codec import point_len, scalar_len  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dot_ring_amd", "csrc")
P, N = r.P, r.N
HEX96 = re.compile(r"^[0-9a-f]{96}$")
X0 = (0, r.sqrt(r.B))


def _vectors(golden_dir, name):
    with open(os.path.join(golden_dir, "h2c", name)) as f:
        return json.load(f)


def _base(golden_dir):
    with open(os.path.join(golden_dir, "base", "p384_base_vectors.json")) as f:
        return json.load(f)


# ---------------------------------------------------------------- the restatement against the reference's data
def test_restatement_reproduces_the_vector_files(golden_dir):
    matched_u = matched_q = matched_p = 0
    for name, nu in (("p384_ro.json", False), ("p384_nu.json", True)):
        doc = _vectors(golden_dir, name)
        dst = doc["dst"].encode()
        assert dst == (r.DST_NU if nu else r.DST_RO) and len(dst) == 44 and doc["suite"].encode() == dst[len(b"QUUX-V01-CS02-with-"):]
        assert len(doc["vectors"]) == 5
        for v in doc["vectors"]:
            us = r.hash_to_field(v["msg"].encode(), 1 if nu else 2, dst)
            assert [int(u, 16) for u in v["u"]] == us and all(HEX96.match(u) for u in v["u"])
            matched_u += len(us)
            images = [r.map_to_curve(u) for u in us]
            for key, image in zip(("Q",) if nu else ("Q0", "Q1"), images):
                assert (int(v[key]["x"], 16), int(v[key]["y"], 16)) == image and r.on_curve(image)       # no record excepted
                matched_q += 1
            total = None
            for image in images:
                total = r.add(total, image)
            assert total == (int(v["P"]["x"], 16), int(v["P"]["y"], 16))
            matched_p += 1
    assert (matched_u, matched_q, matched_p) == (15, 15, 10)


def test_restatement_reproduces_the_public_keys(golden_dir):
    recs = _base(golden_dir)
    assert len(recs) == 5 and {len(v["sk"]) // 2 for v in recs} == {48}
    for v in recs:
        assert r.public_key(bytes.fromhex(v["sk"])).hex() == v["pk"] and len(v["pk"]) == 98
        assert v["h"] == v["gamma"] == v["proof_c"] == v["proof_s"] == v["beta"] == ""       # the reference holds no P-384 proof bytes


def test_facts_the_kernels_rely_on():
    assert P == 2**384 - 2**128 - 2**96 + 2**32 - 1 and P % 4 == 3 and N.bit_length() == 384 and N < P and N % 2 == 1
    # the radix identity behind the Montgomery step: p = -1 + 2^4 B - 2^12 B^3 - 2^16 B^4 + 2^20 B^13, so -p^-1 = 1 mod B
    b28 = 1 << 28
    assert P == -1 + 2**4 * b28 - 2**12 * b28**3 - 2**16 * b28**4 + 2**20 * b28**13 and (-pow(P, -1, b28)) % b28 == 1
    assert r.R == b28**14 and r.R % P == (2**8 - 2**12 * b28 + 2**20 * b28**3 + 2**24 * b28**4) % P      # F384::small's limbs
    assert 2**384 % P == 2**128 + 2**96 - 2**32 + 1                              # carry's fold, the 72-byte reduction
    assert (49 * 384 + 57) // 17 == 1110 <= 40 * 28 and 21 * P < 2**389          # the division steps' batches and their bound
    assert r.on_curve(r.G) and r.mul(N, r.G) is None and r.mul(N - 1, r.G) == r.neg(r.G) and r.BLINDING == r.G
    # the map's exceptional branch: Z u^2 = -1 iff u^2 = 1 / 12; B / (Z A) is the x of a point, and all three inputs land on it
    x1 = r.B * pow(r.Z * r.A % P, -1, P) % P
    assert r.sqrt(r.rhs(x1)) is not None
    assert 12 * r.S * r.S % P == 1
    for u in (0, r.S, P - r.S):
        assert (r.Z * r.Z * pow(u, 4, P) + r.Z * u * u) % P == 0
        assert r.map_to_curve(u)[0] == x1 and r.on_curve(r.map_to_curve(u))
    for u in (1, 2, P - 1, 12345):
        assert (r.Z * r.Z * pow(u, 4, P) + r.Z * u * u) % P != 0
        assert r.map_to_curve(P - u) == r.neg(r.map_to_curve(u))                 # so (u, p - u) cancels
    # Z = -12 is a non-square and -Z = 12 has a root
    assert pow(r.Z % P, (P - 1) // 2, P) == P - 1 and r.sqrt(12) is not None
    assert r.on_curve(X0) and r.sqrt(r.B) is not None and r.rhs(0) != 0          # x = 0 is on the curve; (0, 0) is not
    assert r.encode(None) == b"\x00" and r.decode(b"\x00") == "bad" and r.decode(bytes(49)) == "bad"
    assert (r.TINY_LEN, r.THIN_LEN, r.PEDERSEN_LEN) == (113, 146, 292)
    assert r.RO.scalar_len == 48 and r.RO.nonce_len == 64 == (384 + 128 + 7) // 8
    for chunk, value in ((0, 0), (P, 0), (P + 1, 1), (2 * P, 0), (2**384, 2**384 - P), (2**576 - 1, (2**576 - 1) % P)):
        assert r.reduce_be72(chunk.to_bytes(72, "big")) == value


def test_restatement_vrf_layer_is_self_consistent(golden_dir):
    v = _base(golden_dir)[1]
    sk, alpha, ad = bytes.fromhex(v["sk"]), bytes.fromhex(v["alpha"]), bytes.fromhex(v["ad"])
    pk = r.public_key(sk)
    for suite in (r.RO, r.NU):
        tiny, thin = suite.ietf_prove(sk, alpha, ad), suite.ietf_prove(sk, alpha, ad, thin=True)
        ped, _ = suite.pedersen_prove(sk, alpha, ad)
        assert (len(tiny), len(thin), len(ped)) == (113, 146, 292)
        assert r.ietf_verify(suite, pk, tiny, alpha, ad) and r.ietf_verify(suite, pk, thin, alpha, ad, thin=True)
        assert r.pedersen_verify(suite, ped, alpha, ad)
        assert not r.ietf_verify(suite, pk, tiny, alpha + b"x", ad) and not r.pedersen_verify(suite, ped, alpha, ad + b"x")
    assert r.RO.ietf_prove(sk, alpha, ad) != r.NU.ietf_prove(sk, alpha, ad)


# ---------------------------------------------------------------- the host build of the device headers
def _build(tmp, source, name, std="c++20"):
    out = os.path.join(str(tmp), name)
    # (-std=c++20: divstep28.hip.h shifts negative values left, which is defined from C++20 on; signed overflow stays undefined)
    subprocess.run(["g++", "-O2", "-std=" + std, "-fsanitize=undefined", "-fno-sanitize-recover", "-I", CSRC, source, "-o", out, "-pthread"], check=True)
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("p384"), os.path.join(ROOT, "tests", "native", "p384_host_check.cpp"), "p384_host_check")


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


def _image(image):
    return " ".join(map(str, image))


def test_host_field_at_the_limb_bounds_of_the_contract(exe):
    pairs = r.contract_pairs(random.Random(1))
    rows = _run(exe, ["field " + _image(a) + " " + _image(b) for a, b in pairs])
    for (a, b), row in zip(pairs, rows):
        got, flags = [int(x, 16) for x in row[:14]], [int(x) for x in row[14:]]
        e = r.field_expectations(a, b)
        # (the two inversions, by division steps and by the chain of p - 2, are columns 8 and 9)
        assert got[:10] == [e["mul"], e["sqr"], e["add"], e["sub"], e["neg"], e["a"], e["small4"], e["smallneg"], e["inv"], e["inv"]], (a, b)
        assert got[11] == e["a"] and got[12] == e["sqr"] and got[13] == 2 * e["mul"] % P
        assert flags == [int(e["square"]), e["odd"], int(e["zero"]), int(e["equal"]), 1, 1]
        if e["square"]:
            assert got[10] * got[10] % P == e["a"]
    values = {tuple(image): value for image, value in r.SPELLED}
    seen = 0
    for (a, _), row in zip(pairs, rows):                                  # limbs that spell p, p + 1, 2^384, 2^392 - 1
        if tuple(a) in values:
            assert int(row[11], 16) == values[tuple(a)]
            seen += 1
    assert seen >= 4 and values[tuple(r.limbs(P))] == 0
    quads = r.mul2_quads(random.Random(6))
    rows = _run(exe, ["mul2 " + " ".join(_image(x) for x in q) for q in quads])
    for q, row in zip(quads, rows):
        a, b, c, dd = (r.limb_value(x) for x in q)
        assert int(row[0], 16) == (a * b + c * dd) % P
    rows = _run(exe, ["words " + _hx(v) for v in (0, 1, P - 1, P, P + 1, 2**384 - 1)])
    assert [(int(a, 16), b) for a, b in rows] == [(0, "1"), (1, "1"), (P - 1, "1"), (0, "0"), (1, "0"), ((2**384 - 1) % P, "0")]


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
    us = [0, 1, P - 1, r.S, P - r.S] + [rng.randrange(P) for _ in range(5)]
    rows = _run(exe, ["map " + _hx(u) for u in us])
    assert [(int(x, 16), int(y, 16)) for x, y in rows] == [r.map_to_curve(u) for u in us]


def test_host_scalar_recoding(exe):
    rng = random.Random(4)
    ks = [0, 1, N - 1, N, 2**384 - 1, int("7" * 96, 16), int("8" * 96, 16), rng.randrange(2**384)]
    carries = []
    for k, row in zip(ks, _run(exe, ["recode " + _hx(k) for k in ks])):
        digits = [int(x) for x in row]
        assert len(digits) == 97 and all(-8 <= x <= 7 for x in digits[:96]) and digits[96] in (0, 1)
        assert sum(x * 16**i for i, x in enumerate(digits)) == k         # 96 digits and the carry out of the top one as digit 96
        carries.append(digits[96])
    assert carries[4] == 1 and carries[6] == 1 and carries[0] == 0        # the 97th window is needed


# ---------------------------------------------------------------- the library on the host
def test_host_hash_to_field_equals_the_restatement(golden_dir):
    msgs = [b"", b"abc", b"a" * 129, bytes(range(200))]
    for cid, per, dst in ((_native.CURVE_P384_RO, 2, r.DST_RO), (_native.CURVE_P384_NU, 1, r.DST_NU)):
        out = _native.p384_hash_to_field_batch(cid, msgs)
        assert out == b"".join(u.to_bytes(48, "little") for m in msgs for u in r.hash_to_field(m, per, dst))
    for name, cid in (("p384_ro.json", _native.CURVE_P384_RO), ("p384_nu.json", _native.CURVE_P384_NU)):
        doc = _vectors(golden_dir, name)
        out = _native.p384_hash_to_field_batch(cid, [v["msg"].encode() for v in doc["vectors"]])
        assert out == b"".join(int(u, 16).to_bytes(48, "little") for v in doc["vectors"] for u in v["u"])
    pt = d.P384.point_type
    assert pt.hash_to_field_pairs([b"abc"], [b"s"]) == b"".join(u.to_bytes(48, "little") for u in r.hash_to_field(b"sabc", 2, r.DST_RO))
    for cid in (19, 21, 23, 24, 15, 4):
        with pytest.raises(ValueError, match="DR_CURVE_P384_RO or DR_CURVE_P384_NU"):
            _native.p384_hash_to_field_batch(cid, [b"a"])
    for other in (_native.ed448_hash_to_field_batch, _native.curve448_hash_to_field_batch, _native.blsg1_hash_to_field_batch,
                  _native.p521_hash_to_field_batch):
        with pytest.raises(ValueError):
            other(_native.CURVE_P384_RO, [b"a"])


HASH_CHECK = r'''
#include <cstdio>
#include "hosth2c.hpp"
// lines `r <144 hex digits>`: fp384_reduce_be72, 96 hex digits out; lines `s <n>`: Sha384 of the n bytes (7 i + 1) mod 256
int main() {
    char op[8];
    while (std::scanf("%7s", op) == 1) {
        if (op[0] == 'r') {
            unsigned char in[72], out[48];
            for (int i = 0; i < 72; i++) { unsigned v; if (std::scanf("%2x", &v) != 1) return 2; in[i] = (unsigned char)v; }
            drh::fp384_reduce_be72(in, out);
            for (int i = 47; i >= 0; i--) std::printf("%02x", out[i]);
        } else {
            unsigned n;
            if (std::scanf("%u", &n) != 1 || n > 1024) return 2;
            static unsigned char buf[1024];
            unsigned char out[48];
            for (unsigned i = 0; i < n; i++) buf[i] = (unsigned char)(i * 7 + 1);
            drh::Sha384 h;
            h.update(buf, n / 2);
            h.update(buf + n / 2, n - n / 2);
            h.final(out);
            for (int i = 0; i < 48; i++) std::printf("%02x", out[i]);
        }
        std::printf("\n");
    }
    return 0;
}
'''


def test_72_byte_reduction_and_sha384_in_a_sanitized_program(tmp_path):
    """the reduction of the library's hash_to_field on chunks that spell 0, p, p + 1, 2 p, 2^384, 2^576 - 1 and random values, and its
    SHA-384 against hashlib at the lengths around the padding's edges, in a stand-alone program"""
    src = tmp_path / "hash_check.cpp"
    src.write_text(HASH_CHECK)
    prog = _build(tmp_path, str(src), "hash_check", std="c++17")
    rng = random.Random(5)
    chunks = [0, P, P + 1, 2 * P, 2**384, 2**576 - 1, ((2**192 - 1) << 384) + P, ((2**192 - 1) << 384) + P - 1, 2**575]
    chunks += [rng.randrange(2**576) for _ in range(16)]
    lens = [0, 1, 111, 112, 127, 128, 129, 300]
    lines = ["r " + c.to_bytes(72, "big").hex() for c in chunks] + ["s %d" % n for n in lens]
    run = subprocess.run([prog], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    rows = run.stdout.split()
    assert [int(row, 16) for row in rows[: len(chunks)]] == [c % P for c in chunks]
    assert rows[len(chunks):] == [hashlib.sha384(bytes((7 * i + 1) & 255 for i in range(n))).hexdigest() for n in lens]


def test_point_type_on_the_host():
    pt = d.P384.point_type
    assert pt._WIDE and pt._SUITE == "p384" and pt._P == P and pt._N == N and pt._SW_A == -3 and pt._SW_B == r.B and pt._H == 1
    assert pt._SEC1_LEN == 48
    g = pt.generator_point()
    assert (g.x, g.y) == r.G and g.is_on_curve() and not g.is_identity()
    assert g.point_to_string() == r.encode(r.G) and len(g.point_to_string()) == 49
    assert pt.string_to_point(r.encode(r.neg(r.G))) == -g and pt.string_to_point(g.point_to_string(compressed=False)) == g
    assert pt.identity().point_to_string() == b"\x00" and pt.string_to_point(b"\x00").is_identity()
    two = g + g
    assert (two.x, two.y) == r.add(r.G, r.G) and (g - g).is_identity() and g.double() == two and g.clear_cofactor() is g
    assert pt.string_to_point(r.encode(X0)) == pt(*X0)
    no_point = next(x for x in range(2, 40) if r.sqrt(r.rhs(x)) is None)
    for bad, text in ((b"\x02" + P.to_bytes(48, "big"), "not in field"), (b"\x02" + no_point.to_bytes(48, "big"), "Invalid point encoding"),
                      (b"\x05" + bytes(48), "prefix"), (b"\x02" + bytes(32), "length"), (b"", "Empty")):
        with pytest.raises(ValueError, match=text):
            pt.string_to_point(bad)
    with pytest.raises(ValueError):
        pt(1, 1)
    with pytest.raises(ValueError):
        pt(P, 0)
    pts = [g, pt.identity(), two]
    packed = pt._pack(pts)
    assert packed == r.raw(r.G) + bytes(96) + r.raw(r.add(r.G, r.G)) and pt._unpack(packed) == pts
    assert pt._scalars([0, 1, N, N + 5, -1, 2**600]) == b"".join(k.to_bytes(48, "little") for k in (0, 1, 0, 5, N - 1, 2**600 % N))
    assert g != d.P256.point_type.generator_point() and g != d.P521.point_type.generator_point()
    assert d.P384_NU.point_type.generator_point() == g                           # the variants of one curve compare and add


def test_names_ids_exports_and_lengths():
    assert d.P384 is d.P384_RO and d.P384_NU is not d.P384_RO
    for name in ("P384", "P384_RO", "P384_NU"):
        assert hasattr(d, name) and name not in d.__all__                        # Curve448's convention: the recorded surface pins __all__
    assert (_native.CURVE_P384_RO, _native.CURVE_P384_NU) == (25, 26)
    for cv, cid, e2c in ((d.P384_RO, 25, "sswu"), (d.P384_NU, 26, "sswu_nu")):
        sp = cv.curve.params
        assert sp.curve_id == cid and sp.e2c == e2c and sp.suite_id == b"P384_XMD:SHA-384_SSWU_RO_" and sp.cofactor == 1
        assert sp.hash_fn().name == "sha384" and sp.hash_fn().digest_size == 48
        assert sp.generator == r.G and sp.auxiliary_points.blinding_base == r.G
        assert sp.encoding.point_len == 49 and sp.encoding.challenge_len == 24 and sp.encoding.endian == "little"
        assert sp.field_modulus == P and sp.subgroup_order == N
        assert point_len(cv) == 49 and scalar_len(cv) == 48
        assert d.PedersenVRF[cv].proof_len() == 292
        with pytest.raises(ValueError, match="Twisted Edwards"):
            d.RingVRF[cv]
        with pytest.raises(ValueError, match="Twisted Edwards"):
            d.RingProofParams(cv=cv)
        for scheme in (d.TinyVRF, d.ThinVRF, d.PedersenVRF):
            assert scheme[cv].cv is cv
    w = _native._WIDE["p384"]
    assert (w.elem, w.point, w.scalar, w.enc, w.limbs, w.records, w.nu, w.flagged) == (48, 96, 48, 49, 56, 13, 26, "decode_points")
    names = ["dr_p384_hash_to_field_batch", "dr_p384_map_to_curve", "dr_p384_encode_to_curve_batch", "dr_p384_scalar_mul_batch",
             "dr_p384_msm_groups", "dr_p384_decode_points", "dr_p384_field_selftest", "dr_p384_law_selftest"]
    lib = _native.lib()
    for name in names:
        assert name in _native.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert sorted(s for s in _native.EXPORTED_SYMBOLS if s.startswith("dr_p384")) == sorted(names)
    with open(os.path.join(ROOT, "include", "dotring_hip.h")) as f:
        header = f.read()
    declared = re.findall(r"DR_API\s+[\w\s\*]+?\b(dr_\w+)\s*\(", header)
    assert sorted(declared) == sorted(_native.EXPORTED_SYMBOLS)
    assert "enum { DR_CURVE_P384_RO = 25, DR_CURVE_P384_NU = 26 };" in header
    for call in ("map_to_curve", "encode_to_curve_batch", "scalar_mul_batch", "msm_groups", "decode_points", "field_selftest"):
        assert callable(getattr(_native.Context, "p384_" + call))
    assert callable(_native.p384_hash_to_field_batch)
