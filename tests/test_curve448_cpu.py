"""Curve448_RO / Curve448_NU without a GPU: the big-integer restatement (curve448_ref.py) against the strings of the reference's two
RFC 9380 vector files, the facts the device law relies on (which of A - 2, A + 2, A^2 - 4, -A, -1 are squares, the group order, the
points of order 4), the host build of c448_law.hip.h under -fsanitize=undefined against integers (every pair of a set of points with the
exceptional ones in it, and the extreme limb images of the contract), the Python point type on the host, names, ids and exports, and the
pin of the restatement's VRF layer on the reference's Bandersnatch SHAKE128 proof files.

The tests of the checker alone pass without the feature: test_restatement_reproduces_the_vector_files, test_facts_the_law_relies_on,
test_inner_curve_law_matches_the_montgomery_law, test_xof_suite_reproduces_the_bandersnatch_shake128_files and
test_restatement_vrf_layer_is_self_consistent.  The others need dot_ring_amd.Curve448*, dr_curve448_* or csrc/c448_law.hip.h."""
import hashlib
import json
import os
import random
import re
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import curve448_ref as c  # noqa: E402
import ed448_ref as e4  # noqa: E402

import dot_ring_amd as d  # noqa: E402
from dot_ring_amd import _native  # noqa: E402
from dot_ring_amd.vrf.codec import point_len, scalar_len  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dot_ring_amd", "csrc")
P, N, A = c.P, c.N, c.A
HEX112 = re.compile(r"^[0-9a-f]{112}$")
# the one record of the two files that is no point of the curve (the restatement's image of the same u is): curve448_nu.json, vector 2,
# whose y string lacks one hexadecimal digit
NOT_A_POINT = {("curve448_nu.json", 2, "Q")}


def _vectors(golden_dir, name):
    with open(os.path.join(golden_dir, "h2c", name)) as f:
        return json.load(f)


def _num(s):
    assert HEX112.match(s), s
    return int(s, 16)


# ---------------------------------------------------------------- the restatement against the reference's vectors
def test_restatement_reproduces_the_vector_files(golden_dir):
    matched_p = excluded = 0
    for name, nu in (("curve448_ro.json", False), ("curve448_nu.json", True)):
        doc = _vectors(golden_dir, name)
        dst = doc["dst"].encode()
        assert dst == (c.DST_NU if nu else c.DST_RO) and len(dst) == 49 and doc["suite"].encode() == dst[len(b"QUUX-V01-CS02-with-"):]
        assert len(doc["vectors"]) == 5
        for index, v in enumerate(doc["vectors"]):
            msg = v["msg"].encode()
            us = c.hash_to_field(msg, 1 if nu else 2, dst)
            assert [_num(u) for u in v["u"]] == us                       # every u, no exception
            images = [c.map_to_curve(u) for u in us]
            for key, img in zip(("Q",) if nu else ("Q0", "Q1"), images):
                if (name, index, key) in NOT_A_POINT:
                    # its y has 111 digits: read as it stands it is no point of the curve, and it is the image's y with one
                    # hexadecimal digit missing
                    x, y_str = _num(v[key]["x"]), v[key]["y"]
                    assert len(y_str) == 111 and not c.on_curve((x, int(y_str, 16))) and c.on_curve(img)
                    full = f"{img[1]:0112x}"
                    assert x == img[0] and any(full[:i] + full[i + 1:] == y_str for i in range(112))
                    excluded += 1
                else:
                    assert (_num(v[key]["x"]), _num(v[key]["y"])) == img
            pt = (c.encode_to_curve_nu if nu else c.encode_to_curve_ro)(msg)
            assert (_num(v["P"]["x"]), _num(v["P"]["y"])) == pt          # every P, no exception
            assert pt is not None and c.mul(N, pt) is None
            matched_p += 1
    assert matched_p == 10 and excluded == len(NOT_A_POINT) == 1


def _is_probable_prime(n):
    r, s = n - 1, 0
    while r % 2 == 0:
        r, s = r // 2, s + 1
    for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        x = pow(a, r, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def test_facts_the_law_relies_on():
    # a = A - 2 is a square and d = A + 2 is not: add-2008-bbjlp is complete on the inner curve; A^2 - 4 a non-square: v = 0 at (0, 0)
    # alone; -A a non-square: u = 0 maps to (0, 0); -1 a non-square: p = 3 mod 4
    assert c.is_square(A - 2) and not c.is_square(A + 2) and not c.is_square(A * A - 4) and not c.is_square(-A) and not c.is_square(-1)
    assert (c.INNER_A, c.INNER_D) == (A - 2, A + 2) == (156324, 156328)
    assert not c.on_curve((1, 0)) and all(not c.on_curve((1, v)) for v in (1, 2)) and not c.is_square(1 + A + 1)   # u = 1 is on no point
    assert c.on_curve(c.G) and c.G[0] == 5 and c.mul(N, c.G) is None and _is_probable_prime(N) and _is_probable_prime(P)
    # (0, 0) has order 2 and (-1, +-sqrt(A - 2)) order 4, doubling to (0, 0): 4 | #E, n | #E, and 4 n is the only multiple of 4 n
    # within Hasse's interval
    assert c.on_curve(c.TWO_TORSION) and c.add(c.TWO_TORSION, c.TWO_TORSION) is None
    for t4 in (c.T4, c.neg(c.T4)):
        assert t4[0] == P - 1 and t4[1] ** 2 % P == A - 2 and c.on_curve(t4)
        assert c.add(t4, t4) == c.TWO_TORSION and c.mul(4, t4) is None and c.mul(3, t4) == c.neg(t4)
    assert (P + 1 - 4 * N) ** 2 <= 4 * P and (4 * N) ** 2 > 16 * P
    q = c.add(c.G, c.T4)                                                 # a point of order 4 n
    assert c.mul(N, q) is not None and c.mul(2 * N, q) is not None and c.mul(4 * N, q) is None
    assert c.mul(-3, c.G) == c.neg(c.mul(3, c.G)) and c.mul(4 * N + 5, q) == c.mul(5, q)
    # the valueless inputs of the map, and the one that maps to (0, 0)
    for u in (1, P - 1):
        with pytest.raises(ValueError, match="No inverse exists"):
            c.map_to_curve(u)
    assert c.map_to_curve(0) == c.TWO_TORSION


def _special_points(rng, extra=4):
    return ([None, c.TWO_TORSION, c.T4, c.neg(c.T4), c.G, c.neg(c.G), c.add(c.G, c.TWO_TORSION), c.add(c.G, c.T4)]
            + [c.mul(rng.randrange(1, 4 * N), c.add(c.G, c.T4)) for _ in range(extra)])


def _inner_add(p1, p2):
    (x1, y1), (x2, y2) = p1, p2
    t = c.INNER_D * x1 * x2 * y1 * y2 % P
    return (x1 * y2 + y1 * x2) * pow(1 + t, -1, P) % P, (y1 * y2 - c.INNER_A * x1 * x2) * pow(1 - t, -1, P) % P


def test_inner_curve_law_matches_the_montgomery_law():
    """the birational map carries the reference's affine law to the affine Edwards addition on a x^2 + y^2 = 1 + d x^2 y^2"""
    pts = _special_points(random.Random(21))
    for p1 in pts:
        assert c.inner_on_curve(c.to_inner(p1)) and c.from_inner(c.to_inner(p1)) == p1
        for p2 in pts:
            assert c.from_inner(_inner_add(c.to_inner(p1), c.to_inner(p2))) == c.add(p1, p2)


# ---------------------------------------------------------------- c448_law.hip.h on the host, under the undefined-behaviour sanitizer
@pytest.fixture(scope="module")
def law_checker(tmp_path_factory):
    exe = tmp_path_factory.mktemp("curve448") / "c448_law_host_check"
    # (-std=c++20: divstep28.hip.h shifts negative values left, which is defined from C++20 on; signed overflow stays undefined)
    subprocess.run(["g++", "-O2", "-std=c++20", "-fsanitize=undefined", "-fno-sanitize-recover", "-I", CSRC,
                    os.path.join(ROOT, "tests", "native", "c448_law_host_check.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def _ask(exe, lines):
    run = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]                        # (a column overflow aborts the program)
    rows = run.stdout.strip().splitlines()
    assert len(rows) == len(lines)
    return [row.split() for row in rows]


def _arg(pt):
    return "1 0 0" if pt is None else f"0 {pt[0]:x} {pt[1]:x}"


def _stored(fields):
    flag, u, v = int(fields[0]), int(fields[1], 16), int(fields[2], 16)
    assert len(fields[1]) == len(fields[2]) == 112 and u < P and v < P
    if flag:
        assert u == v == 0                                                # the identity stores zero bytes
        return None
    return u, v


def test_device_law_on_the_host_against_integers(law_checker):
    pts = _special_points(random.Random(448))
    lines, want = [], []
    for p1 in pts:
        for p2 in pts:                                                    # every pair, P + P through `add` among them
            lines.append(f"add {_arg(p1)} {_arg(p2)}")
            want.append(c.add(p1, p2))
        lines.append(f"sub {_arg(p1)} {_arg(p1)}")                        # P + (-P)
        want.append(None)
        lines.append(f"sub {_arg(c.G)} {_arg(p1)}")
        want.append(c.add(c.G, c.neg(p1)))
        lines.append(f"dbl {_arg(p1)}")
        want.append(c.add(p1, p1))
    for fields, line, w in zip(_ask(law_checker, lines), lines, want):
        assert _stored(fields) == w, line[:80]


def test_device_map_on_the_host_against_integers(law_checker):
    rng = random.Random(9380)
    us = [0, 1, P - 1, 2, P - 2, 7] + [rng.randrange(P) for _ in range(8)]
    lines = [f"ell2 {u:x}" for u in us]
    for u, fields in zip(us, _ask(law_checker, lines)):
        if u in (1, P - 1):
            assert fields[0] == "0"
            continue
        assert fields[0] == "1" and _stored(fields[1:]) == c.map_to_curve(u), u
    assert c.map_to_curve(0) == (0, 0)
    cases = [(c.G, 1), (c.TWO_TORSION, 1), (c.T4, 1), ((5, 5), 0), ((1, 0), 0), ((0, 1), 0), (c.add(c.G, c.T4), 1)]
    rows = _ask(law_checker, [f"oncurve {u:x} {v:x}" for (u, v), _ in cases])
    assert [int(r[0]) for r in rows] == [w for _, w in cases]


NORMAL = 2**28 + 2**10


def _val(limbs):
    return sum(x << (28 * i) for i, x in enumerate(limbs))


def _extremes(lo, hi, rng, extra=2):
    yield [hi] * 16
    yield [lo] * 16
    yield [hi if i % 2 else lo for i in range(16)]
    yield [lo if i % 2 else hi for i in range(16)]
    for _ in range(extra):
        yield [rng.randint(lo, hi) for _ in range(16)]


def test_device_law_at_the_extreme_limb_images(law_checker):
    """m448_add and m448_dbl take coordinates "n" (limbs in (-2^10, 2^28 + 2^10)) with x possibly negated ("1 n"): every combination of
    the all-positive, all-negative and alternating images, as projective values against the formulas in integers"""
    rng = random.Random(28)
    a, dd = c.INNER_A, c.INNER_D
    xs = list(_extremes(-NORMAL + 1, NORMAL - 1, rng))
    ns = list(_extremes(-(2**10) + 1, NORMAL - 1, rng))
    lines, want = [], []
    for x1 in xs:
        for yz1 in ns:
            lines.append("rawdbl " + " ".join(str(t) for limbs in (x1, yz1, yz1[::-1]) for t in limbs))
            X, Y, Z = _val(x1), _val(yz1), _val(yz1[::-1])
            B, C, D = (X + Y) ** 2, X * X, Y * Y
            E = a * C
            F = E + D
            J = F - 2 * Z * Z
            want.append(((B - C - D) * J % P, F * (E - D) % P, F * J % P))
            for x2 in xs[:4]:
                for yz2 in ns[:4]:
                    lines.append("rawadd " + " ".join(str(t) for limbs in (x1, yz1, yz1[::-1], x2, yz2[::-1], yz2) for t in limbs))
                    X2, Y2, Z2 = _val(x2), _val(yz2[::-1]), _val(yz2)
                    AA = Z * Z2
                    B, C, D = AA * AA, X * X2, Y * Y2
                    E = dd * C * D
                    F, G = B - E, B + E
                    want.append((AA * F * ((X + Y) * (X2 + Y2) - C - D) % P, AA * G * (D - a * C) % P, F * G % P))
    for fields, line, w in zip(_ask(law_checker, lines), lines, want):
        assert tuple(int(f, 16) for f in fields) == w, line[:40]


# ---------------------------------------------------------------- the Python point type on the host
def test_names_and_parameters():
    assert d.Curve448 is d.Curve448_RO and d.Curve448_NU is not d.Curve448_RO
    from dot_ring_amd import Curve448_RO  # noqa: F401  (importable)
    assert not {"Curve448", "Curve448_RO", "Curve448_NU"} & set(d.__all__)      # the recorded point surface names __all__'s variants
    for cv, cid, e2c in ((d.Curve448_RO, 21, "ell2"), (d.Curve448_NU, 22, "ell2_nu")):
        sp = cv.curve.params
        assert sp.suite_id == c.SUITE_ID and sp.hash_fn is hashlib.shake_256 and sp.xof and sp.cofactor == 4
        assert sp.curve_id == cid == cv.point_type._CV and sp.e2c == e2c
        assert sp.field_modulus == P and sp.subgroup_order == N and sp.generator == c.G and sp.a == A
        assert sp.auxiliary_points.blinding_base == c.G and not sp.auxiliary_points.accumulator_base and not sp.auxiliary_points.padding_point
        assert sp.encoding.point_len == 56 and sp.encoding.uncompressed and sp.encoding.challenge_len == 28
        assert point_len(cv) == 112 and scalar_len(cv) == 56
        assert d.PedersenVRF[cv].proof_len() == 4 * 112 + 2 * 56 == len(c.RO.pedersen_prove(bytes(range(1, 57)), b"m", b"")[0])
        assert d.TinyVRF[cv].cv is cv and d.ThinVRF[cv].cv is cv
        with pytest.raises(ValueError):
            d.RingVRF[cv]
        with pytest.raises(ValueError):
            d.RingProofParams(cv=cv)
        pt = cv.point_type
        assert pt._WIDE and pt._SUITE == "curve448" and pt._IDENTITY_BYTES == b"\xff" * 112 and pt._NO_IMAGE == "No inverse exists"
    assert (_native.CURVE_CURVE448_RO, _native.CURVE_CURVE448_NU) == (21, 22)
    w = _native._WIDE["curve448"]
    assert (w.elem, w.point, w.scalar, w.enc, w.nu, w.flagged) == (56, 112, 56, 112, 22, "decode_points")


def test_point_codec_and_group_on_the_host():
    pt = d.Curve448.point_type
    g = pt.generator_point()
    assert (g.x, g.y) == c.G and g.is_on_curve() and not g.is_identity()
    o = pt.identity()
    assert (o.x, o.y) == (None, None) and o.is_identity() and o.is_on_curve()
    as_pt = lambda t: o if t is None else pt(*t)  # noqa: E731
    pts = _special_points(random.Random(5), extra=2)
    for p1 in pts:
        for p2 in pts:
            assert as_pt(p1) + as_pt(p2) == as_pt(c.add(p1, p2))
        assert -as_pt(p1) == as_pt(c.neg(p1)) and as_pt(p1).double() == as_pt(c.add(p1, p1)) and as_pt(p1) - as_pt(p1) == o
        assert as_pt(p1).clear_cofactor() == as_pt(c.mul(4, p1))
    assert hash(g) == hash(pt(*c.G)) and g != d.Curve25519.point_type.generator_point()
    raw = g.point_to_string()
    assert raw == c.raw(c.G) and len(raw) == 112 and pt.string_to_point(raw) == g and pt.string_to_point(raw.hex()) == g
    assert pt.string_to_point(bytes(112)) == pt(0, 0)                          # (0, 0) is a point of the curve
    with pytest.raises(ValueError, match="Cannot serialize point at infinity"):
        o.point_to_string()
    with pytest.raises(ValueError, match="Point is not on the curve"):
        pt.string_to_point(c.raw((1, 1)))
    with pytest.raises(ValueError, match="Invalid point coordinates"):
        pt.string_to_point(c.raw((P, 1)))
    with pytest.raises(ValueError, match="Invalid point coordinates"):
        pt.string_to_point(b"\xff" * 112)                                      # the library's identity bytes are no encoding
    with pytest.raises(ValueError, match="Invalid point length"):
        pt.string_to_point(raw[:-1])
    with pytest.raises(ValueError, match="Invalid point coordinates"):
        pt(5, None)
    assert pt._pack([g, o, pt(0, 0)]) == c.raw(c.G) + b"\xff" * 112 + bytes(112)
    assert pt._unpack(c.raw(c.G) + b"\xff" * 112 + bytes(112)) == [g, o, pt(0, 0)]
    # scalars leave reduced mod 4 n, the order of the group: exact for every integer and every point
    assert pt._scalars([0, 1, N, 4 * N, 4 * N + 3, -1]) == b"".join(k.to_bytes(56, "little") for k in (0, 1, N, 0, 3, 4 * N - 1))
    assert d.Curve448_NU.point_type is not pt and d.Curve448.point(g) is g and d.Curve448.point(*c.G) == g


def test_curve25519_keeps_its_surface_under_the_shared_base():
    from dot_ring_amd.curve import Curve25519Point, Curve448Point, _MontgomeryPoint

    assert issubclass(Curve25519Point, _MontgomeryPoint) and issubclass(Curve448Point, _MontgomeryPoint)
    pt = d.Curve25519.point_type
    g = pt.generator_point()
    assert len(g.point_to_string()) == 64 and pt.string_to_point(g.point_to_string()) == g and pt._IDENTITY_BYTES == b"\xff" * 64
    assert pt._trusted((1 << 256) - 1, (1 << 256) - 1).is_identity() and (g + (-g)).is_identity() and (g + g) - g == g
    with pytest.raises(ValueError, match="Invalid point length: expected 64, got 63"):
        pt.string_to_point(bytes(63))
    assert g == d.Curve25519_NU.point_type.generator_point()


def test_exported_symbols_and_enum():
    names = ["dr_curve448_hash_to_field_batch", "dr_curve448_map_to_curve", "dr_curve448_encode_to_curve_batch",
             "dr_curve448_scalar_mul_batch", "dr_curve448_msm_groups", "dr_curve448_decode_points", "dr_curve448_law_selftest"]
    lib = _native.lib()
    for name in names:
        assert name in _native.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert not any(s.startswith("dr_curve448") for s in _native.EXPORTED_SYMBOLS if s not in names)      # no field selftest, no flag-byte calls
    with open(os.path.join(ROOT, "include", "dotring_hip.h")) as f:
        header = f.read()
    declared = re.findall(r"DR_API\s+[\w\s\*]+?\b(dr_\w+)\s*\(", header)
    assert sorted(declared) == sorted(_native.EXPORTED_SYMBOLS)
    assert "DR_CURVE_CURVE448_RO = 21, DR_CURVE_CURVE448_NU = 22" in header
    for call in ("map_to_curve", "encode_to_curve_batch", "scalar_mul_batch", "msm_groups", "decode_points"):
        assert callable(getattr(_native.Context, "curve448_" + call))


@pytest.mark.parametrize("count", [2, 1])
def test_host_hash_to_field(golden_dir, count):
    cv = d.Curve448_RO if count == 2 else d.Curve448_NU
    cid = cv.curve.params.curve_id
    dst = c.DST_RO if count == 2 else c.DST_NU
    doc = _vectors(golden_dir, "curve448_ro.json" if count == 2 else "curve448_nu.json")
    msgs = [v["msg"].encode() for v in doc["vectors"]]
    raw = _native.curve448_hash_to_field_batch(cid, msgs)
    assert raw == b"".join(int(u, 16).to_bytes(56, "little") for v in doc["vectors"] for u in v["u"])
    rng = random.Random(448)
    msgs = [rng.randbytes(n) for n in (0, 1, 83, 217, 300)]
    salts = [rng.randbytes(1 + n) for n in range(5)]
    want = b"".join(u.to_bytes(56, "little") for m, s in zip(msgs, salts) for u in c.hash_to_field(s + m, count, dst))
    assert cv.point_type.hash_to_field_pairs(msgs, salts) == want
    assert raw != _native.ed448_hash_to_field_batch(19 if count == 2 else 20, [v["msg"].encode() for v in doc["vectors"]])   # its own DST
    for bad in (0, 13, 19, 20, 23):
        with pytest.raises(ValueError):
            _native.curve448_hash_to_field_batch(bad, [b"x"])
    for bad in (21, 22):
        with pytest.raises(ValueError):
            _native.ed448_hash_to_field_batch(bad, [b"x"])
        with pytest.raises(ValueError):
            _native.blsg1_hash_to_field_batch(bad, [b"x"])


# ---------------------------------------------------------------- the restatement's VRF layer, pinned on vectors the reference holds
def test_xof_suite_reproduces_the_bandersnatch_shake128_files(golden_dir):
    from oracle.pyref import bandersnatch as bsn

    assert type(c.RO) is e4.XofSuite and type(c.NU) is e4.XofSuite
    s128 = bsn.SHAKE128
    with bsn.using(s128):
        suite = type(c.RO)(s128.suite_id, bsn.N, bsn.G, s128.blinding_base, bsn.add, bsn.enc_point,
                           lambda data: bsn.encode_to_curve(s128, data), hashlib.shake_128, bsn.IDENTITY)

        def load(kind):
            with open(os.path.join(golden_dir, "dot-ring", f"bandersnatch_shake128_ell2_{kind}.json")) as f:
                return json.load(f)

        for v in load("tiny"):
            sk, al, ad = (bytes.fromhex(v[k]) for k in ("sk", "alpha", "ad"))
            assert suite.ietf_prove(sk, al, ad).hex() == v["gamma"] + v["proof_c"] + v["proof_s"]
        for v in load("thin"):
            sk, al, ad = (bytes.fromhex(v[k]) for k in ("sk", "alpha", "ad"))
            assert suite.ietf_prove(sk, al, ad, thin=True).hex() == v["gamma"] + v["proof_r"] + v["proof_s"]
        for v in load("pedersen"):
            sk, al, ad = (bytes.fromhex(v[k]) for k in ("sk", "alpha", "ad"))
            proof, blinding = suite.pedersen_prove(sk, al, ad)
            assert proof.hex() == v["gamma"] + v["proof_pk_com"] + v["proof_r"] + v["proof_ok"] + v["proof_s"] + v["proof_sb"]
            assert suite.enc_scalar(blinding).hex() == v["blinding"]


def test_restatement_vrf_layer_is_self_consistent(golden_dir):
    """a Curve448 proof of the restatement verifies under the restatement's own verifier; the lengths follow from the widths: 112-byte
    points, 56-byte scalars and the 16-byte challenge the reference's VRF layer squeezes for every suite"""
    with open(os.path.join(golden_dir, "base", "curve448_base_vectors.json")) as f:
        base = json.load(f)
    assert all(v["gamma"] == v["proof_c"] == v["proof_s"] == v["beta"] == "" for v in base)      # the reference holds no proof bytes
    sk, alpha, ad = bytes.fromhex(base[0]["sk"]), bytes.fromhex(base[0]["alpha"]), b"ad"
    pk = c.raw(c.mul(int.from_bytes(sk, "little") % N, c.G))
    tiny, thin, ped = c.RO.ietf_prove(sk, alpha, ad), c.RO.ietf_prove(sk, alpha, ad, thin=True), c.RO.pedersen_prove(sk, alpha, ad)[0]
    assert (len(tiny), len(thin), len(ped)) == (112 + 16 + 56, 112 + 112 + 56, 4 * 112 + 2 * 56)
    assert c.ietf_verify(c.RO, pk, tiny, alpha, ad) and c.ietf_verify(c.RO, pk, thin, alpha, ad, thin=True) and c.pedersen_verify(c.RO, ped, alpha, ad)
    assert not c.ietf_verify(c.RO, pk, tiny, alpha + b"x", ad) and not c.ietf_verify(c.RO, pk, thin, alpha, ad + b"x", thin=True)
    assert not c.pedersen_verify(c.RO, ped, alpha, b"")
