"""Ed448_RO / Ed448_NU without a GPU: the big-integer restatement (ed448_ref.py) against every string of the reference's two RFC 9380
vector files, the facts the kernels rely on (the group order, the three inputs without an image and why there are no others, the images
of order 4), the library's host hash_to_field against vectors and restatement, every limb constant of the new headers recomputed from
its integer, the host build of fe448.hip.h under -fsanitize=undefined at the limb bounds of its contract, the Python point type on the
host, and the pin of the restatement's XOF / scalar-width / nonce-width changes on the reference's Bandersnatch SHAKE128 proof files."""
import hashlib
import json
import os
import random
import re
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ed448_ref as e  # noqa: E402

import dot_ring_amd as d  # noqa: E402
from dot_ring_amd import _native  # noqa: E402
from dot_ring_amd.vrf.codec import point_len, scalar_len  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dot_ring_amd", "csrc")
P, N = e.P, e.N
HEX112 = re.compile(r"^[0-9a-f]{112}$")


def _vectors(golden_dir, name):
    with open(os.path.join(golden_dir, "h2c", name)) as f:
        return json.load(f)


def _num(s, seen):
    assert HEX112.match(s), s           # a well-formed 448-bit number
    seen.append(s)
    return int(s, 16)


# ---------------------------------------------------------------- the restatement against the reference's vectors
def test_restatement_reproduces_all_65_strings(golden_dir):
    seen = []
    for name, nu in (("ed448_ro.json", False), ("ed448_nu.json", True)):
        doc = _vectors(golden_dir, name)
        dst = doc["dst"].encode()
        assert dst == (e.DST_NU if nu else e.DST_RO) and doc["suite"].encode() == dst[len(b"QUUX-V01-CS02-with-"):]
        assert len(doc["vectors"]) == 5
        for v in doc["vectors"]:
            msg = v["msg"].encode()
            us = e.hash_to_field(msg, 1 if nu else 2, dst)
            assert [_num(u, seen) for u in v["u"]] == us
            images = [e.map_to_curve(u) for u in us]
            for key, img in zip(("Q",) if nu else ("Q0", "Q1"), images):
                assert (_num(v[key]["x"], seen), _num(v[key]["y"], seen)) == img
            pt = (e.encode_to_curve_nu if nu else e.encode_to_curve_ro)(msg)
            assert (_num(v["P"]["x"], seen), _num(v["P"]["y"], seen)) == pt
            assert pt != e.O and e.mul(N, pt) == e.O
    assert len(seen) == 65
    assert e.DST_NU == e.DST_RO.replace(b"_RO_", b"_NU_")


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


def test_group_order_is_4n():
    assert e.on_curve(e.G) and e.mul(N, e.G) == e.O and e.G != e.O
    assert _is_probable_prime(N) and _is_probable_prime(P) and P % 4 == 3
    assert pow(e.D, (P - 1) // 2, P) == P - 1                   # d is a non-square: the addition is complete
    # a point of order 4, so 4 | #E; n | #E by G; 4 n is the only multiple of 4 n within Hasse's interval (its width 4 sqrt(p) < 4 n)
    assert e.on_curve((1, 0)) and e.add((1, 0), (1, 0)) == (0, P - 1) and e.mul(4, (1, 0)) == e.O
    assert (P + 1 - 4 * N) ** 2 <= 4 * P and (4 * N) ** 2 > 16 * P
    pt = e.add(e.mul(7, e.G), (1, 0))                            # a point of order 4 n
    assert e.on_curve(pt) and e.mul(N, pt) != e.O and e.mul(2 * N, pt) != e.O and e.mul(4 * N, pt) == e.O


# ---------------------------------------------------------------- the map's inputs without a value
def _polmulmod(a, b, f):
    """a b mod f over F_p; polynomials as coefficient lists, low degree first; f monic"""
    out = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            out[i + j] = (out[i + j] + x * y) % P
    n = len(f) - 1
    for k in range(len(out) - 1, n - 1, -1):
        c = out[k]
        if c:
            for j in range(n + 1):
                out[k - n + j] = (out[k - n + j] - c * f[j]) % P
    return (out + [0] * n)[:n]


def _polgcd_degree(a, b):
    def trim(q):
        q = list(q)
        while q and q[-1] == 0:
            q.pop()
        return q
    a, b = trim(a), trim(b)
    while b:
        inv = pow(b[-1], -1, P)
        while len(a) >= len(b):
            c = a[-1] * inv % P
            sh = len(a) - len(b)
            a = trim([(x - c * b[i - sh]) % P if i >= sh else x for i, x in enumerate(a)])
            if not a:
                break
        a, b = b, a
    return len(a) - 1


def _roots_in_fp(f):
    """degree of gcd(x^p - x, f): the number of distinct roots of f in F_p"""
    x, acc = [0, 1, 0, 0], [1, 0, 0, 0]
    for bit in bin(P)[2:]:
        acc = _polmulmod(acc, acc, f)
        if bit == "1":
            acc = _polmulmod(acc, x, f)
    acc[1] = (acc[1] - 1) % P
    return _polgcd_degree(f, acc)


def test_three_inputs_have_no_image_and_no_others_can():
    a = e.MONT_A
    for u in (0, 1, P - 1):
        s, t = e.ell2_mont(u)
        assert (s, t) == (0, 0)                                 # -A is a non-square: x2 = 0, the Montgomery point of order 2
        xn, xd, yn, yd = e.mont_to_edwards_fractions(s, t)
        assert yd == 0 and xd != 0
        with pytest.raises(ValueError, match="Point is not on the curve"):
            e.map_to_curve(u)
    assert pow(-a % P, (P - 1) // 2, P) == P - 1
    # on the curve v^2 = u^3 + A u^2 + u:  x_den = u^4 + 4 u^3 + (4 A - 2) u^2 + 4 u + 1,  y_den = u (-u^4 - 2 A u^3 - 6 u^2 - 2 A u - 1)
    rng = random.Random(448)
    for _ in range(20):
        s, t = e.ell2_mont(rng.randrange(P))
        xn, xd, yn, yd = e.mont_to_edwards_fractions(s, t)
        assert xd == (s**4 + 4 * s**3 + (4 * a - 2) * s * s + 4 * s + 1) % P
        assert yd == s * (-s**4 - 2 * a * s**3 - 6 * s * s - 2 * a * s - 1) % P
    assert _roots_in_fp([1, 4, (4 * a - 2) % P, 4, 1]) == 0
    assert _roots_in_fp([1, 2 * a, 6, 2 * a, 1]) == 0            # (the y quartic, negated: monic)
    assert _roots_in_fp([(-1) % P, 0, 0, 0, 1]) == 2             # (the helper on a quartic with known roots) x^4 - 1: +-1 only, p = 3 mod 4


def test_no_input_reaches_montgomery_x_plus_minus_one():
    """The Montgomery points with x = +-1 would be the images of order 4.  x = 1 is not the x of a point (A + 2 is a non-square), and
    the two points with x = -1 are reached by no u: both routes of Elligator 2 ask for u^2 = 1 - A or 1 / (1 - A), non-squares.  So the
    map never sees them — and every image lies in the prime-order subgroup, the 4-isogeny from curve448 having a kernel of order 4.  The
    rational map itself sends them to (0, +-1), which has no zero denominator."""
    a = e.MONT_A
    assert e.sqrt(a + 2) is None and e.sqrt(a - 2) is not None
    for target in (1, P - 1):
        for x1 in (target, (-target - a) % P):                  # x = x1, or x = x2 = -x1 - A
            u2 = (1 + a * pow(x1, -1, P)) % P                   # x1 = -A / (1 - u^2)
            u = e.sqrt(u2)
            assert u is None or e.ell2_mont(u)[0] != target
    assert e.sqrt(1 - a) is None
    v = e.sqrt(a - 2)
    xn, xd, yn, yd = e.mont_to_edwards_fractions(P - 1, v)
    assert xd != 0 and yd != 0 and xn == 0 and yn * pow(yd, -1, P) % P in (1, P - 1)
    rng = random.Random(4)
    for _ in range(6):
        img = e.map_to_curve(rng.randrange(2, P - 1))
        assert e.mul(N, img) == e.O


# ---------------------------------------------------------------- the library's host hash_to_field
LENGTHS = (0, 1, 517, 81, 82, 83, 217, 218, 219)


@pytest.mark.parametrize("variant,count", [("RO", 2), ("NU", 1)])
def test_host_hash_to_field(golden_dir, variant, count):
    cv = d.Ed448_RO if count == 2 else d.Ed448_NU
    cid = _native.CURVE_ED448_RO if count == 2 else _native.CURVE_ED448_NU
    dst = e.DST_RO if count == 2 else e.DST_NU
    doc = _vectors(golden_dir, "ed448_ro.json" if count == 2 else "ed448_nu.json")
    msgs = [v["msg"].encode() for v in doc["vectors"]]
    raw = _native.ed448_hash_to_field_batch(cid, msgs)
    assert len(raw) == 56 * count * len(msgs)
    for i, v in enumerate(doc["vectors"]):
        for j, u in enumerate(v["u"]):
            assert int.from_bytes(raw[56 * (count * i + j) : 56 * (count * i + j + 1)], "little") == int(u, 16)
    rng = random.Random(9380)
    msgs = [rng.randbytes(n) for n in LENGTHS]
    want = b"".join(u.to_bytes(56, "little") for m in msgs for u in e.hash_to_field(m, count, dst))
    assert _native.ed448_hash_to_field_batch(cid, msgs) == want
    assert cv.point_type.hash_to_field_pairs(msgs) == want
    salts = [rng.randbytes(1 + n % 40) for n in LENGTHS]
    want = b"".join(u.to_bytes(56, "little") for m, s in zip(msgs, salts) for u in e.hash_to_field(s + m, count, dst))
    assert cv.point_type.hash_to_field_pairs(msgs, salts) == want
    assert _native.ed448_hash_to_field_batch(cid, []) == b""
    for bad in (0, 10, 15, 17, 18, 21):
        with pytest.raises(ValueError):
            _native.ed448_hash_to_field_batch(bad, [b"x"])


# ---------------------------------------------------------------- constants of the headers
def _array(text, name):
    m = re.search(name + r"\[[^\]]*\]\s*=\s*\{([^}]*)\}", text)
    assert m, name
    return [int(tok.strip().rstrip("u"), 16) for tok in m.group(1).split(",")]


def test_header_constants():
    with open(os.path.join(CSRC, "fe448.hip.h")) as f:
        fe = f.read()
    with open(os.path.join(CSRC, "kernels_ed448.hip.h")) as f:
        kn = f.read()
    p17 = _array(fe, "P17")
    assert len(p17) == 17 and p17[16] == 0 and sum(v << (28 * i) for i, v in enumerate(p17)) == P and all(v < 1 << 28 for v in p17)
    assert (-pow(P, -1, 1 << 28)) % (1 << 28) == 1                                   # the n0 passed to inv_divsteps
    assert int(re.search(r"EDWARDS_D_NEG = (\d+)", fe).group(1)) == (-e.D) % P == 39081
    assert int(re.search(r"MONT_A = (\d+)", fe).group(1)) == e.MONT_A
    batches = int(re.search(r"F448_DIVSTEP_BATCHES = (\d+)", fe).group(1))
    steps = (49 * 448 + 57) // 17
    assert batches * 28 >= steps > (batches - 1) * 28 and (batches // 2 + 1) < 32    # |out| < 24 p: fits the seventeenth limb
    assert int(re.search(r"L448 = (\d+)", fe).group(1)) * 28 == 448 and int(re.search(r"W448 = (\d+)", fe).group(1)) * 32 == 448
    order = _array(kn, "E448_ORDER")
    assert len(order) == 14 and sum(v << (32 * i) for i, v in enumerate(order)) == N
    assert int(re.search(r"E448_WINDOWS = (\d+)", kn).group(1)) == 448 // 4 + 1
    # the exponent of the chain in f448_pow_p34 and what the roots make of it
    assert (P - 3) // 4 == 2**446 - 2**222 - 1 == ((2**223 - 1) << 223) + 2**222 - 1 and (P + 1) // 4 == (P - 3) // 4 + 1
    # the accumulator budget: output column 8 collects 9 + 15 + 2 x 7 products
    assert 38 * 3 * (2**28 + 2**10) ** 2 + 2**40 < 2**63 and 38 * 4 * (2**28) ** 2 > 2**63
    # LDS: 8 entries x 3 coordinates x 16 limb words x 64 lanes x 4 bytes
    assert 8 * 3 * 16 * 64 * 4 == 98304 <= 163840


# ---------------------------------------------------------------- fe448.hip.h on the host, under the undefined-behaviour sanitizer
@pytest.fixture(scope="module")
def field_checker(tmp_path_factory):
    exe = tmp_path_factory.mktemp("ed448") / "ed448_field_host_check"
    # (-std=c++20: divstep28.hip.h shifts negative values left, which is defined from C++20 on; signed overflow stays undefined)
    subprocess.run(["g++", "-O2", "-std=c++20", "-fsanitize=undefined", "-fno-sanitize-recover", "-I", CSRC,
                    os.path.join(ROOT, "tests", "native", "ed448_field_host_check.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def _val(limbs):
    return sum(x << (28 * i) for i, x in enumerate(limbs))


NORMAL = 2**28 + 2**10


def _images(bound, rng, extra=12):
    yield [bound] * 16
    yield [-bound] * 16
    yield [bound if i % 2 else -bound for i in range(16)]
    yield [-bound if i % 2 else bound for i in range(16)]
    for _ in range(extra):
        yield [rng.randint(-bound, bound) for _ in range(16)]


def test_field_on_the_host_at_the_contract_bounds(field_checker):
    rng = random.Random(448)
    lines, want = [], []

    def ask(op, *operands):
        lines.append(op + " " + " ".join(str(x) for limbs in operands for x in limbs))

    for ka, kb in ((1, 3), (3, 1), (2, 1.5), (1.5, 2), (1, 1)):           # every split of the product's budget ka kb <= 3
        for a in _images(int(ka * NORMAL), rng):
            for b in _images(int(kb * NORMAL), rng, extra=2):
                ask("mul", a, b)
                want.append(_val(a) * _val(b) % P)
    for a in _images(int(1.7 * NORMAL), rng):
        ask("sqr", a)
        want.append(_val(a) ** 2 % P)
    for a in _images(2**31 - 2**5 - 1, rng):
        ask("carry", a)
        want.append(("carry", _val(a) % P))
        ask("pack", a)
        want.append(_val(a) % P)
    for a in _images(2**30, rng):
        ask("small39081", a)
        want.append(_val(a) * 39081 % P)
        ask("small156326", a)
        want.append(_val(a) * 156326 % P)
    for a in _images(NORMAL, rng):
        ask("inv", a)
        want.append(pow(_val(a) % P, P - 2, P))
        ask("sqrt", a)
        want.append(("sqrt", _val(a) % P))
        ask("p34", a)
        want.append(pow(_val(a) % P, (P - 3) // 4, P))
    for v in (0, 1, 2, P - 1, P, P + 1, 2**448 - 1, 2**224, 2**224 + 1):  # canonical and non-canonical values below 2^448
        a = [(v >> (28 * i)) & (2**28 - 1) for i in range(16)]
        ask("pack", a)
        want.append(v % P)
        ask("inv", a)
        want.append(pow(v % P, P - 2, P))
        ask("sqrt", a)
        want.append(("sqrt", v % P))
    run = subprocess.run([field_checker], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]                         # (a column overflow aborts the program)
    rows = run.stdout.strip().splitlines()
    assert len(rows) == len(lines)
    for line, row, w in zip(lines, rows, want):
        fields = row.split()
        got = int(fields[0], 16)
        assert len(fields[0]) == 112 and got < P, line[:60]
        if isinstance(w, tuple) and w[0] == "sqrt":
            square = pow(w[1], (P - 1) // 2, P) in (0, 1)
            assert int(fields[1]) == square and got == pow(w[1], (P + 1) // 4, P), line[:60]
            assert not square or got * got % P == w[1]
        elif isinstance(w, tuple):
            assert got == w[1], line[:60]
            assert all(-(2**10) < int(x) < 2**28 + 2**10 for x in fields[1:]) and len(fields) == 17     # carry() returns a normal value
        else:
            assert got == w, line[:60]


# ---------------------------------------------------------------- the Python point type on the host
def test_names_and_parameters():
    assert d.Ed448 is d.Ed448_RO and d.Ed448_NU is not d.Ed448_RO
    assert {"Ed448", "Ed448_RO", "Ed448_NU"} <= set(d.__all__)
    for cv, cid, e2c in ((d.Ed448_RO, 19, "ell2"), (d.Ed448_NU, 20, "ell2_nu")):
        sp = cv.curve.params
        assert sp.suite_id == e.SUITE_ID and sp.hash_fn is hashlib.shake_256 and sp.xof and sp.cofactor == 4
        assert sp.curve_id == cid == cv.point_type._CV and sp.e2c == e2c
        assert sp.field_modulus == P and sp.subgroup_order == N and sp.generator == e.G and sp.a == 1 and sp.d % P == e.D
        assert sp.auxiliary_points.blinding_base == e.G and not sp.auxiliary_points.accumulator_base and not sp.auxiliary_points.padding_point
        assert sp.encoding.point_len == 56 and sp.encoding.uncompressed and sp.encoding.challenge_len == 64
        assert point_len(cv) == 112 and scalar_len(cv) == 56
        assert (N.bit_length() + 128 + 7) // 8 == 72
        assert d.PedersenVRF[cv].proof_len() == 560
        assert d.TinyVRF[cv].cv is cv and d.ThinVRF[cv].cv is cv
        with pytest.raises(ValueError):
            d.RingVRF[cv]
        with pytest.raises(ValueError):
            d.RingProofParams(cv=cv)
    assert (_native.CURVE_ED448_RO, _native.CURVE_ED448_NU) == (19, 20)


def test_point_codec_and_group_on_the_host():
    pt = d.Ed448.point_type
    g = pt.generator_point()
    assert (g.x, g.y) == e.G and g.is_on_curve() and not g.is_identity()
    o = pt.identity()
    assert (o.x, o.y) == (0, 1) and o.is_identity() and o.is_on_curve()
    two = g + g
    assert (two.x, two.y) == e.add(e.G, e.G) and g.double() == two and two - g == g and (-g).x == P - g.x and g + (-g) == o and g + o == g
    three = two + g
    assert (three.x, three.y) == e.mul(3, e.G)
    raw = g.point_to_string()
    assert raw == e.raw(e.G) and len(raw) == 112 and pt.string_to_point(raw) == g and pt.string_to_point(raw.hex()) == g
    assert pt.string_to_point(e.raw(e.O)) == o
    with pytest.raises(ValueError, match="Point is not on the curve"):
        pt.string_to_point(e.raw((1, 1)))
    with pytest.raises(ValueError, match="Invalid point coordinates"):
        pt.string_to_point(e.raw((P, 1)))
    with pytest.raises(ValueError, match="Point is not on the curve"):
        pt(0, 0)
    q = pt(1, 0)                                                            # a point of order 4
    assert q + pt(P - 1, 0) == o and q + pt(0, P - 1) == pt(P - 1, 0) and d.Ed448.point(g) is g and d.Ed448.point(*e.G) == g
    assert q.double() == o                       # te_affine_point.py:149: the reference's doubling gives the identity where y = 0
    cleared = pt(*e.map_to_curve(7)).clear_cofactor()
    assert (cleared.x, cleared.y) == e.clear_cofactor(e.map_to_curve(7))
    assert d.Ed448_NU.point_type is not pt


def test_exported_symbols():
    names = ["dr_ed448_hash_to_field_batch", "dr_ed448_map_to_curve", "dr_ed448_encode_to_curve_batch", "dr_ed448_scalar_mul_batch",
             "dr_ed448_msm_groups", "dr_ed448_decode_points", "dr_ed448_field_selftest"]
    lib = _native.lib()
    for name in names:
        assert name in _native.EXPORTED_SYMBOLS and hasattr(lib, name)
    with open(os.path.join(ROOT, "include", "dotring_hip.h")) as f:
        header = f.read()
    declared = re.findall(r"DR_API\s+[\w\s\*]+?\b(dr_\w+)\s*\(", header)
    assert sorted(declared) == sorted(_native.EXPORTED_SYMBOLS)
    assert "DR_CURVE_ED448_RO = 19, DR_CURVE_ED448_NU = 20" in header


# ---------------------------------------------------------------- the restatement's VRF layer, pinned on vectors the reference holds
def test_xof_suite_reproduces_the_bandersnatch_shake128_files(golden_dir):
    from oracle.pyref import bandersnatch as bsn

    s128 = bsn.SHAKE128
    with bsn.using(s128):
        suite = e.XofSuite(s128.suite_id, bsn.N, bsn.G, s128.blinding_base, bsn.add, bsn.enc_point,
                           lambda data: bsn.encode_to_curve(s128, data), hashlib.shake_128, bsn.IDENTITY)
        assert suite.scalar_len == 32 and suite.nonce_len == 48

        def load(kind):
            with open(os.path.join(golden_dir, "dot-ring", f"bandersnatch_shake128_ell2_{kind}.json")) as f:
                return json.load(f)

        for v in load("tiny"):
            sk, al, ad = (bytes.fromhex(v[k]) for k in ("sk", "alpha", "ad"))
            assert suite.ietf_prove(sk, al, ad).hex() == v["gamma"] + v["proof_c"] + v["proof_s"]
            assert suite.point_to_hash(bsn.decompress(bytes.fromhex(v["gamma"]))).hex() == v["beta"][:64]
        for v in load("thin"):
            sk, al, ad = (bytes.fromhex(v[k]) for k in ("sk", "alpha", "ad"))
            assert suite.ietf_prove(sk, al, ad, thin=True).hex() == v["gamma"] + v["proof_r"] + v["proof_s"]
        for v in load("pedersen"):
            sk, al, ad = (bytes.fromhex(v[k]) for k in ("sk", "alpha", "ad"))
            proof, blinding = suite.pedersen_prove(sk, al, ad)
            assert proof.hex() == v["gamma"] + v["proof_pk_com"] + v["proof_r"] + v["proof_ok"] + v["proof_s"] + v["proof_sb"]
            assert suite.enc_scalar(blinding).hex() == v["blinding"]


def test_restatement_vrf_layer_is_self_consistent():
    """an Ed448 Tiny and Thin proof of the restatement verifies under the restatement's own verifier, with the stated lengths"""
    sk, alpha, ad = bytes(range(57)), b"test message", b"ad"
    pk = e.raw(e.mul(int.from_bytes(sk, "little") % N, e.G))
    tiny, thin = e.RO.ietf_prove(sk, alpha, ad), e.RO.ietf_prove(sk, alpha, ad, thin=True)
    assert len(tiny) == 184 and len(thin) == 280 and len(e.RO.pedersen_prove(sk, alpha, ad)[0]) == 560
    assert e.ietf_verify(e.RO, pk, tiny, alpha, ad) and e.ietf_verify(e.RO, pk, thin, alpha, ad, thin=True)
    assert not e.ietf_verify(e.RO, pk, tiny, alpha + b"x", ad) and not e.ietf_verify(e.RO, pk, thin, alpha, ad + b"x", thin=True)
