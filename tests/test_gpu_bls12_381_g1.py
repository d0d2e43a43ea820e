"""BLS12-381 G1 hashing on the GPU (DR_CURVE_BLS12_381_G1 = 15, DR_CURVE_BLS12_381_G1_NU = 16; csrc/kernels_g1_h2c.hip.h): what the
description adds to the device field at the limb bounds the map and the law feed, the map of RFC 9380 against the vector files and
the big-integer restatement (bls12_381_g1_ref.py), scalar multiplication and grouped MSMs on points inside and OUTSIDE G1 (E(Fq) has
order h r: a scalar reduced mod r would be wrong there), the SEC1 decoder with and without the subgroup check, the refusals, and the
other suites' bytes afterwards (the scalar-multiplication template is shared).  Shapes: n in {1, 64, 65} — a tail lane, a full wave,
a second workgroup — and one run of 300."""
import ctypes
import json
import os
import random
import struct
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bls12_381_g1_ref as g1  # noqa: E402
import secp256k1_ref as k1  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
P, R_ORDER = g1.P, g1.R_ORDER
RO, NU = 15, 16
R392 = 1 << 392
R392_INV = pow(R392, -1, P)
LENGTHS = (0, 1, 55, 56, 64, 119, 120, 517)
WELL_FORMED = 96


def _h2c(variant):
    return json.load(open(os.path.join(GOLDEN, "h2c", f"bls12_381_G1_{variant}.json")))["vectors"]


def _xy(v):
    return int(v["x"], 16), int(v["y"], 16)


def raw(pt):
    return bytes(96) if pt is None else pt[0].to_bytes(48, "little") + pt[1].to_bytes(48, "little")


def pts_of(blob):
    out = []
    for i in range(0, len(blob), 96):
        x, y = int.from_bytes(blob[i : i + 48], "little"), int.from_bytes(blob[i + 48 : i + 96], "little")
        out.append(None if x == 0 and y == 0 else (x, y))
    return out


def _us(us):
    return b"".join(u.to_bytes(48, "little") for u in us)


def _sc(ks):
    return b"".join(k.to_bytes(32, "little") for k in ks)


_CACHE = {}


def outside_point():
    """`Q` of an NU vector: a point of E(Fq) that is not in G1"""
    if "outside" not in _CACHE:
        q = g1.map_to_curve(int(_h2c("nu")[1]["u"][0], 16))
        assert q == _xy(_h2c("nu")[1]["Q"]) and g1.on_curve(q) and not g1.valid_point(q)
        _CACHE["outside"] = q
    return _CACHE["outside"]


def hashed_point():
    return _xy(_h2c("ro")[2]["P"])


def random_images():
    """300 field elements and their images, computed once"""
    if "images" not in _CACHE:
        rng = random.Random(12381)
        us = [rng.randrange(P) for _ in range(300)]
        _CACHE["images"] = (us, [g1.map_to_curve(u) for u in us])
    return _CACHE["images"]


# ---------------------------------------------------------------- field
def carried(v):
    """the carried limb image of the integer v: limbs 0..12 in [0, 2^28), the rest in the signed top limb"""
    return [(v >> (28 * i)) & 0xFFFFFFF for i in range(13)] + [v >> 364]


def _pack(rows):
    return b"".join(struct.pack("<14i", *row) for row in rows)


def _val(limbs):
    return sum(v << (28 * i) for i, v in enumerate(limbs))


def test_field_selftest_at_contract_bounds(ctx):
    """limb images at the bounds the map and the law feed: products (n), carried sums of two, carried values up to 24.3 p (the law's
    12 (X1 Z2 + X2 Z1)), and the negations of those; residues 0, 1, p - 1, squares and non-squares.  Expected values are big integers:
    a register image a stands for a 2^-392 mod p, and every record is the canonical value of that kind."""
    rng = random.Random(28)
    mont = lambda x: x * R392 % P  # noqa: E731
    residues = [0, 1, P - 1, 4, P - 4]
    for _ in range(12):
        x = rng.randrange(2, P)
        residues += [x * x % P, 11 * x * x % P]                                    # a square and a non-square (11 is none: -11 is one, -1 is not)
    assert pow(11, (P - 1) // 2, P) == P - 1
    A, B = [], []
    for x in residues:
        m = mont(x)
        wide = carried(mont(rng.randrange(P)) + rng.choice((23, -24)) * P)         # c24.3: the law's widest carried operand
        assert abs(_val(wide)) < 25 * P and all(0 <= w < 1 << 28 for w in wide[:13])
        for image in (carried(m),                                                  # n
                      carried(m + P) if m < P // 2 else carried(m - P),            # the ends of a normal value's range (-p/2, 1.5 p)
                      carried(m + 2 * P),                                          # a carried sum of two
                      [-w for w in carried((P - m) % P)],                          # a negated normal
                      [-w for w in carried((P - m) % P + 2 * P)]):                 # a negated carried sum of two
            assert _val(image) % P == m
            A.append(image)
            B.append(wide if len(A) % 2 else carried(mont(rng.randrange(P))))
    n = len(A)
    assert n > 128                                                                 # three workgroups, the last one partial
    out, flags = ctx.blsg1_field_selftest(_pack(A), _pack(B))
    assert len(out) == 240 * n and len(flags) == n
    squares = 0
    for i in range(n):
        rec = [int.from_bytes(out[240 * i + 48 * j : 240 * i + 48 * j + 48], "little") for j in range(5)]
        x, y = _val(A[i]) * R392_INV % P, _val(B[i]) * R392_INV % P
        root = pow(x, (P + 1) // 4, P)
        is_square = root * root % P == x
        squares += is_square
        assert rec[0] == pow(x, (P - 3) // 4, P), i
        assert rec[1] == (root if is_square else 0), i
        assert rec[2] == (x if i % 2 else y), i
        assert rec[3] == 12 * x % P, i
        assert rec[4] == 2 * x * y % P, i
        assert flags[i] == (1 if is_square else 0) | (2 if x & 1 else 0) | (4 if x == 0 else 0), i
    assert 40 < squares < n - 40


# ---------------------------------------------------------------- the map
def test_map_to_curve_vectors(ctx):
    ro, nu = _h2c("ro"), _h2c("nu")
    singles = [int(u, 16) for v in ro for u in v["u"]] + [int(v["u"][0], 16) for v in nu]
    fields = [v[q] for v in ro for q in ("Q0", "Q1")] + [v["Q"] for v in nu]
    out, ok = ctx.blsg1_map_to_curve(_us(singles), 1, clear=False)
    assert ok == b"\x01" * 15
    checked = 0
    for got, field in zip(pts_of(out), fields):                                    # (five of the 30 strings are malformed: test_bls12_381_g1_cpu.py)
        for coord, text in zip(got, (field["x"], field["y"])):
            if len(text) == WELL_FORMED and " " not in text:
                assert coord == int(text, 16)
                checked += 1
    assert checked == 25
    assert pts_of(out) == [g1.map_to_curve(u) for u in singles]
    out, ok = ctx.blsg1_map_to_curve(_us(singles[:10]), 2, clear=True)
    assert ok == b"\x01" * 5 and pts_of(out) == [_xy(v["P"]) for v in ro]
    out, ok = ctx.blsg1_map_to_curve(_us(singles[10:]), 1, clear=True)
    assert ok == b"\x01" * 5 and pts_of(out) == [_xy(v["P"]) for v in nu]


def test_map_to_curve_edges_and_random(ctx):
    s = g1.sqrt(-pow(g1.SSWU_Z, -1, P) % P)                                        # u^2 = -1 / Z: the tv2 = 0 branch besides u = 0
    assert s is not None
    edges = [0, 1, P - 1, s, P - s]
    out, ok = ctx.blsg1_map_to_curve(_us(edges), 1, clear=False)
    assert ok == b"\x01" * 5 and pts_of(out) == [g1.map_to_curve(u) for u in edges]
    u = 0x1234567
    pairs = [u, u, u, P - u, 0, 0, s, P - s]                                       # a doubling in the sum; a cancelling pair; ...
    for clear in (False, True):
        out, ok = ctx.blsg1_map_to_curve(_us(pairs), 2, clear=clear)
        want = [g1.map_sum(pairs[2 * i : 2 * i + 2], clear) for i in range(4)]
        assert ok == b"\x01" * 4 and pts_of(out) == want
        assert want[1] is None and out[96:192] == bytes(96)                        # u and -u: the identity, 96 zero bytes, ok = 1
        assert want[0] == (g1.clear_cofactor if clear else (lambda q: q))(g1.add(g1.map_to_curve(u), g1.map_to_curve(u)))
    us, images = random_images()
    for n in (1, 64, 65, 300):
        for clear in (False, True):
            out, ok = ctx.blsg1_map_to_curve(_us(us[:n]), 1, clear=clear)
            assert ok == b"\x01" * n
            assert pts_of(out) == [g1.clear_cofactor(q) if clear else q for q in images[:n]]
    for n in (1, 64, 65, 150):
        sums = [g1.add(images[2 * i], images[2 * i + 1]) for i in range(n)]
        for clear in (False, True):
            out, ok = ctx.blsg1_map_to_curve(_us(us[: 2 * n]), 2, clear=clear)
            assert ok == b"\x01" * n
            assert pts_of(out) == [g1.clear_cofactor(q) if clear else q for q in sums]
    for bad in (P, P + 1, (1 << 384) - 1):
        with pytest.raises(ValueError):
            ctx.blsg1_map_to_curve(_us([5, bad]), 1)
    # the kernel of the isogeny: elements whose SSWU image has a root of the denominators as its x (the reference's modular inverse
    # raises there) give ok = 0, alone and as either member of a pair, and leave their neighbours alone
    import dot_ring_amd as d

    kus = list(g1.KERNEL_US)
    mixed = [us[0], kus[0], us[1], kus[1], kus[2], us[2]]
    out, ok = ctx.blsg1_map_to_curve(_us(mixed), 1, clear=False)
    assert ok == bytes([1, 0, 1, 0, 0, 1])
    assert [pts_of(out)[i] for i in (0, 2, 5)] == images[:3]
    for clear in (False, True):
        out, ok = ctx.blsg1_map_to_curve(_us(mixed), 2, clear=clear)
        assert ok == bytes([0, 0, 0])
        out, ok = ctx.blsg1_map_to_curve(_us(kus + us[: 65 - len(kus)]), 1, clear=clear)
        assert ok == bytes([0] * len(kus) + [1] * (65 - len(kus)))
    for cv in (d.BLS12_381_G1_RO, d.BLS12_381_G1_NU):
        with pytest.raises(ValueError, match="not invertible"):
            cv.point_type.map_to_curve_simple_swu(kus[0])
        with pytest.raises(ValueError, match="not invertible"):
            cv.point_type.encode_to_curve_from_field(_us(kus[:2]))
    lib = __import__("dot_ring_amd")._native.lib()
    out_xy, flags = ctypes.create_string_buffer(192), ctypes.create_string_buffer(2)
    for per_item in (0, 3, -1):
        assert lib.dr_blsg1_map_to_curve(ctx.handle, bytes(288), 1, per_item, 1, out_xy, flags) == -1


def test_encode_to_curve_batch(ctx):
    import dot_ring_amd as d

    rng = random.Random(9380)
    for cv, variant, name, ref in ((d.BLS12_381_G1_RO, RO, "ro", g1.encode_to_curve_ro), (d.BLS12_381_G1_NU, NU, "nu", g1.encode_to_curve_nu)):
        vectors = _h2c(name)
        msgs = [v["msg"].encode() for v in vectors]
        assert pts_of(ctx.blsg1_encode_to_curve_batch(variant, msgs)) == [_xy(v["P"]) for v in vectors]
        msgs = [bytes(rng.randrange(256) for _ in range(length)) for length in LENGTHS for _ in range(2)]
        salts = [bytes(rng.randrange(256) for _ in range(32 * (i % 2))) for i in range(len(msgs))]
        want = [ref(s + m) for m, s in zip(msgs, salts)]
        assert pts_of(ctx.blsg1_encode_to_curve_batch(variant, msgs, salts)) == want
        point_type = cv.point_type
        batch = point_type.encode_to_curve_batch(msgs, salts)
        assert [(q.x, q.y) for q in batch] == want
        for i in (0, 3, 15):
            assert point_type.encode_to_curve(msgs[i], salts[i]) == batch[i]
        assert point_type.encode_to_curve_from_field(point_type.hash_to_field_pairs(msgs, salts)) == batch
        assert cv.curve.valid_point(batch[0]) and point_type.encode_to_curve_batch([]) == []
    q = d.BLS12_381_G1.point_type.map_to_curve_simple_swu(7)
    assert (q.x, q.y) == g1.map_to_curve(7) and not d.BLS12_381_G1.curve.valid_point(q)


# ---------------------------------------------------------------- the group
EDGE_SCALARS = (0, 1, 2, 8, R_ORDER - 1, R_ORDER, R_ORDER + 1, 1 << 255, (1 << 256) - 1)


def test_scalar_mul_edge_scalars(ctx):
    """every edge scalar on the generator, on a hashed point and on a point outside G1: there r Q is NOT the identity — the case that
    catches a reduction of the scalar modulo r"""
    outside = outside_point()
    terms = [(pt, k) for pt in (g1.G, hashed_point(), outside) for k in EDGE_SCALARS]
    want = [g1.mul(k, pt) for pt, k in terms]
    assert g1.mul(R_ORDER, g1.G) is None and g1.mul(R_ORDER, hashed_point()) is None and g1.mul(R_ORDER, outside) is not None
    for n in (1, len(terms)):
        got = ctx.blsg1_scalar_mul_batch(b"".join(raw(pt) for pt, _ in terms[:n]), _sc([k for _, k in terms[:n]]))
        assert pts_of(got) == want[:n]
    # a tail lane, a full wave, a second workgroup; identity inputs among them
    rng = random.Random(65)
    base = [g1.G, hashed_point(), outside, None]
    for n in (64, 65):
        pts = [base[i % 4] for i in range(n)]
        ks = [rng.randrange(1 << 256) for _ in range(n)]
        cache = _CACHE.setdefault("mul", {})
        exp = [cache.setdefault((i % 4, k), g1.mul(k, pt)) for i, (pt, k) in enumerate(zip(pts, ks))]
        assert pts_of(ctx.blsg1_scalar_mul_batch(b"".join(raw(pt) for pt in pts), _sc(ks))) == exp
    with pytest.raises(ValueError):
        ctx.blsg1_scalar_mul_batch(P.to_bytes(48, "little") + bytes(48), bytes(32))


def test_point_mul_python(ctx):
    import dot_ring_amd as d

    point_type = d.BLS12_381_G1.point_type
    mk = lambda pt: point_type.identity() if pt is None else point_type(*pt)  # noqa: E731
    gen, outside = point_type.generator_point(), mk(outside_point())
    rng = random.Random(192)
    order = g1.H * R_ORDER
    assert (gen * R_ORDER).is_identity() and not (outside * R_ORDER).is_identity()
    assert (outside * order).is_identity() and (gen * order).is_identity()
    for pt in (gen, outside):
        ref = (pt.x, pt.y)
        for k in (-1, -5, -(1 << 300) - 7, 1 << 256, (1 << 256) + 1, order - 1, order + 1, rng.randrange(1 << 256, 1 << 400)):
            assert pt * k == mk(g1.mul(k, ref)), k
        assert -5 * pt == -(pt * 5) and pt * 0 == point_type.identity()
        assert pt.clear_cofactor() == mk(g1.clear_cofactor(ref)) and d.BLS12_381_G1.curve.valid_point(pt.clear_cofactor())
    assert d.BLS12_381_G1.curve.valid_point(gen) and not d.BLS12_381_G1.curve.valid_point(outside)
    assert not d.BLS12_381_G1.curve.valid_point(point_type.identity())
    # the group properties the reference's test_curve_property_based asks
    ident = point_type.identity()
    p1, p2, p3 = gen * 5, gen * 7, outside
    a, b = rng.randrange(1, R_ORDER), rng.randrange(1, R_ORDER)
    assert p1 + ident == p1 and ident + p1 == p1 and p1 - p1 == ident and p1 + (-p1) == ident
    assert p1 + p2 == p2 + p1 == gen * 12 and (p1 + p2) + p3 == p1 + (p2 + p3)
    assert p3 * (a + b) == p3 * a + p3 * b and (p3 * a) * b == p3 * (a * b) and (p1 + p3) * a == p1 * a + p3 * a
    assert p3.double() == p3 + p3 == p3 * 2 and (p1 * a).is_on_curve() and gen * 1 == gen
    assert point_type.msm([p1, p3, ident], [a, -b, 5]) == p1 * a - p3 * b
    assert point_type.msm([], []) == ident
    # the module's batch helpers take these points too
    from dot_ring_amd.curve import msm_groups, scalar_mul_batch

    assert scalar_mul_batch([gen, outside], [5, R_ORDER]) == [gen * 5, outside * R_ORDER]
    assert scalar_mul_batch([gen, outside], [-5, 1 << 300]) == [gen * -5, outside * (1 << 300)]
    assert msm_groups([gen, outside, gen, outside], [1, 2, 3, 4], 2) == [gen + outside * 2, gen * 3 + outside * 4]
    with pytest.raises(ValueError):
        point_type.msm([p1], [1, 2])


def test_msm_groups(ctx):
    import dot_ring_amd as d

    rng = random.Random(64)
    outside, hashed = outside_point(), hashed_point()
    cache = _CACHE.setdefault("mul", {})
    base = [g1.G, hashed, outside, None, g1.neg(outside)]

    def term_sum(pts, ks):
        acc = None
        for pt, k in zip(pts, ks):
            acc = g1.add(acc, cache.setdefault((base.index(pt), k), g1.mul(k, pt)))
        return acc

    for m in (1, 2, 63, 64):
        groups = 3 if m < 63 else 2
        pts, ks = [], []
        for grp in range(groups):
            gp = [base[rng.randrange(4)] for _ in range(m)]
            gk = [rng.choice((0, 1, R_ORDER, rng.randrange(1 << 256), rng.randrange(1 << 64))) for _ in range(m)]
            if m >= 2 and grp == 0:                                                # coinciding terms
                gp[1], gk[1] = gp[0], gk[0]
            if m >= 2 and grp == 1:                                                # cancelling terms: k Q and k (-Q)
                gp[0], gp[1] = outside, g1.neg(outside)
                gk[0] = gk[1] = rng.randrange(1 << 256)
            pts += gp
            ks += gk
        got = pts_of(ctx.blsg1_msm_groups(b"".join(raw(pt) for pt in pts), _sc(ks), m))
        assert got == [term_sum(pts[grp * m : grp * m + m], ks[grp * m : grp * m + m]) for grp in range(groups)], m
    # all identities and all zero scalars
    assert pts_of(ctx.blsg1_msm_groups(bytes(96 * 4), _sc([5, 6, 7, 8]), 2)) == [None, None]
    assert pts_of(ctx.blsg1_msm_groups(raw(g1.G) * 4, bytes(32 * 4), 4)) == [None]
    # m = 65: the entry point refuses it, as the other grouped MSMs do; the Python msm folds in levels
    with pytest.raises(ValueError):
        ctx.blsg1_msm_groups(raw(g1.G) * 65, _sc([1] * 65), 65)
    with pytest.raises(ValueError):
        ctx.blsg1_msm_groups(raw(g1.G), _sc([1]), 0)
    point_type = d.BLS12_381_G1.point_type
    mk = lambda pt: point_type.identity() if pt is None else point_type(*pt)  # noqa: E731
    pts = [base[i % 4] for i in range(65)]
    ks = [rng.randrange(1 << 64) if i % 5 else rng.randrange(1 << 256) for i in range(65)]
    assert point_type.msm([mk(pt) for pt in pts], ks) == mk(term_sum(pts, ks))


# ---------------------------------------------------------------- decoding
def test_decode_points(ctx):
    import dot_ring_amd as d

    outside, hashed = outside_point(), hashed_point()
    rng = random.Random(49)
    x_bad = next(x for x in iter(lambda: rng.randrange(P), None) if g1.sqrt((x ** 3 + 4) % P) is None)
    good = [g1.G, g1.neg(g1.G), hashed, g1.neg(hashed)]
    assert {pt[1] & 1 for pt in good} == {0, 1}                                    # both parities
    on_curve = lambda x: g1.sqrt((x ** 3 + 4) % P) is not None  # noqa: E731
    cases = [(g1.sec1_encode(pt), pt, True) for pt in good]
    cases += [(g1.sec1_encode(pt), pt, False) for pt in (outside, g1.neg(outside))]          # on the curve, outside G1
    for prefix in (0x00, 0x01, 0x04, 0x05, 0x06, 0x07, 0x82, 0xFF):
        cases.append((bytes([prefix]) + g1.sec1_encode(g1.G)[1:], "bad", False))
    cases.append((b"\x02" + P.to_bytes(48, "big"), "bad", False))                  # x = p is refused although 0^3 + 4 is a square
    assert on_curve(0)
    xm = P - 1                                                                     # x = p - 1: whichever it is
    pm = g1.sec1_decode(b"\x03" + xm.to_bytes(48, "big"))
    cases.append((b"\x03" + xm.to_bytes(48, "big"), pm, pm != "bad" and g1.valid_point(pm)))
    cases.append((b"\x02" + x_bad.to_bytes(48, "big"), "bad", False))              # a non-residue
    cases.append((b"\x02" + ((1 << 384) - 1).to_bytes(48, "big"), "bad", False))
    for enc, want, _ in cases:
        assert g1.sec1_decode(enc) == want
    for n in (1, 64, 65):
        picks = [cases[i % len(cases)] for i in range(n)] if n > 1 else [cases[4]]
        blob = b"".join(enc for enc, _, _ in picks)
        for check in (False, True):
            out, ok = ctx.blsg1_decode_points(blob, check)
            accept = [want != "bad" and (in_g1 or not check) for _, want, in_g1 in picks]
            assert list(ok) == [1 if a else 0 for a in accept]
            assert pts_of(out) == [want if a else None for (_, want, _), a in zip(picks, accept)]
    assert not g1.valid_point(outside)
    point_type = d.BLS12_381_G1.point_type
    for pt in good + [outside]:
        obj = point_type(*pt)
        for compressed in (True, False):
            assert point_type.string_to_point(obj.point_to_string(compressed)) == obj
        assert obj.point_to_string() == g1.sec1_encode(pt)
    assert point_type.string_to_point(b"\x00").is_identity() and point_type.identity().point_to_string() == b"\x00"
    for enc, want, _ in cases:
        if want == "bad":
            with pytest.raises(ValueError):
                point_type.string_to_point(enc)
    assert d.BLS12_381_G1.curve.valid_point(point_type(*hashed)) and not d.BLS12_381_G1.curve.valid_point(point_type(*outside))


# ---------------------------------------------------------------- refusals
def test_refusals(ctx):
    """ids 15 and 16 on the 64-byte entry points — dr_te_*, hash_to_field / encode_to_curve, the Pedersen and IETF provers and
    verifiers, the ring prover's creation and the Ring-VRF prove / verify calls (single and multi, on a real Bandersnatch prover):
    DR_ERR_INVALID, for the curve id's sake; the VRF classes raise.  The dr_bsn_* entry points and their GLV paths take no curve id
    (they are Bandersnatch's), so there is nothing to refuse there."""
    import dot_ring_amd as d
    from dot_ring_amd import _native
    from dot_ring_amd.ring_proof.device_prover import get_device_prover

    lib = _native.lib()
    INVALID = _native.DR_ERR_INVALID
    off = (ctypes.c_uint64 * 2)(0, 1)
    buf = lambda n=512: ctypes.create_string_buffer(n)  # noqa: E731
    verdict = (ctypes.c_int * 1)()

    def refused(rc):
        assert rc == INVALID
        assert b"curve" in lib.dr_last_error()

    # a Bandersnatch ring prover of 8 keys, as smoke() builds it, for the calls that take a prover
    keys = [d.Bandersnatch.public_key_from_secret((500 + i).to_bytes(32, "little")) for i in range(8)]
    ring = d.Ring(keys, d.RingProofParams.from_ring_size(8, test_vectors=True))
    prover = get_device_prover(ring)
    provers, ctxs = (ctypes.c_void_p * 1)(prover.handle), (ctypes.c_void_p * 1)(ctx.handle)
    vk = _native.RingVerifierKeyStruct()
    vk.log2n, vk.fs_prefix, vk.fs_prefix_len = 9, b"x", 1
    index, ok = (ctypes.c_uint32 * 1)(0), ctypes.c_int(0)
    for cid in (RO, NU):
        refused(lib.dr_te_scalar_mul_batch(ctx.handle, cid, bytes(64), bytes(32), 1, buf()))
        refused(lib.dr_te_msm(ctx.handle, cid, bytes(64), bytes(32), 1, buf()))
        refused(lib.dr_te_msm_groups(ctx.handle, cid, bytes(64), bytes(32), 1, 1, buf()))
        refused(lib.dr_te_decode_points(ctx.handle, cid, bytes(64), 1, buf(), buf()))
        refused(lib.dr_te_fixed_base_msm_groups(ctx.handle, cid, bytes(64), 1, bytes(32), 1, buf()))
        made = ctypes.c_void_p()
        assert lib.dr_ring_prover_create_te(ctx.handle, cid, None, 9, 8, bytes(64), bytes(64), bytes(64), bytes(64), ctypes.byref(made)) == INVALID
        assert not made.value
        for xof in (0, 2):
            suite = _native.vrf_suite(b"BLS12381G1_XMD:SHA-256_SSWU_RO_", xof, bytes(64), bytes(64), cid)
            s = ctypes.byref(suite)
            refused(lib.dr_hash_to_field_batch(s, b"a", off, 1, buf()))
            refused(lib.dr_encode_to_curve_batch(ctx.handle, s, b"a", off, None, None, 1, buf()))
            refused(lib.dr_pedersen_prove_batch(ctx.handle, s, 1, b"a", off, b"a", off, b"a", off, bytes(32), buf(), buf()))
            refused(lib.dr_pedersen_verify_batch(ctx.handle, s, 1, bytes(512), bytes(64), off, b"a", off, b"a", off, verdict))
            for thin in (0, 1):
                refused(lib.dr_ietf_prove_batch(ctx.handle, s, thin, 1, b"a", off, b"a", off, b"a", off, bytes(32), buf(), buf()))
                refused(lib.dr_ietf_verify_batch(ctx.handle, s, thin, 1, bytes(512), bytes(64), b"a", off, b"a", off, b"a", off, buf()))
            refused(lib.dr_ringvrf_verify_batch(ctx.handle, s, ctypes.byref(vk), 1, bytes(784), b"a", off, b"a", off, None, None, bytes(32),
                                                ctypes.byref(ok)))
            refused(lib.dr_ringvrf_verify_batch_multi(ctxs, 1, s, ctypes.byref(vk), 1, bytes(784), b"a", off, b"a", off, None, None, bytes(32),
                                                      ctypes.byref(ok)))
            refused(lib.dr_ringvrf_prove_batch(prover.handle, s, 1, b"a", off, b"a", off, None, None, bytes(32), index, b"x", 1, None, buf(1024),
                                               buf(1024)))
            refused(lib.dr_ringvrf_prove_batch_multi(provers, 1, s, 1, b"a", off, b"a", off, None, None, bytes(32), index, b"x", 1, None,
                                                     buf(1024), buf(1024)))
            assert ok.value == 0
    # the library's own calls take no other curve's data: 64-byte points are not 96-byte points
    with pytest.raises(ValueError):
        ctx.blsg1_scalar_mul_batch(bytes(64), bytes(32))
    with pytest.raises(ValueError):
        ctx.blsg1_decode_points(bytes(33), False)
    for cv in (d.BLS12_381_G1_RO, d.BLS12_381_G1_NU):
        for scheme in (d.TinyVRF, d.ThinVRF, d.PedersenVRF, d.RingVRF):
            with pytest.raises(ValueError, match="no key or proof of it can be decoded"):
                scheme[cv]
        with pytest.raises(ValueError):
            d.RingProofParams(cv=cv)


def test_other_suites_after_g1_calls(ctx):
    """the scalar-multiplication template is shared: after G1 calls on this context a secp256k1 proof still has the restatement's bytes
    and an Ed25519 proof the vector file's"""
    import dot_ring_amd as d

    ctx.blsg1_scalar_mul_batch(raw(g1.G) * 65, _sc([(1 << 256) - 1] * 65))
    ctx.blsg1_map_to_curve(_us([1, 2]), 2)
    d.BLS12_381_G1.point_type.generator_point() * 5
    sk, al, ad = (7).to_bytes(32, "little"), b"after g1", b"ad"
    assert d.TinyVRF[d.Secp256k1].prove(al, sk, ad).encode() == k1.RO.ietf_prove(sk, al, ad)
    v = json.load(open(os.path.join(GOLDEN, "dot-ring", "ed25519_sha-512_tai_tiny.json")))[0]
    proof = d.TinyVRF[d.Ed25519].prove(bytes.fromhex(v["alpha"]), bytes.fromhex(v["sk"]), bytes.fromhex(v["ad"]))
    assert proof.encode() == b"".join(bytes.fromhex(v[f]) for f in ("gamma", "proof_c", "proof_s"))
