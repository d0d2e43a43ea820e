"""BLS12-381 G2 hashing on the GPU (DR_CURVE_BLS12_381_G2 = 17, DR_CURVE_BLS12_381_G2_NU = 18; csrc/fq2_28.hip.h and
csrc/kernels_g2_h2c.hip.h): the device Fq2 at the limb bounds the map and the law feed, the map of RFC 9380 against the vector files and
the big-integer restatement (bls12_381_g2_ref.py), the clearing by psi against the multiplication by h_eff, scalar multiplication by
768-bit scalars on points inside and OUTSIDE G2 (E(Fq2) has order h2 r: a scalar reduced mod r would be wrong there), the curve and
subgroup check, the refusals, and a G1 hash and a secp256k1 proof afterwards (the chain of (p - 3) / 4 is shared with the G1 unit).
Shapes: n in {1, 64, 65} — a tail lane, a full wave, a second workgroup — and one run of 300.  Every comparison is exact.

No test reaches ok = 0 of the map: the kernel of the 3-isogeny has no point whose x lies on E'(Fq2)
(test_bls12_381_g2_cpu.py::test_kernel_of_the_isogeny_is_unreachable), so no input has an image with Z = 0."""
import ctypes
import json
import os
import random
import struct
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bls12_381_g1_ref as g1  # noqa: E402
import bls12_381_g2_ref as g2  # noqa: E402
import secp256k1_ref as k1  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
P, R_ORDER, H_EFF, ORDER = g2.P, g2.R_ORDER, g2.H_EFF, g2.H2 * g2.R_ORDER
RO, NU = 17, 18
R392 = 1 << 392
R392_INV = pow(R392, -1, P)
LENGTHS = (0, 1, 55, 56, 64, 119, 120, 517)


def _h2c(variant):
    return json.load(open(os.path.join(GOLDEN, "h2c", f"bls12_381_G2_{variant}.json")))["vectors"]


def _f(v):
    return int(v["re"], 16), int(v["im"], 16)           # (int() strips the white space of the three malformed strings)


def _xy(v):
    return _f(v["x"]), _f(v["y"])


def fq2_raw(a):
    return a[0].to_bytes(48, "little") + a[1].to_bytes(48, "little")


def raw(pt):
    return bytes(192) if pt is None else fq2_raw(pt[0]) + fq2_raw(pt[1])


def fq2_of(blob):
    return int.from_bytes(blob[:48], "little"), int.from_bytes(blob[48:96], "little")


def pts_of(blob):
    out = []
    for i in range(0, len(blob), 192):
        x, y = fq2_of(blob[i : i + 96]), fq2_of(blob[i + 96 : i + 192])
        out.append(None if x == (0, 0) and y == (0, 0) else (x, y))
    return out


def _us(us):
    return b"".join(fq2_raw(u) for u in us)


def _sc(ks):
    return b"".join(k.to_bytes(96, "little") for k in ks)


_CACHE = {}


def outside_point():
    """`Q0` of an RO vector: a point of E(Fq2) that is not in G2"""
    if "outside" not in _CACHE:
        q = _xy(_h2c("ro")[1]["Q0"])
        assert g2.on_curve(q) and not g2.in_g2(q)
        _CACHE["outside"] = q
    return _CACHE["outside"]


def hashed_point():
    return _xy(_h2c("ro")[2]["P"])


def random_images():
    """300 field elements, their images and the cleared images, computed once"""
    if "images" not in _CACHE:
        rng = random.Random(22381)
        us = [(rng.randrange(P), rng.randrange(P)) for _ in range(300)]
        images = [g2.map_to_curve(u) for u in us]
        _CACHE["images"] = (us, images, [g2.clear_cofactor_psi(q) for q in images])
    return _CACHE["images"]


# ---------------------------------------------------------------- field
def carried(v):
    """the carried limb image of the integer v: limbs 0..12 in [0, 2^28), the rest in the signed top limb"""
    return [(v >> (28 * i)) & 0xFFFFFFF for i in range(13)] + [v >> 364]


def _val(limbs):
    return sum(v << (28 * i) for i, v in enumerate(limbs))


def _pack(rows):
    return b"".join(struct.pack("<28i", *(c0 + c1)) for c0, c1 in rows)


def test_field_selftest_at_contract_bounds(ctx):
    """a: carried images of either component over (-2.1 p, 1.1 p), what the addition feeds its folds and b3 (products n, the same minus
    p and minus 2 p), with the most positive limbs a carried value can have (0..12 all 2^28 - 1) at both ends of that range; b: what
    a product's other side sees — carried values up to 20.6 p either way (the doubling's Y^2 - 3 b3 Z^2 + 18 p) and NEGATED carried
    values (limbs 0..12 all non-positive, down to -(2^28 - 1): conj, neg).  Residues: 0, 1, i, p - 1 in either component, squares and
    non-squares, c1 = 0, c0 = 0.  Expected values are big integers: an image a stands for a 2^-392 mod p."""
    from dot_ring_amd.curve import Fp2

    rng = random.Random(228)
    mont = lambda x: x % P * R392 % P  # noqa: E731
    residues = [(0, 0), (1, 0), (0, 1), (P - 1, 0), (0, P - 1), (P - 1, P - 1), (4, 0), (0, 4), (P - 4, 0), (5, 0), (0, 5)]
    for _ in range(10):
        x = (rng.randrange(P), rng.randrange(P))
        residues += [g2.f2_sqr(x), g2.f2_mul(g2.SSWU_Z, g2.f2_sqr(x)), (rng.randrange(P), 0), (0, rng.randrange(P))]
    top_full = lambda top: [0xFFFFFFF] * 13 + [top]  # noqa: E731
    A, B = [], []
    for x in residues:
        for shift0, shift1 in ((0, 0), (-1, -2), (-2, 0), (0, -1)):
            A.append((carried(mont(x[0]) + shift0 * P), carried(mont(x[1]) + shift1 * P)))
    # the extreme limb images (their residues are whatever they are): all low limbs at 2^28 - 1, top limb at either end of the range
    A += [(top_full(0x1A000), top_full(-0x30000)), (top_full(-0x30000), top_full(0x1A000)), (top_full(0), top_full(-1)),
          ([0] * 13 + [0x1A011], [0] * 13 + [-0x34000])]
    for i in range(len(A)):
        wide = [carried(mont(rng.randrange(P)) + rng.choice((19, -20)) * P) for _ in range(2)]
        negated = [[-w for w in carried(mont(rng.randrange(P)) + rng.choice((0, 2)) * P)] for _ in range(2)]
        B.append((wide, negated, [wide[0], negated[1]], [[-0xFFFFFFF] * 13 + [-0x1A000], top_full(0x1A000)])[i % 4])
    for c0, c1 in A:
        for c in (c0, c1):
            assert -2.1 * P < _val(c) < 1.1 * P and all(0 <= w < 1 << 28 for w in c[:13])
    for c0, c1 in B:
        for c in (c0, c1):
            assert abs(_val(c)) < 20.6 * P and all(abs(w) < 1 << 28 for w in c[:13])
    n = len(A)
    assert n > 128                                                                 # three workgroups, the last one partial
    out, flags = ctx.blsg2_field_selftest(_pack(A), _pack(B))
    assert len(out) == 480 * n and len(flags) == n
    squares = 0
    for i in range(n):
        rec = [fq2_of(out[480 * i + 96 * j : 480 * i + 96 * j + 96]) for j in range(5)]
        x = tuple(_val(c) * R392_INV % P for c in A[i])
        y = tuple(_val(c) * R392_INV % P for c in B[i])
        is_square = g2.f2_is_square(x)
        squares += is_square
        assert rec[0] == g2.f2_mul(x, y), i
        assert rec[1] == g2.f2_sqr(x), i
        assert rec[2] == (g2.ZERO if x == g2.ZERO else g2.f2_inv(x)), i
        assert rec[3] == g2.f2_mul((12, 12), x), i
        if is_square:
            assert g2.f2_sqr(rec[4]) == x, i
            assert rec[4] == Fp2(x[0], x[1], P).sqrt().to_tuple(), i                 # the same route: the same one of the two roots
        else:
            assert rec[4] == g2.ZERO, i
        assert flags[i] == (1 if is_square else 0) | (2 if g2.f2_sgn0(x) else 0) | (4 if x == g2.ZERO else 0), i
    assert 40 < squares < n - 20


# ---------------------------------------------------------------- the map
def test_map_to_curve_vectors(ctx):
    ro, nu = _h2c("ro"), _h2c("nu")
    singles = [_f(u) for v in ro for u in v["u"]] + [_f(v["u"][0]) for v in nu]
    images = [_xy(v[q]) for v in ro for q in ("Q0", "Q1")] + [_xy(v["Q0"]) for v in nu]
    out, ok = ctx.blsg2_map_to_curve(_us(singles), 1, clear=False)
    assert ok == b"\x01" * 15 and pts_of(out) == images
    out, ok = ctx.blsg2_map_to_curve(_us(singles[:10]), 2, clear=True)
    assert ok == b"\x01" * 5 and pts_of(out) == [_xy(v["P"]) for v in ro]
    out, ok = ctx.blsg2_map_to_curve(_us(singles[10:]), 1, clear=True)
    assert ok == b"\x01" * 5 and pts_of(out) == [_xy(v["P"]) for v in nu]
    out, ok = ctx.blsg2_map_to_curve(_us(singles[:10]), 2, clear=False)
    assert ok == b"\x01" * 5 and pts_of(out) == [g2.add(images[2 * i], images[2 * i + 1]) for i in range(5)]
    out, ok = ctx.blsg2_map_to_curve(_us(singles), 1, clear=True)
    assert ok == b"\x01" * 15 and pts_of(out) == [g2.clear_cofactor_psi(q) for q in images]


def test_map_to_curve_edges_pairs_and_random(ctx):
    x = 0x123456789ABCDEF
    edges = [(0, 0), (1, 0), (0, 1), (P - 1, P - 1), (0, x), (x, 0), (0, x + 1), (x + 1, 0)]    # (0, x): sgn0 falls through to the imaginary part
    out, ok = ctx.blsg2_map_to_curve(_us(edges), 1, clear=False)
    assert ok == b"\x01" * len(edges) and pts_of(out) == [g2.map_to_curve(u) for u in edges]
    u = (0x1234567, 0x7654321)
    pairs = [u, u, u, g2.f2_neg(u), (0, 0), (0, 0), (0, x), (0, P - x)]              # a doubling in the sum; a cancelling pair; ...
    for clear in (False, True):
        out, ok = ctx.blsg2_map_to_curve(_us(pairs), 2, clear=clear)
        want = [g2.map_sum(pairs[2 * i : 2 * i + 2], clear) for i in range(4)]
        assert ok == b"\x01" * 4 and pts_of(out) == want
        assert want[1] is None and out[192:384] == bytes(192) and want[3] is None    # u and -u: the identity, 192 zero bytes, ok = 1
        q = g2.map_to_curve(u)
        assert want[0] == (g2.clear_cofactor if clear else (lambda pt: pt))(g2.add(q, q))
    us, images, cleared = random_images()
    for n in (1, 64, 65, 300):
        for clear in (False, True):
            out, ok = ctx.blsg2_map_to_curve(_us(us[:n]), 1, clear=clear)
            assert ok == b"\x01" * n and pts_of(out) == (cleared if clear else images)[:n]
    for n in (1, 64, 65):
        sums = [g2.add(images[2 * i], images[2 * i + 1]) for i in range(n)]
        out, ok = ctx.blsg2_map_to_curve(_us(us[: 2 * n]), 2, clear=False)
        assert ok == b"\x01" * n and pts_of(out) == sums
        out, ok = ctx.blsg2_map_to_curve(_us(us[: 2 * n]), 2, clear=True)
        assert ok == b"\x01" * n and pts_of(out) == [g2.add(cleared[2 * i], cleared[2 * i + 1]) for i in range(n)]   # clearing is a homomorphism


def test_bad_inputs(ctx):
    for bad in ((P, 0), (0, P), (P + 1, 1), ((1 << 384) - 1, 0), (0, (1 << 384) - 1)):
        for per_item in (1, 2):
            with pytest.raises(ValueError):
                ctx.blsg2_map_to_curve(_us([(5, 5), bad]), per_item)
        with pytest.raises(ValueError):
            ctx.blsg2_scalar_mul_batch(fq2_raw(bad) + bytes(96), bytes(96))
        with pytest.raises(ValueError):
            ctx.blsg2_check_points(bytes(96) + fq2_raw(bad))
    for per_item in (0, 3, -1):
        with pytest.raises(ValueError):
            ctx.blsg2_map_to_curve(_us([(5, 5)] * 6), per_item)
    with pytest.raises(ValueError):
        ctx.blsg2_scalar_mul_batch(bytes(96), bytes(32))                           # a G1 point and scalar are not a G2 point and scalar
    for variant in (15, 16, 19):
        with pytest.raises(ValueError):
            ctx.blsg2_encode_to_curve_batch(variant, [b"abc"])
    for variant in (RO, NU):
        with pytest.raises(ValueError):
            ctx.blsg1_encode_to_curve_batch(variant, [b"abc"])
    assert ctx.blsg2_map_to_curve(b"", 1) == (b"", b"") and ctx.blsg2_scalar_mul_batch(b"", b"") == b""


def test_encode_to_curve_batch(ctx):
    import dot_ring_amd as d

    rng = random.Random(32381)
    for name, variant, encode, cv in (("ro", RO, g2.encode_to_curve_ro, d.BLS12_381_G2_RO), ("nu", NU, g2.encode_to_curve_nu, d.BLS12_381_G2_NU)):
        vecs = _h2c(name)
        out = ctx.blsg2_encode_to_curve_batch(variant, [v["msg"].encode() for v in vecs])
        assert pts_of(out) == [_xy(v["P"]) for v in vecs]
        msgs = [bytes(rng.randrange(256) for _ in range(length)) for length in LENGTHS]
        salts = [bytes(rng.randrange(256) for _ in range(32 if i % 2 else 0)) for i in range(len(msgs))]
        want = [encode(s + m) for m, s in zip(msgs, salts)]
        assert pts_of(ctx.blsg2_encode_to_curve_batch(variant, msgs, salts)) == want
        assert pts_of(ctx.blsg2_encode_to_curve_batch(variant, [s + m for m, s in zip(msgs, salts)])) == want
        point_type = cv.point_type
        got = point_type.encode_to_curve_batch(msgs, salts)
        assert [(p.x.to_tuple(), p.y.to_tuple()) for p in got] == want
        single = point_type.encode_to_curve(msgs[3], salts[3])
        assert single == got[3] and single.is_on_curve() and type(single) is point_type
        assert point_type.encode_to_curve_from_field(point_type.hash_to_field_pairs(msgs, salts)) == got
        mapped = point_type.map_to_curve_simple_swu((3, 4))
        assert (mapped.x.to_tuple(), mapped.y.to_tuple()) == g2.map_to_curve((3, 4))
        assert point_type.encode_to_curve_batch([]) == []


# ---------------------------------------------------------------- the group
def test_scalar_mul(ctx):
    """the scalars of the issue on the generator, a hashed point (in G2) and a Q0 (outside G2), in ONE launch whose waves start at bit
    767; then the three shapes with short scalars (the walk starts at the wave's top set bit)"""
    import dot_ring_amd as d

    outside, hashed = outside_point(), hashed_point()
    scalars = [0, 1, 2, R_ORDER - 1, R_ORDER, R_ORDER + 1, H_EFF, ORDER - 1, ORDER, 1 << 767, (1 << 768) - 1]
    pts = [pt for pt in (g2.G, hashed, outside) for _ in scalars]
    ks = scalars * 3
    got = pts_of(ctx.blsg2_scalar_mul_batch(b"".join(raw(pt) for pt in pts), _sc(ks)))
    assert got == [g2.mul(k, pt) for k, pt in zip(ks, pts)]
    by = lambda pt, k: got[[g2.G, hashed, outside].index(pt) * len(scalars) + scalars.index(k)]  # noqa: E731
    assert by(g2.G, R_ORDER) is None and by(hashed, R_ORDER) is None and by(hashed, R_ORDER + 1) == hashed
    assert by(outside, R_ORDER) is not None                                        # a reduction mod r would give the identity
    assert by(outside, ORDER) is None and by(outside, ORDER - 1) == g2.neg(outside) and g2.in_g2(by(outside, H_EFF))
    rng = random.Random(42381)
    base = [g2.G, hashed, outside, None]
    for n in (1, 64, 65):
        pts = [base[i % 4] for i in range(n)]
        ks = [rng.randrange(1 << rng.choice((1, 9, 17))) for _ in range(n)]
        assert pts_of(ctx.blsg2_scalar_mul_batch(b"".join(raw(pt) for pt in pts), _sc(ks))) == [g2.mul(k, pt) for k, pt in zip(ks, pts)]
    # the point class: negative, plain, and above 2^768 (reduced mod h2 r on the host)
    point_type = d.BLS12_381_G2.point_type
    q = point_type(*outside)
    as_ref = lambda pt: None if pt.is_identity() else (pt.x.to_tuple(), pt.y.to_tuple())  # noqa: E731
    assert as_ref(q * 5) == g2.mul(5, outside) and as_ref(q * -5) == g2.mul(-5, outside) and as_ref(5 * q) == g2.mul(5, outside)
    assert (q * 0).is_identity() and (q * ORDER).is_identity() and not (q * R_ORDER).is_identity()
    assert as_ref(q * ((1 << 770) + 12345)) == g2.mul(((1 << 770) + 12345) % ORDER, outside)
    assert as_ref(q.clear_cofactor()) == g2.clear_cofactor(outside) == g2.clear_cofactor_psi(outside)
    assert (point_type.identity() * 7).is_identity() and as_ref(point_type.generator_point() * R_ORDER) is None


def test_two_clearing_routes_agree_on_the_device(ctx):
    us, images, cleared = random_images()
    mapped, ok = ctx.blsg2_map_to_curve(_us(us[:65]), 1, clear=False)
    assert ok == b"\x01" * 65
    by_scalar = ctx.blsg2_scalar_mul_batch(mapped, _sc([H_EFF] * 65))
    by_psi, ok = ctx.blsg2_map_to_curve(_us(us[:65]), 1, clear=True)
    assert by_scalar == by_psi and pts_of(by_psi) == cleared[:65]


def test_check_points(ctx):
    us, images, cleared = random_images()
    off_curve = ((1, 1), (1, 1))
    assert not g2.on_curve(off_curve)
    twisted = (g2.G[0], g2.f2_add(g2.G[1], (1, 0)))
    cases = [(g2.G, 1, 1), (hashed_point(), 1, 1), (outside_point(), 1, 0), (off_curve, 0, 0), (twisted, 0, 0), (None, 1, 1),
             (g2.neg(hashed_point()), 1, 1), (g2.mul(R_ORDER, outside_point()), 1, 0)]
    cases += [(q, 1, 0) for q in images[:30]] + [(q, 1, 1) for q in cleared[:27]]
    assert len(cases) == 65
    for n in (1, 64, 65):
        blob = b"".join(raw(pt) for pt, _, _ in cases[:n])
        assert ctx.blsg2_check_points(blob, subgroup=False) == bytes(c for _, c, _ in cases[:n])
        assert ctx.blsg2_check_points(blob, subgroup=True) == bytes(s for _, _, s in cases[:n])
    assert ctx.blsg2_check_points(b"") == b""


# ---------------------------------------------------------------- refusals
def test_ids_17_and_18_are_refused_at_the_64_byte_entry_points(ctx):
    """as ids 15 and 16 (test_gpu_bls12_381_g1.py::test_refusals): dr_te_*, hash_to_field / encode_to_curve, the Pedersen and IETF
    provers and verifiers, the ring prover's creation and the Ring-VRF calls: DR_ERR_INVALID, for the curve id's sake"""
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
        suite = _native.vrf_suite(b"BLS12381G2_XMD:SHA-256_SSWU_RO_", 2, bytes(64), bytes(64), cid)
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
    for cv in (d.BLS12_381_G2_RO, d.BLS12_381_G2_NU):
        for scheme in (d.TinyVRF, d.ThinVRF, d.PedersenVRF, d.RingVRF):
            with pytest.raises(ValueError, match="no point codec"):
                scheme[cv]
        with pytest.raises(ValueError):
            d.RingProofParams(cv=cv)


def test_g1_and_secp256k1_after_g2_calls(ctx):
    """the chain of (p - 3) / 4 and the small multiples are shared with the G1 unit (kernels_g1_h2c.hip.h), and the stage buffer is one of
    the context's scratch buffers: after G2 calls on this context a G1 hash still has the vector file's bytes and a secp256k1 proof the
    restatement's"""
    import dot_ring_amd as d

    ctx.blsg2_map_to_curve(_us([(1, 2), (3, 4)]), 2)
    ctx.blsg2_scalar_mul_batch(raw(g2.G) * 65, _sc([(1 << 20) - 1] * 65))
    vecs = json.load(open(os.path.join(GOLDEN, "h2c", "bls12_381_G1_ro.json")))["vectors"]
    out = ctx.blsg1_encode_to_curve_batch(15, [v["msg"].encode() for v in vecs])
    want = b"".join(int(v["P"]["x"], 16).to_bytes(48, "little") + int(v["P"]["y"], 16).to_bytes(48, "little") for v in vecs)
    assert out == want
    assert d.BLS12_381_G1.point_type.encode_to_curve(b"abc").x == g1.encode_to_curve_ro(b"abc")[0]
    sk, al, ad = (7).to_bytes(32, "little"), b"after g2", b"ad"
    assert d.TinyVRF[d.Secp256k1].prove(al, sk, ad).encode() == k1.RO.ietf_prove(sk, al, ad)
