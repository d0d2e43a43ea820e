"""Ed448 on the GPU (DR_CURVE_ED448_RO = 19, DR_CURVE_ED448_NU = 20; csrc/fe448.hip.h and csrc/kernels_ed448.hip.h): the device field at
the limb bounds the law and the map feed, the map of RFC 9380 against the vector files and the big-integer restatement (ed448_ref.py),
scalar multiplication by 448-bit scalars used as they are — on the generator, on a hashed point and on a point of order 4 n OUTSIDE the
prime-order subgroup, where a scalar reduced mod n on the device would be wrong — grouped MSMs, the decoder, the Tiny / Thin / Pedersen
VRFs byte for byte against the restatement (whose XOF and width handling test_ed448_cpu.py pins on the reference's Bandersnatch
SHAKE128 files), the refusals, and an Ed25519_RO proof and a G1 hash afterwards.
Shapes: n in {1, 64, 65} — a tail lane, a full wave, a second workgroup — and one run of 300.  Every comparison is exact.

Three things the kernels cannot be shown, because no input has them (test_ed448_cpu.py::test_no_input_reaches_montgomery_x_plus_minus_one):
an image with Montgomery x = +-1, an image outside the prime-order subgroup — the 4-isogeny from curve448 lands in it — and a pair
(u, -u) summing to the identity: the map depends on u^2 alone.  The point outside the subgroup used below is 7 G + (1, 0)."""
import ctypes
import json
import os
import random
import struct
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ed448_ref as e  # noqa: E402
import h2c_ref  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
P, N = e.P, e.N
RO, NU = 19, 20
NORMAL = 2**28 + 2**10
OUTSIDE = e.add(e.mul(7, e.G), (1, 0))                    # order 4 n


def _h2c(variant):
    return json.load(open(os.path.join(GOLDEN, "h2c", f"ed448_{variant}.json")))["vectors"]


def _base():
    return json.load(open(os.path.join(GOLDEN, "base", "ed448_base_vectors.json")))


def _xy(v):
    return int(v["x"], 16), int(v["y"], 16)


def _us(values):
    return b"".join(int(u).to_bytes(56, "little") for u in values)


def _sc(values):
    return b"".join(int(k).to_bytes(56, "little") for k in values)


def pts_of(blob):
    return [(int.from_bytes(blob[i : i + 56], "little"), int.from_bytes(blob[i + 56 : i + 112], "little")) for i in range(0, len(blob), 112)]


@pytest.fixture(scope="module")
def hashed():
    return e.encode_to_curve_ro(b"a hashed point")


# ---------------------------------------------------------------- the field
def _limbs(images):
    return b"".join(struct.pack("<16i", *img) for img in images)


def _val(img):
    return sum(x << (28 * i) for i, x in enumerate(img))


def _split(v):
    return [(v >> (28 * i)) & (2**28 - 1) for i in range(16)]


def test_field_selftest_at_the_limb_bounds(ctx):
    """records: a b, a^2, a + b, a - b, -a, carry(a), 39081 a, a^-1, a^((p + 1) / 4), a, 156326 a; flags: square, odd, zero, a = b.
    a is at most 1 n (what sqr and the roots take), b up to 3 n (the product's budget ka kb <= 3)"""
    rng = random.Random(448)
    a_imgs, b_imgs = [], []
    for v in (0, 1, 2, P - 1, P, P + 1, 2**448 - 1, 2**224, 4, P - 4):          # canonical values and non-canonical ones in [p, 2^448)
        a_imgs.append(_split(v))
        b_imgs.append(_split(rng.randrange(P)))
    for bound_a, bound_b in ((NORMAL, 3 * NORMAL), (NORMAL, NORMAL)):
        for sa in (1, -1):
            for sb in (1, -1):
                a_imgs.append([sa * bound_a] * 16)
                b_imgs.append([sb * bound_b] * 16)
                a_imgs.append([sa * bound_a if i % 2 else -sa * bound_a for i in range(16)])
                b_imgs.append([sb * bound_b if i % 2 else -sb * bound_b for i in range(16)])
    while len(a_imgs) < 65:
        a_imgs.append([rng.randint(-NORMAL, NORMAL) for _ in range(16)])
        b_imgs.append([rng.randint(-3 * NORMAL, 3 * NORMAL) for _ in range(16)])
    a_imgs.append(_split(9))
    b_imgs.append([x + y for x, y in zip(_split(9), _split(P))])                # a = b mod p in another image
    out, flags = ctx.ed448_field_selftest(_limbs(a_imgs), _limbs(b_imgs))
    squares = 0
    for i, (ai, bi) in enumerate(zip(a_imgs, b_imgs)):
        a, b = _val(ai) % P, _val(bi) % P
        rec = [int.from_bytes(out[616 * i + 56 * r : 616 * i + 56 * r + 56], "little") for r in range(11)]
        square = pow(a, (P - 1) // 2, P) in (0, 1)
        squares += square
        want = [a * b % P, a * a % P, (a + b) % P, (a - b) % P, -a % P, a, 39081 * a % P, pow(a, P - 2, P), pow(a, (P + 1) // 4, P), a, 156326 * a % P]
        assert rec == want, i
        assert not square or rec[8] * rec[8] % P == a
        assert flags[i] == (1 if square else 0) | (2 if a & 1 else 0) | (4 if a == 0 else 0) | (8 if a == b else 0), i
    assert 10 < squares < len(a_imgs) - 10                                      # squares and non-squares both
    assert int.from_bytes(out[7 * 56 : 8 * 56], "little") == 0                  # 0^-1 = 0
    assert flags[-1] & 8


# ---------------------------------------------------------------- the map
@pytest.mark.parametrize("variant", ["ro", "nu"])
def test_map_reproduces_the_vectors(ctx, variant):
    vecs = _h2c(variant)
    per = 2 if variant == "ro" else 1
    us = [int(u, 16) for v in vecs for u in v["u"]]
    images = [_xy(v[k]) for v in vecs for k in (("Q0", "Q1") if per == 2 else ("Q",))]
    raw, ok = ctx.ed448_map_to_curve(_us(us), 1, clear=False)                   # u -> Q0 / Q1 / Q
    assert pts_of(raw) == images and set(ok) == {1}
    raw, ok = ctx.ed448_map_to_curve(_us(us), per, clear=True)                  # -> P
    assert pts_of(raw) == [_xy(v["P"]) for v in vecs] and set(ok) == {1}
    raw, ok = ctx.ed448_map_to_curve(_us(us), per, clear=False)
    assert pts_of(raw) == [images[per * i] if per == 1 else e.add(images[2 * i], images[2 * i + 1]) for i in range(len(vecs))]
    raw, ok = ctx.ed448_map_to_curve(_us(us), 1, clear=True)
    assert pts_of(raw) == [e.clear_cofactor(q) for q in images]


def test_map_inputs_without_a_value(ctx):
    import dot_ring_amd as d

    us = [0, 1, P - 1, 2, P - 2, 3]
    raw, ok = ctx.ed448_map_to_curve(_us(us), 1, clear=False)
    assert list(ok) == [0, 0, 0, 1, 1, 1] and raw[: 3 * 112] == bytes(3 * 112)
    assert pts_of(raw)[3:] == [e.map_to_curve(u) for u in us[3:]]
    raw, ok = ctx.ed448_map_to_curve(_us([2, 0, 1, 3, 4, 5]), 2, clear=True)     # one valueless element spoils its item
    assert list(ok) == [0, 0, 1] and raw[: 2 * 112] == bytes(2 * 112)
    assert pts_of(raw)[2] == e.clear_cofactor(e.add(e.map_to_curve(4), e.map_to_curve(5)))
    pt = d.Ed448.point_type
    for u in (0, 1, P - 1):
        with pytest.raises(ValueError, match="Point is not on the curve"):
            pt.map_to_curve(u)
    q = pt.map_to_curve(2)
    assert (q.x, q.y) == e.map_to_curve(2)
    for bad in (_us([P]), _us([2**448 - 1])):
        with pytest.raises(ValueError):
            ctx.ed448_map_to_curve(bad, 1)
    with pytest.raises(ValueError):
        ctx.ed448_map_to_curve(_us([1, 2, 3]), 3)


def test_map_pairs(ctx):
    """(u, u) and (u, -u) both double the image: the map depends on u^2 alone — the sign of the root is fixed by the parity of its
    canonical value (the reference's e2 ^ e3), not by u — so no pair of inputs is known to sum to the identity, which the scalar
    multiplications below store instead (k = 0, 4 n)"""
    u = 0x1234567
    img = e.map_to_curve(u)
    assert e.map_to_curve(P - u) == img
    raw, ok = ctx.ed448_map_to_curve(_us([u, u, u, P - u]), 2, clear=False)
    assert pts_of(raw) == [e.add(img, img)] * 2 and list(ok) == [1, 1]
    raw, ok = ctx.ed448_map_to_curve(_us([u, P - u]), 2, clear=True)
    assert pts_of(raw) == [e.mul(8, img)] and list(ok) == [1]


@pytest.mark.parametrize("n", [1, 64, 65])
def test_map_against_the_restatement(ctx, n):
    rng = random.Random(n)
    us = [rng.randrange(P) for _ in range(2 * n)]
    raw, ok = ctx.ed448_map_to_curve(_us(us), 2)
    assert set(ok) == {1}
    assert pts_of(raw) == [e.clear_cofactor(e.add(e.map_to_curve(us[2 * i]), e.map_to_curve(us[2 * i + 1]))) for i in range(n)]


def test_map_300_elements_and_clearing_is_multiplication_by_four(ctx):
    rng = random.Random(300)
    us = [rng.randrange(P) for _ in range(300)]
    raw, ok = ctx.ed448_map_to_curve(_us(us), 1, clear=False)
    assert set(ok) == {1} and pts_of(raw) == [e.map_to_curve(u) for u in us]
    cleared, _ = ctx.ed448_map_to_curve(_us(us), 1, clear=True)
    assert ctx.ed448_scalar_mul_batch(raw, _sc([4] * 300)) == cleared


@pytest.mark.parametrize("variant,cid", [("ro", RO), ("nu", NU)])
def test_encode_to_curve_batch(ctx, variant, cid):
    import dot_ring_amd as d

    vecs = _h2c(variant)
    out = ctx.ed448_encode_to_curve_batch(cid, [v["msg"].encode() for v in vecs])
    assert pts_of(out) == [_xy(v["P"]) for v in vecs]
    fn = e.encode_to_curve_ro if cid == RO else e.encode_to_curve_nu
    rng = random.Random(cid)
    msgs = [rng.randbytes(n) for n in (0, 1, 81, 82, 83, 217, 218, 219, 517)]
    salts = [rng.randbytes(1 + i) for i in range(len(msgs))]
    assert pts_of(ctx.ed448_encode_to_curve_batch(cid, msgs, salts)) == [fn(s + m) for m, s in zip(msgs, salts)]
    assert pts_of(ctx.ed448_encode_to_curve_batch(cid, msgs)) == [fn(m) for m in msgs]
    cv = d.Ed448_RO if cid == RO else d.Ed448_NU
    got = cv.point_type.encode_to_curve_batch(msgs[:3], salts[:3])
    assert [(p.x, p.y) for p in got] == [fn(s + m) for m, s in zip(msgs[:3], salts[:3])]
    one = cv.point_type.encode_to_curve(msgs[1], salts[1])
    assert (one.x, one.y) == fn(salts[1] + msgs[1])
    assert cv.point_type.encode_to_curve_from_field(cv.point_type.hash_to_field_pairs(msgs[:2], salts[:2])) == got[:2]


# ---------------------------------------------------------------- scalar multiplication
# the last two: every nibble 7 (the largest digit everywhere, no carry) and every nibble 8 (a carry out of every digit, up into window 113)
SCALARS = [0, 1, 2, 4, N - 1, N, N + 1, 4 * N - 1, 4 * N, 2**447, 2**448 - 1, int("7" * 112, 16), int("8" * 112, 16)]


@pytest.mark.parametrize("base", ["generator", "hashed", "outside"])
def test_scalar_mul_takes_scalars_as_they_are(ctx, hashed, base):
    pt = {"generator": e.G, "hashed": hashed, "outside": OUTSIDE}[base]
    got = pts_of(ctx.ed448_scalar_mul_batch(e.raw(pt) * len(SCALARS), _sc(SCALARS)))
    assert got == [e.mul(k, pt) for k in SCALARS]
    if base == "outside":
        # n Q != O here: a device that reduced mod n would answer O for k = n and Q for k = n + 1
        assert got[5] != e.O and got[5] == e.mul(N % 4, (1, 0)) and got[6] != pt and got[8] == e.O
    else:
        assert got[5] == e.O and got[6] == pt


@pytest.mark.parametrize("n", [1, 64, 65, 300])
def test_scalar_mul_batches(ctx, hashed, n):
    rng = random.Random(n)
    bases = [e.G, hashed, OUTSIDE, e.O, (1, 0), (0, P - 1)]
    pts = [bases[i % len(bases)] for i in range(n)]
    ks = [rng.randrange(2**448) for _ in range(n)]
    got = pts_of(ctx.ed448_scalar_mul_batch(b"".join(e.raw(p) for p in pts), _sc(ks)))
    check = range(n) if n <= 65 else rng.sample(range(n), 40)
    for i in check:
        assert got[i] == e.mul(ks[i], pts[i]), i
    with pytest.raises(ValueError):
        ctx.ed448_scalar_mul_batch(_us([P, 1]), _sc([1]))


def test_python_mul_reduces_mod_n(hashed):
    import dot_ring_amd as d

    pt = d.Ed448.point_type
    g, q = pt.generator_point(), pt(*OUTSIDE)
    for k in (0, 1, N - 1, N, N + 5, 2**448 + 3, -1):
        r = g * k
        assert (r.x, r.y) == e.mul(k % N, e.G)
        r = q * k                                         # the reference's __mul__: k mod n, whatever the point's order
        assert (r.x, r.y) == e.mul(k % N, OUTSIDE)
    assert 3 * g == g * 3
    many = d.curve.scalar_mul_batch([g, pt(*hashed)], [N + 2, 7])
    assert [(p.x, p.y) for p in many] == [e.mul(2, e.G), e.mul(7, hashed)]


@pytest.mark.parametrize("m", [1, 2, 63, 64])
def test_msm_groups(ctx, hashed, m):
    rng = random.Random(m)
    groups = 3 if m < 63 else 2
    bases = [e.G, hashed, OUTSIDE, e.O]
    pts = [bases[rng.randrange(4)] for _ in range(groups * m)]
    ks = [rng.randrange(2**448) if i % 5 else rng.randrange(16) for i in range(groups * m)]
    got = pts_of(ctx.ed448_msm_groups(b"".join(e.raw(p) for p in pts), _sc(ks), m))
    assert got == [e.msm(pts[g * m : (g + 1) * m], ks[g * m : (g + 1) * m]) for g in range(groups)]
    with pytest.raises(ValueError):
        ctx.ed448_msm_groups(e.raw(e.G) * 65, _sc([1] * 65), 65)


def test_python_msm_folds_beyond_64_terms(hashed):
    import dot_ring_amd as d

    pt = d.Ed448.point_type
    rng = random.Random(70)
    pts = [e.G, hashed] * 35
    ks = [rng.randrange(N) for _ in range(70)]
    want = e.msm(pts, ks)
    points = [pt(*p) for p in pts]
    r = pt.msm(points, ks)
    assert (r.x, r.y) == want
    (r2,) = d.curve.msm_groups(points, ks, 70)
    assert r2 == r
    assert pt.msm([], []) == pt.identity()
    pair = d.curve.msm_groups(points[:4], [1, 2, -3, N + 4], 2)
    assert [(p.x, p.y) for p in pair] == [e.msm(pts[:2], [1, 2]), e.msm(pts[2:4], [N - 3, 4])]


# ---------------------------------------------------------------- the decoder
def test_decoder(ctx, hashed):
    import dot_ring_amd as d
    from dot_ring_amd.vrf.codec import dec_point, dec_points

    off_curve = (1, 1)
    cases = [e.O, (0, P - 1), (1, 0), (P - 1, 0), e.G, hashed, OUTSIDE, off_curve]
    blob = b"".join(e.raw(p) for p in cases) + _us([P, 1]) + _us([0, P + 1]) + _us([P + 1, 0])
    out, ok = ctx.ed448_decode_points(blob, check=False)
    assert list(ok) == [1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0]
    out1, ok1 = ctx.ed448_decode_points(blob, check=True)
    assert list(ok1) == [0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0]
    for o, flags in ((out, ok), (out1, ok1)):
        for i, f in enumerate(flags):
            assert o[112 * i : 112 * i + 112] == (blob[112 * i : 112 * i + 112] if f else bytes(112))
    for n in (1, 64, 65):
        pts = [e.G if i % 3 else OUTSIDE for i in range(n)]
        _, flags = ctx.ed448_decode_points(b"".join(e.raw(p) for p in pts), check=True)
        assert list(flags) == [1 if i % 3 else 0 for i in range(n)]
    cv = d.Ed448
    assert [(p.x, p.y) for p in dec_points(cv, [e.raw(e.G), e.raw(hashed)])] == [e.G, hashed]
    for bad, text in ((e.raw(e.O), "not a valid nonidentity subgroup point"), (e.raw(OUTSIDE), "not a valid nonidentity subgroup point"),
                      (e.raw(off_curve), "Point is not on the curve"), (_us([P, 1]), "Invalid point coordinates"),
                      (e.raw(e.G)[:111], "point must be exactly 112 bytes")):
        with pytest.raises(ValueError, match=text):
            dec_point(cv, bad)
    pt = cv.point_type
    assert d.curve.valid_points([pt(*e.G), pt(*OUTSIDE), pt.identity(), pt(*hashed)]) == [True, False, False, True]
    assert cv.curve.valid_point(pt(*hashed)) and not cv.curve.valid_point(pt(1, 0))


# ---------------------------------------------------------------- the VRFs
def _records():
    return [(bytes.fromhex(v["sk"]), bytes.fromhex(v["alpha"]), bytes.fromhex(v["ad"])) for v in _base()]


@pytest.fixture(scope="module")
def restated():
    """the restatement's proofs of every (sk, alpha, ad) of the base file, computed once"""
    out = []
    for sk, alpha, ad in _records():
        out.append({"tiny": e.RO.ietf_prove(sk, alpha, ad), "thin": e.RO.ietf_prove(sk, alpha, ad, thin=True),
                    "pedersen": e.RO.pedersen_prove(sk, alpha, ad)})
    return out


def test_vrf_proofs_equal_the_restatement(restated):
    import dot_ring_amd as d

    cv = d.Ed448
    recs = _records()
    assert len(recs[0][0]) == 57                                                  # the reference's keys: reduced mod n
    alphas, sks, ads = [r[1] for r in recs], [r[0] for r in recs], [r[2] for r in recs]
    tiny = d.TinyVRF[cv].prove_batch(alphas, sks, ads)
    thin = d.ThinVRF[cv].prove_batch(alphas, sks, ads)
    ped = d.PedersenVRF[cv].prove_batch(alphas, sks, ads)
    for i, (sk, alpha, ad) in enumerate(recs):
        x = int.from_bytes(sk, "little") % N
        pk = cv.public_key_from_secret(sk)
        assert pk == e.raw(e.mul(x, e.G)) and len(pk) == 112
        assert tiny[i].encode() == restated[i]["tiny"] and len(tiny[i].encode()) == 184
        assert thin[i].encode() == restated[i]["thin"] and len(thin[i].encode()) == 280
        assert ped[i].encode() == restated[i]["pedersen"][0] and len(ped[i].encode()) == 560
        assert ped[i]._blinding_factor == restated[i]["pedersen"][1]
        for scheme, proof in ((d.TinyVRF[cv], tiny[i]), (d.ThinVRF[cv], thin[i])):
            back = scheme.decode(proof.encode())
            assert back == proof and back.verify(pk, alpha, ad)
            assert e.ietf_verify(e.RO, pk, proof.encode(), alpha, ad, thin=scheme.THIN)
            assert scheme.proof_to_hash(proof.output_point) == e.RO.point_to_hash(e.mul(x, e.RO.e2c(alpha)))
        back = d.PedersenVRF[cv].decode(ped[i].encode())
        assert back.encode() == ped[i].encode() and back.verify(alpha, ad) and ped[i].verify_unblinding(pk, ped[i]._blinding_factor)
    assert d.TinyVRF[cv].prove(alphas[0], sks[0], ads[0]) == tiny[0]


def test_vrf_over_the_nonuniform_variant():
    import dot_ring_amd as d

    cv = d.Ed448_NU
    sk, alpha, ad = _records()[1]
    pk = cv.public_key_from_secret(sk)
    tiny, thin, ped = d.TinyVRF[cv].prove(alpha, sk, ad), d.ThinVRF[cv].prove(alpha, sk, ad), d.PedersenVRF[cv].prove(alpha, sk, ad)
    assert tiny.encode() == e.NU.ietf_prove(sk, alpha, ad) and thin.encode() == e.NU.ietf_prove(sk, alpha, ad, thin=True)
    assert ped.encode() == e.NU.pedersen_prove(sk, alpha, ad)[0]
    assert tiny.verify(pk, alpha, ad) and thin.verify(pk, alpha, ad) and ped.verify(alpha, ad)
    assert tiny.encode() != d.TinyVRF[d.Ed448_RO].prove(alpha, sk, ad).encode()


def _flip(blob, byte, bit=0):
    out = bytearray(blob)
    out[byte] ^= 1 << bit
    return bytes(out)


def test_spoiled_proofs_do_not_verify(restated):
    import dot_ring_amd as d

    cv = d.Ed448
    sk, alpha, ad = _records()[1]
    pk = cv.public_key_from_secret(sk)
    other_pk = cv.public_key_from_secret(b"\x05" * 57)
    for scheme, blob in ((d.TinyVRF[cv], restated[1]["tiny"]), (d.ThinVRF[cv], restated[1]["thin"])):
        proof = scheme.decode(blob)
        assert proof.verify(pk, alpha, ad)
        assert not proof.verify(pk, alpha + b"x", ad) and not proof.verify(pk, alpha, ad + b"x") and not proof.verify(other_pk, alpha, ad)
        assert not scheme.decode(_flip(blob, len(blob) - 56)).verify(pk, alpha, ad)                      # s
        if not scheme.THIN:
            assert not scheme.decode(_flip(blob, 112)).verify(pk, alpha, ad)                             # c
        with pytest.raises(ValueError):
            scheme.decode(_flip(blob, 3))                                                                 # a point: off the curve
        with pytest.raises(ValueError, match="Invalid public key"):
            proof.verify(_flip(pk, 3), alpha, ad)
        with pytest.raises(ValueError, match="scalar is not canonical"):
            scheme.decode(blob[:-56] + N.to_bytes(56, "little"))
        with pytest.raises(ValueError, match="proof length"):
            scheme.decode(blob[:-1])
    blob = restated[1]["pedersen"][0]
    proof = d.PedersenVRF[cv].decode(blob)
    assert proof.verify(alpha, ad) and not proof.verify(alpha + b"x", ad) and not proof.verify(alpha, ad + b"x")
    assert not d.PedersenVRF[cv].decode(_flip(blob, 448)).verify(alpha, ad)                              # s
    assert not d.PedersenVRF[cv].decode(_flip(blob, 504)).verify(alpha, ad)                              # s_b
    with pytest.raises(ValueError, match="Invalid point in proof"):
        d.PedersenVRF[cv].decode(_flip(blob, 115))
    assert not proof.verify_unblinding(other_pk, restated[1]["pedersen"][1])


def test_batch_verify(restated):
    import dot_ring_amd as d

    cv = d.Ed448
    recs = _records()[:3]
    alphas, ads = [r[1] for r in recs], [r[2] for r in recs]
    pks = [cv.public_key_from_secret(r[0]) for r in recs]
    thin = [d.ThinVRF[cv].decode(restated[i]["thin"]) for i in range(3)]
    assert d.ThinVRF[cv].batch_verify(thin, pks, alphas, ads)
    assert not d.ThinVRF[cv].batch_verify(thin, pks, [alphas[0], alphas[1] + b"x", alphas[2]], ads)
    spoiled = [thin[0], d.ThinVRF[cv].decode(_flip(restated[1]["thin"], 224)), thin[2]]
    assert not d.ThinVRF[cv].batch_verify(spoiled, pks, alphas, ads)
    ped = [d.PedersenVRF[cv].decode(restated[i]["pedersen"][0]) for i in range(3)]
    assert d.PedersenVRF[cv].batch_verify(ped, alphas, ads)
    assert not d.PedersenVRF[cv].batch_verify(ped, alphas, [ads[0], ads[1], ads[2] + b"x"])
    spoiled = [ped[0], ped[1], d.PedersenVRF[cv].decode(_flip(restated[2]["pedersen"][0], 448))]
    assert not d.PedersenVRF[cv].batch_verify(spoiled, alphas, ads)


# ---------------------------------------------------------------- refusals and regressions
def test_ids_19_and_20_are_refused_elsewhere(ctx):
    import dot_ring_amd as d
    from dot_ring_amd import _native

    lib = _native.lib()
    INVALID = _native.DR_ERR_INVALID
    off = (ctypes.c_uint64 * 2)(0, 1)
    buf = lambda n=1024: ctypes.create_string_buffer(n)  # noqa: E731
    verdict = (ctypes.c_int * 1)()
    for cid in (RO, NU):
        assert lib.dr_te_scalar_mul_batch(ctx.handle, cid, bytes(64), bytes(32), 1, buf()) == INVALID
        assert b"curve" in lib.dr_last_error()
        assert lib.dr_te_msm(ctx.handle, cid, bytes(64), bytes(32), 1, buf()) == INVALID
        assert lib.dr_te_msm_groups(ctx.handle, cid, bytes(64), bytes(32), 1, 1, buf()) == INVALID
        assert lib.dr_te_decode_points(ctx.handle, cid, bytes(64), 1, buf(), buf()) == INVALID
        assert lib.dr_te_fixed_base_msm_groups(ctx.handle, cid, bytes(64), 1, bytes(32), 1, buf()) == INVALID
        made = ctypes.c_void_p()
        assert lib.dr_ring_prover_create_te(ctx.handle, cid, None, 9, 8, bytes(64), bytes(64), bytes(64), bytes(64), ctypes.byref(made)) == INVALID
        assert not made.value
        suite = _native.vrf_suite(e.SUITE_ID, 2, bytes(64), bytes(64), cid)
        s = ctypes.byref(suite)
        assert lib.dr_hash_to_field_batch(s, b"a", off, 1, buf()) == INVALID
        assert lib.dr_encode_to_curve_batch(ctx.handle, s, b"a", off, None, None, 1, buf()) == INVALID
        assert lib.dr_pedersen_prove_batch(ctx.handle, s, 1, b"a", off, b"a", off, b"a", off, bytes(32), buf(), buf()) == INVALID
        assert lib.dr_pedersen_verify_batch(ctx.handle, s, 1, bytes(512), bytes(64), off, b"a", off, b"a", off, verdict) == INVALID
        for thin in (0, 1):
            assert lib.dr_ietf_prove_batch(ctx.handle, s, thin, 1, b"a", off, b"a", off, b"a", off, bytes(32), buf(), buf()) == INVALID
            assert lib.dr_ietf_verify_batch(ctx.handle, s, thin, 1, bytes(512), bytes(64), b"a", off, b"a", off, b"a", off, buf()) == INVALID
        with pytest.raises(ValueError):
            _native.blsg1_hash_to_field_batch(cid, [b"a"])
        with pytest.raises(ValueError):
            _native.blsg2_hash_to_field_batch(cid, [b"a"])
        with pytest.raises(ValueError):
            ctx.blsg1_encode_to_curve_batch(cid, [b"a"])
        with pytest.raises(ValueError):
            ctx.blsg2_encode_to_curve_batch(cid, [b"a"])
    for cid in (15, 17, 3):
        with pytest.raises(ValueError):
            ctx.ed448_encode_to_curve_batch(cid, [b"a"])
    for cv in (d.Ed448_RO, d.Ed448_NU):
        with pytest.raises(ValueError):
            d.RingVRF[cv]
        with pytest.raises(ValueError):
            d.RingProofParams(cv=cv)


def test_ed25519_and_g1_after_ed448_calls(ctx):
    """the context's io buffers and the worker threads are shared: after Ed448 calls on this context an Ed25519_RO proof still has the
    restatement's bytes and a G1 hash the vector file's"""
    import dot_ring_amd as d

    ctx.ed448_map_to_curve(_us([2, 3]), 2)
    ctx.ed448_scalar_mul_batch(e.raw(e.G) * 65, _sc([(1 << 440) - 1] * 65))
    sk, al, ad = (7).to_bytes(32, "little"), b"after ed448", b"ad"
    assert d.TinyVRF[d.Ed25519_RO].prove(al, sk, ad).encode() == h2c_ref.ED25519_RO.ietf_prove(sk, al, ad)
    vecs = json.load(open(os.path.join(GOLDEN, "h2c", "bls12_381_G1_ro.json")))["vectors"]
    out = ctx.blsg1_encode_to_curve_batch(15, [v["msg"].encode() for v in vecs])
    assert out == b"".join(int(v["P"]["x"], 16).to_bytes(48, "little") + int(v["P"]["y"], 16).to_bytes(48, "little") for v in vecs)
