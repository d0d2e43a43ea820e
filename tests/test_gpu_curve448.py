"""Curve448 on the GPU (DR_CURVE_CURVE448_RO = 21, DR_CURVE_CURVE448_NU = 22; csrc/c448_law.hip.h and csrc/kernels_curve448.hip.h): the
map of RFC 9380 against the vector files and the big-integer restatement (curve448_ref.py), with the valueless inputs, the input that
maps to (0, 0) and a pair of inputs whose images cancel; scalar multiplication by 448-bit scalars used as they are on points of every
kind the law treats apart — the generator, a hashed point, G + (0, 0), a point of order 4 n, (0, 0), a point of order 4 and the
identity; grouped MSMs; the decoder in both modes; the Tiny / Thin / Pedersen VRFs byte for byte against the restatement (whose XOF and
width handling test_curve448_cpu.py pins on the reference's Bandersnatch SHAKE128 files); the refusals; and an Ed448 proof, a
Curve25519 proof and a G1 hash afterwards.  The identity travels as 112 bytes of 0xff in both directions at every entry point.
Shapes: n in {1, 64, 65} — a tail lane, a full wave, a second workgroup — and one run of 300.  Every comparison is exact."""
import ctypes
import json
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import curve25519_ref  # noqa: E402
import curve448_ref as c  # noqa: E402
import ed448_ref  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
P, N, A = c.P, c.N, c.A
RO, NU = 21, 22
FF = b"\xff" * 112
G_PLUS_TWO = c.add(c.G, c.TWO_TORSION)
OUTSIDE = c.add(c.G, c.T4)                                 # order 4 n
NOT_A_POINT = {("nu", 2, "Q")}                             # a record with a 111-digit y (test_curve448_cpu.py shows that it is no point)


def _h2c(variant):
    return json.load(open(os.path.join(GOLDEN, "h2c", f"curve448_{variant}.json")))["vectors"]


def _base():
    return json.load(open(os.path.join(GOLDEN, "base", "curve448_base_vectors.json")))


def _xy(v):
    return int(v["x"], 16), int(v["y"], 16)


def _us(values):
    return b"".join(int(u).to_bytes(56, "little") for u in values)


_sc = _us


def raw(pt):
    return FF if pt is None else c.raw(pt)


def pts_of(blob):
    """the identity is 112 bytes of 0xff and nothing else"""
    out = []
    for i in range(0, len(blob), 112):
        rec = blob[i : i + 112]
        out.append(None if rec == FF else (int.from_bytes(rec[:56], "little"), int.from_bytes(rec[56:], "little")))
    return out


@pytest.fixture(scope="module")
def hashed():
    return c.encode_to_curve_ro(b"a hashed point")


# ---------------------------------------------------------------- the map
@pytest.mark.parametrize("variant", ["ro", "nu"])
def test_map_reproduces_the_vectors(ctx, variant):
    vecs = _h2c(variant)
    per = 2 if variant == "ro" else 1
    us = [int(u, 16) for v in vecs for u in v["u"]]
    images = [c.map_to_curve(u) for u in us]
    recorded = [(i, k) for i, v in enumerate(vecs) for k in (("Q0", "Q1") if per == 2 else ("Q",))]
    for (i, k), img in zip(recorded, images):
        if (variant, i, k) not in NOT_A_POINT:
            assert _xy(vecs[i][k]) == img
    raw1, ok = ctx.curve448_map_to_curve(_us(us), 1, clear=False)               # u -> Q0 / Q1 / Q
    assert pts_of(raw1) == images and set(ok) == {1}
    out, ok = ctx.curve448_map_to_curve(_us(us), per, clear=True)               # -> P
    assert pts_of(out) == [_xy(v["P"]) for v in vecs] and set(ok) == {1}
    out, ok = ctx.curve448_map_to_curve(_us(us), per, clear=False)
    assert pts_of(out) == [images[i] if per == 1 else c.add(images[2 * i], images[2 * i + 1]) for i in range(len(vecs))]
    out, ok = ctx.curve448_map_to_curve(_us(us), 1, clear=True)
    assert pts_of(out) == [c.mul(4, q) for q in images]
    if per == 2:
        out, ok = ctx.curve448_map_to_curve(_us(us[:8]), 2, clear=True)         # per_item 2 on another grouping
        assert pts_of(out) == [c.mul(4, c.add(images[2 * i], images[2 * i + 1])) for i in range(4)]


def test_map_inputs_without_a_value_and_the_one_that_maps_to_the_two_torsion(ctx):
    import dot_ring_amd as d

    us = [0, 1, P - 1, 2, P - 2, 3]
    out, ok = ctx.curve448_map_to_curve(_us(us), 1, clear=False)
    assert list(ok) == [1, 0, 0, 1, 1, 1] and out[: 3 * 112] == bytes(3 * 112)  # u = 0 -> (0, 0) with ok = 1; u = +-1: zero bytes, ok = 0
    assert pts_of(out)[3:] == [c.map_to_curve(u) for u in us[3:]] and c.map_to_curve(0) == (0, 0)
    out, ok = ctx.curve448_map_to_curve(_us([0]), 1, clear=True)                # 4 (0, 0) = O
    assert list(ok) == [1] and out == FF
    out, ok = ctx.curve448_map_to_curve(_us([2, 1, P - 1, 3, 4, 5, 0, 6]), 2, clear=True)    # one valueless element spoils its item
    assert list(ok) == [0, 0, 1, 1] and out[: 2 * 112] == bytes(2 * 112)
    assert pts_of(out)[2:] == [c.mul(4, c.add(c.map_to_curve(4), c.map_to_curve(5))), c.mul(4, c.add((0, 0), c.map_to_curve(6)))]
    pt = d.Curve448.point_type
    for u in (1, P - 1):
        with pytest.raises(ValueError, match="No inverse exists"):
            pt.map_to_curve(u)
    assert pt.map_to_curve(0) == pt(0, 0)
    q = pt.map_to_curve(2)
    assert (q.x, q.y) == c.map_to_curve(2)
    for bad in (_us([P]), _us([2**448 - 1])):
        with pytest.raises(ValueError):
            ctx.curve448_map_to_curve(bad, 1)
    with pytest.raises(ValueError):
        ctx.curve448_map_to_curve(_us([1, 2, 3]), 3)


def _cancelling_pair():
    """(u, u') with map(u') = -map(u).  -Q is not the image of -u (the map depends on u^2 alone), but an x that is the x1 of u is also
    the x2 of u' with u'^2 = 1 - A / (x + A) whenever that is a square, and the two routes fix opposite parities of y."""
    rng = random.Random(448)
    for _ in range(64):
        u = rng.randrange(2, P - 1)
        x, y = c.map_to_curve(u)
        if (x * (1 - u * u) + A) % P:                       # x is the x2 of u: try the next
            continue
        w = c.sqrt(1 - A * pow(x + A, -1, P))
        if w is not None and c.map_to_curve(w) == (x, -y % P):
            return u, w
    return None


def test_map_pairs_that_double_and_a_pair_that_cancels(ctx):
    u = 0x1234567
    img = c.map_to_curve(u)
    assert c.map_to_curve(P - u) == img
    out, ok = ctx.curve448_map_to_curve(_us([u, u, u, P - u]), 2, clear=False)
    assert pts_of(out) == [c.add(img, img)] * 2 and list(ok) == [1, 1]
    pair = _cancelling_pair()
    assert pair is not None                                                      # (found at the seed above)
    for clear in (False, True):
        out, ok = ctx.curve448_map_to_curve(_us([*pair, pair[1], pair[0], pair[0], 5]), 2, clear=clear)
        assert list(ok) == [1, 1, 1] and out[:224] == FF * 2                     # the identity as 0xff, with a value
        rest = c.add(c.map_to_curve(pair[0]), c.map_to_curve(5))
        assert pts_of(out)[2] == (c.mul(4, rest) if clear else rest)


@pytest.mark.parametrize("n", [1, 64, 65])
def test_map_against_the_restatement(ctx, n):
    rng = random.Random(n)
    us = [rng.randrange(P) for _ in range(2 * n)]
    out, ok = ctx.curve448_map_to_curve(_us(us), 2)
    assert set(ok) == {1}
    assert pts_of(out) == [c.mul(4, c.add(c.map_to_curve(us[2 * i]), c.map_to_curve(us[2 * i + 1]))) for i in range(n)]


def test_map_300_elements_and_clearing_is_multiplication_by_four(ctx):
    rng = random.Random(300)
    us = [rng.randrange(P) for _ in range(300)]
    out, ok = ctx.curve448_map_to_curve(_us(us), 1, clear=False)
    assert set(ok) == {1} and pts_of(out) == [c.map_to_curve(u) for u in us]
    cleared, _ = ctx.curve448_map_to_curve(_us(us), 1, clear=True)
    assert ctx.curve448_scalar_mul_batch(out, _sc([4] * 300)) == cleared


@pytest.mark.parametrize("variant,cid", [("ro", RO), ("nu", NU)])
def test_encode_to_curve_batch(ctx, variant, cid):
    import dot_ring_amd as d

    vecs = _h2c(variant)
    out = ctx.curve448_encode_to_curve_batch(cid, [v["msg"].encode() for v in vecs])
    assert pts_of(out) == [_xy(v["P"]) for v in vecs]
    fn = c.encode_to_curve_ro if cid == RO else c.encode_to_curve_nu
    rng = random.Random(cid)
    msgs = [rng.randbytes(n) for n in (0, 1, 83, 217, 517)]
    salts = [rng.randbytes(1 + i) for i in range(len(msgs))]
    assert pts_of(ctx.curve448_encode_to_curve_batch(cid, msgs, salts)) == [fn(s + m) for m, s in zip(msgs, salts)]
    cv = d.Curve448_RO if cid == RO else d.Curve448_NU
    got = cv.point_type.encode_to_curve_batch(msgs[:3], salts[:3])
    assert [(p.x, p.y) for p in got] == [fn(s + m) for m, s in zip(msgs[:3], salts[:3])]
    one = cv.point_type.encode_to_curve(msgs[1])
    assert (one.x, one.y) == fn(msgs[1])
    assert cv.point_type.encode_to_curve_from_field(cv.point_type.hash_to_field_pairs(msgs[:2], salts[:2])) == got[:2]
    # a valueless element: DR_ERR_INVALID from the library's own round (the map's flags), the reference's text in Python
    from dot_ring_amd import _native
    with pytest.raises(ValueError, match="No inverse exists"):
        cv.point_type.encode_to_curve_from_field(_us([2, 1] if cid == RO else [P - 1]))
    assert _native.DR_ERR_INVALID == -1
    with pytest.raises(ValueError):
        ctx.curve448_encode_to_curve_batch(19, [b"a"])


# ---------------------------------------------------------------- scalar multiplication
# the last two: every nibble 7 (the largest digit everywhere, no carry) and every nibble 8 (a carry out of every digit, up into window 113)
SCALARS = [0, 1, 2, 4, N - 1, N, N + 1, 2 * N, 4 * N - 1, 4 * N, 2**447, 2**448 - 1, int("7" * 112, 16), int("8" * 112, 16)]


def test_scalar_mul_takes_scalars_as_they_are(ctx, hashed):
    bases = [c.G, hashed, G_PLUS_TWO, OUTSIDE, c.TWO_TORSION, c.T4, None]
    pts = [b for b in bases for _ in SCALARS]
    got = pts_of(ctx.curve448_scalar_mul_batch(b"".join(raw(p) for p in pts), _sc(SCALARS * len(bases))))   # 98 items
    for j, base in enumerate(bases):
        assert got[len(SCALARS) * j : len(SCALARS) * (j + 1)] == [c.mul(k, base) for k in SCALARS], j
    at = lambda j, k: got[len(SCALARS) * j + SCALARS.index(k)]  # noqa: E731
    assert at(0, N) is None and at(0, N + 1) == c.G and at(0, 0) is None
    # n Q != O outside the subgroup: a device that reduced mod n would answer O for k = n and Q for k = n + 1
    assert at(3, N) == c.mul(N % 4, c.T4) and at(3, N + 1) != OUTSIDE and at(3, 4 * N) is None and at(3, 2 * N) == c.TWO_TORSION
    assert at(2, N) == c.TWO_TORSION and at(4, 1) == (0, 0) and at(4, 2) is None and at(5, 2) == (0, 0) and at(5, 4) is None
    assert all(at(6, k) is None for k in SCALARS)


@pytest.mark.parametrize("n", [1, 64, 65, 300])
def test_scalar_mul_batches(ctx, hashed, n):
    rng = random.Random(n)
    bases = [c.G, hashed, OUTSIDE, None, c.TWO_TORSION, c.neg(c.T4), G_PLUS_TWO]
    pts = [bases[i % len(bases)] for i in range(n)]
    ks = [rng.randrange(2**448) for _ in range(n)]
    got = pts_of(ctx.curve448_scalar_mul_batch(b"".join(raw(p) for p in pts), _sc(ks)))
    check = range(n) if n <= 65 else rng.sample(range(n), 40)
    for i in check:
        assert got[i] == c.mul(ks[i], pts[i]), i
    with pytest.raises(ValueError):
        ctx.curve448_scalar_mul_batch(_us([P, 1]), _sc([1]))
    with pytest.raises(ValueError):
        ctx.curve448_scalar_mul_batch(b"\xff" * 111 + b"\xfe", _sc([1]))          # all but the identity's bytes: a coordinate above p


def test_python_mul_is_exact_for_every_integer(hashed):
    import dot_ring_amd as d

    pt = d.Curve448.point_type
    as_t = lambda p: None if p.is_identity() else (p.x, p.y)  # noqa: E731
    g, q = pt.generator_point(), pt(*OUTSIDE)
    for k in (0, 1, N - 1, N, N + 5, 4 * N, 4 * N + 3, 2**448 + 3, -1, -N):
        assert as_t(g * k) == c.mul(k, c.G)
        assert as_t(q * k) == c.mul(k, OUTSIDE)                                   # MGAffinePoint.__mul__ does not reduce mod n
    assert 3 * g == g * 3 and (pt.identity() * 5).is_identity() and as_t(pt(0, 0) * 3) == (0, 0)
    many = d.curve.scalar_mul_batch([g, pt(*hashed), pt.identity()], [N + 2, 7, 9])
    assert [as_t(p) for p in many] == [c.mul(2, c.G), c.mul(7, hashed), None]
    assert as_t(q.clear_cofactor()) == c.mul(4, OUTSIDE)


@pytest.mark.parametrize("m", [1, 2, 63, 64])
def test_msm_groups(ctx, hashed, m):
    rng = random.Random(m)
    groups = 3 if m < 63 else 2
    bases = [c.G, hashed, OUTSIDE, None, c.TWO_TORSION, c.T4]
    pts = [bases[rng.randrange(len(bases))] for _ in range(groups * m)]
    ks = [rng.randrange(2**448) if i % 5 else rng.randrange(16) for i in range(groups * m)]
    got = pts_of(ctx.curve448_msm_groups(b"".join(raw(p) for p in pts), _sc(ks), m))
    assert got == [c.msm(pts[g * m : (g + 1) * m], ks[g * m : (g + 1) * m]) for g in range(groups)]
    with pytest.raises(ValueError):
        ctx.curve448_msm_groups(c.raw(c.G) * 65, _sc([1] * 65), 65)


def test_msm_groups_that_cancel_repeat_and_hold_the_identity(ctx, hashed):
    k = 2**447 + 12345
    groups = [
        ([hashed, c.neg(hashed)], [k, k]),                                        # P and -P with equal scalars: the identity
        ([c.TWO_TORSION, c.TWO_TORSION], [1, 1]),                                 # (0, 0) twice: the identity
        ([c.TWO_TORSION, c.TWO_TORSION], [1, 2]),                                 # (0, 0)
        ([None, c.G], [7, 3]),
        ([None, None], [1, 2]),
        ([c.G, c.G], [5, N - 5]),
        ([c.T4, c.neg(c.T4)], [1, 3]),                                            # T4 + 3 (-T4) = -2 T4 = (0, 0)
    ]
    pts = [p for g in groups for p in g[0]]
    ks = [s for g in groups for s in g[1]]
    got = pts_of(ctx.curve448_msm_groups(b"".join(raw(p) for p in pts), _sc(ks), 2))
    assert got == [c.msm(*g) for g in groups] == [None, None, (0, 0), c.mul(3, c.G), None, None, (0, 0)]


def test_python_msm_folds_beyond_64_terms(hashed):
    import dot_ring_amd as d

    pt = d.Curve448.point_type
    rng = random.Random(70)
    pts = [c.G, hashed] * 35
    ks = [rng.randrange(N) for _ in range(70)]
    want = c.msm(pts, ks)
    points = [pt(*p) for p in pts]
    r = pt.msm(points, ks)
    assert (r.x, r.y) == want
    (r2,) = d.curve.msm_groups(points, ks, 70)
    assert r2 == r
    assert pt.msm([], []) == pt.identity()
    pair = d.curve.msm_groups(points[:4], [1, 2, -3, N + 4], 2)
    assert [(p.x, p.y) for p in pair] == [c.msm(pts[:2], [1, 2]), c.msm(pts[2:4], [-3, 4])]
    assert pt.msm([points[1], -points[1]], [9, 9]).is_identity()


# ---------------------------------------------------------------- the decoder
def test_decoder(ctx, hashed):
    import dot_ring_amd as d
    from dot_ring_amd.vrf.codec import dec_point, dec_points

    off_curve = (5, 5)
    cases = [raw(off_curve), _us([P, 0]), _us([0, P + 1]), raw(c.TWO_TORSION), raw(c.T4), raw(OUTSIDE), FF, raw(c.G), raw(hashed),
             raw(G_PLUS_TWO)]
    blob = b"".join(cases)
    out, ok = ctx.curve448_decode_points(blob, check=False)
    assert list(ok) == [0, 0, 0, 1, 1, 1, 0, 1, 1, 1]
    out1, ok1 = ctx.curve448_decode_points(blob, check=True)
    assert list(ok1) == [0, 0, 0, 0, 0, 0, 0, 1, 1, 0]
    for o, flags in ((out, ok), (out1, ok1)):
        for i, f in enumerate(flags):
            assert o[112 * i : 112 * i + 112] == (cases[i] if f else bytes(112))
    assert [c.decode(x) != "bad" for x in cases] == [bool(f) for f in ok] and [c.decode(x, check=True) != "bad" for x in cases] == [bool(f) for f in ok1]
    for n in (1, 64, 65):
        pts = [c.G if i % 3 else OUTSIDE for i in range(n)]
        _, flags = ctx.curve448_decode_points(b"".join(raw(p) for p in pts), check=True)
        assert list(flags) == [1 if i % 3 else 0 for i in range(n)]
    cv = d.Curve448
    assert [(p.x, p.y) for p in dec_points(cv, [raw(c.G), raw(hashed)])] == [c.G, hashed]
    for bad, text in ((raw(c.TWO_TORSION), "not a valid nonidentity subgroup point"), (raw(OUTSIDE), "not a valid nonidentity subgroup point"),
                      (raw(off_curve), "Point is not on the curve"), (_us([P, 1]), "Invalid point coordinates"), (FF, "Invalid point coordinates"),
                      (raw(c.G)[:111], "point must be exactly 112 bytes")):
        with pytest.raises(ValueError, match=text):
            dec_point(cv, bad)
    pt = cv.point_type
    assert d.curve.valid_points([pt(*c.G), pt(*OUTSIDE), pt.identity(), pt(*hashed), pt(0, 0)]) == [True, False, False, True, False]
    assert cv.curve.valid_point(pt(*hashed)) and not cv.curve.valid_point(pt(*c.T4))


# ---------------------------------------------------------------- the VRFs
def _records():
    return [(bytes.fromhex(v["sk"]), bytes.fromhex(v["alpha"]), bytes.fromhex(v["ad"])) for v in _base()]


@pytest.fixture(scope="module")
def restated():
    """the restatement's proofs of every (sk, alpha, ad) of the base file, computed once"""
    out = []
    for sk, alpha, ad in _records():
        out.append({"tiny": c.RO.ietf_prove(sk, alpha, ad), "thin": c.RO.ietf_prove(sk, alpha, ad, thin=True),
                    "pedersen": c.RO.pedersen_prove(sk, alpha, ad)})
    return out


def test_vrf_proofs_equal_the_restatement(restated):
    import dot_ring_amd as d

    cv = d.Curve448
    recs = _records()
    alphas, sks, ads = [r[1] for r in recs], [r[0] for r in recs], [r[2] for r in recs]
    tiny = d.TinyVRF[cv].prove_batch(alphas, sks, ads)
    thin = d.ThinVRF[cv].prove_batch(alphas, sks, ads)
    ped = d.PedersenVRF[cv].prove_batch(alphas, sks, ads)
    for i, (sk, alpha, ad) in enumerate(recs):
        x = int.from_bytes(sk, "little") % N
        pk = cv.public_key_from_secret(sk)
        assert pk == c.raw(c.mul(x, c.G)) and len(pk) == 112
        # the lengths are the restatement's: 112-byte points, 56-byte scalars, the 16-byte challenge of every suite
        assert tiny[i].encode() == restated[i]["tiny"] and len(restated[i]["tiny"]) == 112 + 16 + 56
        assert thin[i].encode() == restated[i]["thin"] and len(restated[i]["thin"]) == 112 + 112 + 56
        assert ped[i].encode() == restated[i]["pedersen"][0] and len(restated[i]["pedersen"][0]) == 4 * 112 + 2 * 56
        assert ped[i]._blinding_factor == restated[i]["pedersen"][1]
        for scheme, proof in ((d.TinyVRF[cv], tiny[i]), (d.ThinVRF[cv], thin[i])):
            back = scheme.decode(proof.encode())
            assert back == proof and back.verify(pk, alpha, ad)
            assert c.ietf_verify(c.RO, pk, proof.encode(), alpha, ad, thin=scheme.THIN)
            assert scheme.proof_to_hash(proof.output_point) == c.RO.point_to_hash(c.mul(x, c.RO.e2c(alpha)))
        back = d.PedersenVRF[cv].decode(ped[i].encode())
        assert back.encode() == ped[i].encode() and back.verify(alpha, ad) and ped[i].verify_unblinding(pk, ped[i]._blinding_factor)
        assert c.pedersen_verify(c.RO, ped[i].encode(), alpha, ad)
    assert d.TinyVRF[cv].prove(alphas[0], sks[0], ads[0]) == tiny[0]


def test_vrf_over_the_nonuniform_variant():
    import dot_ring_amd as d

    cv = d.Curve448_NU
    sk, alpha, ad = _records()[1]
    pk = cv.public_key_from_secret(sk)
    tiny, thin, ped = d.TinyVRF[cv].prove(alpha, sk, ad), d.ThinVRF[cv].prove(alpha, sk, ad), d.PedersenVRF[cv].prove(alpha, sk, ad)
    assert tiny.encode() == c.NU.ietf_prove(sk, alpha, ad) and thin.encode() == c.NU.ietf_prove(sk, alpha, ad, thin=True)
    assert ped.encode() == c.NU.pedersen_prove(sk, alpha, ad)[0]
    assert tiny.verify(pk, alpha, ad) and thin.verify(pk, alpha, ad) and ped.verify(alpha, ad)
    assert tiny.encode() != d.TinyVRF[d.Curve448_RO].prove(alpha, sk, ad).encode()


def _flip(blob, byte, bit=0):
    out = bytearray(blob)
    out[byte] ^= 1 << bit
    return bytes(out)


def test_spoiled_proofs_do_not_verify(restated):
    import dot_ring_amd as d

    cv = d.Curve448
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
        with pytest.raises(ValueError):
            scheme.decode(FF + blob[112:])                                                                # the identity has no encoding
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
    with pytest.raises(ValueError, match="Cannot serialize point at infinity"):
        cv.point_type.identity().point_to_string()


def test_batch_verify(restated):
    import dot_ring_amd as d

    cv = d.Curve448
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
def test_ids_21_and_22_are_refused_elsewhere(ctx):
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
        suite = _native.vrf_suite(c.SUITE_ID, 2, bytes(64), bytes(64), cid)
        s = ctypes.byref(suite)
        assert lib.dr_hash_to_field_batch(s, b"a", off, 1, buf()) == INVALID
        assert lib.dr_encode_to_curve_batch(ctx.handle, s, b"a", off, None, None, 1, buf()) == INVALID
        assert lib.dr_pedersen_prove_batch(ctx.handle, s, 1, b"a", off, b"a", off, b"a", off, bytes(32), buf(), buf()) == INVALID
        assert lib.dr_pedersen_verify_batch(ctx.handle, s, 1, bytes(512), bytes(64), off, b"a", off, b"a", off, verdict) == INVALID
        for thin in (0, 1):
            assert lib.dr_ietf_prove_batch(ctx.handle, s, thin, 1, b"a", off, b"a", off, b"a", off, bytes(32), buf(), buf()) == INVALID
            assert lib.dr_ietf_verify_batch(ctx.handle, s, thin, 1, bytes(512), bytes(64), b"a", off, b"a", off, b"a", off, buf()) == INVALID
        for hash_only in (_native.blsg1_hash_to_field_batch, _native.blsg2_hash_to_field_batch, _native.ed448_hash_to_field_batch):
            with pytest.raises(ValueError):
                hash_only(cid, [b"a"])
        for encode in (ctx.blsg1_encode_to_curve_batch, ctx.blsg2_encode_to_curve_batch, ctx.ed448_encode_to_curve_batch):
            with pytest.raises(ValueError):
                encode(cid, [b"a"])
    for cid in (15, 17, 19, 20, 3, 13):
        with pytest.raises(ValueError):
            ctx.curve448_encode_to_curve_batch(cid, [b"a"])
    for cv in (d.Curve448_RO, d.Curve448_NU):
        with pytest.raises(ValueError):
            d.RingVRF[cv]
        with pytest.raises(ValueError):
            d.RingProofParams(cv=cv)


def test_ed448_curve25519_and_g1_after_curve448_calls(ctx):
    """the context's io buffers and the worker threads are shared: after Curve448 calls on this context an Ed448 proof and a Curve25519
    proof still have their restatements' bytes and a G1 hash the vector file's"""
    import dot_ring_amd as d

    ctx.curve448_map_to_curve(_us([2, 3]), 2)
    ctx.curve448_scalar_mul_batch((c.raw(c.G) + FF) * 33, _sc([(1 << 440) - 1] * 66))
    sk, al, ad = bytes(range(1, 58)), b"after curve448", b"ad"
    assert d.TinyVRF[d.Ed448].prove(al, sk, ad).encode() == ed448_ref.RO.ietf_prove(sk, al, ad)
    sk = (7).to_bytes(32, "little")
    assert d.TinyVRF[d.Curve25519].prove(al, sk, ad).encode() == curve25519_ref.RO.ietf_prove(sk, al, ad)
    vecs = json.load(open(os.path.join(GOLDEN, "h2c", "bls12_381_G1_ro.json")))["vectors"]
    out = ctx.blsg1_encode_to_curve_batch(15, [v["msg"].encode() for v in vecs])
    assert out == b"".join(int(v["P"]["x"], 16).to_bytes(48, "little") + int(v["P"]["y"], 16).to_bytes(48, "little") for v in vecs)
