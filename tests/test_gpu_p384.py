"""P-384 on the GPU (DR_CURVE_P384_RO = 25, DR_CURVE_P384_NU = 26; csrc/fp384.hip.h, csrc/p384_law.hip.h, csrc/kernels_p384.hip.h), bit
for bit against the big-integer restatement (p384_ref.py): the field selftest at the limb bounds of the contract with the images of
zero; the map of RFC 9380 on the vector files, at the three inputs of its exceptional branch, on a cancelling and a doubling pair; scalar
multiplication by every kind of 384-bit scalar, used as it is, on the generator, its negative, a point with x = 0, the identity and
random points; grouped MSMs (a group that cancels, one that repeats a point as Pedersen's G, G does, one with the identity); the SEC1
decoder; the Tiny / Thin / Pedersen VRFs byte for byte against the restatement (whose width handling test_p521_cpu.py pins on the
reference's P-256 proof files); the refusals; and a P-521 proof, a P-256 proof and a G1 hash afterwards.  96 zero bytes are the identity
in both directions.  Shapes: n in {1, 64, 65} — a tail lane, a full wave, a second workgroup — and one run of 300.  Every comparison is
exact."""
import ctypes
import json
import os
import random
import struct
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import h2c_ref  # noqa: E402
import p384_ref as r  # noqa: E402
import p521_ref  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
P, N = r.P, r.N
RO, NU = 25, 26
X0 = (0, r.sqrt(r.B))                                      # x = 0 is on the curve: b is a square
NIBBLES_7 = int("7" * 96, 16)
NIBBLES_8 = int("8" * 96, 16)                              # every digit -8 and a carry out of the top one: window 96
RECORDS = 13


def _h2c(variant):
    return json.load(open(os.path.join(GOLDEN, "h2c", f"p384_{variant}.json")))["vectors"]


def _base():
    return json.load(open(os.path.join(GOLDEN, "base", "p384_base_vectors.json")))


def _xy(v):
    return int(v["x"], 16), int(v["y"], 16)


def _us(values):
    return b"".join(int(u).to_bytes(48, "little") for u in values)


_sc = _us


def pts_of(blob):
    out = []
    for i in range(0, len(blob), 96):
        x, y = int.from_bytes(blob[i : i + 48], "little"), int.from_bytes(blob[i + 48 : i + 96], "little")
        out.append(None if x == 0 and y == 0 else (x, y))
    return out


@pytest.fixture(scope="module")
def randoms():
    rng = random.Random(384)
    return [r.mul(rng.randrange(1, N), r.G) for _ in range(3)]


# ---------------------------------------------------------------- the field
def test_field_selftest_at_the_limb_bounds(ctx):
    pairs = r.contract_pairs(random.Random(1))
    pack = lambda images: b"".join(struct.pack("<14i", *image) for image in images)  # noqa: E731
    out, flags = ctx.p384_field_selftest(pack([a for a, _ in pairs]), pack([b for _, b in pairs]))
    assert len(out) == len(pairs) * RECORDS * 48 and len(flags) == len(pairs)
    for i, (a, b) in enumerate(pairs):
        rec = [int.from_bytes(out[(RECORDS * i + j) * 48 : (RECORDS * i + j + 1) * 48], "little") for j in range(RECORDS)]
        e = r.field_expectations(a, b)
        assert rec[:8] == [e["mul"], e["sqr"], e["add"], e["sub"], e["neg"], e["a"], e["small4"], e["inv"]], (i, a[:2], b[:2])
        assert rec[9] == e["a"] and rec[10] == e["smallneg"]
        assert rec[11] == e["sqr"] and rec[12] == 2 * e["mul"] % P           # the square of the fold's output; the fused pair of products
        assert flags[i] == (1 if e["square"] else 0) | (2 if e["odd"] else 0) | (4 if e["zero"] else 0) | (8 if e["equal"] else 0)
        if e["square"]:
            assert rec[8] * rec[8] % P == e["a"]
    for image, value in r.SPELLED:                         # limbs that spell p, p + 1, 2^384, 2^392 - 1: those values over R
        i = next(j for j, (a, _) in enumerate(pairs) if a == image)
        assert int.from_bytes(out[(RECORDS * i + 9) * 48 : (RECORDS * i + 10) * 48], "little") == value


# ---------------------------------------------------------------- the map
@pytest.mark.parametrize("variant", ["ro", "nu"])
def test_map_reproduces_the_vectors(ctx, variant):
    vecs = _h2c(variant)
    per = 2 if variant == "ro" else 1
    us = [int(u, 16) for v in vecs for u in v["u"]]
    images = [r.map_to_curve(u) for u in us]
    recorded = [_xy(v[k]) for v in vecs for k in (("Q0", "Q1") if per == 2 else ("Q",))]
    assert recorded == images                              # every record, none excepted
    for clear in (False, True):                            # the cofactor is 1: `clear` changes nothing
        raw1, ok = ctx.p384_map_to_curve(_us(us), 1, clear=clear)
        assert ok == b"\x01" * len(us) and pts_of(raw1) == images
        raw2, ok = ctx.p384_map_to_curve(_us(us), per, clear=clear)
        assert ok == b"\x01" * len(vecs) and pts_of(raw2) == [_xy(v["P"]) for v in vecs]


def test_map_at_its_exceptional_inputs(ctx):
    us = [0, r.S, P - r.S, 1, P - 1, 2, P - 2]
    raw, ok = ctx.p384_map_to_curve(_us(us), 1)
    assert ok == b"\x01" * len(us) and pts_of(raw) == [r.map_to_curve(u) for u in us]
    x1 = r.B * pow(r.Z * r.A % P, -1, P) % P
    assert [pt[0] for pt in pts_of(raw)[:3]] == [x1] * 3   # tv1 = 0: all three land on B / (Z A)
    # map(p - u) = -map(u): the pair cancels to 96 zero bytes; (u, u) is a doubling through the addition
    pairs = [7, P - 7, 7, 7, r.S, P - r.S, 0, 0]
    raw, ok = ctx.p384_map_to_curve(_us(pairs), 2)
    q = r.map_to_curve(7)
    assert ok == b"\x01" * 4 and raw[:96] == bytes(96)
    assert pts_of(raw) == [None, r.add(q, q), None, r.add(r.map_to_curve(0), r.map_to_curve(0))]


@pytest.mark.parametrize("n", [1, 64, 65, 300])
def test_map_batch_sizes(ctx, n):
    rng = random.Random(n)
    us = [rng.randrange(P) for _ in range(n)]
    raw, ok = ctx.p384_map_to_curve(_us(us), 1)
    got = pts_of(raw)
    assert ok == b"\x01" * n and all(r.on_curve(pt) for pt in got)
    for i in sorted({0, n // 2, n - 1}):                   # (the restatement's map costs two exponentiations: three lanes of each run)
        assert got[i] == r.map_to_curve(us[i])
    raw2, _ = ctx.p384_map_to_curve(_us(us), 1)
    assert raw2 == raw


@pytest.mark.parametrize("variant", ["ro", "nu"])
def test_encode_to_curve_batch(ctx, variant):
    vecs = _h2c(variant)
    cid = RO if variant == "ro" else NU
    msgs = [v["msg"].encode() for v in vecs]
    assert pts_of(ctx.p384_encode_to_curve_batch(cid, msgs)) == [_xy(v["P"]) for v in vecs]
    salts = [b"", b"salt", b"", b"x" * 200, b"s"][: len(msgs)]
    e2c = r.encode_to_curve_ro if variant == "ro" else r.encode_to_curve_nu
    assert pts_of(ctx.p384_encode_to_curve_batch(cid, msgs, salts)) == [e2c(s + m) for s, m in zip(salts, msgs)]
    import dot_ring_amd as d

    cv = d.P384_RO if variant == "ro" else d.P384_NU
    pt = cv.point_type.encode_to_curve(msgs[1], b"salt")
    assert (pt.x, pt.y) == e2c(b"salt" + msgs[1])
    assert cv.point_type.map_to_curve_simple_swu(5).x == r.map_to_curve(5)[0]


# ---------------------------------------------------------------- scalar multiplication and MSMs
def test_scalar_mul_scalars_by_points_in_one_launch(ctx, randoms):
    rng = random.Random(2)
    scalars = [0, 1, 2, N - 1, N, N + 1, 1 << 383, (1 << 384) - 1, NIBBLES_7, NIBBLES_8, rng.randrange(1 << 384), rng.randrange(1 << 384)]
    points = [r.G, r.neg(r.G), X0, None] + randoms
    ks = [k for k in scalars for _ in points]
    ps = [pt for _ in scalars for pt in points]
    assert len(ks) == 84                                   # a full wave and a tail
    got = pts_of(ctx.p384_scalar_mul_batch(b"".join(r.raw(pt) for pt in ps), _sc(ks)))
    assert got == [r.mul(k % N, pt) for k, pt in zip(ks, ps)]


def test_msm_groups(ctx, randoms):
    rng = random.Random(3)
    for m in (1, 2, 63, 64):
        groups = 2 if m > 2 else 3
        pts = [randoms[i % 3] if i % 5 else r.G for i in range(groups * m)]
        ks = [rng.randrange(1 << 16) if i % 7 else rng.randrange(1 << 384) for i in range(groups * m)]     # (short ones: the restatement's time)
        got = pts_of(ctx.p384_msm_groups(b"".join(r.raw(pt) for pt in pts), _sc(ks), m))
        assert got == [r.msm(pts[g * m : g * m + m], [k % N for k in ks[g * m : g * m + m]]) for g in range(groups)]
    a, b = randoms[0], randoms[1]
    # a group that cancels, a group that repeats one point (Pedersen's x G + b G), a group that holds the identity
    pts = [a, r.neg(a), b, r.mul(5, b)] + [r.G, r.G, r.G, r.G] + [a, None, None, b]
    ks = [9, 9, 5, N - 1] + [11, 13, N - 24, 0] + [3, 12345, 0, 4]
    got = pts_of(ctx.p384_msm_groups(b"".join(r.raw(pt) for pt in pts), _sc(ks), 4))
    assert got == [None, None, r.add(r.mul(3, a), r.mul(4, b))]
    got = pts_of(ctx.p384_msm_groups(r.raw(r.G) * 2, _sc([11, 13]), 2))
    assert got == [r.mul(24, r.G)]


def test_python_msm_folds_70_terms(ctx, randoms):
    import dot_ring_amd as d

    rng = random.Random(4)
    pt = d.P384.point_type
    pts = [randoms[i % 3] for i in range(70)]
    ks = [rng.randrange(-5, 1 << 400) for _ in range(70)]
    got = pt.msm([pt(*p) for p in pts], ks)
    assert (got.x, got.y) == r.msm(pts, [k % N for k in ks])
    g = pt.generator_point()
    assert (g * N).is_identity() and g * (N + 2) == g + g and g * -1 == -g


# ---------------------------------------------------------------- the decoder
def test_decoder(ctx, randoms):
    good = [r.G, r.neg(r.G), X0, r.neg(X0)] + randoms
    assert {pt[1] & 1 for pt in good} == {0, 1}
    strings = [r.encode(pt) for pt in good]
    none = [x for x in range(2, 40) if r.sqrt(r.rhs(x)) is None][:4]                     # x on no point
    bad = [b"\x02" + P.to_bytes(48, "big"), b"\x03" + (P + 5).to_bytes(48, "big"), b"\x02" + b"\xff" * 48]
    bad += [b"\x02" + x.to_bytes(48, "big") for x in none]
    bad += [bytes([prefix]) + strings[0][1:] for prefix in (0x00, 0x04, 0x05)]
    bad += [bytes(49)]
    assert len(none) == 4
    for check in (False, True):
        raw, ok = ctx.p384_decode_points(b"".join(strings + bad), check)
        assert ok == b"\x01" * len(good) + b"\x00" * len(bad)
        assert pts_of(raw) == good + [None] * len(bad)
    assert [r.decode(s) for s in bad] == ["bad"] * len(bad) and [r.decode(s) for s in strings] == good
    for n in (1, 64, 65):                                                                # a tail lane, a full wave, a second workgroup
        many = ((strings + bad) * 4)[:n]
        raw, ok = ctx.p384_decode_points(b"".join(many), True)
        want = [r.decode(s) for s in many]
        assert ok == bytes(0 if w == "bad" else 1 for w in want) and pts_of(raw) == [None if w == "bad" else w for w in want]


# ---------------------------------------------------------------- the VRFs
def _records():
    return [(bytes.fromhex(v["sk"]), bytes.fromhex(v["alpha"]), bytes.fromhex(v["ad"])) for v in _base()]


@pytest.fixture(scope="module")
def restated():
    """the restatement's proofs of every (sk, alpha, ad) of the base file, computed once"""
    out = []
    for sk, alpha, ad in _records():
        out.append({"tiny": r.RO.ietf_prove(sk, alpha, ad), "thin": r.RO.ietf_prove(sk, alpha, ad, thin=True),
                    "pedersen": r.RO.pedersen_prove(sk, alpha, ad)})
    return out


def test_vrf_proofs_equal_the_restatement(restated):
    import dot_ring_amd as d

    cv = d.P384
    recs = _records()
    alphas, sks, ads = [x[1] for x in recs], [x[0] for x in recs], [x[2] for x in recs]
    tiny = d.TinyVRF[cv].prove_batch(alphas, sks, ads)
    thin = d.ThinVRF[cv].prove_batch(alphas, sks, ads)
    ped = d.PedersenVRF[cv].prove_batch(alphas, sks, ads)
    for i, (sk, alpha, ad) in enumerate(recs):
        x = int.from_bytes(sk, "little") % N
        pk = cv.public_key_from_secret(sk)
        assert pk == bytes.fromhex(_base()[i]["pk"]) == r.public_key(sk) and len(pk) == 49
        assert tiny[i].encode() == restated[i]["tiny"] and len(restated[i]["tiny"]) == 113
        assert thin[i].encode() == restated[i]["thin"] and len(restated[i]["thin"]) == 146
        assert ped[i].encode() == restated[i]["pedersen"][0] and len(restated[i]["pedersen"][0]) == 292
        assert ped[i]._blinding_factor == restated[i]["pedersen"][1]
        for scheme, proof in ((d.TinyVRF[cv], tiny[i]), (d.ThinVRF[cv], thin[i])):
            back = scheme.decode(proof.encode())
            assert back == proof and back.verify(pk, alpha, ad)
            assert r.ietf_verify(r.RO, pk, proof.encode(), alpha, ad, thin=scheme.THIN)
            assert scheme.proof_to_hash(proof.output_point) == r.RO.point_to_hash(r.mul(x, r.RO.e2c(alpha)))
        back = d.PedersenVRF[cv].decode(ped[i].encode())
        assert back.encode() == ped[i].encode() and back.verify(alpha, ad) and ped[i].verify_unblinding(pk, ped[i]._blinding_factor)
        assert r.pedersen_verify(r.RO, ped[i].encode(), alpha, ad)
    assert d.TinyVRF[cv].prove(alphas[0], sks[0], ads[0]) == tiny[0]


def test_vrf_over_the_nonuniform_variant():
    import dot_ring_amd as d

    cv = d.P384_NU
    sk, alpha, ad = _records()[1]
    pk = cv.public_key_from_secret(sk)
    tiny, thin, ped = d.TinyVRF[cv].prove(alpha, sk, ad), d.ThinVRF[cv].prove(alpha, sk, ad), d.PedersenVRF[cv].prove(alpha, sk, ad)
    assert tiny.encode() == r.NU.ietf_prove(sk, alpha, ad) and thin.encode() == r.NU.ietf_prove(sk, alpha, ad, thin=True)
    assert ped.encode() == r.NU.pedersen_prove(sk, alpha, ad)[0]
    assert tiny.verify(pk, alpha, ad) and thin.verify(pk, alpha, ad) and ped.verify(alpha, ad)
    assert tiny.encode() != d.TinyVRF[d.P384_RO].prove(alpha, sk, ad).encode()


def _flip(blob, byte, bit=0):
    out = bytearray(blob)
    out[byte] ^= 1 << bit
    return bytes(out)


def test_spoiled_proofs_do_not_verify(restated):
    import dot_ring_amd as d

    cv = d.P384
    sk, alpha, ad = _records()[1]
    pk = cv.public_key_from_secret(sk)
    other_pk = cv.public_key_from_secret(b"\x05" * 48)
    for scheme, blob in ((d.TinyVRF[cv], restated[1]["tiny"]), (d.ThinVRF[cv], restated[1]["thin"])):
        proof = scheme.decode(blob)
        assert proof.verify(pk, alpha, ad)
        assert not proof.verify(pk, alpha + b"x", ad) and not proof.verify(pk, alpha, ad + b"x") and not proof.verify(other_pk, alpha, ad)
        assert not scheme.decode(_flip(blob, len(blob) - 48)).verify(pk, alpha, ad)                      # s
        assert not scheme.decode(_flip(blob, 0)).verify(pk, alpha, ad)                                   # O: the other root
        assert not scheme.decode(_flip(blob, 49)).verify(pk, alpha, ad)                                  # Thin: R, the other root; Tiny: c
        with pytest.raises(ValueError):
            scheme.decode(b"\x00" + blob[1:])                                                             # no 49-byte string is the identity
        with pytest.raises(ValueError, match="scalar is not canonical"):
            scheme.decode(blob[:-48] + N.to_bytes(48, "little"))
        with pytest.raises(ValueError, match="proof length"):
            scheme.decode(blob[:-1])
    blob = restated[1]["pedersen"][0]
    proof = d.PedersenVRF[cv].decode(blob)
    assert proof.verify(alpha, ad) and not proof.verify(alpha + b"x", ad) and not proof.verify(alpha, ad + b"x")
    for at in (0, 49, 98, 147, 196, 244):                                                                 # O, Y_bar, R, O_k, s, s_b
        assert not d.PedersenVRF[cv].decode(_flip(blob, at)).verify(alpha, ad)
    assert not proof.verify_unblinding(other_pk, restated[1]["pedersen"][1])
    assert cv.point_type.identity().point_to_string() == b"\x00"


def test_batch_verify(restated):
    import dot_ring_amd as d

    cv = d.P384
    recs = _records()[:3]
    alphas, ads = [x[1] for x in recs], [x[2] for x in recs]
    pks = [cv.public_key_from_secret(x[0]) for x in recs]
    thin = [d.ThinVRF[cv].decode(restated[i]["thin"]) for i in range(3)]
    assert d.ThinVRF[cv].batch_verify(thin, pks, alphas, ads)
    assert not d.ThinVRF[cv].batch_verify(thin, pks, [alphas[0], alphas[1] + b"x", alphas[2]], ads)
    spoiled = [thin[0], d.ThinVRF[cv].decode(_flip(restated[1]["thin"], 98)), thin[2]]
    assert not d.ThinVRF[cv].batch_verify(spoiled, pks, alphas, ads)
    ped = [d.PedersenVRF[cv].decode(restated[i]["pedersen"][0]) for i in range(3)]
    assert d.PedersenVRF[cv].batch_verify(ped, alphas, ads)
    assert not d.PedersenVRF[cv].batch_verify(ped, alphas, [ads[0], ads[1], ads[2] + b"x"])
    spoiled = [ped[0], ped[1], d.PedersenVRF[cv].decode(_flip(restated[2]["pedersen"][0], 196))]
    assert not d.PedersenVRF[cv].batch_verify(spoiled, alphas, ads)


# ---------------------------------------------------------------- refusals and regressions
def test_refusals(ctx):
    import dot_ring_amd as d
    from dot_ring_amd import _native

    g = r.raw(r.G)
    with pytest.raises(ValueError, match="not a canonical field element"):
        ctx.p384_scalar_mul_batch(P.to_bytes(48, "little") + g[48:], _sc([1]))
    with pytest.raises(ValueError, match="not a canonical field element"):
        ctx.p384_scalar_mul_batch(g[:48] + b"\xff" * 48, _sc([1]))
    with pytest.raises(ValueError, match="not a canonical field element"):
        ctx.p384_map_to_curve(_us([P]), 1)
    with pytest.raises(ValueError):
        ctx.p384_map_to_curve(_us([1, 2, 3]), 3)
    for cid in (15, 17, 19, 21, 22, 23, 24, 4, 8):
        with pytest.raises(ValueError, match="DR_CURVE_P384_RO or DR_CURVE_P384_NU"):
            ctx.p384_encode_to_curve_batch(cid, [b"a"])
        with pytest.raises(ValueError):
            _native.p384_hash_to_field_batch(cid, [b"a"])
    lib = _native.lib()
    INVALID = _native.DR_ERR_INVALID
    off = (ctypes.c_uint64 * 2)(0, 1)
    buf = lambda n=1024: ctypes.create_string_buffer(n)  # noqa: E731
    for cid in (RO, NU):
        assert lib.dr_te_scalar_mul_batch(ctx.handle, cid, bytes(64), bytes(32), 1, buf()) == INVALID
        assert lib.dr_te_msm_groups(ctx.handle, cid, bytes(64), bytes(32), 1, 1, buf()) == INVALID
        assert lib.dr_te_decode_points(ctx.handle, cid, bytes(64), 1, buf(), buf()) == INVALID
        suite = _native.vrf_suite(r.SUITE_ID, 0, bytes(64), bytes(64), cid)
        s = ctypes.byref(suite)
        assert lib.dr_hash_to_field_batch(s, b"a", off, 1, buf()) == INVALID
        assert lib.dr_encode_to_curve_batch(ctx.handle, s, b"a", off, None, None, 1, buf()) == INVALID
        for hash_only in (_native.blsg1_hash_to_field_batch, _native.blsg2_hash_to_field_batch, _native.ed448_hash_to_field_batch,
                          _native.curve448_hash_to_field_batch, _native.p521_hash_to_field_batch):
            with pytest.raises(ValueError):
                hash_only(cid, [b"a"])
        for encode in (ctx.blsg1_encode_to_curve_batch, ctx.ed448_encode_to_curve_batch, ctx.curve448_encode_to_curve_batch,
                       ctx.p521_encode_to_curve_batch):
            with pytest.raises(ValueError):
                encode(cid, [b"a"])
    for cv in (d.P384_RO, d.P384_NU):
        with pytest.raises(ValueError):
            d.RingVRF[cv]
        with pytest.raises(ValueError):
            d.RingProofParams(cv=cv)


def test_p521_p256_and_g1_after_p384_calls(ctx):
    """the context's io buffers and the worker threads are shared: after P-384 calls on this context a P-521 proof and a P-256 proof
    still have their restatements' bytes and a G1 hash the vector file's"""
    import dot_ring_amd as d

    ctx.p384_map_to_curve(_us([2, 3]), 2)
    ctx.p384_scalar_mul_batch((r.raw(r.G) + bytes(96)) * 33, _sc([(1 << 384) - 1] * 66))
    sk, al, ad = bytes(range(1, 58)), b"after p384", b"ad"
    assert d.TinyVRF[d.P521].prove(al, sk, ad).encode() == p521_ref.RO.ietf_prove(sk, al, ad)
    sk = (7).to_bytes(32, "little")
    assert d.TinyVRF[d.P256_RO].prove(al, sk, ad).encode() == h2c_ref.P256_RO.ietf_prove(sk, al, ad)
    vecs = json.load(open(os.path.join(GOLDEN, "h2c", "bls12_381_G1_ro.json")))["vectors"]
    out = ctx.blsg1_encode_to_curve_batch(15, [v["msg"].encode() for v in vecs])
    assert out == b"".join(int(v["P"]["x"], 16).to_bytes(48, "little") + int(v["P"]["y"], 16).to_bytes(48, "little") for v in vecs)
