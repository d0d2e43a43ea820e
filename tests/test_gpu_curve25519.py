"""Curve25519_RO / Curve25519_NU on the GPU (DR_CURVE_CURVE25519_RO = 13, DR_CURVE_CURVE25519_NU = 14; kernels_curve25519.hip.h): the map,
scalar-multiplication, grouped-MSM and decoder kernels and the Tiny / Thin / Pedersen suites, bit-exact against the big-integer
restatement (curve25519_ref.py) — the exceptional points of the birational map (the identity, (0, 0)) and small-order points included."""
import ctypes
import json
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import curve25519_ref as c  # noqa: E402
import secp256k1_ref as k1  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ("curve25519_ro", "curve25519_nu")
SCALARS = [0, 1, 2, 8, c.N - 1, c.N, c.N + 1, 2**252, 2**256 - 1]


def _h2c(name):
    return json.load(open(os.path.join(GOLDEN, "h2c", f"{name}.json")))["vectors"]


def _base():
    return json.load(open(os.path.join(GOLDEN, "base", "curve25516_base_vectors.json")))


def _xy(v):
    return int(v["x"], 16), int(v["y"], 16)


def _us(us):
    return b"".join(u.to_bytes(32, "little") for u in us)


def _suite(name):
    """(curve variant, restatement suite, DST, elements per message)"""
    import dot_ring_amd as d

    return {"curve25519_ro": (d.Curve25519_RO, c.RO, c.DST_RO, 2), "curve25519_nu": (d.Curve25519_NU, c.NU, c.DST_NU, 1)}[name]


def _pack(pts):
    """(u || v bytes, flag bytes) of restatement points (None: the identity)"""
    return b"".join(bytes(64) if p is None else c.raw(p) for p in pts), bytes(1 if p is None else 0 for p in pts)


def _unpack(raw, flags):
    out = []
    for i, f in enumerate(flags):
        if f:
            assert raw[64 * i : 64 * i + 64] == bytes(64)
            out.append(None)
        else:
            out.append((int.from_bytes(raw[64 * i : 64 * i + 32], "little"), int.from_bytes(raw[64 * i + 32 : 64 * i + 64], "little")))
    return out


@pytest.fixture(scope="module")
def points():
    """restatement points shared by the tests: the generator, mapped points (cofactor not cleared), subgroup points, torsion"""
    rng = random.Random(77)
    tors = c.torsion_points()
    order4 = next(t for t in tors if t is not None and t != c.TWO_TORSION and c.mul(4, t) is None)
    order8 = next(t for t in tors if t is not None and c.mul(4, t) is not None)
    mapped = [c.map_to_curve(rng.randrange(c.P)) for _ in range(6)]
    sub = [c.mul(rng.randrange(1, c.N), c.G) for _ in range(6)]
    return {"tors": tors, "order4": order4, "order8": order8, "mapped": mapped, "sub": sub}


# ---------------------------------------------------------------- hash to field, the map
@pytest.mark.parametrize("name", NAMES)
def test_h2c_vectors(ctx, name):
    cv, ref, dst, per = _suite(name)
    vs = _h2c(name)
    msgs = [v["msg"].encode() for v in vs]
    us = cv.point_type.hash_to_field_pairs(msgs)
    assert us == b"".join(_us([int(u, 16) for u in v["u"]]) for v in vs)
    raw, flags = ctx.curve25519_map_to_curve(us, per)
    assert _unpack(raw, flags) == [_xy(v["P"]) for v in vs]
    # Q: one element at a time with the cofactor not cleared (the file's one off-curve record is held to the restatement: test_curve25519_cpu)
    singles = [int(u, 16) for v in vs for u in v["u"]]
    raw, flags = ctx.curve25519_map_to_curve(_us(singles), 1, clear_cofactor=False)
    assert _unpack(raw, flags) == [c.map_to_curve(u) for u in singles]
    on_file = [_xy(v[k]) for v in vs for k in (("Q",) if per == 1 else ("Q0", "Q1"))]
    assert sum(1 for got, want in zip(_unpack(raw, flags), on_file) if got == want) == len(singles) - (per - 1)
    pts = cv.point_type.encode_to_curve_batch(msgs)
    assert [(p.x, p.y) for p in pts] == [_xy(v["P"]) for v in vs]
    assert cv.point_type.encode_to_curve(msgs[1]) == pts[1]


def test_map_edges_and_random(ctx):
    import dot_ring_amd as d

    rng = random.Random(9380)
    p = c.P
    # 0 is the one input whose Edwards intermediate is undefined (its image is (0, 0)); sqrt(-1/2) does not exist (tv1 = -1 unreachable)
    edge = [0, 1, p - 1, 2, (p - 1) // 2]
    singles = edge + [rng.randrange(p) for _ in range(300)]
    raw, flags = ctx.curve25519_map_to_curve(_us(singles), 1, clear_cofactor=False)
    assert _unpack(raw, flags) == [c.map_to_curve(u) for u in singles]
    assert _unpack(raw, flags)[0] == c.TWO_TORSION
    raw, flags = ctx.curve25519_map_to_curve(_us(singles), 1)                                  # NU: 8 Q; 8 (0, 0) is the identity
    got = _unpack(raw, flags)
    assert got == [c.mul(8, c.map_to_curve(u)) for u in singles] and got[0] is None and flags[0] == 1
    pairs = [(a, b) for a in edge for b in edge] + [(rng.randrange(p), rng.randrange(p)) for _ in range(300)]
    raw, flags = ctx.curve25519_map_to_curve(_us([u for pr in pairs for u in pr]), 2)          # RO
    want = [c.mul(8, c.add(c.map_to_curve(a), c.map_to_curve(b))) for a, b in pairs]
    assert _unpack(raw, flags) == want and None in want
    raw, flags = ctx.curve25519_map_to_curve(_us([u for pr in pairs[:40] for u in pr]), 2, clear_cofactor=False)
    assert _unpack(raw, flags) == [c.add(c.map_to_curve(a), c.map_to_curve(b)) for a, b in pairs[:40]]
    # the point types: the identity comes back as the identity, never as an error
    assert d.Curve25519_NU.point_type.encode_to_curve_from_field(bytes(32))[0].is_identity()
    for bad in (p, p + 1, 2**256 - 1):                                                         # non-canonical input is refused by the host
        with pytest.raises(ValueError):
            ctx.curve25519_map_to_curve(_us([5, bad]), 1)
        with pytest.raises(ValueError):
            ctx.curve25519_map_to_curve(_us([bad, 5]), 2)
    with pytest.raises(ValueError):
        ctx.curve25519_map_to_curve(bytes(33), 1)


@pytest.mark.parametrize("name", NAMES)
def test_encode_to_curve_batch(ctx, name):
    cv, ref, _, _ = _suite(name)
    rng = random.Random(300)
    msgs = [rng.randbytes(n) for n in range(0, 300, 7)]
    got = ctx.encode_to_curve_batch(cv.point_type._suite_struct(), msgs, None)
    assert got == b"".join(c.raw(ref.e2c(m)) for m in msgs)
    salted = ctx.encode_to_curve_batch(cv.point_type._suite_struct(), [b"", b"abc"], [b"salt", b"s" * 40])
    assert salted == c.raw(ref.e2c(b"salt")) + c.raw(ref.e2c(b"s" * 40 + b"abc"))
    pt = cv.point_type.encode_to_curve(b"abc", b"salt")
    assert (pt.x, pt.y) == ref.e2c(b"saltabc")


# ---------------------------------------------------------------- scalar multiplication, grouped MSM
@pytest.mark.parametrize("n", [1, 63, 64, 65, 300])
def test_scalar_mul(ctx, points, n):
    rng = random.Random(n)
    pool = [c.G, c.TWO_TORSION, points["order4"], points["order8"], None] + points["mapped"] + points["sub"]
    pts = [pool[i % len(pool)] for i in range(n)]
    # 17 points and 9 scalars, coprime: the first 153 items (n = 300 alone has them all) meet every (point, scalar) pair once, the rest are random
    assert len(pool) == 17 and len(SCALARS) == 9
    ks = [SCALARS[i % 9] if i < 153 else rng.randrange(2**256) for i in range(n)]
    if n == 1:
        pts, ks = [c.G], [c.N - 1]
    blob, flags = _pack(pts)
    raw, out_flags = ctx.curve25519_scalar_mul_batch(blob, flags, k1_sc(ks))
    # the packer reduces mod l, as for the other suites: small-order components see k mod l
    assert _unpack(raw, out_flags) == [c.mul(k % c.N, p) for k, p in zip(ks, pts)]
    if n == 300:
        # (0, 0): odd k gives (0, 0), even k the identity flag; the identity in gives the identity out
        two = [(k, c.TWO_TORSION) for k in (1, 3, c.N, 2, 8, 0)]
        raw, fl = ctx.curve25519_scalar_mul_batch(*_pack([p for _, p in two]), k1_sc([k for k, _ in two]))
        assert _unpack(raw, fl) == [c.TWO_TORSION, c.TWO_TORSION, None, None, None, None]      # (l mod l = 0)
        raw, fl = ctx.curve25519_scalar_mul_batch(*_pack([None, None]), k1_sc([5, 0]))
        assert bytes(fl) == b"\x01\x01" and raw == bytes(128)
        # the flag is the only form of the identity here: 64 bytes of 0xff with flag 0 are a non-canonical point, with flag 1 they are ignored
        with pytest.raises(ValueError):
            ctx.curve25519_scalar_mul_batch(c.raw(c.G) + b"\xff" * 64, b"\x00\x00", k1_sc([1, 1]))
        with pytest.raises(ValueError):
            ctx.curve25519_msm_groups(c.raw(c.G) + b"\xff" * 64, b"\x00\x00", k1_sc([1, 1]), 2)
        raw, fl = ctx.curve25519_scalar_mul_batch(c.raw(c.G) + b"\xff" * 64, b"\x00\x01", k1_sc([1, 1]))
        assert (raw, bytes(fl)) == (c.raw(c.G) + bytes(64), b"\x00\x01")
        raw, fl = ctx.curve25519_scalar_mul_batch(*_pack([points["order4"]] * 4), k1_sc([1, 2, 3, 4]))
        assert _unpack(raw, fl) == [c.mul(k, points["order4"]) for k in (1, 2, 3, 4)] and fl[3] == 1 and _unpack(raw, fl)[1] == c.TWO_TORSION


def k1_sc(ks):
    return b"".join((k % c.N).to_bytes(32, "little") for k in ks)


@pytest.mark.parametrize("m", [1, 2, 63, 64, 65])
def test_msm_groups(ctx, points, m):
    import dot_ring_amd as d
    from dot_ring_amd.curve import msm_groups

    rng = random.Random(m)
    pool = [c.G, c.TWO_TORSION, points["order4"], None] + points["mapped"][:3] + points["sub"][:3]
    if m == 65:                     # beyond one group: the MSM entry point (groups of 64, then the partial sums)
        pts = [pool[i % len(pool)] for i in range(65)]
        ks = [rng.randrange(c.N) for _ in range(65)]
        cls = d.Curve25519.point_type
        objs = [cls.identity() if p is None else cls(*p) for p in pts]
        got = cls.msm(objs, ks)
        assert ((got.x, got.y) if not got.is_identity() else None) == c.msm(pts, ks)
        assert cls.msm(objs + [-o for o in objs], ks + ks).is_identity()
        with pytest.raises(ValueError):
            ctx.curve25519_msm_groups(*_pack(pts), k1_sc(ks), 65)
        return
    groups = 5 if m < 63 else 3
    pts, ks = [], []
    for g in range(groups):
        gp = [pool[(g + j) % len(pool)] for j in range(m)]
        gk = [rng.randrange(c.N) for _ in range(m)]
        if g == 1 and m >= 2:       # a cancelling pair and a repeated point
            gp[0], gp[1], gk[1] = points["sub"][0], c.neg(points["sub"][0]), gk[0]
            if m > 3:
                gp[2], gp[3] = points["mapped"][0], points["mapped"][0]
        if g == 2:                  # this group sums to the identity
            if m == 1:
                gp, gk = [points["sub"][1]], [0]
            else:
                gp = [points["sub"][j % 6] for j in range(m - 1)]
                gk = gk[: m - 1]
                total = c.msm(gp, gk)
                gp, gk = gp + [c.neg(total) if total else None], gk + [1]
        pts += gp
        ks += gk
    raw, fl = ctx.curve25519_msm_groups(*_pack(pts), k1_sc(ks), m)
    want = [c.msm(pts[g * m : g * m + m], ks[g * m : g * m + m]) for g in range(groups)]
    assert _unpack(raw, fl) == want and want[2] is None
    # the generic entry point carries the identity as 64 bytes of 0xff
    cls = d.Curve25519.point_type
    got = msm_groups([cls.identity() if p is None else cls(*p) for p in pts], ks, m)
    assert [None if g.is_identity() else (g.x, g.y) for g in got] == want


# ---------------------------------------------------------------- the decoder
def test_decoder(ctx, points):
    import dot_ring_amd as d
    from dot_ring_amd.vrf.codec import dec_point, dec_points, enc_point

    rng = random.Random(64)
    valid = points["sub"] + [c.mul(rng.randrange(1, c.N), c.G) for _ in range(60)] + [c.G]
    small = [t for t in points["tors"] if t is not None]
    mixed = [c.add(points["sub"][0], t) for t in small] + points["mapped"]
    g = c.G
    bad = [(g[0] + c.P).to_bytes(32, "little") + g[1].to_bytes(32, "little"), g[0].to_bytes(32, "little") + (g[1] + c.P).to_bytes(32, "little"),
           c.raw((g[0], (g[1] + 1) % c.P)), c.raw((9, 1)), b"\xff" * 64, (2**255 - 1).to_bytes(32, "little") * 2]
    encs = [c.raw(p) for p in valid + small + mixed] + bad
    assert c.raw(c.TWO_TORSION) in encs
    blob = b"".join(encs)
    for check in (False, True):
        out, ok = ctx.curve25519_decode_points(blob, check=check)
        for i, e in enumerate(encs):
            want = c.decode(e, check=check)
            assert ok[i] == (0 if want == "bad" else 1), (i, check)
            assert out[64 * i : 64 * i + 64] == (bytes(64) if want == "bad" else e), (i, check)
    codec_ok = ctx.curve25519_decode_points(blob, check=False)[1]
    check_ok = ctx.curve25519_decode_points(blob, check=True)[1]
    nv, ns = len(valid), len(small)
    assert bytes(codec_ok[: nv + ns]) == b"\x01" * (nv + ns) and bytes(check_ok[nv : nv + ns + 7]) == bytes(ns + 7)   # small order and mixed refused
    assert bytes(check_ok[:nv]) == b"\x01" * nv and bytes(codec_ok[-len(bad) :]) == bytes(len(bad))
    for cid in (13, 14):                       # the generic entry point is the checking decoder
        assert ctx.bsn_decode_points(blob, cid) == ctx.curve25519_decode_points(blob, check=True)
    got = dec_points(d.Curve25519, encs[:nv])
    assert [(q.x, q.y) for q in got] == valid and [enc_point(q) for q in got] == encs[:nv]
    for e in [encs[nv], encs[nv + 3], bad[0], bad[2], encs[0][:63], encs[0] + b"\x00"]:
        with pytest.raises(ValueError):
            dec_point(d.Curve25519, e)
    assert d.Curve25519.point_type.string_to_point(bytes(64)) == d.Curve25519.point_type(0, 0)      # the codec alone accepts (0, 0)
    assert not d.Curve25519.curve.valid_point(d.Curve25519.point_type(0, 0))


# ---------------------------------------------------------------- the VRFs
def _flip(blob, pos):
    return blob[:pos] + bytes([blob[pos] ^ 1]) + blob[pos + 1 :]


def _verifies(fn):
    try:
        return bool(fn())
    except ValueError:
        return False


@pytest.mark.parametrize("name", NAMES)
def test_base_records(ctx, name):
    import dot_ring_amd as d
    from dot_ring_amd.vrf.codec import point_len, scalar_len

    cv, ref, _, _ = _suite(name)
    # vrf/codec.py of the reference: point_len = 32 x 2 (uncompressed), challenge 16, scalar 32 -> 64 + 16 + 32, 2 x 64 + 32, 4 x 64 + 2 x 32
    assert (point_len(cv), scalar_len(cv)) == (64, 32)
    recs = _base()
    assert len(recs) == 5
    other_pk = cv.public_key_from_secret((99).to_bytes(32, "little"))
    for v in recs:
        sk, al, ad = (bytes.fromhex(v[k]) for k in ("sk", "alpha", "ad"))
        pk = cv.public_key_from_secret(sk)
        assert pk == ref.enc(ref.mul(k1.le(sk), ref.g)) and not v["pk"]             # (the file leaves pk empty)
        for salt in (b"", b"salt"):
            tiny = d.TinyVRF[cv].prove(al, sk, ad, salt)
            thin = d.ThinVRF[cv].prove(al, sk, ad, salt)
            ped = d.PedersenVRF[cv].prove(al, sk, ad, salt)
            want_ped, blinding = ref.pedersen_prove(sk, al, ad, salt=salt)
            assert (len(tiny.encode()), len(thin.encode()), len(ped.encode())) == (112, 160, 320)
            assert tiny.encode() == ref.ietf_prove(sk, al, ad, salt=salt)
            assert thin.encode() == ref.ietf_prove(sk, al, ad, thin=True, salt=salt)
            assert ped.encode() == want_ped
            beta = ref.point_to_hash(ref.mul(k1.le(sk), ref.e2c(salt + al)))
            assert d.TinyVRF[cv].proof_to_hash(tiny.output_point) == beta == d.PedersenVRF[cv].proof_to_hash(ped.output_point)
            for vrf, proof, widths in ((d.TinyVRF[cv], tiny, (64, 16, 32)), (d.ThinVRF[cv], thin, (64, 64, 32))):
                blob = proof.encode()
                rt = vrf.decode(blob)
                assert rt.encode() == blob and rt.verify(pk, al, ad, salt)
                assert not rt.verify(pk, al + b"\x01", ad, salt) and not rt.verify(pk, al, ad + b"\x01", salt)
                assert not rt.verify(pk, al, ad, salt + b"x") and not rt.verify(other_pk, al, ad, salt)
                pos = 0
                for w in widths:                                   # one byte of each field
                    assert not _verifies(lambda: vrf.decode(_flip(blob, pos + w - 1)).verify(pk, al, ad, salt))
                    pos += w
            blob = ped.encode()
            rt = d.PedersenVRF[cv].decode(blob)
            assert rt.encode() == blob and rt.verify(al, ad, salt) and rt.verify_unblinding(pk, blinding)
            assert not rt.verify(al + b"\x01", ad, salt) and not rt.verify(al, ad + b"\x01", salt) and not rt.verify(al, ad, salt + b"x")
            assert not rt.verify_unblinding(other_pk, blinding)
            pos = 0
            for w in (64, 64, 64, 64, 32, 32):
                assert not _verifies(lambda: d.PedersenVRF[cv].decode(_flip(blob, pos + w - 1)).verify(al, ad, salt))
                pos += w


@pytest.mark.parametrize("scheme", ["tiny", "thin", "pedersen"])
@pytest.mark.parametrize("name", NAMES)
def test_prove_batch_300(ctx, name, scheme):
    import dot_ring_amd as d
    from dot_ring_amd.curve import scalar_mul_batch

    cv, ref, _, _ = _suite(name)
    vrf = {"tiny": d.TinyVRF, "thin": d.ThinVRF, "pedersen": d.PedersenVRF}[scheme][cv]
    rng = random.Random(13)
    B = 300
    sks = [rng.randrange(1, ref.n).to_bytes(32, "little") for _ in range(B)]
    als = [b"alpha-%d" % i for i in range(B)]
    ads = [b"ad-%d" % (i % 5) for i in range(B)]
    salts = [b"s%d" % i if i % 2 else b"" for i in range(B)]
    proofs = vrf.prove_batch(als, sks, ads, salts)
    for i in range(0, B, 30):                                      # the single calls and the restatement
        assert vrf.prove(als[i], sks[i], ads[i], salts[i]).encode() == proofs[i].encode(), i
        if scheme == "pedersen":
            want, _ = ref.pedersen_prove(sks[i], als[i], ads[i], salt=salts[i])
        else:
            want = ref.ietf_prove(sks[i], als[i], ads[i], thin=scheme == "thin", salt=salts[i])
        assert proofs[i].encode() == want, i
    gen = cv.point_type.generator_point()
    pks = [pk.point_to_string() for pk in scalar_mul_batch([gen] * B, [k1.le(sk) for sk in sks])]       # all 300 in one launch
    assert pks[3] == cv.public_key_from_secret(sks[3])
    other = cv.point_type.encode_to_curve(b"another point")
    if scheme == "tiny":                                           # Tiny proofs carry no R: they verify one by one
        assert all(proofs[i].verify(pks[i], als[i], ads[i], salts[i]) for i in range(0, 40, 5))
        p = proofs[7]
        for bad in (type(p)(other, p.c, p.s), type(p)(p.output_point, p.c ^ 1, p.s), type(p)(p.output_point, p.c, (p.s + 1) % ref.n)):
            assert not bad.verify(pks[7], als[7], ads[7], salts[7])
    if scheme == "thin":
        assert vrf.batch_verify(proofs, pks, als, ads, salts)                   # all 300
        p = proofs[7]
        for bad in (type(p)(other, p.r, p.s), type(p)(p.output_point, other, p.s), type(p)(p.output_point, p.r, (p.s + 1) % ref.n)):
            assert not vrf.batch_verify(proofs[:7] + [bad] + proofs[8:], pks, als, ads, salts)
    if scheme == "pedersen":
        assert vrf.batch_verify(proofs, als, ads, salts)
        p = proofs[5]
        for bad in (type(p)(other, p.blinded_pk, p.result_point, p.ok, p.s, p.sb), type(p)(p.output_point, p.blinded_pk, other, p.ok, p.s, p.sb),
                    type(p)(p.output_point, p.blinded_pk, p.result_point, p.ok, (p.s + 1) % ref.n, p.sb),
                    type(p)(p.output_point, p.blinded_pk, p.result_point, p.ok, p.s, (p.sb + 1) % ref.n)):
            assert not vrf.batch_verify(proofs[:5] + [bad] + proofs[6:], als, ads, salts)


# ---------------------------------------------------------------- refusals, residue, the other suites
def test_refusals(ctx):
    import dot_ring_amd as d
    from dot_ring_amd import _native

    lib = _native.lib()
    off = (ctypes.c_uint64 * 2)(0, 0)
    for cv, cid in ((d.Curve25519_RO, 13), (d.Curve25519_NU, 14)):
        suite = cv.point_type._suite_struct()
        assert suite.xof == 0 and suite.curve == cid
        verdict = ctypes.create_string_buffer(1)
        rc = lib.dr_ietf_verify_batch(ctx.handle, ctypes.byref(suite), 0, 1, bytes(112), bytes(64), b"", off, b"", off, None, None, verdict)
        assert rc == _native.DR_ERR_INVALID
        bad = _native.vrf_suite(suite._keep, 2, bytes(suite.generator_xy), bytes(suite.blinding_base_xy), cid)     # SHA-256: not this suite's hash
        out_xy = ctypes.create_string_buffer(64)
        rc = lib.dr_encode_to_curve_batch(ctx.handle, ctypes.byref(bad), b"a", (ctypes.c_uint64 * 2)(0, 1), None, None, 1, out_xy)
        assert rc == _native.DR_ERR_INVALID
        with pytest.raises(ValueError):
            d.RingProofParams(cv=cv)
        good = d.TinyVRF[cv].prove(b"a", (5).to_bytes(32, "little"), b"").encode()
        for vrf, n in ((d.TinyVRF[cv], 112), (d.ThinVRF[cv], 160), (d.PedersenVRF[cv], 320)):
            for blob in (bytes(n - 1), bytes(n + 1), good[:80]):                                   # wrong lengths (80: an Ed25519 Tiny proof's)
                with pytest.raises(ValueError):
                    vrf.decode(blob)
        g = c.G
        off_curve = c.raw((g[0], (g[1] + 1) % c.P))
        with pytest.raises(ValueError):
            d.TinyVRF[cv].decode(off_curve + good[64:])                                            # gamma off the curve
        with pytest.raises(ValueError):
            d.TinyVRF[cv].decode(bytes(64) + good[64:])                                            # gamma = (0, 0): on the curve, not in the subgroup
        # a proof point that is the identity has no encoding: the secret key 0 makes every point of a Tiny proof the identity
        with pytest.raises(ValueError):
            d.TinyVRF[cv].prove(b"a", bytes(32), b"")
        with pytest.raises(ValueError):
            d.PedersenVRF[cv].prove_batch([b"a"] * 3, [(5).to_bytes(32, "little"), bytes(32), (6).to_bytes(32, "little")], [b""] * 3)
        with pytest.raises(ValueError):
            cv.public_key_from_secret(bytes(32))
    # coordinates at or above p are refused; id 12 is no curve
    n1 = ctypes.create_string_buffer(64)
    assert lib.dr_te_scalar_mul_batch(ctx.handle, 13, (c.P).to_bytes(32, "little") + bytes(32), bytes(32), 1, n1) == _native.DR_ERR_INVALID
    assert lib.dr_te_scalar_mul_batch(ctx.handle, 12, bytes(64), bytes(32), 1, n1) == _native.DR_ERR_INVALID
    assert lib.dr_te_scalar_mul_batch(ctx.handle, 15, bytes(64), bytes(32), 1, n1) == _native.DR_ERR_INVALID


def test_no_secret_residue_after_prove(ctx):
    import dot_ring_amd as d
    from dot_ring_amd import runtime

    rt = runtime.context()
    for cv in (d.Curve25519_RO, d.Curve25519_NU):
        for vrf in (d.TinyVRF[cv], d.ThinVRF[cv], d.PedersenVRF[cv]):
            vrf.prove_batch([b"r%d" % i for i in range(70)], [(1000 + i).to_bytes(32, "little") for i in range(70)], [b""] * 70)
            assert rt.scratch_residue() == 0


def test_other_suites_after_curve25519_calls(ctx, golden_dir):
    import dot_ring_amd as d

    for cv in (d.Curve25519_RO, d.Curve25519_NU):
        d.PedersenVRF[cv].prove_batch([b"a"] * 80, [(7).to_bytes(32, "little")] * 80, [b""] * 80)
    fields = ("gamma", "proof_pk_com", "proof_r", "proof_ok", "proof_s", "proof_sb")
    hx = lambda v, k: bytes.fromhex(v[k])  # noqa: E731
    for rel, cv in (("ark-vrf/ed25519_sha-512_tai_pedersen.json", d.Ed25519), ("ark-vrf/bandersnatch_sha-512_ell2_pedersen.json", d.Bandersnatch)):
        for v in json.load(open(os.path.join(golden_dir, rel))):
            proof = d.PedersenVRF[cv].prove(hx(v, "alpha"), hx(v, "sk"), hx(v, "ad"))
            assert proof.encode() == b"".join(hx(v, f) for f in fields)
    vs = json.load(open(os.path.join(GOLDEN, "h2c", "ed25519_ro.json")))["vectors"]
    got = d.Ed25519_RO.point_type.encode_to_curve_batch([v["msg"].encode() for v in vs])
    assert [(p.x, p.y) for p in got] == [_xy(v["P"]) for v in vs]
