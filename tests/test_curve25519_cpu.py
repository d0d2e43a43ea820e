"""Curve25519_RO / Curve25519_NU without a GPU: the big-integer restatement (curve25519_ref.py) against the reference's hash-to-curve
vectors, its Montgomery law against the Ed25519 law through the birational map the kernels compute through (the exceptional points
included), the fact the kernels' argument rests on (486660 is not a square), the suite layer's round trips, and the package's host
side (names, ids, codec, single additions, map_to_curve)."""
import json
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import curve25519_ref as c  # noqa: E402
import ed25519_ref as ed  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VARIANTS = {"curve25519_ro": (c.DST_RO, c.encode_to_curve_ro, 2, c.RO), "curve25519_nu": (c.DST_NU, c.encode_to_curve_nu, 1, c.NU)}


def _h2c(name):
    return json.load(open(os.path.join(GOLDEN, "h2c", f"{name}.json")))


def _base():
    return json.load(open(os.path.join(GOLDEN, "base", "curve25516_base_vectors.json")))


def _xy(v):
    return int(v["x"], 16), int(v["y"], 16)


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_restatement_reproduces_h2c_vectors(name):
    dst, e2c, per, _ = VARIANTS[name]
    doc = _h2c(name)
    assert doc["dst"].encode() == dst and len(doc["vectors"]) >= 5
    off_curve = []
    for v in doc["vectors"]:
        msg = v["msg"].encode()
        us = c.hash_to_field(msg, per, dst)
        assert us == [int(u, 16) for u in v["u"]]
        qs = [c.map_to_curve(u) for u in us]
        for q, want in zip(qs, [_xy(v["Q"])] if per == 1 else [_xy(v["Q0"]), _xy(v["Q1"])]):
            if c.on_curve(want):
                assert q == want
            else:               # the reference's file holds ONE record that is no point of the curve (its tests read P only): u still agrees
                off_curve.append((v["msg"], want))
                assert q[0] == want[0]
        assert e2c(msg) == _xy(v["P"])
        assert c.mul(c.N, _xy(v["P"])) is None                       # the cofactor is cleared
        assert c.mul(8 * c.N, qs[0]) is None
    # every u, Q and P of both files, but for Q0 of the RO file's last vector, whose v is not a root of the curve equation at its u
    assert [m for m, _ in off_curve] == ([doc["vectors"][-1]["msg"]] if per == 2 else [])


def test_486660_is_not_a_square():
    """no rational point has u = -1: there v^2 = -1 + 486662 - 1 = 486660 (the kernels' load form divides by u + 1)"""
    assert pow(486660, (c.P - 1) // 2, c.P) == c.P - 1
    # and the other facts kernels_curve25519.hip.h states: (0, 0) is the only point with v = 0, the element 0 alone maps to it
    assert pow((c.A * c.A - 4) % c.P, (c.P - 1) // 2, c.P) == c.P - 1
    assert pow(-c.A % c.P, (c.P - 1) // 2, c.P) == c.P - 1
    assert c.map_to_curve(0) == c.TWO_TORSION and c.on_curve(c.TWO_TORSION)
    assert (c.C * c.C + 486664) % c.P == 0


def test_law_agrees_with_ed25519_through_the_map():
    rng = random.Random(25519)
    assert c.to_edwards(c.G) == ed.G or c.to_edwards(c.G) == ed.neg(ed.G)         # (which one depends on the root c)
    pts = [c.mul(rng.randrange(1, c.N), c.G) for _ in range(6)] + [c.map_to_curve(rng.randrange(c.P)) for _ in range(6)]
    tors = c.torsion_points()
    assert None in tors and c.TWO_TORSION in tors and len(set(tors)) == 8
    orders = {t: next(k for k in (1, 2, 4, 8) if c.mul(k, t) is None) for t in tors}
    assert sorted(orders.values()) == [1, 2, 4, 4, 8, 8, 8, 8]
    pts += tors + [c.add(pts[0], tors[1]), c.add(pts[7], tors[3])]
    for pt in pts:
        assert c.on_curve(pt) and ed.on_curve(c.to_edwards(pt)) and c.from_edwards(c.to_edwards(pt)) == pt
    for p1 in pts:
        for p2 in pts + [p1, c.neg(p1), c.TWO_TORSION]:
            assert c.to_edwards(c.add(p1, p2)) == ed.add(c.to_edwards(p1), c.to_edwards(p2)), (p1, p2)
    for pt in pts:
        assert c.add(pt, c.neg(pt)) is None and c.add(pt, None) == pt and c.add(None, pt) == pt
        k = rng.randrange(c.N)
        assert c.to_edwards(c.mul(k, pt)) == ed.mul(k, c.to_edwards(pt))
    assert c.add(c.TWO_TORSION, c.TWO_TORSION) is None
    for _ in range(4):                                                        # 8 l P = O for mapped points
        assert c.mul(8 * c.N, c.map_to_curve(rng.randrange(c.P))) is None


def test_codec():
    rng = random.Random(3)
    pt = c.mul(rng.randrange(1, c.N), c.G)
    assert c.decode(c.encode(pt)) == pt and c.decode(c.encode(pt), check=True) == pt and len(c.encode(pt)) == 64
    assert c.decode(c.raw(c.TWO_TORSION)) == c.TWO_TORSION and c.decode(c.raw(c.TWO_TORSION), check=True) == "bad"
    for t in c.torsion_points()[1:]:
        assert c.decode(c.raw(t)) == t and c.decode(c.raw(t), check=True) == "bad"
        mixed = c.add(pt, t)
        assert c.decode(c.raw(mixed)) == mixed and c.decode(c.raw(mixed), check=True) == "bad"
    assert c.decode(c.raw((pt[0], (pt[1] + 1) % c.P))) == "bad"
    assert c.decode((pt[0] + c.P).to_bytes(32, "little") + pt[1].to_bytes(32, "little")) == "bad"
    assert c.decode(c.raw(pt)[:63]) == "bad"
    with pytest.raises(ValueError):
        c.encode(None)


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_suite_round_trips(name):
    suite = VARIANTS[name][3]
    recs = _base()
    assert len(recs) == 5
    for v in recs:
        sk, al, ad = (bytes.fromhex(v[k]) for k in ("sk", "alpha", "ad"))
        pk = suite.enc(suite.mul(int.from_bytes(sk, "little"), suite.g))
        tiny, thin = suite.ietf_prove(sk, al, ad), suite.ietf_prove(sk, al, ad, thin=True)
        ped, _ = suite.pedersen_prove(sk, al, ad)
        assert (len(pk), len(tiny), len(thin), len(ped)) == (64, 112, 160, 320)
        assert c.ietf_verify(suite, pk, tiny, al, ad) and c.ietf_verify(suite, pk, thin, al, ad, thin=True)
        assert c.pedersen_verify(suite, ped, al, ad)
        assert not c.ietf_verify(suite, pk, tiny, al + b"x", ad) and not c.ietf_verify(suite, pk, thin, al, ad + b"x", thin=True)
        assert not c.pedersen_verify(suite, ped, al + b"x", ad)
        assert c.decode(tiny[:64], check=True) == suite.mul(int.from_bytes(sk, "little"), suite.e2c(al))
    assert suite.enc(suite.mul(1, suite.g)) == c.raw(c.G)                # sk = 1: the generator is the public key


# ---------------------------------------------------------------- the package's host side
def test_names_ids_and_params():
    import dot_ring_amd as d
    from dot_ring_amd import _native
    from dot_ring_amd.vrf.codec import point_len

    assert {"Curve25519", "Curve25519_RO", "Curve25519_NU"} <= set(d.__all__)
    assert d.Curve25519 is d.Curve25519_RO and d.Curve25519_NU is not d.Curve25519_RO
    assert (_native.CURVE_CURVE25519_RO, _native.CURVE_CURVE25519_NU) == (13, 14)
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "dotring_hip.h")).read()
    assert "DR_CURVE_CURVE25519_RO = 13, DR_CURVE_CURVE25519_NU = 14" in header
    for call in ("dr_curve25519_scalar_mul_batch", "dr_curve25519_msm_groups", "dr_curve25519_decode_points", "dr_curve25519_map_to_curve"):
        assert call in header and call in _native.EXPORTED_SYMBOLS
    for cv, cid, e2c in ((d.Curve25519_RO, 13, "ell2"), (d.Curve25519_NU, 14, "ell2_nu")):
        sp = cv.curve.params
        assert (sp.curve_id, sp.e2c, sp.suite_id, sp.cofactor) == (cid, e2c, c.SUITE_ID, 8)
        assert (sp.field_modulus, sp.subgroup_order, sp.generator, sp.auxiliary_points.blinding_base) == (c.P, c.N, c.G, c.G)
        assert sp.encoding.uncompressed and sp.encoding.challenge_len == 16 and point_len(cv) == 64 and _native.curve_point_len(cid) == 64
        assert d.TinyVRF[cv].cv is cv
        assert d.PedersenVRF[cv].proof_len() == 320
        with pytest.raises(ValueError):
            d.RingProofParams(cv=cv)
    assert point_len(d.Ed25519) == 32 and point_len(d.P256) == 33 and point_len(d.Bandersnatch) == 32


def test_point_class_host_operations():
    import dot_ring_amd as d
    from dot_ring_amd.curve import pack_points, pack_points_flagged, unpack_points, unpack_points_flagged

    pt = d.Curve25519.point_type
    rng = random.Random(8)
    g = pt.generator_point()
    assert (g.x, g.y) == c.G and g.is_on_curve() and pt.identity().is_identity() and pt.identity().is_on_curve()
    tors = [pt(*t) if t else pt.identity() for t in c.torsion_points()]
    raw_pts = [c.mul(rng.randrange(1, c.N), c.G) for _ in range(4)] + c.torsion_points()
    objs = [pt(*t) if t else pt.identity() for t in raw_pts]
    for a, ra in zip(objs, raw_pts):
        for b, rb in zip(objs + [a], raw_pts + [ra]):
            s = a + b
            assert ((s.x, s.y) if not s.is_identity() else None) == c.add(ra, rb)
        assert (a - a).is_identity() and (-a + a).is_identity() and a.double() == a + a
    zero = pt(0, 0)
    assert zero.double().is_identity() and zero in tors
    with pytest.raises(ValueError):
        pt(9, 1)
    with pytest.raises(ValueError):
        pt(c.P + 9, c.G[1])
    # codec
    assert g.point_to_string() == c.raw(c.G) and pt.string_to_point(c.raw(c.G)) == g and pt.string_to_point(bytes(64)) == zero
    with pytest.raises(ValueError):
        pt.identity().point_to_string()
    for bad in (c.raw((9, 1)), c.raw(c.G)[:63], (c.P + 9).to_bytes(32, "little") + c.G[1].to_bytes(32, "little")):
        with pytest.raises(ValueError):
            pt.string_to_point(bad)
    # map_to_curve on the host: one image, the cofactor not cleared
    for name in sorted(VARIANTS):
        for v in _h2c(name)["vectors"]:
            got = [pt.map_to_curve(int(u, 16)) for u in v["u"]]
            assert [(q.x, q.y) for q in got] == [c.map_to_curve(int(u, 16)) for u in v["u"]]     # (held against the file's Q above)
    assert pt.map_to_curve(0) == zero
    # the identity's two packed forms
    assert pack_points([g, pt.identity(), zero]) == c.raw(c.G) + b"\xff" * 64 + bytes(64)
    assert unpack_points(pt, pack_points([g, pt.identity(), zero])) == [g, pt.identity(), zero]
    blob, flags = pack_points_flagged([g, pt.identity(), zero])
    assert (blob, flags) == (c.raw(c.G) + bytes(128), b"\x00\x01\x00")
    assert unpack_points_flagged(pt, blob, flags) == [g, pt.identity(), zero]
