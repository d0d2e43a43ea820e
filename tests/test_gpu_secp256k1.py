"""secp256k1 on the GPU (DR_CURVE_SECP256K1 = 6, DR_CURVE_SECP256K1_NU = 7): the device field at the bounds of its contract, the map of
RFC 9380 against the hash-to-curve vectors the reference holds and against the big-integer restatement (secp256k1_ref.py), the group
calls, decoding, and the Tiny / Thin / Pedersen provers and verifiers against the restatement's bytes — the reference holds no proof
vectors for this curve; test_secp256k1_cpu.py shows the restatement's VRF layer reproducing the P-256 ones."""
import ctypes
import json
import os
import random
import struct
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import secp256k1_ref as r  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RO, NU = 6, 7
M29 = (1 << 29) - 1
MAP_SEED = 2024          # chosen with the restatement: of its 1000 field elements, each SSWU branch takes at least 400 (asserted below)


def _h2c(variant):
    return json.load(open(os.path.join(GOLDEN, "h2c", f"secp256k1_{variant}.json")))["vectors"]


def _base():
    return json.load(open(os.path.join(GOLDEN, "base", "secp256k1_base_vectors.json")))


def _xy(v):
    return int(v["x"], 16), int(v["y"], 16)


def _us(us):
    return b"".join(u.to_bytes(32, "little") for u in us)


def _sc(ks):
    return b"".join(k.to_bytes(32, "little") for k in ks)


def _points(rng, k):
    return [r.mul(rng.randrange(1, r.N), r.G) for _ in range(k)]


def _variants():
    import dot_ring_amd as d

    return ((d.Secp256k1_RO, r.RO), (d.Secp256k1_NU, r.NU))


# ---------------------------------------------------------------- field
def _val(limbs):
    return sum(v << (29 * i) for i, v in enumerate(limbs))


def _pack(rows):
    return b"".join(struct.pack("<9i", *row) for row in rows)


def test_field_ops_at_contract_bounds(ctx):
    rng = random.Random(29)
    top = [M29] * 8 + [(1 << 24) - 1]
    top[2] = (1 << 29) + (1 << 15) - 1                        # the largest normal
    low = [0] * 9
    low[2] = -(1 << 15) + 1                                   # the smallest
    rnd = lambda: [rng.randrange(1 << 29) for _ in range(8)] + [rng.randrange(1 << 24)]  # noqa: E731
    p_limbs = [(r.P >> (29 * i)) & M29 for i in range(9)]
    A = [top, low, top, low, [0] * 9, [1] + [0] * 8, p_limbs, [v - 1 if i == 0 else v for i, v in enumerate(p_limbs)]]
    B = [top, top, low, low, rnd(), rnd(), rnd(), top]
    A += [rnd() for _ in range(120)]
    B += [rnd() for _ in range(120)]
    n_normal = len(A)
    # mul's widest operands: a normal times a sum / difference of two; mul_small and carry on sums of three
    for sign in (1, -1):
        for _ in range(20):
            x, y = rnd(), rnd()
            A.append(rnd())
            B.append([a + sign * b for a, b in zip(x, y)])
        A.append(top)
        B.append([a + sign * b for a, b in zip(top, top)] if sign == 1 else [a - b for a, b in zip(low, top)])
    n_mul = len(A)
    for _ in range(20):
        x, y, z = rnd(), rnd(), rnd()
        A.append([a + b + c for a, b, c in zip(x, y, z)])
        B.append([0] * 9)
    A.append([3 * v for v in top])
    B.append([0] * 9)
    A.append([-3 * v for v in top])
    B.append([0] * 9)
    out, flags = ctx.secp256k1_field_selftest(_pack(A), _pack(B))
    P = r.P
    for i, (a, b) in enumerate(zip(A, B)):
        va, vb = _val(a), _val(b)
        rec = [int.from_bytes(out[(12 * i + k) * 32 : (12 * i + k + 1) * 32], "little") for k in range(12)]
        assert rec[2] == (va + vb) % P and rec[3] == (va - vb) % P and rec[4] == -va % P, i
        assert rec[5] == va % P and rec[9] == va % P and rec[10] == 21 * va % P and rec[11] == va * va % P, i
        assert rec[7] == (pow(va, -1, P) if va % P else 0), i
        root = r.sqrt(va)
        assert bool(flags[i] & 1) == (root is not None) and rec[8] in ((0,) if root is None else (root, P - root)), i
        assert bool(flags[i] & 2) == bool(va % P & 1), i
        if i < n_mul:
            assert rec[0] == va * vb % P, i
        if i < n_normal:
            assert rec[1] == va * va % P and rec[6] == 2 * va * vb % P, i


# ---------------------------------------------------------------- the map
def test_map_to_curve_vectors(ctx):
    ro, nu = _h2c("ro"), _h2c("nu")
    singles = [int(u, 16) for v in ro for u in v["u"]] + [int(v["u"][0], 16) for v in nu]
    want = [_xy(v[q]) for v in ro for q in ("Q0", "Q1")] + [_xy(v["Q"]) for v in nu]
    raw, ok = ctx.secp256k1_map_to_curve(_us(singles), 1)
    assert ok == b"\x01" * len(singles)
    assert [raw[64 * i : 64 * i + 64] for i in range(len(singles))] == [r.raw(q) for q in want]
    raw, ok = ctx.secp256k1_map_to_curve(_us(singles[:10]), 2)
    assert ok == b"\x01" * 5 and [raw[64 * i : 64 * i + 64] for i in range(5)] == [r.raw(_xy(v["P"])) for v in ro]
    assert [r.raw(_xy(v["P"])) for v in nu] == [r.raw(q) for q in want[10:]]


def test_map_to_curve_edges_and_random(ctx):
    import dot_ring_amd as d

    rng = random.Random(MAP_SEED)
    us = [rng.randrange(r.P) for _ in range(1000)]
    branch = [r.sswu(u)[1] for u in us]
    assert 400 <= sum(branch) <= 600                              # gx1 a square / not: at least 400 each
    us = [0, r.P - 1, 1] + us
    raw, ok = ctx.secp256k1_map_to_curve(_us(us), 1)
    assert ok == b"\x01" * len(us)
    singles = [r.map_to_curve(u) for u in us]
    for i, q in enumerate(singles):
        assert raw[64 * i : 64 * i + 64] == r.raw(q), (i, us[i])
    us2 = us[:1002] + [us[5], us[5]] + [us[6], r.P - us[6]]      # ... a pair that doubles, and one whose images cancel (u and -u)
    raw, ok = ctx.secp256k1_map_to_curve(_us(us2), 2)
    maps = {u: r.map_to_curve(u) for u in us2}
    for i in range(len(us2) // 2):
        assert raw[64 * i : 64 * i + 64] == r.raw(r.add(maps[us2[2 * i]], maps[us2[2 * i + 1]])), i
    assert raw[-64:] == bytes(64)
    pt = d.Secp256k1.point_type.map_to_curve_simple_swu(us[7])
    assert (pt.x, pt.y) == singles[7]
    with pytest.raises(ValueError):
        ctx.secp256k1_map_to_curve(_us([r.P]), 1)                 # not a canonical field element (DR_ERR_INVALID)


def test_encode_to_curve_batch(ctx):
    rng = random.Random(41)
    msgs = [rng.randbytes(rng.randrange(0, 120)) for _ in range(1000)]
    salts = [rng.randbytes(rng.randrange(0, 20)) if i % 3 else b"" for i in range(1000)]
    for cv, ref in _variants():
        got = cv.point_type.encode_to_curve_batch(msgs, salts)
        for i in range(1000):
            assert (got[i].x, got[i].y) == ref.e2c(salts[i] + msgs[i]), (cv.name, i)
        for i in (0, 1, 500, 999):
            assert cv.point_type.encode_to_curve(msgs[i], salts[i]) == got[i]
        assert cv.point_type.encode_to_curve_batch(msgs[:7]) == [cv.point_type.encode_to_curve(m) for m in msgs[:7]]
        assert cv.point_type.encode_to_curve_from_field(cv.point_type.hash_to_field_pairs(msgs[:9], salts[:9])) == got[:9]
    ro = _h2c("ro")
    got = _variants()[0][0].point_type.encode_to_curve_batch([v["msg"].encode() for v in ro])
    assert [(g.x, g.y) for g in got] == [_xy(v["P"]) for v in ro]
    nu = _h2c("nu")
    got = _variants()[1][0].point_type.encode_to_curve_batch([v["msg"].encode() for v in nu])
    assert [(g.x, g.y) for g in got] == [_xy(v["P"]) for v in nu]


# ---------------------------------------------------------------- group calls
@pytest.mark.parametrize("cv", [RO, NU])
def test_scalar_mul_edge_scalars(ctx, cv):
    rng = random.Random(3)
    pts = _points(rng, 70)
    edge = [0, 1, 2, r.N - 1, r.N, r.N + 1, 2**256 - 1]
    ks = [edge[i % len(edge)] if i < 3 * len(edge) else rng.randrange(2**256) for i in range(len(pts))]
    raw = ctx.bsn_scalar_mul_batch(b"".join(map(r.raw, pts)), _sc(ks), cv)
    for i, (pt, k) in enumerate(zip(pts, ks)):
        assert raw[64 * i : 64 * i + 64] == r.raw(r.mul(k % r.N, pt)), (i, k)
    assert ctx.bsn_scalar_mul_batch(bytes(64), _sc([12345]), cv) == bytes(64)


def test_point_mul_python(ctx):
    import dot_ring_amd as d

    g = d.Secp256k1.point_type.generator_point()
    assert (g * 0).is_identity() and (g * r.N).is_identity() and g * 1 == g and g * (r.N + 1) == g
    assert ((g * -3).x, (g * -3).y) == r.neg(r.mul(3, r.G))
    q = 5 * g
    assert (q.x, q.y) == r.mul(5, r.G) and d.Secp256k1.curve.valid_point(q)


@pytest.mark.parametrize("m", [1, 2, 63, 64, 65])
def test_msm_groups(ctx, m):
    rng = random.Random(5 + m)
    if m == 65:                                   # the grouped call takes at most 64 terms: the single MSM serves 65
        pts = _points(rng, 65)
        ks = [rng.randrange(2**256) for _ in pts]
        assert ctx.bsn_msm(b"".join(map(r.raw, pts)), _sc(ks), RO) == r.raw(r.msm(pts, ks))
        return
    groups = 5
    pts, ks = [], []
    for g in range(groups):
        gp = _points(rng, m)
        gk = [rng.randrange(2**256) for _ in gp]
        if m >= 2 and g == 1:
            gp[1], gk[1] = gp[0], gk[0]                  # P + P inside one group
        if m >= 2 and g == 2:
            gp[1], gk[1] = r.neg(gp[0]), gk[0]           # P + (-P) inside one group
        if g == 3:
            gp[0] = None                                 # an identity term
        pts += gp
        ks += gk
    raw = ctx.bsn_msm_groups(b"".join(map(r.raw, pts)), _sc(ks), m, RO)
    for g in range(groups):
        assert raw[64 * g : 64 * g + 64] == r.raw(r.msm(pts[g * m : g * m + m], ks[g * m : g * m + m])), g
    if m >= 2:
        q = _points(rng, 1)[0]
        assert ctx.bsn_msm_groups(r.raw(q) + r.raw(r.neg(q)), _sc([7, 7]), 2, NU) == bytes(64)


@pytest.mark.parametrize("n", [1, 64, 65, 4097])
def test_single_msm(ctx, n):
    import dot_ring_amd as d

    rng = random.Random(11 + n)
    base = _points(rng, 8)
    pts = [base[i % 8] for i in range(n)]
    ks = [rng.randrange(r.N) for _ in range(n)]
    sums = [sum(ks[i] for i in range(j, n, 8)) % r.N for j in range(8)]
    want = r.msm(base, sums)
    assert ctx.bsn_msm(b"".join(map(r.raw, pts)), _sc(ks), RO) == r.raw(want)
    if n == 65:
        pt_cls = d.Secp256k1.point_type
        got = pt_cls.msm([pt_cls(*p) for p in pts], ks)
        assert (got.x, got.y) == want
    assert ctx.bsn_msm(b"", b"", RO) == bytes(64)


def test_fixed_base_groups(ctx):
    rng = random.Random(17)
    ks = [rng.randrange(2**256) for _ in range(40)] + [0, r.N]
    for base in (r.G, r.BLINDING):
        raw = ctx.te_fixed_base_msm_groups(r.raw(base), _sc(ks), RO)
        for i, k in enumerate(ks):
            assert raw[64 * i : 64 * i + 64] == r.raw(r.mul(k % r.N, base)), i
    raw = ctx.te_fixed_base_msm_groups(r.raw(r.G) + r.raw(r.BLINDING), _sc(ks), NU)
    for g in range(len(ks) // 2):
        assert raw[64 * g : 64 * g + 64] == r.raw(r.msm([r.G, r.BLINDING], ks[2 * g : 2 * g + 2])), g


# ---------------------------------------------------------------- decoding
def test_decode_points(ctx):
    import dot_ring_amd as d

    rng = random.Random(23)
    pts = _points(rng, 40)
    assert {p[1] & 1 for p in pts} == {0, 1}
    encs = [r.encode(p) for p in pts]
    x = 1
    while r.sqrt(r.rhs(x)) is not None:
        x += 1
    gx = r.G[0].to_bytes(32, "big")
    encs += [b"\x02" + r.P.to_bytes(32, "big"), b"\x03" + (2**256 - 1).to_bytes(32, "big"), b"\x02" + x.to_bytes(32, "big"),
             b"\x03" + x.to_bytes(32, "big"), b"\x00" + gx, b"\x04" + gx, b"\x05" + gx, b"\x00" + bytes(32), b"\x82" + gx]
    blob = b"".join(encs)
    for check in (True, False):
        out, ok = ctx.secp256k1_decode_points(blob, check)
        for i, e in enumerate(encs):
            want = r.decode(e, check)
            assert ok[i] == (0 if want == "bad" else 1), (i, check)
            assert out[64 * i : 64 * i + 64] == (bytes(64) if want == "bad" else r.raw(want)), (i, check)
    for cv in (RO, NU):
        out, ok = ctx.bsn_decode_points(blob, cv)
        assert bytes(ok) == bytes([0 if r.decode(e) == "bad" else 1 for e in encs])
    with pytest.raises(ValueError):
        ctx.secp256k1_decode_points(blob[:-1])
    from dot_ring_amd.vrf.codec import dec_point, dec_points

    got = dec_points(d.Secp256k1, encs[:40])
    assert [(g.x, g.y) for g in got] == pts
    for bad in encs[40:] + [encs[0][:32], encs[0] + b"\x00"]:
        with pytest.raises(ValueError):
            dec_point(d.Secp256k1, bad)


# ---------------------------------------------------------------- the VRFs
def _flip(blob, pos):
    return blob[:pos] + bytes([blob[pos] ^ 1]) + blob[pos + 1 :]


def _verifies(fn):
    """a verifier's verdict; an altered proof may also fail to decode"""
    try:
        return bool(fn())
    except ValueError:
        return False


@pytest.mark.parametrize("variant", ["ro", "nu"])
def test_base_records(ctx, variant):
    import dot_ring_amd as d

    cv, ref = _variants()[0 if variant == "ro" else 1]
    other_pk = cv.public_key_from_secret((99).to_bytes(32, "little"))
    for v in _base():
        sk, pk, al, ad = (bytes.fromhex(v[k]) for k in ("sk", "pk", "alpha", "ad"))
        assert cv.public_key_from_secret(sk) == pk
        for salt in (b"", b"salt"):
            tiny = d.TinyVRF[cv].prove(al, sk, ad, salt)
            thin = d.ThinVRF[cv].prove(al, sk, ad, salt)
            ped = d.PedersenVRF[cv].prove(al, sk, ad, salt)
            want_ped, blinding = ref.pedersen_prove(sk, al, ad, salt=salt)
            assert tiny.encode() == ref.ietf_prove(sk, al, ad, salt=salt) and len(tiny.encode()) == 81
            assert thin.encode() == ref.ietf_prove(sk, al, ad, thin=True, salt=salt) and len(thin.encode()) == 98
            assert ped.encode() == want_ped and len(want_ped) == 196
            gamma = ref.mul(r.le(sk), ref.e2c(salt + al))
            assert d.TinyVRF[cv].proof_to_hash(tiny.output_point) == ref.point_to_hash(gamma)
            for vrf, proof, widths in ((d.TinyVRF[cv], tiny, (33, 16, 32)), (d.ThinVRF[cv], thin, (33, 33, 32))):
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
            for w in (33, 33, 33, 33, 32, 32):
                assert not _verifies(lambda: d.PedersenVRF[cv].decode(_flip(blob, pos + w - 1)).verify(al, ad, salt))
                pos += w
    kp_pk, kp_sk = cv.secret_from_seed(bytes(range(32)))
    assert cv.public_key_from_secret(kp_sk) == kp_pk and r.encode(r.mul(r.le(kp_sk) % r.N, r.G)) == kp_pk


@pytest.mark.parametrize("scheme", ["tiny", "thin", "pedersen"])
def test_prove_batch_300(ctx, scheme):
    import dot_ring_amd as d

    cv, ref = _variants()[0]
    vrf = {"tiny": d.TinyVRF, "thin": d.ThinVRF, "pedersen": d.PedersenVRF}[scheme][cv]
    rng = random.Random(13)
    B = 300
    sks = [rng.randrange(1, r.N).to_bytes(32, "little") for _ in range(B)]
    als = [b"alpha-%d" % i for i in range(B)]
    ads = [b"ad-%d" % (i % 5) for i in range(B)]
    salts = [b"s%d" % i if i % 2 else b"" for i in range(B)]
    proofs = vrf.prove_batch(als, sks, ads, salts)
    for i in range(B):
        if scheme == "pedersen":
            want, _ = ref.pedersen_prove(sks[i], als[i], ads[i], salt=salts[i])
        else:
            want = ref.ietf_prove(sks[i], als[i], ads[i], thin=scheme == "thin", salt=salts[i])
        assert proofs[i].encode() == want, i
    for i in (0, 17, B - 1):
        assert vrf.prove(als[i], sks[i], ads[i], salts[i]).encode() == proofs[i].encode()
    pks = [cv.public_key_from_secret(sk) for sk in sks]
    if scheme == "tiny":                                           # Tiny proofs carry no R: they verify one by one
        assert all(proofs[i].verify(pks[i], als[i], ads[i], salts[i]) for i in range(0, B, 10))
        bad = vrf.decode(proofs[7].encode())
        bad.s = (bad.s + 1) % r.N
        assert not bad.verify(pks[7], als[7], ads[7], salts[7])
    if scheme == "thin":
        assert vrf.batch_verify(proofs, pks, als, ads, salts)
        bad = vrf.decode(proofs[7].encode())
        bad.s = (bad.s + 1) % r.N
        assert not vrf.batch_verify(proofs[:7] + [bad] + proofs[8:], pks, als, ads, salts)
    if scheme == "pedersen":
        assert vrf.batch_verify(proofs, als, ads, salts)
        p = proofs[5]
        bad = type(p)(p.output_point, p.blinded_pk, p.result_point, p.ok, p.s, (p.sb + 1) % r.N)
        assert not vrf.batch_verify(proofs[:5] + [bad] + proofs[6:], als, ads, salts)
    # the nonuniform variant through the same batch calls
    cvn, refn = _variants()[1]
    vrfn = {"tiny": d.TinyVRF, "thin": d.ThinVRF, "pedersen": d.PedersenVRF}[scheme][cvn]
    got = vrfn.prove_batch(als[:20], sks[:20], ads[:20], salts[:20])
    for i in range(20):
        want = refn.pedersen_prove(sks[i], als[i], ads[i], salt=salts[i])[0] if scheme == "pedersen" else \
            refn.ietf_prove(sks[i], als[i], ads[i], thin=scheme == "thin", salt=salts[i])
        assert got[i].encode() == want, i


def test_refusals(ctx):
    import dot_ring_amd as d
    from dot_ring_amd import _native

    lib = _native.lib()
    off = (ctypes.c_uint64 * 2)(0, 0)
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dot_ring_amd", "data",
                           "bls12-381-srs-2-11-uncompressed-zcash.bin"), "rb") as f:
        blob = f.read()
    srs = ctx.srs_load(blob[8 : 8 + 96 * 1537])
    for cv, cid in ((d.Secp256k1_RO, RO), (d.Secp256k1_NU, NU)):
        suite = cv.point_type._suite_struct()
        assert suite.xof == 2 and suite.curve == cid
        out = ctypes.c_void_p()
        rc = lib.dr_ring_prover_create_te(ctx.handle, cid, srs.handle, 9, 1, bytes(32), bytes(32), bytes(64 * 512), bytes(64), ctypes.byref(out))
        assert rc == _native.DR_ERR_INVALID and not out.value
        verdict = ctypes.create_string_buffer(1)
        rc = lib.dr_ietf_verify_batch(ctx.handle, ctypes.byref(suite), 0, 1, bytes(81), bytes(33), b"", off, b"", off, None, None, verdict)
        assert rc == _native.DR_ERR_INVALID
        vk = _native.RingVerifierKeyStruct()
        vk.log2n, vk.fs_prefix, vk.fs_prefix_len = 9, b"x", 1
        ok = ctypes.c_int(0)
        rc = lib.dr_ringvrf_verify_batch(ctx.handle, ctypes.byref(suite), ctypes.byref(vk), 1, bytes(784), b"", off, b"", off, None, None,
                                         bytes(32), ctypes.byref(ok))
        assert rc == _native.DR_ERR_INVALID and ok.value == 0
        # a transcript hash other than SHA-256 is refused for these curves
        bad = _native.vrf_suite(suite._keep, 0, bytes(suite.generator_xy), bytes(suite.blinding_base_xy), cid)
        out_xy = ctypes.create_string_buffer(64)
        rc = lib.dr_encode_to_curve_batch(ctx.handle, ctypes.byref(bad), b"a", (ctypes.c_uint64 * 2)(0, 1), None, None, 1, out_xy)
        assert rc == _native.DR_ERR_INVALID
        with pytest.raises(ValueError):
            d.RingProofParams(cv=cv)
    srs.close()
    # the dr_bsn_* (GLV) names carry no curve id and are Bandersnatch's: a secp256k1 point is not even a pair of elements of its field
    out = ctypes.create_string_buffer(64)
    assert lib.dr_bsn_scalar_mul_batch(ctx.handle, r.raw(r.G), _sc([1]), 1, out) == _native.DR_ERR_INVALID
    assert lib.dr_bsn_msm(ctx.handle, r.raw(r.G), _sc([1]), 1, out) == _native.DR_ERR_INVALID


def test_no_secret_residue_after_prove(ctx):
    import dot_ring_amd as d
    from dot_ring_amd import runtime

    c = runtime.context()
    for cv in (d.Secp256k1_RO, d.Secp256k1_NU):
        for vrf in (d.TinyVRF[cv], d.ThinVRF[cv], d.PedersenVRF[cv]):
            vrf.prove_batch([b"r%d" % i for i in range(70)], [(1000 + i).to_bytes(32, "little") for i in range(70)], [b""] * 70)
            assert c.scratch_residue() == 0


def test_other_suites_after_secp256k1_calls(ctx, golden_dir):
    import dot_ring_amd as d

    d.PedersenVRF[d.Secp256k1].prove_batch([b"a"] * 80, [(7).to_bytes(32, "little")] * 80, [b""] * 80)
    fields = ("gamma", "proof_pk_com", "proof_r", "proof_ok", "proof_s", "proof_sb")
    for rel, cv in (("ark-vrf/bandersnatch_sha-512_ell2_pedersen.json", d.Bandersnatch),
                    ("ark-vrf/jubjub_sha-512_tai_pedersen.json", d.JubJub),
                    ("ark-vrf/bandersnatch_sw_sha-512_tai_pedersen.json", d.Bandersnatch_SW),
                    ("ark-vrf/ed25519_sha-512_tai_pedersen.json", d.Ed25519),
                    ("ark-vrf/secp256r1_sha-256_tai_pedersen.json", d.P256)):
        vectors = json.load(open(os.path.join(golden_dir, rel)))
        hx = lambda v, k: bytes.fromhex(v[k])  # noqa: E731
        batch = d.PedersenVRF[cv].prove_batch([hx(v, "alpha") for v in vectors] * 12, [hx(v, "sk") for v in vectors] * 12,
                                              [hx(v, "ad") for v in vectors] * 12)
        assert [p.encode() for p in batch] == [b"".join(hx(v, f) for f in fields) for v in vectors] * 12
