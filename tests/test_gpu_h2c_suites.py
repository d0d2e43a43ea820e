"""The RFC 9380 variants of P-256 and Ed25519 on the GPU (DR_CURVE_P256_RO = 8, DR_CURVE_P256_NU = 9, DR_CURVE_ED25519_RO = 10,
DR_CURVE_ED25519_NU = 11): hash_to_field and the two map kernels against the hash-to-curve vectors the reference holds and against
the big-integer restatement (h2c_ref.py), edge inputs, the SEC1 mode of the P-256 decoder, and the Tiny / Thin / Pedersen provers and
verifiers against the restatement's bytes.  The reference holds no proof vectors for these variants, and no recordings of its own
outputs exist (its package imports gmpy2 unconditionally); test_h2c_suites_cpu.py shows the restatement's VRF layer reproducing the
reference's P-256 and Ed25519 try-and-increment proof files."""
import ctypes
import json
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ed25519_ref as ed  # noqa: E402
import h2c_ref as h  # noqa: E402
import p256_ref as p256  # noqa: E402
import secp256k1_ref as k1  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ("p256_ro", "p256_nu", "ed25519_ro", "ed25519_nu")
ED_ID = ed.raw(ed.O)


def _h2c(name):
    return json.load(open(os.path.join(GOLDEN, "h2c", f"{name}.json")))["vectors"]


def _base(curve):
    return json.load(open(os.path.join(GOLDEN, "base", f"{curve}_base_vectors.json")))


def _xy(v):
    return int(v["x"], 16), int(v["y"], 16)


def _us(us):
    return b"".join(u.to_bytes(32, "little") for u in us)


def _sc(ks):
    return b"".join(k.to_bytes(32, "little") for k in ks)


def _suite(name):
    """(curve variant, restatement suite, restated hash_to_field, DST, elements per message, is Ed25519)"""
    import dot_ring_amd as d

    return {"p256_ro": (d.P256_RO, h.P256_RO, h.p256_hash_to_field, h.P256_DST_RO, 2, False),
            "p256_nu": (d.P256_NU, h.P256_NU, h.p256_hash_to_field, h.P256_DST_NU, 1, False),
            "ed25519_ro": (d.Ed25519_RO, h.ED25519_RO, h.ed_hash_to_field, h.ED_DST_RO, 2, True),
            "ed25519_nu": (d.Ed25519_NU, h.ED25519_NU, h.ed_hash_to_field, h.ED_DST_NU, 1, True)}[name]


def _ed_image8(us):
    """what k_ed25519_map_to_curve returns for one item: 8 times the sum of the images, or None where an image has no value"""
    acc = ed.O
    for u in us:
        try:
            acc = ed.add(acc, h.ed_map_to_curve(u))
        except ValueError:
            return None
    return h.ed_clear_cofactor(acc)


def _p256_image(us):
    acc = None
    for u in us:
        acc = p256.add(acc, h.p256_map_to_curve(u))
    return acc


def _check_ed_items(ctx, items, per):
    out, ok = ctx.ed25519_map_to_curve(_us([u for it in items for u in it]), per)
    for i, it in enumerate(items):
        want = _ed_image8(it)
        assert ok[i] == (0 if want is None else 1), (i, it)
        if want is not None:
            assert out[64 * i : 64 * i + 64] == ed.raw(want), (i, it)
    return out, ok


def _check_p256_items(ctx, items, per):
    out, ok = ctx.p256_map_to_curve(_us([u for it in items for u in it]), per)
    assert bytes(ok) == b"\x01" * len(items)
    for i, it in enumerate(items):
        assert out[64 * i : 64 * i + 64] == p256.raw(_p256_image(it)), (i, it)
    return out


# ---------------------------------------------------------------- hash to field and the maps
@pytest.mark.parametrize("name", NAMES)
def test_hash_to_field_vectors(ctx, name):
    from dot_ring_amd import _native

    cv, _, _, _, count, _ = _suite(name)
    vs = _h2c(name)
    got = _native.hash_to_field_batch(cv.point_type._suite_struct(), [v["msg"].encode() for v in vs])
    assert got == _us([int(u, 16) for v in vs for u in v["u"]]) and len(got) == 32 * count * len(vs)


def test_p256_map_vectors(ctx):
    ro, nu = _h2c("p256_ro"), _h2c("p256_nu")
    singles = [(int(u, 16), _xy(q)) for v in ro for u, q in ((v["u"][0], v["Q0"]), (v["u"][1], v["Q1"]))]
    singles += [(int(v["u"][0], 16), _xy(v["Q"])) for v in nu]
    out, ok = ctx.p256_map_to_curve(_us([u for u, _ in singles]), 1)
    assert bytes(ok) == b"\x01" * len(singles)
    assert out == b"".join(p256.raw(q) for _, q in singles)
    out, ok = ctx.p256_map_to_curve(_us([int(u, 16) for v in ro for u in v["u"]]), 2)
    assert bytes(ok) == b"\x01" * len(ro) and out == b"".join(p256.raw(_xy(v["P"])) for v in ro)
    # NU: P = Q (cofactor 1)
    assert [_xy(v["P"]) for v in nu] == [_xy(v["Q"]) for v in nu]


def test_ed25519_map_vectors(ctx):
    ro, nu = _h2c("ed25519_ro"), _h2c("ed25519_nu")
    # the kernel clears the cofactor, so a single image comes back as 8 Q: against 8 times the vector's Q0 / Q1 / Q, and for the
    # nonuniform vectors that is P itself
    singles = [(int(u, 16), _xy(q)) for v in ro for u, q in ((v["u"][0], v["Q0"]), (v["u"][1], v["Q1"]))]
    singles += [(int(v["u"][0], 16), _xy(v["Q"])) for v in nu]
    out, ok = ctx.ed25519_map_to_curve(_us([u for u, _ in singles]), 1)
    assert bytes(ok) == b"\x01" * len(singles)
    assert out == b"".join(ed.raw(h.ed_clear_cofactor(q)) for _, q in singles)
    assert out[64 * 2 * len(ro) :] == b"".join(ed.raw(_xy(v["P"])) for v in nu)
    out, ok = ctx.ed25519_map_to_curve(_us([int(u, 16) for v in ro for u in v["u"]]), 2)
    assert bytes(ok) == b"\x01" * len(ro) and out == b"".join(ed.raw(_xy(v["P"])) for v in ro)
    # the host's single image (no cofactor cleared) is the vector's Q itself
    import dot_ring_amd as d

    for u, q in singles:
        got = d.Ed25519_RO.point_type.map_to_curve(u)
        assert (got.x, got.y) == q


def test_p256_map_edge_inputs(ctx):
    p, z = p256.P, h.P256_Z
    edge = [0, 1, p - 1]
    # the u != 0 with Z^2 u^4 + Z u^2 = 0 is u^2 = -1 / Z: it exists iff -1 / Z = 1 / 10 is a square mod p
    w = p256.sqrt(pow(-z, -1, p))
    assert w is not None, "-1/Z is a square mod p256: the exceptional input exists"
    for u in (w, p - w):
        assert (z * z * pow(u, 4, p) + z * u * u) % p == 0 and u != 0
        edge.append(u)
    _check_p256_items(ctx, [(u,) for u in edge], 1)
    _check_p256_items(ctx, [(a, b) for a in edge for b in edge], 2)          # (u, u) doubles, (u, -u) cancels: the restatement says which
    # (u, -u) has the same x and opposite parity of y: the two images cancel and the sum is the identity, 64 zero bytes
    out = _check_p256_items(ctx, [(5, p - 5), (w, p - w)], 2)
    assert out == bytes(128)


def test_ed25519_map_edge_inputs(ctx):
    q = ed.P
    # the u with Z u^2 = -1 would need -1 / 2 to be a square mod 2^255 - 19; it is not (2 is not, -1 is), so no such input exists
    assert pow(-pow(2, -1, q) % q, (q - 1) // 2, q) == q - 1
    edge = [0, 1, q - 1, 2, q - 2]
    assert _ed_image8((0,)) is None                                        # 0 maps to v = 0: the reference's inverse fails
    out, ok = _check_ed_items(ctx, [(u,) for u in edge], 1)
    assert ok[0] == 0 and bytes(ok[1:]) == b"\x01" * 4
    _check_ed_items(ctx, [(a, b) for a in edge for b in edge], 2)
    import dot_ring_amd as d

    with pytest.raises(ValueError):
        d.Ed25519_NU.point_type.encode_to_curve_from_field(bytes(32))


def test_maps_random_inputs_and_membership(ctx):
    from dot_ring_amd import _native

    rng = random.Random(9380)
    n = 4096
    # P-256: every output on the curve and equal to the restatement's, both branches of the map taken
    us = [rng.randrange(p256.P) for _ in range(n)]
    out, ok = ctx.p256_map_to_curve(_us(us), 1)
    assert bytes(ok) == b"\x01" * n
    for i in range(n):
        pt = (int.from_bytes(out[64 * i : 64 * i + 32], "little"), int.from_bytes(out[64 * i + 32 : 64 * i + 64], "little"))
        assert pt[0] < p256.P and pt[1] < p256.P and p256.on_curve(pt) and pt[1] % 2 == us[i] % 2, i
    for i in range(n):
        assert out[64 * i : 64 * i + 64] == p256.raw(h.p256_map_to_curve(us[i])), i
    taken_x2 = sum(1 for u in us[:300] if p256.sqrt(p256.rhs(_p256_x1(u))) is None)
    assert 90 <= taken_x2 <= 210                                            # both branches of the map
    out2, ok = ctx.p256_map_to_curve(_us(us), 2)
    assert bytes(ok) == b"\x01" * (n // 2)
    for i in range(n // 2):
        assert out2[64 * i : 64 * i + 64] == p256.raw(_p256_image(us[2 * i : 2 * i + 2])), i
    # Ed25519: every output in the prime-order subgroup (l P = O through the scalar multiplication kernel) and equal to the restatement's
    us = [rng.randrange(1, ed.P) for _ in range(n)]
    out, ok = ctx.ed25519_map_to_curve(_us(us), 1)
    assert bytes(ok) == b"\x01" * n
    # the kernel reduces scalars mod l, so l P = O is asked for as (l - 1) P = -P
    lm1 = ctx.bsn_scalar_mul_batch(out, _sc([ed.N - 1] * n), _native.CURVE_ED25519)
    for i in range(n):
        x = int.from_bytes(out[64 * i : 64 * i + 32], "little")
        assert lm1[64 * i : 64 * i + 32] == (-x % ed.P).to_bytes(32, "little") and lm1[64 * i + 32 : 64 * i + 64] == out[64 * i + 32 : 64 * i + 64], i
        assert out[64 * i : 64 * i + 64] != ED_ID
    squares = 0
    for i in range(n):
        assert out[64 * i : 64 * i + 64] == ed.raw(_ed_image8((us[i],))), i
    for i in range(300):
        x1 = -h.MONT_A * pow(2 * us[i] * us[i] + 1, -1, ed.P) % ed.P
        squares += pow(((x1 + h.MONT_A) * x1 + 1) * x1 % ed.P, (ed.P - 1) // 2, ed.P) == 1
    assert 90 <= squares <= 210                                             # both branches of Elligator 2
    out2, ok = ctx.ed25519_map_to_curve(_us(us), 2)
    assert bytes(ok) == b"\x01" * (n // 2)
    for i in range(n // 2):
        assert out2[64 * i : 64 * i + 64] == ed.raw(_ed_image8(us[2 * i : 2 * i + 2])), i


def _p256_x1(u):
    p, a, b, z = p256.P, p256.A, p256.B, h.P256_Z
    tv1 = (z * z * pow(u, 4, p) + z * u * u) % p
    return b * pow(z * a % p, -1, p) % p if tv1 == 0 else -b * pow(a, -1, p) * (1 + pow(tv1, -1, p)) % p


def test_maps_refuse_noncanonical_inputs(ctx):
    from dot_ring_amd import _native

    lib = _native.lib()
    out, ok = ctypes.create_string_buffer(128), ctypes.create_string_buffer(2)
    for fn, p in ((lib.dr_p256_map_to_curve, p256.P), (lib.dr_ed25519_map_to_curve, ed.P)):
        for bad in (p, p + 1, 2**256 - 1):
            assert fn(ctx.handle, _us([5, bad]), 2, 1, out, ok) == _native.DR_ERR_INVALID
            assert fn(ctx.handle, _us([bad, 5]), 1, 2, out, ok) == _native.DR_ERR_INVALID
        assert fn(ctx.handle, _us([5, p - 1]), 1, 2, out, ok) == 0
        assert fn(ctx.handle, _us([5]), 1, 3, out, ok) == _native.DR_ERR_INVALID
        assert fn(ctx.handle, None, 0, 1, None, None) == 0
    with pytest.raises(ValueError):
        ctx.p256_map_to_curve(bytes(33), 1)


# ---------------------------------------------------------------- encode to curve
@pytest.mark.parametrize("name", NAMES)
def test_encode_to_curve_batch(ctx, name):
    cv, ref, _, _, _, is_ed = _suite(name)
    raw = ed.raw if is_ed else p256.raw
    rng = random.Random(300)
    msgs = [v["msg"].encode() for v in _h2c(name)] + [rng.randbytes(n) for n in range(301)]      # lengths 0 .. 300, the empty one included
    assert msgs.count(b"") == 2
    got = ctx.encode_to_curve_batch(cv.point_type._suite_struct(), msgs, None)
    vs = _h2c(name)
    assert got[: 64 * len(vs)] == b"".join(raw(_xy(v["P"])) for v in vs)
    for i, m in enumerate(msgs):
        assert got[64 * i : 64 * i + 64] == raw(ref.e2c(m)), i
    # salted: salt || message is what is hashed; the point type's calls agree
    salts = [b"", b"salt", b"s" * 40]
    salted = ctx.encode_to_curve_batch(cv.point_type._suite_struct(), [b"", b"abc", msgs[9]], salts)
    assert salted == b"".join(raw(ref.e2c(s + m)) for s, m in zip(salts, [b"", b"abc", msgs[9]]))
    pt = cv.point_type.encode_to_curve(b"abc", b"salt")
    assert (pt.x, pt.y) == ref.e2c(b"saltabc")
    pts = cv.point_type.encode_to_curve_from_field(cv.point_type.hash_to_field_pairs([b"abc", b"x"], [b"salt", b""]))
    assert [(q.x, q.y) for q in pts] == [ref.e2c(b"saltabc"), ref.e2c(b"x")]


# ---------------------------------------------------------------- the P-256 SEC1 codec
def test_p256_sec1_decode(ctx):
    import dot_ring_amd as d
    from dot_ring_amd.vrf.codec import dec_point, dec_points, enc_point

    rng = random.Random(23)
    pts = [p256.mul(rng.randrange(1, p256.N), p256.G) for _ in range(40)]
    assert {p[1] & 1 for p in pts} == {0, 1}
    encs = [h.p256_sec1_encode(p) for p in pts]
    x = 1
    while p256.sqrt(p256.rhs(x)) is not None:
        x += 1
    gx = p256.G[0].to_bytes(32, "big")
    tai_forms = [p256.encode(p) for p in pts[:6]] + [bytes(32) + b"\x40"]
    encs += [b"\x02" + p256.P.to_bytes(32, "big"), b"\x03" + (2**256 - 1).to_bytes(32, "big"), b"\x02" + x.to_bytes(32, "big"),
             b"\x03" + x.to_bytes(32, "big"), b"\x00" + gx, b"\x04" + gx, b"\x05" + gx, b"\x00" + bytes(32), b"\x82" + gx] + tai_forms
    blob = b"".join(encs)
    for cid in (8, 9):
        out, ok = ctx.bsn_decode_points(blob, cid)
        for i, e in enumerate(encs):
            want = h.p256_sec1_decode(e)
            assert ok[i] == (0 if want == "bad" else 1), (i, cid)
            assert out[64 * i : 64 * i + 64] == (bytes(64) if want == "bad" else p256.raw(want)), (i, cid)
    # the try-and-increment suite reads the same strings by ITS rules: its own forms decode, and a SEC1 string is read canonically first
    out, ok = ctx.bsn_decode_points(blob, 4)
    for i, e in enumerate(encs):
        want = p256.decode(e)
        assert ok[i] == (0 if want == "bad" else 1), i
    assert bytes(ok[-7:-1]) == b"\x01" * 6
    got = dec_points(d.P256_RO, encs[:40])
    assert [(g.x, g.y) for g in got] == pts and [enc_point(g) for g in got] == encs[:40]
    for bad in encs[40:49] + [encs[0][:32], encs[0] + b"\x00"]:
        with pytest.raises(ValueError):
            dec_point(d.P256_RO, bad)
    # 0x00 and 0x04 forms on the host, as Secp256k1Point treats them
    pt_cls = d.P256_NU.point_type
    assert pt_cls.string_to_point(b"\x00").is_identity()
    q = pt_cls.string_to_point(b"\x04" + gx + p256.G[1].to_bytes(32, "big"))
    assert (q.x, q.y) == p256.G and q.point_to_string(compressed=False)[0] == 4


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

    cv, ref, _, _, _, is_ed = _suite(name)
    pl = 32 if is_ed else 33
    recs = _base("ed25519" if is_ed else "p256")
    assert len(recs) == 5
    other_pk = cv.public_key_from_secret((99).to_bytes(32, "little"))
    for v in recs:
        sk, al, ad = (bytes.fromhex(v[k]) for k in ("sk", "alpha", "ad"))
        pk = cv.public_key_from_secret(sk)
        assert pk == ref.enc(ref.mul(k1.le(sk), ref.g))
        if v["pk"]:
            assert pk.hex() == v["pk"]
        else:
            assert is_ed                                    # Ed25519's file leaves pk empty
        for salt in (b"", b"salt"):
            tiny = d.TinyVRF[cv].prove(al, sk, ad, salt)
            thin = d.ThinVRF[cv].prove(al, sk, ad, salt)
            ped = d.PedersenVRF[cv].prove(al, sk, ad, salt)
            want_ped, blinding = ref.pedersen_prove(sk, al, ad, salt=salt)
            lengths = (80, 96, 192) if is_ed else (81, 98, 196)
            assert (len(tiny.encode()), len(thin.encode()), len(ped.encode())) == lengths
            assert tiny.encode() == ref.ietf_prove(sk, al, ad, salt=salt)
            assert thin.encode() == ref.ietf_prove(sk, al, ad, thin=True, salt=salt)
            assert ped.encode() == want_ped
            for vrf, proof, widths in ((d.TinyVRF[cv], tiny, (pl, 16, 32)), (d.ThinVRF[cv], thin, (pl, pl, 32))):
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
            for w in (pl, pl, pl, pl, 32, 32):
                assert not _verifies(lambda: d.PedersenVRF[cv].decode(_flip(blob, pos + w - 1)).verify(al, ad, salt))
                pos += w


@pytest.mark.parametrize("scheme", ["tiny", "thin", "pedersen"])
@pytest.mark.parametrize("name", NAMES)
def test_prove_batch_300(ctx, name, scheme):
    import dot_ring_amd as d

    cv, ref, _, _, _, _ = _suite(name)
    vrf = {"tiny": d.TinyVRF, "thin": d.ThinVRF, "pedersen": d.PedersenVRF}[scheme][cv]
    rng = random.Random(13)
    B = 300
    sks = [rng.randrange(1, ref.n).to_bytes(32, "little") for _ in range(B)]
    als = [b"alpha-%d" % i for i in range(B)]
    ads = [b"ad-%d" % (i % 5) for i in range(B)]
    salts = [b"s%d" % i if i % 2 else b"" for i in range(B)]
    proofs = vrf.prove_batch(als, sks, ads, salts)
    for i in range(B):                                             # the single calls
        assert vrf.prove(als[i], sks[i], ads[i], salts[i]).encode() == proofs[i].encode(), i
    for i in range(0, B, 25):                                      # and the restatement
        if scheme == "pedersen":
            want, _ = ref.pedersen_prove(sks[i], als[i], ads[i], salt=salts[i])
        else:
            want = ref.ietf_prove(sks[i], als[i], ads[i], thin=scheme == "thin", salt=salts[i])
        assert proofs[i].encode() == want, i
    pks = [cv.public_key_from_secret(sk) for sk in sks[:40]]
    if scheme == "tiny":                                           # Tiny proofs carry no R: they verify one by one
        assert all(proofs[i].verify(pks[i], als[i], ads[i], salts[i]) for i in range(0, 40, 5))
        bad = vrf.decode(proofs[7].encode())
        bad.s = (bad.s + 1) % ref.n
        assert not bad.verify(pks[7], als[7], ads[7], salts[7])
    if scheme == "thin":
        assert vrf.batch_verify(proofs[:40], pks, als[:40], ads[:40], salts[:40])
        bad = vrf.decode(proofs[7].encode())
        bad.s = (bad.s + 1) % ref.n
        assert not vrf.batch_verify(proofs[:7] + [bad] + proofs[8:40], pks, als[:40], ads[:40], salts[:40])
    if scheme == "pedersen":
        assert vrf.batch_verify(proofs, als, ads, salts)
        p = proofs[5]
        bad = type(p)(p.output_point, p.blinded_pk, p.result_point, p.ok, p.s, (p.sb + 1) % ref.n)
        assert not vrf.batch_verify(proofs[:5] + [bad] + proofs[6:], als, ads, salts)


# ---------------------------------------------------------------- refusals, residue, the other suites
def test_refusals(ctx):
    import dot_ring_amd as d
    from dot_ring_amd import _native

    lib = _native.lib()
    off = (ctypes.c_uint64 * 2)(0, 0)
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dot_ring_amd", "data",
                           "bls12-381-srs-2-11-uncompressed-zcash.bin"), "rb") as f:
        blob = f.read()
    srs = ctx.srs_load(blob[8 : 8 + 96 * 1537])
    for cv, cid, xof, wrong in ((d.P256_RO, 8, 2, 0), (d.P256_NU, 9, 2, 1), (d.Ed25519_RO, 10, 0, 2), (d.Ed25519_NU, 11, 0, 1)):
        suite = cv.point_type._suite_struct()
        assert suite.xof == xof and suite.curve == cid
        pl = _native.curve_point_len(cid)
        out = ctypes.c_void_p()
        rc = lib.dr_ring_prover_create_te(ctx.handle, cid, srs.handle, 9, 1, bytes(32), bytes(32), bytes(64 * 512), bytes(64), ctypes.byref(out))
        assert rc == _native.DR_ERR_INVALID and not out.value
        verdict = ctypes.create_string_buffer(1)
        rc = lib.dr_ietf_verify_batch(ctx.handle, ctypes.byref(suite), 0, 1, bytes(pl + 48), bytes(pl), b"", off, b"", off, None, None, verdict)
        assert rc == _native.DR_ERR_INVALID
        vk = _native.RingVerifierKeyStruct()
        vk.log2n, vk.fs_prefix, vk.fs_prefix_len = 9, b"x", 1
        ok = ctypes.c_int(0)
        rc = lib.dr_ringvrf_verify_batch(ctx.handle, ctypes.byref(suite), ctypes.byref(vk), 1, bytes(784), b"", off, b"", off, None, None,
                                         bytes(32), ctypes.byref(ok))
        assert rc == _native.DR_ERR_INVALID and ok.value == 0
        # a transcript hash other than the suite's is refused
        bad = _native.vrf_suite(suite._keep, wrong, bytes(suite.generator_xy), bytes(suite.blinding_base_xy), cid)
        out_xy = ctypes.create_string_buffer(64)
        rc = lib.dr_encode_to_curve_batch(ctx.handle, ctypes.byref(bad), b"a", (ctypes.c_uint64 * 2)(0, 1), None, None, 1, out_xy)
        assert rc == _native.DR_ERR_INVALID
        with pytest.raises(ValueError):
            d.RingProofParams(cv=cv)
    srs.close()
    assert _native.lib().dr_te_scalar_mul_batch(ctx.handle, 12, bytes(64), bytes(32), 1, ctypes.create_string_buffer(64)) == _native.DR_ERR_INVALID


def test_no_secret_residue_after_prove(ctx):
    import dot_ring_amd as d
    from dot_ring_amd import runtime

    c = runtime.context()
    for cv in (d.P256_RO, d.P256_NU, d.Ed25519_RO, d.Ed25519_NU):
        for vrf in (d.TinyVRF[cv], d.ThinVRF[cv], d.PedersenVRF[cv]):
            vrf.prove_batch([b"r%d" % i for i in range(70)], [(1000 + i).to_bytes(32, "little") for i in range(70)], [b""] * 70)
            assert c.scratch_residue() == 0


def test_other_suites_after_h2c_calls(ctx, golden_dir):
    import dot_ring_amd as d

    for cv in (d.P256_RO, d.Ed25519_NU):
        d.PedersenVRF[cv].prove_batch([b"a"] * 80, [(7).to_bytes(32, "little")] * 80, [b""] * 80)
    fields = ("gamma", "proof_pk_com", "proof_r", "proof_ok", "proof_s", "proof_sb")
    for rel, cv in (("ark-vrf/ed25519_sha-512_tai_pedersen.json", d.Ed25519), ("ark-vrf/secp256r1_sha-256_tai_pedersen.json", d.P256)):
        vectors = json.load(open(os.path.join(golden_dir, rel)))
        hx = lambda v, k: bytes.fromhex(v[k])  # noqa: E731
        for v in vectors:
            proof = d.PedersenVRF[cv].prove(hx(v, "alpha"), hx(v, "sk"), hx(v, "ad"))
            assert proof.encode() == b"".join(hx(v, f) for f in fields)
    # secp256k1's RO map, whose kernel is now an instance of the shared template
    v = json.load(open(os.path.join(GOLDEN, "h2c", "secp256k1_ro.json")))["vectors"]
    got = ctx.encode_to_curve_batch(d.Secp256k1_RO.point_type._suite_struct(), [x["msg"].encode() for x in v], None)
    assert got == b"".join(k1.raw(_xy(x["P"])) for x in v)
    sk = bytes.fromhex(json.load(open(os.path.join(GOLDEN, "base", "secp256k1_base_vectors.json")))[0]["sk"])
    assert d.TinyVRF[d.Secp256k1].prove(b"abc", sk, b"").encode() == k1.RO.ietf_prove(sk, b"abc", b"")
