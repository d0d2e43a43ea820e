"""Bandersnatch_SW on the GPU (DR_CURVE_BANDERSNATCH_SW): the suite's 8 vector files byte for byte, the SW decoder, the group
calls and try-and-increment of curve 2 against the big-integer restatement (sw_ref.py), proving at batch size, and the other
suites' bytes after SW calls in the same context."""
import glob
import json
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sw_ref as r  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILES = sorted(glob.glob(os.path.join(GOLDEN, "*", "bandersnatch_sw_sha*_tai_*.json")))
CV2 = 2


def _scheme(path):
    import dot_ring_amd as d

    name = os.path.basename(path)
    if "pedersen" in name:
        return d.PedersenVRF, ("gamma", "proof_pk_com", "proof_r", "proof_ok", "proof_s", "proof_sb")
    if "thin" in name:
        return d.ThinVRF, ("gamma", "proof_r", "proof_s")
    return d.TinyVRF, ("gamma", "proof_c", "proof_s")


@pytest.mark.parametrize("path", FILES, ids=lambda p: "/".join(p.split(os.sep)[-2:]))
def test_vectors(ctx, path):
    import dot_ring_amd as d

    cv = d.Bandersnatch_SW
    scheme, fields = _scheme(path)
    vrf = scheme[cv]
    vectors = json.load(open(path))
    hx = lambda v, k: bytes.fromhex(v[k])  # noqa: E731
    proofs = []
    for v in vectors:
        sk, al, ad, pk = hx(v, "sk"), hx(v, "alpha"), hx(v, "ad"), hx(v, "pk")
        want = b"".join(hx(v, f) for f in fields)
        assert cv.public_key_from_secret(sk) == pk
        h = cv.point_type.encode_to_curve(al)
        assert h.point_to_string().hex() == v["h"] and len(h.point_to_string()) == 33
        proof = vrf.prove(al, sk, ad)
        assert proof.encode() == want
        assert vrf.proof_to_hash(proof.output_point).hex() == v["beta"][:64]
        rt = vrf.decode(want)
        assert rt.encode() == want
        if scheme is d.PedersenVRF:
            assert rt.verify(al, ad) and not rt.verify(al, ad + b"\x01") and not rt.verify(al + b"\x01", ad)
            assert rt.verify_unblinding(pk, int.from_bytes(hx(v, "blinding"), "little"))
        else:
            assert rt.verify(pk, al, ad) and not rt.verify(pk, al, ad + b"\x01") and not rt.verify(pk, al + b"\x01", ad)
        proofs.append(rt)
    batch = vrf.prove_batch([hx(v, "alpha") for v in vectors], [hx(v, "sk") for v in vectors], [hx(v, "ad") for v in vectors])
    assert [p.encode() for p in batch] == [b"".join(hx(v, f) for f in fields) for v in vectors]
    ins, ads = [hx(v, "alpha") for v in vectors], [hx(v, "ad") for v in vectors]
    if scheme is d.PedersenVRF:
        assert vrf.batch_verify(proofs, ins, ads)
        bad = vrf.decode(proofs[1].encode())
        bad = type(bad)(bad.output_point, bad.blinded_pk, bad.result_point, bad.ok, (bad.s + 1) % r.N, bad.sb)
        assert not vrf.batch_verify([proofs[0], bad] + proofs[2:], ins, ads)
    elif scheme is d.ThinVRF:
        pks = [hx(v, "pk") for v in vectors]
        assert vrf.batch_verify(proofs, pks, ins, ads)
        bad = vrf.decode(proofs[1].encode())
        bad.s = (bad.s + 1) % r.N
        assert not vrf.batch_verify([proofs[0], bad] + proofs[2:], pks, ins, ads)
    tail = b"".join(hx(vectors[0], f) for f in fields[1:])
    with pytest.raises(ValueError, match="INVALID|Invalid"):
        vrf.decode(b"\xff" * 33 + tail)


def _decode_cases(rng):
    torsion = _two_torsion()
    encs, pts = [], []
    for _ in range(64):
        pts.append(r.mul(rng.randrange(1, r.N), r.G))
    for q in pts[:16]:
        for t in torsion:
            encs.append(r.encode(r.add(q, t)))                 # Q + T: outside the subgroup
    for t in torsion:
        encs.append(t[0].to_bytes(32, "little") + b"\x00")      # y = 0
    encs += [bytes(32) + b"\x40", bytes(32) + b"\xc0"]
    good = r.encode(pts[0])
    encs += [good[:32] + bytes([good[32] | (1 << b)]) for b in range(6)]
    encs += [r.P.to_bytes(32, "little") + b"\x00", (r.P + 5).to_bytes(32, "little") + b"\x80"]
    x = 1
    while r.sqrt(x ** 3 + r.A * x + r.B) is not None:
        x += 1
    encs.append(x.to_bytes(32, "little") + b"\x00")
    encs += [r.encode(p) for p in pts]
    while len(encs) < 4097:                                    # one full block of 4096 lanes and one partial
        encs.append(r.encode(pts[len(encs) % len(pts)]))
    return encs


def _two_torsion():
    a, dd = r.TE_A % r.P, r.TE_D
    am = 2 * (a + dd) * pow(a - dd, -1, r.P) % r.P
    disc, half = r.sqrt(am * am - 4), pow(2, -1, r.P)
    return [((s + r.A3) * pow(r.MB, -1, r.P) % r.P, 0) for s in (0, (-am + disc) * half % r.P, (-am - disc) * half % r.P)]


def test_decode_points_4097(ctx):
    rng = random.Random(3)
    encs = _decode_cases(rng)
    assert len(encs) == 4097
    xy, ok = ctx.bsn_decode_points(b"".join(encs), CV2)
    cache = {}
    for i, e in enumerate(encs):
        if e not in cache:
            cache[e] = r.decode(e)
        want = cache[e]
        assert ok[i] == (want is not None), (i, e.hex())
        if want is not None:
            assert xy[64 * i : 64 * i + 64] == r.raw(want)


def test_group_calls_curve2(ctx):
    rng = random.Random(5)
    pts = [r.mul(rng.randrange(1, r.N), r.G) for _ in range(8)]
    ks = [0, 1, r.N - 1, r.N] + [rng.randrange(r.N) for _ in range(4)]
    le = lambda k: (k % (1 << 256)).to_bytes(32, "little")  # noqa: E731
    n = 200                                                   # kernel path (no host route for this curve)
    P = [pts[i % 8] for i in range(n)]
    K = [ks[i % 8] if i < 8 else rng.randrange(r.N) for i in range(n)]
    out = ctx.bsn_scalar_mul_batch(b"".join(r.raw(p) for p in P), b"".join(le(k) for k in K), CV2)
    for i in list(range(8)) + rng.sample(range(8, n), 8):
        assert out[64 * i : 64 * i + 64] == r.raw(r.mul(K[i] % r.N, P[i])), i
    assert out[64 * 3 : 64 * 4] == bytes(64) and out[0:64] == bytes(64)
    # MSM (host fold of 64-term groups and the bucket method)
    for m in (5, 300):
        PP, KK = P[:m] if m <= n else P, K[:m]
        if m > n:
            PP = [pts[i % 8] for i in range(m)]
            KK = [rng.randrange(r.N) for _ in range(m)]
        got = ctx.bsn_msm(b"".join(r.raw(p) for p in PP), b"".join(le(k) for k in KK), CV2)
        acc = None
        for p, k in zip(PP, KK):
            acc = r.add(acc, r.mul(k % r.N, p))
        assert got == r.raw(acc), m
    got = ctx.bsn_msm(r.raw(pts[0]) * 2, le(1) + le(r.N - 1), CV2)
    assert got == bytes(64)
    # grouped MSMs
    got = ctx.bsn_msm_groups(b"".join(r.raw(p) for p in P[:120]), b"".join(le(k) for k in K[:120]), 3, CV2)
    for g in range(0, 40, 7):
        acc = None
        for j in range(3):
            acc = r.add(acc, r.mul(K[3 * g + j] % r.N, P[3 * g + j]))
        assert got[64 * g : 64 * g + 64] == r.raw(acc)
    # fixed bases G and the blinding base
    bases = r.raw(r.G) + r.raw(r.BLINDING)
    KK = ks + [rng.randrange(r.N) for _ in range(2 * 100 - len(ks))]
    got = ctx.te_fixed_base_msm_groups(bases, b"".join(le(k) for k in KK), CV2)
    for g in list(range(4)) + [50, 99]:
        want = r.add(r.mul(KK[2 * g] % r.N, r.G), r.mul(KK[2 * g + 1] % r.N, r.BLINDING))
        assert got[64 * g : 64 * g + 64] == r.raw(want), g


def test_encode_to_curve_batch_1024(ctx):
    import dot_ring_amd as d

    P = d.Bandersnatch_SW.point_type
    msgs = [b"sw-h2c-%d" % i for i in range(1024)]
    got = P.encode_to_curve_batch(msgs)
    counters = set()
    for i in list(range(0, 1024, 37))[:28] + [1, 2, 3, 4]:
        pt, c = r.encode_to_curve(msgs[i])
        counters.add(c)
        assert (got[i].x, got[i].y) == pt
    extra = [m for m in (b"sw-ctr-%d" % i for i in range(400)) if r.encode_to_curve(m)[1] >= 2][:2]
    for m in extra:
        assert (P.encode_to_curve(m).x, P.encode_to_curve(m).y) == r.encode_to_curve(m)[0]
    assert max(counters) >= 1 and len(extra) == 2


@pytest.mark.parametrize("scheme", ["tiny", "pedersen"])
def test_prove_batch_1000(ctx, scheme):
    import dot_ring_amd as d

    cv = d.Bandersnatch_SW
    vrf = d.TinyVRF[cv] if scheme == "tiny" else d.PedersenVRF[cv]
    rng = random.Random(11)
    B = 1000
    sks = [rng.randrange(1, r.N).to_bytes(32, "little") for _ in range(B)]
    als = [b"alpha-%d" % i for i in range(B)]
    ads = [b"ad-%d" % (i % 7) for i in range(B)]
    proofs = vrf.prove_batch(als, sks, ads)
    for i in rng.sample(range(B), 4):
        assert vrf.prove(als[i], sks[i], ads[i]).encode() == proofs[i].encode()
    if scheme == "tiny":
        pks = [cv.public_key_from_secret(sk) for sk in sks]
        for i in rng.sample(range(B), 6):
            assert proofs[i].verify(pks[i], als[i], ads[i])
        assert d.ThinVRF[cv].batch_verify(d.ThinVRF[cv].prove_batch(als[:64], sks[:64], ads[:64]), pks[:64], als[:64], ads[:64])
        bad = vrf.decode(proofs[0].encode())
        bad.s = (bad.s + 1) % r.N
        assert not bad.verify(pks[0], als[0], ads[0])
    else:
        assert vrf.batch_verify(proofs, als, ads)
        p = proofs[5]
        bad = type(p)(p.output_point, p.blinded_pk, p.result_point, p.ok, p.s, (p.sb + 1) % r.N)
        assert not vrf.batch_verify(proofs[:5] + [bad] + proofs[6:], als, ads)


def test_other_suites_after_sw_calls(ctx, golden_dir):
    import dot_ring_amd as d

    sw = d.Bandersnatch_SW
    d.PedersenVRF[sw].prove_batch([b"a"] * 80, [(7).to_bytes(32, "little")] * 80, [b""] * 80)    # fills the SW suite's table entries
    for rel, cv in (("ark-vrf/bandersnatch_sha-512_ell2_pedersen.json", d.Bandersnatch),
                    ("ark-vrf/jubjub_sha-512_tai_pedersen.json", d.JubJub)):
        vectors = json.load(open(os.path.join(golden_dir, rel)))
        hx = lambda v, k: bytes.fromhex(v[k])  # noqa: E731
        fields = ("gamma", "proof_pk_com", "proof_r", "proof_ok", "proof_s", "proof_sb")
        batch = d.PedersenVRF[cv].prove_batch([hx(v, "alpha") for v in vectors] * 12, [hx(v, "sk") for v in vectors] * 12,
                                              [hx(v, "ad") for v in vectors] * 12)
        want = [b"".join(hx(v, f) for f in fields) for v in vectors] * 12
        assert [p.encode() for p in batch] == want


def test_device_maps_on_generator_blinding_base_identity(ctx):
    # curve 2 maps SW -> TE on the way in and TE -> SW on the way out: 1 * P gives P back for G, the blinding base and the identity,
    # and k * G on curve 2 is the SW preimage of k * G_te on curve 0
    import dot_ring_amd as d

    le = lambda k: k.to_bytes(32, "little")  # noqa: E731
    pts = [r.G, r.BLINDING, None] * 70                        # beyond the host-route sizes of curve 0
    out = ctx.bsn_scalar_mul_batch(b"".join(r.raw(p) for p in pts), le(1) * len(pts), CV2)
    assert out == b"".join(r.raw(p) for p in pts)
    ks = [random.Random(9).randrange(r.N) for _ in range(3)]
    g_te = tuple(d.Bandersnatch.curve.params.generator)
    assert r.to_te(r.G) == g_te
    te = ctx.bsn_scalar_mul_batch(b"".join(r.raw(g_te) for _ in ks) * 70, b"".join(le(k) for k in ks) * 70, 0)
    sw = ctx.bsn_scalar_mul_batch(r.raw(r.G) * 3 * 70, b"".join(le(k) for k in ks) * 70, CV2)
    for i, k in enumerate(ks):
        v, w = int.from_bytes(te[64 * i : 64 * i + 32], "little"), int.from_bytes(te[64 * i + 32 : 64 * i + 64], "little")
        assert sw[64 * i : 64 * i + 64] == r.raw(r.from_te((v, w))) == r.raw(r.mul(k, r.G))


def test_native_batch_calls_serve_curve2(ctx):
    # dr_ietf_prove_batch / dr_pedersen_prove_batch / dr_pedersen_verify_batch on curve 2: 81 / 98 / 196-byte proofs, SW aux records,
    # and the context's scratch is zero afterwards (secret scalars and nonces wiped)
    import dot_ring_amd as d

    cv = d.Bandersnatch_SW
    path = [p for p in FILES if p.endswith("ark-vrf" + os.sep + "bandersnatch_sw_sha-512_tai_pedersen.json")][0]
    vec = json.load(open(path))
    als, ads, sks = ([bytes.fromhex(v[k]) for v in vec] for k in ("alpha", "ad", "sk"))
    suite = d.PedersenVRF[cv]._suite_struct()
    raw, aux = ctx.pedersen_prove_batch(suite, als, ads, None, b"".join(sks))
    assert len(raw) == 196 * len(vec)
    for i, v in enumerate(vec):
        assert raw[196 * i : 196 * i + 196].hex() == "".join(v[k] for k in ("gamma", "proof_pk_com", "proof_r", "proof_ok", "proof_s", "proof_sb"))
        gamma = r.decode(bytes.fromhex(v["gamma"]))
        assert aux[288 * i : 288 * i + 64] == r.raw(gamma)
    assert ctx.scratch_residue() == 0
    assert ctx.pedersen_verify_batch(suite, raw, als, ads, None)
    bad = bytearray(raw)
    bad[196 + 4 * 33] ^= 1                                    # s of proof 1
    assert not ctx.pedersen_verify_batch(suite, bytes(bad), als, ads, None)
    for thin, plen in ((False, 81), (True, 98)):
        blob, _ = ctx.ietf_prove_batch(d.TinyVRF[cv]._suite_struct(), thin, als, ads, None, b"".join(sks))
        assert len(blob) == plen * len(vec)
        assert ctx.scratch_residue() == 0


def test_curve2_refused_outside_its_guards(ctx):
    le1 = (1).to_bytes(32, "little")
    with pytest.raises(ValueError):
        ctx.bsn_msm_groups(r.raw(r.G) * 65, le1 * 65, 65, CV2)
    with pytest.raises(ValueError):
        ctx.te_fixed_base_msm_groups(r.raw(r.G) * 5, le1 * 5, CV2)
