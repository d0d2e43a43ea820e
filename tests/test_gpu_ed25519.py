"""Ed25519 on the GPU (DR_CURVE_ED25519): the suite's 8 vector files byte for byte through the public API, the group calls, decoding
and try-and-increment of curve 3 against the big-integer restatement (ed25519_ref.py), the device field at the limb bounds of its
contract, proving at batch size, batch verification, refusals, secret residue and the other suites' bytes afterwards."""
import glob
import json
import os
import random
import struct
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ed25519_ref as r  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILES = sorted(glob.glob(os.path.join(GOLDEN, "*", "ed25519_sha*_tai_*.json")))
CV3 = 3
M29 = (1 << 29) - 1


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

    cv = d.Ed25519
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
        assert h.point_to_string().hex() == v["h"]
        proof = vrf.prove(al, sk, ad)
        assert proof.encode() == want
        assert vrf.proof_to_hash(proof.output_point).hex() == v["beta"][:64]
        assert vrf.proof_to_hash(proof.output_point, mul_cofactor=True) == r.point_to_hash(r.decode(hx(v, "gamma")), True)
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
    kp_pk, kp_sk = cv.secret_from_seed(bytes(range(32)))
    assert cv.public_key_from_secret(kp_sk) == kp_pk and r.encode(r.mul(r.le(kp_sk) % r.N, r.G)) == kp_pk


def _points(rng, k):
    return [r.mul(rng.randrange(1, r.N), r.G) for _ in range(k)]


def test_scalar_mul_edge_scalars(ctx):
    rng = random.Random(3)
    pts = _points(rng, 70)
    edge = [0, 1, r.N - 1, r.N, 2**256 - 1, 2**255, 2**253 - 1]
    ks = [edge[i % len(edge)] if i < 3 * len(edge) else rng.randrange(2**256) for i in range(len(pts))]
    raw = ctx.bsn_scalar_mul_batch(b"".join(map(r.raw, pts)), b"".join(k.to_bytes(32, "little") for k in ks), CV3)
    for i, (pt, k) in enumerate(zip(pts, ks)):
        assert raw[64 * i : 64 * i + 64] == r.raw(r.mul(k % r.N, pt)), (i, k)


def test_msm_groups_and_single_msm(ctx):
    rng = random.Random(5)
    m, groups = 5, 13
    pts = _points(rng, m * groups)
    ks = [rng.randrange(2**256) for _ in pts]
    raw = ctx.bsn_msm_groups(b"".join(map(r.raw, pts)), b"".join(k.to_bytes(32, "little") for k in ks), m, CV3)
    for g in range(groups):
        assert raw[64 * g : 64 * g + 64] == r.raw(r.msm(pts[g * m : g * m + m], ks[g * m : g * m + m]))
    for n in (1, 7, 64, 65, 300):
        base = _points(rng, 8)
        pts = [base[i % 8] for i in range(n)]
        ks = [rng.randrange(r.N) for _ in range(n)]
        want = r.O
        for j in range(8):
            want = r.add(want, r.mul(sum(ks[i] for i in range(j, n, 8)) % r.N, base[j]))
        got = ctx.bsn_msm(b"".join(map(r.raw, pts)), b"".join(k.to_bytes(32, "little") for k in ks), CV3)
        assert got == r.raw(want), n
    fixed = ctx.te_fixed_base_msm_groups(r.raw(r.G) + r.raw(r.BLINDING), b"".join(k.to_bytes(32, "little") for k in ks[:20]), CV3)
    for g in range(10):
        assert fixed[64 * g : 64 * g + 64] == r.raw(r.add(r.mul(ks[2 * g], r.G), r.mul(ks[2 * g + 1], r.BLINDING)))


@pytest.mark.parametrize("m", [1, 2, 63, 64, 65])
def test_msm_groups(ctx, m):
    """the grouped MSM over the group sizes at which its fold changes shape (mpad = 1, 2, 64 with and without a dead lane), a number of
    groups that does not fill the last workgroup, and terms that coincide, cancel or are the identity inside a group"""
    rng = random.Random(50 + m)
    base = _points(rng, 16)
    sc = lambda ks: b"".join(k.to_bytes(32, "little") for k in ks)  # noqa: E731
    if m == 65:                                   # the grouped call takes at most 64 terms: the single MSM serves 65
        pts = [base[i % 16] for i in range(65)]
        ks = [rng.randrange(2**256) for _ in pts]
        with pytest.raises(ValueError, match="group size must be in 1..64"):
            ctx.bsn_msm_groups(b"".join(map(r.raw, pts)), sc(ks), 65, CV3)
        assert ctx.bsn_msm(b"".join(map(r.raw, pts)), sc(ks), CV3) == r.raw(r.msm(pts, ks))
        return
    groups = 3 if m >= 63 else 13
    pts, ks = [], []
    for g in range(groups):
        gp = [base[rng.randrange(16)] for _ in range(m)]
        gk = [rng.randrange(2**256) for _ in gp]
        if g == 0:
            gp[0] = r.O                            # an identity term (the whole group when m = 1)
        if m >= 2 and g == 1:
            gp[1], gk[1] = gp[0], gk[0]            # P + P inside one group
        if m >= 2 and g == 2:
            gp[m - 1], gk[m - 1] = r.neg(gp[0]), gk[0]     # k P + k (-P) inside one group, at the two ends of the fold
        pts += gp
        ks += gk
    raw = ctx.bsn_msm_groups(b"".join(map(r.raw, pts)), sc(ks), m, CV3)
    assert len(raw) == 64 * groups
    for g in range(groups):
        assert raw[64 * g : 64 * g + 64] == r.raw(r.msm(pts[g * m : g * m + m], ks[g * m : g * m + m])), g
    if m == 2:                                     # a group that cancels to the identity
        assert ctx.bsn_msm_groups(r.raw(base[0]) + r.raw(r.neg(base[0])), sc([7, 7]), 2, CV3) == r.raw(r.O)


def _decode_cases(rng):
    cases = []
    for _ in range(150):
        cases.append(r.encode(r.mul(rng.randrange(1, r.N), r.G)))                   # valid
        cases.append(rng.randrange(2**256).to_bytes(32, "little"))                   # mostly no root, some with torsion
    tp = r.torsion_points()
    for t in tp:
        cases.append(r.encode(t))
        cases.append(r.encode(r.add(r.mul(rng.randrange(1, r.N), r.G), t)))
    for k in range(19):
        cases.append((r.P + k).to_bytes(32, "little"))
        cases.append(((r.P + k) | (1 << 255)).to_bytes(32, "little"))
    for y in (1, r.P - 1):
        cases.append(y.to_bytes(32, "little"))
        cases.append((y | (1 << 255)).to_bytes(32, "little"))
    return cases


def test_decode_points_with_and_without_check(ctx):
    rng = random.Random(9)
    cases = _decode_cases(rng)
    for check in (True, False):
        out, ok = ctx.ed25519_decode_points(b"".join(cases), check)
        for i, enc in enumerate(cases):
            want = r.decode(enc, check=check)
            assert ok[i] == (want is not None), (i, check)
            if want is not None:
                assert out[64 * i : 64 * i + 64] == r.raw(want)
    out, ok = ctx.bsn_decode_points(b"".join(cases), CV3)          # dr_te_decode_points: the checked decoder
    assert list(ok) == [int(r.decode(enc) is not None) for enc in cases]


def test_encode_to_curve_1000(ctx):
    import dot_ring_amd as d

    msgs = [b"tai-%d" % i for i in range(1000)]
    got = d.Ed25519.point_type.encode_to_curve_batch(msgs)
    counters = []
    for m, pt in zip(msgs, got):
        want, ctr = r.encode_to_curve(m)
        assert (pt.x, pt.y) == want
        counters.append(ctr)
    assert max(counters) > 0


def _pack(ls):
    return b"".join(struct.pack("<9i", *l) for l in ls)


def _value(l):
    return sum(x << (29 * i) for i, x in enumerate(l))


def test_field_ops_at_contract_bounds(ctx):
    rng = random.Random(21)
    p = r.P
    A, B = [], []
    top29 = (1 << 29) + (1 << 17)
    # extreme images: all limbs at the bound (both signs), canonical values near p and 2^255, zero, one
    for _ in range(96):
        A.append([rng.choice([top29, -top29, rng.randrange(-top29, top29)]) for _ in range(8)] + [rng.randrange(-(1 << 23), 1 << 23)])
        B.append([rng.choice([top29, -top29, rng.randrange(-top29, top29)]) for _ in range(8)] + [rng.randrange(-(1 << 23), 1 << 23)])
    for v in [0, 1, p - 1, p, p + 1, p + 18, 2**255 - 1, 2, 4, (p - 1) // 2, (p + 1) // 2]:
        A.append([(v >> (29 * i)) & M29 for i in range(8)] + [v >> 232])
        B.append([(3 >> (29 * i)) & M29 for i in range(8)] + [0])
    out, flags = ctx.fe25519_ops_selftest(_pack(A), _pack(B))
    rec = lambda i, j: int.from_bytes(out[352 * i + 32 * j : 352 * i + 32 * j + 32], "little")  # noqa: E731
    for i, (la, lb) in enumerate(zip(A, B)):
        a, b = _value(la) % p, _value(lb) % p
        assert rec(i, 0) == a * b % p
        assert rec(i, 1) == a * a % p
        assert rec(i, 2) == (a + b) % p and rec(i, 3) == (a - b) % p and rec(i, 4) == -a % p
        assert rec(i, 5) == a and rec(i, 9) == a
        assert rec(i, 6) == 2 * a * b % p
        assert rec(i, 7) == (pow(a, p - 2, p))
        sq = r.sqrt(a)
        assert (flags[i] & 1) == (sq is not None)
        if sq is not None:
            assert rec(i, 8) in (sq, -sq % p)
        ratio = r.sqrt(a * pow(b, -1, p)) if b else None
        if b:
            assert ((flags[i] >> 1) & 1) == (ratio is not None)
            if ratio is not None:
                assert rec(i, 10) * rec(i, 10) * b % p == a
        assert ((flags[i] >> 2) & 1) == (a > -a % p)
    # the widest operands mul and sqr accept: limbs 0..7 at 2^29.95 in both operands (products 2^59.9), top limbs 2^26; all of one
    # sign is the worst column
    w95 = int(2 ** 29.95)
    wide = [[rng.choice([w95, -w95]) if k % 2 else s * w95 for _ in range(8)] + [s << 26] for k in range(64) for s in [(-1) ** (k // 2)]]
    wide2 = [[rng.choice([w95, -w95]) if k % 3 else s * w95 for _ in range(8)] + [s << 26] for k in range(64) for s in [(-1) ** (k // 4)]]
    out, _ = ctx.fe25519_ops_selftest(_pack(wide), _pack(wide2))
    for i, (la, lb) in enumerate(zip(wide, wide2)):
        a, b = _value(la) % p, _value(lb) % p
        assert rec(i, 0) == a * b % p
        assert rec(i, 1) == a * a % p
        assert rec(i, 5) == a


@pytest.mark.parametrize("scheme", ["tiny", "thin", "pedersen"])
def test_prove_batch_300(ctx, scheme):
    import dot_ring_amd as d

    cv = d.Ed25519
    vrf = {"tiny": d.TinyVRF, "thin": d.ThinVRF, "pedersen": d.PedersenVRF}[scheme][cv]
    rng = random.Random(13)
    B = 300
    sks = [rng.randrange(1, r.N).to_bytes(32, "little") for _ in range(B)]
    als = [b"alpha-%d" % i for i in range(B)]
    ads = [b"ad-%d" % (i % 5) for i in range(B)]
    proofs = vrf.prove_batch(als, sks, ads)
    for i in range(B):
        if scheme == "pedersen":
            want, _ = r.pedersen_prove(sks[i], als[i], ads[i])
        else:
            want = r.ietf_prove(sks[i], als[i], ads[i], thin=scheme == "thin")
        assert proofs[i].encode() == want, i
    if scheme == "thin":
        pks = [cv.public_key_from_secret(sk) for sk in sks]
        assert vrf.batch_verify(proofs, pks, als, ads)
        bad = vrf.decode(proofs[7].encode())
        bad.s = (bad.s + 1) % r.N
        assert not vrf.batch_verify(proofs[:7] + [bad] + proofs[8:], pks, als, ads)
    if scheme == "pedersen":
        assert vrf.batch_verify(proofs, als, ads)
        p = proofs[5]
        bad = type(p)(p.output_point, p.blinded_pk, p.result_point, p.ok, p.s, (p.sb + 1) % r.N)
        assert not vrf.batch_verify(proofs[:5] + [bad] + proofs[6:], als, ads)


def test_refusals(ctx):
    import ctypes

    import dot_ring_amd as d
    from dot_ring_amd import _native

    lib = _native.lib()
    sp = d.Ed25519.curve.params
    le = lambda v: int(v).to_bytes(32, "little")  # noqa: E731
    suite = _native.vrf_suite(sp.suite_id, False, le(sp.generator[0]) + le(sp.generator[1]),
                              le(sp.auxiliary_points.blinding_base[0]) + le(sp.auxiliary_points.blinding_base[1]), CV3)
    # the ring prover: curve 3 is refused after the SRS and the other arguments pass
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dot_ring_amd", "data",
                           "bls12-381-srs-2-11-uncompressed-zcash.bin"), "rb") as f:
        blob = f.read()
    srs = ctx.srs_load(blob[8 : 8 + 96 * 1537])
    out = ctypes.c_void_p()
    rc = lib.dr_ring_prover_create_te(ctx.handle, CV3, srs.handle, 9, 1, bytes(32), bytes(32), bytes(64 * 512), bytes(64), ctypes.byref(out))
    assert rc == _native.DR_ERR_INVALID and not out.value
    srs.close()
    # dr_ietf_verify_batch and the Ring-VRF verifier refuse the suite
    verdict = ctypes.create_string_buffer(1)
    off = (ctypes.c_uint64 * 2)(0, 0)
    rc = lib.dr_ietf_verify_batch(ctx.handle, ctypes.byref(suite), 0, 1, bytes(80), bytes(32), b"", off, b"", off, None, None, verdict)
    assert rc == _native.DR_ERR_INVALID
    vk = _native.RingVerifierKeyStruct()
    vk.log2n, vk.fs_prefix, vk.fs_prefix_len = 9, b"x", 1
    ok = ctypes.c_int(0)
    rc = lib.dr_ringvrf_verify_batch(ctx.handle, ctypes.byref(suite), ctypes.byref(vk), 1, bytes(784), b"", off, b"", off, None, None,
                                     bytes(32), ctypes.byref(ok))
    assert rc == _native.DR_ERR_INVALID and ok.value == 0
    with pytest.raises(ValueError):
        d.RingProofParams(cv=d.Ed25519)


def test_no_secret_residue_after_prove(ctx):
    import dot_ring_amd as d
    from dot_ring_amd import runtime

    c = runtime.context()
    for vrf in (d.TinyVRF[d.Ed25519], d.ThinVRF[d.Ed25519], d.PedersenVRF[d.Ed25519]):
        vrf.prove_batch([b"r%d" % i for i in range(70)], [(1000 + i).to_bytes(32, "little") for i in range(70)], [b""] * 70)
        assert c.scratch_residue() == 0


def test_other_suites_after_ed25519_calls(ctx, golden_dir):
    import dot_ring_amd as d

    d.PedersenVRF[d.Ed25519].prove_batch([b"a"] * 80, [(7).to_bytes(32, "little")] * 80, [b""] * 80)
    fields = ("gamma", "proof_pk_com", "proof_r", "proof_ok", "proof_s", "proof_sb")
    for rel, cv in (("ark-vrf/bandersnatch_sha-512_ell2_pedersen.json", d.Bandersnatch),
                    ("ark-vrf/jubjub_sha-512_tai_pedersen.json", d.JubJub),
                    ("ark-vrf/bandersnatch_sw_sha-512_tai_pedersen.json", d.Bandersnatch_SW)):
        vectors = json.load(open(os.path.join(golden_dir, rel)))
        hx = lambda v, k: bytes.fromhex(v[k])  # noqa: E731
        batch = d.PedersenVRF[cv].prove_batch([hx(v, "alpha") for v in vectors] * 12, [hx(v, "sk") for v in vectors] * 12,
                                              [hx(v, "ad") for v in vectors] * 12)
        assert [p.encode() for p in batch] == [b"".join(hx(v, f) for f in fields) for v in vectors] * 12
