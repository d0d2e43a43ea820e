"""P-256 on the GPU (DR_CURVE_P256): the suite's 9 vector files byte for byte through the public API, the group calls, decoding
(with the SEC1 fallback) and try-and-increment of curve 4 against the big-integer restatement (p256_ref.py), the device field at the
limb bounds of its contract, proving at batch size, batch verification, refusals, secret residue and the other suites' bytes
afterwards."""
import glob
import json
import os
import random
import struct
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import p256_ref as r  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILES = sorted(glob.glob(os.path.join(GOLDEN, "*", "secp256r1_sha*_tai_*.json")))
CV4 = 4
M29 = (1 << 29) - 1
FALLBACK_ALPHAS = [240, 967, 1184, 987]


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

    cv = d.P256
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
        assert vrf.proof_to_hash(proof.output_point, mul_cofactor=True).hex() == v["beta"][:64]      # cofactor 1
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


def _sc(ks):
    return b"".join(k.to_bytes(32, "little") for k in ks)


def test_scalar_mul_edge_scalars(ctx):
    rng = random.Random(3)
    pts = _points(rng, 70)
    edge = [0, 1, r.N - 1, r.N, 2**256 - 1, 2**255, (r.N - 1) // 2, r.N + 1]
    ks = [edge[i % len(edge)] if i < 3 * len(edge) else rng.randrange(2**256) for i in range(len(pts))]
    raw = ctx.bsn_scalar_mul_batch(b"".join(map(r.raw, pts)), _sc(ks), CV4)
    for i, (pt, k) in enumerate(zip(pts, ks)):
        assert raw[64 * i : 64 * i + 64] == r.raw(r.mul(k % r.N, pt)), (i, k)
    # the identity in, the identity out
    assert ctx.bsn_scalar_mul_batch(bytes(64), _sc([12345]), CV4) == bytes(64)


@pytest.mark.parametrize("m", [1, 2, 63, 64, 65])
def test_msm_groups(ctx, m):
    rng = random.Random(5 + m)
    groups = 5 if m <= 64 else 0
    if m == 65:                                   # the grouped call takes at most 64 terms: the single MSM serves 65
        pts = _points(rng, 65)
        ks = [rng.randrange(2**256) for _ in pts]
        assert ctx.bsn_msm(b"".join(map(r.raw, pts)), _sc(ks), CV4) == r.raw(r.msm(pts, ks))
        return
    pts, ks = [], []
    for g in range(groups):
        gp = _points(rng, m)
        gk = [rng.randrange(2**256) for _ in gp]
        if m >= 2 and g == 1:
            gp[1] = gp[0]                          # P + P inside one group
            gk[1] = gk[0]
        if m >= 2 and g == 2:
            gp[1] = r.neg(gp[0])                   # P + (-P) inside one group
            gk[1] = gk[0]
        if g == 3:
            gp[0] = None                           # an identity term
        pts += gp
        ks += gk
    raw = ctx.bsn_msm_groups(b"".join(map(r.raw, pts)), _sc(ks), m, CV4)
    for g in range(groups):
        assert raw[64 * g : 64 * g + 64] == r.raw(r.msm(pts[g * m : g * m + m], ks[g * m : g * m + m])), g
    if m >= 2:                                     # a group that cancels to the identity: 64 zero bytes
        q = _points(rng, 1)[0]
        assert ctx.bsn_msm_groups(r.raw(q) + r.raw(r.neg(q)), _sc([7, 7]), 2, CV4) == bytes(64)


@pytest.mark.parametrize("n", [1, 64, 65, 4097])
def test_single_msm(ctx, n):
    rng = random.Random(11 + n)
    base = _points(rng, 8)
    pts = [base[i % 8] for i in range(n)]
    ks = [rng.randrange(r.N) for _ in range(n)]
    want = r.O
    for j in range(8):
        want = r.add(want, r.mul(sum(ks[i] for i in range(j, n, 8)) % r.N, base[j]))
    assert ctx.bsn_msm(b"".join(map(r.raw, pts)), _sc(ks), CV4) == r.raw(want)


def test_fixed_base_groups(ctx):
    rng = random.Random(17)
    ks = [rng.randrange(r.N) for _ in range(20)]
    fixed = ctx.te_fixed_base_msm_groups(r.raw(r.G) + r.raw(r.BLINDING), _sc(ks), CV4)
    for g in range(10):
        assert fixed[64 * g : 64 * g + 64] == r.raw(r.add(r.mul(ks[2 * g], r.G), r.mul(ks[2 * g + 1], r.BLINDING)))


def _decode_cases(rng):
    cases = []
    for p in _points(rng, 120):
        cases.append(r.encode(p))                                                       # valid
    for _ in range(200):
        cases.append(rng.randrange(2**264).to_bytes(33, "little"))                      # mostly bad flags
    for _ in range(200):
        cases.append(rng.randrange(2**256).to_bytes(32, "little") + rng.choice([b"\x00", b"\x80"]))   # x >= p, no root, valid
    for p in _points(rng, 60):                                                          # SEC1 strings: many decode by the fallback
        cases.append(bytes([2 + (p[1] & 1)]) + p[0].to_bytes(32, "big"))
    cases += [bytes(32) + b"\x40", bytes(32) + b"\xc0", b"\x01" + bytes(31) + b"\x40", b"\x02" + bytes(31) + b"\x40", b"\x02" + b"\xff" * 32]
    for bit in range(6):
        cases.append(r.encode(r.G)[:32] + bytes([1 << bit]))
    for k in (0, 1, 2**200, 2**256 - r.P - 1):
        cases.append((r.P + k).to_bytes(32, "little") + b"\x80")
    for x in range(4, 60):
        if r.sqrt(r.rhs(x)) is None:
            cases.append(x.to_bytes(32, "little") + b"\x00")
    return cases


def test_decode_points_in_each_mode(ctx):
    rng = random.Random(9)
    cases = _decode_cases(rng)
    assert sum(r.decoded_by_fallback(c) for c in cases) > 20
    blob = b"".join(cases)
    for check in (True, False):
        out, ok = ctx.p256_decode_points(blob, check)
        for i, enc in enumerate(cases):
            want = r.decode(enc, check=check)
            assert ok[i] == (want != "bad"), (i, check, enc.hex())
            if want != "bad":
                assert out[64 * i : 64 * i + 64] == r.raw(want), (i, check)
    out, ok = ctx.bsn_decode_points(blob, CV4)             # dr_te_decode_points: the checked decoder
    assert list(ok) == [int(r.decode(enc) != "bad") for enc in cases]
    for i, enc in enumerate(cases):
        if ok[i]:
            assert out[64 * i : 64 * i + 64] == r.raw(r.decode(enc))


def test_encode_to_curve_1000_and_fallback_alphas(ctx):
    import dot_ring_amd as d

    msgs = [b"tai-%d" % i for i in range(1000)] + [i.to_bytes(4, "little") for i in FALLBACK_ALPHAS]
    got = d.P256.point_type.encode_to_curve_batch(msgs)
    counters, fallbacks = [], 0
    for m, pt in zip(msgs, got):
        want, ctr, by_fallback = r.encode_to_curve(m)
        assert (pt.x, pt.y) == want, m
        counters.append(ctr)
        fallbacks += by_fallback
    assert max(counters) > 0 and fallbacks >= len(FALLBACK_ALPHAS)
    for i in FALLBACK_ALPHAS:                              # one at a time as well (the single-input path)
        pt = d.P256.point_type.encode_to_curve(i.to_bytes(4, "little"))
        assert (pt.x, pt.y) == r.encode_to_curve(i.to_bytes(4, "little"))[0]


def _pack(ls):
    return b"".join(struct.pack("<9i", *l) for l in ls)


def _value(l):
    return sum(x << (29 * i) for i, x in enumerate(l))


def test_field_ops_at_contract_bounds(ctx):
    rng = random.Random(21)
    p, rinv = r.P, pow(2**261, -1, r.P)
    A, B = [], []
    top = (1 << 29) + (1 << 27)                            # the limb bound of a reduced element
    for _ in range(128):
        A.append([rng.choice([top, -top, rng.randrange(-top, top)]) for _ in range(8)] + [rng.randrange(-(1 << 26), 1 << 26)])
        B.append([rng.choice([top, -top, rng.randrange(-top, top)]) for _ in range(8)] + [rng.randrange(-(1 << 26), 1 << 26)])
    for v in [0, 1, p - 1, p, p + 1, 2**256 - 1, 2, 4, (p - 1) // 2, (p + 1) // 2, 2**261 % p, 2**256 % p]:
        A.append([(v >> (29 * i)) & M29 for i in range(8)] + [v >> 232])
        B.append([3, 0, 0, 0, 0, 0, 0, 0, 0])
    out, flags = ctx.p256_field_ops_selftest(_pack(A), _pack(B))
    rec = lambda i, j: int.from_bytes(out[384 * i + 32 * j : 384 * i + 32 * j + 32], "little")  # noqa: E731
    for i, (la, lb) in enumerate(zip(A, B)):
        a, b = _value(la) * rinv % p, _value(lb) * rinv % p
        assert rec(i, 0) == a * b % p
        assert rec(i, 1) == a * a % p
        assert rec(i, 2) == (a + b) % p and rec(i, 3) == (a - b) % p and rec(i, 4) == -a % p
        assert rec(i, 5) == a and rec(i, 9) == a and rec(i, 10) == a and rec(i, 11) == a * a % p
        assert rec(i, 6) == 2 * a * b % p
        assert rec(i, 7) == pow(a, p - 2, p)
        sq = r.sqrt(a)
        assert (flags[i] & 1) == (sq is not None)
        if sq is not None:
            assert rec(i, 8) in (sq, -sq % p)
        assert ((flags[i] >> 1) & 1) == (a > -a % p) and ((flags[i] >> 2) & 1) == (a & 1)
    # reduce at its own bounds (limbs up to 2^31 - 8 in magnitude, tops of both signs, so h = top >> 24 spans [-128, 127]) and the
    # square of its result — sqr(reduce(a)) is the fused case a gfx950 compiler got wrong (fp256.hip.h).  Only records 10 and 11
    # are within their contracts for these rows.
    edge = (1 << 31) - 8
    red = []
    for k in range(160):
        top = [edge, -edge, (1 << 30), -(1 << 30), (1 << 24) + k, -(1 << 24) - k, rng.randrange(-edge, edge)][k % 7]
        lim = [rng.choice([edge, -edge, rng.randrange(-edge, edge)]) for _ in range(8)] if k % 2 else [rng.randrange(1 << 29) for _ in range(8)]
        if abs(_value(lim + [top])) < 2**262:
            red.append(lim + [top])
    out, _ = ctx.p256_field_ops_selftest(_pack(red), _pack(red))
    for i, la in enumerate(red):
        a = _value(la) * rinv % p
        assert rec(i, 10) == a and rec(i, 11) == a * a % p, la
    # the widest operands mul and sqr accept: limbs 0..7 at 2^29.9 in both (products 2^59.8), top limbs 2^26, all of one sign
    w = int(2**29.9)
    wide = [[s * w] * 8 + [s << 26] for s in (1, -1) for _ in range(4)] + [[rng.choice([w, -w]) for _ in range(8)] + [1 << 26] for _ in range(56)]
    wide2 = [[s * w] * 8 + [s << 26] for s in (1, -1, -1, 1) for _ in range(2)] + [[rng.choice([w, -w]) for _ in range(8)] + [-(1 << 26)] for _ in range(56)]
    out, _ = ctx.p256_field_ops_selftest(_pack(wide), _pack(wide2))
    for i, (la, lb) in enumerate(zip(wide, wide2)):
        a, b = _value(la) * rinv % p, _value(lb) * rinv % p
        assert rec(i, 0) == a * b % p and rec(i, 11) == a * a % p
        assert rec(i, 1) == a * a % p
        assert rec(i, 5) == a


@pytest.mark.parametrize("scheme", ["tiny", "thin", "pedersen"])
def test_prove_batch_300(ctx, scheme):
    import dot_ring_amd as d

    cv = d.P256
    vrf = {"tiny": d.TinyVRF, "thin": d.ThinVRF, "pedersen": d.PedersenVRF}[scheme][cv]
    rng = random.Random(13)
    B = 300
    sks = [rng.randrange(1, r.N).to_bytes(32, "little") for _ in range(B)]
    als = [b"alpha-%d" % i for i in range(B - 4)] + [i.to_bytes(4, "little") for i in FALLBACK_ALPHAS]
    ads = [b"ad-%d" % (i % 5) for i in range(B)]
    proofs = vrf.prove_batch(als, sks, ads)
    for i in range(B):
        if scheme == "pedersen":
            want, _ = r.pedersen_prove(sks[i], als[i], ads[i])
        else:
            want = r.ietf_prove(sks[i], als[i], ads[i], thin=scheme == "thin")
        assert proofs[i].encode() == want, i
    for i in (0, 17, B - 1):
        assert vrf.prove(als[i], sks[i], ads[i]).encode() == proofs[i].encode()
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
    sp = d.P256.curve.params
    le = lambda v: int(v).to_bytes(32, "little")  # noqa: E731
    suite = _native.vrf_suite(sp.suite_id, sp.hash_fn, le(sp.generator[0]) + le(sp.generator[1]),
                              le(sp.auxiliary_points.blinding_base[0]) + le(sp.auxiliary_points.blinding_base[1]), CV4)
    assert suite.xof == 2
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dot_ring_amd", "data",
                           "bls12-381-srs-2-11-uncompressed-zcash.bin"), "rb") as f:
        blob = f.read()
    srs = ctx.srs_load(blob[8 : 8 + 96 * 1537])
    out = ctypes.c_void_p()
    rc = lib.dr_ring_prover_create_te(ctx.handle, CV4, srs.handle, 9, 1, bytes(32), bytes(32), bytes(64 * 512), bytes(64), ctypes.byref(out))
    assert rc == _native.DR_ERR_INVALID and not out.value
    srs.close()
    verdict = ctypes.create_string_buffer(1)
    off = (ctypes.c_uint64 * 2)(0, 0)
    rc = lib.dr_ietf_verify_batch(ctx.handle, ctypes.byref(suite), 0, 1, bytes(81), bytes(33), b"", off, b"", off, None, None, verdict)
    assert rc == _native.DR_ERR_INVALID
    vk = _native.RingVerifierKeyStruct()
    vk.log2n, vk.fs_prefix, vk.fs_prefix_len = 9, b"x", 1
    ok = ctypes.c_int(0)
    rc = lib.dr_ringvrf_verify_batch(ctx.handle, ctypes.byref(suite), ctypes.byref(vk), 1, bytes(784), b"", off, b"", off, None, None,
                                     bytes(32), ctypes.byref(ok))
    assert rc == _native.DR_ERR_INVALID and ok.value == 0
    u = ctypes.create_string_buffer(64)
    assert lib.dr_hash_to_field_batch(ctypes.byref(suite), b"", off, 1, u) == _native.DR_ERR_INVALID
    # a transcript hash the library does not know is refused, not read as SHAKE128
    bad = _native.vrf_suite(sp.suite_id, 2, bytes(suite.generator_xy), bytes(suite.blinding_base_xy), CV4)
    bad.xof = 3
    out_xy = ctypes.create_string_buffer(64)
    rc = lib.dr_encode_to_curve_batch(ctx.handle, ctypes.byref(bad), b"a", (ctypes.c_uint64 * 2)(0, 1), None, None, 1, out_xy)
    assert rc == _native.DR_ERR_INVALID
    with pytest.raises(ValueError):
        d.RingProofParams(cv=d.P256)


def test_no_secret_residue_after_prove(ctx):
    import dot_ring_amd as d
    from dot_ring_amd import runtime

    c = runtime.context()
    for vrf in (d.TinyVRF[d.P256], d.ThinVRF[d.P256], d.PedersenVRF[d.P256]):
        vrf.prove_batch([b"r%d" % i for i in range(70)], [(1000 + i).to_bytes(32, "little") for i in range(70)], [b""] * 70)
        assert c.scratch_residue() == 0


def test_other_suites_after_p256_calls(ctx, golden_dir):
    import dot_ring_amd as d

    d.PedersenVRF[d.P256].prove_batch([b"a"] * 80, [(7).to_bytes(32, "little")] * 80, [b""] * 80)
    fields = ("gamma", "proof_pk_com", "proof_r", "proof_ok", "proof_s", "proof_sb")
    for rel, cv in (("ark-vrf/bandersnatch_sha-512_ell2_pedersen.json", d.Bandersnatch),
                    ("ark-vrf/jubjub_sha-512_tai_pedersen.json", d.JubJub),
                    ("ark-vrf/bandersnatch_sw_sha-512_tai_pedersen.json", d.Bandersnatch_SW),
                    ("ark-vrf/ed25519_sha-512_tai_pedersen.json", d.Ed25519)):
        vectors = json.load(open(os.path.join(golden_dir, rel)))
        hx = lambda v, k: bytes.fromhex(v[k])  # noqa: E731
        batch = d.PedersenVRF[cv].prove_batch([hx(v, "alpha") for v in vectors] * 12, [hx(v, "sk") for v in vectors] * 12,
                                              [hx(v, "ad") for v in vectors] * 12)
        assert [p.encode() for p in batch] == [b"".join(hx(v, f) for f in fields) for v in vectors] * 12
