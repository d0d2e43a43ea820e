"""Baby JubJub on the GPU (DR_CURVE_BABYJUBJUB): the suite's 8 vector files byte for byte through the public API, the group calls,
decoding and try-and-increment of curve 5 against the big-integer restatement (babyjubjub_ref.py), the device field (fbn254.hip.h)
at the limb bounds of its contract with its square root, proving at batch size, batch verification, refusals, secret residue and
the other suites' bytes afterwards."""
import glob
import json
import os
import random
import struct
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import babyjubjub_ref as r  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILES = sorted(glob.glob(os.path.join(GOLDEN, "*", "baby*jubjub_sha*_tai_*.json")))
CV5 = 5
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

    cv = d.BabyJubJub
    assert len(FILES) == 8
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
    edge = [0, 1, r.N - 1, r.N, r.N + 1, 42 * r.N, 42 * r.N + 1, 2**256 - 1, 2**255, 2**251 - 1]
    ks = [edge[i % len(edge)] if i < 3 * len(edge) else rng.randrange(2**256) for i in range(len(pts))]
    raw = ctx.bsn_scalar_mul_batch(b"".join(map(r.raw, pts)), b"".join(k.to_bytes(32, "little") for k in ks), CV5)
    for i, (pt, k) in enumerate(zip(pts, ks)):
        assert raw[64 * i : 64 * i + 64] == r.raw(r.mul(k % r.N, pt)), (i, k)


def test_msm_groups_and_single_msm(ctx):
    rng = random.Random(5)
    base = _points(rng, 16)
    for m, groups in ((1, 70), (5, 13), (63, 3), (64, 3)):
        pts = [base[rng.randrange(16)] for _ in range(m * groups)]
        ks = [rng.randrange(2**256) for _ in pts]
        raw = ctx.bsn_msm_groups(b"".join(map(r.raw, pts)), b"".join(k.to_bytes(32, "little") for k in ks), m, CV5)
        for g in range(groups):
            assert raw[64 * g : 64 * g + 64] == r.raw(r.msm(pts[g * m : g * m + m], ks[g * m : g * m + m])), (m, g)
    with pytest.raises(Exception):
        ctx.bsn_msm_groups(b"".join(map(r.raw, base * 5))[: 65 * 64], bytes(65 * 32), 65, CV5)     # groups of at most 64 terms
    for n in (1, 7, 63, 64, 65, 300):
        base = _points(rng, 8)
        pts = [base[i % 8] for i in range(n)]
        ks = [rng.randrange(r.N) for _ in range(n)]
        want = r.O
        for j in range(8):
            want = r.add(want, r.mul(sum(ks[i] for i in range(j, n, 8)) % r.N, base[j]))
        got = ctx.bsn_msm(b"".join(map(r.raw, pts)), b"".join(k.to_bytes(32, "little") for k in ks), CV5)
        assert got == r.raw(want), n
    fixed = ctx.te_fixed_base_msm_groups(r.raw(r.G) + r.raw(r.BLINDING), b"".join(k.to_bytes(32, "little") for k in ks[:20]), CV5)
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
            ctx.bsn_msm_groups(b"".join(map(r.raw, pts)), sc(ks), 65, CV5)
        assert ctx.bsn_msm(b"".join(map(r.raw, pts)), sc(ks), CV5) == r.raw(r.msm(pts, ks))
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
    raw = ctx.bsn_msm_groups(b"".join(map(r.raw, pts)), sc(ks), m, CV5)
    assert len(raw) == 64 * groups
    for g in range(groups):
        assert raw[64 * g : 64 * g + 64] == r.raw(r.msm(pts[g * m : g * m + m], ks[g * m : g * m + m])), g
    if m == 2:                                     # a group that cancels to the identity
        assert ctx.bsn_msm_groups(r.raw(base[0]) + r.raw(r.neg(base[0])), sc([7, 7]), 2, CV5) == r.raw(r.O)


def _decode_cases(rng):
    cases = []
    for _ in range(150):
        cases.append(r.encode(r.mul(rng.randrange(1, r.N), r.G)))                   # valid
        cases.append(rng.randrange(2**256).to_bytes(32, "little"))                   # mostly no root, some with torsion
    tp = r.torsion_points()
    for t in tp:
        cases.append(r.encode(t))
        cases.append(r.encode(r.add(r.mul(rng.randrange(1, r.N), r.G), t)))
    for k in list(range(8)) + [2**254 - r.P - 1, 2**254 - r.P, 2**255 - 1 - r.P]:
        cases.append((r.P + k).to_bytes(32, "little"))
        cases.append(((r.P + k) | (1 << 255)).to_bytes(32, "little"))
    for _ in range(20):                                                               # valid points with bit 254 set
        enc = bytearray(r.encode(r.mul(rng.randrange(1, r.N), r.G)))
        enc[31] |= 0x40
        cases.append(bytes(enc))
    for y in (1, r.P - 1):
        cases.append(y.to_bytes(32, "little"))
        cases.append((y | (1 << 255)).to_bytes(32, "little"))
    return cases


def test_decode_points_with_and_without_check(ctx):
    rng = random.Random(9)
    cases = _decode_cases(rng)
    for check in (True, False):
        out, ok = ctx.bjj_decode_points(b"".join(cases), check)
        for i, enc in enumerate(cases):
            want = r.decode(enc, check=check)
            assert ok[i] == (want is not None), (i, check)
            if want is not None:
                assert out[64 * i : 64 * i + 64] == r.raw(want)
    out, ok = ctx.bsn_decode_points(b"".join(cases), CV5)          # dr_te_decode_points: the checked decoder
    assert list(ok) == [int(r.decode(enc) is not None) for enc in cases]


def test_decode_is_first_call_of_two_fresh_contexts():
    """The square-root tables are built on the host once per process and copied to the device once per context, by the first call that
    needs them and not by context creation: two contexts one after the other, each one's first call of any kind a checked decode of
    three valid encodings and one that is not on the curve."""
    from dot_ring_amd import _native

    off_curve = next(y.to_bytes(32, "little") for y in range(2, 100) if r.decode(y.to_bytes(32, "little"), check=False) is None)
    cases = [r.encode(r.mul(k, r.G)) for k in (1, 2, r.N - 1)]
    cases.insert(2, off_curve)
    want = [r.decode(enc) for enc in cases]
    assert [w is not None for w in want] == [True, True, False, True]
    for _ in range(2):
        c = _native.Context(0)
        try:
            out, ok = c.bjj_decode_points(b"".join(cases), True)
        finally:
            c.close()
        assert list(ok) == [1, 1, 0, 1]
        for i, w in enumerate(want):
            if w is not None:
                assert out[64 * i : 64 * i + 64] == r.raw(w)


def test_encode_to_curve_1000(ctx):
    import dot_ring_amd as d

    msgs = [b"tai-%d" % i for i in range(1000)] + [i.to_bytes(4, "little") for i in (5, 6, 2901)]
    got = d.BabyJubJub.point_type.encode_to_curve_batch(msgs)
    counters = []
    for m, pt in zip(msgs, got):
        want, ctr = r.encode_to_curve(m)
        assert (pt.x, pt.y) == want, m
        counters.append(ctr)
    assert max(counters) >= 12 and counters[-3:] == [1, 0, 18]       # masked counters; 2901 reaches the third decode launch
    pt = d.BabyJubJub.point_type.encode_to_curve((2901).to_bytes(4, "little"))
    assert (pt.x, pt.y) == r.encode_to_curve((2901).to_bytes(4, "little"))[0]


def _pack(ls):
    return b"".join(struct.pack("<9i", *l) for l in ls)


def _value(l):
    return sum(x << (29 * i) for i, x in enumerate(l))


R = 1 << 261


def _image(e):
    """the canonical Montgomery limb image of the element e (limbs 0..7 below 2^29, limb 8 the rest)"""
    v = e * R % r.P
    return [(v >> (29 * i)) & M29 for i in range(8)] + [v >> 232]


def _elem(l):
    return _value(l) * pow(R, -1, r.P) % r.P


def _check_records(out, flags, A, B, full):
    p = r.P
    rec = lambda i, j: int.from_bytes(out[384 * i + 32 * j : 384 * i + 32 * j + 32], "little")  # noqa: E731
    for i, (la, lb) in enumerate(zip(A, B)):
        a, b = _elem(la), _elem(lb)
        assert rec(i, 0) == a * b % p, i
        assert rec(i, 1) == a * a % p, i
        assert rec(i, 5) == a and rec(i, 9) == a, i
        if not full:
            continue
        assert rec(i, 2) == (a + b) % p and rec(i, 3) == (a - b) % p and rec(i, 4) == -a % p, i
        assert rec(i, 6) == 2 * a * b % p, i
        assert rec(i, 7) == pow(a, p - 2, p), i
        assert rec(i, 10) == a * b % p and rec(i, 11) == a, i
        sq = r.sqrt(a)
        assert (flags[i] & 1) == (sq is not None), i
        assert rec(i, 8) in ((sq, -sq % p) if sq is not None else (0,)), i
        assert ((flags[i] >> 2) & 1) == (a > -a % p), i


def test_field_ops_at_contract_bounds(ctx):
    rng = random.Random(21)
    p = r.P
    A, B = [], []
    top = 1 << 29
    # every operation's bounds at once: limbs 0..7 up to 2^29 in magnitude (mul2's bound), limb 8 up to 2^24 (|a b + b a| < 2^514)
    for _ in range(96):
        A.append([rng.choice([top, -top, rng.randrange(-top, top)]) for _ in range(8)] + [rng.randrange(-(1 << 24), 1 << 24)])
        B.append([rng.choice([top, -top, rng.randrange(-top, top)]) for _ in range(8)] + [rng.randrange(-(1 << 24), 1 << 24)])
    for _ in range(32):
        s = rng.choice([1, -1])
        A.append([s * top] * 8 + [s << 24])
        B.append([s * top] * 8 + [s << 24])
    # canonical images of special elements, and raw values just around p and 2^256
    for e in [0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, r.NONRESIDUE, r.D, 4]:
        A.append(_image(e))
        B.append(_image(3))
    for v in [p, p + 1, 2 * p - 1, 2**256 - 1, 2**255]:
        A.append([(v >> (29 * i)) & M29 for i in range(8)] + [v >> 232])
        B.append(_image(7))
    out, flags = ctx.bjj_field_ops_selftest(_pack(A), _pack(B))
    _check_records(out, flags, A, B, True)
    # the widest operands mul and sqr accept: limbs at 2^29.65 (products 2^59.3), all of one sign the worst column
    w = int(2 ** 29.65)
    wide = [[rng.choice([w, -w]) if k % 2 else s * w for _ in range(8)] + [s << 24] for k in range(64) for s in [(-1) ** (k // 2)]]
    wide2 = [[rng.choice([w, -w]) if k % 3 else s * w for _ in range(8)] + [s << 24] for k in range(64) for s in [(-1) ** (k // 4)]]
    out, flags = ctx.bjj_field_ops_selftest(_pack(wide), _pack(wide2))
    _check_records(out, flags, wide, wide2, False)


def test_field_sqrt(ctx):
    p = r.P
    rng = random.Random(23)
    c = pow(r.NONRESIDUE, r.Q, p)
    elems = [0, 1, p - 1, 4, r.NONRESIDUE, r.D, 2 * r.NONRESIDUE % p]
    elems += [pow(c, 1 << k, p) for k in range(29)]                     # 2-Sylow elements of every order 2^28 .. 1
    elems += [pow(c, rng.randrange(1 << 28), p) for _ in range(64)]     # random members of the 2-Sylow subgroup
    elems += [rng.randrange(p) for _ in range(200)]
    elems += [rng.randrange(p) ** 2 % p for _ in range(100)]
    A, B = [_image(e) for e in elems], [_image(1)] * len(elems)
    out, flags = ctx.bjj_field_ops_selftest(_pack(A), _pack(B))
    seen_non = 0
    for i, e in enumerate(elems):
        root = int.from_bytes(out[384 * i + 256 : 384 * i + 288], "little")
        if r.is_square(e):
            assert flags[i] & 1 and root * root % p == e, (i, e)
        else:
            assert not flags[i] & 1 and root == 0, (i, e)
            seen_non += 1
    assert seen_non > 50


@pytest.mark.parametrize("scheme", ["tiny", "thin", "pedersen"])
def test_prove_batch_300(ctx, scheme):
    import dot_ring_amd as d

    cv = d.BabyJubJub
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
    sp = d.BabyJubJub.curve.params
    le = lambda v: int(v).to_bytes(32, "little")  # noqa: E731
    suite = _native.vrf_suite(sp.suite_id, False, le(sp.generator[0]) + le(sp.generator[1]),
                              le(sp.auxiliary_points.blinding_base[0]) + le(sp.auxiliary_points.blinding_base[1]), CV5)
    # the ring prover: curve 3 is refused after the SRS and the other arguments pass
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dot_ring_amd", "data",
                           "bls12-381-srs-2-11-uncompressed-zcash.bin"), "rb") as f:
        blob = f.read()
    srs = ctx.srs_load(blob[8 : 8 + 96 * 1537])
    out = ctypes.c_void_p()
    rc = lib.dr_ring_prover_create_te(ctx.handle, CV5, srs.handle, 9, 1, bytes(32), bytes(32), bytes(64 * 512), bytes(64), ctypes.byref(out))
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
    with pytest.raises(ValueError, match="primitive 2048-th root of unity"):
        d.RingProofParams(cv=d.BabyJubJub)



def test_no_secret_residue_after_prove(ctx):
    import dot_ring_amd as d
    from dot_ring_amd import runtime

    c = runtime.context()
    for vrf in (d.TinyVRF[d.BabyJubJub], d.ThinVRF[d.BabyJubJub], d.PedersenVRF[d.BabyJubJub]):
        vrf.prove_batch([b"r%d" % i for i in range(70)], [(1000 + i).to_bytes(32, "little") for i in range(70)], [b""] * 70)
        assert c.scratch_residue() == 0


def test_other_suites_after_babyjubjub_calls(ctx, golden_dir):
    import dot_ring_amd as d

    d.PedersenVRF[d.BabyJubJub].prove_batch([b"a"] * 80, [(7).to_bytes(32, "little")] * 80, [b""] * 80)
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
