"""Big-integer restatement of the reference's BLS12_381_G2_RO / BLS12_381_G2_NU (specs/bls12_381_G2.py), written from RFC 9380
(section 5: hash_to_field by expand_message_xmd over SHA-256 with m = 2 and L = 64; 6.6.2: simplified SWU; 6.6.3 and appendix E.3: the
3-isogeny from E': y^2 = x^3 + 240 i x + 1012 (1 + i) to E: y^2 = x^3 + 4 (1 + i); 8.8.2: Z = -(2 + i) and h_eff; appendix G.3: the
cofactor clearing by the endomorphism psi) and the reference's behaviour:

  the sum of two images (RO) or one image (NU) on E, then times h_eff (the reference's 636-bit `cofactor`);
  Fp2.sgn0: the parity of the real part, or of the imaginary part where the real part is zero;
  no point codec (point_to_string / string_to_point raise).

Fp2 elements are (re, im) tuples with i^2 = -1, points are (x, y) tuples of E(Fp2), the identity is None.  E(Fp2) has order H2 * R_ORDER;
a point of it need not lie in G2."""
import hashlib

P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
R_ORDER = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
# the cofactor: #E(Fp2) = H2 * R_ORDER
H2 = 0x5D543A95414E7F1091D50792876A202CD91DE4547085ABAA68A205B2E5A7DDFA628F1CB4D9E82EF21537E293A6691AE1616EC6E786F0C70CF1C38E31C7238E5
# RFC 9380 8.8.2: what hashing multiplies by (the reference's `cofactor`), 636 bits, a multiple of H2
H_EFF = 0xBC69F08F2EE75B3584C6A0EA91B352888E2A8E9145AD7689986FF031508FFE1329C2F178731DB956D82BF015D1212B02EC0EC69D7477C1AE954CBC06689F6A359894C0ADEBBF6B4E8020005AAA95551
BLS_Z_ABS = 0xD201000000010000                   # the curve parameter z = -BLS_Z_ABS (appendix G.3's c1)
CURVE_B = (4, 4)
G = (
    (0x024AA2B2F08F0A91260805272DC51051C6E47AD4FA403B02B4510B647AE3D1770BAC0326A805BBEFD48056C8C121BDB8,
     0x13E02B6052719F607DACD3A088274F65596BD0D09920B61AB5DA61BBDC7F5049334CF11213945D57E5AC7D055D042B7E),
    (0x0CE5D527727D6E118CC9CDC6DA2E351AADFD9BAA8CBDD3A76D429A695160D12C923AC9CC3BACA289E193548608B82801,
     0x0606C4A02EA734CC32ACD2B02BC28B99CB3E287E85A763AF267492AB572E99AB3F370D275CEC1DA1AAA9075FF05F79BE),
)
DST_RO = b"QUUX-V01-CS02-with-BLS12381G2_XMD:SHA-256_SSWU_RO_"
DST_NU = b"QUUX-V01-CS02-with-BLS12381G2_XMD:SHA-256_SSWU_NU_"
SSWU_Z = (P - 2, P - 1)
ISO_A = (0, 240)
ISO_B = (1012, 1012)
# the isogeny's coefficient lists, lowest degree first as RFC 9380 appendix E.3 numbers them (k_(i,0), k_(i,1), ...); the two
# denominators are monic and their leading 1 is not listed
_K1 = 0x5C759507E8E333EBB5B7A9A47D7ED8532C52D39FD3A042A88B58423C50AE15D5C2638E343D9C71C6238AAAAAAAA97D6
ISO_XNUM = (
    (_K1, _K1),
    (0, 0x11560BF17BAA99BC32126FCED787C88F984F87ADF7AE0C7F9A208C6B4F20A4181472AAA9CB8D555526A9FFFFFFFFC71A),
    (0x11560BF17BAA99BC32126FCED787C88F984F87ADF7AE0C7F9A208C6B4F20A4181472AAA9CB8D555526A9FFFFFFFFC71E,
     0x8AB05F8BDD54CDE190937E76BC3E447CC27C3D6FBD7063FCD104635A790520C0A395554E5C6AAAA9354FFFFFFFFE38D),
    (0x171D6541FA38CCFAED6DEA691F5FB614CB14B4E7F4E810AA22D6108F142B85757098E38D0F671C7188E2AAAAAAAA5ED1, 0),
)
ISO_XDEN = (
    (0, P - 72),
    (12, P - 12),
)
_K3 = 0x1530477C7AB4113B59A4C18B076D11930F7DA5D4A07F649BF54439D87D27E500FC8C25EBF8C92F6812CFC71C71C6D706
ISO_YNUM = (
    (_K3, _K3),
    (0, 0x5C759507E8E333EBB5B7A9A47D7ED8532C52D39FD3A042A88B58423C50AE15D5C2638E343D9C71C6238AAAAAAAA97BE),
    (0x11560BF17BAA99BC32126FCED787C88F984F87ADF7AE0C7F9A208C6B4F20A4181472AAA9CB8D555526A9FFFFFFFFC71C,
     0x8AB05F8BDD54CDE190937E76BC3E447CC27C3D6FBD7063FCD104635A790520C0A395554E5C6AAAA9354FFFFFFFFE38F),
    (0x124C9AD43B6CF79BFBF7043DE3811AD0761B0F37A1E26286B0E977C69AA274524E79097A56DC4BD9E1B371C71C718B10, 0),
)
ISO_YDEN = (
    (P - 432, P - 432),
    (0, P - 216),
    (18, P - 18),
)
assert (len(ISO_XNUM), len(ISO_XDEN), len(ISO_YNUM), len(ISO_YDEN)) == (4, 2, 4, 3)


# ---------------------------------------------------------------- Fp2 = Fp[i] / (i^2 + 1)
ZERO, ONE = (0, 0), (1, 0)


def f2(re, im=0):
    return re % P, im % P


def f2_add(a, b):
    return (a[0] + b[0]) % P, (a[1] + b[1]) % P


def f2_sub(a, b):
    return (a[0] - b[0]) % P, (a[1] - b[1]) % P


def f2_neg(a):
    return -a[0] % P, -a[1] % P


def f2_mul(a, b):
    return (a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P


def f2_sqr(a):
    return f2_mul(a, a)


def f2_conj(a):
    return a[0], -a[1] % P


def f2_norm(a):
    return (a[0] * a[0] + a[1] * a[1]) % P


def f2_inv(a):
    """a^-1; ValueError for 0 (the reference's modular inverse raises there)"""
    n = f2_norm(a)
    if n == 0:
        raise ValueError("base is not invertible for the given modulus")
    ni = pow(n, -1, P)
    return a[0] * ni % P, -a[1] * ni % P


def f2_pow(a, e):
    acc = ONE
    for bit in bin(e)[2:]:
        acc = f2_sqr(acc)
        if bit == "1":
            acc = f2_mul(acc, a)
    return acc


def f2_is_square(a):
    """Euler's criterion through the norm: a^((p^2 - 1) / 2) = norm(a)^((p - 1) / 2); 0 counts as a square"""
    return pow(f2_norm(a), (P - 1) // 2, P) != P - 1


def f2_sgn0(a):
    """RFC 9380 4.1 for m = 2 (the reference's Fp2.sgn0)"""
    return (a[0] & 1) | ((a[0] == 0) & (a[1] & 1))


def _fp_sqrt(v):
    r = pow(v, (P + 1) // 4, P)
    return r if r * r % P == v % P else None


def _norm_route_sqrt(a):
    """a root of a by the norm route, for the two constants below only (both have a non-zero imaginary part)"""
    s = _fp_sqrt(f2_norm(a))
    for sign in (1, -1):
        x0 = _fp_sqrt((a[0] + sign * s) * pow(2, -1, P) % P)
        if x0:
            root = x0, a[1] * pow(2 * x0, -1, P) % P
            assert f2_sqr(root) == a
            return root
    raise AssertionError("no root")


_SQRT_I, _SQRT_NEG_I = _norm_route_sqrt((0, 1)), _norm_route_sqrt((0, P - 1))


def f2_sqrt(a):
    """a root of a, None if a is no square: RFC 9380 appendix I.3 for q = p^2 = 9 mod 16, one exponentiation in Fp2 by (q + 7) / 16 and
    the four candidates (it shares nothing with the device's route through the norm and two roots in Fp)"""
    a = f2(*a)
    tv1 = f2_pow(a, (P * P + 7) // 16)
    for k in (ONE, (0, 1), _SQRT_I, _SQRT_NEG_I):
        cand = f2_mul(tv1, k)
        if f2_sqr(cand) == a:
            return cand
    return None


# ---------------------------------------------------------------- hash to field (RFC 9380 section 5), m = 2
def expand_message_xmd(msg, dst, length):
    dst_prime = dst + bytes([len(dst)])
    b0 = hashlib.sha256(bytes(64) + msg + length.to_bytes(2, "big") + b"\x00" + dst_prime).digest()
    blocks = [hashlib.sha256(b0 + b"\x01" + dst_prime).digest()]
    for i in range(2, -(-length // 32) + 1):
        blocks.append(hashlib.sha256(bytes(x ^ y for x, y in zip(b0, blocks[-1])) + bytes([i]) + dst_prime).digest())
    return b"".join(blocks)[:length]


def hash_to_field(msg, count, dst):
    raw = expand_message_xmd(msg, dst, 128 * count)
    e = [int.from_bytes(raw[64 * i : 64 * i + 64], "big") % P for i in range(2 * count)]
    return [(e[2 * i], e[2 * i + 1]) for i in range(count)]


# ---------------------------------------------------------------- the group E(Fp2): y^2 = x^3 + 4 (1 + i)
def on_curve(pt):
    return pt is None or f2_sqr(pt[1]) == f2_add(f2_mul(f2_sqr(pt[0]), pt[0]), CURVE_B)


def neg(pt):
    return None if pt is None else (pt[0], f2_neg(pt[1]))


def add(p1, p2):
    if p1 is None:
        return p2
    if p2 is None:
        return p1
    if p1[0] == p2[0]:
        if f2_add(p1[1], p2[1]) == ZERO:
            return None
        lam = f2_mul(f2_mul((3, 0), f2_sqr(p1[0])), f2_inv(f2_add(p1[1], p1[1])))
    else:
        lam = f2_mul(f2_sub(p2[1], p1[1]), f2_inv(f2_sub(p2[0], p1[0])))
    x = f2_sub(f2_sub(f2_sqr(lam), p1[0]), p2[0])
    return x, f2_sub(f2_mul(lam, f2_sub(p1[0], x)), p1[1])


def mul(k, pt):
    """k pt for any integer k and any point of E(Fp2) (no reduction of k: the point's order need not divide R_ORDER)"""
    if k < 0:
        return mul(-k, neg(pt))
    acc = None
    for bit in bin(k)[2:] if k else "":
        acc = add(acc, acc)
        if bit == "1":
            acc = add(acc, pt)
    return acc


# psi (appendix G.3): the untwist-Frobenius-twist endomorphism, (conj(x) cx, conj(y) cy), and its square (x k, -y)
PSI_CX = f2_inv(f2_pow((1, 1), (P - 1) // 3))
PSI_CY = f2_inv(f2_pow((1, 1), (P - 1) // 2))
PSI2_K = pow(pow(2, (P - 1) // 3, P), -1, P)


def psi(pt):
    return None if pt is None else (f2_mul(f2_conj(pt[0]), PSI_CX), f2_mul(f2_conj(pt[1]), PSI_CY))


def psi2(pt):
    return None if pt is None else ((pt[0][0] * PSI2_K % P, pt[0][1] * PSI2_K % P), f2_neg(pt[1]))


def clear_cofactor_psi(pt):
    """appendix G.3, step by step with c1 = z = -BLS_Z_ABS: [z^2 - z - 1] P + [z - 1] psi(P) + psi^2(2 P)"""
    t1 = mul(-BLS_Z_ABS, pt)
    t2 = psi(pt)
    t3 = psi2(add(pt, pt))
    t3 = add(t3, neg(t2))
    t2 = add(t1, t2)
    t2 = mul(-BLS_Z_ABS, t2)
    t3 = add(t3, t2)
    t3 = add(t3, neg(t1))
    return add(t3, neg(pt))


def clear_cofactor(pt):
    """as the reference does it: times its `cofactor`"""
    return mul(H_EFF, pt)


def in_g2(pt):
    return pt is not None and on_curve(pt) and mul(R_ORDER, pt) is None


# ---------------------------------------------------------------- simplified SWU onto E' (RFC 9380 6.6.2) and the isogeny (E.3)
def iso_rhs(x):
    return f2_add(f2_add(f2_mul(f2_sqr(x), x), f2_mul(ISO_A, x)), ISO_B)


def sswu(u):
    """(x, y) on E'; tv1 = 0 (only u = 0 reaches it: -1 / Z is no square) takes x1 = B' / (Z A')"""
    z_u2 = f2_mul(SSWU_Z, f2_sqr(u))
    tv1 = f2_add(f2_sqr(z_u2), z_u2)
    if tv1 == ZERO:
        x1 = f2_mul(ISO_B, f2_inv(f2_mul(SSWU_Z, ISO_A)))
    else:
        x1 = f2_mul(f2_mul(f2_neg(ISO_B), f2_inv(ISO_A)), f2_add(ONE, f2_inv(tv1)))
    x, gx = x1, iso_rhs(x1)
    if not f2_is_square(gx):
        x = f2_mul(z_u2, x1)
        gx = iso_rhs(x)
    y = f2_sqrt(gx)
    assert y is not None and f2_sqr(y) == gx
    if f2_sgn0(u) != f2_sgn0(y):
        y = f2_neg(y)
    return x, y


def _poly(coeffs, x, monic):
    acc = ONE if monic else ZERO
    for c in reversed(coeffs):
        acc = f2_add(f2_mul(acc, x), c)
    return acc


def iso_map(pt):
    """E' -> E; ValueError where a denominator vanishes (no point of E'(Fp2) reaches it: test_bls12_381_g2_cpu.py)"""
    x, y = pt
    xd, yd = _poly(ISO_XDEN, x, True), _poly(ISO_YDEN, x, True)
    return f2_mul(_poly(ISO_XNUM, x, False), f2_inv(xd)), f2_mul(y, f2_mul(_poly(ISO_YNUM, x, False), f2_inv(yd)))


def map_to_curve(u):
    """map_to_curve_simple_swu: a point of E(Fp2), before any cofactor clearing"""
    pt = iso_map(sswu(u))
    assert on_curve(pt)
    return pt


def map_sum(us, clear):
    acc = None
    for u in us:
        acc = add(acc, map_to_curve(u))
    return clear_cofactor_psi(acc) if clear else acc


def encode_to_curve_ro(data):
    return map_sum(hash_to_field(data, 2, DST_RO), True)


def encode_to_curve_nu(data):
    return map_sum(hash_to_field(data, 1, DST_NU), True)


# ---------------------------------------------------------------- the device's limb images (fq28.hip.h: 14 limbs of 28 bits, R = 2^392)
MONT_R = 1 << 392


def limbs(v):
    """the limb image of the integer v (no Montgomery factor)"""
    return [(v >> (28 * i)) & 0xFFFFFFF for i in range(14)]


def mont_limbs(v):
    return limbs(v % P * MONT_R % P)
