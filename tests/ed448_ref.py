"""Big-integer restatement of Ed448_RO / Ed448_NU (dot_ring/curve/specs/ed448.py), written from RFC 9380 (section 5.3.3 for
expand_message_xof, sections 6.7.2 and 6.8.2 for Elligator 2, appendix D.2 for the rational map in the reference's form) and RFC 7748's
4-isogeny between curve448 and edwards448:

  group    x^2 + y^2 = 1 + d x^2 y^2 with a = 1 and d = -39081 over p = 2^448 - 2^224 - 1, order 4 n, the affine unified addition (complete:
           d is a non-square); the identity is (0, 1).
  hashing  expand_message_xof over SHAKE256 with L = 84 and the DST QUUX-V01-CS02-with- || suite id (_RO_ replaced by _NU_ for the
           nonuniform variant), Elligator 2 onto curve448 (A = 156326, B = 1, Z = -1), the map to the Edwards curve with inv(0) = 0 as the
           reference's modular inverse has it (the result (0, 0) is then no point: ValueError), the sum of two images for RO, times 4.
  codec    x || y, 56 little-endian bytes each; scalars 56 bytes.

The Tiny / Thin / Pedersen layer is `XofSuite`: h2c_ref.Suite (imported, not edited) with three changes — the XOF squeeze
(shake(absorbed).digest(size)), the scalar width, and the nonce width (order bits + 128, rounded up to bytes).  The reference holds no
Ed448 proof bytes, so those three changes are pinned by instantiating the same class for Bandersnatch SHAKE128 over oracle/pyref's group
and reproducing the reference's bandersnatch_shake128_ell2_{tiny,thin,pedersen}.json (tests/test_ed448_cpu.py).
Points are (x, y) tuples."""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import h2c_ref as h  # noqa: E402
import secp256k1_ref as k1  # noqa: E402

P = 2**448 - 2**224 - 1
N = 2**446 - 0x8335DC163BB124B65129C96FDE933D8D723A70AADC873D6D54A7BB0D
H = 4
D = -39081 % P
MONT_A, ELL2_Z = 156326, -1
G = (117812161263436946737282484343310064665180535357016373416879082147939404277809514858788439644911793978499419995990477371552926308078495,
     19)
BLINDING = G
O = (0, 1)
SUITE_ID = b"edwards448_XOF:SHAKE256_ELL2_RO_"
DST_RO = b"QUUX-V01-CS02-with-" + SUITE_ID
DST_NU = DST_RO.replace(b"_RO_", b"_NU_")
XOF_L = 84


def inv0(v):
    """the reference's curve.inv: pow(v, p - 2, p), so inv(0) = 0"""
    return pow(v % P, P - 2, P)


def on_curve(pt):
    x, y = pt
    return (x * x + y * y - 1 - D * x * x % P * y * y) % P == 0


def add(p1, p2):
    (x1, y1), (x2, y2) = p1, p2
    t = D * x1 % P * x2 % P * y1 % P * y2 % P
    return (x1 * y2 + x2 * y1) * pow(1 + t, -1, P) % P, (y1 * y2 - x1 * x2) * pow(1 - t, -1, P) % P


def neg(pt):
    return -pt[0] % P, pt[1]


def mul(k, pt):
    """k pt for any k >= 0 (not reduced: points outside the prime-order subgroup)"""
    acc = O
    while k:
        if k & 1:
            acc = add(acc, pt)
        pt, k = add(pt, pt), k >> 1
    return acc


def msm(pts, ks):
    acc = O
    for pt, k in zip(pts, ks):
        acc = add(acc, mul(k, pt))
    return acc


def raw(pt):
    return pt[0].to_bytes(56, "little") + pt[1].to_bytes(56, "little")


encode = raw


def decode(data, check=False):
    """uncompressed_s2p and the point constructor; check: also curve.valid_point; 'bad' for what the reference refuses"""
    if len(data) != 112:
        return "bad"
    pt = (int.from_bytes(data[:56], "little"), int.from_bytes(data[56:], "little"))
    if pt[0] >= P or pt[1] >= P or not on_curve(pt):
        return "bad"
    if check and (pt == O or mul(N, pt) != O):
        return "bad"
    return pt


# ---------------------------------------------------------------- hashing to the curve
def expand_message_xof(msg, dst, length):
    return hashlib.shake_256(msg + length.to_bytes(2, "big") + dst + bytes([len(dst)])).digest(length)


def hash_to_field(msg, count, dst):
    stream = expand_message_xof(msg, dst, XOF_L * count)
    return [int.from_bytes(stream[XOF_L * i : XOF_L * (i + 1)], "big") % P for i in range(count)]


def sqrt(v):
    r = pow(v % P, (P + 1) // 4, P)
    return r if r * r % P == v % P else None


def ell2_mont(u):
    """RFC 9380 6.7.2 onto curve448: (s, t) with t^2 = s^3 + A s^2 + s"""
    tv1 = ELL2_Z * u * u % P
    if tv1 == P - 1:
        tv1 = 0
    x1 = -MONT_A * pow(tv1 + 1, -1, P) % P
    gx1 = ((x1 + MONT_A) * x1 + 1) * x1 % P
    y = sqrt(gx1)
    e2 = y is not None
    x = x1
    if not e2:
        x = (-x1 - MONT_A) % P
        y = sqrt(tv1 * gx1)
    if e2 ^ (y % 2 == 1):
        y = -y % P
    assert (y * y - ((x + MONT_A) * x + 1) * x) % P == 0
    return x, y


def mont_to_edwards_fractions(u, v):
    """(x_num, x_den, y_num, y_den) of RFC 7748's 4-isogeny from curve448 as appendix D.2 of RFC 9380 states it"""
    u2, v2 = u * u % P, v * v % P
    return (4 * v * (u2 - 1) % P, (u2 * u2 - 2 * u2 + 4 * v2 + 1) % P,
            -u * (u2 * u2 - 2 * u2 - 4 * v2 + 1) % P, (u * u2 * u2 - 2 * u2 * v2 - 2 * u * u2 - 2 * v2 + u) % P)


def map_to_curve(u):
    """Ed448Point.map_to_curve: one image, the cofactor not cleared; ValueError where a denominator vanishes"""
    xn, xd, yn, yd = mont_to_edwards_fractions(*ell2_mont(u % P))
    pt = (xn * inv0(xd) % P, yn * inv0(yd) % P)
    if not on_curve(pt):
        raise ValueError("Point is not on the curve")
    return pt


def clear_cofactor(pt):
    for _ in range(2):
        pt = add(pt, pt)
    return pt


def encode_to_curve_ro(data):
    u0, u1 = hash_to_field(data, 2, DST_RO)
    return clear_cofactor(add(map_to_curve(u0), map_to_curve(u1)))


def encode_to_curve_nu(data):
    (u,) = hash_to_field(data, 1, DST_NU)
    return clear_cofactor(map_to_curve(u))


# ---------------------------------------------------------------- the VRF layer: h2c_ref's with an XOF and wider scalars
def squeeze_xof(hash_fn):
    return lambda absorbed, size: hash_fn(absorbed).digest(size)


class XofSuite(h.Suite):
    """h2c_ref.Suite over an extendable-output transcript hash, with the scalar width and the nonce width of the group order"""

    def __init__(self, suite_id, order, generator, blinding, adder, encode_point, encode_to_curve, hash_fn, identity):
        super().__init__(suite_id, order, generator, blinding, adder, encode_point, encode_to_curve, hash_fn, identity=identity)
        self.squeeze = squeeze_xof(hash_fn)
        self.scalar_len = (order.bit_length() + 7) // 8
        self.nonce_len = (order.bit_length() + 128 + 7) // 8

    def enc_scalar(self, k):
        return (k % self.n).to_bytes(self.scalar_len, "little")

    def nonce(self, secret, transcript):
        expanded = self.squeeze(transcript + b"\x10" + self.enc_scalar(secret), 64)
        return k1.le(self.squeeze(transcript + b"\x11" + expanded, self.nonce_len)) % self.n


def _suite(e2c):
    return XofSuite(SUITE_ID, N, G, BLINDING, add, encode, e2c, hashlib.shake_256, O)


RO = _suite(encode_to_curve_ro)
NU = _suite(encode_to_curve_nu)


def ietf_verify(suite, pk, proof, alpha, ad, thin=False, salt=b""):
    """TinyVRF.verify / ThinVRF.verify of a 184- / 280-byte proof under the 112-byte public key"""
    pk_pt, out = decode(pk, check=True), decode(proof[:112], check=True)
    if pk_pt == "bad" or out == "bad":
        return False
    s = int.from_bytes(proof[-56:], "little")
    i_pt = suite.e2c(salt + alpha)
    t, zs = suite.statement(1 if thin else 0, [(suite.g, pk_pt), (i_pt, out)], ad)
    m_in, m_out = add(suite.g, suite.mul(zs[1], i_pt)), add(pk_pt, suite.mul(zs[1], out))
    if thin:
        r = decode(proof[112:224], check=True)
        if r == "bad":
            return False
        return add(suite.mul(s, m_in), neg(suite.mul(suite.challenge([r], t), m_out))) == r
    c = int.from_bytes(proof[112:128], "little")
    return suite.challenge([add(suite.mul(s, m_in), neg(suite.mul(c, m_out)))], t) == c
