"""Big-integer restatement of P521_RO / P521_NU (dot_ring/curve/specs/p521.py over short_weierstrass/sw_affine_point.py), written
from the reference's behaviour and RFC 9380 (section 5.3.1, expand_message_xmd; section 6.6.2, simplified SWU):

  group    y^2 = x^3 - 3 x + b over p = 2^521 - 1 with the affine chord-and-tangent law: the identity is None.  Prime order n, cofactor 1:
           no point has y = 0.  `mul` takes any integer (k P = (k mod n) P).
  hashing  expand_message_xmd over SHA-512 (Z_pad of 128 bytes), 98-byte big-endian chunks mod p, the DST QUUX-V01-CS02-with- || suite
           id (_RO_ replaced by _NU_ for the nonuniform variant; the suite id of the transcripts stays the RO one), the simplified SWU map
           straight onto the curve (A = -3, B = b, Z = -4, no isogeny), the sum of two images for RO.  Every u has an image; the
           exceptional branch tv1 = 0 is reached by u in {0, 2^520, 2^520 - 1} (Z u^2 = -1 iff u = +-1/2, and 2^520 = 1/2).
  codec    SEC1 compressed, 67 bytes: 0x02 / 0x03 by the parity of y, then x in 66 big-endian bytes.  The identity has no 67-byte string.

The Tiny / Thin / Pedersen layer (`WidthSuite`) is h2c_ref.Suite (SHA-512 in counter mode as the transcript hash) with the scalar width
and the nonce width taken from the group order: 66-byte scalars and an 82-byte nonce squeeze here, 32 and 48 for a 256-bit order — so the
same class instantiated with P-256's constants is held against the reference's P-256 proof vectors (tests/test_p521_cpu.py); the
reference holds no P-521 proof bytes.  The challenge is 16 bytes as for every suite (primitives.CHALLENGE_LEN), whatever the suite's
challenge_len = 32 says: a Tiny proof is 67 + 16 + 66 = 149 bytes, a Thin one 200, a Pedersen one 400.
Points are (x, y) tuples."""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import h2c_ref as h  # noqa: E402
import secp256k1_ref as k1  # noqa: E402

P = 2**521 - 1
N = 0x01FFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFA51868783BF2F966B7FCC0148F709A5D03BB5C9B8899C47AEBB6FB71E91386409
A = -3
B = 0x0051953EB9618E1C9A1F929A21A0B68540EEA2DA725B99B315F3B8B489918EF109E156193951EC7E937B1652C0BD3BB1BF073573DF883D2C34F1EF451FD46B503F00
G = (0x00C6858E06B70404E9CD9E3ECB662395B4429C648139053FB521F828AF606B4D3DBAA14B5E77EFE75928FE1DC127A2FFA8DE3348B3C1856A429BF97E7E31C2E5BD66,
     0x011839296A789A3BC0045C8A5FB42C7D1BD998F54449579B446817AFBD17273E662C97EE72995EF42640C550B9013FAD0761353C7086A272C24088BE94769FD16650)
BLINDING = G                             # the reference's blinding base IS the generator
Z = -4
L = 98
SUITE_ID = b"P521_XMD:SHA-512_SSWU_RO_"
DST_RO = b"QUUX-V01-CS02-with-" + SUITE_ID
DST_NU = DST_RO.replace(b"_RO_", b"_NU_")
O = None
HALF = 2**520                            # 1 / 2 mod p


def rhs(x):
    return (x * x * x + A * x + B) % P


def sqrt(v):
    """a root of v (p = 3 mod 4: v^((p + 1) / 4) = v^(2^519)) or None"""
    r = pow(v % P, 2**519, P)
    return r if r * r % P == v % P else None


def on_curve(pt):
    return pt is None or (pt[1] * pt[1] - rhs(pt[0])) % P == 0


def add(p1, p2):
    if p1 is None:
        return p2
    if p2 is None:
        return p1
    (x1, y1), (x2, y2) = p1, p2
    if x1 == x2:
        if (y1 + y2) % P == 0:
            return None
        lam = (3 * x1 * x1 + A) * pow(2 * y1, -1, P) % P
    else:
        lam = (y2 - y1) * pow(x2 - x1, -1, P) % P
    x3 = (lam * lam - x1 - x2) % P
    return x3, (lam * (x1 - x3) - y1) % P


def neg(pt):
    return None if pt is None else (pt[0], -pt[1] % P)


def mul(k, pt):
    """k pt for any integer k (a negative k negates the point)"""
    if k < 0:
        k, pt = -k, neg(pt)
    acc = None
    while k:
        if k & 1:
            acc = add(acc, pt)
        pt, k = add(pt, pt), k >> 1
    return acc


def msm(pts, ks):
    acc = None
    for pt, k in zip(pts, ks):
        acc = add(acc, mul(k, pt))
    return acc


# ---------------------------------------------------------------- codec (SWAffinePoint.point_to_string / string_to_point)
def raw(pt):
    """the library's 136 bytes: x || y little-endian, zero bytes for the identity"""
    return bytes(136) if pt is None else pt[0].to_bytes(68, "little") + pt[1].to_bytes(68, "little")


def encode(pt):
    if pt is None:
        return b"\x00"
    return bytes([2 + (pt[1] & 1)]) + pt[0].to_bytes(66, "big")


def decode(data):
    """string_to_point for a 67-byte string; 'bad' for what the reference refuses"""
    if len(data) != 67 or data[0] not in (2, 3):
        return "bad"
    x = int.from_bytes(data[1:], "big")
    if x >= P:
        return "bad"
    y = sqrt(rhs(x))
    if y is None:
        return "bad"
    return x, (y if y % 2 == data[0] % 2 else P - y)


# ---------------------------------------------------------------- hashing to the curve
def reduce_be98(chunk):
    return int.from_bytes(chunk, "big") % P


def hash_to_field(msg, count, dst):
    raw_ = h.expand_message_xmd(hashlib.sha512, 128, msg, dst, L * count)
    return [reduce_be98(raw_[L * i : L * i + L]) for i in range(count)]


def map_to_curve(u):
    """map_to_curve_simple_swu: one image"""
    u %= P
    tv1 = (Z * Z * pow(u, 4, P) + Z * u * u) % P
    if tv1 == 0:
        x1 = B * pow(Z * A % P, -1, P) % P
    else:
        x1 = -B * pow(A, -1, P) * (1 + pow(tv1, -1, P)) % P
    x, y = x1, sqrt(rhs(x1))
    if y is None:
        x = Z * u * u * x1 % P
        y = sqrt(rhs(x))
    if u % 2 != y % 2:
        y = P - y
    return x, y


def encode_to_curve_ro(data):
    u0, u1 = hash_to_field(data, 2, DST_RO)
    return add(map_to_curve(u0), map_to_curve(u1))


def encode_to_curve_nu(data):
    (u,) = hash_to_field(data, 1, DST_NU)
    return map_to_curve(u)


# ---------------------------------------------------------------- the VRF layer with the widths of the group order
class WidthSuite(h.Suite):
    """h2c_ref.Suite with the scalar width and the nonce squeeze of the order: (bits + 7) // 8 and (bits + 128 + 7) // 8"""

    def __init__(self, suite_id, order, generator, blinding, adder, encode_point, encode_to_curve, hash_fn, identity=None):
        super().__init__(suite_id, order, generator, blinding, adder, encode_point, encode_to_curve, hash_fn, identity=identity)
        self.scalar_len = (order.bit_length() + 7) // 8
        self.nonce_len = (order.bit_length() + 128 + 7) // 8

    def enc_scalar(self, k):
        return (k % self.n).to_bytes(self.scalar_len, "little")

    def nonce(self, secret, transcript):
        expanded = self.squeeze(transcript + b"\x10" + self.enc_scalar(secret), 64)
        return k1.le(self.squeeze(transcript + b"\x11" + expanded, self.nonce_len)) % self.n


def _suite(e2c):
    return WidthSuite(SUITE_ID, N, G, BLINDING, add, encode, e2c, hashlib.sha512)


RO = _suite(encode_to_curve_ro)
NU = _suite(encode_to_curve_nu)
TINY_LEN, THIN_LEN, PEDERSEN_LEN = 67 + 16 + 66, 67 + 67 + 66, 4 * 67 + 2 * 66


def public_key(sk):
    """public_key_from_secret: the generator times the little-endian integer of a secret of any length"""
    return encode(mul(int.from_bytes(sk, "little"), G))


def ietf_verify(suite, pk, proof, alpha, ad, thin=False, salt=b""):
    """TinyVRF.verify / ThinVRF.verify of a 149- / 200-byte proof under the 67-byte public key"""
    pk_pt, out = decode(pk), decode(proof[:67])
    if pk_pt == "bad" or out == "bad":
        return False
    s = int.from_bytes(proof[-66:], "little")
    i_pt = suite.e2c(salt + alpha)
    t, zs = suite.statement(1 if thin else 0, [(suite.g, pk_pt), (i_pt, out)], ad)
    m_in, m_out = add(suite.g, suite.mul(zs[1], i_pt)), add(pk_pt, suite.mul(zs[1], out))
    if thin:
        r = decode(proof[67:134])
        if r == "bad":
            return False
        return add(suite.mul(s, m_in), neg(suite.mul(suite.challenge([r], t), m_out))) == r
    c = int.from_bytes(proof[67:83], "little")
    r = add(suite.mul(s, m_in), neg(suite.mul(c, m_out)))
    return r is not None and suite.challenge([r], t) == c


def pedersen_verify(suite, proof, alpha, ad, salt=b""):
    pts = [decode(proof[67 * i : 67 * i + 67]) for i in range(4)]
    if "bad" in pts:
        return False
    out, ybar, r, ok = pts
    s, sb = int.from_bytes(proof[268:334], "little"), int.from_bytes(proof[334:], "little")
    i_pt = suite.e2c(salt + alpha)
    t, _ = suite.statement(2, [(i_pt, out)], ad)
    c = suite.challenge([r, ok], t + suite.enc(ybar))
    return (add(suite.mul(s, i_pt), neg(suite.mul(c, out))) == ok
            and add(add(suite.mul(s, suite.g), suite.mul(sb, suite.bb)), neg(suite.mul(c, ybar))) == r)


# ---------------------------------------------------------------- limb images of the device field (csrc/fp521.hip.h)
LIMBS, LIMB_BITS = 19, 28
NORMAL = (1 << 28) + (1 << 15)           # the bound of a "normal" limb: "k n" means |limb| <= k NORMAL


def limbs(v):
    """the image of 0 <= v < 2^532 with limbs in [0, 2^28)"""
    return [(v >> (LIMB_BITS * i)) & ((1 << LIMB_BITS) - 1) for i in range(LIMBS)]


def limb_value(image):
    return sum(x << (LIMB_BITS * i) for i, x in enumerate(image)) % P


ZERO_IMAGES = [limbs(0), limbs(P)]                                         # zero has two images
SPELLED = [(limbs(P), 0), (limbs(P + 1), 1), (limbs(2**521), 1), (limbs(2**532 - 1), (2**532 - 1) % P)]


def extreme_image(k, pattern, rng):
    """an image at the bound k n: all limbs +k n, all -k n, alternating, or random within it"""
    m = k * NORMAL
    if pattern == "pos":
        return [m] * LIMBS
    if pattern == "neg":
        return [-m] * LIMBS
    if pattern == "alt":
        return [m if i % 2 else -m for i in range(LIMBS)]
    return [rng.randint(-m, m) for _ in range(LIMBS)]


def contract_pairs(rng):
    """(a, b) images for mul(a, b) and sqr(a) at the contract's bounds (a <= 2 n; ka kb <= 6: 2 n x 3 n, and 1 n x 6 n with the sum and
    difference still within 32 bits), the two images of zero against each other and everything, and the limbs that spell p, p + 1, 2^521"""
    pairs = []
    for pa in ("pos", "neg", "alt", "rnd"):
        for pb in ("pos", "neg", "alt", "rnd"):
            pairs.append((extreme_image(2, pa, rng), extreme_image(3, pb, rng)))
            pairs.append((extreme_image(1, pa, rng), extreme_image(6, pb, rng)))
    special = ZERO_IMAGES + [image for image, _ in SPELLED] + [limbs(1), limbs(P - 1), limbs(rng.randrange(P))]
    pairs += [(a, b) for a in special for b in special]
    return pairs


def field_expectations(a, b):
    """what the device's and the host's field drivers must give for the pair: the values every record shares"""
    av, bv = limb_value(a), limb_value(b)
    return {"mul": av * bv % P, "sqr": av * av % P, "add": (av + bv) % P, "sub": (av - bv) % P, "neg": -av % P, "a": av,
            "small4": 4 * av % P, "smallneg": -(2**28 - 1) * av % P, "inv": pow(av, -1, P) if av else 0,
            "square": av == 0 or pow(av, (P - 1) // 2, P) == 1, "odd": av & 1, "zero": av == 0, "equal": av == bv}
