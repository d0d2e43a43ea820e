"""Big-integer restatement of P384_RO / P384_NU (dot_ring/curve/specs/p384.py over short_weierstrass/sw_affine_point.py), written
from the reference's behaviour and RFC 9380 (section 5.3.1, expand_message_xmd; section 6.6.2, simplified SWU):

  group    y^2 = x^3 - 3 x + b over p = 2^384 - 2^128 - 2^96 + 2^32 - 1 with the affine chord-and-tangent law: the identity is None.
           Prime order n, cofactor 1: no point has y = 0.  `mul` takes any integer (k P = (k mod n) P).
  hashing  expand_message_xmd over SHA-384 (Z_pad of 128 bytes, 48-byte digests), 72-byte big-endian chunks mod p, the DST
           QUUX-V01-CS02-with- || suite id (_RO_ replaced by _NU_ for the nonuniform variant; the suite id of the transcripts stays the RO
           one), the simplified SWU map straight onto the curve (A = -3, B = b, Z = -12, no isogeny), the sum of two images for RO.  Every
           u has an image; the exceptional branch tv1 = 0 is reached by u in {0, s, p - s} with s^2 = 1 / 12.
  codec    SEC1 compressed, 49 bytes: 0x02 / 0x03 by the parity of y, then x in 48 big-endian bytes.  The identity has no 49-byte string.

The Tiny / Thin / Pedersen layer is p521_ref.WidthSuite (which tests/test_p521_cpu.py pins on the reference's P-256 proof files) with
P-384's constants and SHA-384 as the transcript hash: 48-byte scalars and a 64-byte nonce squeeze.  The reference holds no P-384 proof
bytes.  The challenge is 16 bytes as for every suite: a Tiny proof is 49 + 16 + 48 = 113 bytes, a Thin one 146, a Pedersen one 292.
Points are (x, y) tuples."""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import h2c_ref as h  # noqa: E402
import p521_ref as p521  # noqa: E402

P = 2**384 - 2**128 - 2**96 + 2**32 - 1
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFC7634D81F4372DDF581A0DB248B0A77AECEC196ACCC52973
A = -3
B = 0xB3312FA7E23EE7E4988E056BE3F82D19181D9C6EFE8141120314088F5013875AC656398D8A2ED19D2A85C8EDD3EC2AEF
G = (0xAA87CA22BE8B05378EB1C71EF320AD746E1D3B628BA79B9859F741E082542A385502F25DBF55296C3A545E3872760AB7,
     0x3617DE4A96262C6F5D9E98BF9292DC29F8F41DBD289A147CE9DA3113B5F0B8C00A60B1CE1D7E819D7A431D7C90EA0E5F)
BLINDING = G                             # the reference's blinding base IS the generator
Z = -12
L = 72
SUITE_ID = b"P384_XMD:SHA-384_SSWU_RO_"
DST_RO = b"QUUX-V01-CS02-with-" + SUITE_ID
DST_NU = DST_RO.replace(b"_RO_", b"_NU_")
O = None


def rhs(x):
    return (x * x * x + A * x + B) % P


def sqrt(v):
    """a root of v (p = 3 mod 4: v^((p + 1) / 4)) or None"""
    r = pow(v % P, (P + 1) // 4, P)
    return r if r * r % P == v % P else None


S = min(sqrt(pow(12, -1, P)), P - sqrt(pow(12, -1, P)))      # s^2 = 1 / 12: Z s^2 = -1


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
    """the library's 96 bytes: x || y little-endian, zero bytes for the identity"""
    return bytes(96) if pt is None else pt[0].to_bytes(48, "little") + pt[1].to_bytes(48, "little")


def encode(pt):
    if pt is None:
        return b"\x00"
    return bytes([2 + (pt[1] & 1)]) + pt[0].to_bytes(48, "big")


def decode(data):
    """string_to_point for a 49-byte string; 'bad' for what the reference refuses"""
    if len(data) != 49 or data[0] not in (2, 3):
        return "bad"
    x = int.from_bytes(data[1:], "big")
    if x >= P:
        return "bad"
    y = sqrt(rhs(x))
    if y is None:
        return "bad"
    return x, (y if y % 2 == data[0] % 2 else P - y)


# ---------------------------------------------------------------- hashing to the curve
def reduce_be72(chunk):
    return int.from_bytes(chunk, "big") % P


def hash_to_field(msg, count, dst):
    raw_ = h.expand_message_xmd(hashlib.sha384, 128, msg, dst, L * count)
    return [reduce_be72(raw_[L * i : L * i + L]) for i in range(count)]


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
def _suite(e2c):
    return p521.WidthSuite(SUITE_ID, N, G, BLINDING, add, encode, e2c, hashlib.sha384)


RO = _suite(encode_to_curve_ro)
NU = _suite(encode_to_curve_nu)
TINY_LEN, THIN_LEN, PEDERSEN_LEN = 49 + 16 + 48, 49 + 49 + 48, 4 * 49 + 2 * 48


def public_key(sk):
    """public_key_from_secret: the generator times the little-endian integer of a secret of any length"""
    return encode(mul(int.from_bytes(sk, "little"), G))


def ietf_verify(suite, pk, proof, alpha, ad, thin=False, salt=b""):
    """TinyVRF.verify / ThinVRF.verify of a 113- / 146-byte proof under the 49-byte public key"""
    pk_pt, out = decode(pk), decode(proof[:49])
    if pk_pt == "bad" or out == "bad":
        return False
    s = int.from_bytes(proof[-48:], "little")
    i_pt = suite.e2c(salt + alpha)
    t, zs = suite.statement(1 if thin else 0, [(suite.g, pk_pt), (i_pt, out)], ad)
    m_in, m_out = add(suite.g, suite.mul(zs[1], i_pt)), add(pk_pt, suite.mul(zs[1], out))
    if thin:
        r = decode(proof[49:98])
        if r == "bad":
            return False
        return add(suite.mul(s, m_in), neg(suite.mul(suite.challenge([r], t), m_out))) == r
    c = int.from_bytes(proof[49:65], "little")
    r = add(suite.mul(s, m_in), neg(suite.mul(c, m_out)))
    return r is not None and suite.challenge([r], t) == c


def pedersen_verify(suite, proof, alpha, ad, salt=b""):
    pts = [decode(proof[49 * i : 49 * i + 49]) for i in range(4)]
    if "bad" in pts:
        return False
    out, ybar, r, ok = pts
    s, sb = int.from_bytes(proof[196:244], "little"), int.from_bytes(proof[244:], "little")
    i_pt = suite.e2c(salt + alpha)
    t, _ = suite.statement(2, [(i_pt, out)], ad)
    c = suite.challenge([r, ok], t + suite.enc(ybar))
    return (add(suite.mul(s, i_pt), neg(suite.mul(c, out))) == ok
            and add(add(suite.mul(s, suite.g), suite.mul(sb, suite.bb)), neg(suite.mul(c, ybar))) == r)


# ---------------------------------------------------------------- limb images of the device field (csrc/fp384.hip.h)
# The field is in Montgomery form with R = 2^392: an image stands for its value times R^-1 mod p.
LIMBS, LIMB_BITS = 14, 28
R = 1 << 392
R_INV = pow(R, -1, P)
NORMAL = (1 << 28) + (1 << 22)           # the bound of a "normal" limb 0..12: "k n" means |limb| <= k NORMAL there ...
NORMAL_TOP = 1 << 21                     # ... and |limb 13| <= k NORMAL_TOP, which keeps |value| below k 2^385


def limbs(v):
    """the image of 0 <= v < 2^392 with limbs in [0, 2^28)"""
    return [(v >> (LIMB_BITS * i)) & ((1 << LIMB_BITS) - 1) for i in range(LIMBS)]


def mont(x):
    """the canonical image of the element x"""
    return limbs(x * R % P)


def limb_value(image):
    """the element an image stands for"""
    return sum(x << (LIMB_BITS * i) for i, x in enumerate(image)) * R_INV % P


ZERO_IMAGES = [limbs(0), limbs(P)]                                         # zero has two images among the carried ones
SPELLED = [(limbs(v), v * R_INV % P) for v in (P, P + 1, 2**384, 2**392 - 1)]


def extreme_image(k, pattern, rng):
    """an image at the bound k n: all limbs +k n, all -k n, alternating, or random within it"""
    bound = [k * NORMAL] * (LIMBS - 1) + [k * NORMAL_TOP]
    if pattern == "pos":
        return bound
    if pattern == "neg":
        return [-m for m in bound]
    if pattern == "alt":
        return [m if i % 2 else -m for i, m in enumerate(bound)]
    return [rng.randint(-m, m) for m in bound]


def wide_image(k, pattern, rng):
    """the same with limb 13 at k NORMAL too: within mul's limb budget, outside "k n" by value (k 2^392).  A product with a k n operand
    is still right, though not normal: |T| < 2^395 fits the 32 bits of limb 13."""
    image = extreme_image(k, pattern, rng)
    image[-1] = {"pos": 1, "neg": -1, "alt": 1}.get(pattern, 1) * k * NORMAL
    return image


PATTERNS = ("pos", "neg", "alt", "rnd")


def contract_pairs(rng):
    """(a, b) images for mul(a, b) and sqr(a) at the contract's bounds (a <= 2 n; ka kb <= 8: 2 n x 4 n; and 1 n x 6 n: the drivers also
    add and subtract the pair, and mul2_quads holds 1 n x 7 n: an 8 n limb does not fit 32 bits), one operand with its top limb as large
    as the others, the images of zero against each other and everything, and the limbs that spell p, p + 1, 2^384 and 2^392 - 1"""
    pairs = []
    for pa in PATTERNS:
        for pb in PATTERNS:
            pairs.append((extreme_image(2, pa, rng), extreme_image(4, pb, rng)))
            pairs.append((extreme_image(1, pa, rng), extreme_image(6, pb, rng)))
        pairs.append((wide_image(2, pa, rng), extreme_image(4, pa, rng)))
    special = ZERO_IMAGES + [image for image, _ in SPELLED] + [limbs(1), limbs(P - 1), mont(1), mont(P - 1), limbs(rng.randrange(P))]
    pairs += [(a, b) for a in special for b in special]
    return pairs


def mul2_quads(rng):
    """(a, b, c, d) images for mul2 at ka kb + kc kd = 8: 2 n x 2 n + 2 n x 2 n, 1 n x 5 n + 1 n x 3 n, and 1 n x 7 n + 1 n x 1 n (7 n is the largest class a 32-bit
    limb holds), every sign pattern alike"""
    quads = []
    for pa in PATTERNS:
        quads.append(tuple(extreme_image(2, pa, rng) for _ in range(4)))
        quads.append((extreme_image(1, pa, rng), extreme_image(5, pa, rng), extreme_image(1, pa, rng), extreme_image(3, pa, rng)))
        quads.append((extreme_image(1, pa, rng), extreme_image(7, pa, rng), extreme_image(1, pa, rng), extreme_image(1, pa, rng)))
        quads.append((extreme_image(2, pa, rng), extreme_image(2, "rnd", rng), extreme_image(2, "rnd", rng), extreme_image(2, pa, rng)))
    return quads


def field_expectations(a, b):
    """what the device's and the host's field drivers must give for the pair: the values every record shares"""
    av, bv = limb_value(a), limb_value(b)
    return {"mul": av * bv % P, "sqr": av * av % P, "add": (av + bv) % P, "sub": (av - bv) % P, "neg": -av % P, "a": av,
            "small4": 4 * av % P, "smallneg": -(2**28 - 1) * av % P, "inv": pow(av, -1, P) if av else 0,
            "square": av == 0 or pow(av, (P - 1) // 2, P) == 1, "odd": av & 1, "zero": av == 0, "equal": av == bv}
