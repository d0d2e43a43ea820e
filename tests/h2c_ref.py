"""Big-integer restatement of the RFC 9380 variants of P-256 and Ed25519 (dot_ring/curve/specs/p256.py: P256_RO / P256_NU;
specs/ed25519.py: Ed25519_RO / Ed25519_NU), written from RFC 9380 and the reference's behaviour:

  P-256    expand_message_xmd over SHA-256 (Z_pad of 64 bytes), 48-byte big-endian chunks mod p, the simplified SWU map straight onto
           the curve (A = -3, B = b, Z = -10, no isogeny), the sum of two images for RO; points in the generic SEC1 compressed form
           (0x02 / 0x03 by the parity of y, then x big-endian), not P256_TAI's little-endian-x-plus-flag form.
  Ed25519  expand_message_xmd over SHA-512 (Z_pad of 128 bytes), Elligator 2 onto curve25519 (A = 486662, B = 1, Z = 2) as
           te_curve.py:48-95 runs it, then mont_to_ed25519 with the root curve.mod_sqrt (Tonelli-Shanks, z = 2) returns for -486664, the
           sum of two images for RO, and three doublings; Ed25519's own 32-byte codec.

The Tiny / Thin / Pedersen layer (`Suite`) is secp256k1_ref.Suite with the transcript hash as one more argument, so that the same code
can be held against the reference's P-256 (SHA-256) and Ed25519 (SHA-512) try-and-increment vector files (test_h2c_suites_cpu.py).
Points are (x, y) tuples; P-256's identity is None, Ed25519's is (0, 1)."""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ed25519_ref as ed  # noqa: E402
import p256_ref as p256  # noqa: E402
import secp256k1_ref as k1  # noqa: E402

P256_DST_RO = b"QUUX-V01-CS02-with-P256_XMD:SHA-256_SSWU_RO_"
P256_DST_NU = b"QUUX-V01-CS02-with-P256_XMD:SHA-256_SSWU_NU_"
ED_DST_RO = b"QUUX-V01-CS02-with-edwards25519_XMD:SHA-512_ELL2_RO_"
ED_DST_NU = b"QUUX-V01-CS02-with-edwards25519_XMD:SHA-512_ELL2_NU_"
P256_Z = -10
MONT_A, ELL2_Z = 486662, 2


# ---------------------------------------------------------------- hash to field (RFC 9380 section 5; curve.py:110-185)
def expand_message_xmd(hash_fn, block, msg, dst, length):
    dst_prime = dst + bytes([len(dst)])
    size = hash_fn().digest_size
    b0 = hash_fn(bytes(block) + msg + length.to_bytes(2, "big") + b"\x00" + dst_prime).digest()
    blocks = [hash_fn(b0 + b"\x01" + dst_prime).digest()]
    for i in range(2, -(-length // size) + 1):
        blocks.append(hash_fn(bytes(x ^ y for x, y in zip(b0, blocks[-1])) + bytes([i]) + dst_prime).digest())
    return b"".join(blocks)[:length]


def p256_hash_to_field(msg, count, dst):
    raw = expand_message_xmd(hashlib.sha256, 64, msg, dst, 48 * count)
    return [int.from_bytes(raw[48 * i : 48 * i + 48], "big") % p256.P for i in range(count)]


def ed_hash_to_field(msg, count, dst):
    raw = expand_message_xmd(hashlib.sha512, 128, msg, dst, 48 * count)
    return [int.from_bytes(raw[48 * i : 48 * i + 48], "big") % ed.P for i in range(count)]


# ---------------------------------------------------------------- P-256: simplified SWU (sw_affine_point.py:428-494), SEC1 codec
def p256_map_to_curve(u):
    p, a, b, z = p256.P, p256.A, p256.B, P256_Z
    tv1 = (z * z * pow(u, 4, p) + z * u * u) % p
    if tv1 == 0:
        x1 = b * pow(z * a % p, -1, p) % p
    else:
        x1 = -b * pow(a, -1, p) * (1 + pow(tv1, -1, p)) % p
    x, y = x1, p256.sqrt(p256.rhs(x1))
    if y is None:
        x = z * u * u * x1 % p
        y = p256.sqrt(p256.rhs(x))
    if u % 2 != y % 2:
        y = p - y
    return x, y


def p256_encode_to_curve_ro(data):
    u0, u1 = p256_hash_to_field(data, 2, P256_DST_RO)
    return p256.add(p256_map_to_curve(u0), p256_map_to_curve(u1))


def p256_encode_to_curve_nu(data):
    (u,) = p256_hash_to_field(data, 1, P256_DST_NU)
    return p256_map_to_curve(u)


def p256_sec1_encode(pt):
    return bytes([2 + (pt[1] & 1)]) + pt[0].to_bytes(32, "big")


def p256_sec1_decode(data):
    """SWAffinePoint.string_to_point for a 33-byte string; 'bad' for what the reference refuses"""
    if len(data) != 33 or data[0] not in (2, 3):
        return "bad"
    x = int.from_bytes(data[1:], "big")
    if x >= p256.P:
        return "bad"
    y = p256.sqrt(p256.rhs(x))
    if y is None:
        return "bad"
    return x, (y if y % 2 == data[0] % 2 else p256.P - y)


# ---------------------------------------------------------------- Ed25519: Elligator 2 (te_curve.py:48-95), mont_to_ed25519
def tonelli_shanks(v, p):
    """curve.py:274-330 (mod_sqrt): the root that algorithm returns, with z the first non-residue from 2 up"""
    v %= p
    if v == 0:
        return 0
    if pow(v, (p - 1) // 2, p) != 1:
        raise ValueError("No square root exists")
    q, s = p - 1, 0
    while q % 2 == 0:
        q, s = q // 2, s + 1
    z = 2
    while pow(z, (p - 1) // 2, p) == 1:
        z += 1
    m, c, t, r = s, pow(z, q, p), pow(v, q, p), pow(v, (q + 1) // 2, p)
    while t != 1:
        i, t2 = 1, t * t % p
        while t2 != 1:
            i, t2 = i + 1, t2 * t2 % p
        b = pow(c, 1 << (m - i - 1), p)
        m, c, t, r = i, b * b % p, t * b * b % p, r * b % p
    return r


SQRT_NEG_A_MINUS_2 = tonelli_shanks(-(MONT_A + 2), ed.P)


def ell2_mont(u):
    """(s, t) on curve25519"""
    p = ed.P
    tv1 = ELL2_Z * u * u % p
    if tv1 == p - 1:
        tv1 = 0
    x1 = -MONT_A * pow(tv1 + 1, -1, p) % p
    gx1 = ((x1 + MONT_A) * x1 + 1) * x1 % p
    e2 = gx1 == 0 or pow(gx1, (p - 1) // 2, p) == 1
    x, y2 = (x1, gx1) if e2 else ((-x1 - MONT_A) % p, tv1 * gx1 % p)
    y = tonelli_shanks(y2, p)
    if e2 ^ (y % 2 == 1):
        y = -y % p
    return x, y


def ed_map_to_curve(u):
    """Ed25519Point.map_to_curve; ValueError where the reference's modular inverse fails (t = 0 or s = -1)"""
    p = ed.P
    s, t = ell2_mont(u)
    if t == 0 or (s + 1) % p == 0:
        raise ValueError("base is not invertible for the given modulus")
    pt = (SQRT_NEG_A_MINUS_2 * s * pow(t, -1, p) % p, (s - 1) * pow(s + 1, -1, p) % p)
    assert ed.on_curve(pt)
    return pt


def ed_clear_cofactor(pt):
    for _ in range(3):
        pt = ed.add(pt, pt)
    return pt


def ed_encode_to_curve_ro(data):
    u0, u1 = ed_hash_to_field(data, 2, ED_DST_RO)
    return ed_clear_cofactor(ed.add(ed_map_to_curve(u0), ed_map_to_curve(u1)))


def ed_encode_to_curve_nu(data):
    (u,) = ed_hash_to_field(data, 1, ED_DST_NU)
    return ed_clear_cofactor(ed_map_to_curve(u))


# ---------------------------------------------------------------- the VRF layer, generic over curve and transcript hash
def squeeze_with(hash_fn):
    def squeeze(absorbed, size):
        seed, out, ctr = hash_fn(absorbed).digest(), b"", 0
        while len(out) < size:
            out += hash_fn(seed + ctr.to_bytes(8, "little")).digest()
            ctr += 1
        return out[:size]
    return squeeze


class Suite(k1.Suite):
    """secp256k1_ref.Suite with the transcript hash and the group's identity as arguments (its own are SHA-256 and None)"""

    def __init__(self, suite_id, order, generator, blinding, adder, encode_point, encode_to_curve, hash_fn, identity=None):
        super().__init__(suite_id, order, generator, blinding, adder, encode_point, encode_to_curve)
        self.squeeze, self.identity = squeeze_with(hash_fn), identity

    def mul(self, k, pt):
        acc = self.identity
        for bit in bin(k % self.n)[2:] if k % self.n else "":
            acc = self.add(acc, acc)
            if bit == "1":
                acc = self.add(acc, pt)
        return acc

    def nonce(self, secret, transcript):
        expanded = self.squeeze(transcript + b"\x10" + self.enc_scalar(secret), 64)
        return k1.le(self.squeeze(transcript + b"\x11" + expanded, 48)) % self.n

    def challenge(self, points, transcript):
        return k1.le(self.squeeze(transcript + b"\x40" + b"".join(self.enc(p) for p in points), 16)) % self.n

    def statement(self, scheme, ios, ad):
        t = self.suite_id + bytes([scheme]) + len(ios).to_bytes(8, "little") + b"".join(self.enc(i) + self.enc(o) for i, o in ios)
        t += len(ad).to_bytes(8, "little") + ad
        stream = self.squeeze(t + b"\x30", 16 * (len(ios) - 1)) if len(ios) > 1 else b""
        return t, [1] + [k1.le(stream[16 * j : 16 * j + 16]) % self.n for j in range(len(ios) - 1)]

    def point_to_hash(self, pt):
        return self.squeeze(self.suite_id + b"\x20" + self.enc(pt), 32)


def _p256(encode_point, e2c):
    return Suite(p256.SUITE_ID, p256.N, p256.G, p256.BLINDING, p256.add, encode_point, e2c, hashlib.sha256)


def _ed(e2c):
    return Suite(ed.SUITE_ID, ed.N, ed.G, ed.BLINDING, ed.add, ed.encode, e2c, hashlib.sha512, identity=ed.O)


# the try-and-increment suites (the reference holds proof files for these) and the four RFC 9380 variants (it holds none)
P256_TAI = _p256(p256.encode, lambda data: p256.encode_to_curve(data)[0])
ED25519_TAI = _ed(lambda data: ed.encode_to_curve(data)[0])
P256_RO = _p256(p256_sec1_encode, p256_encode_to_curve_ro)
P256_NU = _p256(p256_sec1_encode, p256_encode_to_curve_nu)
ED25519_RO = _ed(ed_encode_to_curve_ro)
ED25519_NU = _ed(ed_encode_to_curve_nu)
