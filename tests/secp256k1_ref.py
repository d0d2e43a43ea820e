"""Big-integer restatement of the secp256k1 suites (dot_ring/curve/specs/secp256k1.py: Secp256k1_RO and Secp256k1_NU), written from RFC 9380
and the reference's behaviour: the field, the affine group of y^2 = x^3 + 7, the SEC1 compressed codec (0x02 / 0x03 by the parity of
y, then x big-endian), expand_message_xmd with SHA-256 (Z_pad of 64 bytes), hash_to_field (48-byte big-endian chunks mod p), the
simplified SWU map onto E': y^2 = x^3 + A' x + 1771 with Z = -11, the 3-isogeny of RFC 9380 appendix E.1 back to secp256k1, and the
RO / NU encodings of salt || alpha.  The Tiny / Thin / Pedersen layer below (`Suite`) is curve-generic: it takes the curve's constants,
point codec and encode-to-curve as arguments, so that the same code, given P-256's (p256_ref.py), can be held against the vector files
the reference has for that suite (test_secp256k1_cpu.py).  Points are (x, y) tuples; the identity is None."""
import hashlib

P = 2**256 - 2**32 - 977
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
B = 7
G = (0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798,
     0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8)
BLINDING = (0x50929B74C1A04954B78B4B6035E97A5E078A5A0F28EC96D547BFEE9ACE803AC0,
            0x31D3C6863973926E049E637CB1B5F40A36DAC28AF1766968C30C2313F3A38904)
SUITE_ID = b"secp256k1_XMD:SHA-256_SSWU_RO_"                     # both variants
DST_RO = b"QUUX-V01-CS02-with-secp256k1_XMD:SHA-256_SSWU_RO_"
DST_NU = b"QUUX-V01-CS02-with-secp256k1_XMD:SHA-256_SSWU_NU_"
# E' and the map's Z (RFC 9380 section 8.7), the 3-isogeny's coefficients (appendix E.1), highest degree first
ISO_A = 0x3F8731ABDD661ADCA08A5558F0F5D272E953D363CB6F0E5D405447C01A444533
ISO_B = 1771
Z = -11
X_NUM = (0x8E38E38E38E38E38E38E38E38E38E38E38E38E38E38E38E38E38E38DAAAAA88C,
         0x534C328D23F234E6E2A413DECA25CAECE4506144037C40314ECBD0B53D9DD262,
         0x07D3D4C80BC321D5B9F315CEA7FD44C5D595D2FC0BF63B92DFFF1044F17C6581,
         0x8E38E38E38E38E38E38E38E38E38E38E38E38E38E38E38E38E38E38DAAAAA8C7)
X_DEN = (1,
         0xEDADC6F64383DC1DF7C4B2D51B54225406D36B641F5E41BBC52A56612A8C6D14,
         0xD35771193D94918A9CA34CCBB7B640DD86CD409542F8487D9FE6B745781EB49B)
Y_NUM = (0x2F684BDA12F684BDA12F684BDA12F684BDA12F684BDA12F684BDA12F38E38D84,
         0x29A6194691F91A73715209EF6512E576722830A201BE2018A765E85A9ECEE931,
         0xC75E0C32D5CB7C0FA9D0A54B12A0A6D5647AB046D686DA6FDFFC90FC201D71A3,
         0x4BDA12F684BDA12F684BDA12F684BDA12F684BDA12F684BDA12F684B8E38E23C)
Y_DEN = (1,
         0x6484AA716545CA2CF3A70C3FA8FE337E0A3D21162F0D6299A7BF8192BFD2A76F,
         0x7A06534BB8BDB49FD5E9E6632722C2989467C1BFC8E8D978DFB425D2685C2573,
         0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEFFFFF93B)
O = None


# ---------------------------------------------------------------- field and group
def sqrt(v, p=P):
    """a square root of v mod p (p = 3 mod 4), or None"""
    v %= p
    r = pow(v, (p + 1) // 4, p)
    return r if r * r % p == v else None


def rhs(x):
    return (x * x * x + B) % P


def on_curve(pt):
    return pt is None or (pt[1] * pt[1] - rhs(pt[0])) % P == 0


def sw_add(p1, p2, a, p):
    """affine short Weierstrass addition on y^2 = x^3 + a x + b over GF(p)"""
    if p1 is None:
        return p2
    if p2 is None:
        return p1
    (x1, y1), (x2, y2) = p1, p2
    if x1 == x2:
        if (y1 + y2) % p == 0:
            return None
        lam = (3 * x1 * x1 + a) * pow(2 * y1, -1, p) % p
    else:
        lam = (y2 - y1) * pow(x2 - x1, -1, p) % p
    x3 = (lam * lam - x1 - x2) % p
    return x3, (lam * (x1 - x3) - y1) % p


def add(p1, p2):
    return sw_add(p1, p2, 0, P)


def neg(pt):
    return None if pt is None else (pt[0], -pt[1] % P)


def mul(k, pt, adder=add):
    acc = None
    for bit in bin(k)[2:] if k > 0 else "":
        acc = adder(acc, acc)
        if bit == "1":
            acc = adder(acc, pt)
    return acc


def msm(pts, ks):
    acc = None
    for pt, k in zip(pts, ks):
        acc = add(acc, mul(k % N, pt))
    return acc


def raw(pt):
    """the ABI's affine x || y little-endian; the identity is 64 zero bytes"""
    return bytes(64) if pt is None else pt[0].to_bytes(32, "little") + pt[1].to_bytes(32, "little")


# ---------------------------------------------------------------- SEC1 compressed codec (sw_affine_point.py)
def encode(pt):
    return bytes([2 + (pt[1] & 1)]) + pt[0].to_bytes(32, "big")


def decode(data, check=True):
    """string_to_point for a 33-byte string; 'bad' for what the reference refuses.  No encoding of the identity exists, so `check`
    (dec_point's valid_point: not the identity, cofactor 1) changes nothing here; it is kept for the shape of the other restatements."""
    if len(data) != 33 or data[0] not in (2, 3):
        return "bad"
    x = int.from_bytes(data[1:], "big")
    if x >= P:
        return "bad"
    y = sqrt(rhs(x))
    if y is None:
        return "bad"
    if y % 2 != data[0] % 2:
        y = P - y
    return x, y


# ---------------------------------------------------------------- hash to field (RFC 9380 section 5; curve.py:110-185)
def expand_message_xmd(msg, dst, length):
    dst_prime = dst + bytes([len(dst)])
    ell = -(-length // 32)
    b0 = hashlib.sha256(bytes(64) + msg + length.to_bytes(2, "big") + b"\x00" + dst_prime).digest()
    blocks = [hashlib.sha256(b0 + b"\x01" + dst_prime).digest()]
    for i in range(2, ell + 1):
        blocks.append(hashlib.sha256(bytes(x ^ y for x, y in zip(b0, blocks[-1])) + bytes([i]) + dst_prime).digest())
    return b"".join(blocks)[:length]


def hash_to_field(msg, count, dst):
    raw_bytes = expand_message_xmd(msg, dst, 48 * count)
    return [int.from_bytes(raw_bytes[48 * i : 48 * i + 48], "big") % P for i in range(count)]


# ---------------------------------------------------------------- simplified SWU and the isogeny (RFC 9380 sections 6.6.2, 6.6.3)
def sswu(u):
    """(x, y) on E' and whether gx1 was a square (the branch taken)"""
    tv1 = (Z * Z * pow(u, 4, P) + Z * u * u) % P
    if tv1 == 0:
        x1 = ISO_B * pow(Z * ISO_A % P, -1, P) % P
    else:
        x1 = -ISO_B * pow(ISO_A, -1, P) * (1 + pow(tv1, -1, P)) % P
    gx1 = (x1**3 + ISO_A * x1 + ISO_B) % P
    x2 = Z * u * u * x1 % P
    gx2 = (x2**3 + ISO_A * x2 + ISO_B) % P
    y = sqrt(gx1)
    first = y is not None
    x = x1
    if not first:
        x, y = x2, sqrt(gx2)
    if u % 2 != y % 2:
        y = P - y
    return (x, y), first


def horner(coefficients, x):
    v = 0
    for c in coefficients:
        v = (v * x + c) % P
    return v


def iso_map(pt):
    x, y = pt
    return (horner(X_NUM, x) * pow(horner(X_DEN, x), -1, P) % P, y * horner(Y_NUM, x) * pow(horner(Y_DEN, x), -1, P) % P)


def map_to_curve(u):
    return iso_map(sswu(u)[0])


def encode_to_curve_ro(data):
    u0, u1 = hash_to_field(data, 2, DST_RO)
    return add(map_to_curve(u0), map_to_curve(u1))


def encode_to_curve_nu(data):
    (u,) = hash_to_field(data, 1, DST_NU)
    return map_to_curve(u)


# ---------------------------------------------------------------- the VRF layer, generic over the curve (primitives.py, vrf/ietf, vrf/pedersen)
def le(b):
    return int.from_bytes(b, "little")


def squeeze(absorbed, size):
    """SHA-256 in counter mode: the transcript hash of the 256-bit Weierstrass suites"""
    seed, out, ctr = hashlib.sha256(absorbed).digest(), b"", 0
    while len(out) < size:
        out += hashlib.sha256(seed + ctr.to_bytes(8, "little")).digest()
        ctr += 1
    return out[:size]


class Suite:
    """Tiny, Thin and Pedersen provers over: the suite id, the group order, generator and blinding base, the group's addition, the point
    codec (`encode`) and encode-to-curve (bytes -> point)."""

    def __init__(self, suite_id, order, generator, blinding, adder, encode_point, encode_to_curve):
        self.suite_id, self.n, self.g, self.bb = suite_id, order, generator, blinding
        self.add, self.enc, self.e2c = adder, encode_point, encode_to_curve

    def mul(self, k, pt):
        return mul(k % self.n, pt, self.add)

    def enc_scalar(self, k):
        return (k % self.n).to_bytes(32, "little")

    def nonce(self, secret, transcript):
        expanded = squeeze(transcript + b"\x10" + self.enc_scalar(secret), 64)
        return le(squeeze(transcript + b"\x11" + expanded, 48)) % self.n

    def challenge(self, points, transcript):
        return le(squeeze(transcript + b"\x40" + b"".join(self.enc(p) for p in points), 16)) % self.n

    def statement(self, scheme, ios, ad):
        t = self.suite_id + bytes([scheme]) + len(ios).to_bytes(8, "little") + b"".join(self.enc(i) + self.enc(o) for i, o in ios)
        t += len(ad).to_bytes(8, "little") + ad
        stream = squeeze(t + b"\x30", 16 * (len(ios) - 1)) if len(ios) > 1 else b""
        return t, [1] + [le(stream[16 * j : 16 * j + 16]) % self.n for j in range(len(ios) - 1)]

    def point_to_hash(self, pt):
        return squeeze(self.suite_id + b"\x20" + self.enc(pt), 32)

    def ietf_prove(self, sk, alpha, ad, thin=False, salt=b""):
        """Tiny (O || c || s, 81 bytes) or Thin (O || R || s, 98 bytes)"""
        x = le(sk) % self.n
        i_pt = self.e2c(salt + alpha)
        pk, out = self.mul(x, self.g), self.mul(x, i_pt)
        t, zs = self.statement(1 if thin else 0, [(self.g, pk), (i_pt, out)], ad)
        m = self.add(self.g, self.mul(zs[1], i_pt))
        k = self.nonce(x, t)
        r = self.mul(k, m)
        c = self.challenge([r], t)
        s = (k + c * x) % self.n
        if thin:
            return self.enc(out) + self.enc(r) + self.enc_scalar(s)
        return self.enc(out) + c.to_bytes(16, "little") + self.enc_scalar(s)

    def pedersen_prove(self, sk, alpha, ad, salt=b""):
        """(proof O || Y_bar || R || O_k || s || s_b, 196 bytes; blinding factor)"""
        x = le(sk) % self.n
        i_pt = self.e2c(salt + alpha)
        out = self.mul(x, i_pt)
        t, _ = self.statement(2, [(i_pt, out)], ad)
        b = self.nonce(x, t + b"\x12")
        ybar = self.add(self.mul(x, self.g), self.mul(b, self.bb))
        t += self.enc(ybar)
        k, kb = self.nonce(x, t), self.nonce(b, t)
        r, ok = self.add(self.mul(k, self.g), self.mul(kb, self.bb)), self.mul(k, i_pt)
        c = self.challenge([r, ok], t)
        proof = self.enc(out) + self.enc(ybar) + self.enc(r) + self.enc(ok) + self.enc_scalar(k + c * x) + self.enc_scalar(kb + c * b)
        return proof, b


RO = Suite(SUITE_ID, N, G, BLINDING, add, encode, encode_to_curve_ro)
NU = Suite(SUITE_ID, N, G, BLINDING, add, encode, encode_to_curve_nu)
