"""Big-integer restatement of the Ed25519 suite (dot_ring/curve/specs/ed25519.py, Ed25519_TAI variant) as the reference runs it:
the twisted Edwards law with a = -1 over 2^255 - 19, the 32-byte codec with the reference's sign rule (x > p - x, point.py:150-214,
not RFC 8032's parity), its decoding rules (te_affine_point.py:297-316 and the point constructor), try-and-increment
(point.py:252-296) and the Tiny, Thin and Pedersen provers (vrf/ietf/tiny.py, thin.py, pedersen/vrf.py, primitives.py).
Points are (x, y) tuples; the identity is (0, 1)."""
import hashlib

P = 2**255 - 19
N = 2**252 + 0x14DEF9DEA2F79CD65812631A5CF5D3ED
H = 8
A = -1
D = 0x52036CEE2B6FFE738CC740797779E89800700A4D4141D8AB75EB4DCA135978A3
G = (0x216936D3CD6E53FEC0A4E231FDD6DC5C692CC7609525A7B2C9562D608F25D51A,
     0x6666666666666666666666666666666666666666666666666666666666666658)
BLINDING = (45003173884697328536089278691112838614164406922820087464913813433380838325453,
            31256014272390301975555524011230972931324093235775711248505761870355310252869)
SUITE_ID = b"Ed25519-SHA512-TAI-v1"
O = (0, 1)
SQRT_M1 = pow(2, (P - 1) // 4, P)


def sqrt(v):
    """a square root of v mod P, or None"""
    v %= P
    r = pow(v, (P + 3) // 8, P)
    if r * r % P != v:
        r = r * SQRT_M1 % P
    return r if r * r % P == v else None


def on_curve(pt):
    x, y = pt
    return (A * x * x + y * y - 1 - D * x * x * y * y) % P == 0


def add(p1, p2):
    (x1, y1), (x2, y2) = p1, p2
    t = D * x1 * x2 * y1 * y2 % P
    return (x1 * y2 + x2 * y1) * pow(1 + t, -1, P) % P, (y1 * y2 - A * x1 * x2) * pow(1 - t, -1, P) % P


def neg(pt):
    return -pt[0] % P, pt[1]


def mul(k, pt):
    acc = O
    for bit in bin(k)[2:] if k > 0 else "":
        acc = add(acc, acc)
        if bit == "1":
            acc = add(acc, pt)
    return acc


def msm(pts, ks):
    acc = O
    for pt, k in zip(pts, ks):
        acc = add(acc, mul(k % N, pt))
    return acc


def raw(pt):
    return pt[0].to_bytes(32, "little") + pt[1].to_bytes(32, "little")


def encode(pt):
    out = bytearray(pt[1].to_bytes(32, "little"))
    if pt[0] > -pt[0] % P:
        out[31] |= 0x80
    return bytes(out)


def encode_parity(pt):
    """RFC 8032's rule (the low bit of x), for the cases where the two differ"""
    out = bytearray(pt[1].to_bytes(32, "little"))
    out[31] |= (pt[0] & 1) << 7
    return bytes(out)


def decode(data, check=True):
    """the point, or None for what the reference refuses: y >= p, no root; with check, also the identity and any point with a
    torsion component (not in the prime-order subgroup).  x = 0 ignores the sign bit (both candidates are 0)."""
    sign = data[31] >> 7
    y = int.from_bytes(data[:31] + bytes([data[31] & 0x7F]), "little")
    if y >= P:
        return None
    den = (A - D * y * y) % P
    if den == 0:
        return None
    x = sqrt((1 - y * y) * pow(den, -1, P))
    if x is None:
        return None
    lo, hi = sorted((x, -x % P))
    pt = (hi if sign else lo, y)
    if check and (mul(H, pt) == O or mul(N, pt) != O):
        return None
    return pt


def torsion_points():
    """the 8 points of order dividing 8: the multiples of l Q for a point Q whose l Q has order 8"""
    y = 2
    while True:
        q = decode(y.to_bytes(32, "little"), check=False)
        if q is not None:
            t = mul(N, q)
            if mul(4, t) != O:
                return [mul(j, t) for j in range(8)]
        y += 1


# ---------------------------------------------------------------- transcripts (primitives.py), SHA-512 counter mode
def squeeze(absorbed, size):
    seed, out, ctr = hashlib.sha512(absorbed).digest(), b"", 0
    while len(out) < size:
        out += hashlib.sha512(seed + ctr.to_bytes(8, "little")).digest()
        ctr += 1
    return out[:size]


def enc_scalar(k):
    return (k % N).to_bytes(32, "little")


def le(b):
    return int.from_bytes(b, "little")


def encode_to_curve(data):
    """(point, counter): the candidate is the 32 squeezed bytes as they are (bit 255 cleared, then the same sign put back)"""
    prefix = SUITE_ID + b"\x60" + len(data).to_bytes(8, "little") + data
    for counter in range(256):
        pt = decode(squeeze(prefix + bytes([counter]), 32), check=False)
        if pt is None:
            continue
        pt = mul(H, pt)
        if pt != O:
            return pt, counter
    raise ValueError("hash_to_curve_tai failed")


def nonce(secret, transcript):
    expanded = squeeze(transcript + b"\x10" + enc_scalar(secret), 64)
    return le(squeeze(transcript + b"\x11" + expanded, 48)) % N


def challenge(points, transcript):
    return le(squeeze(transcript + b"\x40" + b"".join(encode(p) for p in points), 16)) % N


def statement(scheme, ios, ad):
    """(transcript bytes, delinearisation weights)"""
    t = SUITE_ID + bytes([scheme]) + len(ios).to_bytes(8, "little") + b"".join(encode(i) + encode(o) for i, o in ios)
    t += len(ad).to_bytes(8, "little") + ad
    stream = squeeze(t + b"\x30", 16 * (len(ios) - 1)) if len(ios) > 1 else b""
    return t, [1] + [le(stream[16 * j : 16 * j + 16]) % N for j in range(len(ios) - 1)]


def point_to_hash(pt, mul_cofactor=False):
    if mul_cofactor:
        pt = mul(H, pt)
    return squeeze(SUITE_ID + b"\x20" + encode(pt), 32)


def ietf_prove(sk, alpha, ad, thin=False, salt=b""):
    """Tiny (O || c || s, 80 bytes) or Thin (O || R || s, 96 bytes)"""
    x = le(sk) % N
    i_pt, _ = encode_to_curve(salt + alpha)
    pk, out = mul(x, G), mul(x, i_pt)
    t, zs = statement(1 if thin else 0, [(G, pk), (i_pt, out)], ad)
    m = add(G, mul(zs[1], i_pt))
    k = nonce(x, t)
    r = mul(k, m)
    c = challenge([r], t)
    s = (k + c * x) % N
    if thin:
        return encode(out) + encode(r) + enc_scalar(s)
    return encode(out) + c.to_bytes(16, "little") + enc_scalar(s)


def pedersen_prove(sk, alpha, ad, salt=b""):
    """(proof O || Y_bar || R || O_k || s || s_b, blinding factor)"""
    x = le(sk) % N
    i_pt, _ = encode_to_curve(salt + alpha)
    out = mul(x, i_pt)
    t, _ = statement(2, [(i_pt, out)], ad)
    b = nonce(x, t + b"\x12")
    ybar = add(mul(x, G), mul(b, BLINDING))
    t += encode(ybar)
    k, kb = nonce(x, t), nonce(b, t)
    r, ok = add(mul(k, G), mul(kb, BLINDING)), mul(k, i_pt)
    c = challenge([r, ok], t)
    proof = encode(out) + encode(ybar) + encode(r) + encode(ok) + enc_scalar(k + c * x) + enc_scalar(kb + c * b)
    return proof, b
