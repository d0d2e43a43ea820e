"""Big-integer restatement of the Baby JubJub suite (dot_ring/curve/specs/baby_jubjub.py) as the reference runs it: the twisted
Edwards law with a = 1 over the BN254 scalar field, the 32-byte codec with the reference's sign rule (x > p - x, point.py:150-214),
its decoding rules (te_affine_point.py:297-316 and the point constructor), try-and-increment with the candidate masked to the field's
254 bits (point.py:252-296) and the Tiny, Thin and Pedersen provers (vrf/ietf/tiny.py, thin.py, pedersen/vrf.py, primitives.py).
Points are (x, y) tuples; the identity is (0, 1)."""
import hashlib

P = 21888242871839275222246405745257275088548364400416034343698204186575808495617
N = 2736030358979909402780800718157159386076813972158567259200215660948447373041
H = 8
A = 1
D = 9706598848417545097372247223557719406784115219466060233080913168975159366771
G = (19698561148652590122159747500897617769866003486955115824547446575314762165298,
     19298250018296453272277890825869354524455968081175474282777126169995084727839)
BLINDING = (15549380791300914366206471199568039679131690710803662429646809536753521087193,
            15218614024055502695611547593111691164731001864276292210438920202280814188379)
ACCUMULATOR = (6402374321243162085389111671722843560682527921646684137786768606010797479351,
               9735581299071570006712034490635195155689931359428941496570758703259384062170)
PADDING = (11167490195257431015694161063225325511805242064780376648595733691987293447528,
           18403369502642103292159933062507105566469227524991433735553439433605496057425)
SUITE_ID = b"BabyJubJub-SHA512-TAI-v1"
O = (0, 1)
S = 28                                   # p - 1 = Q 2^S
Q = (P - 1) >> S
NONRESIDUE = 5


def is_square(v):
    v %= P
    return v == 0 or pow(v, (P - 1) // 2, P) == 1


def sqrt(v):
    """a square root of v mod P by Tonelli-Shanks, or None"""
    v %= P
    if v == 0:
        return 0
    if not is_square(v):
        return None
    m, c, t, r = S, pow(NONRESIDUE, Q, P), pow(v, Q, P), pow(v, (Q + 1) // 2, P)
    while t != 1:
        i, t2 = 1, t * t % P
        while t2 != 1:
            i, t2 = i + 1, t2 * t2 % P
        b = pow(c, 1 << (m - i - 1), P)
        m, c, t, r = i, b * b % P, t * b * b % P, r * b % P
    return r


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


def mask_candidate(cand, masked=True):
    """point.py:282-287, the TE branch: keep the sign (bit 7 of byte 31), clear the bits above the field's bit length (here bit 6),
    put the sign back"""
    if not masked:
        return cand
    out = bytearray(cand)
    shave = 8 * len(out) - P.bit_length()
    sign = out[-1] & 0x80
    out[-1] &= (1 << (8 - shave)) - 1
    out[-1] |= sign
    return bytes(out)


def encode_to_curve(data, masked=True):
    """(point, counter).  masked=False runs the loop on the unmasked candidates (what a suite with shave = 0 would do), to show where
    the mask matters."""
    prefix = SUITE_ID + b"\x60" + len(data).to_bytes(8, "little") + data
    for counter in range(256):
        pt = decode(mask_candidate(squeeze(prefix + bytes([counter]), 32), masked), check=False)
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
