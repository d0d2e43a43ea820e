"""Big-integer restatement of the P-256 suite (dot_ring/curve/specs/p256.py, the P256_TAI variant) as the reference runs it: the short
Weierstrass law with a = -3, the 33-byte codec (x little-endian, then a flag byte: bit 7 = y > p - y, bit 6 = infinity, bits 0..5
must be clear), the SEC1 fallback for strings that start with 0x02 / 0x03 (x = the big-endian bytes 1..32, y of that parity),
try-and-increment with SHA-256 (point.py:252-296: 32 squeezed bytes and the flag 0x80) and the Tiny, Thin and Pedersen provers
(vrf/ietf/tiny.py, thin.py, pedersen/vrf.py, primitives.py).  Points are (x, y) tuples; the identity is None."""
import hashlib

P = 2**256 - 2**224 + 2**192 + 2**96 - 1
N = 0xFFFFFFFF00000000FFFFFFFFFFFFFFFFBCE6FAADA7179E84F3B9CAC2FC632551
H = 1
A = -3
B = 0x5AC635D8AA3A93E7B3EBBD55769886BC651D06B0CC53B0F63BCE3C3E27D2604B
G = (0x6B17D1F2E12C4247F8BCE6E563A440F277037D812DEB33A0F4A13945D898C296,
     0x4FE342E2FE1A7F9B8EE7EB4A7C0F9E162BCE33576B315ECECBB6406837BF51F5)
BLINDING = (100063053743935619201936855760019111820847755970243670581468062459849338000,
            113675507039234898358330549589155441528265243038226986303017485279501143145422)
SUITE_ID = b"Secp256r1-SHA256-TAI-v1"
O = None


def sqrt(v):
    """a square root of v mod P (p = 3 mod 4), or None"""
    v %= P
    r = pow(v, (P + 1) // 4, P)
    return r if r * r % P == v else None


def rhs(x):
    return (x * x * x + A * x + B) % P


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
    acc = None
    for bit in bin(k)[2:] if k > 0 else "":
        acc = add(acc, acc)
        if bit == "1":
            acc = add(acc, pt)
    return acc


def msm(pts, ks):
    acc = None
    for pt, k in zip(pts, ks):
        acc = add(acc, mul(k % N, pt))
    return acc


def raw(pt):
    """the ABI's affine x || y; the identity is 64 zero bytes"""
    return bytes(64) if pt is None else pt[0].to_bytes(32, "little") + pt[1].to_bytes(32, "little")


def encode(pt):
    if pt is None:
        return bytes(32) + b"\x40"
    return pt[0].to_bytes(32, "little") + (b"\x80" if pt[1] > -pt[1] % P else b"\x00")


def _canonical(data):
    flag = data[32]
    if flag & 0x3F:
        return "bad"
    if flag & 0x40:
        return O if not (flag & 0x80) and not any(data[:32]) else "bad"
    x = int.from_bytes(data[:32], "little")
    if x >= P:
        return "bad"
    y = sqrt(rhs(x))
    if y is None:
        return "bad"
    small, large = sorted((y, -y % P))
    return x, large if flag & 0x80 else small


def _sec1(data):
    x = int.from_bytes(data[1:33], "big")
    if x >= P:
        return "bad"
    y = sqrt(rhs(x))
    if y is None:
        return "bad"
    if y % 2 != data[0] % 2:
        y = P - y
    return x, y


def decode(data, check=True):
    """string_to_point (with the SEC1 fallback for a first byte 0x02 / 0x03), then with check dec_point's valid_point: not the
    identity.  'bad' for what the reference refuses."""
    assert len(data) == 33
    pt = _canonical(data)
    if pt == "bad" and data[0] in (2, 3):
        pt = _sec1(data)
    if pt != "bad" and check and pt is None:
        return "bad"
    return pt


def decoded_by_fallback(data):
    return data[0] in (2, 3) and _canonical(data) == "bad" and _sec1(data) != "bad"


# ---------------------------------------------------------------- transcripts (primitives.py), SHA-256 counter mode
def squeeze(absorbed, size):
    seed, out, ctr = hashlib.sha256(absorbed).digest(), b"", 0
    while len(out) < size:
        out += hashlib.sha256(seed + ctr.to_bytes(8, "little")).digest()
        ctr += 1
    return out[:size]


def enc_scalar(k):
    return (k % N).to_bytes(32, "little")


def le(b):
    return int.from_bytes(b, "little")


def tai_candidate(data, counter):
    prefix = SUITE_ID + b"\x60" + len(data).to_bytes(8, "little") + data
    return squeeze(prefix + bytes([counter]), 32) + b"\x80"


def encode_to_curve(data):
    """(point, counter, by_fallback): the first candidate that decodes (cofactor 1: nothing to clear)"""
    for counter in range(256):
        cand = tai_candidate(data, counter)
        pt = decode(cand, check=False)
        if pt != "bad" and pt is not None:
            return pt, counter, decoded_by_fallback(cand)
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


def point_to_hash(pt):
    return squeeze(SUITE_ID + b"\x20" + encode(pt), 32)


def ietf_prove(sk, alpha, ad, thin=False, salt=b""):
    """Tiny (O || c || s, 81 bytes) or Thin (O || R || s, 98 bytes)"""
    x = le(sk) % N
    i_pt, _, _ = encode_to_curve(salt + alpha)
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
    """(proof O || Y_bar || R || O_k || s || s_b, 196 bytes; blinding factor)"""
    x = le(sk) % N
    i_pt, _, _ = encode_to_curve(salt + alpha)
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
