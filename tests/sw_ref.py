"""Big-integer restatement of the Bandersnatch_SW suite's boundary (dot_ring/curve/specs/bandersnatch_sw.py,
short_weierstrass/sw_affine_point.py, ring_proof/ring_curve.py, curve/point.py:252-296): affine law, 33-byte codec, the
SW <-> twisted Edwards maps and try-and-increment.  The identity is None."""
import hashlib

P = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
N = 0x1CFB69D4CA675F520CCE760202687600FF8F87007419047174FD06B52876E7E1
A = 10773120815616481058602537765553212789256758185246796157495669123169359657269
B = 29569587568322301171008055308580903175558631321415017492731745847794083609535
G = (30900340493481298850216505686589334086208278925799850409469406976849338430199,
     12663882780877899054958035777720958383845500985908634476792678820121468453298)
BLINDING = (28115362618644671219696075022370511395136332234538034358311199318506963235315,
            3900851469868158154936962463930962496000252801946757953905982128670530185313)
MB = 25465760566081946422412445027709227188579564747101592991722834452325077642517
A3 = 9992940898322946442093665462003920523391277922024982836398934612730118446984
TE_A, TE_D = -5, 0x6389C12633C267CBC66E3BF86BE3B6D8CB66677177E54F92B369F2F5188D58E7
SUITE_ID = b"Bandersnatch-SW-SHA512-TAI-v1"


def sqrt(v):
    """a square root of v mod P, or None (Tonelli-Shanks)"""
    v %= P
    if v == 0:
        return 0
    if pow(v, (P - 1) // 2, P) != 1:
        return None
    q, s = P - 1, 0
    while q % 2 == 0:
        q, s = q // 2, s + 1
    z = 5
    m, c, t, r = s, pow(z, q, P), pow(v, q, P), pow(v, (q + 1) // 2, P)
    while t != 1:
        i, t2 = 0, t
        while t2 != 1:
            t2, i = t2 * t2 % P, i + 1
        b = pow(c, 1 << (m - i - 1), P)
        m, c, t, r = i, b * b % P, t * b * b % P, r * b % P
    return r


def on_curve(pt):
    return pt is None or (pt[1] * pt[1] - pt[0] ** 3 - A * pt[0] - B) % P == 0


def add(p1, p2):
    if p1 is None:
        return p2
    if p2 is None:
        return p1
    if p1[0] == p2[0]:
        return double(p1) if p1[1] == p2[1] else None
    lam = (p2[1] - p1[1]) * pow(p2[0] - p1[0], -1, P) % P
    x3 = (lam * lam - p1[0] - p2[0]) % P
    return x3, (lam * (p1[0] - x3) - p1[1]) % P


def double(pt):
    if pt is None or pt[1] == 0:
        return None
    lam = (3 * pt[0] * pt[0] + A) * pow(2 * pt[1], -1, P) % P
    x3 = (lam * lam - 2 * pt[0]) % P
    return x3, (lam * (pt[0] - x3) - pt[1]) % P


def mul(k, pt):
    acc = None
    for bit in bin(k)[2:] if k > 0 else "":
        acc = double(acc)
        if bit == "1":
            acc = add(acc, pt)
    return acc


def raw(pt):
    """the ABI's 64-byte record: x || y little-endian, 64 zero bytes for the identity"""
    return bytes(64) if pt is None else pt[0].to_bytes(32, "little") + pt[1].to_bytes(32, "little")


def encode(pt):
    if pt is None:
        return bytes(32) + b"\x40"
    return pt[0].to_bytes(32, "little") + (b"\x00" if pt[1] <= -pt[1] % P else b"\x80")


def decode(data, subgroup=True):
    """the point, or None for every encoding the reference rejects"""
    x, flag = int.from_bytes(data[:32], "little"), data[32]
    if flag & 0x7F or x >= P:
        return None
    y = sqrt(x ** 3 + A * x + B)
    if not y:
        return None
    small, large = sorted((y, -y % P))
    pt = (x, large if flag & 0x80 else small)
    if subgroup and (mul(4, pt) is None or mul(N, pt) is not None):
        return None
    return pt


def to_te(pt):
    if pt is None:
        return 0, 1
    s, t = (MB * pt[0] - A3) % P, MB * pt[1] % P
    return s * pow(t, -1, P) % P, (s - 1) * pow(s + 1, -1, P) % P


def from_te(pt):
    v, w = pt
    if (v, w) == (0, 1):
        return None
    s = (1 + w) * pow(1 - w, -1, P) % P
    t = s * pow(v, -1, P) % P
    return (s + A3) * pow(MB, -1, P) % P, t * pow(MB, -1, P) % P


def te_add(p1, p2):
    (x1, y1), (x2, y2) = p1, p2
    t = TE_D * x1 * x2 * y1 * y2 % P
    return (x1 * y2 + x2 * y1) * pow(1 + t, -1, P) % P, (y1 * y2 - TE_A * x1 * x2) * pow(1 - t, -1, P) % P


def te_mul(k, pt):
    acc = (0, 1)
    for bit in bin(k)[2:]:
        acc = te_add(acc, acc)
        if bit == "1":
            acc = te_add(acc, pt)
    return acc


def _squeeze(absorbed, size):
    seed, out, ctr = hashlib.sha512(absorbed).digest(), b"", 0
    while len(out) < size:
        out += hashlib.sha512(seed + ctr.to_bytes(8, "little")).digest()
        ctr += 1
    return out[:size]


def encode_to_curve(data):
    """(point, counter) of try-and-increment for salt || alpha = data"""
    prefix = SUITE_ID + b"\x60" + len(data).to_bytes(8, "little") + data
    for counter in range(256):
        cand = bytearray(_squeeze(prefix + bytes([counter]), 32))
        cand[31] &= 0x7F
        pt = decode(bytes(cand) + b"\x80", subgroup=False)
        if pt is None:
            continue
        pt = mul(4, pt)
        if pt is not None:
            return pt, counter
    raise ValueError("hash_to_curve_tai failed")
