"""Big-integer restatement of Curve25519_RO / Curve25519_NU (dot_ring/curve/specs/curve25519.py over montgomery/mg_affine_point.py),
written from the reference's behaviour:

  group    v^2 = u^3 + 486662 u^2 + u over 2^255 - 19 with the reference's affine chord-and-tangent law: the identity is None, a doubling
           with v = 0 and a vertical chord give the identity.
  hashing  expand_message_xmd over SHA-512 (Z_pad of 128 bytes) with the DST QUUX-V01-CS02-with- || suite id (_RO_ replaced by _NU_ for
           the nonuniform variant: both share one params object, so the suite id stays the RO one), Elligator 2 (h2c_ref.ell2_mont: the
           map the Ed25519 variants run before their change of model; it has no failing inverse), the sum of two images for RO, times 8.
  codec    u || v, 32 little-endian bytes each; the identity has no encoding; decoding checks the ranges and the curve equation only.

The Tiny / Thin / Pedersen layer is h2c_ref.Suite, the generic layer that reproduces all of the reference's Ed25519 and P-256 proof files
(test_h2c_suites_cpu.py): the reference holds no proof vectors for this curve, so the Curve25519 proof bytes rest on that layer.
Points are (u, v) tuples; `to_edwards` / `from_edwards` are the birational map the kernels compute through (ed25519_ref's (x, y))."""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ed25519_ref as ed  # noqa: E402
import h2c_ref as h  # noqa: E402

P, N, H = ed.P, ed.N, 8
A = h.MONT_A
G = (9, 14781619447589544791020593568409986887264606134616475288964881837755586237401)
BLINDING = G
SUITE_ID = b"curve25519_XMD:SHA-512_ELL2_RO_"
DST_RO = b"QUUX-V01-CS02-with-" + SUITE_ID
DST_NU = DST_RO.replace(b"_RO_", b"_NU_")
O = None
TWO_TORSION = (0, 0)
C = h.SQRT_NEG_A_MINUS_2          # sqrt(-486664): the factor of the birational map (either root serves, used in both directions)


def on_curve(pt):
    return pt is None or (pt[1] * pt[1] - ((pt[0] + A) * pt[0] + 1) * pt[0]) % P == 0


def add(p1, p2):
    """MGAffinePoint.__add__ with B = 1"""
    if p1 is None:
        return p2
    if p2 is None:
        return p1
    (x1, y1), (x2, y2) = p1, p2
    if x1 == x2 and y1 == y2:
        if y1 == 0:
            return None
        lam = (3 * x1 * x1 + 2 * A * x1 + 1) * pow(2 * y1, -1, P) % P
    elif x1 == x2:
        return None
    else:
        lam = (y2 - y1) * pow(x2 - x1, -1, P) % P
    x3 = (lam * lam - A - x1 - x2) % P
    return x3, (lam * (x1 - x3) - y1) % P


def neg(pt):
    return None if pt is None else (pt[0], -pt[1] % P)


def mul(k, pt):
    """k pt for any k >= 0 (not reduced: small-order points), double-and-add as the reference's"""
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


# ---------------------------------------------------------------- the birational map to Ed25519
def to_edwards(pt):
    if pt is None:
        return ed.O
    if pt == TWO_TORSION:
        return (0, P - 1)
    u, v = pt
    return C * u * pow(v, -1, P) % P, (u - 1) * pow(u + 1, -1, P) % P


def from_edwards(pt):
    if pt == ed.O:
        return None
    if pt == (0, P - 1):
        return TWO_TORSION
    x, y = pt
    u = (1 + y) * pow(1 - y, -1, P) % P
    return u, C * u * pow(x, -1, P) % P


def torsion_points():
    """the 8 points of order dividing 8 (None among them), through ed25519_ref's"""
    return [from_edwards(t) for t in ed.torsion_points()]


# ---------------------------------------------------------------- codec (mg_affine_point.py:348-389)
def raw(pt):
    return pt[0].to_bytes(32, "little") + pt[1].to_bytes(32, "little")


def encode(pt):
    if pt is None:
        raise ValueError("Cannot serialize point at infinity")
    return raw(pt)


def decode(data, check=False):
    """string_to_point for 64 bytes; check: also curve.valid_point (a non-identity point of the prime-order subgroup); 'bad' otherwise"""
    if len(data) != 64:
        return "bad"
    pt = (int.from_bytes(data[:32], "little"), int.from_bytes(data[32:], "little"))
    if pt[0] >= P or pt[1] >= P or not on_curve(pt):
        return "bad"
    if check:
        cleared = mul(H, pt)
        if cleared is None or mul(pow(H, -1, N), cleared) != pt:
            return "bad"
    return pt


# ---------------------------------------------------------------- hashing to the curve
def hash_to_field(msg, count, dst):
    return h.ed_hash_to_field(msg, count, dst)


def map_to_curve(u):
    """MGAffinePoint.map_to_curve: one image, the cofactor not cleared"""
    pt = h.ell2_mont(u)
    assert on_curve(pt)
    return pt


def encode_to_curve_ro(data):
    u0, u1 = hash_to_field(data, 2, DST_RO)
    return mul(H, add(map_to_curve(u0), map_to_curve(u1)))


def encode_to_curve_nu(data):
    (u,) = hash_to_field(data, 1, DST_NU)
    return mul(H, map_to_curve(u))


# ---------------------------------------------------------------- the VRF layer: h2c_ref's generic one
def _suite(e2c):
    return h.Suite(SUITE_ID, N, G, BLINDING, add, encode, e2c, hashlib.sha512, identity=None)


RO = _suite(encode_to_curve_ro)
NU = _suite(encode_to_curve_nu)


def ietf_verify(suite, pk, proof, alpha, ad, thin=False, salt=b""):
    """TinyVRF.verify / ThinVRF.verify of a 112- / 160-byte proof under the 64-byte public key"""
    pk_pt, out = decode(pk, check=True), decode(proof[:64], check=True)
    if pk_pt == "bad" or out == "bad":
        return False
    s = int.from_bytes(proof[-32:], "little")
    i_pt = suite.e2c(salt + alpha)
    t, zs = suite.statement(1 if thin else 0, [(suite.g, pk_pt), (i_pt, out)], ad)
    m_in, m_out = add(suite.g, suite.mul(zs[1], i_pt)), add(pk_pt, suite.mul(zs[1], out))
    if thin:
        r = decode(proof[64:128], check=True)
        if r == "bad":
            return False
        c = suite.challenge([r], t)
        return add(suite.mul(s, m_in), neg(suite.mul(c, m_out))) == r
    c = int.from_bytes(proof[64:80], "little")
    r = add(suite.mul(s, m_in), neg(suite.mul(c, m_out)))
    return r is not None and suite.challenge([r], t) == c


def pedersen_verify(suite, proof, alpha, ad, salt=b""):
    pts = [decode(proof[64 * i : 64 * i + 64], check=True) for i in range(4)]
    if "bad" in pts:
        return False
    out, ybar, r, ok = pts
    s, sb = int.from_bytes(proof[256:288], "little"), int.from_bytes(proof[288:], "little")
    i_pt = suite.e2c(salt + alpha)
    t, _ = suite.statement(2, [(i_pt, out)], ad)
    c = suite.challenge([r, ok], t + suite.enc(ybar))
    return (add(suite.mul(s, i_pt), neg(suite.mul(c, out))) == ok
            and add(add(suite.mul(s, suite.g), suite.mul(sb, suite.bb)), neg(suite.mul(c, ybar))) == r)
