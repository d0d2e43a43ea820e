"""Big-integer restatement of Curve448_RO / Curve448_NU (dot_ring/curve/specs/curve448.py over montgomery/mg_affine_point.py),
written from the reference's behaviour and RFC 9380 (section 5.3.3, expand_message_xof; section 6.7.2, Elligator 2):

  group    v^2 = u^3 + 156326 u^2 + u over p = 2^448 - 2^224 - 1 with the reference's affine chord-and-tangent law: the identity is
           None, a doubling with v = 0 and a vertical chord give the identity.  Order 4 n; (0, 0) has order 2, (-1, +-sqrt(A - 2))
           order 4.  `mul` does not reduce the scalar, as MGAffinePoint.__mul__ does not.
  hashing  expand_message_xof over SHAKE256 with L = 84 and the DST QUUX-V01-CS02-with- || suite id (_RO_ replaced by _NU_ for the
           nonuniform variant; the suite id stays the RO one), Elligator 2 with Z = -1 (ed448_ref.ell2_mont: the map Ed448 runs before
           its isogeny), the sum of two images for RO, times 4.  map_to_curve(u) for u in {1, p - 1} raises ValueError("No inverse
           exists"): the reference compares the reduced Z u^2 with -1, which never holds, and then inverts 0.  u = 0 maps to (0, 0).
  codec    u || v, 56 little-endian bytes each; the identity has no encoding; decoding checks the ranges and the curve equation only.

The Tiny / Thin / Pedersen layer is ed448_ref.XofSuite (h2c_ref.Suite with the XOF squeeze, the scalar width and the nonce width of
the order), which tests/test_ed448_cpu.py and tests/test_curve448_cpu.py pin on the reference's Bandersnatch SHAKE128 proof files.  The
challenge is 16 bytes as for every suite: the reference's VRF layer squeezes primitives.CHALLENGE_LEN = 16 bytes whatever
encoding.challenge_len (28 here, 64 for Ed448) says, so a Tiny proof is 112 + 16 + 56 = 184 bytes.
Points are (u, v) tuples; `to_inner` / `from_inner` are the birational map the kernels compute through (c448_law.hip.h)."""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ed448_ref as e4  # noqa: E402

P, N, H = e4.P, e4.N, 4
A = e4.MONT_A
G = (5, 355293926785568175264127502063783334808976399387714271831880898435169088786967410002932673765864550910142774147268105838985595290606362)
BLINDING = G
SUITE_ID = b"curve448_XOF:SHAKE256_ELL2_RO_"
DST_RO = b"QUUX-V01-CS02-with-" + SUITE_ID
DST_NU = DST_RO.replace(b"_RO_", b"_NU_")
O = None
TWO_TORSION = (0, 0)
INNER_A, INNER_D = A - 2, A + 2          # the inner Edwards curve a x^2 + y^2 = 1 + d x^2 y^2
INNER_O = (0, 1)


def sqrt(v):
    return e4.sqrt(v)


def is_square(v):
    return v % P == 0 or pow(v % P, (P - 1) // 2, P) == 1


T4 = (P - 1, sqrt(A - 2))                # a point of order 4 (the other is its negative)


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
    """k pt for any integer k (not reduced; a negative k negates the point), double-and-add as the reference's"""
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


# ---------------------------------------------------------------- the birational map to the inner Edwards curve
def to_inner(pt):
    if pt is None:
        return INNER_O
    if pt == TWO_TORSION:
        return (0, P - 1)
    u, v = pt
    return u * pow(v, -1, P) % P, (u + 1) * pow(u - 1, -1, P) % P


def from_inner(pt):
    if pt == INNER_O:
        return None
    if pt == (0, P - 1):
        return TWO_TORSION
    x, y = pt
    u = (y + 1) * pow(y - 1, -1, P) % P
    return u, u * pow(x, -1, P) % P


def inner_on_curve(pt):
    x, y = pt
    return (INNER_A * x * x + y * y - 1 - INNER_D * x * x % P * y * y) % P == 0


# ---------------------------------------------------------------- codec (mg_affine_point.py:348-389)
def raw(pt):
    return pt[0].to_bytes(56, "little") + pt[1].to_bytes(56, "little")


def encode(pt):
    if pt is None:
        raise ValueError("Cannot serialize point at infinity")
    return raw(pt)


def decode(data, check=False):
    """string_to_point for 112 bytes; check: also curve.valid_point (a non-identity point with n P = O); 'bad' otherwise"""
    if len(data) != 112:
        return "bad"
    pt = (int.from_bytes(data[:56], "little"), int.from_bytes(data[56:], "little"))
    if pt[0] >= P or pt[1] >= P or not on_curve(pt):
        return "bad"
    if check and mul(N, pt) is not None:
        return "bad"
    return pt


# ---------------------------------------------------------------- hashing to the curve
def hash_to_field(msg, count, dst):
    return e4.hash_to_field(msg, count, dst)


def map_to_curve(u):
    """MGAffinePoint.map_to_curve: one image, the cofactor not cleared"""
    u %= P
    if u * u % P == 1:
        raise ValueError("No inverse exists")          # mod_inverse(tv1 + 1) with tv1 = p - 1
    pt = e4.ell2_mont(u)
    assert on_curve(pt)
    return pt


def encode_to_curve_ro(data):
    u0, u1 = hash_to_field(data, 2, DST_RO)
    return mul(H, add(map_to_curve(u0), map_to_curve(u1)))


def encode_to_curve_nu(data):
    (u,) = hash_to_field(data, 1, DST_NU)
    return mul(H, map_to_curve(u))


# ---------------------------------------------------------------- the VRF layer: ed448_ref's XOF one
def _suite(e2c):
    return e4.XofSuite(SUITE_ID, N, G, BLINDING, add, encode, e2c, hashlib.shake_256, None)


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
    r = add(suite.mul(s, m_in), neg(suite.mul(c, m_out)))
    return r is not None and suite.challenge([r], t) == c


def pedersen_verify(suite, proof, alpha, ad, salt=b""):
    pts = [decode(proof[112 * i : 112 * i + 112], check=True) for i in range(4)]
    if "bad" in pts:
        return False
    out, ybar, r, ok = pts
    s, sb = int.from_bytes(proof[448:504], "little"), int.from_bytes(proof[504:], "little")
    i_pt = suite.e2c(salt + alpha)
    t, _ = suite.statement(2, [(i_pt, out)], ad)
    c = suite.challenge([r, ok], t + suite.enc(ybar))
    return (add(suite.mul(s, i_pt), neg(suite.mul(c, out))) == ok
            and add(add(suite.mul(s, suite.g), suite.mul(sb, suite.bb)), neg(suite.mul(c, ybar))) == r)
