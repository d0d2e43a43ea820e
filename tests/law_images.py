"""Lanes and a checker for the group laws of the nine wave curves on RAW limb images (csrc/wave_curve.hip.h, wave_law_selftest), shared
by tests/test_gpu_wave_laws.py (the device), tests/test_law_images_cpu.py (the builder and the checker themselves) and the host builds
of the laws under -fsanitize=undefined (tests/native/*_host_check.cpp, the `lane` line); for the law of Bandersnatch and JubJub over the
9 x 29-bit Fr (csrc/curve.hip.h and te_madd, dr_te_law_selftest: the same thirteen slots and four more, tests/test_gpu_te_law.py); and,
in the second half of the file, records and a checker for csrc/fr29.hip.h itself on raw limb images (dr_fr_raw_selftest,
tests/test_gpu_fr_raw.py, proven by tests/test_fr_images_cpu.py).

A lane is two real points P and Q of the curve, each coordinate a limb image at an edge of a class the law documents for it, and a
control word.  The classes are TRANSCRIBED from the headers (the citation stands beside each); nothing here is a measured number.  The
checker compares every slot the law returns with the curve's big-integer reference (tests/*_ref.py) by cross-multiplication, and asks
that every returned coordinate lies in the class the law documents for what it returns: the next mul, to_lds or shuffle relies on it.

An image of a residue v in a class: the target integer V = (v R mod p) + k p is written limb by limb from a CORNER of the class (every limb
at its upper bound, every limb at its lower bound, or the two alternating patterns) as corner -+ digit with digits in [0, 2^bits), the
top limb taking what is left.  Limbs below the top are then within one radix unit of their bound; k runs over the multiples of p for
which the top limb and the value stay inside the class, and the smallest and the largest are both used."""
import os
import random
import struct
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import babyjubjub_ref as bjj  # noqa: E402
import bls12_381_g1_ref as g1  # noqa: E402
import curve448_ref as c448  # noqa: E402
import ed25519_ref as e25  # noqa: E402
import ed448_ref as e448  # noqa: E402
import p256_ref as p256  # noqa: E402
import p384_ref as p384  # noqa: E402
import p521_ref as p521  # noqa: E402
import secp256k1_ref as k1  # noqa: E402

SLOTS = 13
TE_SLOTS = 17                # dr_te_law_selftest: the thirteen, then te_madd, te_madd four times, add of two law outputs, the endomorphism
SLOT_MADD, SLOT_MADD4, SLOT_ADD_OUT, SLOT_ENDO = 13, 14, 15, 16
ROW_NEGATED = 1 << 16        # the control bit that negates the row's x and dt limb-wise, as te_msm_walk does
SLOT_ADD, SLOT_SUB, SLOT_DBL, SLOT_DBL_NO_T, SLOT_NEG, SLOT_LDS, SLOT_KEEP, SLOT_CHAIN = 0, 1, 2, 3, 4, 5, 6, 7
WINDOWS = 6
CORNERS = ("hi", "lo", "alt0", "alt1")


class LimbClass:
    """limb l[i] in [lo[i], hi[i]] (inclusive) and, where the header bounds the value, vlo < value < vhi (vmax: |value| < vmax)"""

    def __init__(self, name, lo, hi, vmax=None, vlo=None, vhi=None):
        assert len(lo) == len(hi) and all(a <= b for a, b in zip(lo, hi))
        self.name, self.lo, self.hi = name, list(lo), list(hi)
        self.vlo, self.vhi = (-vmax, vmax) if vmax is not None else (vlo, vhi)

    def contains(self, image, bits):
        if len(image) != len(self.lo) or any(not (a <= x <= b) for x, a, b in zip(image, self.lo, self.hi)):
            return False
        v = value_of(image, bits)
        return (self.vlo is None or self.vlo < v) and (self.vhi is None or v < self.vhi)

    def negated(self):
        return LimbClass("-" + self.name, [-b for b in self.hi], [-a for a in self.lo], vlo=None if self.vhi is None else -self.vhi,
                         vhi=None if self.vlo is None else -self.vlo)

    def corner(self, which):
        if which == "hi":
            return list(self.hi)
        if which == "lo":
            return list(self.lo)
        odd = which == "alt1"
        return [(self.hi[i] if (i % 2 == 1) == odd else self.lo[i]) for i in range(len(self.lo))]


def value_of(image, bits):
    return sum(x << (bits * i) for i, x in enumerate(image))


def image_at(cls, which, target, bits):
    """the image of the integer `target` written from the corner `which` of cls, or None if the top limb or the value leaves the class"""
    corner = cls.corner(which)
    n, base = len(corner), 1 << bits
    d = target - value_of(corner, bits)
    image = []
    for i in range(n - 1):
        up = corner[i] == cls.lo[i]            # from a lower bound the digit is added, from an upper bound taken off
        digit = d % base if up else -d % base
        limb = corner[i] + digit if up else corner[i] - digit
        image.append(limb)
        d = (d - (limb - corner[i])) >> bits
    image.append(corner[n - 1] + d)
    assert value_of(image, bits) == target
    return image if cls.contains(image, bits) else None


def k_range(cls, which, residue, p, bits):
    """the smallest and the largest k for which residue + k p has an image at the corner"""
    vlo, vhi = value_of(cls.lo, bits), value_of(cls.hi, bits)
    if cls.vlo is not None:
        vlo = max(vlo, cls.vlo)
    if cls.vhi is not None:
        vhi = min(vhi, cls.vhi)
    kmin, kmax = (vlo - residue) // p - 1, (vhi - residue) // p + 1
    while kmin <= kmax and image_at(cls, which, residue + kmin * p, bits) is None:
        kmin += 1
    while kmax >= kmin and image_at(cls, which, residue + kmax * p, bits) is None:
        kmax -= 1
    assert kmin <= kmax, (cls.name, which)
    return kmin, kmax


def digits(v, limbs, bits):
    """the image of 0 <= v with limbs in [0, 2^bits), the top limb taking what is left"""
    return [(v >> (bits * i)) & ((1 << bits) - 1) if i < limbs - 1 else v >> (bits * i) for i in range(limbs)]


# ---------------------------------------------------------------- the curves
class Curve:
    """What the lanes and the checker need of a curve.
      ref              its tests/*_ref.py module; to_ref / from_ref map an inner affine point (x, y) (None: Z = 0) to the reference's and
                       back: the identity for all but Curve448, whose law runs on the Edwards curve E_M birational to it
      kind             "sw": identity (0 : Y : 0), cneg negates y;  "ed": identity (0 : Z : Z), cneg negates x (and t when extended)
      cls_p, cls_q     {coordinate: [classes]}: what the law documents for its first operand and the operand of dbl, and for the second
                       operand of add; the FIRST class of a negated coordinate is the one cneg negates (a table entry)
      p_neg, q_neg     whether P / Q may be handed over once negated
      cls_out          {coordinate: class} of what add, dbl and dbl_no_t return
      cls_lds          None where the table keeps limb images (from_lds gives back the very image), otherwise the class from_lds documents
      cneg_carries     cneg returns a carried coordinate (in cls_p's first class) instead of the limb-wise negation
      slots            how many slots a record returns; te_id: the curve id of dr_te_law_selftest, whose records carry a table row
                       (x2, y2, d x2 y2) in cls_lds' class and return slots 13 .. 16; endo: the scalar the endomorphism of slot 16
                       multiplies by (None: the slot is not written)
      lds_canonical    the LDS table keeps the canonical representative: slot 5 is slot 0's very value mod p, digit by digit
      no_t_zero        dbl_no_t returns the zero image as T"""

    def __init__(self, name, suite, limbs, bits, R, p, ref, kind, order, cls_p, cls_q, cls_out, one_image, specials, extended=False,
                 p_neg=True, q_neg=True, to_ref=None, from_ref=None, cneg_carries=False, cls_lds=None, slots=SLOTS, te_id=None, endo=None,
                 lds_canonical=False, no_t_zero=False, d=None):
        self.slots, self.te_id, self.endo, self.lds_canonical, self.no_t_zero, self.d = slots, te_id, endo, lds_canonical, no_t_zero, d
        self.name, self.suite, self.limbs, self.bits, self.R, self.p, self.ref = name, suite, limbs, bits, R % p, p, ref
        self.kind, self.order, self.extended = kind, order, extended
        self.cls_p, self.cls_q, self.cls_out, self.cls_lds = cls_p, cls_q, cls_out, cls_lds
        self.p_neg, self.q_neg, self.cneg_carries = p_neg, q_neg, cneg_carries
        self.one_image, self.specials = one_image, specials
        self.to_ref = to_ref or (lambda pt: pt)
        self.from_ref = from_ref or (lambda pt: pt)
        self.coords = ("x", "y", "z", "t") if extended else ("x", "y", "z")
        self.neg_coords = ("y",) if kind == "sw" else (("x", "t") if extended else ("x",))
        self.r_inv = pow(self.R, -1, p)

    # inner affine points: None is the identity of a Weierstrass curve; an Edwards curve has (0, 1)
    def identity(self):
        return None if self.kind == "sw" else (0, 1)

    def add(self, a, b):
        return self.from_ref(self.ref.add(self.to_ref(a), self.to_ref(b)))

    def neg(self, a):
        return self.from_ref(self.ref.neg(self.to_ref(a)))

    def lift(self, pt, scale):
        """projective (extended: with T = X Y / Z) coordinates, residues mod p, of an inner affine point under a non-zero scale"""
        p = self.p
        r = {"x": 0, "y": scale % p, "z": 0} if pt is None else {"x": pt[0] * scale % p, "y": pt[1] * scale % p, "z": scale % p}
        if self.extended:
            r["t"] = pt[0] * pt[1] * scale % p
        return r

    def same_point(self, xyz, pt, with_t=True):
        """whether the projective residues are the inner affine point, by cross-multiplication; the identity by the curve's own form;
        for extended points also T Z = X Y"""
        p = self.p
        X, Y, Z = (xyz[c] % p for c in "xyz")
        if self.extended and with_t and (xyz["t"] * Z - X * Y) % p:
            return False
        if pt is None:
            return Z == 0 and X == 0 and Y != 0
        if Z == 0:
            return False
        if self.kind == "ed" and pt == (0, 1):
            return X == 0 and Y == Z
        return (X - pt[0] * Z) % p == 0 and (Y - pt[1] * Z) % p == 0

    def residue(self, image):
        """the field element an image stands for"""
        return value_of(image, self.bits) * self.r_inv % self.p

    def random_point(self, rng):
        return self.from_ref(self.ref.mul(rng.randrange(1, self.order), self.ref.G))


def _all(cls, coords="xyz"):
    return {c: [cls] for c in coords}


def _x0_points(ref):
    """the points with x = 0 of a Weierstrass curve y^2 = x^3 + a x + b, if b is a square"""
    y = ref.sqrt(ref.B)
    return [] if y is None else [(0, y), (0, ref.P - y)]


def _small_one(limbs):
    return [1] + [0] * (limbs - 1)


# ---- P-384 (fp384.hip.h, p384_law.hip.h over sw3_law.hip.h)
def _p384():
    # fp384.hip.h, "normal": limbs 0..12 in [-2^22, 2^28 + 2^22), limb 13 in (-2^21, 2^21), |value| < 2^385
    n = LimbClass("n", [-(1 << 22)] * 13 + [-(1 << 21) + 1], [(1 << 28) + (1 << 22) - 1] * 13 + [(1 << 21) - 1], 1 << 385)
    # fp384.hip.h, "k n" with k = 1: |limb| <= 2^28 + 2^22 for limbs 0..12, |limb 13| <= 2^21, |value| < 2^385
    m, t = (1 << 28) + (1 << 22), 1 << 21
    n1 = LimbClass("1 n", [-m] * 13 + [-t], [m] * 13 + [t], 1 << 385)
    # sw3_law.hip.h: "A point's coordinates are x: 1 n, y: n (1 n once negated), z: n, in and out"
    cls = {"x": [n1], "y": [n], "z": [n]}
    # F384::small(1) = R mod p in signed limbs (fp384.hip.h): 2^8 - 2^12 B + 2^20 B^3 + 2^24 B^4
    one = [0] * 14
    one[0], one[1], one[3], one[4] = 1 << 8, -(1 << 12), 1 << 20, 1 << 24
    return Curve("P-384", "p384", 14, 28, 1 << 392, p384.P, p384, "sw", p384.N, cls, cls, {"x": n1, "y": n, "z": n}, one, _x0_points(p384))


# ---- P-521 (fp521.hip.h, p521_law.hip.h over sw3_law.hip.h)
def _p521():
    # fp521.hip.h, "normal": limbs 0..17 in (-2^15, 2^28 + 2^15), limb 18 in [0, 2^17); the value has no bound of its own
    n = LimbClass("n", [-(1 << 15) + 1] * 18 + [0], [(1 << 28) + (1 << 15) - 1] * 18 + [(1 << 17) - 1])
    # fp521.hip.h, "k n" with k = 1: |limb| <= 2^28 + 2^15, EVERY limb
    m = (1 << 28) + (1 << 15)
    n1 = LimbClass("1 n", [-m] * 19, [m] * 19)
    # sw3_law.hip.h: "A point's coordinates are x: 1 n, y: n (1 n once negated), z: n, in and out"
    cls = {"x": [n1], "y": [n], "z": [n]}
    return Curve("P-521", "p521", 19, 28, 1, p521.P, p521, "sw", p521.N, cls, cls, {"x": n1, "y": n, "z": n}, _small_one(19), _x0_points(p521))


# ---- secp256k1 (fsecp256k1.hip.h, kernels_secp256k1.hip.h)
def _secp256k1():
    # fsecp256k1.hip.h, "normal": limbs 0, 1, 3..7 in [0, 2^29), limb 2 in (-2^15, 2^29 + 2^15), limb 8 in [0, 2^24)
    lo, hi = [0] * 9, [(1 << 29) - 1] * 8 + [(1 << 24) - 1]
    lo[2], hi[2] = -(1 << 15) + 1, (1 << 29) + (1 << 15) - 1
    n = LimbClass("n", lo, hi)
    # kernels_secp256k1.hip.h, k1_dbl and k1_add: "coordinates n in, n out"; k1_cneg carries what it negates ("r.y = carry(cneg(...))"), so
    # no coordinate is ever handed over negated
    return Curve("secp256k1", "secp256k1", 9, 29, 1, k1.P, k1, "sw", k1.N, _all(n), _all(n), {c: n for c in "xyz"}, _small_one(9), [],
                 p_neg=False, q_neg=False, cneg_carries=True)


# ---- P-256 (fp256.hip.h, kernels_p256.hip.h)
def _p256():
    p = p256.P
    # fp256.hip.h, "normal": limbs 0..7 in [0, 2^29), limb 8 in (-2^26, 2^26); |value| < 2^258
    n = LimbClass("n", [0] * 8 + [-(1 << 26) + 1], [(1 << 29) - 1] * 8 + [(1 << 26) - 1], 1 << 258)
    # fp256.hip.h, fp_reduce: "reduced": limbs 0..7 in (-2^27, 2^29 + 2^27), limb 8 in [0, 2^24), |value| < 2^256 + 2^231
    r = LimbClass("r", [-(1 << 27) + 1] * 8 + [0], [(1 << 29) + (1 << 27) - 1] * 8 + [(1 << 24) - 1], (1 << 256) + (1 << 231))
    # kernels_p256.hip.h, p256_dbl and p256_add: "coordinates n or r (y possibly negated by p256_cneg) in, n out"
    cls = {c: [n, r] for c in "xyz"}
    return Curve("P-256", "p256", 9, 29, 1 << 261, p, p256, "sw", p256.N, cls, cls, {c: n for c in "xyz"}, digits((1 << 261) % p, 9, 29), [])


# ---- BLS12-381 E(Fq) (fq28.hip.h, kernels_g1_h2c.hip.h)
def _blsg1():
    p = g1.P
    top = 3 * p // 2 >> 364
    # kernels_g1_h2c.hip.h: "cK = carried (limbs 0..12 in [0, 2^28), a small signed top limb) with |value| < K p.  A coordinate is c1.5";
    # the top limb is what the value leaves it
    c15 = LimbClass("c1.5", [0] * 13 + [-top - 1], [(1 << 28) - 1] * 13 + [top], (3 * p + 1) // 2)
    # "w = a wide product (limbs 0..12 in [0, 2^28), value in (-0.14 p, 1.14 p))"; the top limb is what the value leaves it
    n = LimbClass("w", [0] * 13 + [(-(14 * p // 100) - 1) >> 364], [(1 << 28) - 1] * 13 + [114 * p // 100 >> 364], vlo=-(14 * p // 100) - 1,
                  vhi=114 * p // 100 + 1)
    # g1h_dbl, g1h_add: "coordinates c1.5 in, w out"; g1h_cneg carries: "c1.5"
    # a point of E(Fq) outside G1: the first x from 1 with a root, which r does not kill
    x = 1
    while True:
        y = g1.sqrt((x**3 + g1.CURVE_B) % p)
        if y is not None and g1.mul(g1.R_ORDER, (x, y)) is not None:
            break
        x += 1
    outside = (x, y)
    return Curve("BLS12-381 E(Fq)", "blsg1", 14, 28, 1 << 392, p, g1, "sw", g1.R_ORDER, _all(c15), _all(c15), {c: n for c in "xyz"},
                 digits((1 << 392) % p, 14, 28), [outside, g1.neg(outside)], p_neg=False, q_neg=False, cneg_carries=True)


# ---- Ed448 (fe448.hip.h, e448_law.hip.h) and Curve448 (c448_law.hip.h)
def _n448():
    # fe448.hip.h, "normal": limbs in (-2^10, 2^28 + 2^10), all sixteen; the value has no bound of its own
    return LimbClass("n", [-(1 << 10) + 1] * 16, [(1 << 28) + (1 << 10) - 1] * 16)


def _ed448():
    # e448_law.hip.h: e448_dbl "coordinates n in, n out"; e448_add "Coordinates n (x possibly negated: 1 n) in, n out".  P goes through
    # both, so only Q's x is handed over negated
    n = _n448()
    p = e448.P
    specials = [(0, p - 1), (1, 0), (p - 1, 0)]          # order 2 and the two points of order 4
    return Curve("Ed448", "ed448", 16, 28, 1, p, e448, "ed", e448.N, _all(n), _all(n), {c: n for c in "xyz"}, _small_one(16), specials, p_neg=False)


def _curve448():
    # c448_law.hip.h: m448_dbl and m448_add "coordinates n (x possibly negated: 1 n) in, n out".  The law runs on E_M; the reference adds
    # Montgomery points, reached through the birational map of the header (curve448_ref.to_inner / from_inner, with its flagged identity
    # and (0, 0))
    n = _n448()
    specials = [c448.to_inner(c448.TWO_TORSION), c448.to_inner(c448.T4), c448.to_inner(c448.neg(c448.T4))]     # (0 : -1 : 1), y = 0
    return Curve("Curve448", "curve448", 16, 28, 1, c448.P, c448, "ed", e448.N, _all(n), _all(n), {c: n for c in "xyz"}, _small_one(16),
                 specials, to_ref=c448.from_inner, from_ref=c448.to_inner)


# ---- Ed25519 (fe25519.hip.h, kernels_ed25519.hip.h) and Baby JubJub (fbn254.hip.h, kernels_bjj.hip.h): extended coordinates
def _torsion(ref):
    return [t for t in ref.torsion_points() if t != (0, 1)]


def _ed25519():
    p = e25.P
    # fe25519.hip.h, "normal": limbs 0, 2..7 in [0, 2^29), limb 1 in (-2^17, 2^29 + 2^17), limb 8 in [0, 2^23); values never need a bound
    lo, hi = [0] * 9, [(1 << 29) - 1] * 8 + [(1 << 23) - 1]
    lo[1], hi[1] = -(1 << 17) + 1, (1 << 29) + (1 << 17) - 1
    n = LimbClass("n", lo, hi)
    # kernels_ed25519.hip.h, ed_dbl and ed_add_dt: "coordinates n (x and t possibly negated by ed_cneg) in, n out"
    # Ed25519Curve: "canonical words ... in the LDS table": fe_pack's representative in [0, p), read back by fe_unpack
    canon = LimbClass("canonical", [0] * 9, [(1 << 29) - 1] * 8 + [(1 << 23) - 1], vlo=-1, vhi=p)
    return Curve("Ed25519", "ed25519", 9, 29, 1, p, e25, "ed", e25.N, _all(n, "xyzt"), _all(n, "xyzt"), {c: n for c in "xyzt"}, _small_one(9),
                 _torsion(e25), extended=True, cls_lds={c: canon for c in "xyzt"})


def _bjj():
    p = bjj.P
    # fbn254.hip.h, "normal": limbs 0..7 in [0, 2^29), limb 8 in (-2^22, 2^23), value in (-2^253, p + 2^253)
    n = LimbClass("n", [0] * 8 + [-(1 << 22) + 1], [(1 << 29) - 1] * 8 + [(1 << 23) - 1], vlo=-(1 << 253), vhi=p + (1 << 253))
    # kernels_bjj.hip.h, bjj_dbl and bjj_add_dt: "coordinates n (x and t possibly negated by bjj_cneg) in, n out"
    # bn_to_words: "a normal ... moved into [0, 2^256): carried, p added when it is negative — bn_unpack_raw reads it back as a normal of
    # the same value mod p": a normal that is not negative
    words = LimbClass("n >= 0", [0] * 9, [(1 << 29) - 1] * 8 + [(1 << 23) - 1], vlo=-1, vhi=p + (1 << 253))
    return Curve("Baby JubJub", "bjj", 9, 29, 1 << 261, p, bjj, "ed", bjj.N, _all(n, "xyzt"), _all(n, "xyzt"), {c: n for c in "xyzt"},
                 digits((1 << 261) % p, 9, 29), _torsion(bjj), extended=True, cls_lds={c: words for c in "xyzt"})


# ---- Bandersnatch and JubJub (fr29.hip.h, curve.hip.h, kernels_te.hip.h): extended coordinates over the 9 x 29-bit Fr
class TeRef:
    """oracle/pyref/bandersnatch.py in the add / neg / mul(k, pt) / G shape of the tests/*_ref.py modules, under using(suite).  mul is
    plain double-and-add on the affine law and does not reduce k, so N R is a torsion point and not the identity by decree; a sum at
    infinity (Bandersnatch: a = -5 is no square, two points of order 2 are not affine) raises ZeroDivisionError"""

    def __init__(self, suite):
        from oracle.pyref import bandersnatch as bsn

        self.bsn, self.suite, self.P = bsn, suite, bsn.P
        with bsn.using(suite):
            self.G, self.N, self.A, self.D, self.COFACTOR = bsn.G, bsn.N, bsn.A, bsn.D, bsn.COFACTOR

    def add(self, a, b):
        with self.bsn.using(self.suite):
            try:
                return self.bsn.add(a, b)
            except ValueError as exc:                            # pow(0, -1, p): a denominator of the affine law is zero
                raise ZeroDivisionError(str(exc)) from exc

    def neg(self, a):
        return self.bsn.neg(a)

    def mul(self, k, pt):
        acc = (0, 1)
        while k > 0:
            if k & 1:
                acc = self.add(acc, pt)
            pt = self.add(pt, pt)
            k >>= 1
        return acc

    def on_curve(self, pt):
        with self.bsn.using(self.suite):
            return self.bsn.on_curve(pt)

    def sqrt(self, v):
        return self.bsn.sqrt(v)


def te_small_points(ref):
    """(torsion, outside): the affine points of small order other than the identity, as multiples of N R for curve points R found on
    the CPU by their x, and points outside the prime-order subgroup (one per kind: N R a torsion point; N R at infinity)"""
    p, torsion, outside, at_infinity = ref.P, [], [], []
    x = 1
    while x < 60:
        x += 1
        y = ref.sqrt((1 - ref.A * x * x) * pow(1 - ref.D * x * x, -1, p) % p)
        if y is None:
            continue
        R_ = (x, y)
        assert ref.on_curve(R_)
        try:
            T = ref.mul(ref.N, R_)
        except ZeroDivisionError:
            if not at_infinity:
                at_infinity.append(R_)
            continue
        if T == (0, 1):
            continue
        if not outside or (ref.mul(ref.COFACTOR // 2, T) != (0, 1) and ref.mul(ref.COFACTOR // 2, ref.mul(ref.N, outside[0])) == (0, 1)):
            outside[:1] = [R_]                                   # prefer one whose torsion part has the full order
        S = T
        while S != (0, 1):                                       # every multiple of the torsion point
            if S not in torsion:
                torsion.append(S)
            S = ref.add(S, T)
    return sorted(torsion), outside + at_infinity


def glv_lambda(order):
    """the scalar the endomorphism multiplies by, from the lattice basis glv_decompose of csrc/hostproto.hpp uses: k = k1 + k2 lambda with
    (a1, b1) and (a2, -a1) in the lattice x + y lambda = 0 mod n"""
    import re

    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dot_ring_amd", "csrc", "hostproto.hpp")).read()
    text = text[text.index("inline bool glv_decompose"):]

    def two(name):
        m = re.search(r"static const uint64_t %s\[2\] = \{(0x[0-9a-fA-F]+)ULL, (0x[0-9a-fA-F]+)ULL\}" % name, text)
        return int(m.group(1), 16) | int(m.group(2), 16) << 64

    a1, b1, a2 = two("A1"), two("B1"), two("A2")
    lam = -a1 * pow(b1, -1, order) % order
    assert (a2 - a1 * lam) % order == 0
    return lam


def _te(name, suite_name, te_id, with_endo):
    from oracle.pyref import bandersnatch as bsn

    ref = TeRef(getattr(bsn, suite_name))
    p, top = ref.P, 29 * 8
    # fr29.hip.h:12 "normal": limbs 0..7 in [0, 2^29), limb 8 small and signed, value in (-p/2, 1.5 p); the top limb is what the value
    # leaves it.  curve.hip.h:6-7: "coordinates come in normal (or negated normal: limbs within (-2^29, 2^29), |value| <= 1.5 p) and go
    # out normal"; te_cneg negates x and t, so those two are the ones handed over negated
    vlo, vhi = -(p // 2) - 1, 3 * p // 2 + 1
    n = LimbClass("n", [0] * 8 + [(vlo >> top) - 1], [(1 << 29) - 1] * 8 + [vhi >> top], vlo=vlo, vhi=vhi)
    # kernels_te.hip.h:20 "the table keeps canonical 8-word coordinates", fr29.hip.h:128 "canonical words (< p, < 2^255) reinterpreted in
    # radix 2^29": lds_load_point and a table row (te_msm_walk: unpack(load_fr_std(...))) are unpack of canonical words
    canon = LimbClass("canonical", [0] * 9, [(1 << 29) - 1] * 8 + [p >> top], vlo=-1, vhi=p)
    torsion, outside = te_small_points(ref)
    cv = Curve(name, "te", 9, 29, 1 << 261, p, ref, "ed", ref.N, _all(n, "xyzt"), _all(n, "xyzt"), {c: n for c in "xyzt"},
               digits((1 << 261) % p, 9, 29), torsion + outside, extended=True, cls_lds={c: canon for c in "xyzt"}, slots=TE_SLOTS,
               te_id=te_id, endo=glv_lambda(ref.N) if with_endo else None, lds_canonical=True, no_t_zero=True, d=ref.D)
    cv.torsion, cv.outside = torsion, outside
    return cv


def _bandersnatch():
    return _te("Bandersnatch", "SHA512", 0, True)


def _jubjub():
    return _te("JubJub", "JUBJUB", 1, False)


CURVES = ("ed25519", "bjj", "p256", "secp256k1", "blsg1", "ed448", "curve448", "p521", "p384")       # the nine wave curves
TE_CURVES = ("bandersnatch", "jubjub")                                                              # curve.hip.h over fr29
_BUILDERS = {"bandersnatch": _bandersnatch, "jubjub": _jubjub, "ed25519": _ed25519, "bjj": _bjj, "p256": _p256, "secp256k1": _secp256k1, "blsg1": _blsg1, "ed448": _ed448,
             "curve448": _curve448, "p521": _p521, "p384": _p384}
_CACHE = {}


def curve(name):
    if name not in _CACHE:
        _CACHE[name] = _BUILDERS[name]()
    return _CACHE[name]


# ---------------------------------------------------------------- lanes
# the six windows: bit w negates the table term of window w, bit 8 + w replaces it by the identity.  A negated term, an identity term,
# two equal signs in a row (both signs), and mixtures
CONTROLS = (0x0000, 0x003F, 0x0015, 0x002A, 0x0100 | 0x0002, 0x2100 | 0x000C, 0x3F00, 0x1200 | 0x0021, 0x0006 | 0x0800)


class Lane:
    def __init__(self, what, P, Q, images, control):
        self.what, self.P, self.Q, self.images, self.control = what, P, Q, images, control      # images: {"P": {c: image}, "Q": {...}}
        self._want = None
        self.row = None          # dr_te_law_selftest: the affine point of the table row; its images are images["R"]: x, y, dt


class Builder:
    def __init__(self, cv, seed=2024):
        self.cv, self.rng = cv, random.Random(f"{cv.name}/{seed}")
        self.lanes = []
        # (operand, coordinate, class, corner, "kmin" | "kmax") and (operand, coordinate, "negated", corner) reached by some lane
        self.seen = set()

    def image(self, cls, residue, corner, kmode):
        cv = self.cv
        target = residue * cv.R % cv.p
        kmin, kmax = k_range(cls, corner, target, cv.p, cv.bits)
        k = {"kmin": kmin, "kmax": kmax}.get(kmode)
        if k is None:
            k = self.rng.randint(kmin, kmax)
        image = image_at(cls, corner, target + k * cv.p, cv.bits)
        assert image is not None and cls.contains(image, cv.bits) and cv.residue(image) == residue % cv.p
        return image, ("kmin" if k == kmin else None, "kmax" if k == kmax else None)

    def point_images(self, operand, pt, corner=None, kmode=None, negate=False, which=None):
        """the images of a point's coordinates under a random scale; corner / kmode / which (the index of the class) None: drawn per
        coordinate.  negate: the coordinates cneg negates are the limb-wise negation of an image of their negative in the class of a table
        entry: what cneg hands to add"""
        cv, rng = self.cv, self.rng
        classes = cv.cls_p if operand == "P" else cv.cls_q
        xyz = cv.lift(pt, rng.randrange(1, cv.p))
        images = {}
        for c in cv.coords:
            co, km = corner or rng.choice(CORNERS), kmode or rng.choice(("kmin", "kmax", "any"))
            if negate and c in cv.neg_coords:
                cls = classes[c][0]
                image, ends = self.image(cls, -xyz[c] % cv.p, co, km)
                images[c] = [-x for x in image]
                assert cls.negated().contains(images[c], cv.bits) and cv.residue(images[c]) == xyz[c]
                self.seen.add((operand, c, "negated", co))
            else:
                cls = classes[c][which % len(classes[c])] if which is not None else rng.choice(classes[c])
                images[c], ends = self.image(cls, xyz[c], co, km)
                for e in ends:
                    if e:
                        self.seen.add((operand, c, cls.name, co, e))
        return images

    def lane(self, what, P, Q, p_images, q_images):
        control = CONTROLS[len(self.lanes) % len(CONTROLS)]
        self.lanes.append(Lane(what, P, Q, {"P": p_images, "Q": q_images}, control))

    def own_identity(self):
        """the image identity() itself returns"""
        cv = self.cv
        zero, one = [0] * cv.limbs, list(cv.one_image)
        own = {"x": zero, "y": one, "z": zero if cv.kind == "sw" else one}
        if cv.extended:
            own["t"] = zero
        return own

    def build(self):
        cv, rng = self.cv, self.rng
        rp = cv.random_point
        kinds = max(len(v) for v in cv.cls_p.values())
        # every coordinate of both points at every corner of every class, at the smallest and at the largest k
        for which in range(kinds):
            for corner in CORNERS:
                for kmode in ("kmin", "kmax"):
                    P, Q = rp(rng), rp(rng)
                    self.lane(f"corner {corner} {kmode} {which}", P, Q, self.point_images("P", P, corner, kmode, which=which),
                              self.point_images("Q", Q, corner, kmode, which=which))
        # each coordinate independently in each kind of image
        for j in range(12):
            P, Q = rp(rng), rp(rng)
            self.lane(f"mixed {j}", P, Q, self.point_images("P", P), self.point_images("Q", Q))
        # the once-negated class
        if cv.q_neg:
            for corner in CORNERS:
                P, Q = rp(rng), rp(rng)
                self.lane(f"negated {corner}", P, Q, self.point_images("P", P, corner, "kmax", negate=cv.p_neg),
                          self.point_images("Q", Q, corner, "kmin", negate=True))
        # Q = P as the same image; under another scale and other images; Q = -P; Q = 2 P
        P = rp(rng)
        images = self.point_images("P", P, "hi", "kmax", which=0)
        self.lane("Q = P, one image", P, P, images, {c: list(v) for c, v in images.items()})
        self.lane("Q = P, another scale", P, P, self.point_images("P", P), self.point_images("Q", P))
        self.lane("Q = -P", P, cv.neg(P), self.point_images("P", P), self.point_images("Q", cv.neg(P)))
        self.lane("Q = 2 P", P, cv.add(P, P), self.point_images("P", P), self.point_images("Q", cv.add(P, P)))
        # the identity, as identity()'s own image and as scaled images of it
        O, own = cv.identity(), self.own_identity()
        Q = rp(rng)
        self.lane("P = O own", O, Q, own, self.point_images("Q", Q))
        self.lane("Q = O own", Q, O, self.point_images("P", Q), own)
        self.lane("P = Q = O own", O, O, own, own)
        for corner in CORNERS:
            Q = rp(rng)
            self.lane(f"P = O scaled {corner}", O, Q, self.point_images("P", O, corner), self.point_images("Q", Q))
            self.lane(f"Q = O scaled {corner}", Q, O, self.point_images("P", Q), self.point_images("Q", O, corner))
        self.lane("P = Q = O scaled", O, O, self.point_images("P", O), self.point_images("Q", O))
        # the points a random scalar never gives
        for i, s in enumerate(cv.specials):
            R_ = rp(rng)
            self.lane(f"P special {i}", s, R_, self.point_images("P", s), self.point_images("Q", R_))
            self.lane(f"Q special {i}", R_, s, self.point_images("P", R_), self.point_images("Q", s, negate=cv.q_neg))
            self.lane(f"P = Q special {i}", s, s, self.point_images("P", s, "hi"), self.point_images("Q", s, "lo"))
            t = cv.specials[(i + 1 + i // 2) % len(cv.specials)]
            self.lane(f"special {i} + another", s, t, self.point_images("P", s), self.point_images("Q", t))
        # more than a wave of them: a tail lane in a second workgroup
        while len(self.lanes) < 70:
            P, Q = rp(rng), rp(rng)
            self.lane(f"mixed {len(self.lanes)}", P, Q, self.point_images("P", P), self.point_images("Q", Q, negate=cv.q_neg and rng.random() < 0.3))
        if cv.te_id is not None:
            self.rows()
        return self

    def rows(self):
        """dr_te_law_selftest: a table row (x2, y2, d x2 y2) per lane, in the form te_msm_walk hands to te_madd: unpack of the canonical
        words k_te_msm_prepare packed (one image per residue), negated limb-wise on the device where the control word says.  Rows are
        prime-order points (what the endomorphism of slot 16 is defined on) or the identity; on a curve without the endomorphism also
        the small-order points.  Some rows are the lane's own P or -P, so that te_madd doubles and cancels."""
        cv, rng = self.cv, self.rng
        for i, lane in enumerate(self.lanes):
            what = lane.what.split()
            if what[0] == "mixed" and int(what[1]) % 4 == 0:
                row = lane.P
            elif what[0] == "mixed" and int(what[1]) % 4 == 1:
                row = cv.neg(lane.P)
            elif what[0] == "corner" and what[2] == "kmin" and what[1] == "lo":
                row = cv.identity()
            elif cv.endo is None and lane.what.startswith("P special"):
                row = lane.P
            else:
                row = cv.random_point(rng)
            lane.row = row
            dt = cv.d * row[0] * row[1] % cv.p
            lane.images["R"] = {c: digits(v * cv.R % cv.p, cv.limbs, cv.bits) for c, v in (("x", row[0]), ("y", row[1]), ("dt", dt))}
            if i % 3 == 1:
                lane.control |= ROW_NEGATED


_POOLS = {}


def pool(name):
    """the lanes of a curve (built once, seeded) and what the builder reached"""
    if name not in _POOLS:
        _POOLS[name] = Builder(curve(name)).build()
    return _POOLS[name]


def pack_lanes(cv, lanes):
    """(points, controls) as the bytes dr_<suite>_law_selftest takes"""
    words = []
    for lane in lanes:
        words += [x for who in ("P", "Q") for c in cv.coords for x in lane.images[who][c]]
        if cv.te_id is not None:                                                       # dr_te_law_selftest: then the table row
            words += [x for c in ("x", "y", "dt") for x in lane.images["R"][c]]
    return struct.pack(f"<{len(words)}i", *words), struct.pack(f"<{len(lanes)}I", *[lane.control for lane in lanes])


def unpack_slots(cv, raw, count):
    """[{slot: {coordinate: image}}] of the device's output"""
    per = len(cv.coords) * cv.limbs
    words = struct.unpack(f"<{count * cv.slots * per}i", raw)
    out = []
    for i in range(count):
        slots = {}
        for s in range(cv.slots):
            if (s == SLOT_DBL_NO_T and not cv.extended) or (s == SLOT_ENDO and cv.endo is None):
                continue
            at = (i * cv.slots + s) * per
            slots[s] = {c: list(words[at + j * cv.limbs : at + (j + 1) * cv.limbs]) for j, c in enumerate(cv.coords)}
        out.append(slots)
    return out


# ---------------------------------------------------------------- the checker
def expected(cv, lane):
    """{slot: inner affine point} by the reference law (computed once per lane)"""
    if lane._want is None:
        P, Q = lane.P, lane.Q
        want = {SLOT_ADD: cv.add(P, Q), SLOT_SUB: cv.add(P, cv.neg(Q)), SLOT_DBL: cv.add(P, P), SLOT_NEG: cv.neg(P), SLOT_KEEP: P}
        if cv.extended:
            want[SLOT_DBL_NO_T] = want[SLOT_DBL]
        want[SLOT_LDS] = table = want[SLOT_ADD]
        acc = P
        for w in range(WINDOWS):
            for _ in range(4):
                acc = cv.add(acc, acc)
            if not (lane.control >> (8 + w)) & 1:
                acc = cv.add(acc, cv.neg(table) if (lane.control >> w) & 1 else table)
            want[SLOT_CHAIN + w] = acc
        if lane.row is not None:
            row = cv.neg(lane.row) if lane.control & ROW_NEGATED else lane.row
            want[SLOT_MADD] = cv.add(P, row)
            twice = cv.add(row, row)
            want[SLOT_MADD4] = cv.add(twice, twice)
            want[SLOT_ADD_OUT] = cv.add(want[SLOT_ADD], want[SLOT_DBL])
            if cv.endo is not None:
                want[SLOT_ENDO] = cv.from_ref(cv.ref.mul(cv.endo, cv.to_ref(lane.row)))            # of the row as given, not negated
        lane._want = want
    return lane._want


SLOT_NAMES = {SLOT_ADD: "add", SLOT_SUB: "sub", SLOT_DBL: "dbl", SLOT_DBL_NO_T: "dbl_no_t", SLOT_NEG: "cneg", SLOT_LDS: "lds", SLOT_KEEP: "keep",
              SLOT_MADD: "madd", SLOT_MADD4: "madd4", SLOT_ADD_OUT: "add_out", SLOT_ENDO: "endo"}


def out_classes(cv, slot, c):
    """the classes the headers document for coordinate c of a slot (any one of them)"""
    if slot in (SLOT_NEG, SLOT_KEEP):
        # cneg hands back what it was given, some coordinates negated or not: the in-classes, or their negation; one that carries returns
        # a coordinate of the in-class
        if cv.cneg_carries or c not in cv.neg_coords:
            return list(cv.cls_p[c])
        return list(cv.cls_p[c]) + [cls.negated() for cls in cv.cls_p[c]]
    if slot == SLOT_LDS and cv.cls_lds is not None:
        return [cv.cls_lds[c]]
    return [cv.cls_out[c]]


def check_lane(cv, lane, slots, stats=None):
    """the failures of one lane's slots (an empty list: all is well); stats collects the largest |limb| and |value| per (op, coordinate)"""
    bad = []
    want = expected(cv, lane)
    for slot, images in sorted(slots.items()):
        op = SLOT_NAMES.get(slot, "chain")
        xyz = {c: cv.residue(images[c]) for c in cv.coords}
        if not cv.same_point(xyz, want[slot], with_t=slot != SLOT_DBL_NO_T):
            bad.append(f"{lane.what}: slot {slot} ({op}) is not the reference's point")
        if slot == SLOT_DBL_NO_T and cv.no_t_zero and any(images["t"]):
            bad.append(f"{lane.what}: slot {slot} ({op}) t = {images['t']} is not the zero image")
        for c in cv.coords:
            classes = out_classes(cv, slot, c)
            if not any(cls.contains(images[c], cv.bits) for cls in classes):
                bad.append(f"{lane.what}: slot {slot} ({op}) {c} = {images[c]} is outside its class {classes[0].name}{where_outside(classes[0], images[c], cv.bits)}")
            if stats is not None and slot not in (SLOT_NEG, SLOT_KEEP):
                limb, val = max(abs(x) for x in images[c]), abs(value_of(images[c], cv.bits))
                old = stats.get((op, c), (0, 0))
                stats[(op, c)] = (max(old[0], limb), max(old[1], val))
    if not cv.cneg_carries:
        # cneg is the field's limb-wise conditional negation: the images themselves are known
        for slot, sign in ((SLOT_NEG, -1), (SLOT_KEEP, 1)):
            if slot in slots:
                for c in cv.coords:
                    s = sign if c in cv.neg_coords else 1
                    if slots[slot][c] != [s * x for x in lane.images["P"][c]]:
                        bad.append(f"{lane.what}: slot {slot} ({SLOT_NAMES[slot]}) {c} is not the image of P{' negated' if s < 0 else ''}")
    if SLOT_LDS in slots and SLOT_ADD in slots and cv.cls_lds is None:
        # the table keeps limb images: from_lds gives back exactly what to_lds took
        if slots[SLOT_LDS] != slots[SLOT_ADD]:
            bad.append(f"{lane.what}: the point read back from LDS is not the image that was stored")
    if SLOT_LDS in slots and SLOT_ADD in slots and cv.lds_canonical:
        # the table keeps the canonical representative of what was stored: the same residue, digit by digit
        for c in cv.coords:
            if slots[SLOT_LDS][c] != digits(value_of(slots[SLOT_ADD][c], cv.bits) % cv.p, cv.limbs, cv.bits):
                bad.append(f"{lane.what}: slot {SLOT_LDS} (lds) {c} is not the canonical image of slot 0's {c}")
    return bad


def where_outside(cls, image, bits):
    """which limb of an image leaves the class, or that its value does"""
    for j, (x, a, b) in enumerate(zip(image, cls.lo, cls.hi)):
        if not a <= x <= b:
            return f": limb {j} = {x} is not in [{a}, {b}]"
    return f": the value {value_of(image, bits)} is not in ({cls.vlo}, {cls.vhi})"


def check_all(cv, lanes, all_slots, stats=None):
    assert len(lanes) == len(all_slots)
    bad = []
    for lane, slots in zip(lanes, all_slots):
        bad += check_lane(cv, lane, slots, stats)
    return bad


def format_stats(cv, stats):
    """one line per (op, coordinate): the largest |limb| and |value| reached, as powers of two"""
    import math

    lines = []
    for (op, c), (limb, val) in sorted(stats.items()):
        lines.append(f"{cv.name:16s} {op:8s} {c}: max |limb| 2^{math.log2(limb) if limb else 0:.3f}  max |value| 2^{math.log2(val) if val else 0:.2f}")
    return "\n".join(lines)


def reimage(cv, lane, rng):
    """the reference's own results as slots: every expected point lifted under a random scale and imaged in its out-class"""
    slots = {}
    for slot, pt in expected(cv, lane).items():
        xyz = cv.lift(pt, rng.randrange(1, cv.p))
        images = {}
        for c in cv.coords:
            cls = out_classes(cv, slot, c)[0]
            target = xyz[c] * cv.R % cv.p
            corner = rng.choice(CORNERS)
            kmin, kmax = k_range(cls, corner, target, cv.p, cv.bits)
            images[c] = image_at(cls, corner, target + rng.randint(kmin, kmax) * cv.p, cv.bits)
        slots[slot] = images
    if cv.cls_lds is None:
        slots[SLOT_LDS] = {c: list(v) for c, v in slots[SLOT_ADD].items()}
    if cv.lds_canonical:
        slots[SLOT_LDS] = {c: digits(value_of(v, cv.bits) % cv.p, cv.limbs, cv.bits) for c, v in slots[SLOT_ADD].items()}
    if cv.no_t_zero:
        slots[SLOT_DBL_NO_T]["t"] = [0] * cv.limbs
    if not cv.cneg_carries:
        slots[SLOT_KEEP] = {c: list(v) for c, v in lane.images["P"].items()}
        slots[SLOT_NEG] = {c: [-x if c in cv.neg_coords else x for x in v] for c, v in lane.images["P"].items()}
    return slots


def lane_line(cv, lane):
    """the `lane` line of the host checks: the images of P and Q, then the control word"""
    words = [x for who in ("P", "Q") for c in cv.coords for x in lane.images[who][c]]
    return "lane " + " ".join(str(x) for x in words) + f" {lane.control}"


def parse_lane_line(cv, text):
    """{slot: {coordinate: image}} of the host check's answer: the slots it runs (no LDS, no dbl_no_t), each as its raw limbs"""
    words = [int(t) for t in text.split()]
    order = [SLOT_ADD, SLOT_SUB, SLOT_DBL, SLOT_NEG, SLOT_KEEP] + [SLOT_CHAIN + w for w in range(WINDOWS)]
    per = len(cv.coords) * cv.limbs
    assert len(words) == per * len(order), (len(words), per * len(order))
    slots = {}
    for k, s in enumerate(order):
        slots[s] = {c: words[k * per + j * cv.limbs : k * per + (j + 1) * cv.limbs] for j, c in enumerate(cv.coords)}
    return slots


# ================================================================ fr29.hip.h itself on raw limb images (dr_fr_raw_selftest)
# A record is four images a, b, c, d; the device runs every operation on every record, and a record names the operations whose contract
# its images meet: only those are checked.  The reference is Python integers: the value of a result (sum l[i] 2^(29 i)) against the
# value the header promises - a congruence mod p for the Montgomery products and the inverse, the very integer for carries, the
# addition chains and the canonical words - and every returned limb and value against the class the header documents for that return.
FR_P = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
FR_R = 1 << 261
FR_TOP = 29 * 8
M29 = (1 << 29) - 1
FR_LIMB_SLOTS = ("mul", "sqr", "mul2", "carry", "carry_u", "sub_3p", "reduce_small", "repack", "inv", "aA_b", "bmaA_b", "aA_j", "bmaA_j")
FR_WORD_SLOTS = ("canon29", "canon29_small", "fs_to_std", "to_mont256")
FR_FLAGS = ("is_zero", "equal")
FR_IN_WORDS, FR_OUT_WORDS = 4 * 9, len(FR_LIMB_SLOTS) * 9 + len(FR_WORD_SLOTS) * 8 + 1
# the bounds, each TRANSCRIBED from the header line beside it
FR_MUL_WIDE, FR_MUL_NARROW = 1 << 30, 1 << 29            # fr29.hip.h:15 "max|a_i| max|b_j| <= 2^59.5 (2^30 x 2^29, ..."
FR_MUL_BOTH = (16 << 29) // 10                           # fr29.hip.h:15 "... or 1.6 * 2^29 twice"; :18 "sqr(a): max|a_i| <= 1.6 * 2^29"
FR_MUL_VALUE = 35 * FR_P * FR_P                          # fr29.hip.h:16 "|a| |b| <= 35 p^2 for a normal result"
FR_MUL2_LIMB = M29                                       # fr29.hip.h:18 "mul2(a, b, c, d): all limbs below 2^29 in magnitude, |a b + c d| <= 35 p^2"
FR_CARRY_LIMB = (1 << 31) - 5                            # fr29.hip.h, carry(): "|limb| < 2^31 - 4" (t = l[i] + c with c in [-4, 3] must fit)
FR_CARRY_U_LIMB = (1 << 32) - 8                          # curve.hip.h, carry_u(): low limbs "below 2^32 - 7 as unsigned" (t = l[i] + c, c <= 7)
FR_REDUCE_VALUE = 30 * FR_P                              # fr29.hip.h, reduce_small: "|value| < 30 p" in, "|value| < 0.51 p" out
FR_CANON_VALUE = 8 * FR_P                                # fr29.hip.h, canon29: "any value with |value| < 8 p"
FR_ZERO_VALUE = 4 * FR_P                                 # fr29.hip.h, is_zero / equal: "exact tests for |value| < 4 p"
FR_PRODUCT_LO, FR_PRODUCT_HI = -(4 * FR_P // 100), 104 * FR_P // 100      # curve.hip.h:66 "products of normal operands (limbs in [0, 2^29),
#                                                                           values in (-0.04 p, 1.04 p))": the ends te_aA / te_b_minus_aA take
_VLO, _VHI = -(FR_P // 2) - 1, 3 * FR_P // 2 + 1
FR_NORMAL = LimbClass("normal", [0] * 8 + [(_VLO >> FR_TOP) - 1], [M29] * 8 + [_VHI >> FR_TOP], vlo=_VLO, vhi=_VHI)       # fr29.hip.h:12
FR_CARRIED = LimbClass("carried", [0] * 8 + [-(1 << 31)], [M29] * 8 + [(1 << 31) - 1])                                       # fr29.hip.h:19
FR_SIGNED29 = LimbClass("within (-2^29, 2^29)", [-M29] * 9, [M29] * 9)                                                       # curve.hip.h:68, :76
FR_LAZY = LimbClass("lazy", [-(1 << 30)] * 9, [1 << 30] * 9)                     # a form for exact values: limbs near +-2^30
FR_BIG = LimbClass("big", [-FR_CARRY_LIMB] * 9, [FR_CARRY_LIMB] * 9)              # ... and near the bound of carry()


def fr_value(image, unsigned_low=False):
    """sum l[i] 2^(29 i); unsigned_low: limbs 0..7 read as the 32-bit unsigned words carry_u takes"""
    return sum(((x & 0xFFFFFFFF) if unsigned_low and i < 8 else x) << (29 * i) for i, x in enumerate(image))


def fr_digits(v):
    """the carried image of any integer: limbs 0..7 in [0, 2^29), the signed top limb what is left"""
    return digits(v, 9, 29)


def fr_at(low, want):
    """limbs 0..7 exactly as given, the top limb such that the value is the nearest to `want` that is not beyond it (seen from zero):
    the low limbs sit AT their bound and the value within 2^232 = p / 7.6e6 of its bound"""
    lv = fr_value(list(low) + [0])
    top = (want - lv) >> FR_TOP if want >= 0 else -((lv - want) >> FR_TOP)
    return list(low) + [top]


def fr_exact(v, form):
    """an image of the integer v: "digits" (carried), or written from a corner of FR_LAZY / FR_BIG ("lazy hi", "big alt0", ...)"""
    if form == "digits":
        return fr_digits(v)
    cls, corner = form.split()
    image = image_at({"lazy": FR_LAZY, "big": FR_BIG}[cls], corner, v, 29)
    assert image is not None and fr_value(image) == v
    return image


def fr_pattern(which, m):
    """eight low limbs of magnitude m: all positive, all negative, or alternating"""
    return {"+": [m] * 8, "-": [-m] * 8, "+-": [m, -m] * 4, "-+": [-m, m] * 4}[which]


class FrRecord:
    def __init__(self, what, ops, a, b=None, c=None, d=None):
        zero = [0] * 9
        self.what, self.ops = what, frozenset(ops)
        self.a, self.b, self.c, self.d = (list(x) if x is not None else list(zero) for x in (a, b, c, d))
        assert self.ops <= set(FR_LIMB_SLOTS + FR_WORD_SLOTS + FR_FLAGS), self.ops
        assert all(-(1 << 31) <= x < (1 << 32) for img in (self.a, self.b, self.c, self.d) for x in img)


def _isqrt(n):
    import math

    return math.isqrt(n)


def build_fr_records(seed=2025):
    p, rng, out = FR_P, random.Random(f"fr29/{seed}"), []
    forms = ["digits"] + [f"{cls} {corner}" for cls in ("lazy", "big") for corner in CORNERS]

    def add(what, ops, a, b=None, c=None, d=None):
        out.append(FrRecord(what, ops, a, b, c, d))

    # ---- mul: the limb bound and the value bound together, every arrangement of signs; then the same pair swapped
    for wide, narrow, va in ((FR_MUL_WIDE, FR_MUL_NARROW, 7 * p), (FR_MUL_BOTH, FR_MUL_BOTH, _isqrt(FR_MUL_VALUE))):
        for pa in ("+", "-", "+-", "-+"):
            for pb in ("+", "-", "+-"):
                for sa, sb in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
                    a = fr_at(fr_pattern(pa, wide), sa * va)
                    b = fr_at(fr_pattern(pb, narrow), sb * (FR_MUL_VALUE // abs(fr_value(a))))
                    ops = {"mul"} | ({"sqr"} if wide == FR_MUL_BOTH else set())
                    add(f"mul {wide}x{narrow} {pa} {pb} {sa} {sb}", ops, a, b)
                    if pb != "+-" or pa == "+-":
                        add(f"mul swapped {wide}x{narrow} {pa} {pb} {sa} {sb}", {"mul"}, b, a)
    for s in (1, -1):                                    # the top limb at the bound too
        a = [s * FR_MUL_WIDE] * 9
        add(f"mul top limb {s}", {"mul"}, a, fr_at(fr_pattern("+", FR_MUL_NARROW), FR_MUL_VALUE // abs(fr_value(a))))
    # ---- mul beyond 35 p^2: correct, and wider by |a b| / R (fr29.hip.h:16-17)
    for sa, sb in ((1, 1), (1, -1), (-1, -1)):
        add(f"mul beyond {sa} {sb}", {"mul"}, fr_at(fr_pattern("+", FR_MUL_WIDE), sa * 20 * p), fr_at(fr_pattern("-", FR_MUL_NARROW), sb * 10 * p))
    # ---- sqr: limbs at 1.6 * 2^29, |a|^2 just under 35 p^2
    for pa in ("+", "-", "+-", "-+"):
        for s in (1, -1):
            add(f"sqr {pa} {s}", {"sqr"}, fr_at(fr_pattern(pa, FR_MUL_BOTH), s * _isqrt(FR_MUL_VALUE)))
    # ---- mul2: all four operands at +-(2^29 - 1); a b + c d at +-35 p^2 with the two products of the same and of opposite signs
    root = _isqrt(FR_MUL_VALUE // 2)
    for pats in ("++++", "----", "+-+-", "+--+", "-++-"):
        pp = list(pats)
        for total in (1, -1):
            a = fr_at(fr_pattern(pp[0], FR_MUL2_LIMB), root)
            b = fr_at(fr_pattern(pp[1], FR_MUL2_LIMB), total * (FR_MUL_VALUE // 2 // fr_value(a)))
            c = fr_at(fr_pattern(pp[2], FR_MUL2_LIMB), -root)
            d = fr_at(fr_pattern(pp[3], FR_MUL2_LIMB), -total * (FR_MUL_VALUE // 2 // abs(fr_value(c))))
            add(f"mul2 same signs {pats} {total}", {"mul2"}, a, b, c, d)
            # opposite: a b = +-100 p^2 and c d the other way, 35 p^2 apart
            a = fr_at(fr_pattern(pp[0], FR_MUL2_LIMB), 10 * p)
            b = fr_at(fr_pattern(pp[1], FR_MUL2_LIMB), total * 10 * p)
            c = fr_at(fr_pattern(pp[2], FR_MUL2_LIMB), -10 * p)
            need = abs(fr_value(a) * fr_value(b)) - FR_MUL_VALUE                    # |c d| must be at least this
            d = fr_at(fr_pattern(pp[3], FR_MUL2_LIMB), total * (-(-need // abs(fr_value(c))) + (1 << FR_TOP)))
            add(f"mul2 opposite signs {pats} {total}", {"mul2"}, a, b, c, d)
    for pa in ("+-", "-+"):
        a = fr_at(fr_pattern(pa, FR_MUL2_LIMB), root)
        add(f"mul2 alternating {pa}", {"mul2"}, a, fr_at(fr_pattern(pa, FR_MUL2_LIMB), FR_MUL_VALUE // 2 // fr_value(a)), a,
            fr_at(fr_pattern("-+" if pa == "+-" else "+-", FR_MUL2_LIMB), FR_MUL_VALUE // 2 // fr_value(a)))
    # ---- carry: negative and mixed-sign limbs at the bound, and ordinary ones
    for pa in ("+", "-", "+-", "-+"):
        for top in (12345, -12345, (1 << 30), -(1 << 30)):
            add(f"carry {pa} {top}", {"carry"}, fr_pattern(pa, FR_CARRY_LIMB) + [top])
    for j in range(8):
        add(f"carry mixed {j}", {"carry"}, [rng.randint(-FR_CARRY_LIMB, FR_CARRY_LIMB) for _ in range(9)])
    # ---- carry_u and sub_3p: sums of normals, low limbs up to the unsigned bound
    normal_top = FR_NORMAL.hi[8]
    for k in range(1, 8):                                # k normals with every low limb at 2^29 - 1, at the top of their value range
        ops = {"carry_u", "sub_3p"}
        add(f"carry_u {k} normals", ops, [k * M29] * 8 + [k * normal_top])
        add(f"carry_u {k} normals, low", ops, [k * M29] * 8 + [k * FR_NORMAL.lo[8]])
    for top in (0, 5 * normal_top, -normal_top):
        add(f"carry_u at the bound {top}", {"carry_u", "sub_3p"}, [FR_CARRY_U_LIMB] * 8 + [top])
        add(f"carry_u alternating {top}", {"carry_u", "sub_3p"}, [FR_CARRY_U_LIMB, 0] * 4 + [top])
    add("carry_u zero", {"carry_u", "sub_3p"}, [0] * 9)
    for k in (1, 6):                                     # both ends of sub_3p's (0, 6 p), every low limb k (2^29 - 1)
        add(f"sub_3p just under 6 p, {k}", {"carry_u", "sub_3p"}, fr_at([k * M29] * 8, 6 * p - 1))
        add(f"sub_3p just above 0, {k}", {"carry_u", "sub_3p"}, fr_at([k * M29] * 8, 2 << FR_TOP))
    for j in range(8):
        add(f"carry_u mixed {j}", {"carry_u", "sub_3p"}, [rng.randint(0, FR_CARRY_U_LIMB) for _ in range(8)] + [rng.randint(-normal_top, 6 * normal_top)])
    # ---- reduce_small: within one unit of +-30 p, and around every (q + 1/2) p, where the float rounding of the top limb picks q: the
    # two integers beside the half, and eight units of the top limb to either side (the band the float's 24 bits can move q in)
    for i, v in enumerate((FR_REDUCE_VALUE - 1, -(FR_REDUCE_VALUE - 1), FR_REDUCE_VALUE - (1 << FR_TOP), -(FR_REDUCE_VALUE - (1 << FR_TOP)))):
        for form in ("digits", "lazy hi", "big lo", "big alt0"):
            add(f"reduce_small edge {i} {form}", {"reduce_small"}, fr_exact(v, form))
    for q in range(-30, 30):
        half = (2 * q + 1) * p // 2                      # floor((q + 1/2) p); p is odd, so the half itself is no integer
        for j, v in enumerate((half, half + 1, half - (8 << FR_TOP), half + 1 + (8 << FR_TOP))):
            if abs(v) < FR_REDUCE_VALUE:
                add(f"reduce_small half {q} {j}", {"reduce_small"}, fr_exact(v, forms[(q + 30 + j) % len(forms)]))
    # ---- canon29 (k p + v, k = -8 .. 7), canon29_small (the same inside (-p, 3 p)), pack / unpack, inv, the conversions, is_zero
    n = 0
    for k in range(-8, 8):
        for v in (0, 1, p - 1):
            value = k * p + v
            for form in ("digits", forms[1 + n % 8]):
                n += 1
                ops = {"canon29", "repack", "inv", "fs_to_std", "carry"}
                if not form.startswith("big"):           # a product with K256 (limbs below 2^29) takes limbs up to 2^30
                    ops.add("to_mont256")
                if -p < value < 3 * p:
                    ops.add("canon29_small")
                if abs(value) <= FR_ZERO_VALUE and (v == 0 or abs(value) < FR_ZERO_VALUE):
                    ops.add("is_zero")
                add(f"canon {k} p + {v if v < 2 else 'p - 1'} {form}", ops, fr_exact(value, form))
    for v in (-p + 1, 3 * p - 1):                        # the very ends of (-p, 3 p)
        for form in ("digits", "lazy lo", "big alt1"):
            add(f"canon29_small end {v // p} {form}", {"canon29_small", "canon29", "repack"}, fr_exact(v, form))
    # ---- is_zero: every k p, |k| <= 4, from images that are not carried; and non-zero values that pass the limb-0 filter
    for k in range(-4, 5):
        for form in forms[1:]:
            add(f"is_zero {k} p {form}", {"is_zero", "canon29"}, fr_exact(k * p, form))
    for k in (-3, 0, 3):
        for dd in list(range(0, 5)) + list(range((1 << 29) - 4, 1 << 29)):
            v = (dd - k) % (1 << 29) + (rng.randrange(1, p >> 30) << 29)          # k p + v = dd mod 2^29 (p = 1 mod 2^29), 0 < v < p
            if v % p == 0 or abs(k * p + v) >= FR_ZERO_VALUE:
                continue
            form = forms[(dd + k) % len(forms)]
            image = fr_exact(k * p + v, form)
            assert (image[0] & M29) == dd
            add(f"is_zero passes the filter {k} {dd} {form}", {"is_zero", "canon29"}, image)
    # ---- equal: a - b = k p, and one beside it
    for k in range(-4, 5):
        for off in (0, 1, -1):
            if abs(k * p + off) >= FR_ZERO_VALUE and off:
                continue
            va = rng.randrange(-p // 2, 3 * p // 2)
            form = forms[(k + 4) % len(forms)]
            a, b = fr_exact(va, "digits" if form.startswith("big") else form), fr_exact(va - k * p - off, "lazy lo" if form.startswith("big") else "digits")
            add(f"equal {k} p + {off}", {"equal"}, a, b)
    # ---- te_aA / te_b_minus_aA: A and B at both ends of what a product of normal operands returns (a carried image: one per value),
    # and with every low limb at 2^29 - 1
    ends = (FR_PRODUCT_LO, FR_PRODUCT_HI, ((FR_PRODUCT_HI >> FR_TOP) << FR_TOP) - 1, ((FR_PRODUCT_LO >> FR_TOP) + 2 << FR_TOP) - 1, 0)
    for i, va in enumerate(ends):
        for j, vb in enumerate(ends):
            add(f"aA end {i} ({va / p:.3f} p), end {j} ({vb / p:.3f} p)",{"aA_b", "bmaA_b", "aA_j", "bmaA_j"}, fr_digits(va), fr_digits(vb))
    return out


_FR_RECORDS = None


def fr_records():
    global _FR_RECORDS
    if _FR_RECORDS is None:
        _FR_RECORDS = build_fr_records()
    return _FR_RECORDS


def fr_spread(count=65):
    """`count` records from across the pool with every operation among them (and already among the first: a call of one record is
    still checked for something): the first record that names each operation, then every k-th of the rest"""
    records = fr_records()
    picked = []
    for op in FR_LIMB_SLOTS + FR_WORD_SLOTS + FR_FLAGS:
        first = next(r for r in records if op in r.ops)
        if first not in picked:
            picked.append(first)
    rest = [r for r in records if r not in picked]
    picked += rest[:: len(rest) // (count - len(picked))][: count - len(picked)]
    assert len(picked) == count
    return picked


def pack_fr_records(records):
    words = [x - (1 << 32) if x >= (1 << 31) else x for r in records for img in (r.a, r.b, r.c, r.d) for x in img]
    return struct.pack(f"<{len(words)}i", *words)


def unpack_fr_results(raw, count):
    """[{name: nine limbs | an integer (the 8-word results) | a flag}] of the device's output"""
    words = struct.unpack(f"<{count * FR_OUT_WORDS}I", raw)
    out = []
    for i in range(count):
        w = words[i * FR_OUT_WORDS : (i + 1) * FR_OUT_WORDS]
        res = {name: [x - (1 << 32) if x >= (1 << 31) else x for x in w[9 * s : 9 * s + 9]] for s, name in enumerate(FR_LIMB_SLOTS)}
        at = 9 * len(FR_LIMB_SLOTS)
        for s, name in enumerate(FR_WORD_SLOTS):
            res[name] = sum(x << (32 * j) for j, x in enumerate(w[at + 8 * s : at + 8 * s + 8]))
        res["is_zero"], res["equal"] = w[-1] & 1, (w[-1] >> 1) & 1
        out.append(res)
    return out


# ---- the operations in Python integers, limb for limb where the header fixes the limbs (a carried image is unique, and so is the m of
# a Montgomery product); the checker uses them to NAME the limb that differs, the CPU tests as the reference's own results
_P_INV = pow(FR_P, -1, FR_R)


def fr_montgomery(pairs):
    """(sum a b + m p) / R with the one m in [0, R) that makes the division exact, carried"""
    s = sum(fr_value(a) * fr_value(b) for a, b in pairs)
    m = -s * _P_INV % FR_R
    return fr_digits((s + m * FR_P) >> 261)


def _limbwise(f, *images):
    return [f(*xs) for xs in zip(*images)]


def fr_model(r):
    """what the header promises for a record, as {name: result}; reduce_small and inv as ONE admissible result"""
    p, a, b = FR_P, r.a, r.b
    va = fr_value(a)
    u = fr_digits(fr_value(a, True))
    p3 = fr_digits(3 * p)
    five = fr_digits(fr_value([5 * x for x in a[:8]] + [5 * a[8]]))
    fiveb = fr_digits(fr_value([5 * x + y for x, y in zip(a[:8], b[:8])] + [5 * a[8] + b[8]]))
    inv = pow(va * pow(FR_R, -1, p) % p, -1, p) if va % p else 0
    return {
        "mul": fr_montgomery([(a, b)]), "sqr": fr_montgomery([(a, a)]), "mul2": fr_montgomery([(a, b), (r.c, r.d)]),
        "carry": fr_digits(va), "carry_u": u, "sub_3p": _limbwise(lambda x, y: x - y, u, p3),
        "reduce_small": fr_digits(va - (2 * va + p) // (2 * p) * p), "repack": fr_digits(va % p), "inv": fr_digits(inv * FR_R % p),
        "aA_b": _limbwise(lambda x, y: y - x, five, p3), "bmaA_b": _limbwise(lambda x, y: x - y, fiveb, p3),
        "aA_j": [-x for x in a], "bmaA_j": fr_digits(va + fr_value(b)),
        "canon29": va % p, "canon29_small": va % p, "fs_to_std": va * pow(FR_R, -1, p) % p, "to_mont256": (va << 256) * pow(FR_R, -1, p) % p,
        "is_zero": int(va % p == 0), "equal": int((va - fr_value(b)) % p == 0),
    }


def fr_model_words(r):
    """fr_model as the device's output words"""
    m = fr_model(r)
    words = [x & 0xFFFFFFFF for name in FR_LIMB_SLOTS for x in m[name]]
    words += [(m[name] >> (32 * j)) & 0xFFFFFFFF for name in FR_WORD_SLOTS for j in range(8)]
    return struct.pack(f"<{FR_OUT_WORDS}I", *words, m["is_zero"] | m["equal"] << 1)


def fr_mul_class(product):
    """what fr29.hip.h:12-17 documents for a Montgomery product of the integer a b (+ c d): normal up to 35 p^2, beyond it "wider by
    |a b| / (R / p) p": limbs 0..7 in [0, 2^29) either way"""
    if abs(product) <= FR_MUL_VALUE:
        return FR_NORMAL
    wide = abs(product) // FR_R + 1
    return LimbClass("wide product", [0] * 8 + [-(1 << 31)], [M29] * 8 + [(1 << 31) - 1], vlo=-wide, vhi=FR_P + wide)


def check_fr_record(r, res, stats=None):
    """the failures of one record's results (an empty list: all is well): the slot, what it should be, and the limb that differs"""
    p, bad = FR_P, []
    va, vb = fr_value(r.a), fr_value(r.b)
    model = fr_model(r)

    def differs(name):
        got, want = res[name], model[name]
        j = next((j for j in range(9) if got[j] != want[j]), None)
        return "" if j is None else f"; limb {j} = {got[j]}, the header's arithmetic gives {want[j]}"

    def limbs_in(name, cls):
        if not cls.contains(res[name], 29):
            bad.append(f"{r.what}: slot {name} = {res[name]} is outside its class {cls.name}{where_outside(cls, res[name], 29)}{differs(name)}")

    def congruent(name, want_times_r):
        """value(result) R^-1 = expected, i.e. value(result) = expected R (mod p)"""
        if (fr_value(res[name]) - want_times_r) % p:
            bad.append(f"{r.what}: slot {name} = {res[name]} is not congruent to what the reference computes{differs(name)}")

    def exactly(name, want):
        if fr_value(res[name]) != want:
            bad.append(f"{r.what}: slot {name} = {res[name]} has the value {fr_value(res[name])}, not {want}{differs(name)}")

    r_inv = pow(FR_R, -1, p)
    for name in sorted(r.ops):
        if name in ("mul", "sqr", "mul2"):
            product = {"mul": va * vb, "sqr": va * va, "mul2": va * vb + fr_value(r.c) * fr_value(r.d)}[name]
            congruent(name, product * r_inv)
            limbs_in(name, fr_mul_class(product))
        elif name == "carry":
            exactly(name, va)
            limbs_in(name, FR_CARRIED)
        elif name == "carry_u":
            exactly(name, fr_value(r.a, True))
            limbs_in(name, FR_CARRIED)
        elif name == "sub_3p":
            v = fr_value(r.a, True)
            exactly(name, v - 3 * p)
            # fr29.hip.h, sub_3p: "limbs of a normal -> limbs in (-2^29, 2^29)"; the top limb too for "a value known to lie in (0, 6p)"
            if 0 < v < 6 * p:
                limbs_in(name, FR_SIGNED29)
            elif any(abs(x) > M29 for x in res[name][:8]):
                bad.append(f"{r.what}: slot {name} = {res[name]} has a low limb outside (-2^29, 2^29){differs(name)}")
        elif name == "reduce_small":
            congruent(name, va)
            limbs_in(name, LimbClass("carried, |value| < 0.51 p", FR_CARRIED.lo, FR_CARRIED.hi, vmax=51 * p // 100 + 1))
        elif name == "repack":
            if res[name] != fr_digits(va % p):
                bad.append(f"{r.what}: slot {name} = {res[name]} is not the canonical image{differs(name)}")
        elif name == "inv":
            congruent(name, (pow(va * r_inv % p, -1, p) if va % p else 0) * FR_R)
            limbs_in(name, FR_NORMAL)
        elif name == "aA_b":
            exactly(name, 3 * p - 5 * va)                                             # curve.hip.h:76 "3p - 5A in (-2.2 p, 3.2 p)", limbs within (-2^29, 2^29)
            limbs_in(name, LimbClass(FR_SIGNED29.name, FR_SIGNED29.lo, FR_SIGNED29.hi, vlo=-22 * p // 10, vhi=32 * p // 10 + 1))
        elif name == "bmaA_b":
            exactly(name, vb + 5 * va - 3 * p)                                        # curve.hip.h:67 "B + 5A - 3p in (-3.3 p, 3.3 p)"
            limbs_in(name, LimbClass(FR_SIGNED29.name, FR_SIGNED29.lo, FR_SIGNED29.hi, vmax=33 * p // 10))
        elif name == "aA_j":
            if res[name] != [-x for x in r.a]:                                        # curve.hip.h:76 "JubJub -A"
                bad.append(f"{r.what}: slot {name} = {res[name]} is not the limb-wise negation{differs(name)}")
        elif name == "bmaA_j":
            exactly(name, va + vb)                                                    # curve.hip.h:67 "kept as B + A (<= 2.1 p)"
            limbs_in(name, LimbClass("carried, <= 2.1 p", FR_CARRIED.lo, FR_CARRIED.hi, vlo=-p, vhi=21 * p // 10 + 1))
        elif name in FR_WORD_SLOTS or name in FR_FLAGS:
            if res[name] != model[name]:
                bad.append(f"{r.what}: {name} = {res[name]:#x}, the reference computes {model[name]:#x}")
        if stats is not None and name in FR_LIMB_SLOTS:
            old = stats.get(name, (0, 0))
            stats[name] = (max(old[0], max(abs(x) for x in res[name])), max(old[1], abs(fr_value(res[name]))))
    return bad


def check_fr_records(records, results, stats=None):
    assert len(records) == len(results)
    return [b for r, res in zip(records, results) for b in check_fr_record(r, res, stats)]


def format_fr_stats(stats):
    import math

    return "\n".join(f"fr29 {name:13s} max |limb| 2^{math.log2(limb) if limb else 0:.3f}  max |value| {val / FR_P:.4f} p" for name, (limb, val) in sorted(stats.items()))
