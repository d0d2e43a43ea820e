"""Lanes and a checker for the group laws of the nine wave curves on RAW limb images (csrc/wave_curve.hip.h, wave_law_selftest), shared
by tests/test_gpu_wave_laws.py (the device), tests/test_law_images_cpu.py (the builder and the checker themselves) and the host builds
of the laws under -fsanitize=undefined (tests/native/*_host_check.cpp, the `lane` line).

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
      cneg_carries     cneg returns a carried coordinate (in cls_p's first class) instead of the limb-wise negation"""

    def __init__(self, name, suite, limbs, bits, R, p, ref, kind, order, cls_p, cls_q, cls_out, one_image, specials, extended=False,
                 p_neg=True, q_neg=True, to_ref=None, from_ref=None, cneg_carries=False, cls_lds=None):
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


# ---- P-384 (fp384.hip.h, p384_law.hip.h)
def _p384():
    # fp384.hip.h, "normal": limbs 0..12 in [-2^22, 2^28 + 2^22), limb 13 in (-2^21, 2^21), |value| < 2^385
    n = LimbClass("n", [-(1 << 22)] * 13 + [-(1 << 21) + 1], [(1 << 28) + (1 << 22) - 1] * 13 + [(1 << 21) - 1], 1 << 385)
    # fp384.hip.h, "k n" with k = 1: |limb| <= 2^28 + 2^22 for limbs 0..12, |limb 13| <= 2^21, |value| < 2^385
    m, t = (1 << 28) + (1 << 22), 1 << 21
    n1 = LimbClass("1 n", [-m] * 13 + [-t], [m] * 13 + [t], 1 << 385)
    # p384_law.hip.h: "A point's coordinates are x: 1 n, y: n (1 n once negated), z: n, in and out"
    cls = {"x": [n1], "y": [n], "z": [n]}
    # F384::small(1) = R mod p in signed limbs (fp384.hip.h): 2^8 - 2^12 B + 2^20 B^3 + 2^24 B^4
    one = [0] * 14
    one[0], one[1], one[3], one[4] = 1 << 8, -(1 << 12), 1 << 20, 1 << 24
    return Curve("P-384", "p384", 14, 28, 1 << 392, p384.P, p384, "sw", p384.N, cls, cls, {"x": n1, "y": n, "z": n}, one, _x0_points(p384))


# ---- P-521 (fp521.hip.h, p521_law.hip.h)
def _p521():
    # fp521.hip.h, "normal": limbs 0..17 in (-2^15, 2^28 + 2^15), limb 18 in [0, 2^17); the value has no bound of its own
    n = LimbClass("n", [-(1 << 15) + 1] * 18 + [0], [(1 << 28) + (1 << 15) - 1] * 18 + [(1 << 17) - 1])
    # fp521.hip.h, "k n" with k = 1: |limb| <= 2^28 + 2^15, EVERY limb
    m = (1 << 28) + (1 << 15)
    n1 = LimbClass("1 n", [-m] * 19, [m] * 19)
    # p521_law.hip.h: "A point's coordinates are x: 1 n, y: n (1 n once negated), z: n, in and out"
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


_BUILDERS = {"ed25519": _ed25519, "bjj": _bjj, "p256": _p256, "secp256k1": _secp256k1, "blsg1": _blsg1, "ed448": _ed448,
             "curve448": _curve448, "p521": _p521, "p384": _p384}
CURVES = tuple(_BUILDERS)
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
        return self


_POOLS = {}


def pool(name):
    """the lanes of a curve (built once, seeded) and what the builder reached"""
    if name not in _POOLS:
        _POOLS[name] = Builder(curve(name)).build()
    return _POOLS[name]


def pack_lanes(cv, lanes):
    """(points, controls) as the bytes dr_<suite>_law_selftest takes"""
    words = [x for lane in lanes for who in ("P", "Q") for c in cv.coords for x in lane.images[who][c]]
    return struct.pack(f"<{len(words)}i", *words), struct.pack(f"<{len(lanes)}I", *[lane.control for lane in lanes])


def unpack_slots(cv, raw, count):
    """[{slot: {coordinate: image}}] of the device's output"""
    per = len(cv.coords) * cv.limbs
    words = struct.unpack(f"<{count * SLOTS * per}i", raw)
    out = []
    for i in range(count):
        slots = {}
        for s in range(SLOTS):
            if s == SLOT_DBL_NO_T and not cv.extended:
                continue
            at = (i * SLOTS + s) * per
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
        lane._want = want
    return lane._want


SLOT_NAMES = {SLOT_ADD: "add", SLOT_SUB: "sub", SLOT_DBL: "dbl", SLOT_DBL_NO_T: "dbl_no_t", SLOT_NEG: "cneg", SLOT_LDS: "lds", SLOT_KEEP: "keep"}


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
        for c in cv.coords:
            classes = out_classes(cv, slot, c)
            if not any(cls.contains(images[c], cv.bits) for cls in classes):
                bad.append(f"{lane.what}: slot {slot} ({op}) {c} = {images[c]} is outside its class {classes[0].name}")
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
    return bad


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
