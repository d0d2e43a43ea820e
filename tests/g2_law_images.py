"""Lanes and a checker for the group law of BLS12-381's E(Fq2) on RAW limb images (csrc/kernels_g2_msm.hip.h, k_blsg2_law_selftest over
csrc/kernels_g2_h2c.hip.h's g2h_add / g2h_dbl / g2h_neg), the counterpart of law_images.py for a curve whose coordinates are pairs:
shared by tests/test_gpu_g2_law.py (the device) and tests/test_g2_msm_cpu.py (the builder and the checker themselves).

A lane is two real points P and Q of E(Fq2) — in G2, outside it, equal, inverse, the identity (0 : 1 : 0) — under a random projective
scale, each COMPONENT (c0, c1) of each coordinate a limb image at a corner of a class the headers document for a coordinate, and a
control word.  The classes are TRANSCRIBED from the headers, the citation beside each; nothing here is a measured number.  The checker
compares every slot with the big-integer restatement (bls12_381_g2_ref.py) by cross-multiplication over Fp2, and asks that every
returned component lies in the class the headers document for what the law returns.  The image machinery (LimbClass, image_at, k_range,
the corners, the control words) is law_images.py's."""
import os
import random
import struct
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bls12_381_g2_ref as g2  # noqa: E402
from law_images import CONTROLS, CORNERS, LimbClass, image_at, k_range, value_of, where_outside  # noqa: E402

P = g2.P
LIMBS, BITS, R = 14, 28, g2.MONT_R % g2.P
R_INV = pow(R, -1, P)
SLOTS, WINDOWS = 13, 6
SLOT_ADD, SLOT_SUB, SLOT_DBL, SLOT_UNUSED, SLOT_NEG, SLOT_REC, SLOT_KEEP, SLOT_CHAIN = 0, 1, 2, 3, 4, 5, 6, 7
COORDS = ("x", "y", "z")
M28 = (1 << 28) - 1


def _carried(name, vlo, vhi):
    """fq2_28.hip.h:9 "cK  carried: limbs 0..12 in [0, 2^28), a small signed top limb, |value| < K p"; the top limb is what the value
    leaves it (fq28.hip.h:95 "carry propagation: limbs 0..12 into [0, 2^28), the rest into the signed top limb")"""
    return LimbClass(name, [0] * 13 + [vlo >> 364], [M28] * 13 + [vhi >> 364], vlo=vlo, vhi=vhi)


# fq2_28.hip.h:7-8 "n   a product: limbs 0..12 in [0, 2^28), a small signed top limb, value in (-0.02 p, 1.02 p) when |a b| + |c d| < 50
# p^2 ..., and in (-0.41 p, 1.41 p) at the 1024 p^2 limit".  The law's rows reach 561 p^2 (kernels_g2_h2c.hip.h:100), so the n of a law
# output is the one at the limit.
N = _carried("n", -(41 * P // 100) - 1, 141 * P // 100 + 1)
# kernels_g2_h2c.hip.h:11-12 "A COORDINATE is c3: an n, the carried sum of two n (c2.1) or a carried negation of either"
C21 = _carried("c2.1", -(21 * P // 10), 21 * P // 10)
C3 = _carried("c3", -3 * P, 3 * P)
# fq2_28.hip.h:71-72, mul_add: "Out: the carried sum of two n, c2.1 (c2.9 at the 1024 limit)"; every row of the law is below 1024 p^2
C29 = _carried("c2.9", -(29 * P // 10), 29 * P // 10)
IN_CLASSES = (N, C21, C3)
# kernels_g2_h2c.hip.h:105 g2h_add "coordinates c3 in, c2.1 out" — three mul_add, whose own contract gives c2.9 at rows up to 1024 p^2 —
# and :89 g2h_dbl "coordinates c3 in; X, Z n and Y c2.1 out": X and Z one product each, Y a mul_add
OUT_ADD = {"x": C29, "y": C29, "z": C29}
OUT_DBL = {"x": N, "y": C29, "z": N}
ONE_IMAGE = [(R >> (BITS * i)) & M28 for i in range(LIMBS)]        # Fq28::one(): 2^392 mod p, limb by limb


def residue(image):
    return value_of(image, BITS) * R_INV % P


def carry(image):
    """fq28.hip.h:96, carry(): limbs 0..12 into [0, 2^28), the rest into the signed top limb"""
    out, c = [], 0
    for x in image[:-1]:
        t = x + c
        out.append(t & M28)
        c = t >> 28
    return out + [image[-1] + c]


def lift(pt, scale):
    """projective coordinates (Fp2 residues) of an affine point (None: the identity) under a non-zero Fp2 scale"""
    if pt is None:
        return {"x": g2.ZERO, "y": scale, "z": g2.ZERO}
    return {"x": g2.f2_mul(pt[0], scale), "y": g2.f2_mul(pt[1], scale), "z": scale}


def same_point(xyz, pt):
    """whether the projective residues are the affine point, by cross-multiplication over Fp2; the identity is (0 : Y : 0), Y != 0"""
    X, Y, Z = xyz["x"], xyz["y"], xyz["z"]
    if pt is None:
        return Z == g2.ZERO and X == g2.ZERO and Y != g2.ZERO
    if Z == g2.ZERO:
        return False
    return X == g2.f2_mul(pt[0], Z) and Y == g2.f2_mul(pt[1], Z)


class Lane:
    def __init__(self, what, P_, Q, images, control):
        self.what, self.P, self.Q, self.images, self.control = what, P_, Q, images, control      # images: {"P": {c: (image0, image1)}, "Q": ...}
        self._want = None


class Builder:
    def __init__(self, seed=2026):
        self.rng = random.Random(f"g2-law/{seed}")
        self.lanes = []
        self.seen = set()        # (operand, coordinate, component, class, corner, "kmin" | "kmax") reached by some lane
        # points of G2: a ladder from a random multiple of the generator; points outside it: the same plus the special point
        import g2_msm_cases

        self.special = g2_msm_cases.SPECIAL
        inside = [g2.mul(self.rng.randrange(1, g2.R_ORDER), g2.G)]
        for _ in range(47):
            inside.append(g2.add(inside[-1], g2.G))
        self.inside = inside
        self.outside = [g2.add(pt, self.special) for pt in inside[:16]]

    def point(self, outside=None):
        if outside is None:
            outside = self.rng.random() < 0.3
        return self.rng.choice(self.outside if outside else self.inside)

    def scale(self):
        while True:
            s = (self.rng.randrange(P), self.rng.randrange(P))
            if s != g2.ZERO:
                return s

    def image(self, cls, res, corner, kmode):
        target = res * R % P
        kmin, kmax = k_range(cls, corner, target, P, BITS)
        k = {"kmin": kmin, "kmax": kmax}.get(kmode)
        if k is None:
            k = self.rng.randint(kmin, kmax)
        image = image_at(cls, corner, target + k * P, BITS)
        assert image is not None and cls.contains(image, BITS) and residue(image) == res % P
        return image, [e for e, at in (("kmin", kmin), ("kmax", kmax)) if k == at]

    def point_images(self, operand, pt, corner=None, kmode=None, which=None):
        """the images of a point's six components under a random scale; corner / kmode / which (the index of the class) None: drawn per
        component"""
        rng = self.rng
        xyz = lift(pt, self.scale())
        images = {}
        for c in COORDS:
            pair = []
            for comp in (0, 1):
                co, km = corner or rng.choice(CORNERS), kmode or rng.choice(("kmin", "kmax", "any"))
                cls = IN_CLASSES[which] if which is not None else rng.choice(IN_CLASSES)
                image, ends = self.image(cls, xyz[c][comp], co, km)
                for e in ends:
                    self.seen.add((operand, c, comp, cls.name, co, e))
                pair.append(image)
            images[c] = tuple(pair)
        return images

    def lane(self, what, P_, Q, p_images, q_images):
        self.lanes.append(Lane(what, P_, Q, {"P": p_images, "Q": q_images}, CONTROLS[len(self.lanes) % len(CONTROLS)]))

    @staticmethod
    def own_identity():
        """the image g2h_identity() itself returns: (0 : 1 : 0)"""
        zero = [0] * LIMBS
        return {"x": (zero, zero), "y": (list(ONE_IMAGE), zero), "z": (zero, zero)}

    def build(self):
        pi = self.point_images
        # every component of both points at every corner of every class, at the smallest and at the largest k; P and Q in G2 or not
        for which in range(len(IN_CLASSES)):
            for j, corner in enumerate(CORNERS):
                for kmode in ("kmin", "kmax"):
                    A, B = self.point(outside=j % 2 == 1), self.point(outside=kmode == "kmax")
                    self.lane(f"corner {corner} {kmode} {IN_CLASSES[which].name}", A, B, pi("P", A, corner, kmode, which), pi("Q", B, corner, kmode, which))
        # each component independently in each kind of image
        for j in range(12):
            A, B = self.point(), self.point()
            self.lane(f"mixed {j}", A, B, pi("P", A), pi("Q", B))
        # Q = P as the same image; under another scale and other images; Q = -P; Q = 2 P — in G2 and outside it
        for tag, A in (("in G2", self.point(False)), ("outside G2", self.point(True))):
            images = pi("P", A, "hi", "kmax", 2)
            self.lane(f"Q = P, one image, {tag}", A, A, images, {c: (list(v[0]), list(v[1])) for c, v in images.items()})
            self.lane(f"Q = P, another scale, {tag}", A, A, pi("P", A), pi("Q", A))
            self.lane(f"Q = -P, {tag}", A, g2.neg(A), pi("P", A), pi("Q", g2.neg(A)))
            self.lane(f"Q = 2 P, {tag}", A, g2.add(A, A), pi("P", A), pi("Q", g2.add(A, A)))
        # the identity, as g2h_identity()'s own image and as scaled images of it
        own = self.own_identity()
        B = self.point()
        self.lane("P = O own", None, B, own, pi("Q", B))
        self.lane("Q = O own", B, None, pi("P", B), own)
        self.lane("P = Q = O own", None, None, own, own)
        for corner in CORNERS:
            B = self.point()
            self.lane(f"P = O scaled {corner}", None, B, pi("P", None, corner), pi("Q", B))
            self.lane(f"Q = O scaled {corner}", B, None, pi("P", B), pi("Q", None, corner))
        self.lane("P = Q = O scaled", None, None, pi("P", None), pi("Q", None))
        # the special point itself and its negative
        for i, s in enumerate((self.special, g2.neg(self.special))):
            B = self.point(False)
            self.lane(f"P special {i}", s, B, pi("P", s), pi("Q", B))
            self.lane(f"Q special {i}", B, s, pi("P", B), pi("Q", s))
            self.lane(f"P = Q special {i}", s, s, pi("P", s, "hi"), pi("Q", s, "lo"))
        self.lane("special + its negative", self.special, g2.neg(self.special), pi("P", self.special), pi("Q", g2.neg(self.special)))
        # more than a wave of them: a tail lane in a second workgroup
        while len(self.lanes) < 70:
            A, B = self.point(), self.point()
            self.lane(f"mixed {len(self.lanes)}", A, B, pi("P", A), pi("Q", B))
        return self


_POOL = None


def pool():
    """the lanes (built once, seeded) and what the builder reached"""
    global _POOL
    if _POOL is None:
        _POOL = Builder().build()
    return _POOL


def pack_lanes(lanes):
    """(points, controls) as the bytes dr_blsg2_law_selftest takes: P then Q, each x, y, z of 28 limbs, c0's then c1's"""
    words = [x for lane in lanes for who in ("P", "Q") for c in COORDS for comp in (0, 1) for x in lane.images[who][c][comp]]
    return struct.pack(f"<{len(words)}i", *words), struct.pack(f"<{len(lanes)}I", *[lane.control for lane in lanes])


def unpack_slots(raw, count):
    """[{slot: {coordinate: (image0, image1)}}] of the device's output; slot 3 is not written"""
    per = len(COORDS) * 2 * LIMBS
    words = struct.unpack(f"<{count * SLOTS * per}i", raw)
    out = []
    for i in range(count):
        slots = {}
        for s in range(SLOTS):
            if s == SLOT_UNUSED:
                continue
            at = (i * SLOTS + s) * per
            slots[s] = {c: (list(words[at + 2 * j * LIMBS : at + (2 * j + 1) * LIMBS]), list(words[at + (2 * j + 1) * LIMBS : at + (2 * j + 2) * LIMBS]))
                        for j, c in enumerate(COORDS)}
        out.append(slots)
    return out


def expected(lane):
    """{slot: affine point} by the restatement (computed once per lane)"""
    if lane._want is None:
        A, B = lane.P, lane.Q
        want = {SLOT_ADD: g2.add(A, B), SLOT_SUB: g2.add(A, g2.neg(B)), SLOT_DBL: g2.add(A, A), SLOT_NEG: g2.neg(A), SLOT_KEEP: A}
        want[SLOT_REC] = record = want[SLOT_ADD]
        acc = A
        for w in range(WINDOWS):
            acc = g2.add(acc, acc)
            if not (lane.control >> (8 + w)) & 1:
                acc = g2.add(acc, g2.neg(record) if (lane.control >> w) & 1 else record)
            want[SLOT_CHAIN + w] = acc
        lane._want = want
    return lane._want


def out_class(slot, c):
    """the class the headers document for a component of coordinate c of a slot"""
    if slot in (SLOT_NEG, SLOT_KEEP):
        return C3                       # what it was given, y perhaps through carry(neg()): "or a carried negation of either"
    return OUT_DBL[c] if slot == SLOT_DBL else OUT_ADD[c]


def check_lane(lane, slots, stats=None):
    """the failures of one lane's slots (an empty list: all is well); stats collects the largest |value| / p per (op, coordinate)"""
    bad = []
    want = expected(lane)
    for slot, images in sorted(slots.items()):
        xyz = {c: (residue(images[c][0]), residue(images[c][1])) for c in COORDS}
        if not same_point(xyz, want[slot]):
            bad.append(f"{lane.what}: slot {slot} is not the restatement's point")
        for c in COORDS:
            cls = out_class(slot, c)
            for comp in (0, 1):
                if not cls.contains(images[c][comp], BITS):
                    bad.append(f"{lane.what}: slot {slot} {c}.c{comp} = {images[c][comp]} is outside its class {cls.name}{where_outside(cls, images[c][comp], BITS)}")
                if stats is not None and slot not in (SLOT_NEG, SLOT_KEEP, SLOT_REC):
                    key = ("dbl" if slot == SLOT_DBL else "add", c)
                    stats[key] = max(stats.get(key, 0.0), abs(value_of(images[c][comp], BITS)) / P)
    given = lane.images["P"]
    # cneg(P, false) selects P: the very images; cneg(P, true) is g2h_neg: x and z the very images, y = carry(neg(y)) limb by limb
    if SLOT_KEEP in slots and any(list(slots[SLOT_KEEP][c][comp]) != list(given[c][comp]) for c in COORDS for comp in (0, 1)):
        bad.append(f"{lane.what}: slot {SLOT_KEEP} is not the image of P")
    if SLOT_NEG in slots:
        for c in COORDS:
            for comp in (0, 1):
                model = carry([-x for x in given[c][comp]]) if c == "y" else list(given[c][comp])
                if list(slots[SLOT_NEG][c][comp]) != model:
                    bad.append(f"{lane.what}: slot {SLOT_NEG} {c}.c{comp} is not {'carry(neg(y))' if c == 'y' else 'the image of P'}")
    # a record keeps limb images: wave_msm_get gives back exactly what wave_msm_put took
    if SLOT_REC in slots and SLOT_ADD in slots and slots[SLOT_REC] != slots[SLOT_ADD]:
        bad.append(f"{lane.what}: the point read back from its record is not the image that was stored")
    return bad


def check_all(lanes, all_slots, stats=None):
    assert len(lanes) == len(all_slots)
    bad = []
    for lane, slots in zip(lanes, all_slots):
        bad += check_lane(lane, slots, stats)
    return bad


def reimage(lane, rng):
    """the restatement's own results as slots: every expected point lifted under a random scale and imaged in its out-class"""
    slots = {}
    for slot, pt in expected(lane).items():
        xyz = lift(pt, (rng.randrange(1, P), rng.randrange(P)))
        images = {}
        for c in COORDS:
            pair = []
            for comp in (0, 1):
                cls, corner = out_class(slot, c), rng.choice(CORNERS)
                target = xyz[c][comp] * R % P
                kmin, kmax = k_range(cls, corner, target, P, BITS)
                pair.append(image_at(cls, corner, target + rng.randint(kmin, kmax) * P, BITS))
            images[c] = tuple(pair)
        slots[slot] = images
    given = lane.images["P"]
    slots[SLOT_REC] = {c: (list(v[0]), list(v[1])) for c, v in slots[SLOT_ADD].items()}
    slots[SLOT_KEEP] = {c: (list(v[0]), list(v[1])) for c, v in given.items()}
    slots[SLOT_NEG] = {c: tuple(carry([-x for x in im]) if c == "y" else list(im) for im in given[c]) for c in COORDS}
    return slots
