"""The input families of the bucket method under dr_te_msm (Ed25519, Baby JubJub, P-256, secp256k1, Curve25519) and dr_blsg1_msm
(BLS12-381's E(Fq)): csrc/wave_msm.hip.h from NARROW_PIP_FROM terms on.  Shared by test_narrow_msm_cpu.py, which proves on the host what
bucket lists they make, and test_gpu_narrow_msm.py, which runs them on the GPU.

The plan's restatement (Tiling, digits), the ladder's start and the heavy-list bound are wide_msm_cases'; the suites, the cases and the
families are restated here, because these curves differ where it matters: the 64-byte curves REDUCE every scalar mod the group order n
before its digits are read (so digits, lists and expectations are those of k mod n, and a small-order point T under k contributes
(k mod n) T), while E(Fq) takes its scalars as they are (a point Q outside G1 under k >= r contributes k Q).

Every point is a known multiple m G of the generator (a ladder a G, (a + 1) G, ...), the identity, a small-order point or such a Q, so
the expected value of a case is a closed form: one or two multiplications of the restatement, whatever the size."""
import os
import random
import re
import sys
from functools import lru_cache

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import babyjubjub_ref  # noqa: E402
import bls12_381_g1_ref  # noqa: E402
import curve25519_ref  # noqa: E402
import ed25519_ref  # noqa: E402
import p256_ref  # noqa: E402
import secp256k1_ref  # noqa: E402
from wide_msm_cases import HEAVY, LADDER_A, Tiling, digits  # noqa: E402,F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "dot_ring_amd", "csrc", "msm_plan.hpp")) as _f:
    _from = re.search(r"NARROW_PIP_FROM = (\d+)", _f.read())
FROM = int(_from.group(1)) if _from else 257     # (a tree without the constant: its tests then fail one by one, not at import)
TOP = 1 << 256                         # scalars are 32 bytes
# n -> (c, (W at 252, 254, 257 bits), H, index groups, families or None for all six)
PLANS = {
    FROM: (7, (36, 37, 37), 64, 1, None),
    1031: (7, (36, 37, 37), 64, 2, ("ladder", "equal", "edges")),
    4103: (8, (32, 32, 33), 128, 4, ("ladder", "equal", "edges")),
    16387: (9, (28, 29, 29), 256, 8, None),
    65539: (10, (26, 26, 26), 512, 16, ("ladder", "equal")),
}
LADDER = 4103


class Suite:
    """cv: the curve id dr_te_msm takes (None: dr_blsg1_msm); aliases: the other ids of the same group; bits: what the tiling covers;
    reduce: the path reduces scalars mod the order; identity: its spelling at the ABI; special: a small-order point (reduce) or a point
    outside G1 (E(Fq)) and the order of the former"""

    def __init__(self, name, ref, cv, aliases, bits, order, fe, identity, o, special, special_order=0):
        self.name, self.ref, self.cv, self.aliases, self.bits, self.order, self.fe = name, ref, cv, aliases, bits, order, fe
        self.identity, self.o, self.special, self.special_order = identity, o, special, special_order
        self.reduce = cv is not None

    def raw(self, pt):
        if pt is None or pt == self.o:
            return self.identity
        return pt[0].to_bytes(self.fe, "little") + pt[1].to_bytes(self.fe, "little")

    def red(self, k):
        return k % self.order if self.reduce else k


def _outside_g1():
    ref, x = bls12_381_g1_ref, 1
    while True:
        y = ref.sqrt((x**3 + ref.CURVE_B) % ref.P)
        if y is not None and (y * y - x**3 - ref.CURVE_B) % ref.P == 0 and ref.mul(ref.R_ORDER, (x, y)) is not None:
            return (x, y)
        x += 1


SUITES = {
    "ed25519": Suite("ed25519", ed25519_ref, 3, (10, 11), 254, ed25519_ref.N, 32, ed25519_ref.raw((0, 1)), (0, 1), ed25519_ref.torsion_points()[1], 8),
    "bjj": Suite("bjj", babyjubjub_ref, 5, (), 252, babyjubjub_ref.N, 32, babyjubjub_ref.raw((0, 1)), (0, 1), babyjubjub_ref.torsion_points()[1], 8),
    "p256": Suite("p256", p256_ref, 4, (8, 9), 257, p256_ref.N, 32, bytes(64), None, None),
    "secp256k1": Suite("secp256k1", secp256k1_ref, 6, (7,), 257, secp256k1_ref.N, 32, bytes(64), None, None),
    "curve25519": Suite("curve25519", curve25519_ref, 13, (14,), 254, ed25519_ref.N, 32, b"\xff" * 64, None, curve25519_ref.torsion_points()[1], 8),
    "blsg1": Suite("blsg1", bls12_381_g1_ref, None, (), 257, bls12_381_g1_ref.R_ORDER, 48, bytes(96), None, _outside_g1()),
}
NAMES = tuple(SUITES)


@lru_cache(maxsize=None)
def ladder(name):
    """(a + i) G for i < LADDER, by affine additions; term i of a larger case takes point i % LADDER"""
    ref = SUITES[name].ref
    pts = [ref.mul(LADDER_A, ref.G)]
    for _ in range(LADDER - 1):
        pts.append(ref.add(pts[-1], ref.G))
    return pts


@lru_cache(maxsize=None)
def _raw_ladder(name):
    s = SUITES[name]
    return [s.raw(pt) for pt in ladder(name)], [s.raw(s.ref.neg(pt)) for pt in ladder(name)]


class Case:
    """terms: (kind, value, scalar) with kind "m" (the ladder point of index value), "neg" (its negative), "id" (the identity) or
    "special" (the suite's small-order point, or on E(Fq) its point outside G1)"""

    def __init__(self, suite, family, n, terms, claims=None):
        self.suite, self.family, self.n, self.terms, self.claims = suite, family, n, terms, claims or {}
        self.name = f"{suite}-{family}-{n}"
        assert len(terms) == n and all(0 <= k < TOP for _, _, k in terms)

    @property
    def scalars(self):
        return [k for _, _, k in self.terms]

    def packed(self):
        s = SUITES[self.suite]
        pos, negs = _raw_ladder(self.suite)
        sp = s.raw(s.special) if s.special is not None else None
        pts = [pos[v] if kind == "m" else negs[v] if kind == "neg" else s.identity if kind == "id" else sp for kind, v, _ in self.terms]
        return b"".join(pts), b"".join(k.to_bytes(32, "little") for k in self.scalars)

    def expected(self):
        s = SUITES[self.suite]
        ref = s.ref
        total = sum(s.red(k) * (LADDER_A + v) * (1 if kind == "m" else -1) for kind, v, k in self.terms if kind in ("m", "neg")) % s.order
        out = ref.mul(total, ref.G) if total else s.o
        tors = sum(s.red(k) for kind, _, k in self.terms if kind == "special")
        if tors and s.reduce and tors % s.special_order:
            out = ref.add(out, ref.mul(tors % s.special_order, s.special))
        elif tors and not s.reduce:
            out = ref.add(out, ref.mul(tors, s.special))
        return s.raw(out)


def _rng(*key):
    return random.Random("narrow-msm/" + "/".join(str(x) for x in key))


def _full(rng):
    return rng.getrandbits(256)


def _below(rng, s):
    """well below the order: no reduction changes it, so its digits can be chosen"""
    return rng.getrandbits(s.order.bit_length() - 2)


def ladder_case(name, n, tag="ladder"):
    rng = _rng(name, tag, n)
    return Case(name, tag, n, [("m", i % LADDER, _full(rng)) for i in range(n)])


def equal_case(name, n):
    """one scalar for all terms over a pool of 16 points: every window has one list per index group, of all its terms"""
    s, rng = SUITES[name], _rng(name, "equal", n)
    k = _below(rng, s) | 1 << (s.order.bit_length() - 3)
    t = Tiling(n, s.bits)
    return Case(name, "equal", n, [("m", i % 16, k) for i in range(n)], {"lengths": sorted({-(-(g + 1) * n // t.groups) - -(-g * n // t.groups) for g in range(t.groups)})})


def lengths_case(name, n):
    """64 terms with one scalar whose lowest digit is 1, 65 with one whose lowest digit is 2, and distinct scalars whose lowest digit is 3
    or more: in window 0 of index group 0, bucket 0 has exactly 64 entries and bucket 1 exactly 65"""
    s, rng = SUITES[name], _rng(name, "lengths", n)
    t = Tiling(n, s.bits)
    w0 = t.widths[0]
    low = lambda k, d: (k >> (w0 + 1) << (w0 + 1)) | d                      # window 0 = d, the bit above it clear
    k1, k2 = low(_below(rng, s), 1), low(_below(rng, s), 2)
    terms = [("m", i, k1) for i in range(64)] + [("m", i, k2) for i in range(64, 129)]
    terms += [("m", i % LADDER, low(_below(rng, s), rng.randrange(3, 1 << (w0 - 1)))) for i in range(129, n)]
    assert n // t.groups >= 129
    return Case(name, "lengths", n, terms)


def cancel_case(name, n, identity_total):
    """(P, -P) pairs under one scalar and (P, P) repeats; identity_total: nothing but such pairs (and, where n is odd, one identity point
    under a full-width scalar), whose sum is the identity"""
    s, rng = SUITES[name], _rng(name, "cancel", n, identity_total)
    if identity_total:
        terms = []
        for j in range(n // 2):
            k = _full(rng) if j >= 40 else 0x1234567 + (1 << (s.order.bit_length() - 3))     # 40 pairs share one scalar: lists of 80
            terms += [("m", j % LADDER, k), ("neg", j % LADDER, k)]
        if n % 2:
            terms.append(("id", 0, _full(rng)))
        return Case(name, "cancel-identity", n, terms)
    u, v = _full(rng), _full(rng)
    terms = []
    for j in range(65):
        terms += [("m", j, u), ("neg", j, u)]                  # 130 terms of one scalar that sum to the identity
    terms += [("m", 7, v)] * 100                               # one point a hundred times
    terms += [("m", i % LADDER, _full(rng)) for i in range(len(terms), n)]
    return Case(name, "cancel-mixed", n, terms)


def nibbles(digit):
    return int(("%x" % digit) * 64, 16)


def edge_scalars(s):
    return [0, 1, s.order - 1, s.order, s.order + 1, TOP - 1, nibbles(7), nibbles(8)]


def edges_case(name, n):
    s, rng = SUITES[name], _rng(name, "edges", n)
    terms = [("m", i, k) for i, k in enumerate(edge_scalars(s))]
    terms += [("id", 0, k) for k in (0, 1, TOP - 1, _full(rng))]
    if s.special is not None:
        # every scalar at or above the order: on the cofactor curves (k mod n) T is not k T, on E(Fq) k Q is not (k mod r) Q
        ks = [s.order, s.order + 1, TOP - 1, _full(rng) | 1 << 255]
        if s.reduce:       # the total must not vanish, and leaving the scalars unreduced must change it: the last scalar is chosen for that
            good = lambda v: sum(k % s.order for k in v) % s.special_order not in (0, sum(v) % s.special_order)
            ks.append(next(q * s.order + r for q in (1, 2, 3) for r in (2, 3, 5) if good(ks + [q * s.order + r])))
        else:
            ks.append(2 * s.order + 3)
        assert all(s.order <= k < TOP for k in ks)
        terms += [("special", 0, k) for k in ks]
    terms += [("m", i % LADDER, _full(rng)) for i in range(len(terms), n - 2)]
    terms += [("id", 0, _full(rng)), ("m", (n - 1) % LADDER, TOP - 1)]
    return Case(name, "edges", n, terms)


FAMILIES = ("ladder", "equal", "lengths", "cancel-mixed", "cancel-identity", "edges")


def build(name, family, n):
    """a case that nobody keeps: the large ones are megabytes of terms"""
    return {"ladder": ladder_case, "equal": equal_case, "lengths": lengths_case, "edges": edges_case,
            "cancel-mixed": lambda a, b: cancel_case(a, b, False), "cancel-identity": lambda a, b: cancel_case(a, b, True)}[family](name, n)


def plan_families(n):
    return PLANS[n][4] or FAMILIES


def plan_keys():
    """(suite, family, n) of every case"""
    return [(name, family, n) for name in NAMES for n in PLANS for family in plan_families(n)]
