"""The input families of the wide suites' bucket method (dr_wide_msm: csrc/wave_msm.hip.h), shared by test_wide_msm_plan_cpu.py, which
proves on the host what bucket lists they make, and test_gpu_wide_msm.py and test_gpu_wide_msm_plans.py, which run them on the GPU.

Every point is a known multiple m G of the suite's generator (a ladder a G, (a + 1) G, ... built by affine additions), the identity, or
a small-order point Q, so the expected value of a case is the closed form (sum k_i m_i mod n) G + (sum of Q's scalars mod ord Q) Q: one
or two multiplications of the restatement (p384_ref, p521_ref, ed448_ref, curve448_ref), whatever the size."""
import os
import random
import re
import sys
from functools import lru_cache

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import curve448_ref  # noqa: E402
import ed448_ref  # noqa: E402
import p384_ref  # noqa: E402
import p521_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "dot_ring_amd", "csrc", "msm_plan.hpp")) as _f:
    _plan = _f.read()
FROM = int(re.search(r"WIDE_PIP_FROM = (\d+)", _plan).group(1))
HEAVY = int(re.search(r"TE_HEAVY_BUCKET = (\d+)", _plan).group(1))
SIZES = (FROM, 1030, 4100)            # one index group, two, and the second window width
# The upper half of the plan (test_gpu_wide_msm_plans.py): n -> (c, (W at 385, 449, 522 bits), H, index groups, families).  No size is a
# multiple of its group count, so every group bound is a ceiling that differs from the floor.  1031 and 4103: the plans of 1030 and 4100
# with a remainder; 16383 and 65535: the densest windows of widths 8 and 9 (one below a threshold); 16387 and 65539: widths 9 and 10, the
# second with two bins per lane of the sort; 131075: 32 index groups; 262147: the cap of 64
PLANS = {
    1031: (7, (55, 65, 75), 64, 2, ("ladder", "equal", "edges")),
    4103: (8, (49, 57, 66), 128, 4, ("ladder", "equal", "edges")),
    16383: (8, (49, 57, 66), 128, 8, None),
    16387: (9, (43, 50, 58), 256, 8, None),
    65535: (9, (43, 50, 58), 256, 16, ("ladder", "equal")),
    65539: (10, (39, 45, 53), 512, 16, None),
    131075: (10, (39, 45, 53), 512, 32, ("ladder", "equal")),
    262147: (10, (39, 45, 53), 512, 64, ("ladder", "equal")),
}


class Suite:
    def __init__(self, name, ref, bits, nbytes, identity, small=None, small_order=1):
        self.name, self.ref, self.bits, self.nbytes, self.identity = name, ref, bits, nbytes, identity
        self.order = ref.N
        self.top = 1 << (bits - 1)                       # scalars are below this
        self.small, self.small_order = small, small_order

    def raw(self, pt):
        return self.identity if pt is None or pt == getattr(self.ref, "O", None) else self.ref.raw(pt)

    @property
    def words(self):
        return self.nbytes // 4


SUITES = {
    "p384": Suite("p384", p384_ref, 385, 48, bytes(96)),
    "p521": Suite("p521", p521_ref, 522, 68, bytes(136)),
    "ed448": Suite("ed448", ed448_ref, 449, 56, ed448_ref.raw((0, 1)), small=(1, 0), small_order=4),
    "curve448": Suite("curve448", curve448_ref, 449, 56, b"\xff" * 112, small=(0, 0), small_order=2),
}
NAMES = tuple(SUITES)


# ---------------------------------------------------------------- the plan, restated (msm_plan.hpp: plan_wide_msm)
class Tiling:
    def __init__(self, n, bits):
        self.c = 7 if n < 4096 else 8 if n < 16384 else 9 if n < 65536 else 10
        self.W = -(-bits // self.c)
        base, rem = divmod(bits, self.W)
        self.widths = [base + (1 if w >= self.W - rem else 0) for w in range(self.W)]
        self.starts = [sum(self.widths[:w]) for w in range(self.W)]
        self.cmax = max(self.widths)
        self.H = 1 << (self.cmax - 1)
        self.groups = 1
        while self.groups < 64 and n // (self.groups * 2 * self.H) >= 8:
            self.groups *= 2


def digits(k, t):
    """Booth's signed digits (wide_recode.hip.h: wide_digit)"""
    out = []
    for s, w in zip(t.starts, t.widths):
        v = ((k << 1) >> s) & ((1 << (w + 1)) - 1)
        out.append((v >> 1) + (v & 1) - (((v >> w) & 1) << w))
    return out


# ---------------------------------------------------------------- points
LADDER_A = 0x5EED0123456789ABCDEF


@lru_cache(maxsize=None)
def ladder(name):
    """(a + i) G for i < 4100, by affine additions; term i of a larger case takes point i % 4100"""
    ref = SUITES[name].ref
    pts = [ref.mul(LADDER_A, ref.G)]
    for _ in range(max(SIZES) - 1):
        pts.append(ref.add(pts[-1], ref.G))
    return pts


@lru_cache(maxsize=None)
def _raw_ladder(name):
    return [SUITES[name].raw(pt) for pt in ladder(name)]


class Case:
    """terms: (kind, value, scalar) with kind "m" (the ladder point of index value), "neg" (its negative), "id" (the identity) or
    "small" (the suite's small-order point)"""

    def __init__(self, suite, family, n, terms, claims=None):
        self.suite, self.family, self.n, self.terms, self.claims = suite, family, n, terms, claims or {}
        self.name = f"{suite}-{family}-{n}"
        assert len(terms) == n and all(0 <= k < SUITES[suite].top for _, _, k in terms)

    @property
    def scalars(self):
        return [k for _, _, k in self.terms]

    def packed(self):
        s = SUITES[self.suite]
        lad, raws, ref = ladder(self.suite), _raw_ladder(self.suite), s.ref
        pts = []
        for kind, v, _ in self.terms:
            pts.append(raws[v] if kind == "m" else s.raw(ref.neg(lad[v])) if kind == "neg" else s.identity if kind == "id" else s.raw(s.small))
        return b"".join(pts), b"".join(k.to_bytes(s.nbytes, "little") for k in self.scalars)

    def expected(self):
        s = SUITES[self.suite]
        ref = s.ref
        total = sum(k * (LADDER_A + v) * (1 if kind == "m" else -1) for kind, v, k in self.terms if kind in ("m", "neg")) % s.order
        out = ref.mul(total, ref.G) if total else getattr(ref, "O", None)
        tors = sum(k for kind, _, k in self.terms if kind == "small")
        if s.small is not None and tors % s.small_order:
            out = ref.add(out, ref.mul(tors % s.small_order, s.small))
        return s.raw(out)


LADDER = max(SIZES)


def _rng(*key):
    return random.Random("wide-msm/" + "/".join(str(x) for x in key))


def _full(rng, s):
    return rng.getrandbits(s.bits - 1)


def ladder_case(name, n, tag="ladder"):
    s, rng = SUITES[name], _rng(name, tag, n)
    return Case(name, tag, n, [("m", i % LADDER, _full(rng, s)) for i in range(n)])


def equal_case(name, n):
    """one scalar for all terms over a pool of 16 points: every window has one list per index group, of all its terms"""
    s, rng = SUITES[name], _rng(name, "equal", n)
    k = _full(rng, s) | 1 << (s.bits - 2)
    t = Tiling(n, s.bits)
    return Case(name, "equal", n, [("m", i % 16, k) for i in range(n)], {"lengths": sorted({-(-(g + 1) * n // t.groups) - -(-g * n // t.groups) for g in range(t.groups)})})


def lengths_case(name, n):
    """64 terms with one scalar whose lowest digit is 1, 65 with one whose lowest digit is 2, and distinct scalars whose lowest digit is 3
    or more: in window 0 of index group 0, bucket 0 has exactly 64 entries and bucket 1 exactly 65"""
    s, rng = SUITES[name], _rng(name, "lengths", n)
    t = Tiling(n, s.bits)
    w0 = t.widths[0]
    low = lambda k, d: (k >> (w0 + 1) << (w0 + 1)) | d                      # window 0 = d, the bit above it clear
    k1, k2 = low(_full(rng, s), 1), low(_full(rng, s), 2)
    terms = [("m", i, k1) for i in range(64)] + [("m", i, k2) for i in range(64, 129)]
    terms += [("m", i % LADDER, low(_full(rng, s), rng.randrange(3, 1 << (w0 - 1)))) for i in range(129, n)]
    assert n // t.groups >= 129
    return Case(name, "lengths", n, terms)


def cancel_case(name, n, identity_total):
    """(P, -P) pairs under one scalar and (P, P) repeats; identity_total: nothing but such pairs (and, where n is odd, one identity point
    under a full-width scalar), whose sum is the identity"""
    s, rng = SUITES[name], _rng(name, "cancel", n, identity_total)
    if identity_total:
        terms = []
        for j in range(n // 2):
            k = _full(rng, s) if j >= 40 else 0x1234567 + (1 << (s.bits - 3))     # 40 pairs share one scalar: lists of 80
            terms += [("m", j % LADDER, k), ("neg", j % LADDER, k)]
        if n % 2:
            terms.append(("id", 0, _full(rng, s)))
        return Case(name, "cancel-identity", n, terms)
    u, v = _full(rng, s), _full(rng, s)
    terms = []
    for j in range(65):
        terms += [("m", j, u), ("neg", j, u)]                  # 130 terms of one scalar that sum to the identity
    terms += [("m", 7, v)] * 100                               # one point a hundred times
    terms += [("m", i % LADDER, _full(rng, s)) for i in range(len(terms), n)]
    return Case(name, "cancel-mixed", n, terms)


def nibbles(s, digit):
    return int(("%x" % digit) * (-(-(s.bits - 1) // 4)), 16) & (s.top - 1)


def edge_scalars(s):
    return [0, 1, s.order - 1, s.order, s.order + 1, s.top - 1, nibbles(s, 7), nibbles(s, 8)]


def edges_case(name, n):
    s, rng = SUITES[name], _rng(name, "edges", n)
    terms = [("m", i, k) for i, k in enumerate(edge_scalars(s))]
    terms += [("id", 0, k) for k in (0, 1, s.top - 1, _full(rng, s))]
    if s.small is not None:
        ks = [s.order, s.order + 1, s.top - 1, _full(rng, s) | 1 << (s.bits - 2)]
        # the total must not vanish, and a reduction mod n of each scalar must change it: the last scalar is chosen for that
        good = lambda v: sum(v) % s.small_order and sum(k % s.order for k in v) % s.small_order != sum(v) % s.small_order
        ks.append(next(q * s.order + r for q in (1, 2, 3) for r in (2, 3) if good(ks + [q * s.order + r])))
        assert all(k >= s.order for k in ks) and sum(ks) % s.small_order and sum(k % s.order for k in ks) % s.small_order != sum(ks) % s.small_order
        terms += [("small", 0, k) for k in ks]
    terms += [("m", i % LADDER, _full(rng, s)) for i in range(len(terms), n - 2)]
    terms += [("id", 0, _full(rng, s)), ("m", (n - 1) % LADDER, s.top - 1)]
    return Case(name, "edges", n, terms)


FAMILIES = ("ladder", "equal", "lengths", "cancel-mixed", "cancel-identity", "edges")


def build(name, family, n):
    """a case that nobody keeps: the large ones are tens of megabytes of terms"""
    return {"ladder": ladder_case, "equal": equal_case, "lengths": lengths_case, "edges": edges_case,
            "cancel-mixed": lambda a, b: cancel_case(a, b, False), "cancel-identity": lambda a, b: cancel_case(a, b, True)}[family](name, n)


case = lru_cache(maxsize=None)(build)


def plan_families(n):
    return PLANS[n][4] or FAMILIES


def plan_keys():
    """(suite, family, n) of every case of PLANS"""
    return [(name, family, n) for name in NAMES for n in PLANS for family in plan_families(n)]


def all_cases():
    return [case(name, family, n) for name in NAMES for n in SIZES for family in FAMILIES]
