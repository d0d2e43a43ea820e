"""The inputs of the G2 sums of scalar multiples (dr_blsg2_msm, dr_blsg2_msm_groups, Bls12381G2Point.msm): BLS12-381's E(Fq2) as one
more suite of narrow_msm_cases.py, whose Case and family builders run over it unchanged — the curve takes its 32-byte scalars as they
are, like E(Fq), over 257 tiled bits.  The suite is registered in a PRIVATE instance of that module (loaded from its file under a name
of its own), so the suite table the narrow tests iterate is what it was, whatever is imported beside them.  Shared by
test_g2_msm_cpu.py, which proves on the host what bucket lists the families make, and test_gpu_g2_msm.py, which runs them on the GPU.

Every point is a known multiple (a + i) G of G2's generator, the identity (192 zero bytes) or `special`, a point Q of E(Fq2) outside G2
(k Q with k >= r differs from (k mod r) Q), so the expected value of a case is a closed form of the big-integer restatement
bls12_381_g2_ref.py: one or two multiplications, whatever the size."""
import importlib.util
import os
import re
import sys
from collections import Counter

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bls12_381_g2_ref as g2  # noqa: E402

_spec = importlib.util.spec_from_file_location("g2_private_narrow_msm_cases", os.path.join(os.path.dirname(os.path.abspath(__file__)), "narrow_msm_cases.py"))
cases = importlib.util.module_from_spec(_spec)           # narrow_msm_cases.py's code with a suite table of its own
_spec.loader.exec_module(cases)
FAMILIES, HEAVY, LADDER, LADDER_A, TOP = cases.FAMILIES, cases.HEAVY, cases.LADDER, cases.LADDER_A, cases.TOP
Case, Tiling, build, digits, ladder, ladder_case = cases.Case, cases.Tiling, cases.build, cases.digits, cases.ladder, cases.ladder_case

NAME = "blsg2"
BITS = 257                                # what the tiling covers: one bit more than a 32-byte scalar can have
ORDER_E = g2.H2 * g2.R_ORDER              # #E(Fq2): the exponent of every point


def _threshold():
    """BLSG2_PIP_FROM of csrc/msm_plan.hpp: a number, or the name of another constant of that file"""
    with open(os.path.join(cases.ROOT, "dot_ring_amd", "csrc", "msm_plan.hpp")) as f:
        text = f.read()
    found = re.search(r"BLSG2_PIP_FROM = (\w+)", text)
    if not found:
        return 257                        # (a tree without the constant: its tests then fail one by one, not at import)
    value = found.group(1)
    return int(value) if value.isdigit() else int(re.search(value + r" = (\d+)", text).group(1))


FROM = _threshold()
# n -> (c, W, H, index groups, families): the threshold with all six, two uneven groups, width 8 with four groups, width 9 with eight.
# Width 10 and 16 groups are plan and sort code that E(Fq2) shares unchanged with E(Fq); test_gpu_narrow_msm.py runs them there.
PLANS = {
    FROM: (7, 37, 64, 1, FAMILIES),
    1031: (7, 37, 64, 2, ("ladder", "equal", "edges")),
    4103: (8, 33, 128, 4, ("ladder", "cancel-mixed")),
    16387: (9, 29, 256, 8, ("ladder",)),
}


def raw_fp2(a):
    return a[0].to_bytes(48, "little") + a[1].to_bytes(48, "little")


def raw(pt):
    """x || y, each c0 || c1, 4 x 48 bytes little-endian; the identity is 192 zero bytes"""
    return bytes(192) if pt is None else raw_fp2(pt[0]) + raw_fp2(pt[1])


def point_of(b):
    if b == bytes(192):
        return None
    v = [int.from_bytes(b[i : i + 48], "little") for i in range(0, 192, 48)]
    return (v[0], v[1]), (v[2], v[3])


def outside_g2():
    """the first point (x, y) with x = 1 + j i, j = 0, 1, ..., whose x^3 + 4 (1 + i) is a square and which r does not kill"""
    j = 0
    while True:
        x = (1, j)
        y = g2.f2_sqrt(g2.f2_add(g2.f2_mul(g2.f2_sqr(x), x), g2.CURVE_B))
        if y is not None and g2.mul(g2.R_ORDER, (x, y)) is not None:
            return x, y
        j += 1


class G2Suite(cases.Suite):
    def raw(self, pt):
        return raw(pt)


SPECIAL = outside_g2()
SUITE = G2Suite(NAME, g2, None, (), BITS, g2.R_ORDER, 96, bytes(192), None, SPECIAL)
# Case and the family builders look their suite up by name, in the private instance's table
cases.SUITES[NAME] = SUITE


def plan_keys():
    """(family, n) of every case"""
    return [(family, n) for n, plan in PLANS.items() for family in plan[4]]


def lists(case):
    """{(window, index group, bucket): (entries, negative entries)} of a case's scalars under its plan, by Tiling / digits — the
    restatement of what k_blsg2_msm_sort makes"""
    t = Tiling(case.n, BITS)
    bounds = [-(-g * case.n // t.groups) for g in range(t.groups + 1)]
    total, negative = Counter(), Counter()
    g = 0
    for i, k in enumerate(case.scalars):
        while i >= bounds[g + 1]:
            g += 1
        for w, d in enumerate(digits(k, t)):
            if d:
                total[(w, g, abs(d) - 1)] += 1
                negative[(w, g, abs(d) - 1)] += d < 0
    return {key: (count, negative[key]) for key, count in total.items()}
