"""CPU: the host side of the G2 sums of scalar multiples (dr_blsg2_msm, Bls12381G2Point.msm) and the inputs of their GPU tests.
dr::G2hLaw (csrc/g2_law.hpp) and dr::wide_combine over it run from the library's own headers, compiled for the host under the
undefined-behaviour sanitizer as a stand-alone program (tests/native/g2_msm_host_check.cpp), against the big-integer restatement
bls12_381_g2_ref.py.  Bls12381G2Point._terms runs with the context replaced by a stub that answers from the restatement.  The case
module g2_msm_cases.py is held to its own claims by Tiling / digits, and the lanes and the checker of g2_law_images.py to theirs — so
what test_gpu_g2_msm.py and test_gpu_g2_law.py run on the GPU is proved here to be what they say it is."""
import math
import os
import random
import struct
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bls12_381_g2_ref as g2  # noqa: E402
import g2_law_images as L  # noqa: E402
import g2_msm_cases as cases  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("g2_msm") / "g2_msm_host_check"
    subprocess.run(["g++", "-O2", "-std=c++20", "-fsanitize=undefined", "-fno-sanitize-recover", "-Wno-psabi", "-I", os.path.join(ROOT, "dot_ring_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "g2_msm_host_check.cpp"), "-o", str(out)], check=True)
    return str(out)


def test_threshold_and_plans(exe):
    from dot_ring_amd import _native

    proc = subprocess.run([exe], capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr
    lines = proc.stdout.splitlines()
    assert lines[0] == f"from {cases.FROM}" and _native.BLSG2_PIP_FROM == cases.FROM >= 257
    assert cases.BITS == 256 + 1 and cases.SUITE.reduce is False and cases.TOP == 1 << 256
    assert "dr_blsg2_msm" in _native.EXPORTED_SYMBOLS and "dr_blsg2_msm_groups" in _native.EXPORTED_SYMBOLS and "dr_blsg2_law_selftest" in _native.EXPORTED_SYMBOLS
    for line, (n, (c, W, H, groups, _)) in zip(lines[1:], cases.PLANS.items()):
        t = cases.Tiling(n, cases.BITS)
        assert (t.c, t.W, t.H, t.groups, t.cmax) == (c, W, H, groups, c)
        assert line == f"plan n={n} c={c} W={W} H={H} groups={groups} sets={W * groups}"
        assert n == cases.FROM or n % groups


# ---------------------------------------------------------------- the host law
def _law_points():
    hashed = g2.encode_to_curve_ro(b"g2 msm host law")
    assert g2.in_g2(g2.G) and g2.in_g2(hashed) and g2.on_curve(cases.SPECIAL) and not g2.in_g2(cases.SPECIAL)
    return g2.G, hashed, cases.SPECIAL


def test_host_law_equals_the_restatement(exe, tmp_path):
    """the generator, a hashed point, a point outside G2, ladder points; equal points, inverse pairs and the identity on either side —
    add, dbl and their sum through from_abi and to_abi"""
    G, hashed, special = _law_points()
    lad = cases.ladder(cases.NAME)[:8]
    named = [G, hashed, special, g2.neg(special), g2.add(special, G)]
    rng = random.Random("g2-msm/law")
    pairs = [(a, b) for a in named for b in named]                                            # equal points and (special, -special) among them
    pairs += [(rng.choice(lad), rng.choice(lad + named)) for _ in range(12)]
    pairs += [(p, p) for p in lad[:2]] + [(p, g2.neg(p)) for p in (G, hashed, lad[0])]
    pairs += [(None, G), (G, None), (None, special), (special, None), (None, None)]
    path = tmp_path / "law.txt"
    path.write_text("".join(f"{cases.raw(a).hex()} {cases.raw(b).hex()}\n" for a, b in pairs))
    proc = subprocess.run([exe, "law", str(path)], capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr
    got = [line.split() for line in proc.stdout.splitlines()]
    want = []
    for a, b in pairs:
        sm, db = g2.add(a, b), g2.add(a, a)
        want.append([cases.raw(sm).hex(), cases.raw(db).hex(), cases.raw(g2.add(sm, db)).hex()])
    assert got == want
    assert bytes(192).hex() in {w for row in want for w in row}
    assert want[-1] == [bytes(192).hex()] * 3                                                 # 192 zero bytes in, 192 zero bytes out


def test_malformed_input_is_refused(exe, tmp_path):
    path = tmp_path / "bad.txt"
    path.write_text("00 11\n")
    assert subprocess.run([exe, "law", str(path)], capture_output=True, text=True).returncode == 2
    path.write_text("sums 257\n" + "00" * 192 + "\n")
    assert subprocess.run([exe, "combine", str(path)], capture_output=True, text=True).returncode == 2


def test_host_combine_equals_the_restatement(exe, tmp_path):
    """set sums m G (ladder points, some negated, some the identity, and the special point in some sets) for the plans of 257, 1031
    and 4103 terms at 257 bits: the program's combination is (sum_w 2^start_w sum_g m_wg) G + (sum of the special sets' weights) Q"""
    lad = cases.ladder(cases.NAME)
    rng = random.Random("g2-msm/combine")
    blocks, want = [], []
    for n in (257, 1031, 4103, "identity"):
        t = cases.Tiling(257 if n == "identity" else n, cases.BITS)
        total, outside, lines = 0, 0, []
        for w in range(t.W):
            for g in range(t.groups):
                kind = "id" if n == "identity" else rng.choice(["m", "m", "m", "neg", "id", "special"])
                i = rng.randrange(len(lad))
                pt = None if kind == "id" else cases.SPECIAL if kind == "special" else lad[i] if kind == "m" else g2.neg(lad[i])
                total += (0 if kind in ("id", "special") else (cases.LADDER_A + i) * (1 if kind == "m" else -1)) << t.starts[w]
                outside += (kind == "special") << t.starts[w]
                lines.append(cases.raw(pt).hex())
        blocks.append(f"sums {257 if n == 'identity' else n}\n" + "\n".join(lines) + "\n")
        want.append(cases.raw(g2.add(g2.mul(total % g2.R_ORDER, g2.G), g2.mul(outside % cases.ORDER_E, cases.SPECIAL))).hex())
    path = tmp_path / "sums.txt"
    path.write_text("".join(blocks))
    proc = subprocess.run([exe, "combine", str(path)], capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr
    assert proc.stdout.split() == want and want[-1] == bytes(192).hex() and len(set(want)) == 4


# ---------------------------------------------------------------- Bls12381G2Point._terms
class _StubContext:
    """answers blsg2_scalar_mul_batch from the restatement and counts the calls"""

    def __init__(self):
        self.calls = []

    def blsg2_scalar_mul_batch(self, pts, ks):
        n = len(ks) // 96
        assert len(pts) == 192 * n and len(ks) == 96 * n
        self.calls.append(n)
        return b"".join(cases.raw(g2.mul(int.from_bytes(ks[96 * i : 96 * i + 96], "little"), cases.point_of(pts[192 * i : 192 * i + 192]))) for i in range(n))


TERM_SCALARS = (0, 1, g2.R_ORDER, (1 << 256) - 1, 1 << 256, 1 << 512, (1 << 768) - 1, (1 << 770) + 12345, -5)


def _as_ref(pt):
    return None if pt.is_identity() else ((pt.x.re, pt.x.im), (pt.y.re, pt.y.im))


def test_terms_keep_the_sum_below_2_256(monkeypatch):
    """scalars 0, 1, r, 2^256 - 1, 2^256, 2^512, 2^768 - 1, 2^770 + 12345 and -5 over the generator and over a point outside G2: every
    scalar of the terms is below 2^256, the terms sum to k P, and the shifted points of all wide scalars come from ONE batch"""
    import dot_ring_amd as d
    from dot_ring_amd import curve

    pt_type = d.BLS12_381_G2.point_type
    assert pt_type._COFACTOR == g2.H2 and pt_type._N == g2.R_ORDER and pt_type._H == g2.H_EFF
    # the argument of valid_points' docstring
    assert g2.H_EFF % g2.H2 == 0 and math.gcd(g2.H_EFF, g2.R_ORDER) == 1 and g2.H2 % g2.R_ORDER != 0
    stub = _StubContext()
    monkeypatch.setattr(curve.runtime, "context", lambda: stub)
    for base in (g2.G, cases.SPECIAL):
        P = pt_type(*base)
        for k in TERM_SCALARS:
            pts, ks = pt_type._terms([P], [k])
            assert len(pts) == len(ks) and all(0 <= v < 1 << 256 for v in ks)
            acc = None
            for pt, v in zip(pts, ks):
                acc = g2.add(acc, g2.mul(v, _as_ref(pt)))
            assert acc == g2.mul(k % cases.ORDER_E, base) == g2.mul(k, base), k
    # the splits: one term below 2^256, two below 2^512, three from there on (2^768 - 1 and 2^770 + 12345 exceed #E(Fq2) and are reduced)
    count = lambda k: len(pt_type._terms([pt_type(*g2.G)], [k])[0])
    assert [count(k) for k in TERM_SCALARS] == [1, 1, 1, 1, 2, 3, 3, 3, 3]
    stub.calls.clear()
    P, Q = pt_type(*g2.G), pt_type(*cases.SPECIAL)
    pts, ks = pt_type._terms([P, Q] * len(TERM_SCALARS), [k for k in TERM_SCALARS for _ in (0, 1)])
    assert stub.calls == [2 * (1 + 2 + 2 + 2 + 2)] and len(pts) == 2 * sum([1, 1, 1, 1, 2, 3, 3, 3, 3])
    want = None
    for k in TERM_SCALARS:
        want = g2.add(want, g2.add(g2.mul(k, g2.G), g2.mul(k, cases.SPECIAL)))
    acc = None
    for pt, v in zip(pts, ks):
        acc = g2.add(acc, g2.mul(v, _as_ref(pt)))
    assert acc == want
    stub.calls.clear()
    assert pt_type._terms([P, pt_type.identity()], [5, 7])[1] == [5, 7] and stub.calls == []


# ---------------------------------------------------------------- the case module's own claims
@pytest.mark.parametrize("family,n", cases.plan_keys())
def test_case_sizes_and_scalars(family, n):
    case = cases.build(cases.NAME, family, n)
    assert case.n == n == len(case.terms) and all(0 <= k < 1 << 256 for k in case.scalars)
    pts, ks = case.packed()
    assert len(pts) == 192 * n and len(ks) == 32 * n and len(case.expected()) == 192
    t = cases.Tiling(n, cases.BITS)
    for k in case.scalars[:: max(1, n // 64)]:
        ds = cases.digits(k, t)
        assert sum(dg << st for dg, st in zip(ds, t.starts)) == k and all(abs(dg) <= 1 << (w - 1) for dg, w in zip(ds, t.widths))
    if family == "ladder":           # the seeded ladder scalars make no heavy list: their GPU runs are the per-lane walk alone
        assert max(v[0] for v in cases.lists(case).values()) < cases.HEAVY
    if family == "cancel-identity":
        assert case.expected() == bytes(192)


def test_families_cover_what_they_claim():
    s = cases.SUITE
    assert [(f, n) for f, n in cases.plan_keys() if n == cases.FROM] == [(f, cases.FROM) for f in cases.FAMILIES] and len(cases.FAMILIES) == 6
    assert {n: fams for n, (_, _, _, _, fams) in cases.PLANS.items() if n != cases.FROM} == \
        {1031: ("ladder", "equal", "edges"), 4103: ("ladder", "cancel-mixed"), 16387: ("ladder",)}
    # lengths: lists of exactly 64 and 65 entries in window 0 of the one index group, on either side of the hand-over between the kernels
    lengths = cases.lists(cases.build(cases.NAME, "lengths", cases.FROM))
    assert lengths[(0, 0, 0)] == (64, 0) and lengths[(0, 0, 1)] == (65, 0) and cases.HEAVY == 64
    assert sum(1 for v in lengths.values() if v[0] > cases.HEAVY) >= cases.PLANS[cases.FROM][1] - 1
    # the cancelling families have heavy lists too
    for family in ("cancel-mixed", "cancel-identity"):
        assert any(v[0] > cases.HEAVY for v in cases.lists(cases.build(cases.NAME, family, cases.FROM)).values())
    mixed = cases.lists(cases.build(cases.NAME, "cancel-mixed", 4103))
    assert any(v[0] >= 130 for v in mixed.values()) and any(100 <= v[0] < 130 for v in mixed.values())
    # edges: the eight edge scalars, five identities, five special terms with scalars at or above r
    edges = cases.build(cases.NAME, "edges", cases.FROM)
    assert edges.scalars[:8] == [0, 1, s.order - 1, s.order, s.order + 1, (1 << 256) - 1, int("7" * 64, 16), int("8" * 64, 16)]
    special = [t[2] for t in edges.terms if t[0] == "special"]
    assert len(special) == 5 and all(k >= s.order for k in special) and sum(1 for t in edges.terms if t[0] == "id") == 5
    assert g2.mul(sum(special), cases.SPECIAL) != g2.mul(sum(special) % s.order, cases.SPECIAL)          # reducing mod r would show


@pytest.mark.parametrize("n", (cases.FROM, 1031))
def test_equal_has_one_heavy_list_per_digit_and_group(n):
    case = cases.build(cases.NAME, "equal", n)
    t = cases.Tiling(n, cases.BITS)
    ds = cases.digits(case.scalars[0], t)
    got = cases.lists(case)
    assert len(set(case.scalars)) == 1 and case.scalars[0] < cases.SUITE.order
    assert sorted(got) == sorted((w, g, abs(d) - 1) for w, d in enumerate(ds) if d for g in range(t.groups))
    assert all(count > cases.HEAVY and neg == (count if ds[w] < 0 else 0) for (w, _, _), (count, neg) in got.items())
    assert sorted({count for count, _ in got.values()}) == case.claims["lengths"] == {cases.FROM: [cases.FROM], 1031: [515, 516]}[n]


# ---------------------------------------------------------------- the lanes of the law and their checker
def test_lanes_sit_at_the_corners_of_the_documented_classes():
    pool = L.pool()
    assert len(pool.lanes) >= 70 and len({lane.what for lane in pool.lanes}) == len(pool.lanes)
    p = g2.P
    # the classes as the headers give them
    assert [c.name for c in L.IN_CLASSES] == ["n", "c2.1", "c3"] and L.C3.vhi == 3 * p and L.C3.vlo == -3 * p
    assert all(c.lo[:13] == [0] * 13 and c.hi[:13] == [(1 << 28) - 1] * 13 for c in (L.N, L.C21, L.C29, L.C3))
    assert L.N.vlo < -(4 * p // 10) and L.N.vhi > 14 * p // 10 and L.C29.vhi < L.C3.vhi and L.ONE_IMAGE == g2.limbs(g2.MONT_R % p)
    for lane in pool.lanes:
        for who, pt in (("P", lane.P), ("Q", lane.Q)):
            assert g2.on_curve(pt)
            xyz = {}
            for c in L.COORDS:
                for image in lane.images[who][c]:
                    assert len(image) == 14 and L.C3.contains(image, 28) and all(-(1 << 31) <= x < 1 << 31 for x in image)
                xyz[c] = tuple(L.residue(image) for image in lane.images[who][c])
            assert L.same_point(xyz, pt), lane.what
    # every component of both operands reached every corner of every class at both ends of its range
    want = {(who, c, comp, cls.name, corner, end) for who in "PQ" for c in L.COORDS for comp in (0, 1) for cls in L.IN_CLASSES
            for corner in L.CORNERS for end in ("kmin", "kmax")}
    assert want <= pool.seen
    kinds = {lane.what.split(",")[0] for lane in pool.lanes}
    assert {"Q = P", "Q = -P", "Q = 2 P", "P = O own", "Q = O own", "P = Q = O own", "P = Q = O scaled", "special + its negative"} <= kinds
    inside = [g2.in_g2(lane.P) for lane in pool.lanes if lane.P is not None]
    assert any(inside) and not all(inside)
    assert {lane.control for lane in pool.lanes} == set(L.CONTROLS)
    pts, ctl = L.pack_lanes(pool.lanes)
    assert len(pts) == len(pool.lanes) * 2 * 3 * 28 * 4 and len(ctl) == 4 * len(pool.lanes)


def test_checker_accepts_the_restatement_and_rejects_what_is_wrong():
    pool = L.pool()
    rng = random.Random("g2-law/checker")
    lanes = pool.lanes[::3]
    good = [L.reimage(lane, rng) for lane in lanes]
    stats = {}
    assert L.check_all(lanes, good, stats) == [] and stats and max(stats.values()) < 3
    lane = next(ln for ln in lanes if ln.P is not None and ln.Q is not None and g2.add(ln.P, ln.Q) is not None)
    slots = L.reimage(lane, rng)
    copy = lambda s: {k: {c: (list(v[0]), list(v[1])) for c, v in img.items()} for k, img in s.items()}
    # a wrong slot: the sum where the difference belongs
    wrong = copy(slots)
    wrong[L.SLOT_SUB] = wrong[L.SLOT_ADD]
    assert any(f"slot {L.SLOT_SUB} is not the restatement's point" in b for b in L.check_lane(lane, wrong))
    # c0 and c1 of one coordinate swapped
    wrong = copy(slots)
    wrong[L.SLOT_DBL]["x"] = wrong[L.SLOT_DBL]["x"][::-1]
    assert any(f"slot {L.SLOT_DBL} is not the restatement's point" in b for b in L.check_lane(lane, wrong))
    # a limb outside its class, the value kept: limb 0 raised by 2^28, limb 1 lowered by one
    wrong = copy(slots)
    image = wrong[L.SLOT_CHAIN + 2]["y"][1]
    image[0] += 1 << 28
    image[1] -= 1
    bad = L.check_lane(lane, wrong)
    assert len(bad) == 1 and "is outside its class c2.9: limb 0" in bad[0]
    # a value outside its class: 4 p added to a component of the doubling's X (an n)
    wrong = copy(slots)
    image = wrong[L.SLOT_DBL]["z"][0]
    wrong[L.SLOT_DBL]["z"] = (L.carry([a + 4 * b for a, b in zip(image, g2.limbs(g2.P))]), wrong[L.SLOT_DBL]["z"][1])
    bad = L.check_lane(lane, wrong)
    assert len(bad) == 1 and "outside its class n" in bad[0]
    # the record path and cneg are exact
    wrong = copy(slots)
    wrong[L.SLOT_REC]["z"][0][3] ^= 1
    assert any("read back from its record" in b for b in L.check_lane(lane, wrong))
    wrong = copy(slots)
    wrong[L.SLOT_NEG]["y"] = tuple([-x for x in im] for im in lane.images["P"]["y"])          # negated, but not carried
    assert any("carry(neg(y))" in b for b in L.check_lane(lane, wrong)) or all(x == 0 for im in lane.images["P"]["y"] for x in im[:13])
    wrong = copy(slots)
    wrong[L.SLOT_KEEP]["x"][1][0] += 1
    assert any(f"slot {L.SLOT_KEEP} is not the image of P" in b for b in L.check_lane(lane, wrong))
    # slot 3 is not part of what is read
    raw = b"".join(b"".join(struct.pack("<28i", *(slots.get(s, slots[0])[c][0] + slots.get(s, slots[0])[c][1])) for c in L.COORDS) for s in range(L.SLOTS))
    assert L.SLOT_UNUSED not in L.unpack_slots(raw, 1)[0] and L.unpack_slots(raw, 1)[0] == slots
