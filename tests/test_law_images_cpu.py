"""The lanes and the checker of tests/law_images.py without a GPU: every built image lies in the class its header documents, every
corner of every in-class is reached at the smallest and at the largest multiple of p, the checker accepts the reference's own results
re-imaged and rejects a limb changed by one, a point replaced by its negative and an image one unit outside its out-class; and the
host builds of the 384-, 521- and 448-bit laws under -fsanitize=undefined run the same lanes through the same checker (the `lane` line of
tests/native/*_host_check.cpp), where a signed column overflow at the edge of a contract aborts.

The same for the lanes of Bandersnatch and JubJub (dr_te_law_selftest): their table rows, the four further slots and the scalar of
the endomorphism.  Their products are montmul9x29_asm, gfx950 assembly: there is no host build of this law to run under a sanitizer,
and none is loaded into Python."""
import os
import random
import subprocess

import pytest

import law_images as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dot_ring_amd", "csrc")


@pytest.mark.parametrize("name", L.CURVES + L.TE_CURVES)
def test_every_image_is_in_its_class_and_every_corner_is_reached(name):
    cv, pool = L.curve(name), L.pool(name)
    assert len(pool.lanes) > 65
    for lane in pool.lanes:
        for who, classes, negatable in (("P", cv.cls_p, cv.p_neg), ("Q", cv.cls_q, cv.q_neg)):
            xyz = {c: cv.residue(lane.images[who][c]) for c in cv.coords}
            assert cv.same_point(xyz, lane.P if who == "P" else lane.Q), lane.what
            for c in cv.coords:
                image = lane.images[who][c]
                ok = any(cls.contains(image, cv.bits) for cls in classes[c])
                if negatable and c in cv.neg_coords:
                    ok = ok or classes[c][0].negated().contains(image, cv.bits)
                assert ok, (lane.what, who, c)
    unit = 1 << cv.bits
    for who, classes, negatable in (("P", cv.cls_p, cv.p_neg), ("Q", cv.cls_q, cv.q_neg)):
        for c in cv.coords:
            for cls in classes[c]:
                for corner in L.CORNERS:
                    assert (who, c, cls.name, corner, "kmin") in pool.seen and (who, c, cls.name, corner, "kmax") in pool.seen, (who, c, corner)
                    at = cls.corner(corner)
                    near = [lane for lane in pool.lanes if all(abs(x - b) < unit for x, b in zip(lane.images[who][c], at))]
                    assert near, (who, c, cls.name, corner)
            if negatable and c in cv.neg_coords:
                assert {k[3] for k in pool.seen if k[:3] == (who, c, "negated")} == set(L.CORNERS)
    controls = {lane.control for lane in pool.lanes}
    assert any(k & 0x3F for k in controls) and any(k & 0x3F00 for k in controls)                          # a negated term, an identity term
    assert any((k & 3) == 3 and not (k >> 8) & 3 for k in controls) and any((k & 3) == 0 and not (k >> 8) & 3 for k in controls)   # equal signs in a row


@pytest.mark.parametrize("name", L.CURVES + L.TE_CURVES)
def test_checker_accepts_the_reference_and_rejects_what_is_wrong(name):
    cv, pool = L.curve(name), L.pool(name)
    rng = random.Random(name)
    for lane in pool.lanes:
        assert L.check_lane(cv, lane, L.reimage(cv, lane, rng)) == [], lane.what
    # a lane of two ordinary points
    lane = next(x for x in pool.lanes if x.what.startswith("mixed"))
    for slot in (L.SLOT_ADD, L.SLOT_DBL, L.SLOT_CHAIN + 5):
        for c in cv.coords:
            slots = L.reimage(cv, lane, rng)
            j = rng.randrange(cv.limbs)
            slots[slot][c][j] += 1 if slots[slot][c][j] < cv.cls_out[c].hi[j] else -1
            bad = L.check_lane(cv, lane, slots)
            assert any("not the reference's point" in b for b in bad), (slot, c)
    for slot in (L.SLOT_ADD, L.SLOT_SUB, L.SLOT_DBL, L.SLOT_CHAIN, L.SLOT_CHAIN + 5):
        slots = L.reimage(cv, lane, rng)
        for c in cv.neg_coords:
            slots[slot][c] = [-x for x in slots[slot][c]]                                                 # the negative of the point
        if slot == L.SLOT_ADD:
            slots[L.SLOT_LDS] = {c: list(v) for c, v in slots[slot].items()}
        assert any("not the reference's point" in b for b in L.check_lane(cv, lane, slots)), slot
    for slot in (L.SLOT_ADD, L.SLOT_DBL, L.SLOT_CHAIN + 2):
        for c in cv.coords:
            cls = cv.cls_out[c]
            for j in (0, cv.limbs // 2, cv.limbs - 1):
                for edge in ("hi", "lo"):
                    slots = L.reimage(cv, lane, rng)
                    slots[slot][c][j] = cls.hi[j] + 1 if edge == "hi" else cls.lo[j] - 1
                    assert any("outside its class" in b for b in L.check_lane(cv, lane, slots)), (slot, c, j, edge)
    cls = cv.cls_out["y"]
    if cls.vhi is not None and L.value_of(cls.hi, cv.bits) >= cls.vhi:
        # where the limb bounds alone allow more than the value bound: inside every limb bound, outside by value
        assert not cls.contains(list(cls.hi), cv.bits)
    # the LDS round trip must give back the stored image (a table of limb images) or the same point in from_lds' class
    slots = L.reimage(cv, lane, rng)
    slots[L.SLOT_LDS]["z"][0] ^= 1
    assert any("LDS" in b or "slot 5" in b for b in L.check_lane(cv, lane, slots))
    if cv.extended:
        # T Z = X Y is part of the point; the T of dbl_no_t is not
        slots = L.reimage(cv, lane, rng)
        slots[L.SLOT_DBL]["t"][0] ^= 1
        slots[L.SLOT_DBL_NO_T]["t"][0] ^= 1
        bad = L.check_lane(cv, lane, slots)
        if cv.no_t_zero:                              # ... but where the law documents the zero image for it, that is asked
            assert any("slot 2" in b for b in bad) and [b for b in bad if "slot 3" in b] == [b for b in bad if "not the zero image" in b] != []
        else:
            assert any("slot 2" in b for b in bad) and not any("slot 3" in b for b in bad)


@pytest.mark.parametrize("name", L.TE_CURVES)
def test_te_rows_small_points_and_the_four_further_slots(name):
    cv, pool = L.curve(name), L.pool(name)
    p, ref = cv.p, cv.ref
    # the small-order points: Bandersnatch has the one affine point of order 2 (the other two are at infinity: a = -5 is no square) and
    # points whose multiple by N is at infinity; JubJub all seven of its cyclic 8-torsion, orders 2, 4, 4, 8, 8, 8, 8
    orders = sorted(next(k for k in (1, 2, 4, 8) if ref.mul(k, t) == (0, 1)) for t in cv.torsion)
    assert orders == ([2] if name == "bandersnatch" else [2, 4, 4, 8, 8, 8, 8]) and (0, p - 1) in cv.torsion
    assert len(cv.outside) == (2 if name == "bandersnatch" else 1)
    for pt in cv.outside:
        assert ref.on_curve(pt)
        try:
            assert ref.mul(ref.N, pt) != (0, 1)
        except ZeroDivisionError:
            assert name == "bandersnatch"
    for s in cv.specials:
        assert sum(1 for lane in pool.lanes if lane.P == s) >= 3 and sum(1 for lane in pool.lanes if lane.Q == s) >= 2
    # the scalar of the endomorphism, from the lattice basis of glv_decompose: lambda^2 + 2 = 0 mod N
    if cv.endo is not None:
        assert (cv.endo * cv.endo + 2) % ref.N == 0
    # every row is unpack of canonical words, of a point of the curve with dt = d x y; both signs; the identity; P and -P
    canon = cv.cls_lds["x"]
    for lane in pool.lanes:
        x, y, dt = (cv.residue(lane.images["R"][c]) for c in ("x", "y", "dt"))
        assert all(canon.contains(lane.images["R"][c], 29) for c in ("x", "y", "dt")) and (x, y) == lane.row and ref.on_curve(lane.row)
        assert dt == ref.D * x * y % p
        if cv.endo is not None and lane.row != (0, 1):
            assert ref.mul(ref.N, lane.row) == (0, 1)                                                    # what the endomorphism is defined on
    assert {bool(lane.control & L.ROW_NEGATED) for lane in pool.lanes} == {True, False}
    assert any(lane.row == (0, 1) for lane in pool.lanes) and any(lane.row == lane.P != (0, 1) for lane in pool.lanes)
    assert any(lane.row == cv.neg(lane.P) != lane.P for lane in pool.lanes)
    if cv.endo is None:
        assert {lane.row for lane in pool.lanes} >= set(cv.torsion)
    # the checker sees the four further slots, T Z = X Y and the zero T of dbl_no_t, and the canonical LDS image
    rng = random.Random(name)
    lane = next(x for x in pool.lanes if x.what.startswith("mixed") and x.row not in ((0, 1), x.P, cv.neg(x.P)))
    further = [L.SLOT_MADD, L.SLOT_MADD4, L.SLOT_ADD_OUT] + ([L.SLOT_ENDO] if cv.endo is not None else [])
    assert sorted(L.reimage(cv, lane, rng)) == sorted(list(range(13)) + further)
    for slot in further:
        for c in cv.coords:
            slots = L.reimage(cv, lane, rng)
            slots[slot][c][rng.randrange(8)] ^= 1
            assert any(f"slot {slot} " in b and "not the reference's point" in b for b in L.check_lane(cv, lane, slots)), (slot, c)
        slots = L.reimage(cv, lane, rng)
        for c in cv.neg_coords:
            slots[slot][c] = [-v for v in slots[slot][c]]
        assert any(f"slot {slot} " in b for b in L.check_lane(cv, lane, slots)), slot
        slots = L.reimage(cv, lane, rng)
        slots[slot]["y"][3] = 1 << 29
        assert any(f"slot {slot} " in b and "limb 3 = 536870912 is not in" in b for b in L.check_lane(cv, lane, slots)), slot
    slots = L.reimage(cv, lane, rng)
    slots[L.SLOT_DBL_NO_T]["t"][0] = 1
    assert any("not the zero image" in b for b in L.check_lane(cv, lane, slots))
    slots = L.reimage(cv, lane, rng)
    slots[L.SLOT_LDS]["y"] = [v + w for v, w in zip(slots[L.SLOT_LDS]["y"], L.digits(p, 9, 29))]        # the same residue, not canonical
    assert any("slot 5" in b for b in L.check_lane(cv, lane, slots))
    # the row's sign reaches the expectation: the other sign is rejected
    lane.control ^= L.ROW_NEGATED
    lane._want = None
    other = L.reimage(cv, lane, rng)
    lane.control ^= L.ROW_NEGATED
    lane._want = None
    assert any("slot 13" in b for b in L.check_lane(cv, lane, other)) and any("slot 14" in b for b in L.check_lane(cv, lane, other))
    # the record as the device takes it: P, Q, the row, 11 x 9 limbs; 17 points back
    records, controls = L.pack_lanes(cv, pool.lanes[:3])
    assert len(records) == 3 * 11 * 9 * 4 and len(controls) == 12
    assert L.unpack_slots(cv, bytes(3 * 17 * 36 * 4), 3)[0].keys() == set(range(13)) | set(further)


HOST_CHECKS = {"p384": "p384_host_check.cpp", "p521": "p521_host_check.cpp", "curve448": "c448_law_host_check.cpp", "ed448": "e448_law_host_check.cpp"}


@pytest.mark.parametrize("name", sorted(HOST_CHECKS))
def test_host_law_under_the_sanitizer_on_the_same_lanes(name, tmp_path):
    cv, pool = L.curve(name), L.pool(name)
    exe = tmp_path / "host_check"
    # (-std=c++20: divstep28.hip.h shifts negative values left, which is defined from C++20 on; signed overflow stays undefined)
    subprocess.run(["g++", "-O2", "-std=c++20", "-fsanitize=undefined", "-fno-sanitize-recover", "-I", CSRC,
                    os.path.join(ROOT, "tests", "native", HOST_CHECKS[name]), "-o", str(exe)], check=True)
    text = "\n".join(L.lane_line(cv, lane) for lane in pool.lanes) + "\n"
    out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    answers = out.stdout.splitlines()
    assert len(answers) == len(pool.lanes)
    stats = {}
    bad = L.check_all(cv, pool.lanes, [L.parse_lane_line(cv, a) for a in answers], stats)
    print("\n" + L.format_stats(cv, stats))
    assert not bad, bad[:10]
