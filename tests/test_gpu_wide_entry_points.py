"""The host path the three wide suites share (csrc/capi_suite.hpp under the dr_blsg1_*, dr_blsg2_* and dr_ed448_* entry points), on the
GPU: every profiled entry point launches under its own name and no other suite's; a batch returns what its items return one by one,
flags included, across the edge of a 64-thread block (n = 1, 64, 65: G1H_BLOCK = G2H_BLOCK = E448_BLOCK = 64); and a small batch on a
context that has just run a large one returns what a fresh context returns (no stale flag word, and for G2 the per-element flags at
their offset n in io_c).  Inputs are the `u` values and points of the RFC 9380 vector files, cycled; every comparison is exact."""
import itertools
import json
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bls12_381_g1_ref  # noqa: E402
import bls12_381_g2_ref  # noqa: E402
import ed448_ref  # noqa: E402

from dot_ring_amd import _native  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "h2c")
SIZES = (1, 64, 65)
ON_CURVE = {"blsg1": bls12_381_g1_ref.on_curve, "blsg2": bls12_381_g2_ref.on_curve, "ed448": ed448_ref.on_curve}
NAMES = {
    "blsg1": ["k_blsg1_map_to_curve", "k_blsg1_scalar_mul", "k_blsg1_msm_groups", "k_blsg1_decode_points"],
    "blsg2": ["k_blsg2_map_iso", "k_blsg2_sum_clear", "k_blsg2_scalar_mul", "k_blsg2_check_points"],
    "ed448": ["k_ed448_map_to_curve", "k_ed448_scalar_mul", "k_ed448_msm_groups", "k_ed448_check_points"],
}
MAP_NAMES = {"blsg1": ["k_blsg1_map_to_curve"], "blsg2": ["k_blsg2_map_iso", "k_blsg2_sum_clear"], "ed448": ["k_ed448_map_to_curve"]}
VARIANT_RO = {"blsg1": _native.CURVE_BLS12_381_G1, "blsg2": _native.CURVE_BLS12_381_G2, "ed448": _native.CURVE_ED448_RO}
FILES = {"blsg1": "bls12_381_G1", "blsg2": "bls12_381_G2", "ed448": "ed448"}
SUITES = sorted(NAMES)


def _value(suite, v):
    """one coordinate or field element of a vector file: an integer, for G2 the pair (re, im)"""
    return (int(v["re"], 16), int(v["im"], 16)) if suite == "blsg2" else int(v, 16)


def _raw(suite, value, width):
    """... as the entry points take it (little-endian; Fq2 as c0 || c1)"""
    return b"".join(c.to_bytes(48, "little") for c in value) if suite == "blsg2" else value.to_bytes(width, "little")


class Inputs:
    """the field elements, points (x || y), decoder inputs and scalars of one suite: the vector files' in file order, cycled to 130.
    `inside` are the P of the vectors (in the prime-order subgroup), `pts` those and the images before the clearing, Q0 / Q1 / Q (on the
    curve; on the BLS12-381 curves outside the subgroup), on Ed448 also a point of order 4.  Some Q strings of the files are malformed (a digit too many, a blank inside): only strings that
    parse to a point of the curve are used."""

    def __init__(self, suite):
        w = _native._WIDE[suite]
        fe = w.point // 2
        us, pts, inside = [], [], []
        for variant in ("ro", "nu"):
            with open(os.path.join(GOLDEN, f"{FILES[suite]}_{variant}.json")) as f:
                for v in json.load(f)["vectors"]:
                    us += [_raw(suite, _value(suite, u), fe) for u in v["u"]]
                    for k in ("P", "Q0", "Q1", "Q"):
                        try:
                            pt = (_value(suite, v[k]["x"]), _value(suite, v[k]["y"]))
                            if not ON_CURVE[suite](pt):
                                continue
                            pts.append(_raw(suite, pt[0], fe) + _raw(suite, pt[1], fe))
                        except (KeyError, ValueError, OverflowError):
                            continue
                        if k == "P":
                            inside.append(pts[-1])
        assert len(us) == 15 and len(inside) == 10 and len(pts) >= 18 and pts[0] == inside[0]
        assert all(len(u) == w.elem for u in us) and all(len(p) == w.point for p in pts)
        if suite == "ed448":          # the images of this map lie in the prime-order subgroup already (a 4-isogeny precedes them): (1, 0) has order 4
            pts.append(_raw(suite, 1, fe) + _raw(suite, 0, fe))
        self.inside, self.outside = inside, [p for p in pts if p not in inside]
        cyc = lambda xs: list(itertools.islice(itertools.cycle(xs), 130))  # noqa: E731
        self.w, self.suite, self._us, self.pts = w, suite, cyc(us), cyc(pts)
        if suite == "blsg1":                                 # the decoder takes SEC1 compressed strings: 0x02 | parity(y), x big-endian
            self.enc = [bytes([2 + (p[48] & 1)]) + p[:48][::-1] for p in self.pts]
        else:
            self.enc = self.pts
        rng = random.Random(suite)
        self.scalars = [rng.randbytes(w.scalar) for _ in range(130)]

    def us(self, per_item):
        """130 field elements; on Ed448 the first element of item 1 is u = 1, which has no image: a zero flag inside every batch"""
        us = list(self._us)
        if self.suite == "ed448":
            us[per_item] = (1).to_bytes(56, "little")
        return us


_INPUTS = {}


def inputs(suite):
    if suite not in _INPUTS:
        _INPUTS[suite] = Inputs(suite)
    return _INPUTS[suite]


def _flagged(ctx, suite, blob, check):
    """the flag-returning call as (points or b"", flags)"""
    if suite == "blsg2":
        return b"", ctx.blsg2_check_points(blob, subgroup=check)
    return getattr(ctx, f"{suite}_decode_points")(blob, check=check)


# ---------------------------------------------------------------- launch names
@pytest.mark.parametrize("suite", SUITES)
def test_launch_names(suite):
    inp, n = inputs(suite), 3
    ctx = _native.Context(0)
    try:
        ctx.prof_enable(True)
        getattr(ctx, f"{suite}_map_to_curve")(b"".join(inp.us(1)[3 : 3 + n]), 1)
        getattr(ctx, f"{suite}_scalar_mul_batch")(b"".join(inp.pts[:n]), b"".join(inp.scalars[:n]))
        if suite != "blsg2":                                                             # 3 groups of 2
            getattr(ctx, f"{suite}_msm_groups")(b"".join(inp.pts[: 2 * n]), b"".join(inp.scalars[: 2 * n]), 2)
        _flagged(ctx, suite, b"".join(inp.enc[:n]), True)
        for other in SUITES:
            for name in NAMES[other]:
                assert ctx.prof_get(name)[1] == (1 if other == suite else 0), name
        # the batch encoder launches the map under the same name(s), and nothing else
        getattr(ctx, f"{suite}_encode_to_curve_batch")(VARIANT_RO[suite], [b"a", b"", b"abc"])
        for other in SUITES:
            for name in NAMES[other]:
                assert ctx.prof_get(name)[1] == (0 if other != suite else 2 if name in MAP_NAMES[suite] else 1), name
    finally:
        ctx.close()


# ---------------------------------------------------------------- a batch equals its items
def _batch_equals_items(call, items, per_call=1):
    """call(blob of items) for the first n items, n in SIZES, against the single-item calls (each made once); results are tuples of byte
    strings, one record per item in each"""
    singles = [call(b"".join(items[per_call * i : per_call * (i + 1)])) for i in range(max(SIZES))]
    for n in SIZES:
        got = call(b"".join(items[: per_call * n]))
        want = tuple(b"".join(parts) for parts in zip(*singles[:n]))
        assert tuple(got) == want, n
    return singles


@pytest.mark.parametrize("per_item", (1, 2))
@pytest.mark.parametrize("suite", SUITES)
def test_map_to_curve_batch_equals_items(ctx, suite, per_item):
    inp = inputs(suite)
    singles = _batch_equals_items(lambda blob: getattr(ctx, f"{suite}_map_to_curve")(blob, per_item), inp.us(per_item), per_item)
    flags = [s[1][0] for s in singles]
    if suite == "ed448":
        assert flags == [1, 0] + [1] * 63 and singles[1][0] == bytes(112)
    else:
        assert all(flags)


@pytest.mark.parametrize("suite", SUITES)
def test_scalar_mul_batch_equals_items(ctx, suite):
    inp = inputs(suite)
    w = inp.w
    singles = [getattr(ctx, f"{suite}_scalar_mul_batch")(inp.pts[i], inp.scalars[i]) for i in range(max(SIZES))]
    assert all(len(s) == w.point for s in singles) and len(set(singles)) > 1
    for n in SIZES:
        assert getattr(ctx, f"{suite}_scalar_mul_batch")(b"".join(inp.pts[:n]), b"".join(inp.scalars[:n])) == b"".join(singles[:n]), n


@pytest.mark.parametrize("check", (False, True))
@pytest.mark.parametrize("suite", SUITES)
def test_flagged_batch_equals_items(ctx, suite, check):
    inp = inputs(suite)
    singles = _batch_equals_items(lambda blob: _flagged(ctx, suite, blob, check), inp.enc)
    flags = [s[1][0] for s in singles]
    # every input is on the curve, P of a vector in the subgroup, and some input outside it (Inputs)
    assert flags[0] == 1 and (all(flags) if not check else 0 in flags)


# ---------------------------------------------------------------- a shrinking batch on a used context
def _fresh(call):
    c = _native.Context(0)
    try:
        return call(c)
    finally:
        c.close()


@pytest.mark.parametrize("suite", SUITES)
def test_map_after_a_larger_batch(suite):
    us = inputs(suite).us(2)
    big = b"".join(us)
    small = b"".join(us[2:4]) if suite == "ed448" else b"".join(us[7:9])       # Ed448: (1, u), no image: flag 0 where the batch left a 1
    fn = f"{suite}_map_to_curve"
    want = _fresh(lambda c: getattr(c, fn)(small, 2))

    def used(c):
        first = getattr(c, fn)(big, 2)
        assert len(first[1]) == 65
        return getattr(c, fn)(small, 2)

    assert _fresh(used) == want
    assert list(want[1]) == ([0] if suite == "ed448" else [1])


def test_blsg2_check_points_after_a_larger_batch():
    inp = inputs("blsg2")
    big, small = b"".join(itertools.islice(itertools.cycle(inp.inside), 65)), inp.outside[0]
    want = _fresh(lambda c: c.blsg2_check_points(small, subgroup=True))

    def used(c):
        assert c.blsg2_check_points(big, subgroup=True) == bytes([1]) * 65
        return c.blsg2_check_points(small, subgroup=True)

    assert _fresh(used) == want == bytes([0])
