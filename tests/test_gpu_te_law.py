"""GPU: the law of Bandersnatch and JubJub (csrc/curve.hip.h: te_add, te_dbl, te_cneg; csrc/kernels_te.hip.h: te_madd, the LDS table;
bsn_endomorphism) on RAW limb images over the 9 x 29-bit Fr (dr_te_law_selftest) against oracle/pyref/bandersnatch.py, with every
coordinate of P and Q at the edges of the class the headers document and every returned coordinate checked against the class they
document for it.  The lanes and the checker are tests/law_images.py's, proven without a GPU by tests/test_law_images_cpu.py.  All
comparisons are exact; the ranges printed are what the lanes reached and nothing is asserted against them."""
import ctypes
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import law_images as L  # noqa: E402

from dot_ring_amd import _native  # noqa: E402

pytestmark = pytest.mark.gpu


def _run(ctx, cv, lanes):
    records, controls = L.pack_lanes(cv, lanes)
    return L.unpack_slots(cv, ctx.te_law_selftest(cv.te_id, records, controls), len(lanes))


@pytest.mark.parametrize("name", L.TE_CURVES)
def test_the_whole_pool(ctx, name):
    cv, lanes = L.curve(name), L.pool(name).lanes
    stats = {}
    bad = L.check_all(cv, lanes, _run(ctx, cv, lanes), stats)
    print("\n" + L.format_stats(cv, stats))
    assert not bad, (len(bad), bad[:10])


@pytest.mark.parametrize("name", L.TE_CURVES)
def test_a_lone_lane_a_full_wave_and_a_tail_lane(ctx, name):
    """the first 1, 64 and 65 lanes in calls of their own: each must be checked on its own, not against another call"""
    cv, lanes = L.curve(name), L.pool(name).lanes
    assert len(lanes) > 65
    for n in (1, 64, 65):
        bad = L.check_all(cv, lanes[:n], _run(ctx, cv, lanes[:n]))
        assert not bad, (n, len(bad), bad[:10])


@pytest.mark.parametrize("name", L.TE_CURVES)
def test_refusals(ctx, name):
    cv = L.curve(name)
    fn = _native.lib().dr_te_law_selftest
    records, controls = L.pack_lanes(cv, L.pool(name).lanes[:2])
    out = ctypes.create_string_buffer(2 * cv.slots * len(cv.coords) * cv.limbs * 4)
    marker = bytes(out.raw)
    assert fn(ctx.handle, cv.te_id, None, None, 0, None) == 0                             # n = 0 returns at once
    for args in ((None, controls, 2, out), (records, None, 2, out), (records, controls, 2, None)):
        assert fn(ctx.handle, cv.te_id, *args) == _native.DR_ERR_INVALID and "null buffer" in _native.last_error()
    assert fn(ctx.handle, cv.te_id, records, controls, 1 << 24, out) == _native.DR_ERR_INVALID and "batch too large" in _native.last_error()
    for other in (2, 3, 5, 12, -1):                                                       # every other curve id, n = 0 included
        assert fn(ctx.handle, other, records, controls, 2, out) == _native.DR_ERR_INVALID and "unknown curve id" in _native.last_error()
        assert fn(ctx.handle, other, None, None, 0, None) == _native.DR_ERR_INVALID
    assert out.raw == marker                                                              # nothing was written
    assert fn(ctx.handle, cv.te_id, records, controls, 2, out) == 0 and out.raw != marker
