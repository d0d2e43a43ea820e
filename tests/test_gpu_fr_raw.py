"""GPU: csrc/fr29.hip.h and the addition chains of csrc/curve.hip.h on RAW limb images (dr_fr_raw_selftest) against Python integers, every
operand at the bound its header documents: mul at 2^30 x 2^29 and at 1.6 * 2^29 twice with |a||b| at 35 p^2 (and beyond), sqr, mul2 at
+-(2^29 - 1) with a b + c d at +-35 p^2, carry and carry_u at the 32-bit edge, reduce_small beside +-30 p and beside every (q + 1/2) p,
canon29 at +-8 p, canon29_small at the ends of (-p, 3p), is_zero / equal on every k p and on the non-zero values that pass the limb-0
filter, inv, te_aA / te_b_minus_aA at both ends of a product.  The records and the checker are tests/law_images.py's, proven without a
GPU by tests/test_fr_images_cpu.py.  All comparisons are exact; the ranges printed are what the records reached and nothing is asserted
against them."""
import ctypes
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import law_images as L  # noqa: E402

from dot_ring_amd import _native  # noqa: E402

pytestmark = pytest.mark.gpu


def _run(ctx, records):
    return L.unpack_fr_results(ctx.fr_raw_selftest(L.pack_fr_records(records)), len(records))


def test_the_whole_pool(ctx):
    records = L.fr_records()
    stats = {}
    bad = L.check_fr_records(records, _run(ctx, records), stats)
    print("\n" + L.format_fr_stats(stats))
    assert not bad, (len(bad), bad[:10])


def test_a_lone_record_a_full_wave_and_a_tail_record(ctx):
    """1, 64 and 65 records in calls of their own, taken across the pool so that every operation is among them"""
    spread = L.fr_spread(65)
    for n in (1, 64, 65):
        bad = L.check_fr_records(spread[:n], _run(ctx, spread[:n]))
        assert not bad, (n, len(bad), bad[:10])


def test_refusals(ctx):
    fn = _native.lib().dr_fr_raw_selftest
    images = L.pack_fr_records(L.fr_records()[:2])
    out = ctypes.create_string_buffer(2 * L.FR_OUT_WORDS * 4)
    marker = bytes(out.raw)
    assert fn(ctx.handle, None, 0, None) == 0                                             # n = 0 returns at once
    for args in ((None, 2, out), (images, 2, None)):
        assert fn(ctx.handle, *args) == _native.DR_ERR_INVALID and "null buffer" in _native.last_error()
    assert fn(ctx.handle, images, 1 << 24, out) == _native.DR_ERR_INVALID and "batch too large" in _native.last_error()
    assert out.raw == marker                                                              # nothing was written
    assert fn(ctx.handle, images, 2, out) == 0 and out.raw != marker
