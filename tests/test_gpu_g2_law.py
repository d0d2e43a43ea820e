"""The group law of BLS12-381's E(Fq2) on RAW limb images on the GPU (dr_blsg2_law_selftest: csrc/kernels_g2_msm.hip.h,
k_blsg2_law_selftest over G2hCurve): the lanes of g2_law_images.py — real points of E(Fq2) in G2, outside it, equal, inverse and the
identity, every component of every coordinate a limb image at a corner of the class kernels_g2_h2c.hip.h documents for a coordinate
(c3) — through add, add of the negative, dbl, cneg either way, the record of the bucket method and back, and six steps of the bit walk.
Every written slot is compared with the big-integer restatement by cross-multiplication over Fp2, and every returned component must lie
in the class the headers document for what the law returns (test_g2_msm_cpu.py holds the lanes and the checker to their own claims)."""
import ctypes
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import g2_law_images as L  # noqa: E402

pytestmark = pytest.mark.gpu


def _run(ctx, lanes):
    pts, ctl = L.pack_lanes(lanes)
    return L.unpack_slots(ctx.blsg2_law_selftest(pts, ctl), len(lanes))


def test_whole_pool(ctx):
    lanes = L.pool().lanes
    assert len(lanes) > 64
    stats = {}
    bad = L.check_all(lanes, _run(ctx, lanes), stats)
    for (op, c), v in sorted(stats.items()):
        print(f"E(Fq2) {op} {c}: max |value| {v:.3f} p")
    assert bad == [], "\n".join(bad[:20])


@pytest.mark.parametrize("n", (1, 64, 65))
def test_lone_lane_full_wave_and_tail(ctx, n):
    """n = 1: 63 lanes past n recompute record 0 and store nothing; 64: a whole wave; 65: a tail lane alone in a second workgroup"""
    pool = L.pool().lanes
    lanes = pool[-n:] if n < 64 else pool[:n]
    assert L.check_all(lanes, _run(ctx, lanes)) == []


def test_refusals(ctx):
    from dot_ring_amd import _native

    lib = _native.lib()
    lanes = L.pool().lanes[:2]
    pts, ctl = L.pack_lanes(lanes)
    out = ctypes.create_string_buffer(2 * L.SLOTS * 3 * 28 * 4)
    for args in ((None, ctl, 2, out), (pts, None, 2, out), (pts, ctl, 2, None)):
        assert lib.dr_blsg2_law_selftest(ctx.handle, *args) == -1 and _native.last_error() == "null buffer"
    assert lib.dr_blsg2_law_selftest(ctx.handle, pts, ctl, 1 << 24, out) == -1 and _native.last_error() == "batch too large"
    assert lib.dr_blsg2_law_selftest(ctx.handle, None, None, 0, None) == 0
    with pytest.raises(ValueError):
        ctx.blsg2_law_selftest(pts[:-4], ctl)
    assert ctx.blsg2_law_selftest(b"", b"") == b""
    assert L.check_all(lanes, _run(ctx, lanes)) == []
