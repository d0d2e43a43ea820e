"""Batched G1 MSMs over an SRS table with 16 and 32 blocks of odd-multiple rows (dr_srs_precompute_multiples; the recoder instances
for_each_wnaf_multiple_digit<16> and <32> of msm_recode.hip.h, whose host check is tests/native/recode_multiples_wide_check.cpp).  Results
are group sums: a call must return the same bytes as over the plain bases, and a sample of them the oracle's.  The scalar vectors are
those of test_gpu_msm_multiples.py (zero, r - 1, single bits, runs of ones, sign thresholds, random)."""
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_msm_multiples as base  # noqa: E402

pytestmark = pytest.mark.gpu

BITS, WIDTH = base.BITS, base.WIDTH
RECOMMENDED = 32              # msm_plan.hpp: SRS_BATCH_MULTIPLES, what multiples = -1 asks for
PLAN_DIGITS = {8: 16.60, 16: 15.87, 32: 15.15}     # msm_plan.hpp: NAF_MULTIPLE_DIGITS at w = 13

_plain = {}


def _plain_results(ctx, srs_bytes, n, batch):
    """the vectors of a size and their sums over the plain bases, 14 of them checked against the oracle: made once per size"""
    if n not in _plain:
        vecs = base._edge_vectors(n, batch, random.Random(1000 * n + 17))
        srs = ctx.srs_load(srs_bytes[: 96 * n])
        want = ctx.g1_msm_batch(srs, b"".join(vecs), n)
        srs.close()
        for b in list(range(13)) + [batch - 1]:
            assert want[b] == base._oracle_msm_be(srs_bytes, vecs[b], n), b
        _plain[n] = (b"".join(vecs), want)
    return _plain[n]


@pytest.mark.parametrize("multiples", [16, 32])
@pytest.mark.parametrize("n", [150, 1500])
def test_g1_msm_batch_over_wide_multiples_matches_plain(ctx, srs_bytes, n, multiples, monkeypatch):
    """256 MSMs of 150 points (3000 digit slots per set: the plain LDS sort, k_g1_sort_sets) and of 1500 points (30000: the staged sort
    with u32 digit rows, whose multiplier field now holds t < 32) over tables of DOTRING_SRS_MULTIPLES = 16 and 32 blocks (1500 points at
    32: 1.5 GB): table_info reports the width-13 non-adjacent form with that many multipliers and the planner's digit count, fewer than
    at 8; every result equals the one over the plain bases, 14 of those the oracle's; 64 MSMs over the same table take the window rows
    of block 0."""
    batch = 256
    ks, want = _plain_results(ctx, srs_bytes, n, batch)
    monkeypatch.setenv("DOTRING_SRS_MULTIPLES", "8")
    narrow = ctx.srs_load(srs_bytes[: 96 * n]).precompute(BITS, multiples=0)
    digits8 = narrow.table_info(n, batch)["digits_per_scalar"]
    narrow.close()
    monkeypatch.setenv("DOTRING_SRS_MULTIPLES", str(multiples))
    tabled = ctx.srs_load(srs_bytes[: 96 * n]).precompute(BITS, multiples=0)
    try:
        info = tabled.table_info(n, batch)
        assert info["rows"] == 256 and info["tiling"] == "non-adjacent form" and info["tiling_bits"] == WIDTH
        assert info["multiples"] == multiples and info["table_multiples"] == multiples
        assert abs(digits8 - PLAN_DIGITS[8]) < 0.005 and abs(info["digits_per_scalar"] - PLAN_DIGITS[multiples]) < 0.005
        assert info["digits_per_scalar"] < digits8
        few = tabled.table_info(n, 64)
        assert few["multiples"] == 1 and few["table_multiples"] == multiples   # few MSMs: the window rows of block 0
        got = ctx.g1_msm_batch(tabled, ks, n)
        assert got == want, (multiples, [b for b in range(batch) if got[b] != want[b]][:8])
        assert ctx.g1_msm_batch(tabled, ks[: 32 * n * 64], n) == want[:64]
    finally:
        tabled.close()


def test_wide_table_falls_back_by_halves(ctx, srs_bytes, monkeypatch):
    """A table beyond DOTRING_SRS_MULTIPLES_MB gets half the blocks asked for, and half again: 32 -> 16 -> 8, never an error; the counts
    may be asked for directly, -1 asks for the count recommended for batched proving and 0 still for 8."""
    n = 64                                                                     # 64 points: 2 MB per block
    srs = ctx.srs_load(srs_bytes[: 96 * n])
    try:
        monkeypatch.delenv("DOTRING_SRS_MULTIPLES", raising=False)
        for asked, cap_mb, built in ((32, None, 32), (16, None, 16), (32, 40, 16), (32, 20, 8), (16, 20, 8), (-1, None, RECOMMENDED),
                                     (0, None, 8)):
            if cap_mb is None:
                monkeypatch.delenv("DOTRING_SRS_MULTIPLES_MB", raising=False)
            else:
                monkeypatch.setenv("DOTRING_SRS_MULTIPLES_MB", str(cap_mb))
            srs.precompute(BITS, multiples=asked)
            info = srs.table_info(n, 256)
            assert info["table_multiples"] == built and info["multiples"] == built, (asked, cap_mb)
        monkeypatch.setenv("DOTRING_SRS_MULTIPLES", "32")                      # the knob overrides the count asked for
        srs.precompute(BITS, multiples=0)
        assert srs.table_info(n, 256)["table_multiples"] == 32
    finally:
        srs.close()


def test_ring_openings_with_zero_tails_over_wide_multiples(monkeypatch):
    """128 proofs over an 8-key ring (domain 512): the openings phase commits 256 quotients of 1536 coefficients in one call, the second
    half of them zero beyond 511 (MsmTable::short_from) — the same proofs, byte for byte, over SRS tables of 8, 16 and 32 blocks."""
    import dot_ring_amd as d

    cv = d.Bandersnatch
    sks = [(700 + i).to_bytes(32, "little") for i in range(8)]
    keys = [cv.public_key_from_secret(sk) for sk in sks]
    params = d.RingProofParams.from_ring_size(8, test_vectors=True)
    ring = d.Ring(keys, params)
    root = d.RingRoot.from_ring(ring, params)
    count = 128
    alphas = [b"in-%d" % i for i in range(count)]
    ads = [b"ad-%d" % (i % 3) for i in range(count)]
    who = [i % 8 for i in range(count)]
    dev = params.pcs._srs().device()
    encoded = {}
    try:
        for multiples in (8, 16, 32):
            monkeypatch.setenv("DOTRING_SRS_MULTIPLES", str(multiples))
            dev.precompute(BITS, multiples=0)
            info = dev.table_info(3 * 512, 2 * count)
            assert info["tiling"] == "non-adjacent form" and info["multiples"] == multiples
            proofs = d.RingVRF[cv].prove_batch(alphas, ads, [sks[w] for w in who], [keys[w] for w in who], ring, root)
            encoded[multiples] = [p.encode() for p in proofs]
        assert encoded[8] == encoded[16] == encoded[32]
        assert d.RingVRF[cv].batch_verify(proofs, alphas, ads, ring, root)
    finally:
        monkeypatch.delenv("DOTRING_SRS_MULTIPLES", raising=False)
        dev.precompute(BITS, multiples=-1)                                     # the table later tests of this process expect
