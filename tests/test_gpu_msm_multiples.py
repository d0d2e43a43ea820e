"""Batched G1 MSMs over an SRS table with odd-multiple rows (dr_srs_precompute_multiples): block t of the table holds the bit rows of
(2 t + 1) P_i and a digit of the non-adjacent form becomes +-(2 t + 1) b (msm_recode.hip.h: for_each_wnaf_multiple_digit; the host check
is tests/native/recode_multiples_check.cpp).  Results are group sums: with 1, 2, 4 and 8 multiples a call must return the same bytes as over
the plain bases, and a sample of them the oracle's."""
import random

import pytest

from oracle import coracle

pytestmark = pytest.mark.gpu

R = coracle.FR_P
BITS, WIDTH = 12, 13          # 256 MSMs reach the non-adjacent form only with 2048 buckets per set (msm_plan.hpp: L4_BELOW): width 13


def _be_to_le(rec: bytes) -> bytes:
    return rec[:48][::-1] + rec[48:][::-1]


def _oracle_msm_be(blob_be: bytes, ks: bytes, n: int):
    out = coracle.g1_msm_raw(b"".join(_be_to_le(blob_be[96 * i : 96 * i + 96]) for i in range(n)), ks, n)
    if out == bytes(96):
        return None
    return out[:48][::-1] + out[48:][::-1]


def _edge_vectors(n: int, batch: int, rng) -> list:
    """the vectors of test_g1_msm_batched_odd_multiple_buckets (tests/test_gpu_kernels.py), then random ones"""
    vecs = []
    for b in range(batch):
        if b == 0:
            v = [0] * n
        elif b == 1:
            v = [R - 1] * n
        elif b == 2:
            v = [(1 << (i % 255)) % R for i in range(n)]                       # single bits: every row
        elif b == 3:
            v = [((1 << (BITS + 1)) - 1) << ((BITS + 1) * (i % 16)) for i in range(n)]
        elif b == 4:
            v = [5] * n                                                        # one long list
        elif b == 5:
            v = [(1 << 255) % R if i % 2 else ((1 << BITS) << (7 * (i % 30))) % R for i in range(n)]
        elif b == 6:
            v = [((1 << (200 + i % 55)) - 1 - (i % 7)) % R for i in range(n)]  # long runs of ones: the carry crosses every slot
        elif b == 7:
            v = [(int("5" * 64, 16) >> (i % 9)) % R for i in range(n)]         # alternating bits
        elif b == 8:
            v = [(int("a" * 64, 16) >> (i % 5)) % R for i in range(n)]
        elif b == 9:
            v = [R - 1 - i if i % 2 else (R >> 1) + i for i in range(n)]       # top digits on the last rows, (r - 1) / 2 and neighbours
        elif b == 10:
            v = [((1 << WIDTH) - 1) * (1 << (i % 240)) % R for i in range(n)]  # 2^w - 1 at every offset of every slot
        elif b == 11:
            v = [(((1 << (WIDTH - 1)) + (i % 3) - 1) << (i % 241)) % R for i in range(n)]   # around the sign threshold of a digit
        else:
            v = [rng.randrange(R) for _ in range(n)]
        vecs.append(b"".join(x.to_bytes(32, "little") for x in v))
    return vecs


@pytest.mark.parametrize("n", [150, 1500])
def test_g1_msm_batch_over_multiples_matches_plain(ctx, srs_bytes, n, monkeypatch):
    """256 MSMs of 150 points (3000 digit slots per set: the plain LDS sort, k_g1_sort_sets) and of 1500 points (30000: the staged sort
    with u32 digit rows) over tables of DOTRING_SRS_MULTIPLES = 1, 2, 4 and 8 blocks: table_info reports the width-13 non-adjacent form
    with that many multipliers and fewer digits per scalar; every result equals the one over the plain bases, 14 of them the oracle's."""
    batch = 256
    rng = random.Random(1000 * n + 13)
    vecs = _edge_vectors(n, batch, rng)
    ks = b"".join(vecs)
    plain = ctx.srs_load(srs_bytes[: 96 * n])
    want = ctx.g1_msm_batch(plain, ks, n)
    plain.close()
    for b in list(range(13)) + [batch - 1]:
        assert want[b] == _oracle_msm_be(srs_bytes, vecs[b], n), b
    digits = {}
    for multiples in (1, 2, 4, 8):
        monkeypatch.setenv("DOTRING_SRS_MULTIPLES", str(multiples))
        tabled = ctx.srs_load(srs_bytes[: 96 * n]).precompute(BITS, multiples=0)
        info = tabled.table_info(n, batch)
        assert info["rows"] == 256 and info["tiling"] == "non-adjacent form" and info["tiling_bits"] == WIDTH
        assert info["multiples"] == multiples and info["table_multiples"] == multiples
        assert tabled.table_info(n, 64)["multiples"] == 1                      # few MSMs: the window rows of block 0
        digits[multiples] = info["digits_per_scalar"]
        got = ctx.g1_msm_batch(tabled, ks, n)
        assert got == want, (multiples, [b for b in range(batch) if got[b] != want[b]][:8])
        assert ctx.g1_msm_batch(tabled, ks[: 32 * n * 64], n) == want[:64]     # 64 MSMs over the same table: window rows
        tabled.close()
    assert digits[1] > digits[2] > digits[4] > digits[8] and abs(digits[4] - 17.3) < 0.1 and abs(digits[8] - 16.6) < 0.1


def test_srs_precompute_keeps_the_plain_table(ctx, srs_bytes, monkeypatch):
    """dr_srs_precompute (and multiples = 1) builds the table without multiples whatever DOTRING_SRS_MULTIPLES says; a table beyond
    DOTRING_SRS_MULTIPLES_MB gets fewer blocks, never an error."""
    n = 64
    monkeypatch.setenv("DOTRING_SRS_MULTIPLES", "4")
    srs = ctx.srs_load(srs_bytes[: 96 * n]).precompute(BITS)
    assert srs.table_info(n, 256)["table_multiples"] == 1 and srs.table_info(n, 256)["multiples"] == 1
    monkeypatch.setenv("DOTRING_SRS_MULTIPLES_MB", "5")                        # 64 points: 2 MB per block
    srs.precompute(BITS, multiples=8)
    assert srs.table_info(n, 256)["table_multiples"] == 2
    monkeypatch.setenv("DOTRING_SRS_MULTIPLES_MB", "0")
    srs.precompute(BITS, multiples=0)
    assert srs.table_info(n, 256)["table_multiples"] == 1
    monkeypatch.delenv("DOTRING_SRS_MULTIPLES_MB")
    monkeypatch.delenv("DOTRING_SRS_MULTIPLES")
    srs.precompute(BITS, multiples=0)                                          # the library's default count
    assert srs.table_info(n, 256)["table_multiples"] == 8
    srs.close()


def test_ring_openings_with_zero_tails_over_multiples(monkeypatch):
    """128 proofs over an 8-key ring (domain 512): the openings phase commits 256 quotients of 1536 coefficients in one call, the second
    half of them zero beyond 511 (MsmTable::short_from) — the same proofs, byte for byte, over SRS tables of 1, 2, 4 and 8 blocks."""
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
        for multiples in (1, 2, 4, 8):
            monkeypatch.setenv("DOTRING_SRS_MULTIPLES", str(multiples))
            dev.precompute(BITS, multiples=0)
            info = dev.table_info(3 * 512, 2 * count)
            assert info["tiling"] == "non-adjacent form" and info["multiples"] == multiples
            proofs = d.RingVRF[cv].prove_batch(alphas, ads, [sks[w] for w in who], [keys[w] for w in who], ring, root)
            encoded[multiples] = [p.encode() for p in proofs]
        assert encoded[1] == encoded[2] == encoded[4] == encoded[8]
        assert d.RingVRF[cv].batch_verify(proofs, alphas, ads, ring, root)
    finally:
        monkeypatch.delenv("DOTRING_SRS_MULTIPLES", raising=False)
        dev.precompute(BITS, multiples=0)                                      # the table later tests of this process expect
