"""GPU: k_g1_decompress (dr_g1_decompress_batch — the verifier's and the device batch verifier's point decoding) against the
oracle's zcash decoding (oracle/pyref/kzg.py decompress) and the host decoder (dr_g1_decompress), encoding by encoding: SRS
points and random multiples of G1 under both sign flags, x = 0 (the point (0, +-2): on the curve, no subgroup check, as blst),
x = p - 1, x = p, x = 2^381 - 1, x without a square root, the compression bit cleared, the infinity encodings — in batches of
0, 1, 63, 64, 65 and a few thousand (several workgroups of 64 lanes, a ragged tail)."""
import random

import pytest

from dot_ring_amd import _native
from oracle import coracle
from oracle.pyref import kzg

pytestmark = pytest.mark.gpu

P = coracle.FP_P


def _enc(x: int, flags: int) -> bytes:
    """48-byte big-endian x with the three flag bits (7 compressed, 6 infinity, 5 y larger) or-ed into the top byte"""
    b = bytearray(x.to_bytes(48, "big"))
    b[0] |= flags
    return bytes(b)


def _expect(enc: bytes):
    """(ok, 96-byte BE record or None) from the oracle; the host decoder must agree"""
    try:
        pt = kzg.decompress(enc)
    except ValueError:
        with pytest.raises(ValueError):
            _native.g1_decompress(enc)
        return 0, None
    host = _native.g1_decompress(enc)
    if pt is None:
        assert host is None, enc.hex()
        return 1, None
    want = pt[0].to_bytes(48, "big") + pt[1].to_bytes(48, "big")
    assert host == want, enc.hex()
    return 1, want


def _encodings(srs_bytes, rng):
    encs = []
    # SRS points and random multiples of G1, with the right sign flag and with the flipped one (the other root: still valid)
    srs_pts = [(int.from_bytes(srs_bytes[96 * i : 96 * i + 48], "big"), int.from_bytes(srs_bytes[96 * i + 48 : 96 * i + 96], "big"))
               for i in range(0, 2048, 97)]
    pts = srs_pts + [coracle.g1_mul(kzg.G1_GEN, rng.randrange(1, coracle.FR_P)) for _ in range(40)] + [kzg.G1_GEN]
    for x, y in pts:
        larger = y > P - y
        encs.append(_enc(x, 0x80 | (0x20 if larger else 0)))
        encs.append(_enc(x, 0x80 | (0x00 if larger else 0x20)))
    assert all(kzg.compress(pt) in encs for pt in pts[:5])
    # edges of x
    for x in (0, 1, 2, P - 1, P - 2, P, P + 1, (1 << 381) - 1, (1 << 380), 4):
        encs += [_enc(x, 0x80), _enc(x, 0xA0)]
    # random x: about half have no square root of x^3 + 4
    xs = [rng.randrange(P) for _ in range(40)]
    assert sum(coracle.g1_recover_y(x, False) is None for x in xs) > 5
    for x in xs:
        encs.append(_enc(x, rng.choice([0x80, 0xA0])))
    # compression bit cleared (valid x otherwise), and the infinity variants
    x0 = pts[0][0]
    encs += [_enc(x0, 0x00), _enc(x0, 0x20), _enc(0, 0x00), _enc(0, 0x40), _enc(0, 0x60)]
    encs += [_enc(0, 0xC0), _enc(0, 0xE0), _enc(1, 0xC0), _enc(1 << 200, 0xC0), _enc(1 << 380, 0xC0), _enc(x0, 0xC0)]
    return encs


def test_g1_decompress_batch_against_the_oracle(ctx, srs_bytes):
    rng = random.Random(48)
    pool = _encodings(srs_bytes, rng)
    want = {e: _expect(e) for e in pool}
    assert sum(ok for ok, _ in want.values()) > 100 and sum(1 - ok for ok, _ in want.values()) > 30
    assert want[_enc(0, 0xC0)] == (1, None) and want[_enc(0, 0xE0)][0] == 0
    assert want[_enc(0, 0x80)][0] == 1 and want[_enc(0, 0x80)][1][48:] in ((2).to_bytes(48, "big"), (P - 2).to_bytes(48, "big"))
    for n in (0, 1, 63, 64, 65, 3001):
        batch = rng.sample(pool, n) if n <= len(pool) else [rng.choice(pool) for _ in range(n)]
        if n == 1:
            batch = [_enc(0, 0xA0)]
        pts, ok = ctx.g1_decompress_batch(b"".join(batch))
        assert len(pts) == n and len(ok) == n
        for i, e in enumerate(batch):
            w_ok, w_pt = want.get(e) or _expect(e)
            assert (ok[i], pts[i]) == (w_ok, w_pt), (n, i, e.hex())
    # every encoding of the pool once, in one launch
    pts, ok = ctx.g1_decompress_batch(b"".join(pool))
    assert [(ok[i], pts[i]) for i in range(len(pool))] == [want[e] for e in pool]
