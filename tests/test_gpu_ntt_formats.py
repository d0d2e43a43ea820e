"""GPU: the NTT in the ring prover's element formats (dr_ntt_formats_selftest: dr::ntt_run as capi_ring.hip calls it) against the
public-format CPU oracle applied to the decoded values.  The formats are restated in plain integers (ntt_ref.py); the inputs
include records on the edges of the lazy-reduction contract, which finished proofs never produce."""
import functools
import os
import struct
import sys

import pytest

from oracle import coracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ntt_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

P = R.P
SIZES = [4, 9, 10, 11, 12, 14, 16]       # 4: the smallest coset-major transform; 11: the 512-lane kernel; 16: the last size of the raw forms
BATCH = {4: 6, 9: 5, 10: 4, 11: 5, 12: 4, 14: 3, 16: 3}
SCALE = 0x0BADC0DE_12345678_9ABCDEF0_0F1E2D3C_4B5A6978_87960504_03020100_F00DFACE % P
POOL = 42 * 16                           # 16 blocks of every (m, limb pattern) pair: 6 on the edge residues, 10 seeded


@functools.lru_cache(maxsize=None)
def _pool():
    return R.bound_records(POOL, b"fs9 bound records")


def test_the_pool_reaches_the_contract_bounds():
    limbs = R.fs9_unpack(b"".join(rec for rec, _, _ in _pool()))
    low = [l for rec in limbs for l in rec[:8]]
    assert max(low) >= R.LIMB_HI - 16 and min(low) <= R.LIMB_LO + 4 and R.LIMB_LO < min(low) and max(low) < R.LIMB_HI
    values = [R.fs9_value(rec) for rec in limbs]
    assert max(values) == R.VALUE_BOUND - 1 and min(values) <= -3 * P + 1 and all(abs(v) < R.VALUE_BOUND for v in values)
    assert {(v - R.fs9_value(c)) // P for v, c in zip(values, R.fs9_unpack(b"".join(c for _, c, _ in _pool())))} == set(range(-3, 4))
    for (rec, canon, x), v in zip(_pool(), values):
        assert v * R.R_INV % P == x == R.fs9_value(R.fs9_unpack(canon)[0]) * R.R_INV % P


def _directions(log2n):
    w = R.omega(log2n)
    return {"forward": (w, None), "inverse": (pow(w, -1, P), pow(1 << log2n, -1, P)), "scaled": (w, SCALE)}


def _oracle(values_raw, log2n, batch, w, sc):
    n = 1 << log2n
    return b"".join(coracle.ntt_raw(values_raw[32 * n * b : 32 * n * (b + 1)], n, w, sc) for b in range(batch))


def _fs9_vector(count, tag):
    """count records from the pool: (records on the contract bounds, their canonical images, the 32-byte values they stand for)"""
    pool = _pool()
    idx = R.pick(count, len(pool), tag)
    return b"".join(pool[i][0] for i in idx), b"".join(pool[i][1] for i in idx), b"".join(R.b32(pool[i][2]) for i in idx)


def _check_fs9_output(raw, want_std, with_factor):
    """decode FS9 records, compare the values they stand for, and hold them to the documented output form"""
    assert len(raw) // 36 * 32 == len(want_std)
    got, top = bytearray(), 1 << 29
    for rec in struct.iter_unpack("<9i", raw):
        l0, l1, l2, l3, l4, l5, l6, l7, l8 = rec
        v = l0 + (l1 << 29) + (l2 << 58) + (l3 << 87) + (l4 << 116) + (l5 << 145) + (l6 << 174) + (l7 << 203) + (l8 << 232)
        assert min(rec[:8]) >= 0 and max(rec[:8]) < top, rec
        if with_factor:
            assert -P // 2 < v < 3 * P // 2, rec               # a product: normal
        else:
            assert abs(v) * 100 < 51 * P, rec                  # reduce_small
        got += (v * R.R_INV % P).to_bytes(32, "little")
    assert bytes(got) == want_std, R.first_diffs(bytes(got), want_std)


def _std_vector(count, tag):
    """canonical elements: the edge values, then seeded ones"""
    raw = bytearray(R.stream_elements(count, tag))
    for i, v in enumerate((0, 1, P - 1, (P - 1) // 2, (P + 1) // 2, P - 2)[:count]):
        raw[32 * i : 32 * i + 32] = R.b32(v)
    return bytes(raw)


@pytest.mark.parametrize("log2n", SIZES)
def test_std8_separate_source_inverse(ctx, log2n):
    """what the witness interpolation runs: STD8 in from a separate buffer, STD8 out, inverse with 1/n"""
    batch = BATCH[log2n]
    w, sc = _directions(log2n)["inverse"]
    src = _std_vector(batch << log2n, b"std8 %d" % log2n)
    got = ctx.ntt_formats_selftest(src, log2n, batch, w, sc, R.STD8, R.STD8)
    want = _oracle(src, log2n, batch, w, sc)
    assert got == want, R.first_diffs(got, want)


@pytest.mark.parametrize("log2n", SIZES)
def test_std8_scaled_to_fs9(ctx, log2n):
    """the coset evaluations: transform x reads coefficient vector x // 3 and multiplier table x % 3 (records holding s R^2);
    forward, no factor, raw output through reduce_small.  Two coefficient vectors, so x // 3 and x % 3 both vary."""
    n, div, polys = 1 << log2n, 3, 2
    edge = (0, 1, P - 1, (P - 1) // 2, (P + 1) // 2)
    coef = [R.ints_of(R.stream_elements(n, b"scaled coef %d %d" % (log2n, q))) for q in range(polys)]
    mult = [R.ints_of(R.stream_elements(n, b"scaled mult %d %d" % (log2n, c))) for c in range(div)]
    for i in range(min(n, 25)):                                 # every pair of edge values, shifted per vector and per table
        for q in range(polys):
            coef[q][i] = edge[(i + q) % 5]
        for c in range(div):
            mult[c][i] = edge[(i // 5 + c) % 5]
    src = b"".join(R.b32(a) for q in range(polys) for a in coef[q])
    r2 = R.R * R.R % P
    table = b"".join(R.fs9_pack(R.fs9_limbs(s * r2 % P)) for c in range(div) for s in mult[c])
    w, _ = _directions(log2n)["forward"]
    got = ctx.ntt_formats_selftest(src, log2n, polys * div, w, None, R.STD8_SCALED, R.FS9, src_div=div, in_scale=table)
    product = b"".join(R.b32(coef[x // div][i] * mult[x % div][i] % P) for x in range(polys * div) for i in range(n))
    _check_fs9_output(got, _oracle(product, log2n, polys * div, w, None), with_factor=False)


def _coset_vectors(log2n, batch):
    """(source on the bounds, its canonical image, special rows on the bounds, their canonical image, the 4N-point vectors as
    values): point idx is coset idx % 4, row idx // 4; cosets 1..3 coset-major, coset 0 zero but for its last three rows"""
    n = 1 << log2n
    nq = n // 4
    src, src_canon, src_val = _fs9_vector(batch * 3 * nq, b"coset rows %d" % log2n)
    spc, spc_canon, spc_val = _fs9_vector(batch * 3, b"special rows %d" % log2n)
    zero, values = bytes(32), bytearray()
    for x in range(batch):
        for idx in range(n):
            c, j = idx % 4, idx // 4
            if c:
                at = (x * 3 + (c - 1)) * nq + j
                values += src_val[32 * at : 32 * at + 32]
            elif j >= nq - 3:
                at = x * 3 + (j - (nq - 3))
                values += spc_val[32 * at : 32 * at + 32]
            else:
                values += zero
    return src, src_canon, spc, spc_canon, bytes(values)


@pytest.mark.parametrize("log2n", SIZES)
def test_fs9_cosets_to_std8(ctx, log2n):
    """the quotient's interpolation: coset-major FS9 in (aggregated constraint values: the widest records of the prover), STD8
    out, inverse with 1/n.  The records on the bounds and their canonical images give the same bytes, the oracle's."""
    batch = BATCH[log2n]
    w, sc = _directions(log2n)["inverse"]
    src, src_canon, spc, spc_canon, values = _coset_vectors(log2n, batch)
    assert any(values[32 * (4 * ((1 << log2n) // 4 - 3)) :][:32])             # the first special row is not zero: its index matters
    want = _oracle(values, log2n, batch, w, sc)
    got = ctx.ntt_formats_selftest(src, log2n, batch, w, sc, R.FS9_COSETS, R.STD8, special=spc)
    assert got == want, R.first_diffs(got, want)
    canon = ctx.ntt_formats_selftest(src_canon, log2n, batch, w, sc, R.FS9_COSETS, R.STD8, special=spc_canon)
    assert canon == got, R.first_diffs(canon, got)


@pytest.mark.parametrize("direction,fmt_out", [("forward", R.FS9), ("scaled", R.FS9), ("inverse", R.STD8)])
@pytest.mark.parametrize("log2n", SIZES)
def test_fs9_input(ctx, log2n, direction, fmt_out):
    """FS9 records in, on the bounds and canonical: raw output without a factor (reduce_small), with one (a product), and STD8"""
    batch = BATCH[log2n]
    w, sc = _directions(log2n)[direction]
    src, src_canon, values = _fs9_vector(batch << log2n, b"fs9 in %d" % log2n)
    want = _oracle(values, log2n, batch, w, sc)
    got = ctx.ntt_formats_selftest(src, log2n, batch, w, sc, R.FS9, fmt_out)
    canon = ctx.ntt_formats_selftest(src_canon, log2n, batch, w, sc, R.FS9, fmt_out)
    if fmt_out == R.STD8:
        assert got == want, R.first_diffs(got, want)
        assert canon == got
    else:
        _check_fs9_output(got, want, with_factor=sc is not None)
        _check_fs9_output(canon, want, with_factor=sc is not None)


@pytest.mark.parametrize("fmt_out", [R.STD8, R.FS9])
@pytest.mark.parametrize("pad", [1, 2])
@pytest.mark.parametrize("log2n", [10, 12])
def test_zero_padded_source(ctx, log2n, pad, fmt_out):
    """pad > 0: the source holds n / 2^pad coefficients; the transform is that of the vector padded with zeros to n"""
    batch, n = 3, 1 << log2n
    w, sc = _directions(log2n)["forward"]
    src = _std_vector(batch * (n >> pad), b"padded %d %d" % (log2n, pad))
    short = 32 * (n >> pad)
    padded = b"".join(src[short * b : short * (b + 1)] + bytes(32 * n - short) for b in range(batch))
    want = _oracle(padded, log2n, batch, w, sc)
    got = ctx.ntt_formats_selftest(src, log2n, batch, w, sc, R.STD8, fmt_out, pad=pad)
    if fmt_out == R.STD8:
        assert got == want, R.first_diffs(got, want)
    else:
        _check_fs9_output(got, want, with_factor=False)


def test_std8_to_fs9_with_a_factor_above_the_raw_limit(ctx):
    """2^17: beyond the raw forms, a STD8 source with a factor on the way out is still served (and right)"""
    log2n, batch = 17, 1
    w, sc = _directions(log2n)["scaled"]
    src = _std_vector(batch << log2n, b"std8 17")
    _check_fs9_output(ctx.ntt_formats_selftest(src, log2n, batch, w, sc, R.STD8, R.FS9), _oracle(src, log2n, batch, w, sc), with_factor=True)


def test_refusals_launch_nothing(ctx):
    """what the kernels' bookkeeping does not cover is refused before any launch"""
    w17, w3, w9 = R.omega(17), R.omega(3), R.omega(9)
    n17, n9 = 1 << 17, 1 << 9
    table9 = bytes(36 * 3 * n9)
    cases = {
        "FS9 input at 2^17": dict(src=bytes(36 * n17), log2n=17, batch=1, omega=w17, scale=SCALE, fmt_in=R.FS9, fmt_out=R.STD8),
        "coset-major input at 2^17": dict(src=bytes(36 * 3 * (n17 // 4)), log2n=17, batch=1, omega=w17, scale=SCALE, fmt_in=R.FS9_COSETS,
                                          fmt_out=R.STD8, special=bytes(108)),
        "raw output without a factor at 2^17": dict(src=bytes(32 * n17), log2n=17, batch=1, omega=w17, fmt_in=R.STD8, fmt_out=R.FS9),
        "coset-major input at 2^3": dict(src=bytes(36 * 3 * 2 * 2), log2n=3, batch=2, omega=w3, scale=SCALE, fmt_in=R.FS9_COSETS,
                                         fmt_out=R.STD8, special=bytes(108 * 2)),
        "coset-major input without special rows": dict(src=bytes(36 * 3 * (n9 // 4)), log2n=9, batch=1, omega=w9, scale=SCALE,
                                                       fmt_in=R.FS9_COSETS, fmt_out=R.STD8),
        "scaled input without a table": dict(src=bytes(32 * n9), log2n=9, batch=3, omega=w9, fmt_in=R.STD8_SCALED, fmt_out=R.FS9, src_div=3),
        "scaled input with padding": dict(src=bytes(32 * (n9 // 2)), log2n=9, batch=3, omega=w9, fmt_in=R.STD8_SCALED, fmt_out=R.FS9,
                                          src_div=3, pad=1, in_scale=table9[: len(table9) // 2]),
    }
    kernels = ("k_ntt_twiddles", "k_ntt_local", "k_ntt_strided")
    ctx.prof_reset()
    ctx.prof_enable(True)
    try:
        for what, args in cases.items():
            with pytest.raises(ValueError, match="NTT refused"):
                ctx.ntt_formats_selftest(**args)
            assert [ctx.prof_get(k)[1] for k in kernels] == [0, 0, 0], what
        # the counters do count: the last case, made admissible, launches
        ok = dict(cases["scaled input with padding"], src=bytes(32 * n9), pad=0, in_scale=table9)
        assert ctx.ntt_formats_selftest(**ok) == bytes(36 * 3 * n9)
        assert ctx.prof_get("k_ntt_local")[1] == 1
    finally:
        ctx.prof_enable(False)
        ctx.prof_reset()
