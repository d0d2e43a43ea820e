"""GPU: the public NTT (dr_ntt / dr_ntt_dev) at the sizes whose pass shapes nothing else runs — 2^15 .. 2^20: a second and a third
strided pass, one to four row bits, the 2 x 512 tile — bit for bit against the CPU oracle, on structured inputs whose transforms are
also known in closed form or by a direct big-integer sum.  2^21 .. 2^24 repeat the four-bit pass and are not run."""
import functools
import os
import sys

import pytest

from oracle import coracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ntt_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

P = R.P
SCALE = 0x1234567_89ABCDEF_0FEDCBA9_87654321_DEADBEEF_CAFEF00D_01234567_89ABCDEF % P      # "an arbitrary scale"
KINDS = ("random", "all_p_minus_1", "sparse", "alternating")
PARTNER = {"random": "sparse", "sparse": "random", "all_p_minus_1": "alternating", "alternating": "all_p_minus_1"}
DIRECTIONS = ("forward", "inverse", "scaled")


def test_the_roots_of_unity_are_primitive():
    assert pow(R.G32, 1 << 31, P) == P - 1
    for k in (1, 15, 20):
        assert pow(R.omega(k), 1 << (k - 1), P) == P - 1


def _sparse_entries(log2n):
    n = 1 << log2n
    pos = sorted({0, 1, (1 << 10) - 1, 1 << 10, (1 << 14) - 1, 1 << 14, n // 2 - 1, n // 2, n - 1})      # pass and tile boundaries
    vals = R.ints_of(R.stream_elements(len(pos), b"sparse values"))
    vals[0], vals[-1] = P - 1, 1
    assert all(vals)
    return dict(zip(pos, vals))


@functools.lru_cache(maxsize=None)
def _input(log2n, kind):
    n = 1 << log2n
    if kind == "random":
        return R.stream_elements(n)
    if kind == "all_p_minus_1":
        return R.b32(P - 1) * n
    if kind == "alternating":
        return (R.b32(P - 1) + R.b32(0)) * (n // 2)
    raw = bytearray(32 * n)
    for j, v in _sparse_entries(log2n).items():
        raw[32 * j : 32 * j + 32] = R.b32(v)
    return bytes(raw)


def _params(log2n, direction):
    """(omega, scale) of a direction"""
    w = R.omega(log2n)
    if direction == "forward":
        return w, None
    if direction == "inverse":
        return pow(w, -1, P), pow(1 << log2n, -1, P)
    return w, SCALE


@functools.lru_cache(maxsize=None)
def _oracle_shared(log2n, kind, direction):
    w, sc = _params(log2n, direction)
    return coracle.ntt_raw(_input(log2n, kind), 1 << log2n, w, sc)


def _oracle(log2n, kind, direction):
    # up to 2^18 a transform is checked twice (as the first and as the second of a batch): computed once; above, once each
    return (_oracle_shared if log2n <= 18 else _oracle_shared.__wrapped__)(log2n, kind, direction)


def _check_closed_forms(log2n, kind, direction, out):
    """what the transform must be, without the oracle"""
    n = 1 << log2n
    w, sc = _params(log2n, direction)
    sc = 1 if sc is None else sc
    zero = bytes(32)
    if kind == "all_p_minus_1":                     # (p - 1) sum_j w^(i j): -n at i = 0, nothing elsewhere
        assert out[:32] == R.b32(-n * sc % P) and out[32:] == zero * (n - 1)
    if kind == "alternating":                       # (p - 1) sum_(j even) w^(i j): -n/2 at i = 0 and i = n/2
        lead = R.b32(-(n // 2) * sc % P)
        assert out[:32] == lead and out[32 * (n // 2) : 32 * (n // 2) + 32] == lead
        assert out[32 : 32 * (n // 2)] == zero * (n // 2 - 1) and out[32 * (n // 2) + 32 :] == zero * (n // 2 - 1)
    if kind == "sparse":                            # sum_j v_j w^(i j) with Python integers
        entries = _sparse_entries(log2n)
        for i in (0, 1, n - 1, n // 3, n // 2 + 1, (1 << 14) + 1):
            want = sum(v * pow(w, i * j, P) for j, v in entries.items()) * sc % P
            assert out[32 * i : 32 * i + 32] == R.b32(want), i


@pytest.mark.parametrize("direction", DIRECTIONS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("log2n", [15, 16, 17, 18, 19, 20])
def test_ntt_pass_shapes_match_oracle(ctx, log2n, kind, direction):
    """15: a second strided pass of one row bit (2 x 512 tile); 16, 17: two and three row bits; 18: two four-bit passes; 19, 20: a
    third pass.  Two transforms per call up to 2^18 (this input and its partner), one above."""
    n = 1 << log2n
    kinds = (kind, PARTNER[kind]) if log2n <= 18 else (kind,)
    w, sc = _params(log2n, direction)
    got = ctx.ntt(b"".join(_input(log2n, k) for k in kinds), log2n, w, sc)
    assert len(got) == 32 * n * len(kinds)
    for b, k in enumerate(kinds):
        out, want = got[32 * n * b : 32 * n * (b + 1)], _oracle(log2n, k, direction)
        assert out == want, (log2n, k, direction, b, R.first_diffs(out, want))
    _check_closed_forms(log2n, kind, direction, got[: 32 * n])


def test_ntt_dev_on_a_device_buffer_2_15(ctx):
    """the same bytes through dr_ntt_dev: in place on a caller's buffer, forward and back"""
    log2n, n = 15, 1 << 15
    data = _input(log2n, "random") + _input(log2n, "sparse")
    buf = ctx.alloc(len(data))
    try:
        buf.upload(data)
        ctx.ntt_dev(buf, log2n, 2, *_params(log2n, "forward"))
        fwd = buf.download()
        for b, k in enumerate(("random", "sparse")):
            want = _oracle(log2n, k, "forward")
            assert fwd[32 * n * b : 32 * n * (b + 1)] == want, (k, R.first_diffs(fwd[32 * n * b : 32 * n * (b + 1)], want))
        ctx.ntt_dev(buf, log2n, 2, *_params(log2n, "inverse"))
        assert buf.download() == data
    finally:
        buf.free()


def test_twiddle_cache_eviction(ctx):
    """The context keeps 16 twiddle tables, first in first out.  17 (size, root) pairs that nothing else uses, then the first one
    again: 18 tables are built (the first pair's twice), and every transform matches the oracle."""
    pairs = [(5, pow(R.omega(5), e, P)) for e in range(3, 32, 2)] + [(6, pow(R.omega(6), e, P)) for e in (3, 5)]
    assert len(set(pairs)) == 17 and all(pow(w, 1 << (k - 1), P) == P - 1 for k, w in pairs)
    ctx.prof_reset()
    ctx.prof_enable(True)
    try:
        for k, w in pairs + pairs[:1] + pairs[-1:]:
            data = R.stream_elements(3 << k, b"eviction %d" % k)
            got = ctx.ntt(data, k, w, SCALE)
            for b in range(3):
                assert got[(32 << k) * b : (32 << k) * (b + 1)] == coracle.ntt_raw(data[(32 << k) * b : (32 << k) * (b + 1)], 1 << k, w, SCALE), (k, w, b)
        assert ctx.prof_get("k_ntt_twiddles")[1] == 18          # the last call's table was still cached
    finally:
        ctx.prof_enable(False)
        ctx.prof_reset()
