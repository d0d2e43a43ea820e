"""CPU: the register-image builders and the affine reference behind tests/test_gpu_fq28_g1_ops.py (oracle/fq28_forms.py)
decode to the values they are meant to hold, satisfy the forms they claim, and agree with the C oracle's G1 arithmetic — the
reference half of the device test, checked without a GPU."""
import random

import test_montmul_gen

from oracle import coracle
from oracle import fq28_forms as F

P = F.P


def test_constants_match_the_device_parameters():
    assert P == coracle.FP_P and F.R == 1 << 392
    assert F.value(F.P_LIMBS) == P
    # Fq28Params (csrc/fq28.hip.h): P limbs, ONE = R mod p
    assert F.P_LIMBS[0] == 0xFFFAAAB and F.P_LIMBS[13] == 0x001A011
    assert F.normal(F.R % P)[:3] == [0x347FCB8, 0xD800000, 0x002B119]
    assert F.on_curve(F.G1_GEN)
    fq = test_montmul_gen.CASES[0]
    assert fq["p"] == P and fq["n"] == F.NL and fq["bits"] == F.BITS
    assert (fq["shapes"], fq["extreme"], fq["sqr_shape"], fq["mul2_shape"]) == (F.MUL_SHAPES, F.MUL_EXTREME, F.SQR_SHAPE, F.MUL2_SHAPE)


def test_limb_images_hold_their_values_and_forms():
    rng = random.Random(1)
    edges = [0, 1, P - 1, P, P + 1, -1, -P, -P - 1, 8 * P - 1, -(8 * P - 1), 5 * P, -5 * P, (1 << 384) - 1]
    for v in edges + [rng.randrange(-32 * P, 32 * P) for _ in range(500)]:
        n = F.normal(v)
        assert F.value(n) == v and F.is_n(n) and len(n) == F.NL
        w = rng.randrange(P)
        d = F.d_image(v, w)
        assert F.value(d) == v and F.is_d(d)
        s = F.scramble(n, rng, 3)
        assert F.value(s) == v and F.max_limb(s) < (4 << 28) + 3
    for lb, vb in ((1 << 28, 2), (1 << 30, 31), (1 << 29, 8)):
        for _ in range(50):
            l = F.lazy(rng, lb, vb)
            assert F.max_limb(l) < lb and abs(F.value(l)) < vb * P
    for sign in (1, -1):
        e = F.extreme(1 << 29, sign)
        assert F.max_limb(e) == (1 << 29) - 1 and e[-1] == 3 * sign
    for v in (0, 1, P - 1, (1 << 384) - 1):
        assert F.from_words(F.words12(v)) == v
    raw = F.pack_i32([-1, 0, 0xFFFFFFFF, 1 << 31, -(1 << 31)])
    assert F.unpack_i32(raw) == [-1, 0, -1, -(1 << 31), -(1 << 31)]
    # some d images really have negative limbs (y is fed to the device that way)
    assert any(x < 0 for x in F.d_image(F.to_mont(5), rng.randrange(P)))


def test_affine_reference_agrees_with_the_c_oracle():
    rng = random.Random(2)
    g = F.G1_GEN
    pts = [coracle.g1_mul(g, rng.randrange(1, coracle.FR_P)) for _ in range(12)]
    for k in (1, 2, 3, 255, rng.randrange(coracle.FR_P)):
        assert F.mul(g, k) == coracle.g1_mul(g, k)
    assert F.mul(g, coracle.FR_P) is None and F.mul(g, 0) is None
    for a in pts:
        assert F.on_curve(a)
        assert F.dbl(a) == coracle.g1_add(a, a)
        assert F.add(a, F.neg(a)) is None and coracle.g1_add(a, F.neg(a)) is None
        assert F.add(a, None) == a and F.add(None, a) == a
        for b in pts[:4]:
            assert F.add(a, b) == coracle.g1_add(a, b)
    assert F.dbl(None) is None and F.add(None, None) is None


def test_register_images_decode_to_their_points():
    rng = random.Random(3)
    pts = [coracle.g1_mul(F.G1_GEN, rng.randrange(1, coracle.FR_P)) for _ in range(20)] + [None]
    for pt in pts:
        for x_shift in (-1, 0, 1):
            for zz_shift in (0, -1):
                for y_form in ("d", "n"):
                    z = rng.choice([1, 2, P - 1, rng.randrange(1, P)])
                    img = F.xyzz_image(pt, z, rng, x_shift, zz_shift, y_form)
                    assert len(img) == F.XYZZ_RAW_WORDS
                    got, consistent = F.decode_xyzz(img)
                    assert consistent and got == pt
                    if pt is None:
                        assert img == [0] * 56 + [1]
                        continue
                    x, y, zz, zzz, _ = F.split_xyzz(img)
                    assert F.is_n(x) and -5 * P < F.value(x) < 3 * P
                    assert F.is_d(y) and abs(F.value(y)) < 2 * P
                    for c in (zz, zzz):
                        assert F.is_n(c) and -P // 2 < F.value(c) < P + P // 2
        for x_shift in (-1, 0, 1):
            for y_form in ("n", "d", "cneg"):
                img = F.affine_image(pt, rng, x_shift, y_form)
                assert len(img) == 2 * F.NL + 1 and F.decode_affine(img) == pt
                if pt is not None:
                    assert F.is_n(img[: F.NL]) and F.is_d(img[F.NL : 2 * F.NL])
                    if y_form == "cneg":              # limb-wise negation of an N image: limbs in (-2^28, 0]
                        assert all(x <= 0 for x in img[F.NL : 2 * F.NL])
    # an inconsistent image (ZZ^3 != ZZZ^2) is reported as such
    img = F.xyzz_image(pts[0], 7, rng)
    img[3 * F.NL] += 1
    assert F.decode_xyzz(img)[1] is False
