"""ORACLE (test infrastructure only) — raw register images of the G1 kernels' base field and a plain affine reference.

The G1 kernels compute in the unsaturated Fq of dot_ring_amd/csrc/fq28.hip.h: 14 signed 32-bit limbs of 28 bits, value
sum l_i 2^(28 i), Montgomery form x -> x R mod p with R = 2^392, lazy reduction.  This module builds limb images of given
values in the register forms the headers name, classifies images the device returns, decodes XYZZ images
(csrc/g1.hip.h, put_raw layout) and restates the group law in affine coordinates over plain integers.

Register forms (limbs 0..12; limb 13 is the signed top limb and only bounded through the value):
  N  "normal"  limbs in [0, 2^28)              mul / sqr / mul2 / carry outputs, unpacked canonical words
  d            |limb| < 2^28                   difference of two N images
Value ranges of the group law's outputs (each is computed fresh from products, so chains do not widen them):
  mul / sqr / mul2 output              (-p/2, 1.5 p)
  x = carry(sqr - 3 products)          (-5 p, 3 p)      madd / add;  dbl: carry(sqr - 2 products) in (-3.5 p, 2.5 p)
  y (add, dbl: product - product)      (-2 p, 2 p)      madd: mul2 output, normal
  zz, zzz                              (-p/2, 1.5 p)    products (R mod p after g1_from_affine)
What the consumers need: mul |a|, |b| < 32 p and 14 max|a_i| max|b_j| + 2^60 < 2^63; sqr |a_i| <= 2^29; mul2 one operand with
limbs < 2^29, the others < 2^28; canon28 / is_zero_mod_p |value| < 8 p.  The ranges above keep every consumer inside: the
largest is madd's P = U2 - x in (-3.5 p, 6.5 p) read by is_zero_mod_p.
"""
from __future__ import annotations

import array
import random

from . import coracle

P = coracle.FP_P
NL, BITS = 14, 28
MASK = (1 << BITS) - 1
R = 1 << (NL * BITS)
R_INV = pow(R, -1, P)
P_LIMBS = [(P >> (BITS * i)) & MASK for i in range(NL)]
B = 4                                         # y^2 = x^3 + 4
G1_GEN = (
    0x17F1D3A73197D7942695638C4FA9AC0FC3688C4F9774B905A14E3A3F171BAC586C55E83FF97A1AEFFB3AF00ADB22C6BB,
    0x08B3F481E3AAA0F1A09E30ED741D8AE4FCF5E095D5D00AF600DB18CB2C04B3EDD03CC744A2888AE40CAA232946C5E7E1,
)

XYZZ_RAW_WORDS = 4 * NL + 1                  # x, y, zz, zzz limbs, then the infinity flag

# operand shapes of the products the kernels use (limb bound a, limb bound b, |a| / p, |b| / p) — the Fq row of
# tests/test_montmul_gen.py CASES, which runs the generated asm text on them; here they go to the built code objects
MUL_SHAPES = [(1 << 28, 1 << 28, 2, 2), (1 << 30, 1 << 28, 31, 31), (1 << 29, 1 << 29, 31, 31), (1 << 28, 1 << 30, 8, 31)]
MUL_EXTREME = (1 << 30, 1 << 28)
SQR_SHAPE = (1 << 29, 31)
MUL2_SHAPE = ((1 << 29, 8), (1 << 28, 8), (1 << 28, 4), (1 << 28, 2))


# ---------------------------------------------------------------- limb images
def value(limbs) -> int:
    return sum(int(x) << (BITS * i) for i, x in enumerate(limbs))


def normal(v: int) -> list[int]:
    """the carry-normal image of v: limbs 0..12 in [0, 2^28), the rest (signed, floor) in limb 13 — what carry() gives"""
    return [(v >> (BITS * i)) & MASK for i in range(NL - 1)] + [v >> (BITS * (NL - 1))]


def d_image(v: int, w: int) -> list[int]:
    """v as a "d": the limb-wise difference of the N images of v + w and of w (limbs of both signs when w is random)"""
    return [x - y for x, y in zip(normal(v + w), normal(w))]


def scramble(limbs, rng: random.Random, k: int = 1) -> list[int]:
    """the same value with carries moved between neighbouring limbs: limb i gains t 2^28, limb i + 1 loses t, |t| <= k
    (an N image then has |limb| < (k + 1) 2^28 + k)"""
    l = list(limbs)
    for i in range(NL - 1):
        t = rng.randint(-k, k)
        l[i] += t << BITS
        l[i + 1] -= t
    return l


def lazy(rng: random.Random, limb_bound: int, value_bound_p: float) -> list[int]:
    """random limbs with |limb| < limb_bound (limbs 0..12) and |value| < value_bound_p * p"""
    vb = int(value_bound_p * P)
    top = vb >> (BITS * (NL - 1))
    while True:
        l = [rng.randrange(-limb_bound + 1, limb_bound) for _ in range(NL - 1)] + [rng.randrange(-top, top + 1)]
        if abs(value(l)) < vb:
            return l


def extreme(limb_bound: int, sign: int) -> list[int]:
    """every limb at +-(bound - 1), top limb +-3: the largest column sums a product can meet"""
    return [sign * (limb_bound - 1)] * (NL - 1) + [sign * 3]


def is_n(limbs) -> bool:
    return all(0 <= x <= MASK for x in limbs[: NL - 1])


def is_d(limbs) -> bool:
    return all(-(1 << BITS) < x < (1 << BITS) for x in limbs[: NL - 1])


def max_limb(limbs) -> int:
    return max(abs(x) for x in limbs[: NL - 1])


def words12(v: int) -> list[int]:
    """12 little-endian 32-bit words of 0 <= v < 2^384 (the memory form)"""
    return [(v >> (32 * j)) & 0xFFFFFFFF for j in range(12)]


def from_words(words) -> int:
    return sum((int(w) & 0xFFFFFFFF) << (32 * j) for j, w in enumerate(words))


def to_mont(x: int) -> int:
    return x * R % P


def from_mont(v: int) -> int:
    return v * R_INV % P


def pack_i32(words) -> bytes:
    """signed or unsigned 32-bit words -> little-endian bytes"""
    return array.array("i", [((int(w) + (1 << 31)) & 0xFFFFFFFF) - (1 << 31) for w in words]).tobytes()


def unpack_i32(raw: bytes) -> list[int]:
    return array.array("i", raw).tolist()


# ---------------------------------------------------------------- affine reference (None = infinity)
def on_curve(pt) -> bool:
    return pt is None or (pt[1] * pt[1] - pt[0] ** 3 - B) % P == 0


def neg(pt):
    return None if pt is None else (pt[0], (-pt[1]) % P)


def dbl(pt):
    if pt is None or pt[1] == 0:
        return None
    x, y = pt
    lam = 3 * x * x * pow(2 * y, -1, P) % P
    x3 = (lam * lam - 2 * x) % P
    return x3, (lam * (x - x3) - y) % P


def add(a, b):
    if a is None:
        return b
    if b is None:
        return a
    if a[0] == b[0]:
        return dbl(a) if a[1] == b[1] else None
    lam = (b[1] - a[1]) * pow(b[0] - a[0], -1, P) % P
    x3 = (lam * lam - a[0] - b[0]) % P
    return x3, (lam * (a[0] - x3) - a[1]) % P


def mul(pt, k: int):
    acc = None
    for bit in bin(k)[2:] if k > 0 else "":
        acc = dbl(acc)
        if bit == "1":
            acc = add(acc, pt)
    return acc


# ---------------------------------------------------------------- XYZZ / affine register images
def xyzz_image(pt, z: int, rng: random.Random, x_shift: int = 0, zz_shift: int = 0, y_form: str = "d") -> list[int]:
    """57 words: P = (x, y) as X = x Z^2, Y = y Z^3, ZZ = Z^2, ZZZ = Z^3 (Montgomery), infinity as g1_inf().
    x_shift: the x limbs hold the representative X + x_shift p (any of -1, 0, 1 stays in x's range (-5 p, 3 p));
    zz_shift = -1 takes ZZ - p and ZZZ - p where they stay above -p/2 (normal); y_form "d" (a difference of two N images) or "n"."""
    if pt is None:
        return [0] * (4 * NL) + [1]
    zz, zzz = z * z % P, z * z * z % P
    xm, ym = to_mont(pt[0] * zz), to_mont(pt[1] * zzz)
    zzm, zzzm = to_mont(zz), to_mont(zzz)
    if zz_shift < 0:
        zzm, zzzm = (zzm - P if zzm > P // 2 else zzm), (zzzm - P if zzzm > P // 2 else zzzm)
    y = d_image(ym - rng.randrange(2) * P, rng.randrange(P)) if y_form == "d" else normal(ym)
    return normal(xm + x_shift * P) + y + normal(zzm) + normal(zzzm) + [0]


def affine_image(pt, rng: random.Random, x_shift: int = 0, y_form: str = "n") -> list[int]:
    """29 words: x limbs, y limbs, infinity flag.  y_form "n" (unpacked canonical words, as load_affine), "d", or "cneg": the
    limb-wise negation of the N image of -y (what g1_neg_affine makes of a loaded point)"""
    if pt is None:
        return [0] * (2 * NL) + [1]
    xm, ym = to_mont(pt[0]), to_mont(pt[1])
    if y_form == "cneg":
        y = [-x for x in normal(to_mont((-pt[1]) % P))]
    elif y_form == "d":
        y = d_image(ym, rng.randrange(P))
    else:
        y = normal(ym)
    return normal(xm + x_shift * P) + y + [0]


def split_xyzz(words):
    """57 words -> (x, y, zz, zzz limb lists, inf flag)"""
    w = list(words)
    return w[0:NL], w[NL : 2 * NL], w[2 * NL : 3 * NL], w[3 * NL : 4 * NL], w[4 * NL]


def decode_xyzz(words):
    """the affine point an XYZZ image stands for (None for the flag) and whether ZZ^3 == ZZZ^2 (mod p) holds"""
    x, y, zz, zzz, inf = split_xyzz(words)
    if inf & 0xFFFFFFFF:
        return None, True
    X, Y, ZZ, ZZZ = (from_mont(value(c)) for c in (x, y, zz, zzz))
    consistent = ZZ != 0 and (ZZ**3 - ZZZ**2) % P == 0
    if not consistent:
        return ("inconsistent", X, Y, ZZ, ZZZ), False
    return (X * pow(ZZ, -1, P) % P, Y * pow(ZZZ, -1, P) % P), True


def decode_affine(words):
    x, y, inf = list(words[:NL]), list(words[NL : 2 * NL]), words[2 * NL]
    if inf & 0xFFFFFFFF:
        return None
    return from_mont(value(x)), from_mont(value(y))
