// The group law of P-521 (DR_CURVE_P521_RO / DR_CURVE_P521_NU; the reference's specs/p521.py): y^2 = x^3 - 3 x + b over p = 2^521 - 1
// (fp521.hip.h), prime order, cofactor 1.  Homogeneous projective (X : Y : Z), x = X / Z, y = Y / Z, identity (0 : 1 : 0), standard
// form.  The law is the complete one of Renes, Costello and Batina (2016), algorithms 4 (addition) and 6 (doubling) for a = -3, restated
// over this field from kernels_p256.hip.h (whose fused pairs and Montgomery reductions belong to its field): no exceptional cases
// (P + P, P + (-P), the identity on either side) and no branches.  b is a full-width constant in standard form.
//
// The comments give the limb class of every intermediate against fp521.hip.h's contract ("n" = normal, "k n" = |limb| <= k normal; mul
// needs ka kb <= 6, sqr 2 n).  A point's coordinates are x: 1 n, y: n (1 n once negated), z: n, in and out.
//
// The map's description for sswu.hip.h is here as well, so that the host can check it, and the window count of the fixed schedule.
// Plain integer C++ like fp521.hip.h: compiles for the device and, with g++, for the host (tests/native/p521_host_check.cpp, where
// -fsanitize=undefined turns a signed 64-bit column overflow into an abort).
#pragma once
#include "fp521.hip.h"

namespace dr {

struct P521Consts {
    // b = 0x0051953eb9618e1c9a1f929a21a0b68540eea2da725b99b315f3b8b489918ef109e156193951ec7e937b1652c0bd3bb1bf073573df883d2c34f1ef451fd46b503f00
    static constexpr int32_t B[L521] = {0xb503f00, 0x451fd46, 0xc34f1ef, 0xdf883d2, 0xf073573, 0xbd3bb1b, 0xb1652c0, 0xec7e937, 0x6193951, 0xf109e15,
                                        0x489918e, 0x15f3b8b, 0x25b99b3, 0xeea2da7, 0x0b68540, 0x929a21a, 0xe1c9a1f, 0x3eb9618, 0x0005195};
};

struct P521Point {
    F521 x, y, z;
};

DR_L28_FN F521 p521_b() {       // (not F521::constant<>: through it the compiler loads b from memory and the law's kernels change)
    F521 r;
#pragma unroll
    for (int i = 0; i < L521; i++) r.l[i] = P521Consts::B[i];
    return r;
}
DR_L28_FN P521Point p521_identity() { return {F521::zero(), F521::small(1), F521::zero()}; }
DR_L28_FN P521Point p521_from_affine(const F521& x, const F521& y) { return {x, y, F521::small(1)}; }
DR_L28_FN bool p521_is_identity(const P521Point& p) { return is_zero(p.z); }
DR_L28_FN P521Point p521_cneg(const P521Point& p, bool negate) { return {p.x, cneg(p.y, negate), p.z}; }

// algorithm 6, a = -3: 8 products (two by b) and 3 squarings
DR_L28_FN P521Point p521_dbl(const P521Point& p) {
    const F521 b = p521_b();
    const F521 t0 = sqr(p.x), t1 = sqr(p.y), t2 = sqr(p.z);                  // n
    const F521 xy = mul(p.x, p.y), xz = mul(p.x, p.z), yz = mul(p.y, p.z);   // 1 n x 1 n: n
    const F521 xz2 = dbl(xz);                                                // 2 n
    F521 y3 = carry(sub(mul(b, t2), xz2));                                   // b Z^2 - 2 X Z: limbs in (-2 n, n), carried: n
    y3 = carry(add(y3, dbl(y3)));                                            // 3 (...): n
    const F521 xa = sub(t1, y3), ya = add(t1, y3);                           // Y^2 -+ y3: 1 n, 2 n
    const F521 t2b = add(t2, dbl(t2));                                       // 3 Z^2: 3 n
    F521 z3 = carry(sub(sub(mul(b, xz2), t2b), t0));                         // 2 b X Z - 3 Z^2 - X^2 (n x 2 n): limbs in (-4 n, n), carried: n
    z3 = add(z3, dbl(z3));                                                   // 3 (...): 3 n
    const F521 t0b = carry(sub(add(t0, dbl(t0)), t2b));                      // 3 X^2 - 3 Z^2: n
    const F521 yz2 = dbl(yz);                                                // 2 n
    P521Point r;
    r.x = sub(mul(dbl(xy), xa), mul(yz2, z3));                               // 2 X Y xa - 2 Y Z z3 (2 n x 1 n, 2 n x 3 n): 1 n
    r.y = carry(add(mul(xa, ya), mul(t0b, z3)));                             // xa ya + t0b z3 (1 n x 2 n, n x 3 n): n
    r.z = carry(dbl(mul(yz2, dbl(t1))));                                     // 2 (2 Y Z x 2 Y^2) = 8 Y^3 Z (2 n x 2 n): n
    return r;
}

// algorithm 4, a = -3: 14 products (two by b)
DR_L28_FN P521Point p521_add(const P521Point& p, const P521Point& q) {
    const F521 b = p521_b();
    const F521 t0 = mul(p.x, q.x), t1 = mul(p.y, q.y), t2 = mul(p.z, q.z);   // n
    const F521 t3 = sub(mul(add(p.x, p.y), add(q.x, q.y)), add(t0, t1));     // X1 Y2 + X2 Y1 (2 n x 2 n): limbs in (-2 n, n): 2 n
    const F521 t4 = sub(mul(add(p.y, p.z), add(q.y, q.z)), add(t1, t2));     // Y1 Z2 + Y2 Z1: 2 n
    const F521 u = sub(mul(add(p.x, p.z), add(q.x, q.z)), add(t0, t2));      // X1 Z2 + X2 Z1: 2 n
    const F521 x3a = carry(sub(u, mul(b, t2)));                              // u - b t2: n
    const F521 x3b = carry(add(x3a, dbl(x3a)));                              // 3 (...): n
    const F521 z3 = sub(t1, x3b), x3 = add(t1, x3b);                         // 1 n, 2 n
    const F521 t2b = add(t2, dbl(t2));                                       // 3 t2: 3 n
    F521 y3 = carry(sub(sub(mul(b, u), t2b), t0));                           // b u - 3 t2 - t0 (n x 2 n): limbs in (-4 n, n), carried: n
    y3 = add(y3, dbl(y3));                                                   // 3 (...): 3 n
    const F521 t0b = carry(sub(add(t0, dbl(t0)), t2b));                      // 3 t0 - 3 t2: n
    P521Point r;
    r.x = sub(mul(x3, t3), mul(t4, y3));                                     // 2 n x 2 n, 2 n x 3 n: 1 n
    r.y = carry(add(mul(x3, z3), mul(t0b, y3)));                             // 2 n x 1 n, n x 3 n: n
    r.z = carry(add(mul(t4, z3), mul(t3, t0b)));                             // 2 n x 1 n, 2 n x n: n
    return r;
}

// The law as the host side of dr_wide_msm takes it (wide_combine.hpp): the operations of the window combination and the ABI's x || y
// words <-> a point; zero words are the identity, which has Z = 0 and so stores them by 0^-1 = 0
struct P521Law : Limb28Law<P521Law, P521Point> {
    static constexpr bool ZERO_IS_IDENTITY = true;
    DR_L28_MEMBER static P521Point identity() { return p521_identity(); }
    DR_L28_MEMBER static P521Point from_affine(const F521& x, const F521& y) { return p521_from_affine(x, y); }
    DR_L28_MEMBER static P521Point add(const P521Point& p, const P521Point& q) { return p521_add(p, q); }
    DR_L28_MEMBER static P521Point dbl(const P521Point& p) { return p521_dbl(p); }
};

// sswu.hip.h's description of P-521: the simplified SWU map straight onto the curve (A = -3, B = b, Z = -4, no isogeny).  The field is
// in standard form, so A, Z and sqrt(-Z) = 2 are one-limb elements, -Z x is a small multiple and only B x is a full product.  Every
// value sswu_map makes is normal where it is made (norm = carry), so each of its products is n x n or n x 2 n.
struct P521Sswu {
    using Fe = F521;
    using Point = P521Point;
    static constexpr bool ISOGENY = false;
    DR_L28_MEMBER static F521 a() { return F521::small(-3); }
    DR_L28_MEMBER static F521 z() { return F521::small(-4); }
    DR_L28_MEMBER static F521 sqrt_neg_z() { return F521::small(2); }
    DR_L28_MEMBER static F521 one() { return F521::small(1); }
    DR_L28_MEMBER static F521 mul_neg_z(const F521& x) { return mul_small(x, 4); }              // n
    DR_L28_MEMBER static F521 mul_b(const F521& x) { return mul(p521_b(), x); }                  // n x (n or 2 n): n
    DR_L28_MEMBER static F521 norm(const F521& x) { return carry(x); }
    DR_L28_MEMBER static bool is_zero(const F521& x) { return dr::is_zero(x); }
    DR_L28_MEMBER static bool equal(const F521& x, const F521& y) { return dr::equal(x, y); }
    DR_L28_MEMBER static bool is_odd(const F521& x) { return dr::is_odd(x); }
    DR_L28_MEMBER static F521 pow_p34(const F521& x) { return f521_pow_p34(x); }
};

// ---------------------------------------------------------------- the windows of the fixed schedule
// Signed 4-bit digits (wave_recode.hip.h) of a scalar k < 2^521 given as 17 words: k = sum d_w 16^w, d_w in [-8, 7], w = 0..130.  131
// nibbles cover 524 bits; nibble 130 holds bit 520 alone, so with the carry into it d_130 <= 2 and nothing leaves it: 131 windows, and
// no window for a carry out as the 448-bit schedules need.  The nibbles from 131 up come out as 8 (zero).
constexpr int P521_WINDOWS = 131;

}  // namespace dr
