// The group law of P-384 (DR_CURVE_P384_RO / DR_CURVE_P384_NU; the reference's specs/p384.py): y^2 = x^3 - 3 x + b over
// p = 2^384 - 2^128 - 2^96 + 2^32 - 1 (fp384.hip.h, Montgomery form), prime order, cofactor 1.  Homogeneous projective (X : Y : Z),
// x = X / Z, y = Y / Z, identity (0 : 1 : 0).  The law is the complete one of Renes, Costello and Batina (2016), algorithms 4 (addition)
// and 6 (doubling) for a = -3, restated over this field: no exceptional cases (P + P, P + (-P), the identity on either side) and no
// branches.  b is a full-width constant in Montgomery form.  Where the last step of a coordinate is a sum of two products it is ONE
// reduction (fp384.hip.h's mul2), which p521_law.hip.h's field has no room for.
//
// The comments give the limb class of every intermediate against fp384.hip.h's contract ("n" = normal, "k n" = |limb| <= k normal and
// |value| < k 2^385; mul needs ka kb <= 8, mul2 ka kb + kc kd <= 8, sqr 2 n; carry returns n for up to 32 n).  A point's coordinates are
// x: 1 n, y: n (1 n once negated), z: n, in and out.
//
// The map's description for sswu.hip.h is here as well, so that the host can check it, and the window count of the fixed schedule.
// Plain integer C++ like fp384.hip.h: compiles for the device and, with g++, for the host (tests/native/p384_host_check.cpp, where
// -fsanitize=undefined turns a signed 64-bit column overflow into an abort).
#pragma once
#include "fp384.hip.h"

namespace dr {

struct P384Point {
    F384 x, y, z;
};

DR_L28_FN F384 p384_b() { return F384::constant<Fp384Consts::B>(); }
DR_L28_FN P384Point p384_identity() { return {F384::zero(), F384::small(1), F384::zero()}; }
DR_L28_FN P384Point p384_from_affine(const F384& x, const F384& y) { return {x, y, F384::small(1)}; }
DR_L28_FN bool p384_is_identity(const P384Point& p) { return is_zero(p.z); }
DR_L28_FN P384Point p384_cneg(const P384Point& p, bool negate) { return {p.x, cneg(p.y, negate), p.z}; }

// algorithm 6, a = -3: 10 products (two by b), two of them fused into one pair, and 3 squarings; 12 reductions
DR_L28_FN P384Point p384_dbl(const P384Point& p) {
    const F384 b = p384_b();
    const F384 t0 = sqr(p.x), t1 = sqr(p.y), t2 = sqr(p.z);                  // n
    const F384 xy = mul(p.x, p.y), xz = mul(p.x, p.z), yz = mul(p.y, p.z);   // 1 n x 1 n: n
    const F384 xz2 = dbl(xz);                                                // 2 n
    F384 y3 = carry(sub(mul(b, t2), xz2));                                   // b Z^2 - 2 X Z: limbs in (-2 n, n), 3 n by value, carried: n
    y3 = carry(add(y3, dbl(y3)));                                            // 3 (...): n
    const F384 xa = sub(t1, y3), ya = add(t1, y3);                           // Y^2 -+ y3: 1 n, 2 n
    const F384 t2b = add(t2, dbl(t2));                                       // 3 Z^2: 3 n
    F384 z3 = carry(sub(sub(mul(b, xz2), t2b), t0));                         // 2 b X Z - 3 Z^2 - X^2 (n x 2 n): limbs in (-4 n, n), carried: n
    z3 = add(z3, dbl(z3));                                                   // 3 (...): 3 n
    const F384 t0b = carry(sub(add(t0, dbl(t0)), t2b));                      // 3 X^2 - 3 Z^2: 6 n by value, carried: n
    const F384 yz2 = dbl(yz);                                                // 2 n
    P384Point r;
    r.x = sub(mul(dbl(xy), xa), mul(yz2, z3));                               // 2 X Y xa - 2 Y Z z3 (2 n x 1 n, 2 n x 3 n): 1 n
    r.y = mul2(xa, ya, t0b, z3);                                             // xa ya + t0b z3 (1 n x 2 n + n x 3 n = 5): n
    r.z = mul(yz2, dbl(dbl(t1)));                                            // 2 Y Z x 4 Y^2 = 8 Y^3 Z (2 n x 4 n): n
    return r;
}

// algorithm 4, a = -3: 14 products (two by b), four of them fused into two pairs; 12 reductions
DR_L28_FN P384Point p384_add(const P384Point& p, const P384Point& q) {
    const F384 b = p384_b();
    const F384 t0 = mul(p.x, q.x), t1 = mul(p.y, q.y), t2 = mul(p.z, q.z);   // n
    const F384 t3 = sub(mul(add(p.x, p.y), add(q.x, q.y)), add(t0, t1));     // X1 Y2 + X2 Y1 (2 n x 2 n): limbs in (-2 n, n): 2 n
    const F384 t4 = sub(mul(add(p.y, p.z), add(q.y, q.z)), add(t1, t2));     // Y1 Z2 + Y2 Z1: 2 n
    const F384 u = sub(mul(add(p.x, p.z), add(q.x, q.z)), add(t0, t2));      // X1 Z2 + X2 Z1: 2 n
    const F384 x3a = carry(sub(u, mul(b, t2)));                              // u - b t2: 3 n, carried: n
    const F384 x3b = carry(add(x3a, dbl(x3a)));                              // 3 (...): n
    const F384 z3 = sub(t1, x3b), x3 = add(t1, x3b);                         // 1 n, 2 n
    const F384 t2b = add(t2, dbl(t2));                                       // 3 t2: 3 n
    F384 y3 = carry(sub(sub(mul(b, u), t2b), t0));                           // b u - 3 t2 - t0 (n x 2 n): limbs in (-4 n, n), carried: n
    y3 = add(y3, dbl(y3));                                                   // 3 (...): 3 n
    const F384 t0b = carry(sub(add(t0, dbl(t0)), t2b));                      // 3 t0 - 3 t2: n
    P384Point r;
    r.x = sub(mul(x3, t3), mul(t4, y3));                                     // 2 n x 2 n, 2 n x 3 n: 1 n
    r.y = mul2(x3, z3, t0b, y3);                                             // 2 n x 1 n + n x 3 n = 5: n
    r.z = mul2(t4, z3, t3, t0b);                                             // 2 n x 1 n + 2 n x n = 4: n
    return r;
}

// The law as the host side of dr_wide_msm takes it (wide_combine.hpp): the operations of the window combination and the ABI's x || y
// words <-> a point; zero words are the identity, which has Z = 0 and so stores them by 0^-1 = 0.
struct P384Law : Limb28Law<P384Law, P384Point> {
    static constexpr bool ZERO_IS_IDENTITY = true;
    DR_L28_MEMBER static P384Point identity() { return p384_identity(); }
    DR_L28_MEMBER static P384Point from_affine(const F384& x, const F384& y) { return p384_from_affine(x, y); }
    DR_L28_MEMBER static P384Point add(const P384Point& p, const P384Point& q) { return p384_add(p, q); }
    DR_L28_MEMBER static P384Point dbl(const P384Point& p) { return p384_dbl(p); }
};

// sswu.hip.h's description of P-384: the simplified SWU map straight onto the curve (A = -3, B = b, Z = -12, no isogeny).  A and Z are
// the small elements -3 R and -12 R (five signed limbs each, 1 n), -Z x is the small multiple 12 x, and only B x and the product with
// sqrt(-Z) = sqrt(12) meet a full-width constant.  Every value sswu_map makes is normal where it is made (norm = carry), so each of its
// products is n x n or n x 2 n.
struct P384Sswu {
    using Fe = F384;
    using Point = P384Point;
    static constexpr bool ISOGENY = false;
    DR_L28_MEMBER static F384 a() { return F384::small(-3); }
    DR_L28_MEMBER static F384 z() { return F384::small(-12); }
    DR_L28_MEMBER static F384 sqrt_neg_z() { return F384::constant<Fp384Consts::SQRT12>(); }
    DR_L28_MEMBER static F384 one() { return F384::small(1); }
    DR_L28_MEMBER static F384 mul_neg_z(const F384& x) { return mul_small(x, 12); }             // n
    DR_L28_MEMBER static F384 mul_b(const F384& x) { return mul(p384_b(), x); }                  // n x (n or 2 n): n
    DR_L28_MEMBER static F384 norm(const F384& x) { return carry(x); }
    DR_L28_MEMBER static bool is_zero(const F384& x) { return dr::is_zero(x); }
    DR_L28_MEMBER static bool equal(const F384& x, const F384& y) { return dr::equal(x, y); }
    DR_L28_MEMBER static bool is_odd(const F384& x) { return dr::is_odd(x); }
    DR_L28_MEMBER static F384 pow_p34(const F384& x) { return f384_pow_p34(x); }
};

// ---------------------------------------------------------------- the windows of the fixed schedule
// Signed 4-bit digits (wave_recode.hip.h) of a scalar of 12 words: 96 digits and the carry out of the top one as window 96, so every
// 384-bit value has its windows and the host refuses no scalar.
constexpr int P384_WINDOWS = 97;

}  // namespace dr
