// The group law of a short Weierstrass curve y^2 = x^3 - 3 x + b of prime order over a signed 28-bit field (limb28.hip.h), once for
// P-384 (p384_law.hip.h over fp384.hip.h) and P-521 (p521_law.hip.h over fp521.hip.h).  Homogeneous projective (X : Y : Z), x = X / Z,
// y = Y / Z, identity (0 : 1 : 0).  The law is the complete one of Renes, Costello and Batina (2016), algorithms 4 (addition) and 6
// (doubling) for a = -3: no exceptional cases (P + P, P + (-P), the identity on either side) and no branches.  A curve gives a
// description D:
//   Fe       its field element, a Limb28<F>
//   b()      the curve's b as an element, in the field's own form (full width)
//   FUSED    the field has room for mul2 at ka kb + kc kd <= 8 and for a 2 n x 4 n product (fp384.hip.h).  Then the last step of a
//            coordinate that is a sum of two products is ONE reduction; otherwise (fp521.hip.h: mul needs ka kb <= 6, no mul2) it is
//            two products, their sum carried.  The choice stands in the law's body, at the four places it is made: behind a helper
//            the compiler orders the law's kernels differently.
// and gets the point type, the law (sw3_dbl, sw3_add), the law as the host and the device take it (Sw3Law<D>: wide_combine.hpp's
// window combination; Sw3Curve<D>: the law members of the curve's description for wave_curve.hip.h) and the part of sswu.hip.h's
// description of the map that the field does not decide (Sw3Sswu<D>).
//
// The comments give the limb class of every intermediate against the contracts of both fields ("n" = normal, "k n" = |limb| <= k
// normal; mul needs ka kb <= 8 (P-384) or <= 6 (P-521), sqr 2 n; carry returns n), and say so where P-384's bound by value
// (|value| < k 2^385) is a reason for a carry as well.  A point's coordinates are x: 1 n, y: n (1 n once negated), z: n, in and out.
//
// Plain integer C++ like the fields: compiles for the device and, with g++, for the host (tests/native/sw3_host_check.hpp, where
// -fsanitize=undefined turns a signed 64-bit column overflow into an abort).
#pragma once
#include "limb28.hip.h"

namespace dr {

template <class Fe>
struct Sw3Point {
    Fe x, y, z;
};

// algorithm 6, a = -3: 10 products (two by b) and 3 squarings; FUSED: two of the products are one pair, 12 reductions
template <class D>
DR_L28_FN Sw3Point<typename D::Fe> sw3_dbl(const Sw3Point<typename D::Fe>& p) {
    using Fe = typename D::Fe;
    const Fe b = D::b();
    const Fe t0 = sqr(p.x), t1 = sqr(p.y), t2 = sqr(p.z);                    // n
    const Fe xy = mul(p.x, p.y), xz = mul(p.x, p.z), yz = mul(p.y, p.z);     // 1 n x 1 n: n
    const Fe xz2 = dbl(xz);                                                  // 2 n
    Fe y3 = carry(sub(mul(b, t2), xz2));                                     // b Z^2 - 2 X Z: limbs in (-2 n, n) (P-384: 3 n by value), carried: n
    y3 = carry(add(y3, dbl(y3)));                                            // 3 (...): n
    const Fe xa = sub(t1, y3), ya = add(t1, y3);                             // Y^2 -+ y3: 1 n, 2 n
    const Fe t2b = add(t2, dbl(t2));                                         // 3 Z^2: 3 n
    Fe z3 = carry(sub(sub(mul(b, xz2), t2b), t0));                           // 2 b X Z - 3 Z^2 - X^2 (n x 2 n): limbs in (-4 n, n), carried: n
    z3 = add(z3, dbl(z3));                                                   // 3 (...): 3 n
    const Fe t0b = carry(sub(add(t0, dbl(t0)), t2b));                        // 3 X^2 - 3 Z^2 (P-384: 6 n by value), carried: n
    const Fe yz2 = dbl(yz);                                                  // 2 n
    Sw3Point<Fe> r;
    r.x = sub(mul(dbl(xy), xa), mul(yz2, z3));                               // 2 X Y xa - 2 Y Z z3 (2 n x 1 n, 2 n x 3 n): 1 n
    if constexpr (D::FUSED) {
        r.y = mul2(xa, ya, t0b, z3);                                         // xa ya + t0b z3 (1 n x 2 n + n x 3 n = 5): n
        r.z = mul(yz2, dbl(dbl(t1)));                                        // 2 Y Z x 4 Y^2 = 8 Y^3 Z (2 n x 4 n): n
    } else {
        r.y = carry(add(mul(xa, ya), mul(t0b, z3)));                         // xa ya + t0b z3 (1 n x 2 n, n x 3 n): n
        r.z = carry(dbl(mul(yz2, dbl(t1))));                                 // 2 (2 Y Z x 2 Y^2) = 8 Y^3 Z (2 n x 2 n): n
    }
    return r;
}

// algorithm 4, a = -3: 14 products (two by b); FUSED: four of them are two pairs, 12 reductions
template <class D>
DR_L28_FN Sw3Point<typename D::Fe> sw3_add(const Sw3Point<typename D::Fe>& p, const Sw3Point<typename D::Fe>& q) {
    using Fe = typename D::Fe;
    const Fe b = D::b();
    const Fe t0 = mul(p.x, q.x), t1 = mul(p.y, q.y), t2 = mul(p.z, q.z);     // n
    const Fe t3 = sub(mul(add(p.x, p.y), add(q.x, q.y)), add(t0, t1));       // X1 Y2 + X2 Y1 (2 n x 2 n): limbs in (-2 n, n): 2 n
    const Fe t4 = sub(mul(add(p.y, p.z), add(q.y, q.z)), add(t1, t2));       // Y1 Z2 + Y2 Z1: 2 n
    const Fe u = sub(mul(add(p.x, p.z), add(q.x, q.z)), add(t0, t2));        // X1 Z2 + X2 Z1: 2 n
    const Fe x3a = carry(sub(u, mul(b, t2)));                                // u - b t2 (P-384: 3 n by value), carried: n
    const Fe x3b = carry(add(x3a, dbl(x3a)));                                // 3 (...): n
    const Fe z3 = sub(t1, x3b), x3 = add(t1, x3b);                           // 1 n, 2 n
    const Fe t2b = add(t2, dbl(t2));                                         // 3 t2: 3 n
    Fe y3 = carry(sub(sub(mul(b, u), t2b), t0));                             // b u - 3 t2 - t0 (n x 2 n): limbs in (-4 n, n), carried: n
    y3 = add(y3, dbl(y3));                                                   // 3 (...): 3 n
    const Fe t0b = carry(sub(add(t0, dbl(t0)), t2b));                        // 3 t0 - 3 t2: n
    Sw3Point<Fe> r;
    r.x = sub(mul(x3, t3), mul(t4, y3));                                     // 2 n x 2 n, 2 n x 3 n: 1 n
    if constexpr (D::FUSED) {
        r.y = mul2(x3, z3, t0b, y3);                                         // 2 n x 1 n + n x 3 n = 5: n
        r.z = mul2(t4, z3, t3, t0b);                                         // 2 n x 1 n + 2 n x n = 4: n
    } else {
        r.y = carry(add(mul(x3, z3), mul(t0b, y3)));                         // 2 n x 1 n, n x 3 n: n
        r.z = carry(add(mul(t4, z3), mul(t3, t0b)));                         // 2 n x 1 n, 2 n x n: n
    }
    return r;
}

// The law as the host side of dr_wide_msm takes it (wide_combine.hpp; Limb28Law: the ABI's x || y words <-> a point; zero words are
// the identity, which has Z = 0 and so stores them by 0^-1 = 0), and the four small operations, which exist here alone
template <class D>
struct Sw3Law : Limb28Law<Sw3Law<D>, Sw3Point<typename D::Fe>> {
    using Fe = typename D::Fe;
    using Point = Sw3Point<Fe>;
    static constexpr bool ZERO_IS_IDENTITY = true;
    DR_L28_MEMBER static Point identity() { return {Fe::zero(), Fe::small(1), Fe::zero()}; }
    DR_L28_MEMBER static Point from_affine(const Fe& x, const Fe& y) { return {x, y, Fe::small(1)}; }
    DR_L28_MEMBER static bool is_identity(const Point& p) { return is_zero(p.z); }
    DR_L28_MEMBER static Point cneg(const Point& p, bool negate) { return {p.x, dr::cneg(p.y, negate), p.z}; }
    DR_L28_MEMBER static Point add(const Point& p, const Point& q) { return sw3_add<D>(p, q); }
    DR_L28_MEMBER static Point dbl(const Point& p) { return sw3_dbl<D>(p); }
};

// The law members of wave_curve.hip.h's description of the curve.  The description derives from this and adds its block, its windows
// and its scalar form; inv stays a one-line forwarder in each.
template <class D>
struct Sw3Curve : Limb28Curve<typename D::Fe::Field> {
    using Fe = typename D::Fe;
    using Point = Sw3Point<Fe>;
    static constexpr bool EXTENDED = false, ZERO_IS_IDENTITY = true;
    DR_L28_MEMBER static Point identity() { return Sw3Law<D>::identity(); }
    DR_L28_MEMBER static Point from_affine(const Fe& x, const Fe& y) { return Sw3Law<D>::from_affine(x, y); }
    DR_L28_MEMBER static Point add(const Point& p, const Point& q) { return sw3_add<D>(p, q); }
    DR_L28_MEMBER static Point dbl(const Point& p) { return sw3_dbl<D>(p); }
    DR_L28_MEMBER static Point cneg(const Point& p, bool negate) { return Sw3Law<D>::cneg(p, negate); }
};

// What sswu.hip.h's description of the simplified SWU map straight onto such a curve (A = -3, B = b, no isogeny) does not owe to the
// field.  The curve's description derives from this and adds z, sqrt_neg_z, mul_neg_z and pow_p34.  Every value sswu_map makes is
// normal where it is made (norm = carry), so each of its products is n x n or n x 2 n.
template <class D>
struct Sw3Sswu {
    using Fe = typename D::Fe;
    using Point = Sw3Point<Fe>;
    static constexpr bool ISOGENY = false;
    DR_L28_MEMBER static Fe a() { return Fe::small(-3); }
    DR_L28_MEMBER static Fe one() { return Fe::small(1); }
    DR_L28_MEMBER static Fe mul_b(const Fe& x) { return mul(D::b(), x); }                       // n x (n or 2 n): n
    DR_L28_MEMBER static Fe norm(const Fe& x) { return carry(x); }
    DR_L28_MEMBER static bool is_zero(const Fe& x) { return dr::is_zero(x); }
    DR_L28_MEMBER static bool equal(const Fe& x, const Fe& y) { return dr::equal(x, y); }
    DR_L28_MEMBER static bool is_odd(const Fe& x) { return dr::is_odd(x); }
};

}  // namespace dr
