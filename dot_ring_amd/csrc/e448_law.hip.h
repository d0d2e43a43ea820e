// The group law of Ed448 (DR_CURVE_ED448_RO / DR_CURVE_ED448_NU; the reference's specs/ed448.py): x^2 + y^2 = 1 + d x^2 y^2 with a = 1
// and d = -39081 over p = 2^448 - 2^224 - 1 (fe448.hip.h), cofactor 4.  d is a non-square, so the unified addition is complete on all of
// E(F_p).  PROJECTIVE (X : Y : Z), identity (0 : 1 : 1), add-2007-bl and dbl-2007-bl with c = 1 (kernels_ed448.hip.h says why not
// extended coordinates).  The comments give the limb class of every intermediate against fe448.hip.h's contract ("n" = normal, "k n" =
// |limb| <= k normal; mul needs ka kb <= 3, sqr 1 n).  Plain integer C++ like fe448.hip.h and c448_law.hip.h beside it: compiles for the
// device and, with g++, for the host (the window combination of dr_wide_msm; tests/native/wide_msm_plan_check.cpp).
#pragma once
#include "fe448.hip.h"

namespace dr {

struct E448Point {
    F448 x, y, z;
};

DR_L28_FN E448Point e448_identity() { return {F448::zero(), F448::small(1), F448::small(1)}; }
DR_L28_FN E448Point e448_from_affine(const F448& x, const F448& y) { return {x, y, F448::small(1)}; }
DR_L28_FN bool e448_is_identity(const E448Point& p) { return is_zero(p.x) && equal(p.y, p.z); }

// dbl-2007-bl, c = 1: coordinates n in, n out
DR_L28_FN E448Point e448_dbl(const E448Point& p) {
    const F448 B = sqr(carry(add(p.x, p.y)));                // (X + Y)^2: the sum carried to n
    const F448 C = sqr(p.x), D = sqr(p.y);                   // n
    const F448 E = carry(add(C, D));                         // n
    const F448 H = sqr(p.z);                                 // n
    const F448 J = sub(E, dbl(H));                           // E - 2 H: limbs in (-2 n, n): 2 n
    E448Point r;
    r.x = mul(carry(sub(B, add(C, D))), J);                  // (B - C - D) J: n x 2 n
    r.y = mul(E, sub(C, D));                                 // n x 1 n
    r.z = mul(E, J);                                         // n x 2 n
    return r;
}

// add-2007-bl, c = 1, a = 1: unified and, d being a non-square, complete.  Coordinates n (x possibly negated: 1 n) in, n out
DR_L28_FN E448Point e448_add(const E448Point& p, const E448Point& q) {
    const F448 A = mul(p.z, q.z);                                            // n
    const F448 B = sqr(A);                                                   // n
    const F448 C = mul(p.x, q.x), D = mul(p.y, q.y);                         // n
    const F448 E = mul_small(mul(C, D), Fe448Consts::EDWARDS_D_NEG);         // -d C D = 39081 C D: n
    const F448 F = add(B, E), G = sub(B, E);                                 // B - d C D: 2 n; B + d C D: 1 n
    // (X1 + Y1) (X2 + Y2) - C - D: the sums carried to n; limbs in (-2 n, n): 2 n
    const F448 t = sub(mul(carry(add(p.x, p.y)), carry(add(q.x, q.y))), add(C, D));
    E448Point r;
    r.x = mul(mul(A, F), t);                                                 // (n x 2 n) x 2 n
    r.y = mul(mul(A, G), sub(D, C));                                         // (n x 1 n) x 1 n
    r.z = mul(F, G);                                                         // 2 n x 1 n
    return r;
}
DR_L28_FN E448Point e448_cneg(const E448Point& p, bool negate) { return {cneg(p.x, negate), p.y, p.z}; }

// The law as the host side of dr_wide_msm takes it (wide_combine.hpp): the operations of the window combination and the ABI's x || y
// words <-> a point; the identity is (0, 1) as itself and Z is never 0
struct E448Law : Limb28Law<E448Law, E448Point> {
    static constexpr bool ZERO_IS_IDENTITY = false;
    DR_L28_MEMBER static E448Point identity() { return e448_identity(); }
    DR_L28_MEMBER static E448Point from_affine(const F448& x, const F448& y) { return e448_from_affine(x, y); }
    DR_L28_MEMBER static E448Point add(const E448Point& p, const E448Point& q) { return e448_add(p, q); }
    DR_L28_MEMBER static E448Point dbl(const E448Point& p) { return e448_dbl(p); }
};

}  // namespace dr
