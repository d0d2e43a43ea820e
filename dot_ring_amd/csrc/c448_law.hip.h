// The group law of curve448 (DR_CURVE_CURVE448_RO / _NU; the reference's specs/curve448.py over montgomery/mg_affine_point.py):
// Montgomery affine points (u, v) of v^2 = u^3 + A u^2 + u, A = 156326, over p = 2^448 - 2^224 - 1 (fe448.hip.h), cofactor 4.  The
// reference adds them by the affine chord-and-tangent law, which has no complete projective form, and Ed448's kernels cannot serve: the
// map from curve448 to edwards448 is a 4-isogeny, not a birational map.  The law here runs on the Edwards curve that IS birational to
// curve448,
//     E_M : a x^2 + y^2 = 1 + d x^2 y^2,   a = A - 2 = 156324,  d = A + 2 = 156328,
//     x = u / v,  y = (u + 1) / (u - 1);    u = (y + 1) / (y - 1),  v = u / x.
// a is a square and d a non-square in F_p (tests/test_curve448_cpu.py), so the unified addition add-2008-bbjlp is complete on all of
// E_M(F_p); both constants go through mul_small.  (The textbook pair (a, d) = (A + 2, A - 2) is this one under y -> 1 / y and would not
// be complete.)  PROJECTIVE (X : Y : Z), identity (0 : 1 : 1), negation (-x, y).
//
// Exceptional points of the map, all carried explicitly:
//   the identity    has no affine Montgomery coordinates: a flag beside the point, (0 : 1 : 1) inside
//   (0, 0)          the point of order 2 and the only one with v = 0 (A^2 - 4 is a non-square): picked out on loading as (0 : -1 : 1),
//                   produced on storing by inv(0) = 0 (X = 0 makes u = v = 0)
//   u = 1           is not on the curve (A + 2 is a non-square), so Z = v (u - 1) = 0 only at (0, 0)
//   u = -1          IS on the curve, (-1, +-sqrt(A - 2)), the points of order 4; they map to y = 0, x = -+1 / sqrt(A - 2) and need
//                   nothing special (on Curve25519, u = -1 is unreachable)
// The comments give the limb class of every intermediate against fe448.hip.h's contract ("n" = normal, "k n" = |limb| <= k normal; mul
// needs ka kb <= 3, sqr 1 n).  Plain integer C++ like fe448.hip.h: compiles for the device and, with g++, for the host
// (tests/native/c448_law_host_check.cpp, where -fsanitize=undefined turns a signed 64-bit column overflow into an abort).
#pragma once
#include "fe448.hip.h"

namespace dr {

struct M448Consts {
    static constexpr int32_t A = Fe448Consts::MONT_A;
    static constexpr int32_t EDWARDS_A = A - 2, EDWARDS_D = A + 2;
};

struct M448Point {
    F448 x, y, z;
};

DR_L28_FN M448Point m448_identity() { return {F448::zero(), F448::small(1), F448::small(1)}; }
DR_L28_FN bool m448_is_identity(const M448Point& p) { return is_zero(p.x) && equal(p.y, p.z); }
DR_L28_FN M448Point m448_cneg(const M448Point& p, bool negate) { return {cneg(p.x, negate), p.y, p.z}; }

// dbl-2008-bbjlp: coordinates n (x possibly negated: 1 n) in, n out
DR_L28_FN M448Point m448_dbl(const M448Point& p) {
    const F448 B = sqr(carry(add(p.x, p.y)));                // (X + Y)^2: the sum carried to n
    const F448 C = sqr(p.x), D = sqr(p.y);                   // n
    const F448 E = mul_small(C, M448Consts::EDWARDS_A);      // a C: n
    const F448 F = carry(add(E, D));                         // n
    const F448 H = sqr(p.z);                                 // n
    const F448 J = sub(F, dbl(H));                           // F - 2 H: limbs in (-2 n, n): 2 n
    M448Point r;
    r.x = mul(carry(sub(B, add(C, D))), J);                  // (B - C - D) J: n x 2 n
    r.y = mul(F, sub(E, D));                                 // n x 1 n
    r.z = mul(F, J);                                         // n x 2 n
    return r;
}

// add-2008-bbjlp: unified and, d being a non-square and a a square, complete.  Coordinates n (x possibly negated: 1 n) in, n out
DR_L28_FN M448Point m448_add(const M448Point& p, const M448Point& q) {
    const F448 A = mul(p.z, q.z);                                            // n
    const F448 B = sqr(A);                                                   // n
    const F448 C = mul(p.x, q.x), D = mul(p.y, q.y);                         // 1 n x 1 n, n x n: n
    const F448 E = mul_small(mul(C, D), M448Consts::EDWARDS_D);              // d C D: n
    const F448 F = sub(B, E), G = add(B, E);                                 // B - d C D: 1 n; B + d C D: 2 n  (d > 0: e448_add's, swapped)
    // (X1 + Y1) (X2 + Y2) - C - D: the sums carried to n; limbs in (-2 n, n): 2 n
    const F448 t = sub(mul(carry(add(p.x, p.y)), carry(add(q.x, q.y))), add(C, D));
    M448Point r;
    r.x = mul(mul(A, F), t);                                                 // (n x 1 n) x 2 n
    r.y = mul(mul(A, G), sub(D, mul_small(C, M448Consts::EDWARDS_A)));       // (n x 2 n) x (n - n = 1 n)
    r.z = mul(F, G);                                                         // 1 n x 2 n
    return r;
}

// the point of E_M for Montgomery (u, v), both n; `ident`: the identity flag of the input (u, v ignored).  No inversion:
// (X : Y : Z) = (u (u - 1) : (u + 1) v : v (u - 1)); v = 0 is (0, 0) alone, (0 : -1 : 1)
DR_L28_FN M448Point m448_load(const F448& u, const F448& v, bool ident) {
    const F448 one = F448::small(1);
    const F448 um = carry(sub(u, one)), up = carry(add(u, one));             // n
    M448Point r;
    r.x = mul(u, um); r.y = mul(up, v); r.z = mul(v, um);
    const bool two = is_zero(v);
    const bool fixed = two || ident;
    r.x = select(fixed, F448::zero(), r.x);
    r.y = select(fixed, cneg(one, two && !ident), r.y);
    r.z = select(fixed, one, r.z);
    return r;
}
// ... for u = N / D with D != 0 (the Elligator 2 map's fraction; N 1 n, D n, v 1 n): the same three products times D^2,
// (N (N - D) : (N + D) v D : v (N - D) D)
DR_L28_FN M448Point m448_load_fraction(const F448& N, const F448& D, const F448& v) {
    const F448 one = F448::small(1);
    const F448 nm = carry(sub(N, D)), np = carry(add(N, D));                 // n
    M448Point r;
    r.x = mul(N, nm);                                                        // 1 n x n
    r.y = mul(mul(np, v), D);                                                // (n x 1 n) x n
    r.z = mul(mul(v, nm), D);
    const bool two = is_zero(v);
    r.x = select(two, F448::zero(), r.x);
    r.y = select(two, neg(one), r.y);
    r.z = select(two, one, r.z);
    return r;
}
// Montgomery (u, v) of a point, one inversion: i = 1 / (X (Y - Z)), u = (Y + Z) X i, v = (Y + Z) Z i.  The identity (X = 0 and
// Y = Z) returns true and u = v = 0; (0 : -1 : 1) gives (0, 0) through inv(0) = 0, as it must.  u, v: n
DR_L28_FN bool m448_store(const M448Point& p, F448& u, F448& v) {
    const F448 ymz = carry(sub(p.y, p.z)), ypz = carry(add(p.y, p.z));       // n
    const F448 i = inv(mul(p.x, ymz));                                       // 1 n
    const F448 t = mul(ypz, i);                                              // n
    u = mul(t, p.x);
    v = mul(t, p.z);
    return is_zero(p.x) && is_zero(ymz);
}

// The law as the host side of dr_wide_msm takes it (wide_combine.hpp): the operations of the window combination and the ABI's u || v
// words <-> a point; the identity is words of 0xffffffff, in and out (the Curve448 entry points' spelling)
struct M448Law : Limb28Law<M448Law, M448Point> {
    DR_L28_MEMBER static M448Point identity() { return m448_identity(); }
    DR_L28_MEMBER static M448Point add(const M448Point& p, const M448Point& q) { return m448_add(p, q); }
    DR_L28_MEMBER static M448Point dbl(const M448Point& p) { return m448_dbl(p); }
    DR_L28_MEMBER static M448Point from_abi(const uint32_t (&w)[2 * W448]) {
        uint32_t u[W448], v[W448], o = 0xffffffffu;
        for (int j = 0; j < W448; j++) { u[j] = w[j]; v[j] = w[W448 + j]; o &= u[j] & v[j]; }
        if (o == 0xffffffffu) return m448_identity();
        return m448_load(unpack(u), unpack(v), false);
    }
    DR_L28_MEMBER static void to_abi(const M448Point& p, uint32_t (&w)[2 * W448]) {
        F448 u, v;
        const bool ident = m448_store(p, u, v);
        uint32_t uw[W448], vw[W448];
        pack(u, uw);
        pack(v, vw);
        for (int j = 0; j < W448; j++) { w[j] = ident ? 0xffffffffu : uw[j]; w[W448 + j] = ident ? 0xffffffffu : vw[j]; }
    }
};

// v^2 = u^3 + A u^2 + u for u, v n (the decoder's test)
DR_L28_FN bool m448_on_curve(const F448& u, const F448& v) {
    const F448 ua = carry(add(u, F448::small(M448Consts::A)));               // n
    const F448 q = carry(add(mul(u, ua), F448::small(1)));                   // u (u + A) + 1: n
    return equal(sqr(v), mul(u, q));
}

// Elligator 2 onto curve448 (RFC 9380 6.7.2 with Z = -1, as the reference's MGAffinePoint.map_to_curve computes it) in the
// inversion-free shape of appendix G.2.2 (p = 3 mod 4): the first half of kernels_ed448.hip.h's e448_ell2_map, whose comment derives
// it.  The image is (N / D, v), D = 1 - u^2.  has_value = false exactly where u^2 = 1: the reference's comparison of a reduced value
// with -1 never holds there, so it inverts 0 and raises.  u = 0 has the value (0, 0) (N = v = 0: gx1 = -A is a non-square).
DR_L28_FN void m448_ell2(const F448& u /* n, canonical */, F448& N, F448& D, F448& v, bool& has_value) {
    constexpr int32_t A = M448Consts::A;
    const F448 one = F448::small(1);
    F448 u2 = sqr(u);                                                        // -tv1: n
    const bool e1 = equal(u2, one);
    u2 = select(e1, F448::zero(), u2);                                       // (any value: the item is refused)
    const F448 xd = carry(add(one, neg(u2)));                                // 1 - u^2: n
    const F448 xd2 = sqr(xd);
    const F448 gxd = mul(xd2, xd);                                           // xd^3: n
    const F448 au2 = mul_small(u2, A);                                       // A u^2 (= x2n): n
    const F448 g = neg(mul_small(carry(add(mul_small(au2, A), xd2)), A));    // -A (A^2 u^2 + xd^2): 1 n
    const F448 t2 = mul(g, gxd);                                             // n
    const F448 t3 = mul(sqr(gxd), t2);                                       // g gxd^3: n
    const F448 y1 = mul(f448_pow_p34(t3), t2);                               // n
    const F448 y2 = mul(y1, u);                                              // n
    const bool e2 = equal(mul(sqr(y1), gxd), g);
    N = select(e2, F448::small(-A), au2);                                    // x1n = -A or x2n: 1 n
    D = xd;
    v = select(e2, y1, y2);
    v = cneg(v, e2 != is_odd(v));                                            // 1 n
    has_value = !e1;
}

}  // namespace dr
