// The simplified SWU map of RFC 9380 (hashing to a short Weierstrass curve) as one template over a description C of the target: its
// field and point types, the map's constants as compile-time limbs, and the handful of field operations whose names or forms differ
// between the fields.  kernels_secp256k1.hip.h (Secp256k1Sswu: a map onto an isogenous curve, then the 3-isogeny) and
// kernels_p256.hip.h (P256Sswu: the map straight onto the curve, ISOGENY = false) each give one description and one kernel; the
// arithmetic below exists once.  kernels_g1_h2c.hip.h (G1hSswu, BLS12-381 G1) takes sswu_map alone: its 11-isogeny, 48-byte coordinates and
// cofactor clearing have an evaluation and a kernel body of their own there.  C provides
//   Fe, Point                      the field element and the projective point
//   ISOGENY                        whether the image lies on an isogenous curve E' (then XN3..YD0, the isogeny's coefficient lists)
//   a(), z(), sqrt_neg_z(), one()  A of the SWU curve, Z, sqrt(-Z) and 1 as elements (in the field's own form)
//   mul_neg_z(x), mul_b(x)         -Z x and B x for x a normal or a sum of two, in a form mul / sqr accept on both sides (normal where the
//                                  field reduces small multiples; G1hSswu's -Z x is carried, |value| < 11.2 p, within its mul's 32 p)
//   norm(x)                        a sum, difference or negation of such values back to what mul / sqr accept on both sides
//   is_zero, equal, is_odd         on the canonical value (is_odd is sgn0)
//   pow_p34(x)                     x^((p - 3) / 4), p = 3 mod 4
//   BLOCK, identity(), add(P, Q), unpack(w), pack(a, w), inv(a)    as wave_curve.hip.h asks them of its description: a curve's SSWU
//                                  description derives from that one
#pragma once
#if defined(__HIPCC__)
#include "field.hip.h"
#include "wave_curve.hip.h"
#else                                  // a host build of sswu_map and sswu_iso_map alone (tests/native/p521_host_check.cpp)
#define DR_DEV static inline
#endif

namespace dr {

// Simplified SWU in the inversion-free form of RFC 9380 appendix F.2 with the sqrt_ratio of F.2.1.2 (p = 3 mod 4): one exponentiation,
// selects instead of branches.  In: u (normal, canonical value) and its parity.  Out: the point (xn / xd, y) of E', xd != 0.  The
// exceptional case tv2 = Z^2 u^4 + Z u^2 = 0 (u = 0 reaches it) takes xd = Z A, that is x1 = B / (Z A).  Every value is normalised
// where it is made, so each operand of a product below is what the field's mul / sqr accept (normal x normal for the 9 x 29-bit fields).
template <class C>
DR_DEV void sswu_map(const typename C::Fe& u, bool u_odd, typename C::Fe& xn, typename C::Fe& xd, typename C::Fe& y) {
    using Fe = typename C::Fe;
    const Fe A = C::a();
    const Fe tv1 = C::norm(neg(C::mul_neg_z(sqr(u))));                       // Z u^2
    Fe tv2 = C::norm(add(sqr(tv1), tv1));                                    // Z^2 u^4 + Z u^2
    const Fe tv3 = C::mul_b(add(tv2, C::one()));                             // B (tv2 + 1): the numerator of x1
    const Fe tv4 = mul(A, C::norm(select(C::is_zero(tv2), C::z(), neg(tv2))));   // A Z or -A tv2: its denominator
    Fe tv6 = sqr(tv4);
    tv2 = mul(C::norm(add(sqr(tv3), mul(A, tv6))), tv3);                     // tv3^3 + A tv3 tv4^2
    tv6 = mul(tv6, tv4);                                                     // tv4^3: the denominator of gx1
    tv2 = C::norm(add(tv2, C::mul_b(tv6)));                                  // ... + B tv4^3: its numerator
    // sqrt_ratio(tv2, tv6): y1 = sqrt(tv2 / tv6) if that is a square, sqrt(Z tv2 / tv6) otherwise
    const Fe s2 = mul(tv2, tv6);
    const Fe s1 = mul(sqr(tv6), s2);                                         // u v^3
    const Fe y1 = mul(C::pow_p34(s1), s2);
    const bool is_square = C::equal(mul(sqr(y1), tv6), tv2);
    const Fe y2 = mul(y1, C::sqrt_neg_z());
    const Fe yb = mul(mul(tv1, u), y2);                                      // the root for x2 = Z u^2 x1
    xn = select(is_square, tv3, mul(tv1, tv3));
    xd = tv4;
    y = select(is_square, y1, yb);
    y = C::norm(cneg(y, C::is_odd(y) != u_odd));                             // sgn0(y) = sgn0(u)
}

// The isogeny E' -> E on (xn / xd, y), by Horner in xn with the powers of xd as the homogenising factors, kept projective:
// (X : Y : Z) = (XN YD : y YN xd XD : xd XD YD) for x = XN / (xd XD), y' = y YN / YD.  ok = false when a denominator vanishes (Z = 0): the
// kernel of the isogeny, which the reference reports as the failing modular inverse; hashing cannot reach it in practice.  Without an
// isogeny the point is (xn : y xd : xd) and ok always.
template <class C>
DR_DEV typename C::Point sswu_iso_map(const typename C::Fe& xn, const typename C::Fe& xd, const typename C::Fe& y, bool& ok) {
    using Fe = typename C::Fe;
    typename C::Point r;
    if constexpr (!C::ISOGENY) {
        r.x = xn; r.y = mul(y, xd); r.z = xd;
        ok = true;
        return r;
    } else {
        const Fe d2 = sqr(xd), d3 = mul(d2, xd);
        Fe XN = mul2(Fe::template constant<C::XN3>(), xn, Fe::template constant<C::XN2>(), xd);
        XN = mul2(XN, xn, Fe::template constant<C::XN1>(), d2);
        XN = mul2(XN, xn, Fe::template constant<C::XN0>(), d3);
        Fe XD = C::norm(add(xn, mul(Fe::template constant<C::XD1>(), xd)));
        XD = mul2(XD, xn, Fe::template constant<C::XD0>(), d2);
        Fe YN = mul2(Fe::template constant<C::YN3>(), xn, Fe::template constant<C::YN2>(), xd);
        YN = mul2(YN, xn, Fe::template constant<C::YN1>(), d2);
        YN = mul2(YN, xn, Fe::template constant<C::YN0>(), d3);
        Fe YD = C::norm(add(xn, mul(Fe::template constant<C::YD2>(), xd)));
        YD = mul2(YD, xn, Fe::template constant<C::YD1>(), d2);
        YD = mul2(YD, xn, Fe::template constant<C::YD0>(), d3);
        const Fe dx = mul(xd, XD);
        r.x = mul(XN, YD);
        r.y = mul(mul(y, YN), dx);
        r.z = mul(dx, YD);
        ok = !C::is_zero(r.z);
        return r;
    }
}

#if defined(__HIPCC__)
// out[i] = the sum of the images of item i's `per_item` field elements (2: the uniform (RO) encoding, 1: the nonuniform one), u: n x
// per_item x 8 words (canonical, checked by the host), out: n x 16 words affine x || y, ok[i] = 0 where an isogeny denominator
// vanished.  One lane per item; one exponentiation per element and one inversion per item.  The body of both map kernels.
template <class C>
DR_DEV void sswu_map_to_curve(const uint32_t* __restrict__ us, uint32_t* __restrict__ out_xy, uint32_t* __restrict__ ok, uint32_t n,
                              uint32_t per_item) {
    using Fe = typename C::Fe;
    uint32_t i = blockIdx.x * C::BLOCK + threadIdx.x;
    const bool live = i < n;
    if (!live) i = n - 1;
    typename C::Point acc = C::identity();
    bool good = true;
#pragma unroll 1
    for (uint32_t e = 0; e < per_item; e++) {
        uint32_t w[8];
        wave_load8(us + ((size_t)i * per_item + e) * 8, w);
        Fe xn, xd, y;
        sswu_map<C>(C::unpack(w), (w[0] & 1u) != 0, xn, xd, y);
        bool ok_e;
        const typename C::Point pt = sswu_iso_map<C>(xn, xd, y, ok_e);
        good = good && ok_e;
        acc = C::add(acc, pt);
    }
    if (live) {
        wave_store_affine<C>(out_xy + (size_t)i * 16, acc);
        ok[i] = good ? 1u : 0u;
    }
}
#endif

}  // namespace dr
