// BLS12-381 G1 hashing kernels (DR_CURVE_BLS12_381_G1 and DR_CURVE_BLS12_381_G1_NU; the reference's specs/bls12_381_G1.py,
// BLS12_381_G1_RO / BLS12_381_G1_NU): the map of RFC 9380 onto E: y^2 = x^3 + 4 over Fq (fq28.hip.h) — simplified SWU onto the
// isogenous curve E' (sswu.hip.h's map under the description below), the 11-isogeny back, for the uniform (RO) variant the sum of two
// images, and the multiplication by h_eff.  The kernels over it are kernels_g1_h2c_entry.hip.h (one translation unit); this header holds
// no kernel, so that kernels_g2_h2c.hip.h can share its chain, predicates and small multiples.  kernels_g1.hip.h and the MSM
// (XYZZ coordinates with exceptional branches and an infinity flag, g1.hip.h) stay as they are: hashing needs a COMPLETE law, because the
// sum of two images may be a doubling (u0 = u1) or cancel (u1 = -u0) and the cofactor clearing starts from arbitrary points of E(Fq).
//
// Points cross the ABI as affine x || y, 48 + 48 bytes little-endian, canonical standard form; 96 zero bytes are the identity ((0, 0) is
// not on the curve).  Inside: Montgomery form (R = 2^392), homogeneous projective (X : Y : Z), identity (0 : 1 : 0), the complete law of
// Renes, Costello and Batina (2016), algorithms 7 (addition) and 9 (doubling) for a = 0 with b3 = 3 b = 12 — kernels_secp256k1.hip.h's
// law with another constant.  The comments give the limb class and the value range of every intermediate against fq28.hip.h's contract
// (mul / sqr: |limb| products within the 64-bit columns and |value| < 32 p; mul2: one operand with limbs up to 2^29, the others below
// 2^28):  n = a product (limbs 0..12 in [0, 2^28), value in (-0.01 p, 1.01 p));  cK = carried (limbs 0..12 in [0, 2^28), a small signed
// top limb) with |value| < K p.  A coordinate is c1.5 (a product, or a carried negation of one).  A product T of operands a, b lies in
// (a b / R, a b / R + p) and R / p = 2520.3, so a product of LAZY operands leaves n by value: the law's last products, whose operands
// reach |sum| < 352 p^2, return  w = a wide product (limbs 0..12 in [0, 2^28), value in (-0.14 p, 1.14 p)) — inside c1.5, which is all
// the next addition, doubling, inversion or from_mont28 asks of a coordinate.
#pragma once
#include "fq28.hip.h"
#include "sswu.hip.h"
#include "wave_curve.hip.h"

namespace dr {

constexpr int G1H_BLOCK = 64;         // one wave per workgroup, as the other map kernels

struct G1hPoint {
    Fq28 x, y, z;
};

DR_DEV Fq28 select(bool c, const Fq28& a, const Fq28& b) {       // c ? a : b
    Fq28 r;
#pragma unroll
    for (int i = 0; i < L28; i++) r.l[i] = c ? a.l[i] : b.l[i];
    return r;
}

struct G1hConsts {
    // 18 p as a limb image (not a Montgomery form: a multiple of p is 0 in every form): g1h_dbl adds it to keep Y^2 - 36 Z^2 below 32 p
    static constexpr uint32_t P18[14] = {0xffa0006u, 0xedfffffu, 0x7fffb13u, 0xffe877eu, 0xe8a2817u, 0x5158714u, 0x5416ecfu,
                                         0x1f5b517u, 0x0634f59u, 0x5227251u, 0x1cad0bbu, 0x36d947fu, 0x2780afeu, 0x01d4134u};
};

// 4 a, 12 a: lazy additions and a carry (4 x 2^28 and 3 x 2^28 stay below 2^31).  a: c1.5 or a difference of three n -> c6, c18 (c8.1,
// c24.3 for the law's X1 Z2 + X2 Z1 in (-2.02 p, 1.01 p))
DR_DEV Fq28 g1h_mul4(const Fq28& a) { return carry(dbl(dbl(a))); }
DR_DEV Fq28 g1h_mul12(const Fq28& a) {
    const Fq28 a4 = g1h_mul4(a);
    return carry(add(dbl(a4), a4));
}

DR_DEV G1hPoint g1h_identity() {
    G1hPoint p;
    p.x = Fq28::zero(); p.y = Fq28::one(); p.z = Fq28::zero();
    return p;
}

// algorithm 9, a = 0: 2 squarings, 4 products, one fused pair; coordinates c1.5 in, w out (x: 19.1 x 2.02 p^2 / R, within 0.016 p of
// [0, p); y: 352 p^2 / R, within 0.14 p; z: n)
DR_DEV G1hPoint g1h_dbl(const G1hPoint& p) {
    const Fq28 t0 = sqr(p.y);                                                    // Y^2: n
    const Fq28 z8 = carry(dbl(g1h_mul4(t0)));                                    // 8 Y^2: c8.1
    const Fq28 t1 = mul(p.y, p.z);                                               // n
    const Fq28 t2 = g1h_mul12(sqr(p.z));                                         // 12 Z^2: c12.2
    const Fq28 y3a = carry(add(t0, t2));                                         // Y^2 + 12 Z^2: c13.2
    // Y^2 - 36 Z^2 lies in (-36.4 p, 1.01 p); + 18 p: (-18.4 p, 19.1 p), limbs before the carry in (-3 x 2^28, 2^29)
    const Fq28 t0b = carry(add(sub(t0, add(t2, dbl(t2))), Fq28::constant<G1hConsts::P18>()));      // c19.1
    G1hPoint r;
    r.x = mul(t0b, dbl(mul(p.x, p.y)));                                          // 2 (Y^2 - 36 Z^2) X Y: c19.1 x (limbs < 2^29, < 2.02 p)
    r.y = mul2(t0b, y3a, t2, z8);                                                // t0b y3a + 8 . 12 Y^2 Z^2: |sum| < 19.1 x 13.2 + 12.2 x 8.1 < 352 p^2 (1024 p^2 allowed)
    r.z = mul(t1, z8);                                                           // 8 Y^3 Z
    return r;
}

// algorithm 7, a = 0: 6 products, 3 fused pairs; coordinates c1.5 in, w out (x: 75 p^2 / R, within 0.03 p of [0, p); y: 237 p^2 / R,
// within 0.095 p; z: 34 p^2 / R, within 0.014 p)
DR_DEV G1hPoint g1h_add(const G1hPoint& p, const G1hPoint& q) {
    const Fq28 t0 = mul(p.x, q.x), t1 = mul(p.y, q.y), t2 = mul(p.z, q.z);                        // n
    // (X1 + Y1) (X2 + Y2): c3 x (limbs < 2^29, < 3 p) = a product n' in (-0.01 p, 1.01 p); minus two n: c2.1
    const Fq28 t3 = carry(sub(mul(carry(add(p.x, p.y)), add(q.x, q.y)), add(t0, t1)));            // X1 Y2 + X2 Y1: c2.1
    const Fq28 t4 = carry(sub(mul(carry(add(p.y, p.z)), add(q.y, q.z)), add(t1, t2)));            // Y1 Z2 + Y2 Z1: c2.1
    const Fq28 y3 = g1h_mul12(sub(mul(carry(add(p.x, p.z)), add(q.x, q.z)), add(t0, t2)));        // 12 (X1 Z2 + X2 Z1): c24.3
    const Fq28 t0b = carry(add(t0, dbl(t0)));                                                      // 3 X1 X2: c3.1
    const Fq28 t2b = g1h_mul12(t2);                                                                // 12 Z1 Z2: c12.2
    const Fq28 z3 = carry(add(t1, t2b)), t1b = carry(sub(t1, t2b));                                // c13.2, c12.2
    G1hPoint r;
    r.x = mul2(t3, t1b, neg(t4), y3);                                                              // |sum| < 75 p^2
    r.y = mul2(t1b, z3, y3, t0b);                                                                  // |sum| < 237 p^2
    r.z = mul2(z3, t4, t0b, t3);                                                                   // |sum| < 34 p^2
    return r;
}

DR_DEV G1hPoint g1h_cneg(const G1hPoint& p, bool negate) {
    G1hPoint r = p;
    r.y = carry(cneg(p.y, negate));                                                                // c1.5
    return r;
}

// k P for a PUBLIC constant k by its bits, high to low: bit_length(k) - 1 doublings and popcount(k) - 1 additions; every lane takes the
// same (scalar) branches.  h_eff = 0xd201000000010001 (RFC 9380 8.8.1): 63 doublings, 6 additions.
template <int WORDS>
DR_DEV G1hPoint g1h_mul_public(const G1hPoint& P, const uint32_t (&k)[WORDS], int top_bit) {
    G1hPoint acc = P;
#pragma unroll 1
    for (int b = top_bit - 1; b >= 0; b--) {
        acc = g1h_dbl(acc);
        if ((k[b >> 5] >> (b & 31)) & 1u) acc = g1h_add(acc, P);
    }
    return acc;
}
__device__ const uint32_t G1H_H_EFF[2] = {0x00010001u, 0xd2010000u};

// ---------------------------------------------------------------- the description for sswu.hip.h
// E': y^2 = x^3 + A' x + B' (RFC 9380 8.8.1), Z = 11, sqrt(-Z) (-11 is a square mod p), all as Montgomery limb images (R = 2^392).  B'
// is not small, so mul_b is a full product; -Z x = -11 x is lazy.  p = 3 mod 4: the template's sqrt_ratio applies, with pow_p34 the chain below.
// The chain of (p - 3) / 4 by sliding windows over the odd powers x, x^3, x^5, x^7: start from x^3, then per entry c: c >> 2 squarings and
// a product with x^(2 (c & 3) + 1); one squaring at the end.  378 squarings and 108 products.
__device__ const uint8_t G1H_POW_CHAIN[105] = {
    8, 36, 16, 27, 14, 8, 27, 22, 15, 15, 15, 17, 8, 17, 8, 12, 22, 4, 21, 19, 8, 23, 14, 14, 4, 12, 25, 8, 22, 9, 18, 4, 17, 18, 9,
    13, 12, 27, 19, 8, 22, 9, 20, 23, 4, 23, 30, 16, 22, 19, 15, 13, 23, 17, 25, 8, 22, 8, 35, 14, 14, 13, 31, 14, 4, 16, 12, 35, 14, 18,
    19, 15, 15, 15, 15, 9, 18, 4, 26, 8, 23, 15, 15, 15, 15, 15, 14, 9, 23, 15, 9, 19, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 18, 18, 18};
constexpr int G1H_POW_FIRST = 3, G1H_POW_TAIL = 1;
DR_DEV Fq28 g1h_sqr_n(Fq28 a, int n) {
#pragma unroll 1
    for (int i = 0; i < n; i++) a = sqr(a);
    return a;
}
// x^((p - 3) / 4); x with limbs below 2^29 and |x| < 32 p (sqr's contract), n out.  The chain is public: its branches are scalar.
DR_DEV Fq28 g1h_pow_p34(const Fq28& x) {
    const Fq28 x2 = sqr(x), x3 = mul(x2, x), x5 = mul(x3, x2), x7 = mul(x5, x2);
    Fq28 r = x3;
#pragma unroll 1
    for (int i = 0; i < 105; i++) {
        const uint32_t c = G1H_POW_CHAIN[i];
        r = g1h_sqr_n(r, (int)(c >> 2));
        const uint32_t w = c & 3u;
        r = mul(r, w == 0 ? x : w == 1 ? x3 : w == 2 ? x5 : x7);
    }
    return g1h_sqr_n(r, G1H_POW_TAIL);
}

// is_zero / is_odd on the canonical standard-form value (from_mont28 takes any carried |x| < 32 p, and a difference of two such)
DR_DEV bool g1h_is_zero(const Fq28& x) {
    uint32_t w[12], acc = 0;
    from_mont28(x, w);
#pragma unroll
    for (int j = 0; j < 12; j++) acc |= w[j];
    return acc == 0;
}
DR_DEV bool g1h_is_odd(const Fq28& x) {
    uint32_t w[12];
    from_mont28(x, w);
    return (w[0] & 1u) != 0;
}
// the group order r of G1 (255 bits), for the subgroup check: r P = O
__device__ const uint32_t G1H_R[8] = {0x00000001u, 0xffffffffu, 0xfffe5bfeu, 0x53bda402u, 0x09a1d805u, 0x3339d808u, 0x299d7d48u, 0x73eda753u};

// wave_curve.hip.h's description of E(Fq): canonical standard-form words at the ABI (12 per coordinate; 96 zero bytes: the identity),
// Montgomery limbs inside, the limb images of the (n) coordinates in the LDS table (42 words a point, 8 x 42 x 64 x 4 = 86 016 bytes),
// 65 windows over the scalar AS IT IS: E(Fq) has order h r, so a scalar reduced mod r would be wrong for a point outside G1, and the
// recoding's 65th digit takes every 256-bit value.
struct G1hCurve {
    using Fe = Fq28;
    using Point = G1hPoint;
    static constexpr int WORDS = 12, SCALAR_WORDS = 8, BLOCK = G1H_BLOCK, WINDOWS = 65, LDS_WORDS = 14;
    static constexpr bool EXTENDED = false, ZERO_IS_IDENTITY = true;
    DR_DEV static Fq28 unpack(const uint32_t (&w)[12]) { return to_mont28(w); }
    DR_DEV static void pack(const Fq28& a, uint32_t (&w)[12]) { from_mont28(a, w); }
    DR_DEV static Fq28 inv(const Fq28& a) { return dr::inv(a); }
    DR_DEV static void to_lds(const Fq28& a, uint32_t (&w)[14]) { wave_limbs_to_words(a, w); }
    DR_DEV static Fq28 from_lds(const uint32_t (&w)[14]) { return wave_words_to_limbs<Fq28>(w); }
    DR_DEV static G1hPoint identity() { return g1h_identity(); }
    DR_DEV static G1hPoint from_affine(const Fq28& x, const Fq28& y) {
        G1hPoint P;
        P.x = x; P.y = y; P.z = Fq28::one();
        return P;
    }
    DR_DEV static G1hPoint add(const G1hPoint& p, const G1hPoint& q) { return g1h_add(p, q); }
    DR_DEV static G1hPoint dbl(const G1hPoint& p) { return g1h_dbl(p); }
    DR_DEV static G1hPoint cneg(const G1hPoint& p, bool negate) { return g1h_cneg(p, negate); }
    DR_DEV static void load_scalar(const uint32_t* p, uint32_t (&k)[8]) { wave_load8(p, k); }     // no reduction: see above
    DR_DEV static bool below_p(const uint32_t (&w)[12]) {
        uint32_t borrow = 0;
#pragma unroll
        for (int j = 0; j < 12; j++) (void)subb(w[j], FqParams::P[j], borrow);
        return borrow != 0;
    }
    // y^2 = x^3 + 4: ok and a root (either one) if it exists, by v^((p + 1) / 4) = v v^((p - 3) / 4) squared back (y = 0 cannot happen:
    // #E(Fq) is odd).  x: n (or the image of 12 words at or above p, below 9.9 p, which below_p refuses)
    DR_DEV static bool y_of_x(const Fq28& x, Fq28& y) {
        const Fq28 v = carry(dr::add(mul(sqr(x), x), Fq28::constant<Fq28Params::FOUR>()));             // c2.1
        y = mul(g1h_pow_p34(v), v);
        return g1h_is_zero(sub(sqr(y), v));
    }
    DR_DEV static bool is_odd(const Fq28& x) { return g1h_is_odd(x); }
    // r (x, y) = O by the bits of the public r: 254 doublings and 127 additions of the complete law.  For a point of the curve this is
    // the reference's valid_point.
    DR_DEV static bool in_subgroup(const Fq28& x, const Fq28& y) {
        return g1h_is_zero(g1h_mul_public(from_affine(x, carry(y)), G1H_R, 254).z);
    }
};

// sswu.hip.h's description of the map onto E' (see above)
struct G1hSswu : G1hCurve {
    static constexpr bool ISOGENY = true;
    static constexpr uint32_t A[14] = {0x5effb65u, 0x7b0e9afu, 0x2c3688cu, 0x2e2fbe8u, 0xf093be0u, 0x4e56b8eu, 0x51e099cu, 0x22aa2e7u, 0xbb7ea2bu, 0x50194edu, 0xaee9f0bu, 0x4130e5du, 0x3ac15b2u, 0x0019762u};
    static constexpr uint32_t B[14] = {0x2b73540u, 0xa971fe2u, 0xd700d19u, 0xb3af1f2u, 0xb92fe3eu, 0xa0ed883u, 0x27b2b6bu, 0x40a0c1bu, 0x054e265u, 0xed52ae2u, 0xbf6c97fu, 0xc537abcu, 0x6b32a3eu, 0x0001fbeu};
    static constexpr uint32_t Z[14] = {0x4188692u, 0x4a00002u, 0x81d9ca8u, 0x8d914dbu, 0xc9e9248u, 0x6609019u, 0x3930735u, 0x779fd52u, 0x1a814d5u, 0x352b5aau, 0x0a0ec9fu, 0x3fb69f4u, 0x2096bbeu, 0x0008220u};
    static constexpr uint32_t SQRT_NEG_Z[14] = {0x725794eu, 0x22ed8fbu, 0xf79f97fu, 0xa4701d4u, 0x3d58b00u, 0x22b7dfcu, 0x050a61cu, 0x3e5e710u, 0xa63a15eu, 0xdee6cfau, 0x7983f42u, 0x3cc6e9du, 0xb3381abu, 0x0016957u};
    DR_DEV static Fq28 a() { return Fq28::constant<A>(); }
    DR_DEV static Fq28 z() { return Fq28::constant<Z>(); }
    DR_DEV static Fq28 sqrt_neg_z() { return Fq28::constant<SQRT_NEG_Z>(); }
    DR_DEV static Fq28 one() { return Fq28::one(); }
    DR_DEV static Fq28 mul_neg_z(const Fq28& x) { return carry(sub(x, g1h_mul12(x))); }           // -Z x = x - 12 x (Z = +11 here): x n -> c11.2, carried but not normal
    DR_DEV static Fq28 mul_b(const Fq28& x) { return mul(x, Fq28::constant<B>()); }               // x: limbs < 2^29, |x| < 13.4 p (tv2 + 1)
    DR_DEV static Fq28 norm(const Fq28& x) { return carry(x); }
    DR_DEV static bool is_zero(const Fq28& x) { return g1h_is_zero(x); }
    DR_DEV static bool equal(const Fq28& x, const Fq28& y) { return g1h_is_zero(sub(x, y)); }
    DR_DEV static Fq28 pow_p34(const Fq28& x) { return g1h_pow_p34(x); }
};

// The isogeny E' -> E of degree 11 (RFC 9380 appendix E.2) on (xn / xd, y): coefficient lists lowest degree first, 12 / 10 (+ the implied
// leading 1) / 16 / 15 (+ 1), Montgomery limb images.  They are tables in constant memory read by a loop counter — a scalar load, the
// same in every lane; nothing goes to scratch.  sswu_iso_map spells its 3-isogeny out and stays as it is (the existing kernels come out
// unchanged); this is its counterpart for lists of any length.
__device__ const uint32_t G1H_XN[12][14] = {
    {0x030c68du, 0x0ff3af0u, 0xe8c656fu, 0x980858au, 0xb8b5055u, 0x50bb941u, 0x4488cb7u, 0x566f7fbu, 0xf70f3bau, 0xb13d41eu, 0xb84a25au, 0xc92d3ebu, 0x59c2347u, 0x00095eeu},
    {0xbd48ae9u, 0xca385cdu, 0x2aa9c67u, 0x3d220dcu, 0x2803588u, 0x924f70eu, 0xec7b8ceu, 0xc3459f7u, 0x3c7c377u, 0x1ce5782u, 0x9bab1eau, 0x857b73bu, 0x178080bu, 0x000731fu},
    {0xb7ea03du, 0xa13a480u, 0x4c6b938u, 0xc086547u, 0x6afb25du, 0x68803f7u, 0x7360321u, 0x91fe8ecu, 0xe8d3767u, 0x6c2fefau, 0x69d83f9u, 0x62e003bu, 0x30cfadcu, 0x0019c70u},
    {0x756eb7bu, 0xb02870fu, 0x4217068u, 0x3078964u, 0xf7e79d1u, 0xab1672bu, 0xc5111d1u, 0xe867e73u, 0xf5bb8e6u, 0x0cfcb37u, 0xac958b9u, 0x1b35e66u, 0x013e2a9u, 0x000d3b3u},
    {0x76d9a35u, 0xd84bd6au, 0xd85ab74u, 0x8ac08edu, 0x0cb3af0u, 0xb5ace72u, 0x9010984u, 0x9f14418u, 0xaf083bbu, 0xce11733u, 0xf470a6au, 0x95a01bbu, 0x3ce89b5u, 0x0017a6eu},
    {0x6786159u, 0x88e2f43u, 0x3bdb0dcu, 0x9be2177u, 0xd13ed90u, 0x0c6c992u, 0x6708bcfu, 0x7065e9eu, 0x46986bau, 0xdc350aeu, 0x5c69feeu, 0x780646bu, 0x68b2f21u, 0x0011b9au},
    {0x06a5219u, 0xa5c9534u, 0xbe95544u, 0x6a456deu, 0xbf09463u, 0x5f3ac15u, 0x8438851u, 0xccc0cddu, 0x70433e1u, 0x316386du, 0xad5c7deu, 0xf3e8be0u, 0xc947e7au, 0x00153e1u},
    {0x6c4fb39u, 0x45490f0u, 0x9819133u, 0xa8ef501u, 0x687c978u, 0x3fa2a25u, 0x596fa65u, 0xacde2b8u, 0x9e351e0u, 0xe08e5e4u, 0x642dc8bu, 0x9780b04u, 0x7310a58u, 0x0015078u},
    {0x5d06035u, 0xa6ba78du, 0x07600f8u, 0x9a9de79u, 0x0d4b78eu, 0xe93a2e7u, 0x26f4027u, 0xca1ab0fu, 0x4521c42u, 0x5271450u, 0x250dfd6u, 0x4b8f312u, 0x3db162fu, 0x000c321u},
    {0x59006e1u, 0x2057bffu, 0xcb22754u, 0xaee4ae8u, 0x1eae938u, 0x3a15842u, 0x9d9fee3u, 0x265a805u, 0x4ffe802u, 0xc3af4b5u, 0x5721a8au, 0xaef6fa8u, 0x5c7a7ecu, 0x0019e87u},
    {0x93b1c44u, 0x957e7ddu, 0x375f4e8u, 0xd4864e6u, 0xfa83347u, 0x615e569u, 0xcb9f411u, 0xff751c3u, 0x796563du, 0x82b4248u, 0xa557964u, 0x44f3103u, 0x82b6f87u, 0x0007a7au},
    {0xdc7255au, 0x1c50658u, 0xbd5b508u, 0xfbdeb64u, 0x965c0f9u, 0x0e31629u, 0x9ddaf67u, 0xdc3e32fu, 0x8aab07bu, 0x34cba94u, 0xd208f93u, 0x5fd64edu, 0x604e589u, 0x0019679u},};
__device__ const uint32_t G1H_XD[10][14] = {
    {0x0fd9a51u, 0xad77fdbu, 0xfa0bcf0u, 0x1000d8cu, 0x4d11ab8u, 0x124fc8cu, 0x90fdbdau, 0x2d514b0u, 0x5b4a5d0u, 0xb84fc42u, 0x344e7eeu, 0xa9c63adu, 0x3aec192u, 0x00139c8u},
    {0x6dc8390u, 0xea3ba50u, 0x76a3907u, 0x0afcfadu, 0x4493a0au, 0xea3ea41u, 0xaea08deu, 0x5718b76u, 0x89282c4u, 0x7a41c20u, 0xc2957e4u, 0xbeb5cc8u, 0xdbb89f9u, 0x00132e3u},
    {0x01ea679u, 0x57a644au, 0xff0c144u, 0xcd96414u, 0xf445138u, 0xd7a3c1fu, 0x0cb3565u, 0xf78713bu, 0x23832d0u, 0x5c79438u, 0x699d020u, 0xab317f3u, 0xf128db2u, 0x000721cu},
    {0x92b40c5u, 0x7d11827u, 0x0fc13b0u, 0x901696fu, 0x1db5236u, 0x504df72u, 0x37a63e3u, 0xb6c0e97u, 0x2b09fafu, 0x2963573u, 0x94fb7bau, 0x9b6e3e5u, 0x20245d5u, 0x0007942u},
    {0xb46256au, 0x27ae6acu, 0x81f8d8cu, 0x334ede7u, 0x1b50697u, 0x177ebfcu, 0xfc69649u, 0xb8920deu, 0x79f25b1u, 0x12b792bu, 0xb36f019u, 0x54871d9u, 0x06e63d3u, 0x00046cdu},
    {0x42f1feau, 0xc822cd1u, 0x5b50d9du, 0x4295133u, 0x0fa640cu, 0xa85e5bbu, 0x3508cdbu, 0x71eeecbu, 0x28c7eb1u, 0x70f8a91u, 0x2e7da27u, 0x77e790bu, 0xf72c1c2u, 0x0017f98u},
    {0x2683982u, 0xf01151bu, 0x1b3f57bu, 0x65e2d51u, 0xbfc0b2cu, 0xd335d76u, 0xdc6f287u, 0x4a5bf52u, 0xfcfa49bu, 0x3c23398u, 0x5a07f47u, 0x20e1687u, 0x8984d72u, 0x000afceu},
    {0x7164c08u, 0xf074787u, 0x0f0a8acu, 0x0d291b6u, 0x366fda5u, 0xd9c0621u, 0x90c32f8u, 0xcb16261u, 0x046659fu, 0xe78056bu, 0x2dbadd8u, 0x26e85adu, 0xb65f8b8u, 0x0000714u},
    {0x33e522eu, 0x75439c1u, 0x7a73c28u, 0x3b0fb52u, 0xcf341dcu, 0x31403c0u, 0xe677513u, 0x54df788u, 0x7adcbabu, 0x4648ea7u, 0xecadebdu, 0xe99d242u, 0x8ceb0c6u, 0x0013ae7u},
    {0xcfc06c3u, 0xcbc97bau, 0x6c0cb80u, 0x73a8ce8u, 0xf900b6fu, 0x03dcbfcu, 0x8c8af6bu, 0x7328c88u, 0x9bf7020u, 0x6e83d15u, 0xa78754eu, 0x0fca66cu, 0x981da73u, 0x0010190u},};
__device__ const uint32_t G1H_YN[16][14] = {
    {0x39d66d5u, 0x00f3e28u, 0x3674e9du, 0x5861fd5u, 0xae9d8f2u, 0xe86e476u, 0xb02f5c6u, 0xb6c56d5u, 0x185fc0cu, 0x047b429u, 0x923aa80u, 0xdcbda22u, 0xdcd308fu, 0x00157d3u},
    {0x26b9433u, 0xbc5fa54u, 0xc78b5ecu, 0xcccf1c2u, 0x276281fu, 0xcc562d8u, 0xb6bbbccu, 0x30bf3d5u, 0x438cf87u, 0x63196b7u, 0x62c406au, 0x8d5c2b0u, 0x4851ecfu, 0x00173fau},
    {0xd378f14u, 0x06922a5u, 0xe7d4972u, 0xe46e61cu, 0x98e0283u, 0x47768c1u, 0x4044139u, 0x486e964u, 0x5674c1du, 0x2f89171u, 0xaeba406u, 0x77624f9u, 0xc37b93cu, 0x000e3a3u},
    {0xfe4102fu, 0x7095bfau, 0xb077bcau, 0xa6f4ab5u, 0xaeedc15u, 0xa7648cdu, 0xe28e016u, 0x19a5e73u, 0x0090a40u, 0x2d52edcu, 0x2ee6fdeu, 0xc063892u, 0x865b72du, 0x000852du},
    {0xa5c944au, 0x84c7ff8u, 0x6fd6257u, 0xe39f3dau, 0xf653874u, 0x33f5274u, 0x03ab6d5u, 0x1990e20u, 0x7ac98edu, 0x149cd28u, 0x2067ba8u, 0xece6f12u, 0xb49788bu, 0x0011fcdu},
    {0xbc3324fu, 0x1d31111u, 0xd82aa63u, 0xf5f2eb4u, 0x4f303fcu, 0x61d4b0au, 0x504fd27u, 0x2c0443cu, 0x9e5fa4au, 0xf333adfu, 0x18fa71du, 0x765bc81u, 0x68b4399u, 0x000fcb0u},
    {0x7f2fa91u, 0xbfb0d7au, 0x6197ab3u, 0x81e7f0fu, 0x5052271u, 0x615443bu, 0x0f33c8du, 0x5b830d3u, 0xaf1b579u, 0xdbfe3c7u, 0x4aa1630u, 0xc3517b4u, 0x64e9465u, 0x0018c8cu},
    {0x4f07932u, 0xff72f7cu, 0x891b0dcu, 0x91010c8u, 0xa419b5au, 0xc28a0bcu, 0x4af0f47u, 0x201a4c4u, 0x4434f2du, 0xf7d374eu, 0xe0f0b06u, 0xfe11e11u, 0x8ea9a64u, 0x0010ba3u},
    {0xda2a912u, 0xf3844e0u, 0xa33c850u, 0xa4597f6u, 0xe500b99u, 0x3dabcc2u, 0x5ebf823u, 0x8033b73u, 0x0b10cc1u, 0x9ed6054u, 0x35820d3u, 0x9de9cb0u, 0xf98ff87u, 0x0017c40u},
    {0x2e219b0u, 0xaeb03c1u, 0xa1787ccu, 0xfb43e88u, 0xbffd9b5u, 0x00f1052u, 0x997c947u, 0x02ecb32u, 0xf222476u, 0xea58766u, 0x42a4c25u, 0x9ada96fu, 0x72ca9f2u, 0x0001bc9u},
    {0x1697b18u, 0x70ca89fu, 0xc4f381au, 0x109a454u, 0x20b8876u, 0xb72ac94u, 0x83925f6u, 0x3f3c23du, 0x09d95f9u, 0x9284443u, 0xcc8aee1u, 0x26d5212u, 0x3593575u, 0x00171ceu},
    {0xa456c4eu, 0xd5900b8u, 0x9c4bb62u, 0xec3754cu, 0xde439afu, 0x14e718cu, 0xc29a8f7u, 0x2ce9b0au, 0x990e057u, 0xd2b68b5u, 0x7888981u, 0xd2f620eu, 0xdf56773u, 0x0005880u},
    {0x6271fd5u, 0x3000074u, 0xcf5d75du, 0x9dc74b7u, 0xa5ae192u, 0x59eada4u, 0x976a3f4u, 0xe8ad7d0u, 0x571e216u, 0x98fa77au, 0xebf47adu, 0x9ec36e0u, 0xb95e9b1u, 0x0012f17u},
    {0x6546a47u, 0x96b538du, 0x63a9ecbu, 0x19cd546u, 0xc5e0342u, 0x4fe1964u, 0x9118089u, 0x0faf096u, 0x3dc87b0u, 0x23f2c78u, 0xe40afa5u, 0x8d87ad6u, 0xd782843u, 0x000b2bcu},
    {0x087f076u, 0x2b4b6e4u, 0xd9015a9u, 0x9cfa90fu, 0xf46fadfu, 0x3c2c636u, 0xf562766u, 0x6fc05c1u, 0x59155c4u, 0x8a6eb06u, 0x65fea1au, 0x0bcd9d8u, 0xa89a41eu, 0x000a7ffu},
    {0x8864175u, 0x47c17d9u, 0x22ab331u, 0x16e4de8u, 0x6378227u, 0xc4d0053u, 0x7ca2f03u, 0x97b76dau, 0x689fa48u, 0x34f4de4u, 0x89c3b38u, 0xb2bb7ccu, 0xd66f3a3u, 0x0012db8u},};
__device__ const uint32_t G1H_YD[15][14] = {
    {0x54d7133u, 0x9c9d47eu, 0x1610796u, 0x8a970a8u, 0x590982bu, 0xc55c287u, 0xb75cce1u, 0x018898du, 0x2727a48u, 0xe9dec8du, 0x68661f9u, 0x293ebc3u, 0x9a7541cu, 0x001529eu},
    {0x5ed5022u, 0xd64f553u, 0x1118b86u, 0x745f2f5u, 0x8b4eb8bu, 0x0ef5f1cu, 0xe4bee11u, 0x481911cu, 0x11c90a9u, 0x817cabeu, 0x9c17edau, 0x8599053u, 0x094d50du, 0x00094b3u},
    {0x00b46a5u, 0xc76df47u, 0x342308fu, 0x59ba0cdu, 0xebe9955u, 0x20aa69du, 0xb83807eu, 0xb9b20e5u, 0x75e615au, 0x147a68bu, 0x58f9e60u, 0xf0c601bu, 0x1c92d1du, 0x0008957u},
    {0x5db3073u, 0x9fef3b7u, 0xb402026u, 0x75511b3u, 0xdf98902u, 0x8b41ddcu, 0x7f75504u, 0x3538cb4u, 0x6e99343u, 0xe6ca465u, 0x717904au, 0x4eb2b1bu, 0x5bfbb50u, 0x000cca2u},
    {0x7fc709du, 0xba2ea26u, 0x3003cfdu, 0x1c95674u, 0x554d5e3u, 0xf304a64u, 0xb867e27u, 0xe952a42u, 0x7377773u, 0x8eebbd9u, 0x8bf39e2u, 0x0cfbc57u, 0xcdff819u, 0x001967du},
    {0x5e6928cu, 0x52efeebu, 0xb55df97u, 0x8a55b88u, 0x89d1ef2u, 0x1871ffau, 0x89c1921u, 0x85470fau, 0x4e28733u, 0x740aa83u, 0xebc5913u, 0xf49b4beu, 0x94a887bu, 0x0013d79u},
    {0xe18f3d7u, 0x8ceb5fau, 0xcf0bc5eu, 0x0b2923cu, 0x8d82001u, 0xbee26d0u, 0x48b2e3eu, 0x6416b20u, 0x2112909u, 0x1683477u, 0xdc10779u, 0x21b2505u, 0x8d5ac43u, 0x000350cu},
    {0xc0f5ad5u, 0x720e5b8u, 0x53064e0u, 0x965a8d2u, 0x7a6f038u, 0x7ee4b8fu, 0x835a4dbu, 0xae16545u, 0xede16abu, 0x524d14fu, 0x3e5323au, 0xd330b44u, 0xb375300u, 0x0018edfu},
    {0x504a4cfu, 0x4192ec7u, 0x897a6e7u, 0xab5fd8fu, 0x105a4f0u, 0x30e8d93u, 0x3a4fa97u, 0x8754277u, 0xf596f4fu, 0x8653550u, 0x7e800c7u, 0x4abd2b4u, 0x9f2de8cu, 0x000525eu},
    {0x6d72dd5u, 0xa0d449fu, 0x630a22fu, 0x5d61da2u, 0x8b26111u, 0xfd1be77u, 0x43af281u, 0x98c1b10u, 0xd846418u, 0x8c95475u, 0xe8ccf8du, 0xcbace06u, 0xd05f309u, 0x00084b9u},
    {0xd936e47u, 0x0b9285fu, 0xd7c02eau, 0xa8684e6u, 0x6cb7671u, 0xfc08db5u, 0xef4a55bu, 0xa97ed24u, 0x40fb1e8u, 0x9301e9au, 0x9924e0du, 0xe3124bbu, 0xc9a9748u, 0x0009d1au},
    {0x8981ac7u, 0x496a7c3u, 0x003f039u, 0x0eca4d0u, 0xb593fafu, 0x9f25af4u, 0xa742aa8u, 0x7928bf7u, 0x4d32c8du, 0xc7598e0u, 0x617b836u, 0xf672629u, 0xfd4aa0cu, 0x000c38au},
    {0x511b45au, 0x02bf274u, 0x9545249u, 0x0676c8cu, 0x496f2f5u, 0xc6f3ad5u, 0x160cc82u, 0xa8859abu, 0x7d7e5e8u, 0x7f705f0u, 0xd7f8a1fu, 0x3eddffdu, 0x4dcb1efu, 0x00095cfu},
    {0x79fd1bfu, 0x176ca15u, 0xf55b410u, 0x991bf51u, 0x4612056u, 0x1aebfeau, 0xc1885b5u, 0x06c3848u, 0xadb7dddu, 0xdb4b9f1u, 0x8c3eccdu, 0x2f113d7u, 0xf0fd115u, 0x000f0b1u},
    {0x37a34cfu, 0x322e398u, 0x0213164u, 0x2d7ddd2u, 0xc4601d1u, 0x354fc73u, 0xd796eb7u, 0x32faa36u, 0x463826eu, 0xffef4e5u, 0x1e0d4d3u, 0xa46274au, 0x54daaecu, 0x000b250u},};
DR_DEV Fq28 g1h_row(const uint32_t (&row)[14]) {
    Fq28 r;
#pragma unroll
    for (int t = 0; t < L28; t++) r.l[t] = (int32_t)row[t];
    return r;
}
// The four Horner evaluations in xn run side by side, step j sharing the homogenising factor xd^j:  N <- N xn + k_(deg - j) xd^j,  so that
// N = xd^deg N(xn / xd).  Then, as sswu_iso_map,  (X : Y : Z) = (XN YD : y YN xd XD : xd XD YD);  ok = false when a denominator vanishes.
// xn, xd: n; y: c1.5.  Every accumulator is n (a mul2 of n operands) except the two monic starts xn + k xd: c2.1.
DR_DEV G1hPoint g1h_iso_map(const Fq28& xn, const Fq28& xd, const Fq28& y, bool& ok) {
    Fq28 XN = mul2(g1h_row(G1H_XN[11]), xn, g1h_row(G1H_XN[10]), xd);
    Fq28 XD = carry(add(xn, mul(g1h_row(G1H_XD[9]), xd)));
    Fq28 YN = mul2(g1h_row(G1H_YN[15]), xn, g1h_row(G1H_YN[14]), xd);
    Fq28 YD = carry(add(xn, mul(g1h_row(G1H_YD[14]), xd)));
    Fq28 dpow = xd;
#pragma unroll 1
    for (int j = 2; j <= 15; j++) {
        dpow = mul(dpow, xd);                                                    // xd^j
        if (j <= 11) XN = mul2(XN, xn, g1h_row(G1H_XN[11 - j]), dpow);
        if (j <= 10) XD = mul2(XD, xn, g1h_row(G1H_XD[10 - j]), dpow);
        YN = mul2(YN, xn, g1h_row(G1H_YN[15 - j]), dpow);
        YD = mul2(YD, xn, g1h_row(G1H_YD[15 - j]), dpow);
    }
    const Fq28 dx = mul(xd, XD);
    G1hPoint r;
    r.x = mul(XN, YD);
    r.y = mul(mul(y, YN), dx);
    r.z = mul(dx, YD);
    ok = !g1h_is_zero(r.z);
    return r;
}

DR_DEV void g1h_store_affine(uint32_t* out, const G1hPoint& acc) {               // x || y, 24 words; Z = 0 stores 96 zero bytes (0^-1 = 0)
    const Fq28 zi = inv(acc.z);
    uint32_t w[12];
    from_mont28(mul(acc.x, zi), w);
    store_words12(out, w);
    from_mont28(mul(acc.y, zi), w);
    store_words12(out + 12, w);
}

}  // namespace dr
