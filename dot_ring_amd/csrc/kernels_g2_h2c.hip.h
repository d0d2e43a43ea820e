// BLS12-381 G2 hashing kernels (DR_CURVE_BLS12_381_G2 and DR_CURVE_BLS12_381_G2_NU; the reference's specs/bls12_381_G2.py,
// BLS12_381_G2_RO / BLS12_381_G2_NU): the map of RFC 9380 onto E: y^2 = x^3 + 4 (1 + i) over Fq2 (fq2_28.hip.h) — simplified SWU onto the
// isogenous curve E': y^2 = x^3 + 240 i x + 1012 (1 + i), the 3-isogeny back (appendix E.3), for the uniform (RO) variant the sum of two
// images, and the cofactor clearing by the endomorphism psi (appendix G.3) — with a scalar multiplication, a curve / subgroup check and a
// diagnostic of the field.  sswu.hip.h's template does not fit: its sqrt_ratio is one exponentiation by (p - 3) / 4 in a PRIME field;
// g2h_sswu_map below has the same inversion-free shape (xn / xd) with Fq2's square root built from Fq's chain (fq2_28.hip.h).
//
// Points cross the ABI as affine x || y, each coordinate c0 || c1, 4 x 48 bytes little-endian, canonical standard form; 192 zero bytes
// are the identity ((0, 0) is not on the curve).  Inside: Montgomery form, homogeneous projective (X : Y : Z), identity (0 : 1 : 0), the
// complete law of Renes, Costello and Batina (2016), algorithms 7 and 9 for a = 0 with b3 = 3 b = 12 (1 + i) — kernels_g1_h2c.hip.h's law
// over the quadratic extension.  The classes (n, cK) in the comments are fq2_28.hip.h's, per component.  A COORDINATE is c3: an n, the
// carried sum of two n (c2.1) or a carried negation of either.
//
// Staging.  A point is 84 registers, twice G1's, and the clearing holds four of them; so the map runs as two launches on one stream:
//   k_blsg2_map_iso     one lane per FIELD ELEMENT: SSWU and the isogeny; the projective image goes to a context-owned HBM buffer as six
//                       14-limb images (336 bytes an element)
//   k_blsg2_sum_clear   one lane per ITEM: the sum of its one or two images, the clearing, the affine store
// and inside the clearing P, then the running sum, wait in that buffer while the multiplications by |z| run (g2h_clear_cofactor).
#pragma once
#include "fq2_28.hip.h"

namespace dr {

constexpr int G2H_BLOCK = 64;         // one wave per workgroup, as the other map kernels
constexpr int G2H_STAGE_WORDS = 6 * L28;

struct G2hPoint {
    Fq2 x, y, z;
};

// Montgomery limb images (R = 2^392) of the map's constants: 240 and 1012 (A' = 240 i and B' = 1012 (1 + i) act through one Fq product a
// component), sqrt(-5) in Fq (5 = norm(Z)), Z = -(2 + i), the isogeny's coefficients k_(i,j) of appendix E.3 (XN: 4, XD: 2 + the leading
// 1, YN: 4, YD: 3 + the leading 1; c0 then c1), psi's cx = (1 + i)^-((p - 1) / 3) and cy = (1 + i)^-((p - 1) / 2) and psi^2's
// 2^-((p - 1) / 3).  tests/test_bls12_381_g2_cpu.py recomputes every one from its integer.
struct G2hConsts {
    static constexpr uint32_t K240[14] = {0x38d971au, 0xb200031u, 0xa8615e6u, 0x10c7ab9u, 0x7e3b474u, 0xf7b9eb9u, 0x1c8ac67u, 0xde7ef8du, 0x644ceb4u, 0xa67d477u, 0xdba5cfcu, 0x0fba9d5u, 0x49def66u, 0x000bf67u};
    static constexpr uint32_t K1012[14] = {0x8d9b1c4u, 0xb4000cfu, 0xaa45422u, 0xe05c88fu, 0xd093742u, 0x1041395u, 0x98d4027u, 0x5ae28bdu, 0xb5b3a2cu, 0xd4ad031u, 0x37d19dau, 0xacc1043u, 0x5c46e61u, 0x00141acu};
    static constexpr uint32_t SQRT_NEG5[14] = {0xa300f16u, 0xb5407f4u, 0xf2e0189u, 0x109f289u, 0xd163476u, 0xd082982u, 0x2514131u, 0x572eaf2u, 0x257fc31u, 0x8076e7bu, 0x27e19bau, 0x2e91e67u, 0x40ab7bbu, 0x000f077u};
    static constexpr uint32_t Z[2][14] = {{0x96fb13bu, 0x4efffffu, 0x3fa9d86u, 0xe641d71u, 0xd3ff8ebu, 0x99b29edu, 0xef86393u, 0x3f662afu, 0x11614ffu, 0x267d615u, 0x17c0325u, 0xe440fb9u, 0x5363f8bu, 0x000f11cu},
        {0xcb7adf3u, 0x26fffffu, 0x3fd4ea0u, 0xf320443u, 0x9b20bcbu, 0x1d54a7eu, 0xf2fca33u, 0x19759edu, 0xac6b042u, 0x39151c5u, 0x691dcb4u, 0xe56da35u, 0xb903c85u, 0x0014896u}};
    static constexpr uint32_t XN0[2][14] = {{0x09e0c6bu, 0x30c71ceu, 0xd3e7c31u, 0x080bb88u, 0xd13fb03u, 0xdbef69fu, 0xe836004u, 0xbc8765au, 0xc02926cu, 0xc201508u, 0x48bcc9au, 0x34a73b7u, 0x7483a7du, 0x0019c2fu},
        {0x09e0c6bu, 0x30c71ceu, 0xd3e7c31u, 0x080bb88u, 0xd13fb03u, 0xdbef69fu, 0xe836004u, 0xbc8765au, 0xc02926cu, 0xc201508u, 0x48bcc9au, 0x34a73b7u, 0x7483a7du, 0x0019c2fu}};
    static constexpr uint32_t XN1[2][14] = {{0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u},
        {0xc952532u, 0xbf55554u, 0x2a37ce1u, 0xddadfdeu, 0xd928cc7u, 0x0c49b32u, 0x9b10ee3u, 0xb22f822u, 0x9233efbu, 0x5633f22u, 0xa358aafu, 0x41451d5u, 0x5ac2e65u, 0x0002c1au}};
    static constexpr uint32_t XN2[2][14] = {{0x9b51812u, 0x1f55555u, 0x2ae4149u, 0x1127b26u, 0xf5ad848u, 0x1ad1d75u, 0xa8ea961u, 0x1a6d51au, 0xfe5ac07u, 0xa092de4u, 0xe8cf0ebu, 0x45f7bc6u, 0xf14224du, 0x0018a03u},
        {0x64a9299u, 0xdfaaaaau, 0x151be70u, 0xeed6fefu, 0x6c94663u, 0x8624d99u, 0x4d88771u, 0xd917c11u, 0x4919f7du, 0xab19f91u, 0xd1ac557u, 0xa0a28eau, 0x2d61732u, 0x000160du}};
    static constexpr uint32_t XN3[2][14] = {{0x7799757u, 0xc21c71cu, 0x78e854du, 0x56c2a78u, 0xdaef6b1u, 0xbd622a6u, 0xdea2686u, 0xbbf6502u, 0x38ec96du, 0x9de2a8eu, 0x70a448au, 0xb921ca9u, 0x38c1f9bu, 0x000f0deu},
        {0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u}};
    static constexpr uint32_t XD0[2][14] = {{0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u},
        {0x3bb96f0u, 0x2fffff1u, 0xf3e2c5bu, 0x615c643u, 0x22c9bbcu, 0x09d883eu, 0x6de304du, 0xe3f894eu, 0xdc90d81u, 0x8020db8u, 0xc5633f7u, 0x1515824u, 0x55471aeu, 0x00166a5u}};
    static constexpr uint32_t XD1[2][14] = {{0x760834au, 0x2200002u, 0x8204dc2u, 0x9a6fbadu, 0x910a528u, 0xe9ab0aau, 0x3ca6dd4u, 0x51af490u, 0xb58b018u, 0x47c315au, 0x5b6c62eu, 0x40e3470u, 0x86368b8u, 0x000d99au},
        {0x89f2761u, 0xdcffffdu, 0xbdfb1f7u, 0x658ef67u, 0xd137983u, 0xb74ba64u, 0xb9cc2fdu, 0xa1d5c9bu, 0x91e9b6cu, 0x03e9c1bu, 0x5f0f015u, 0xa5b7041u, 0x986d0c7u, 0x000c676u}};
    static constexpr uint32_t YN0[2][14] = {{0xc94688eu, 0x4c84bdfu, 0x8e2ae5du, 0xf4abd49u, 0xd92e31cu, 0x24b6e04u, 0xba0223du, 0x195094cu, 0xb108e51u, 0x7f98fc0u, 0x9477308u, 0x4b3a979u, 0x98274deu, 0x000ba95u},
        {0xc94688eu, 0x4c84bdfu, 0x8e2ae5du, 0xf4abd49u, 0xd92e31cu, 0x24b6e04u, 0xba0223du, 0x195094cu, 0xb108e51u, 0x7f98fc0u, 0x9477308u, 0x4b3a979u, 0x98274deu, 0x000ba95u}};
    static constexpr uint32_t YN1[2][14] = {{0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u},
        {0x1dcb082u, 0xebc71c9u, 0x0fde066u, 0xd32af43u, 0x116cf5du, 0xa99005au, 0x655b52du, 0x0cade66u, 0x9c87dc1u, 0x7e27fc9u, 0x4c5f681u, 0x997af88u, 0x86ba28cu, 0x001890bu}};
    static constexpr uint32_t YN2[2][14] = {{0x3251ea2u, 0x6f55555u, 0x2a8df15u, 0xf76ad82u, 0x676b287u, 0x138dc54u, 0xa1fdc22u, 0x664e69eu, 0xc847581u, 0x7b63683u, 0x4613dcdu, 0x439e6ceu, 0x2602859u, 0x000db0fu},
        {0xcda8c09u, 0x8faaaaau, 0x15720a4u, 0x0893d93u, 0xfad6c24u, 0x8d68ebau, 0x54754b0u, 0x8d36a8du, 0x7f2d603u, 0xd0496f2u, 0x7467875u, 0xa2fbde3u, 0xf8a1126u, 0x000c501u}};
    static constexpr uint32_t YN3[2][14] = {{0x82cb11cu, 0x69a12f6u, 0x425d379u, 0xe314034u, 0xd7c62a8u, 0xa131822u, 0x07f036eu, 0xbd2f963u, 0x5a2d607u, 0x8f4364du, 0xc347b3du, 0x647d802u, 0x4ca08a1u, 0x0003a66u},
        {0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u}};
    static constexpr uint32_t YD0[2][14] = {{0x6673449u, 0x24fffa7u, 0x7750b81u, 0x4830e2du, 0xe570d0eu, 0x1641a27u, 0xc312db1u, 0x963a1fau, 0xc61d772u, 0x8664f05u, 0xfbea87cu, 0xfd7d963u, 0x6678a94u, 0x000478au},
        {0x6673449u, 0x24fffa7u, 0x7750b81u, 0x4830e2du, 0xe570d0eu, 0x1641a27u, 0xc312db1u, 0x963a1fau, 0xc61d772u, 0x8664f05u, 0xfbea87cu, 0xfd7d963u, 0x6678a94u, 0x000478au}};
    static constexpr uint32_t YD1[2][14] = {{0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u},
        {0xb336f7au, 0x91fffd3u, 0x5ba859du, 0x2417ca1u, 0xa3d95ddu, 0xdb9c29bu, 0x5cc2f41u, 0xc4df993u, 0x06c917bu, 0xe908e3eu, 0xdb32f5fu, 0x720bf0au, 0xc28e20au, 0x000f3cdu}};
    static constexpr uint32_t YD2[2][14] = {{0xb10c4efu, 0x3300003u, 0x43074a3u, 0xe7a7984u, 0xd98f7bcu, 0x5e808ffu, 0x5afa4bfu, 0x7a86ed8u, 0x1050824u, 0x6ba4a08u, 0x8922945u, 0x6154ea8u, 0xc951d14u, 0x0014667u},
        {0x4eee5bcu, 0xcbffffcu, 0xfcf8b16u, 0x1857190u, 0x88b26efu, 0x427620fu, 0x9b78c13u, 0x78fe253u, 0x3724360u, 0xe00836eu, 0x3158cfdu, 0x8545609u, 0x5551c6bu, 0x00059a9u}};
    static constexpr uint32_t PSI_CX[2][14] = {{0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u, 0x0000000u},
        {0x58a1811u, 0x96e4867u, 0x1d5c11cu, 0x543e856u, 0x13e6366u, 0x4b0fc91u, 0xae5efbbu, 0x8680210u, 0x9941307u, 0xf700269u, 0xb02eef7u, 0x9086bfcu, 0x6855919u, 0x001291eu}};
    static constexpr uint32_t PSI_CY[2][14] = {{0xcc17b84u, 0xcc5da55u, 0x1835de7u, 0x3e1e677u, 0x9e4ae31u, 0x9b9a07au, 0xd662557u, 0xb7f1997u, 0x71cc4dau, 0xa667f92u, 0x65115feu, 0x4a3370cu, 0xe5b746au, 0x000d16du},
        {0x33e2f27u, 0x32a25aau, 0x27ca1d2u, 0xc1e049eu, 0xc3f707au, 0x055ca94u, 0x2010b7bu, 0x3b93794u, 0xd5a86aau, 0xa544de3u, 0x556a044u, 0x9c66da5u, 0x38ec515u, 0x000cea3u}};
    static constexpr uint32_t PSI2_K[14] = {0x2421b59u, 0xbee4867u, 0x1d31002u, 0x4760184u, 0x4cc5086u, 0xc76dc00u, 0xaae891bu, 0xac70ad2u, 0xfe377c4u, 0xe4686b8u, 0x5ed1568u, 0x8f5a180u, 0x02b5c1fu, 0x000d1a4u};
};
// the public scalars walked bit by bit: |z| (64 bits, weight 6) and the order r of G2 (255 bits)
__device__ const uint32_t G2H_Z_ABS[2] = {0x00010000u, 0xd2010000u};
__device__ const uint32_t G2H_R[8] = {0x00000001u, 0xffffffffu, 0xfffe5bfeu, 0x53bda402u, 0x09a1d805u, 0x3339d808u, 0x299d7d48u, 0x73eda753u};

DR_DEV Fq2 g2h_p18() { return {Fq28::constant<G1hConsts::P18>(), Fq28::constant<G1hConsts::P18>()}; }
DR_DEV Fq2 g2h_b() { return {Fq28::constant<Fq28Params::FOUR>(), Fq28::constant<Fq28Params::FOUR>()}; }       // 4 (1 + i)
// 8 a: n -> c8.2 (limbs x 8 below 2^31 after the inner carry)
DR_DEV Fq2 g2h_mul8(const Fq2& a) { return {carry(dbl(g1h_mul4(a.c0))), carry(dbl(g1h_mul4(a.c1)))}; }
// a carried value in (-2.1 p, 1.1 p) -> (-0.1 p, 1.1 p): two folds a component
DR_DEV Fq2 g2h_fold2(const Fq2& a) { return {fq_fold(fq_fold(a.c0)), fq_fold(fq_fold(a.c1))}; }

DR_DEV G2hPoint g2h_identity() { return {Fq2::zero(), Fq2::one(), Fq2::zero()}; }
DR_DEV G2hPoint g2h_from_affine(const Fq2& x, const Fq2& y) { return {x, y, Fq2::one()}; }
DR_DEV G2hPoint g2h_neg(const G2hPoint& p) { return {p.x, carry(neg(p.y)), p.z}; }
DR_DEV G2hPoint g2h_select(bool c, const G2hPoint& a, const G2hPoint& b) { return {select(c, a.x, b.x), select(c, a.y, b.y), select(c, a.z, b.z)}; }

// algorithm 9, a = 0: 2 squarings, 4 products and one fused sum of two (16 reductions); coordinates c3 in; X, Z n and Y c2.1 out
DR_DEV G2hPoint g2h_dbl(const G2hPoint& p) {
    const Fq2 t0 = sqr(p.y);                                                     // Y^2: n (4 x 3^2 = 36)
    const Fq2 z8 = g2h_mul8(t0);                                                 // 8 Y^2: c8.2
    const Fq2 t1 = mul(p.y, p.z);                                                // n (2 x 3 x 3 = 18)
    const Fq2 t2 = mul_b3(sqr(p.z));                                             // b3 Z^2: components in (-0.5 p, 12.5 p)
    const Fq2 y3a = carry(add(t0, t2));                                          // Y^2 + b3 Z^2: (-0.6 p, 13.6 p), c13.6
    // Y^2 - 3 b3 Z^2 lies in (-37.6 p, 2.6 p); + 18 p: (-19.6 p, 20.6 p), limbs before the carry in (-3 x 2^28, 2^29): c20.6
    const Fq2 t0b = carry(add(sub(t0, add(t2, dbl(t2))), g2h_p18()));
    G2hPoint r;
    r.x = mul(t0b, carry(dbl(mul(p.x, p.y))));                                   // 2 (Y^2 - 3 b3 Z^2) X Y: 2 x 20.6 x 2.1 = 87
    r.y = mul_add(t0b, y3a, t2, z8);                                             // rows: 20.6 x 13.6 + 12.5 x 8.2 = 383; 561 and 205
    r.z = mul(t1, z8);                                                           // 8 Y^3 Z: 2 x 1.1 x 8.2 = 18
    return r;
}

// algorithm 7, a = 0: 6 products and 3 fused sums of two (24 reductions); coordinates c3 in, c2.1 out
DR_DEV G2hPoint g2h_add(const G2hPoint& p, const G2hPoint& q) {
    const Fq2 t0 = mul(p.x, q.x), t1 = mul(p.y, q.y), t2 = mul(p.z, q.z);                          // n (18 each)
    // (X1 + Y1) (X2 + Y2): c6 x c6 (72) = n; minus two n: (-2.1 p, 1.1 p), c2.1
    const Fq2 t3 = carry(sub(mul(carry(add(p.x, p.y)), carry(add(q.x, q.y))), add(t0, t1)));      // X1 Y2 + X2 Y1
    const Fq2 t4 = carry(sub(mul(carry(add(p.y, p.z)), carry(add(q.y, q.z))), add(t1, t2)));      // Y1 Z2 + Y2 Z1
    const Fq2 xz = carry(sub(mul(carry(add(p.x, p.z)), carry(add(q.x, q.z))), add(t0, t2)));      // X1 Z2 + X2 Z1
    const Fq2 y3 = mul_b3(g2h_fold2(xz));                                                          // b3 (...): c14.4
    const Fq2 t0b = carry(add(t0, dbl(t0)));                                                       // 3 X1 X2: c3.1
    const Fq2 t2b = mul_b3(t2);                                                                    // b3 Z1 Z2: (-0.5 p, 12.5 p)
    const Fq2 z3 = carry(add(t1, t2b)), t1b = carry(sub(t1, t2b));                                 // c13.6, c12.6
    G2hPoint r;
    r.x = mul_add(t3, t1b, neg(t4), y3);                                                           // rows: 2.1 x 12.6 + 2.1 x 14.4 = 57; 53 and 61
    r.y = mul_add(t1b, z3, y3, t0b);                                                               // rows: 12.6 x 13.6 + 14.4 x 3.1 = 216; 343 and 90
    r.z = mul_add(z3, t4, t0b, t3);                                                                // rows: 13.6 x 2.1 + 3.1 x 2.1 = 36; 58 and 14
    return r;
}

// k P for a PUBLIC constant k by its bits, high to low: bit_length(k) - 1 doublings and popcount(k) - 1 additions; every lane takes the
// same (scalar) branches
template <int WORDS>
DR_DEV G2hPoint g2h_mul_public(const G2hPoint& P, const uint32_t (&k)[WORDS], int top_bit) {
    G2hPoint acc = P;
#pragma unroll 1
    for (int b = top_bit - 1; b >= 0; b--) {
        acc = g2h_dbl(acc);
        if ((k[b >> 5] >> (b & 31)) & 1u) acc = g2h_add(acc, P);
    }
    return acc;
}

// psi (x, y) = (conj(x) cx, conj(y) cy), the untwist-Frobenius-twist endomorphism, on projective coordinates (conjugation is a field
// automorphism, so Z is conjugated too), and psi^2 (x, y) = (x 2^-((p - 1) / 3), -y)
DR_DEV G2hPoint g2h_psi(const G2hPoint& p) {
    return {mul(conj(p.x), Fq2::constant<G2hConsts::PSI_CX>()), mul(conj(p.y), Fq2::constant<G2hConsts::PSI_CY>()), carry(conj(p.z))};
}
DR_DEV G2hPoint g2h_psi2(const G2hPoint& p) { return {mul_fq(p.x, Fq28::constant<G2hConsts::PSI2_K>()), carry(neg(p.y)), p.z}; }

DR_DEV void g2h_store_limbs(int32_t* o, const Fq28& a) {
#pragma unroll
    for (int t = 0; t < L28; t++) o[t] = a.l[t];
}
DR_DEV Fq28 g2h_load_limbs14(const int32_t* o) {
    Fq28 a;
#pragma unroll
    for (int t = 0; t < L28; t++) a.l[t] = o[t];
    return a;
}
// a projective point <-> its six 14-limb images (x.c0, x.c1, y.c0, y.c1, z.c0, z.c1): the form points take in the stage buffer
DR_DEV void g2h_store_limbs(int32_t* o, const G2hPoint& p) {
    g2h_store_limbs(o, p.x.c0); g2h_store_limbs(o + L28, p.x.c1);
    g2h_store_limbs(o + 2 * L28, p.y.c0); g2h_store_limbs(o + 3 * L28, p.y.c1);
    g2h_store_limbs(o + 4 * L28, p.z.c0); g2h_store_limbs(o + 5 * L28, p.z.c1);
}
DR_DEV G2hPoint g2h_load_limbs(const int32_t* o) {
    return {{g2h_load_limbs14(o), g2h_load_limbs14(o + L28)},
            {g2h_load_limbs14(o + 2 * L28), g2h_load_limbs14(o + 3 * L28)},
            {g2h_load_limbs14(o + 4 * L28), g2h_load_limbs14(o + 5 * L28)}};
}

// RFC 9380 appendix G.3 with c1 = z = -|z|:  [z^2 - z - 1] P + [z - 1] psi(P) + psi^2(2 P)  =  S + |z| T  for  A = |z| P,  T = A - psi(P)
// (minus the RFC's t2 after step 6) and  S = T + psi^2(2 P) - P.  This equals [h_eff] P on all of E(Fq2).  Two walks over the 64 bits of
// |z| (63 doublings and 5 additions each), one more doubling and four additions.  No more than two points and one addition's
// intermediates are live at any time: P, and later S, wait in `park` (this lane's own 84 words of the stage buffer) and are loaded when
// they are next needed; the empty asm statements keep the compiler from holding the parked values in registers instead.
DR_DEV G2hPoint g2h_clear_cofactor(const G2hPoint& P, int32_t* park) {
    g2h_store_limbs(park, P);
    const G2hPoint A = g2h_mul_public(P, G2H_Z_ABS, 63);
    const G2hPoint T = g2h_add(A, g2h_neg(g2h_psi(P)));
    asm volatile("" ::: "memory");
    {
        const G2hPoint P2 = g2h_load_limbs(park);
        const G2hPoint U = g2h_add(g2h_psi2(g2h_dbl(P2)), g2h_neg(P2));                            // psi^2(2 P) - P
        g2h_store_limbs(park, g2h_add(T, U));                                                      // S
    }
    asm volatile("" ::: "memory");
    const G2hPoint C = g2h_mul_public(T, G2H_Z_ABS, 63);
    asm volatile("" ::: "memory");
    return g2h_add(g2h_load_limbs(park), C);
}

// ---------------------------------------------------------------- simplified SWU onto E' (RFC 9380 6.6.2, appendix F.2's shape)
// 240 i x = -240 x1 + 240 x0 i and 1012 (1 + i) x = 1012 (x0 - x1) + 1012 (x0 + x1) i: one Fq product a component.  x: components cK
// (or negated), K < 16: the sums are below 32 p and the products below 32 p^2.  n out.
DR_DEV Fq2 g2h_mul_a(const Fq2& x) {
    const Fq28 k = Fq28::constant<G2hConsts::K240>();
    return {mul(neg(x.c1), k), mul(x.c0, k)};
}
DR_DEV Fq2 g2h_mul_b(const Fq2& x) {
    const Fq28 k = Fq28::constant<G2hConsts::K1012>();
    return {mul(carry(sub(x.c0, x.c1)), k), mul(carry(add(x.c0, x.c1)), k)};
}
// In: u (components n, canonical value) and sgn0(u).  Out: the point (xn / xd, y) of E', xd != 0, sgn0(y) = sgn0(u).  With x1 = tv3 / tv4
// and g(x1) = N / D, D = tv4^3:  g(x1) is a square iff w = N D is, and then y1 = sqrt(w) / D;  otherwise x2 = Z u^2 x1, g(x2) = (Z u^2)^3
// g(x1), and y2 = sqrt((Z u^2)^3 w) / D.  The root of the norm that fq2_sqrt_with needs comes from the ONE chain that decided
// squareness: for a non-square, s1^2 = -norm(w), and norm((Z u^2)^3) = (5 norm(u)^2)^3, so s2 = s1 norm(Z u^2) norm(u) sqrt(-5) squares
// to norm((Z u^2)^3 w).  Two exponentiations (the norm's, the root's) and two inversions (the root's division, D) per element.  The
// exceptional case tv2 = 0 is u = 0 alone (-1 / Z is a non-square): xd = A Z, x1 = B / (Z A), whose g is a square by the choice of Z.
DR_DEV void g2h_sswu_map(const Fq2& u, bool u_sgn, Fq2& xn, Fq2& xd, Fq2& y) {
    const Fq2 u2 = sqr(u);                                                                        // n
    // Z u^2 = -(2 + i) (x0 + x1 i) = (x1 - 2 x0) - (x0 + 2 x1) i: components in (-2.1 p, 1.1 p) and (-3.1 p, 0.1 p), c3.1
    const Fq2 tv1 = {carry(sub(u2.c1, dbl(u2.c0))), carry(neg(add(u2.c0, dbl(u2.c1))))};
    const Fq2 tv1sq = sqr(tv1);                                                                   // n (4 x 3.1^2 = 39)
    const Fq2 tv2 = carry(add(tv1sq, tv1));                                                       // Z^2 u^4 + Z u^2: c4.2
    const Fq2 tv3 = g2h_mul_b(add(tv2, Fq2::one()));                                              // B (tv2 + 1): sums below 10.5 p; n
    const Fq2 tv4 = g2h_mul_a(select(is_zero(tv2), Fq2::constant<G2hConsts::Z>(), neg(tv2)));     // A Z or -A tv2; n
    const Fq2 tv6 = sqr(tv4);
    const Fq2 D = mul(tv6, tv4);                                                                  // tv4^3: the denominator of g(x1)
    const Fq2 N = carry(add(mul(carry(add(sqr(tv3), g2h_mul_a(tv6))), tv3), g2h_mul_b(D)));       // tv3^3 + A tv3 tv4^2 + B tv4^3: c2.1
    const Fq2 w = mul(N, D);
    Fq28 s1;
    const bool is_square = fq2_norm_root(w, s1);
    const Fq2 w2 = mul(mul(tv1sq, tv1), w);                                                       // (Z u^2)^3 w
    const Fq28 s2 = mul(mul(s1, mul(norm(tv1), norm(u))), Fq28::constant<G2hConsts::SQRT_NEG5>());
    const Fq2 root = fq2_sqrt_with(select(is_square, w, w2), select(is_square, s1, s2));
    const Fq2 y1 = mul(root, inv(D));
    xn = select(is_square, tv3, mul(tv1, tv3));
    xd = tv4;
    y = carry(cneg(y1, sgn0(y1) != u_sgn));                                                       // sgn0(y) = sgn0(u); c1.1
}

// The 3-isogeny E' -> E (appendix E.3) on (xn / xd, y): four Horner evaluations in xn side by side, step j sharing the homogenising
// factor xd^j, each step one mul_add:  N <- N xn + k xd^j.  Then, as g1h_iso_map,  (X : Y : Z) = (XN YD : y YN xd XD : xd XD YD).  xn,
// xd: n; y: c1.1; every accumulator c2.1.  ok = false when a denominator vanishes — which NO input reaches: both roots of the x
// denominator and the third root of the y denominator lie in Fq2, and g is a non-square at each, so none is the x of a point of
// E'(Fq2) (tests/test_bls12_381_g2_cpu.py).  The flag stays; it costs one is_zero.
DR_DEV G2hPoint g2h_iso_map(const Fq2& xn, const Fq2& xd, const Fq2& y, bool& ok) {
    using K = G2hConsts;
    const Fq2 d2 = sqr(xd), d3 = mul(d2, xd);
    Fq2 XN = mul_add(Fq2::constant<K::XN3>(), xn, Fq2::constant<K::XN2>(), xd);
    XN = mul_add(XN, xn, Fq2::constant<K::XN1>(), d2);
    XN = mul_add(XN, xn, Fq2::constant<K::XN0>(), d3);
    Fq2 XD = carry(add(xn, mul(Fq2::constant<K::XD1>(), xd)));
    XD = mul_add(XD, xn, Fq2::constant<K::XD0>(), d2);
    Fq2 YN = mul_add(Fq2::constant<K::YN3>(), xn, Fq2::constant<K::YN2>(), xd);
    YN = mul_add(YN, xn, Fq2::constant<K::YN1>(), d2);
    YN = mul_add(YN, xn, Fq2::constant<K::YN0>(), d3);
    Fq2 YD = carry(add(xn, mul(Fq2::constant<K::YD2>(), xd)));
    YD = mul_add(YD, xn, Fq2::constant<K::YD1>(), d2);
    YD = mul_add(YD, xn, Fq2::constant<K::YD0>(), d3);
    const Fq2 dx = mul(xd, XD);
    G2hPoint r;
    r.x = mul(XN, YD);
    r.y = mul(mul(y, YN), dx);
    r.z = mul(dx, YD);
    ok = !is_zero(r.z);
    return r;
}

// ---------------------------------------------------------------- memory forms
DR_DEV Fq2 g2h_load_fq2(const uint32_t* p, bool& sgn, uint32_t& any) {            // 24 canonical words c0 || c1; sgn0 and an OR of all words
    uint32_t w0[12], w1[12], any0 = 0, any1 = 0;
    load_words12(p, w0);
    load_words12(p + 12, w1);
#pragma unroll
    for (int j = 0; j < 12; j++) { any0 |= w0[j]; any1 |= w1[j]; }
    sgn = ((w0[0] & 1u) | ((any0 == 0 ? 1u : 0u) & (w1[0] & 1u))) != 0;
    any = any0 | any1;
    return {to_mont28(w0), to_mont28(w1)};
}
DR_DEV void g2h_store_fq2(uint32_t* p, const Fq2& a) {
    uint32_t w[12];
    from_mont28(a.c0, w); store_words12(p, w);
    from_mont28(a.c1, w); store_words12(p + 12, w);
}
DR_DEV void g2h_store_affine(uint32_t* out, const G2hPoint& acc) {               // x || y, 48 words; Z = 0 stores 192 zero bytes (0^-1 = 0)
    const Fq2 zi = inv(acc.z);
    g2h_store_fq2(out, mul(acc.x, zi));
    g2h_store_fq2(out + 24, mul(acc.y, zi));
}
// a point of the ABI: 48 words; all zero: the identity
DR_DEV G2hPoint g2h_load_affine(const uint32_t* p, bool& identity) {
    bool sx, sy;
    uint32_t ax, ay;
    const Fq2 x = g2h_load_fq2(p, sx, ax), y = g2h_load_fq2(p + 24, sy, ay);
    identity = (ax | ay) == 0;
    return g2h_select(identity, g2h_identity(), g2h_from_affine(x, y));
}

// ---------------------------------------------------------------- kernels
// stage[e] = the projective image on E of field element e (84 limbs), ok_e[e] = 0 where an isogeny denominator vanished.  us: n_elems x
// 24 canonical words (checked by the host).  One lane per element; two exponentiations and two inversions each.
__global__ __launch_bounds__(G2H_BLOCK) void k_blsg2_map_iso(const uint32_t* __restrict__ us, int32_t* __restrict__ stage,
                                                             uint32_t* __restrict__ ok_e, uint32_t n_elems) {
    uint32_t e = blockIdx.x * G2H_BLOCK + threadIdx.x;
    const bool live = e < n_elems;
    if (!live) e = n_elems - 1;      // keep the wave converged; the duplicate result is not stored
    bool u_sgn, ok;
    uint32_t any;
    const Fq2 u = g2h_load_fq2(us + (size_t)e * 24, u_sgn, any);
    Fq2 xn, xd, y;
    g2h_sswu_map(u, u_sgn, xn, xd, y);
    const G2hPoint pt = g2h_iso_map(xn, xd, y, ok);
    if (live) {
        g2h_store_limbs(stage + (size_t)e * G2H_STAGE_WORDS, pt);
        ok_e[e] = ok ? 1u : 0u;
    }
}
// out[i] = the sum of item i's `per_item` (1 or 2) staged images, cleared by psi if `clear`; out: n x 48 words affine x || y (zeros: the
// identity), ok[i] = the AND of its elements' flags.  clear = 0 is the reference's map_to_curve_simple_swu (the Q0 / Q1 of the RFC's
// vectors, per_item = 1) or Q0 + Q1.  One lane per item, one inversion each.  The stage buffer is read, and with `clear` element
// i * per_item's slot is overwritten (P, then the running sum, parked there).
__global__ __launch_bounds__(G2H_BLOCK) void k_blsg2_sum_clear(int32_t* __restrict__ stage, const uint32_t* __restrict__ ok_e,
                                                               uint32_t* __restrict__ out_xy, uint32_t* __restrict__ ok, uint32_t n,
                                                               uint32_t per_item, uint32_t clear) {
    const uint32_t i = blockIdx.x * G2H_BLOCK + threadIdx.x;
    if (i >= n) return;              // no wave-level operation below: a tail lane may leave
    int32_t* slot = stage + (size_t)i * per_item * G2H_STAGE_WORDS;
    G2hPoint acc = g2h_load_limbs(slot);
    uint32_t good = ok_e[(size_t)i * per_item];
    if (per_item == 2) {
        acc = g2h_add(acc, g2h_load_limbs(slot + G2H_STAGE_WORDS));
        good &= ok_e[(size_t)i * 2 + 1];
    }
    if (clear) acc = g2h_clear_cofactor(acc, slot);
    g2h_store_affine(out_xy + (size_t)i * 48, acc);
    ok[i] = good;
}

// out[i] = k[i] P[i] for any point of E(Fq2) and a 768-bit scalar (24 words little-endian, used AS IT IS: #E(Fq2) = h2 r is 762 bits and
// a point need not lie in G2).  A plain left-to-right walk on the complete law — wave_curve.hip.h's LDS window table would need 8 x 3 x
// 28 x 64 x 4 = 172 032 bytes, more than the 163 840 there are — over the scalar's bits read from memory (an array indexed by the loop
// counter would go to scratch), starting at the top set bit of the WAVE's largest scalar.  Scalars here are public (there is no VRF over
// this curve): the addition is skipped where no lane of the wave has the bit, by a wave-uniform branch.
__global__ __launch_bounds__(G2H_BLOCK) void k_blsg2_scalar_mul(const uint32_t* __restrict__ pts, const uint32_t* __restrict__ ks,
                                                                uint32_t* __restrict__ out, uint32_t n) {
    uint32_t i = blockIdx.x * G2H_BLOCK + threadIdx.x;
    const bool live = i < n;
    if (!live) i = n - 1;            // keep the wave converged (the shuffles and the ballot below); the duplicate result is not stored
    const uint32_t* k = ks + (size_t)i * 24;
    int top = -1;
#pragma unroll
    for (int j = 0; j < 24; j++) {
        const uint32_t w = k[j];
        if (w) top = 32 * j + 31 - __clz((int)w);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) top = max(top, __shfl_xor(top, off));
    top = __builtin_amdgcn_readfirstlane(top);
    G2hPoint acc = g2h_identity();
#pragma unroll 1
    for (int b = top; b >= 0; b--) {
        acc = g2h_dbl(acc);
        const bool bit = ((k[b >> 5] >> (b & 31)) & 1u) != 0;
        if (__builtin_amdgcn_ballot_w64(bit) != 0) {
            // the complete law adds the identity where the lane's bit is clear.  P is loaded again for every addition (four Montgomery
            // conversions, 7 % of an addition) so that the walk holds one point, not two, between additions: with P in registers the
            // kernel spilled
            asm volatile("" ::: "memory");
            bool identity;
            const G2hPoint P = g2h_load_affine(pts + (size_t)i * 48, identity);
            acc = g2h_add(acc, g2h_select(bit, P, g2h_identity()));
        }
    }
    if (live) g2h_store_affine(out + (size_t)i * 48, acc);
}

// ok[i] = whether point i (48 canonical words, checked by the host; all zero: the identity, which passes both modes) satisfies y^2 = x^3 +
// 4 (1 + i), and with MODE = G2H_CHECK_SUBGROUP also r P = O by the bits of the public r (254 doublings, 127 additions)
enum { G2H_CHECK_CURVE = 0, G2H_CHECK_SUBGROUP = 1 };
template <int MODE>
__global__ __launch_bounds__(G2H_BLOCK) void k_blsg2_check_points(const uint32_t* __restrict__ pts, uint32_t* __restrict__ ok, uint32_t n) {
    const uint32_t i = blockIdx.x * G2H_BLOCK + threadIdx.x;
    if (i >= n) return;
    bool identity;
    const G2hPoint P = g2h_load_affine(pts + (size_t)i * 48, identity);
    // x^3 + b: n + n, c2.1; for the identity (0 : 1 : 0) the flag decides
    bool good = identity || equal(sqr(P.y), carry(add(mul(sqr(P.x), P.x), g2h_b())));
    if constexpr (MODE == G2H_CHECK_SUBGROUP) good = good && is_zero(g2h_mul_public(P, G2H_R, 254).z);
    ok[i] = good ? 1u : 0u;
}

// Diagnostic (dr_blsg2_field_selftest): fq2_28.hip.h and what this file adds to it, on raw limb images, one lane per (a, b) pair of 2 x 14
// int32 limbs each (c0 then c1), so that tests can drive it at the limb bounds the map and the law feed.  out[i] = five records of 24
// words (c0 || c1), each the canonical standard-form value of the result: a b; a^2; a^-1 (0 for 0); b3 a as the addition computes it
// (two folds, then mul_b3: a's components in (-2.1 p, 1.1 p)); a root of a if it is a square, else 0.  flags[i]: bit 0 a is a square, bit
// 1 sgn0(a), bit 2 a is zero.
constexpr int G2H_SELFTEST_RECORDS = 5;
__global__ __launch_bounds__(64) void k_blsg2_field_selftest(const int32_t* __restrict__ a_limbs, const int32_t* __restrict__ b_limbs, uint32_t n,
                                                            uint32_t* __restrict__ out, uint32_t* __restrict__ flags) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    Fq2 a, b;
#pragma unroll
    for (int t = 0; t < L28; t++) {
        a.c0.l[t] = a_limbs[(size_t)i * 2 * L28 + t]; a.c1.l[t] = a_limbs[(size_t)i * 2 * L28 + L28 + t];
        b.c0.l[t] = b_limbs[(size_t)i * 2 * L28 + t]; b.c1.l[t] = b_limbs[(size_t)i * 2 * L28 + L28 + t];
    }
    uint32_t* o = out + (size_t)i * G2H_SELFTEST_RECORDS * 24;
    g2h_store_fq2(o, mul(a, b));
    g2h_store_fq2(o + 24, sqr(a));
    g2h_store_fq2(o + 48, inv(a));
    g2h_store_fq2(o + 72, mul_b3(g2h_fold2(a)));
    Fq2 root;
    const bool sq = fq2_sqrt(a, root);
    g2h_store_fq2(o + 96, select(sq, root, Fq2::zero()));
    flags[i] = (sq ? 1u : 0u) | (sgn0(a) ? 2u : 0u) | (is_zero(a) ? 4u : 0u);
}

}  // namespace dr
