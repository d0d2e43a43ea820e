// Ed25519 kernels (DR_CURVE_ED25519; the reference's specs/ed25519.py, Ed25519_TAI variant): the twisted Edwards group law with
// a = -1 over GF(2^255 - 19) (fe25519.hip.h) and the kernels that fill, for this curve, the roles kernels_te.hip.h /
// kernels_bsn.hip.h fill for JubJub: variable-base scalar multiplication on a fixed schedule, grouped MSMs, point decoding and the
// device half of try-and-increment.  The existing kernels stay as they are; the Bandersnatch / JubJub / SW code does not include
// this header's field.
//
// Points cross the ABI as x || y little-endian (standard form: this field has no Montgomery form).  Extended coordinates
// (X, Y, Z, T), x = X / Z, y = Y / Z, T = X Y / Z; dbl-2008-hwcd and add-2008-hwcd with a = -1, as curve.hip.h runs them for
// JubJub.  The comments give the limb bound of every intermediate against fe25519.hip.h's contract ("n" = normal).
#pragma once
#include "fe25519.hip.h"
#include "wave_curve.hip.h"
#include "wave_msm.hip.h"

namespace dr {

constexpr int ED_BLOCK = 64;          // one wave per workgroup; 64 KiB of LDS table per wave (X, Y, Z, T x 8 words), as k_bsn_scalar_mul

struct EdPoint {
    F25 x, y, z, t;
};

DR_DEV EdPoint ed_identity() {
    EdPoint p;
    p.x = F25::zero(); p.y = F25::small(1); p.z = F25::small(1); p.t = F25::zero();
    return p;
}

// dbl-2008-hwcd, a = -1.  WITH_T = false skips T3 (the result is only doubled again).  Coordinates n (x and t possibly negated by
// ed_cneg: every operand below is a square or a product, which take a negated normal as they take a normal) in, n out: every coordinate
// is a product (T = 0 without it)
template <bool WITH_T>
DR_DEV EdPoint ed_dbl(const EdPoint& p) {
    const F25 A = sqr(p.x), B = sqr(p.y);                   // n
    const F25 C = dbl(sqr(p.z));                            // < 2^30.01
    const F25 E = carry(dbl(mul(p.x, p.y)));                // 2 x y: n
    const F25 G = sub(B, A);                                // D + B with D = a A = -A: < 2^29.01
    const F25 F = carry(sub(G, C));                         // n
    const F25 H = neg(add(A, B));                           // D - B: < 2^30.01
    EdPoint r;
    r.x = mul(E, F);
    r.y = mul(G, H);
    r.z = mul(F, G);
    if (WITH_T) r.t = mul(E, H);
    else r.t = F25::zero();
    return r;
}

// add-2008-hwcd, a = -1, unified (also right for doubling and the identity).  dt2 = d T2 (the caller's constant or table value).
// Coordinates n (x and t possibly negated by ed_cneg, in either point) in, n out: every coordinate is a product
DR_DEV EdPoint ed_add_dt(const EdPoint& p, const EdPoint& q, const F25& dt2) {
    const F25 A = mul(p.x, q.x), B = mul(p.y, q.y);          // n
    const F25 C = mul(p.t, dt2);                            // n
    const F25 D = mul(p.z, q.z);                            // n
    const F25 E = mul2(p.x, q.y, p.y, q.x);                 // n (operands n or negated n: below 2^29.45)
    const F25 F = sub(D, C), G = add(D, C);                 // < 2^29.01, < 2^30.01
    const F25 H = carry(add(B, A));                         // B - a A: n
    EdPoint r;
    r.x = mul(E, F);
    r.y = mul(G, H);
    r.t = mul(E, H);
    r.z = mul(F, G);
    return r;
}
DR_DEV EdPoint ed_add(const EdPoint& p, const EdPoint& q) {
    return ed_add_dt(p, q, mul(F25::constant<Fe25519Consts::D>(), q.t));
}

DR_DEV EdPoint ed_cneg(const EdPoint& p, bool negate) {
    EdPoint r = p;
    r.x = cneg(p.x, negate);
    r.t = cneg(p.t, negate);
    return r;
}

// k mod l for a 256-bit k: floor((2^256 - 1) / l) = 15, so 16 conditional subtractions (the same count in every lane)
DR_DEV void ed_reduce_mod_order(uint32_t (&k)[8]) {
    constexpr uint32_t L[8] = {0x5cf5d3edu, 0x5812631au, 0xa2f79cd6u, 0x14def9deu, 0x00000000u, 0x00000000u, 0x00000000u, 0x10000000u};
#pragma unroll 1
    for (int it = 0; it < 16; it++) {
        uint32_t d[8], borrow = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) d[i] = subb(k[i], L[i], borrow);
#pragma unroll
        for (int i = 0; i < 8; i++) k[i] = borrow ? k[i] : d[i];
    }
}

// wave_curve.hip.h's description of Ed25519: canonical words at the ABI and in the LDS table, 64 windows (l < 2^253)
struct Ed25519Curve {
    using Fe = F25;
    using Point = EdPoint;
    static constexpr int WORDS = 8, SCALAR_WORDS = 8, BLOCK = ED_BLOCK, WINDOWS = 64, LDS_WORDS = 8;
    static constexpr bool EXTENDED = true, ZERO_IS_IDENTITY = false;
    DR_DEV static F25 unpack(const uint32_t (&w)[8]) { return fe_unpack(w); }
    DR_DEV static void pack(const F25& a, uint32_t (&w)[8]) { fe_pack(a, w); }
    DR_DEV static F25 inv(const F25& a) { return fe_inv(a); }
    DR_DEV static void to_lds(const F25& a, uint32_t (&w)[8]) { fe_pack(a, w); }
    DR_DEV static F25 from_lds(const uint32_t (&w)[8]) { return fe_unpack(w); }
    DR_DEV static EdPoint identity() { return ed_identity(); }
    DR_DEV static EdPoint from_affine(const F25& x, const F25& y) {
        EdPoint P;
        P.x = x; P.y = y; P.z = F25::small(1); P.t = mul(x, y);
        return P;
    }
    DR_DEV static EdPoint add(const EdPoint& p, const EdPoint& q) { return ed_add(p, q); }
    DR_DEV static EdPoint dbl(const EdPoint& p) { return ed_dbl<true>(p); }
    DR_DEV static EdPoint dbl_no_t(const EdPoint& p) { return ed_dbl<false>(p); }
    DR_DEV static EdPoint cneg(const EdPoint& p, bool negate) { return ed_cneg(p, negate); }
    DR_DEV static void load_scalar(const uint32_t* p, uint32_t (&k)[8]) {
        wave_load8(p, k);
        ed_reduce_mod_order(k);
    }
};

// out[i] = k[i] P[i]: wave_curve.hip.h's kernel bodies for this curve
__global__ __launch_bounds__(ED_BLOCK) void k_ed_scalar_mul(const uint32_t* __restrict__ pts, const uint32_t* __restrict__ ks,
                                                            uint32_t* __restrict__ out, uint32_t n) {
    wave_scalar_mul<Ed25519Curve>(pts, ks, out, n);
}
// out[g] = sum_{j<m} k[g m + j] P[g m + j]
__global__ __launch_bounds__(ED_BLOCK) void k_ed_msm_groups(const uint32_t* __restrict__ pts, const uint32_t* __restrict__ ks,
                                                            uint32_t* __restrict__ out, uint32_t groups, uint32_t m, uint32_t mpad) {
    wave_msm_groups<Ed25519Curve>(pts, ks, out, groups, m, mpad);
}
// the bucket method from NARROW_PIP_FROM terms on (wave_msm.hip.h): the stages over Ed25519Curve, set sums out as affine x || y
DR_WAVE_MSM_KERNELS(ed, Ed25519Curve)

// Decoding (the reference's point.py:150-214 with te_affine_point.py:297-316), one lane per 32-byte encoding: the sign is bit 255,
// y the low 255 bits, y >= p rejected; x^2 = (y^2 - 1) / (d y^2 + 1) (= (1 - y^2) / (a - d y^2) with a = -1), no root rejected;
// x is the larger of (x, p - x) iff the sign bit is set.  x = 0 (y = +-1) has both candidates 0, so the sign bit is ignored there,
// and the reference's constructor accepts (0, 1) and (0, -1).  MODE:
//   ED_DEC_CODEC  the codec alone: ok = decoded, out = (x, y)
//   ED_DEC_CHECK  also the prime-order check: Q = 8 P is not the identity and [8^-1 mod l] Q = P (a torsion component of P is
//                 killed by the 8 and does not come back) — the identity and all 8 torsion points are rejected
//   ED_DEC_TAI    the device half of try-and-increment (point.py:252-296, whose masking leaves the 32 squeezed bytes as they are for
//                 this curve): ok = decoded and 8 P is not the identity, out = 8 P
enum { ED_DEC_CODEC = 0, ED_DEC_CHECK = 1, ED_DEC_TAI = 2 };
template <int MODE>
__global__ __launch_bounds__(ED_BLOCK) void k_ed_decode_points(const uint32_t* __restrict__ enc /* n*8 */, uint32_t* __restrict__ out_xy /* n*16 */,
                                                               uint32_t* __restrict__ ok, uint32_t n) {
    __shared__ uint32_t tab[MODE == ED_DEC_CHECK ? wave_table_words<Ed25519Curve>() : 1];
    const int lane = threadIdx.x;
    uint32_t i = blockIdx.x * ED_BLOCK + lane;
    const bool live = i < n;
    if (!live) i = n - 1;
    uint32_t ys[8];
    wave_load8(enc + (size_t)i * 8, ys);
    const bool sign = (ys[7] >> 31) != 0;
    ys[7] &= 0x7fffffffu;
    bool valid;
    {   // y < p: y + 19 does not reach 2^255
        uint32_t c = 19u;
#pragma unroll
        for (int j = 0; j < 7; j++) c = (uint32_t)(((uint64_t)ys[j] + c) >> 32);
        valid = ys[7] + c < 0x80000000u;
    }
    const F25 one = F25::small(1);
    const F25 y = fe_unpack(ys);
    const F25 y2 = sqr(y);
    const F25 u = carry(sub(y2, one));
    const F25 v = carry(add(mul(F25::constant<Fe25519Consts::D>(), y2), one));
    F25 x;
    if (!fe_sqrt_ratio(u, v, x)) valid = false;       // (v = 0 never happens: -1 / d is not a square; u / 0 has no root here either)
    if (is_larger(x) != sign) x = neg(x);
    F25 ox = x, oy = y;
    if constexpr (MODE != ED_DEC_CODEC) {
        const EdPoint P = Ed25519Curve::from_affine(x, y);
        EdPoint Q = P;
#pragma unroll 1
        for (int j = 0; j < 3; j++) Q = ed_dbl<true>(Q);
        if (is_zero(Q.x)) { valid = false; Q = P; }  // 8 P = O (x = 0: 8 P lies in the prime-order subgroup, where only O has x = 0)
        const F25 zi = fe_inv(Q.z);
        const F25 qx = mul(Q.x, zi), qy = mul(Q.y, zi);
        if constexpr (MODE == ED_DEC_TAI) {
            ox = qx; oy = qy;
        } else {
            constexpr uint32_t HINV[8] = {0xe2dc2f79u, 0x6106e529u, 0x7d1cdad0u, 0x07d39db3u, 0x00000000u, 0x00000000u, 0x00000000u, 0x06000000u};
            uint32_t k[8];
#pragma unroll
            for (int j = 0; j < 8; j++) k[j] = HINV[j];
            const EdPoint R = wave_scalar_mul_core<Ed25519Curve>(tab, lane, Ed25519Curve::from_affine(qx, qy), k);
            if (!equal(R.x, mul(x, R.z)) || !equal(R.y, mul(y, R.z))) valid = false;
        }
    }
    if (!valid) { ox = F25::zero(); oy = F25::zero(); }
    if (live) {
        wave_store_fe<Ed25519Curve>(out_xy + (size_t)i * 16, ox);
        wave_store_fe<Ed25519Curve>(out_xy + (size_t)i * 16 + 8, oy);
        ok[i] = valid ? 1u : 0u;
    }
}

// ---------------------------------------------------------------- hashing to the curve (RFC 9380, edwards25519_XMD:SHA-512_ELL2_RO_ / _NU_)
// Elligator 2 onto curve25519 (v^2 = u^3 + A u^2 + u, A = 486662, Z = 2) as the reference's TECurve.map_to_curve_ell2 runs it, then its
// mont_to_ed25519, without an inversion per element.  With tv1 = Z u^2 (0 when it is -1; it never is, -1 / 2 is not a square) and
// d = 1 + tv1:  x1 = -A / d,  gx1 = x1^3 + A x1^2 + x1 = A (A^2 tv1 - d^2) / d^3 =: N / D,  x2 = -x1 - A = -A tv1 / d,  gx2 = tv1 gx1.
// One exponentiation decides the squareness of gx1 and gives the root of whichever is taken: b = N D^3 (N D^7)^((p - 5) / 8) has
// D b^2 = w N for a fourth root of unity w.  w = 1, -1: gx1 is a square with root b, b sqrt(-1).  w = i, -i (i = sqrt(-1), not a
// square, nor is Z = 2): gx2 = Z u^2 gx1 = u^2 b^2 (Z / w), root u b sqrt(-2 i), u b sqrt(2 i).  The sign is the reference's: the root
// negated when (gx1 is a square) xor (the root is odd).
struct Ed25519Ell2 {
    static constexpr uint32_t A[9] = {486662u, 0, 0, 0, 0, 0, 0, 0, 0};
    static constexpr uint32_t A2[9] = {0x04c21c24u, 0x000001b9u, 0, 0, 0, 0, 0, 0, 0};          // A^2
    // sqrt(-486664), the root the reference's mod_sqrt (Tonelli-Shanks from the non-residue 2) returns: the factor of mont_to_ed25519
    static constexpr uint32_t SQRT_NEG_A_MINUS_2[9] = {0x1f457e06u, 0x03702557u, 0x1f46a0b3u, 0x03a7a296u, 0x04f7ec5au, 0x046e01feu, 0x1aef49ecu, 0x1e8c1400u, 0x000f26edu};
    static constexpr uint32_t SQRT_NEG_2I[9] = {0x15f15f3eu, 0x188f26c5u, 0x1406e1ceu, 0x19cff2a5u, 0x02858d0bu, 0x1fb36102u, 0x03d352cbu, 0x0ff607c4u, 0x00547cdbu};
    static constexpr uint32_t SQRT_2I[9] = {0x0a0ea0b1u, 0x0770d93au, 0x0bf91e31u, 0x06300d5au, 0x1d7a72f4u, 0x004c9efdu, 0x1c2cad34u, 0x1009f83bu, 0x002b8324u};
};
// the image of u (normal, canonical) on Ed25519 in extended coordinates; ok = false where the reference's modular inverse fails: the
// Montgomery point has v = 0 (u = 0 reaches it) or u = -1, so that x = sqrt(-486664) u / v or y = (u - 1) / (u + 1) has no value (Z = 0)
DR_DEV EdPoint ed_ell2_map(const F25& u, bool& ok) {
    using K = Ed25519Ell2;
    const F25 one = F25::small(1), A = F25::constant<K::A>();
    F25 tv1 = carry(dbl(sqr(u)));                                            // Z u^2: n
    tv1 = select(is_zero(add(tv1, one)), F25::zero(), tv1);
    const F25 d = carry(add(tv1, one));                                      // n
    const F25 d2 = sqr(d);
    const F25 N = mul(A, sub(mul(F25::constant<K::A2>(), tv1), d2));         // A (A^2 tv1 - d^2): n x (n - n)
    const F25 D = mul(d2, d);
    // b = N D^3 (N D^7)^((p - 5) / 8), as fe_sqrt_ratio
    const F25 D2 = sqr(D);
    const F25 nd3 = mul(N, mul(D2, D));
    const F25 nd7 = mul(nd3, sqr(D2));
    F25 z11;
    const F25 b = mul(nd3, mul(sqr_n(fe_pow_2_250_1(nd7, z11), 2), nd7));
    const F25 vb2 = mul(D, sqr(b));
    const F25 iN = mul(N, F25::constant<Fe25519Consts::SQRT_M1>());
    const bool w_one = equal(vb2, N), w_neg = is_zero(add(vb2, N)), w_i = equal(vb2, iN);
    const bool e2 = w_one || w_neg;                                          // gx1 is a square (N != 0: A^2 - 4 is not a square)
    const F25 f = select(w_one, one, select(w_neg, F25::constant<Fe25519Consts::SQRT_M1>(),
                                            select(w_i, F25::constant<K::SQRT_NEG_2I>(), F25::constant<K::SQRT_2I>())));
    const F25 y1 = mul(b, f);
    F25 y = select(e2, y1, mul(y1, u));
    uint32_t yw[8];
    fe_pack(y, yw);
    y = carry(cneg(y, e2 != ((yw[0] & 1u) != 0)));
    const F25 xn = carry(neg(mul(A, select(e2, one, tv1))));                 // -A or -A tv1 over d: n
    // (u, v) = (xn / d, y) on curve25519 -> Ed25519: x = sqrt(-486664) u / v = a / bb, y = (u - 1) / (u + 1) = c / e
    const F25 a = mul(F25::constant<K::SQRT_NEG_A_MINUS_2>(), xn), bb = mul(d, y);
    const F25 c = carry(sub(xn, d)), e = carry(add(xn, d));
    EdPoint r;
    r.x = mul(a, e); r.y = mul(c, bb); r.z = mul(bb, e); r.t = mul(a, c);
    ok = !is_zero(r.z);
    return r;
}
// out[i] = 8 (the sum of the images of item i's `per_item` field elements) (2: the uniform (RO) encoding, 1: the nonuniform one): the
// reference's _e2c_ell2_ro / _e2c_ell2_nu after hash_to_field.  us: n x per_item x 8 words (canonical, checked by the host), out: n x 16
// words affine x || y, ok[i] = 0 where an image has no value (the output is then meaningless).  One lane per item; one exponentiation
// per element and one inversion per item.
__global__ __launch_bounds__(ED_BLOCK) void k_ed25519_map_to_curve(const uint32_t* __restrict__ us, uint32_t* __restrict__ out_xy,
                                                                   uint32_t* __restrict__ ok, uint32_t n, uint32_t per_item) {
    uint32_t i = blockIdx.x * ED_BLOCK + threadIdx.x;
    const bool live = i < n;
    if (!live) i = n - 1;
    EdPoint acc = ed_identity();
    bool good = true;
#pragma unroll 1
    for (uint32_t e = 0; e < per_item; e++) {
        bool ok_e;
        const EdPoint q = ed_ell2_map(wave_load_fe<Ed25519Curve>(us + ((size_t)i * per_item + e) * 8), ok_e);
        good = good && ok_e;
        acc = ed_add(acc, q);
    }
#pragma unroll 1
    for (int j = 0; j < 3; j++) acc = ed_dbl<true>(acc);                     // the cofactor
    if (live) {
        wave_store_affine<Ed25519Curve>(out_xy + (size_t)i * 16, acc);
        ok[i] = good ? 1u : 0u;
    }
}

// Diagnostic (dr_fe25519_ops_selftest): fe25519.hip.h's operations on raw limb images, one lane per (a, b) pair of 9 int32 limbs each,
// so that tests can drive every operation at the limb bounds its contract allows.  out[i] = eleven canonical 32-byte records:
// a b, a^2, a + b, a - b, -a, carry(a), a b + b a (mul2), a^-1 (0 for 0), sqrt(a) or 0, a itself (pack), sqrt(a / b) or 0;
// flags[i]: bit 0 a is a square, bit 1 a / b has a root (fe_sqrt_ratio), bit 2 a is the larger of (a, -a).
constexpr int FE_SELFTEST_RECORDS = 11;
__global__ __launch_bounds__(64) void k_fe25519_selftest(const int32_t* __restrict__ a_limbs, const int32_t* __restrict__ b_limbs, uint32_t n,
                                                         uint32_t* __restrict__ out, uint32_t* __restrict__ flags) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    F25 a, b;
#pragma unroll
    for (int t = 0; t < LIMBS29; t++) { a.l[t] = a_limbs[(size_t)i * LIMBS29 + t]; b.l[t] = b_limbs[(size_t)i * LIMBS29 + t]; }
    uint32_t* o = out + (size_t)i * FE_SELFTEST_RECORDS * 8;
    wave_store_fe<Ed25519Curve>(o + 0, mul(a, b));
    wave_store_fe<Ed25519Curve>(o + 8, sqr(a));
    wave_store_fe<Ed25519Curve>(o + 16, add(a, b));
    wave_store_fe<Ed25519Curve>(o + 24, sub(a, b));
    wave_store_fe<Ed25519Curve>(o + 32, neg(a));
    wave_store_fe<Ed25519Curve>(o + 40, carry(a));
    wave_store_fe<Ed25519Curve>(o + 48, mul2(a, b, b, a));
    wave_store_fe<Ed25519Curve>(o + 56, fe_inv(a));
    F25 r;
    const bool sq = fe_sqrt_ratio(a, F25::small(1), r);
    wave_store_fe<Ed25519Curve>(o + 64, r);
    wave_store_fe<Ed25519Curve>(o + 72, a);
    const bool rt = fe_sqrt_ratio(a, b, r);
    wave_store_fe<Ed25519Curve>(o + 80, r);
    flags[i] = (sq ? 1u : 0u) | (rt ? 2u : 0u) | (is_larger(a) ? 4u : 0u);
}

// Diagnostic (dr_ed25519_law_selftest): wave_curve.hip.h's wave_law_selftest over Ed25519Curve, the law on raw limb images
__global__ __launch_bounds__(64) void k_ed_law_selftest(const int32_t* __restrict__ pts, const uint32_t* __restrict__ ctl, uint32_t n, int32_t* __restrict__ out) {
    wave_law_selftest<Ed25519Curve>(pts, ctl, n, out);
}

}  // namespace dr
