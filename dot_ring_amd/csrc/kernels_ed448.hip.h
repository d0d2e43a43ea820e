// Ed448 kernels (DR_CURVE_ED448_RO / DR_CURVE_ED448_NU; the reference's specs/ed448.py): the Edwards curve x^2 + y^2 = 1 + d x^2 y^2 with
// a = 1 and d = -39081 over p = 2^448 - 2^224 - 1 (fe448.hip.h), cofactor 4.  d is a non-square, so the unified addition below is
// complete on all of E(F_p); the a = -1 formulas of kernels_ed25519.hip.h do not apply.  The kernels: scalar multiplication on a fixed
// schedule by 56-byte scalars taken AS THEY ARE (any k < 2^448: no reduction on the device, so small-order points and map(clear = 0) 4
// are well defined), grouped MSMs, RFC 9380's Elligator 2 onto curve448 with the reference's mont_to_ed448, a curve / subgroup check,
// and a diagnostic of the field.
//
// Points cross the ABI as affine x || y, 14 + 14 words little-endian, canonical; the identity is (0, 1) as itself.  A point is 112
// bytes, a multiple of 16, so it moves as seven uint4 with no padding; a 56-byte scalar moves as seven uint2.  Inside: PROJECTIVE
// (X : Y : Z), identity (0 : 1 : 1), add-2007-bl (10 M + 1 S + 1 small) and dbl-2007-bl (3 M + 4 S) with c = 1: a window of the
// schedule costs the same products as extended coordinates would (22 M + 17 S against 22 M + 16 S) with 48 live registers a point
// instead of 64 and three quarters of the LDS table.  The comments give the limb class of every intermediate against fe448.hip.h's
// contract ("n" = normal, "k n" = |limb| <= k normal; mul needs ka kb <= 3, sqr 1 n).
//
// The schedule, the memory forms and the two kernel bodies are wave_curve.hip.h's over Ed448Curve: 14 scalar words, 113 windows.
#pragma once
#include "e448_law.hip.h"
#include "wave_curve.hip.h"
#include "wave_msm.hip.h"

namespace dr {

constexpr int E448_BLOCK = 64;        // one wave per workgroup; 96 KiB of LDS table per wave (X, Y, Z x 16 limb words x 8 entries)
constexpr int E448_WINDOWS = 113;     // 112 nibbles of a 448-bit scalar and the carry out of the last digit
constexpr int E448_PT_WORDS = 2 * W448;

// the group order n = 2^446 - 0x8335dc163bb124b65129c96fde933d8d723a70aadc873d6d54a7bb0d, 14 words: the public scalar of the subgroup check.
__device__ const uint32_t E448_ORDER[W448] = {0xab5844f3u, 0x2378c292u, 0x8dc58f55u, 0x216cc272u, 0xaed63690u, 0xc44edb49u, 0x7cca23e9u,
                                              0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0x3fffffffu};

// (the law itself — E448Point, e448_identity, e448_from_affine, e448_is_identity, e448_dbl, e448_add, e448_cneg — is e448_law.hip.h's: the
// host runs it too, for the window combination of dr_wide_msm)

// wave_curve.hip.h's description of Ed448: canonical words at the ABI (14 per coordinate; the identity is (0, 1) as itself), the limb
// images in the LDS table (no packing), and 113 windows over the scalar AS IT IS: 112 nibbles of any k < 2^448 and the carry out of the
// last digit.  Z is never 0 (the law is complete), so the affine store needs nothing special.
struct Ed448Curve : Limb28Curve<Fe448Consts> {
    using Point = E448Point;
    static constexpr int SCALAR_WORDS = W448, BLOCK = E448_BLOCK, WINDOWS = E448_WINDOWS;
    static constexpr bool EXTENDED = false, ZERO_IS_IDENTITY = false;
    DR_DEV static F448 inv(const F448& a) { return dr::inv(a); }     // 1 n; stays here: Limb28Curve supplies no inv
    DR_DEV static E448Point identity() { return e448_identity(); }
    DR_DEV static E448Point from_affine(const F448& x, const F448& y) { return e448_from_affine(x, y); }
    DR_DEV static E448Point add(const E448Point& p, const E448Point& q) { return e448_add(p, q); }
    DR_DEV static E448Point dbl(const E448Point& p) { return e448_dbl(p); }
    DR_DEV static E448Point cneg(const E448Point& p, bool negate) { return e448_cneg(p, negate); }
    DR_DEV static void load_scalar(const uint32_t* p, uint32_t (&k)[W448]) { wave_load_words(p, k); }    // no reduction (head of the file)
};

// out[i] = k[i] P[i].  pts: n x 28 words (x || y), ks: n x 14, out: n x 28.  One lane per multiplication.
__global__ __launch_bounds__(E448_BLOCK) void k_ed448_scalar_mul(const uint32_t* __restrict__ pts, const uint32_t* __restrict__ ks,
                                                                 uint32_t* __restrict__ out, uint32_t n) {
    wave_scalar_mul<Ed448Curve>(pts, ks, out, n);
}
// out[g] = sum_{j<m} k[g m + j] P[g m + j], m <= 64 padded to mpad: one lane per term, folded with shuffles by the complete addition
__global__ __launch_bounds__(E448_BLOCK) void k_ed448_msm_groups(const uint32_t* __restrict__ pts, const uint32_t* __restrict__ ks,
                                                                 uint32_t* __restrict__ out, uint32_t groups, uint32_t m, uint32_t mpad) {
    wave_msm_groups<Ed448Curve>(pts, ks, out, groups, m, mpad);
}


// ---------------------------------------------------------------- the bucket method (dr_wide_msm): wave_msm.hip.h over Ed448Curve
// One MSM of n >= WIDE_PIP_FROM terms; the stages, their operands and the plan are that header's.  W448 scalar words, as they are; the
// set sums leave as records of limb images (k_ed448_msm_prepare, _sort, _accumulate, _accumulate_heavy, _reduce, _fold).
DR_WAVE_MSM_KERNELS_RECORDS(ed448, Ed448Curve)

// ---------------------------------------------------------------- hashing to the curve (RFC 9380, edwards448_XOF:SHAKE256_ELL2_RO_ / _NU_)
// Elligator 2 onto curve448 (v^2 = u^3 + A u^2 + u, A = 156326, Z = -1) as the reference's TECurve.map_to_curve_ell2 computes it, in the
// inversion-free shape of RFC 9380 appendix G.2.2 (p = 3 mod 4), with selects and no branch.  With tv1 = Z u^2 = -u^2 (taken as 0 when it
// is -1, that is u = +-1) and xd = 1 + tv1:  x1 = -A / xd,  gx1 = -A (A^2 (-tv1) + xd^2) / xd^3 =: g / gxd,  x2 = -x1 - A = A tv1' / xd
// (tv1' = -tv1 = u^2),  gx2 = -u^2 gx1.  One exponentiation: y1 = g gxd (g gxd^3)^((p - 3) / 4) has y1^2 gxd = +-g; + : gx1 is a
// square (e2) with root y1; - : gx2 = u^2 y1^2, root u y1.  The sign is the reference's: the root negated when e2 xor (its canonical
// value is odd).  Then the reference's mont_to_ed448 on (u, v) = (N / D, v), N = the x numerator, D = xd, with m = N^2 - D^2,
// w = m^2, q = 4 v^2 D^4:
//   x = 4 v m D^2 / (w + q)                       (x_num D^4 / x_den D^4)
//   y = -N (w - q) / (N w - 2 v^2 D^3 (N^2 + D^2)) (y_num D^5 / y_den D^5)
// kept as fractions: (X : Y : Z) = (XN YD : YN XD : XD YD), the inversion left to the item's affine store.  D = xd is never 0, so Z = 0
// exactly where x_den or y_den is: ok = false there, which only u in {0, 1, p - 1} reach (they land on the Montgomery point (0, 0),
// where y_den = 0; both quartics x_den and y_den / u have no root in F_p: tests/test_ed448_cpu.py).
DR_DEV E448Point e448_ell2_map(const F448& u /* n, canonical */, bool& ok) {
    constexpr int32_t A = Fe448Consts::MONT_A;
    const F448 one = F448::small(1);
    F448 u2 = sqr(u);                                                        // -tv1: n
    const bool e1 = equal(u2, one);                                          // Z u^2 = -1
    u2 = select(e1, F448::zero(), u2);
    const F448 xd = carry(add(one, neg(u2)));                                // 1 - u^2: n
    const F448 xd2 = sqr(xd);
    const F448 gxd = mul(xd2, xd);                                           // xd^3: n
    const F448 au2 = mul_small(u2, A);                                       // A u^2 (= x2n): n
    const F448 g = neg(mul_small(carry(add(mul_small(au2, A), xd2)), A));    // -A (A^2 u^2 + xd^2): 1 n
    const F448 t2 = mul(g, gxd);                                             // n
    const F448 t3 = mul(sqr(gxd), t2);                                       // g gxd^3: n
    const F448 y1 = mul(f448_pow_p34(t3), t2);                               // n
    const F448 y2 = select(e1, F448::zero(), mul(y1, u));                    // n
    const bool e2 = equal(mul(sqr(y1), gxd), g);
    const F448 N = select(e2, F448::small(-A), au2);                         // x1n = -A or x2n: 1 n
    F448 v = select(e2, y1, y2);
    v = cneg(v, e2 != is_odd(v));                                            // 1 n
    // mont_to_ed448
    const F448 n2 = sqr(N), d2 = sqr(xd), v2 = sqr(v);                       // n
    const F448 m = sub(n2, d2);                                              // 1 n
    const F448 w = sqr(m);                                                   // n
    const F448 vd = mul(v2, d2);                                             // v^2 D^2: n
    const F448 q = carry(dbl(dbl(mul(vd, d2))));                             // 4 v^2 D^4: n
    const F448 XD = carry(add(w, q));                                        // n
    const F448 YN = neg(mul(N, sub(w, q)));                                  // 1 n x 1 n; 1 n
    const F448 s = mul(mul(vd, xd), carry(add(n2, d2)));                     // v^2 D^3 (N^2 + D^2): n
    const F448 YD = carry(sub(mul(N, w), dbl(s)));                           // n
    const F448 XN = carry(dbl(dbl(mul(mul(v, m), d2))));                     // 4 v m D^2: (1 n x 1 n) x n, then n
    E448Point r;
    r.x = mul(XN, YD);
    r.y = mul(YN, XD);
    r.z = mul(XD, YD);
    ok = !is_zero(r.z);
    return r;
}
// out[i] = [4 if clear] (the sum of the images of item i's `per_item` field elements) (2: the uniform (RO) encoding, 1: the nonuniform
// one).  us: n x per_item x 14 words (canonical, checked by the host), out: n x 28 words affine x || y, ok[i] = 0 and 112 zero bytes where
// an image has no value.  clear = 0 is the reference's map_to_curve (per_item = 1: the Q0 / Q1 / Q of the RFC's vectors).  One lane per
// item; one exponentiation per element and one inversion per item.
__global__ __launch_bounds__(E448_BLOCK) void k_ed448_map_to_curve(const uint32_t* __restrict__ us, uint32_t* __restrict__ out_xy,
                                                                   uint32_t* __restrict__ ok, uint32_t n, uint32_t per_item, uint32_t clear) {
    uint32_t i = blockIdx.x * E448_BLOCK + threadIdx.x;
    const bool live = i < n;
    if (!live) i = n - 1;
    E448Point acc = e448_identity();
    bool good = true;
#pragma unroll 1
    for (uint32_t e = 0; e < per_item; e++) {
        uint32_t w[W448];
        wave_load_words(us + ((size_t)i * per_item + e) * W448, w);
        bool ok_e;
        const E448Point q = e448_ell2_map(unpack(w), ok_e);
        good = good && ok_e;
        acc = e448_add(acc, q);
    }
    if (clear) {
#pragma unroll 1
        for (int j = 0; j < 2; j++) acc = e448_dbl(acc);                     // the cofactor
    }
    if (live) {
        if (good) wave_store_affine<Ed448Curve>(out_xy + (size_t)i * E448_PT_WORDS, acc);
        else wave_store_zero_words<E448_PT_WORDS>(out_xy + (size_t)i * E448_PT_WORDS);
        ok[i] = good ? 1u : 0u;
    }
}

// One lane per 112-byte x || y.  CHECK = 0: both coordinates below p and the curve equation holds (the identity (0, 1) passes).
// CHECK = 1: additionally not the identity, and n P = O by the fixed schedule over the public words of n.  out = the input and ok = 1,
// or 112 zero bytes and ok = 0.
template <int CHECK>
__global__ __launch_bounds__(E448_BLOCK) void k_ed448_check_points(const uint32_t* __restrict__ enc, uint32_t* __restrict__ out_xy,
                                                                   uint32_t* __restrict__ ok, uint32_t n) {
    __shared__ uint32_t tab[CHECK ? wave_table_words<Ed448Curve>() : 1];
    const int lane = threadIdx.x;
    uint32_t i = blockIdx.x * E448_BLOCK + lane;
    const bool live = i < n;
    if (!live) i = n - 1;
    uint32_t xw[W448], yw[W448];
    wave_load_point_words(enc + (size_t)i * E448_PT_WORDS, xw, yw);
    bool valid = below_p(xw) && below_p(yw);
    const F448 x = unpack(xw), y = unpack(yw);
    const F448 x2 = sqr(x), y2 = sqr(y);
    // x^2 + y^2 = 1 + d x^2 y^2, that is x^2 + y^2 + 39081 x^2 y^2 - 1 = 0: a sum of three n and a small constant
    valid = valid && is_zero(sub(add(add(x2, y2), mul_small(mul(x2, y2), Fe448Consts::EDWARDS_D_NEG)), F448::small(1)));
    if constexpr (CHECK != 0) {
        const E448Point P = e448_from_affine(x, y);
        valid = valid && !e448_is_identity(P);
        uint32_t k[W448];
#pragma unroll
        for (int j = 0; j < W448; j++) k[j] = E448_ORDER[j];
        valid = e448_is_identity(wave_scalar_mul_core<Ed448Curve>(tab, lane, P, k)) && valid;
    }
    if (live) {
        if (valid) wave_store_point_words(out_xy + (size_t)i * E448_PT_WORDS, xw, yw);
        else wave_store_zero_words<E448_PT_WORDS>(out_xy + (size_t)i * E448_PT_WORDS);
        ok[i] = valid ? 1u : 0u;
    }
}

// Diagnostic (dr_ed448_field_selftest): fe448.hip.h's operations on RAW limb images, one lane per (a, b) pair of 16 int32 limbs each, so
// that tests can drive every operation at the limb bounds its contract allows.  out[i] = eleven canonical 56-byte records:
// a b, a^2, a + b, a - b, -a, carry(a), 39081 a, a^-1 (0 for 0), a^((p + 1) / 4) (a root of a when a is a square), a itself (pack),
// 156326 a;  flags[i]: bit 0 a is a square, bit 1 the canonical a is odd, bit 2 a is zero, bit 3 a = b.
constexpr int E448_SELFTEST_RECORDS = 11;
__global__ __launch_bounds__(64) void k_ed448_field_selftest(const int32_t* __restrict__ a_limbs, const int32_t* __restrict__ b_limbs, uint32_t n,
                                                            uint32_t* __restrict__ out, uint32_t* __restrict__ flags) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    F448 a, b;
#pragma unroll
    for (int t = 0; t < L448; t++) { a.l[t] = a_limbs[(size_t)i * L448 + t]; b.l[t] = b_limbs[(size_t)i * L448 + t]; }   // (in place: DESIGN.md section 8x)
    uint32_t* o = out + (size_t)i * E448_SELFTEST_RECORDS * W448;
    auto put = [&](int r, const F448& v) { field_selftest_put(o, r, v); };
    put(0, mul(a, b));
    put(1, sqr(a));
    put(2, add(a, b));
    put(3, sub(a, b));
    put(4, neg(a));
    put(5, carry(a));
    put(6, mul_small(a, Fe448Consts::EDWARDS_D_NEG));
    put(7, inv(a));
    F448 root;
    const bool sq = f448_sqrt(a, root);
    put(8, root);
    put(9, a);
    put(10, mul_small(a, Fe448Consts::MONT_A));
    flags[i] = (sq ? 1u : 0u) | (is_odd(a) ? 2u : 0u) | (is_zero(a) ? 4u : 0u) | (equal(a, b) ? 8u : 0u);
}

// Diagnostic (dr_ed448_law_selftest): wave_curve.hip.h's wave_law_selftest over Ed448Curve, the law on raw limb images
__global__ __launch_bounds__(64) void k_ed448_law_selftest(const int32_t* __restrict__ pts, const uint32_t* __restrict__ ctl, uint32_t n, int32_t* __restrict__ out) {
    wave_law_selftest<Ed448Curve>(pts, ctl, n, out);
}

}  // namespace dr
