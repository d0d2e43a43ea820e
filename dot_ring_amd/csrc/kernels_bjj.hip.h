// Baby JubJub kernels (DR_CURVE_BABYJUBJUB; the reference's specs/baby_jubjub.py): the twisted Edwards group law with a = 1 over
// the BN254 scalar field (fbn254.hip.h) and the kernels that fill, for this curve, the roles kernels_ed25519.hip.h fills for Ed25519:
// variable-base scalar multiplication on a fixed schedule, grouped MSMs, point decoding and the device half of try-and-increment.
// The existing kernels stay as they are; no other kernel includes this header's field.
//
// Points cross the ABI as x || y little-endian, standard form; inside they are extended coordinates (X, Y, Z, T) in Montgomery form,
// x = X / Z, y = Y / Z, T = X Y / Z.  dbl-2008-hwcd and add-2008-hwcd with a = 1: D = a A = A and H = B - a A = B - A.  The
// comments give the limb bound of every intermediate against fbn254.hip.h's contract ("n" = normal).  LDS tables and shuffles keep
// the Montgomery limbs: a table entry is bn_to_words of each coordinate (8 words, value below 2^256, not canonical).
#pragma once
#include "fbn254.hip.h"
#include "wave_curve.hip.h"
#include "wave_msm.hip.h"

namespace dr {

constexpr int BJJ_BLOCK = 64;         // one wave per workgroup; 64 KiB of LDS table per wave (X, Y, Z, T x 8 words), as k_ed_scalar_mul

// Square roots, p - 1 = Q 2^28 (Q odd).  With w = x^((Q-1)/2), R = w x, t = R w = x^Q, t lies in the cyclic group <c> of order
// 2^28, c = 5^Q (5 is the smallest non-residue).  Its logarithm e (t = c^e) is read off in four 7-bit windows, as fr_sqrt_core
// (kernels_bsn.hip.h) does in 8-bit windows for the BLS12-381 scalar field: t^(2^21) is one of the 128 elements of <c^(2^21)>, a
// perfect-hash table gives e mod 2^7, t c^(-e0) raised to 2^14 the next window, and so on — 42 squarings, 7 products and 4 look-ups
// after the exponentiation, the same in every lane.  x is a square iff e is even, and then sqrt(x) = R c^(-e/2).  The tables are
// built on the host once per process and copied to the device once per context (capi_native256.hip: bjj_consts_ready).  Entries are in
// Montgomery form (bn_unpack_raw reads them); the hash is over the low word of the standard (packed) value.
constexpr int BJJ_DL_SLOTS = 4096;
struct BjjConsts {
    uint32_t dl_mul[3][128][8];          // c^(-k 2^(7j))
    uint32_t dl_half[4][128][8];         // c^(-k 2^(7j) / 2)   (j = 0: c^(-(k >> 1)), read for even k only)
    uint32_t dl_hash_mul;                // map[(low word * dl_hash_mul) >> 20] = k for the element c^(k 2^21)
    uint8_t dl_map[BJJ_DL_SLOTS];
};
__device__ BjjConsts g_bjj_consts;

DR_DEV Fbn bjj_table_const(const uint32_t (&w)[8]) { return bn_unpack_raw(w); }
DR_DEV uint32_t bjj_dlog_window(const Fbn& v) {
    uint32_t w[8];
    bn_pack(v, w);
    return g_bjj_consts.dl_map[(w[0] * g_bjj_consts.dl_hash_mul) >> 20] & 127u;     // (every slot a member can reach holds 0..127)
}
// a square root of x (which of the two is unspecified: callers fix the sign); false, root = 0, when x is not a square
DR_DEV bool bjj_sqrt(const Fbn& x, Fbn& root) {
    root = Fbn::zero();
    if (is_zero(x)) return true;
    constexpr uint32_t QM1H[8] = {0x1f0fac9fu, 0xcdcb848au, 0x419f4243u, 0x0c0ac2e9u, 0xc2822db4u, 0x098d014du, 0x83227397u, 0x00000001u};   // (Q-1)/2
    uint32_t e[8];
#pragma unroll
    for (int i = 0; i < 8; i++) e[i] = QM1H[i];
    const Fbn w = bn_pow(x, e);
    Fbn R = mul(w, x);
    Fbn t = mul(R, w);
#pragma unroll 1
    for (int j = 0; j < 4; j++) {
        Fbn v = t;
#pragma unroll 1
        for (int k = 0; k < 21 - 7 * j; k++) v = sqr(v);
        const uint32_t ej = bjj_dlog_window(v);
        if (j == 0 && (ej & 1u)) return false;
        if (j < 3) t = mul(t, bjj_table_const(g_bjj_consts.dl_mul[j][ej]));
        R = mul(R, bjj_table_const(g_bjj_consts.dl_half[j][ej]));
    }
    root = R;
    return true;
}

// ---------------------------------------------------------------- group law
struct BjjPoint {
    Fbn x, y, z, t;
};

DR_DEV BjjPoint bjj_identity() {
    BjjPoint p;
    p.x = Fbn::zero(); p.y = bn_one(); p.z = bn_one(); p.t = Fbn::zero();
    return p;
}

// dbl-2008-hwcd, a = 1.  WITH_T = false skips T3 (the result is only doubled again).  Coordinates n (x and t possibly negated by
// bjj_cneg: every operand below is a square or a product, which take a negated normal as they take a normal) in, n out: every
// coordinate is a product (T = 0 without it)
template <bool WITH_T>
DR_DEV BjjPoint bjj_dbl(const BjjPoint& p) {
    const Fbn A = sqr(p.x), B = sqr(p.y);                   // n
    const Fbn C = dbl(sqr(p.z));                            // limbs < 2^30
    const Fbn E = carry(dbl(mul(p.x, p.y)));                // 2 x y: carried sum of two normals
    const Fbn G = add(A, B);                                // D + B with D = a A = A: limbs < 2^30
    const Fbn F = carry(sub(G, C));                         // carried sum of four normals
    const Fbn H = sub(A, B);                                // D - B: limbs in (-2^29, 2^29)
    BjjPoint r;
    r.x = mul(E, F);
    r.y = mul(G, H);
    r.z = mul(F, G);
    if (WITH_T) r.t = mul(E, H);
    else r.t = Fbn::zero();
    return r;
}

// add-2008-hwcd, a = 1, unified (also right for doubling and the identity: d is not a square, a = 1 is).  dt2 = d T2.  Coordinates n
// (x and t possibly negated by bjj_cneg, in either point) in, n out: every coordinate is a product
DR_DEV BjjPoint bjj_add_dt(const BjjPoint& p, const BjjPoint& q, const Fbn& dt2) {
    const Fbn A = mul(p.x, q.x), B = mul(p.y, q.y);          // n
    const Fbn C = mul(p.t, dt2);                            // n
    const Fbn D = mul(p.z, q.z);                            // n
    const Fbn E = mul2(p.x, q.y, p.y, q.x);                 // n (operands n or negated n)
    const Fbn F = sub(D, C), G = add(D, C);                 // limbs < 2^29 and < 2^30 in magnitude
    const Fbn H = sub(B, A);                                // B - a A
    BjjPoint r;
    r.x = mul(E, F);
    r.y = mul(G, H);
    r.t = mul(E, H);
    r.z = mul(F, G);
    return r;
}
DR_DEV BjjPoint bjj_add(const BjjPoint& p, const BjjPoint& q) {
    return bjj_add_dt(p, q, mul(Fbn::constant<FbnConsts::D>(), q.t));
}

DR_DEV BjjPoint bjj_cneg(const BjjPoint& p, bool negate) {
    BjjPoint r = p;
    r.x = cneg(p.x, negate);
    r.t = cneg(p.t, negate);
    return r;
}

// ---------------------------------------------------------------- memory
// a normal (value in (-2^253, p + 2^253)) as the 8 words of its Montgomery value, moved into [0, 2^256): carried, p added when it is
// negative — bn_unpack_raw reads it back as a normal of the same value mod p (the loop is bn_pack's, in place for the same reason)
DR_DEV void bn_to_words(const Fbn& a, uint32_t (&w)[8]) {
    Fbn c = carry(a);
    c = carry(select(c.l[LIMBS29 - 1] < 0, add(c, Fbn::constant<FbnConsts::P>()), c));
#pragma unroll
    for (int j = 0; j < 8; j++) w[j] = 0;
#pragma unroll
    for (int i = 0; i < LIMBS29; i++) {
        const uint32_t u = (uint32_t)c.l[i];
        const int bit = 29 * i, j = bit >> 5, sh = bit & 31;
        w[j] |= u << sh;
        if (sh > 3 && j + 1 < 8) w[j + 1] |= u >> (32 - sh);
    }
}

// k mod l for a 256-bit k: floor((2^256 - 1) / l) = 42 < 64, so conditional subtractions of 32 l, 16 l, 8 l, 4 l, 2 l and l (the
// same six in every lane)
DR_DEV void bjj_reduce_mod_order(uint32_t (&k)[8]) {
    constexpr uint32_t L[8] = {0x392126f1u, 0x677297dcu, 0x3920ee0au, 0xab3eedb8u, 0xd0302b0bu, 0x370a08b6u, 0x5c263405u, 0x060c89ceu};
#pragma unroll 1
    for (int s = 5; s >= 0; s--) {
        uint32_t d[8], borrow = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            uint32_t lw = L[i] << s;                         // word i of l 2^s (l < 2^251: nothing leaves word 7)
            if (s > 0 && i > 0) lw |= L[i - 1] >> (32 - s);
            d[i] = subb(k[i], lw, borrow);
        }
#pragma unroll
        for (int i = 0; i < 8; i++) k[i] = borrow ? k[i] : d[i];
    }
}

// wave_curve.hip.h's description of Baby JubJub: standard-form words at the ABI, Montgomery limbs inside and Montgomery words
// (bn_to_words / bn_unpack_raw) in the LDS table, 64 windows (l < 2^251)
struct BjjCurve {
    using Fe = Fbn;
    using Point = BjjPoint;
    static constexpr int WORDS = 8, SCALAR_WORDS = 8, BLOCK = BJJ_BLOCK, WINDOWS = 64, LDS_WORDS = 8;
    static constexpr bool EXTENDED = true, ZERO_IS_IDENTITY = false;
    DR_DEV static Fbn unpack(const uint32_t (&w)[8]) { return bn_unpack(w); }
    DR_DEV static void pack(const Fbn& a, uint32_t (&w)[8]) { bn_pack(a, w); }
    DR_DEV static Fbn inv(const Fbn& a) { return bn_inv(a); }
    DR_DEV static void to_lds(const Fbn& a, uint32_t (&w)[8]) { bn_to_words(a, w); }
    DR_DEV static Fbn from_lds(const uint32_t (&w)[8]) { return bn_unpack_raw(w); }
    DR_DEV static BjjPoint identity() { return bjj_identity(); }
    DR_DEV static BjjPoint from_affine(const Fbn& x, const Fbn& y) {
        BjjPoint P;
        P.x = x; P.y = y; P.z = bn_one(); P.t = mul(x, y);
        return P;
    }
    DR_DEV static BjjPoint add(const BjjPoint& p, const BjjPoint& q) { return bjj_add(p, q); }
    DR_DEV static BjjPoint dbl(const BjjPoint& p) { return bjj_dbl<true>(p); }
    DR_DEV static BjjPoint dbl_no_t(const BjjPoint& p) { return bjj_dbl<false>(p); }
    DR_DEV static BjjPoint cneg(const BjjPoint& p, bool negate) { return bjj_cneg(p, negate); }
    DR_DEV static void load_scalar(const uint32_t* p, uint32_t (&k)[8]) {
        wave_load8(p, k);
        bjj_reduce_mod_order(k);
    }
};

// out[i] = k[i] P[i]: wave_curve.hip.h's kernel bodies for this curve
__global__ __launch_bounds__(BJJ_BLOCK) void k_bjj_scalar_mul(const uint32_t* __restrict__ pts, const uint32_t* __restrict__ ks,
                                                              uint32_t* __restrict__ out, uint32_t n) {
    wave_scalar_mul<BjjCurve>(pts, ks, out, n);
}
// out[g] = sum_{j<m} k[g m + j] P[g m + j]
__global__ __launch_bounds__(BJJ_BLOCK) void k_bjj_msm_groups(const uint32_t* __restrict__ pts, const uint32_t* __restrict__ ks,
                                                              uint32_t* __restrict__ out, uint32_t groups, uint32_t m, uint32_t mpad) {
    wave_msm_groups<BjjCurve>(pts, ks, out, groups, m, mpad);
}
// the bucket method from NARROW_PIP_FROM terms on (wave_msm.hip.h): the stages over BjjCurve, set sums out as affine x || y
DR_WAVE_MSM_KERNELS(bjj, BjjCurve)

// Decoding (the reference's point.py:150-214 with te_affine_point.py:297-316), one lane per 32-byte encoding: the sign is bit 255,
// y the low 255 bits, y >= p rejected (so is every encoding with bit 254 set: p < 2^254); x^2 = (1 - y^2) / (1 - d y^2) (a = 1; the
// denominator never vanishes: 1 / d is not a square), no root rejected; x is the larger of (x, p - x) iff the sign bit is set.
// x = 0 (y = +-1) ignores the sign bit.  MODE:
//   BJJ_DEC_CODEC  the codec alone: ok = decoded, out = (x, y)
//   BJJ_DEC_CHECK  also the prime-order check: Q = 8 P is not the identity and [8^-1 mod l] Q = P — the identity and all 8 torsion
//                  points are rejected, as is any point with a torsion component
//   BJJ_DEC_TAI    the device half of try-and-increment (point.py:252-296; the host has already masked the candidate, clearing
//                  bit 254): ok = decoded and 8 P is not the identity, out = 8 P
enum { BJJ_DEC_CODEC = 0, BJJ_DEC_CHECK = 1, BJJ_DEC_TAI = 2 };
template <int MODE>
__global__ __launch_bounds__(BJJ_BLOCK) void k_bjj_decode_points(const uint32_t* __restrict__ enc /* n*8 */, uint32_t* __restrict__ out_xy /* n*16 */,
                                                                 uint32_t* __restrict__ ok, uint32_t n) {
    __shared__ uint32_t tab[MODE == BJJ_DEC_CHECK ? wave_table_words<BjjCurve>() : 1];
    const int lane = threadIdx.x;
    uint32_t i = blockIdx.x * BJJ_BLOCK + lane;
    const bool live = i < n;
    if (!live) i = n - 1;
    uint32_t ys[8];
    wave_load8(enc + (size_t)i * 8, ys);
    const bool sign = (ys[7] >> 31) != 0;
    ys[7] &= 0x7fffffffu;
    bool valid;
    {   // y < p
        uint32_t borrow = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) (void)subb(ys[j], FbnConsts::PW[j], borrow);
        valid = borrow != 0;
    }
    const Fbn one = bn_one();
    const Fbn yy = bn_unpack(ys);
    const Fbn y2 = sqr(yy);
    const Fbn u = sub(one, y2);
    const Fbn v = sub(one, mul(Fbn::constant<FbnConsts::D>(), y2));
    Fbn x;
    if (!bjj_sqrt(mul(u, bn_inv(v)), x)) valid = false;
    if (is_larger(x) != sign) x = neg(x);
    Fbn ox = x, oy = yy;
    if constexpr (MODE != BJJ_DEC_CODEC) {
        const BjjPoint P = BjjCurve::from_affine(x, yy);
        BjjPoint Q = P;
#pragma unroll 1
        for (int j = 0; j < 3; j++) Q = bjj_dbl<true>(Q);
        if (is_zero(Q.x)) { valid = false; Q = P; }  // 8 P = O (x = 0: 8 P lies in the prime-order subgroup, where only O has x = 0)
        const Fbn zi = bn_inv(Q.z);
        const Fbn qx = mul(Q.x, zi), qy = mul(Q.y, zi);
        if constexpr (MODE == BJJ_DEC_TAI) {
            ox = qx; oy = qy;
        } else {
            constexpr uint32_t HINV[8] = {0xb1fd0213u, 0x1a8444e0u, 0x31fcd049u, 0x35d71001u, 0xf62a25aau, 0x9028c79fu, 0x90a16d84u, 0x054af894u};
            uint32_t k[8];
#pragma unroll
            for (int j = 0; j < 8; j++) k[j] = HINV[j];
            const BjjPoint R = wave_scalar_mul_core<BjjCurve>(tab, lane, BjjCurve::from_affine(qx, qy), k);
            if (!equal(R.x, mul(x, R.z)) || !equal(R.y, mul(yy, R.z))) valid = false;
        }
    }
    if (!valid) { ox = Fbn::zero(); oy = Fbn::zero(); }
    if (live) {
        wave_store_fe<BjjCurve>(out_xy + (size_t)i * 16, ox);
        wave_store_fe<BjjCurve>(out_xy + (size_t)i * 16 + 8, oy);
        ok[i] = valid ? 1u : 0u;
    }
}

// Diagnostic (dr_bjj_field_ops_selftest): fbn254.hip.h's operations on raw limb images, one lane per (a, b) pair of 9 int32 limbs
// each (Montgomery images: the element of limbs l is sum l_i 2^(29 i) / 2^261 mod p), so that tests can drive every operation at the
// limb bounds its contract allows.  out[i] = twelve canonical 32-byte records (standard form): a b, a^2, a + b, a - b, -a, carry(a),
// a b + b a (mul2), a^-1 (0 for 0), sqrt(a) or 0, a itself (pack), a b through bn_to_words / bn_unpack_raw (the LDS round trip),
// a through bn_unpack(pack(a)); flags[i]: bit 0 a is a square, bit 2 a is the larger of (a, -a).
constexpr int BJJ_SELFTEST_RECORDS = 12;
__global__ __launch_bounds__(64) void k_bjj_field_selftest(const int32_t* __restrict__ a_limbs, const int32_t* __restrict__ b_limbs, uint32_t n,
                                                           uint32_t* __restrict__ out, uint32_t* __restrict__ flags) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    Fbn a, b;
#pragma unroll
    for (int t = 0; t < LIMBS29; t++) { a.l[t] = a_limbs[(size_t)i * LIMBS29 + t]; b.l[t] = b_limbs[(size_t)i * LIMBS29 + t]; }
    uint32_t* o = out + (size_t)i * BJJ_SELFTEST_RECORDS * 8;
    wave_store_fe<BjjCurve>(o + 0, mul(a, b));
    wave_store_fe<BjjCurve>(o + 8, sqr(a));
    wave_store_fe<BjjCurve>(o + 16, add(a, b));
    wave_store_fe<BjjCurve>(o + 24, sub(a, b));
    wave_store_fe<BjjCurve>(o + 32, neg(a));
    wave_store_fe<BjjCurve>(o + 40, carry(a));
    wave_store_fe<BjjCurve>(o + 48, mul2(a, b, b, a));
    wave_store_fe<BjjCurve>(o + 56, bn_inv(a));
    Fbn r;
    const bool sq = bjj_sqrt(a, r);
    wave_store_fe<BjjCurve>(o + 64, r);
    wave_store_fe<BjjCurve>(o + 72, a);
    uint32_t w[8];
    bn_to_words(mul(a, b), w);
    wave_store_fe<BjjCurve>(o + 80, bn_unpack_raw(w));
    bn_pack(a, w);
    wave_store_fe<BjjCurve>(o + 88, bn_unpack(w));
    flags[i] = (sq ? 1u : 0u) | (is_larger(a) ? 4u : 0u);
}

// Diagnostic (dr_bjj_law_selftest): wave_curve.hip.h's wave_law_selftest over BjjCurve, the law on raw limb images
__global__ __launch_bounds__(64) void k_bjj_law_selftest(const int32_t* __restrict__ pts, const uint32_t* __restrict__ ctl, uint32_t n, int32_t* __restrict__ out) {
    wave_law_selftest<BjjCurve>(pts, ctl, n, out);
}

}  // namespace dr
