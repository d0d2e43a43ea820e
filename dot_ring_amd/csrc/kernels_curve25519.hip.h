// Curve25519 kernels (DR_CURVE_CURVE25519_RO / _NU; the reference's specs/curve25519.py): Montgomery affine points (u, v) of
// v^2 = u^3 + 486662 u^2 + u over GF(2^255 - 19), 64 bytes u || v at the ABI.  The reference adds them by the affine chord-and-tangent
// law (mg_affine_point.py), which has no complete projective form; the group is Ed25519's under the birational map
//     x = c u / v,  y = (u - 1) / (u + 1),      u = (1 + y) / (1 - y),  v = c u / x,      c = sqrt(-486664)
// (Ed25519Ell2::SQRT_NEG_A_MINUS_2 in both directions: either root is an isomorphism as long as both directions use the same one), so
// every kernel here converts on loading, runs the Ed25519 group law and schedule (wave_scalar_mul_core<Ed25519Curve>, untouched), and
// converts back on storing: one launch and one pass over memory per batch.
//
// Loading costs no inversion: with x = a / b, y = e / f the extended point is (a f : e b : b f : a e), here
//     X = c u (u + 1),  Y = (u - 1) v,  Z = v (u + 1),  T = c u (u - 1)
// (a projective input is as good as an affine one to the schedule: the unified addition multiplies by both Z).  Storing costs one:
// i = 1 / (X (Z - Y)),  u = (Z + Y) X i,  v = c (Z + Y) Z i.
//
// Two points have no image under these formulas and are carried explicitly.  The identity <-> Edwards (0, 1): it has no affine
// Montgomery coordinates, and (0, 0) IS a point of this curve (the one of order 2), so 64 zero bytes cannot stand for it as they do on
// the Weierstrass curves: every kernel that takes or can produce the identity has a per-item FLAG word beside the point, 0 = the 16
// words are the point, 1 = the point is the identity (the 16 words are ignored on input and zero on output).  The point of order 2,
// (0, 0) <-> Edwards (0, -1): the only point with v = 0 (u^2 + 486662 u + 1 has no root: 486662^2 - 4 is not a square), picked out on
// loading by v = 0, and produced on storing by 0^-1 = 0 (X = 0 makes u = v = 0).  No other case exists: Z = v (u + 1) = 0 needs
// u = -1, where v^2 = -1 + 486662 - 1 = 486660, which is not a square mod p (tests/test_curve25519_cpu.py checks it with a big
// integer), so no rational point has u = -1; and Z - Y = 0 (y = 1) or X = 0 happen on Ed25519 only at (0, 1) and (0, -1).
#pragma once
#include "kernels_ed25519.hip.h"

namespace dr {

// the Edwards image of (u, v) in extended coordinates; `ident`: the identity flag of the input
DR_DEV EdPoint c25519_to_edwards(const F25& u, const F25& v, bool ident) {
    const F25 one = F25::small(1);
    const F25 cu = mul(F25::constant<Ed25519Ell2::SQRT_NEG_A_MINUS_2>(), u);     // n
    const F25 up = carry(add(u, one)), um = carry(sub(u, one));                  // n
    EdPoint r;
    r.x = mul(cu, up); r.y = mul(um, v); r.z = mul(v, up); r.t = mul(cu, um);
    const bool two = is_zero(v);                                                 // (0, 0) -> (0, -1)
    const F25 ey = cneg(one, two && !ident);
    r.x = select(two || ident, F25::zero(), r.x);
    r.t = select(two || ident, F25::zero(), r.t);
    r.y = select(two || ident, ey, r.y);
    r.z = select(two || ident, one, r.z);
    return r;
}
// u || v of an Edwards point (16 words) and its identity flag; (0, -1) stores (0, 0) through 0^-1 = 0, the identity zeros and flag 1
DR_DEV void c25519_store(uint32_t* out, uint32_t* flag, const EdPoint& p) {
    const F25 zmy = carry(sub(p.z, p.y)), zpy = carry(add(p.z, p.y));            // n
    const F25 inv = fe_inv(mul(p.x, zmy));
    const F25 zi = mul(zpy, inv);
    const bool ident = is_zero(p.x) && is_zero(zmy);
    wave_store_fe<Ed25519Curve>(out, mul(zi, p.x));
    wave_store_fe<Ed25519Curve>(out + 8, mul(mul(F25::constant<Ed25519Ell2::SQRT_NEG_A_MINUS_2>(), zi), p.z));
    *flag = ident ? 1u : 0u;
}
DR_DEV EdPoint c25519_load_term(const uint32_t* pt, const uint32_t* kp, uint32_t flag, uint32_t (&k)[8]) {
    const F25 u = wave_load_fe<Ed25519Curve>(pt), v = wave_load_fe<Ed25519Curve>(pt + 8);
    Ed25519Curve::load_scalar(kp, k);
    return c25519_to_edwards(u, v, flag != 0);
}

// out[i] = k[i] P[i].  pts: n x 16 words u || v canonical, ks: n x 8, id_in / id_out: n flag words, out: n x 16.  The schedule of the
// (secret) scalar is wave_curve.hip.h's: no branch and no bound depends on a digit.  (The body is wave_scalar_mul's of wave_curve.hip.h
// with this file's load and store forms: a change to that template's lane handling belongs here too.)
__global__ __launch_bounds__(ED_BLOCK) void k_c25519_scalar_mul(const uint32_t* __restrict__ pts, const uint32_t* __restrict__ ks,
                                                                const uint32_t* __restrict__ id_in, uint32_t* __restrict__ out,
                                                                uint32_t* __restrict__ id_out, uint32_t n) {
    __shared__ uint32_t tab[wave_table_words<Ed25519Curve>()];
    const int lane = threadIdx.x;
    uint32_t i = blockIdx.x * ED_BLOCK + lane;
    const bool live = i < n;
    if (!live) i = n - 1;            // keep the wave converged; the duplicate result is not stored
    uint32_t k[8];
    const EdPoint P = c25519_load_term(pts + (size_t)i * 16, ks + (size_t)i * 8, id_in[i], k);
    const EdPoint acc = wave_scalar_mul_core<Ed25519Curve>(tab, lane, P, k);
    if (live) c25519_store(out + (size_t)i * 16, id_out + i, acc);
}
// out[g] = sum_{j<m} k[g m + j] P[g m + j]: one lane per term (m padded to mpad, a power of two <= 64), folded with shuffles.  (The body
// is wave_msm_groups' of wave_curve.hip.h with this file's load and store forms: a change to that template's lane handling or fold
// belongs here too.)
__global__ __launch_bounds__(ED_BLOCK) void k_c25519_msm_groups(const uint32_t* __restrict__ pts, const uint32_t* __restrict__ ks,
                                                                const uint32_t* __restrict__ id_in, uint32_t* __restrict__ out,
                                                                uint32_t* __restrict__ id_out, uint32_t groups, uint32_t m, uint32_t mpad) {
    __shared__ uint32_t tab[wave_table_words<Ed25519Curve>()];
    const int lane = threadIdx.x;
    const uint32_t per_block = ED_BLOCK / mpad;
    const uint32_t g = blockIdx.x * per_block + lane / mpad;
    const uint32_t j = lane % mpad;
    const bool live = g < groups && j < m;
    const size_t idx = live ? (size_t)g * m + j : 0;          // dead lanes recompute term 0 and are masked out
    uint32_t k[8];
    const EdPoint P = c25519_load_term(pts + idx * 16, ks + idx * 8, id_in[idx], k);
    const EdPoint r = wave_scalar_mul_core<Ed25519Curve>(tab, lane, P, k);
    EdPoint acc = live ? r : ed_identity();
#pragma unroll 1
    for (uint32_t s = mpad >> 1; s > 0; s >>= 1) acc = ed_add(acc, wave_shfl_down<Ed25519Curve>(acc, s));
    if (g < groups && j == 0) c25519_store(out + (size_t)g * 16, id_out + g, acc);
}

// The bucket method from NARROW_PIP_FROM terms on (wave_msm.hip.h) runs Ed25519's stages (k_ed_msm_sort ... k_ed_msm_fold); only the
// records are made here: the map and its two exceptional points are paid once per term.  The set sums leave as Edwards x || y and the
// host converts the one result (narrow_law.hpp).
__global__ __launch_bounds__(WMSM_BLOCK) void k_c25519_msm_prepare(const uint32_t* __restrict__ pts, const uint32_t* __restrict__ id_in, uint32_t n,
                                                                   uint32_t* __restrict__ table) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const F25 u = wave_load_fe<Ed25519Curve>(pts + (size_t)i * 16), v = wave_load_fe<Ed25519Curve>(pts + (size_t)i * 16 + 8);
    wave_msm_put<Ed25519Curve>(table, i, c25519_to_edwards(u, v, id_in[i] != 0));
}

// Decoding (the reference's MGAffinePoint.string_to_point), one lane per 64-byte u || v: ok = u < p, v < p and v^2 = u^3 + 486662 u^2 + u
// — all the reference checks; out = the 16 words, or zeros.  MODE:
//   C25519_DEC_CODEC  the codec alone (small-order points and (0, 0) are accepted)
//   C25519_DEC_CHECK  also the prime-order check of the reference's curve.valid_point, as ED_DEC_CHECK runs it: Q = 8 P is not the
//                     identity and [8^-1 mod l] Q = P — what the VRF layer's dec_point asks of keys, inputs and proof points
enum { C25519_DEC_CODEC = 0, C25519_DEC_CHECK = 1 };
DR_DEV bool c25519_below_p(const uint32_t (&w)[8]) {   // w + 19 does not reach 2^255
    uint32_t c = 19u;
#pragma unroll
    for (int j = 0; j < 7; j++) c = (uint32_t)(((uint64_t)w[j] + c) >> 32);
    return (uint64_t)w[7] + c < 0x80000000ull;
}
template <int MODE>
__global__ __launch_bounds__(ED_BLOCK) void k_c25519_decode_points(const uint32_t* __restrict__ enc /* n*16 */, uint32_t* __restrict__ out_uv /* n*16 */,
                                                                   uint32_t* __restrict__ ok, uint32_t n) {
    __shared__ uint32_t tab[MODE == C25519_DEC_CHECK ? wave_table_words<Ed25519Curve>() : 1];
    const int lane = threadIdx.x;
    uint32_t i = blockIdx.x * ED_BLOCK + lane;
    const bool live = i < n;
    if (!live) i = n - 1;
    uint32_t uw[8], vw[8];
    wave_load8(enc + (size_t)i * 16, uw);
    wave_load8(enc + (size_t)i * 16 + 8, vw);
    bool valid = c25519_below_p(uw) && c25519_below_p(vw);
    const F25 u = fe_unpack(uw), v = fe_unpack(vw);
    const F25 rhs = mul(u, add(mul(u, add(u, F25::constant<Ed25519Ell2::A>())), F25::small(1)));     // u (u (u + A) + 1): n x (n + n)
    if (!equal(sqr(v), rhs)) valid = false;
    if constexpr (MODE == C25519_DEC_CHECK) {
        const EdPoint P = c25519_to_edwards(u, v, false);
        EdPoint Q = P;
#pragma unroll 1
        for (int j = 0; j < 3; j++) Q = ed_dbl<true>(Q);
        if (is_zero(Q.x)) { valid = false; Q = P; }   // 8 P = O (x = 0: 8 P lies in the prime-order subgroup, where only O has x = 0)
        constexpr uint32_t HINV[8] = {0xe2dc2f79u, 0x6106e529u, 0x7d1cdad0u, 0x07d39db3u, 0x00000000u, 0x00000000u, 0x00000000u, 0x06000000u};
        uint32_t k[8];
#pragma unroll
        for (int j = 0; j < 8; j++) k[j] = HINV[j];
        const EdPoint R = wave_scalar_mul_core<Ed25519Curve>(tab, lane, Q, k);
        if (!equal(mul(R.x, P.z), mul(P.x, R.z)) || !equal(mul(R.y, P.z), mul(P.y, R.z))) valid = false;
    }
    if (live) {
        if (valid) {
            wave_store8(out_uv + (size_t)i * 16, uw);
            wave_store8(out_uv + (size_t)i * 16 + 8, vw);
        } else {
            wave_store_zero8(out_uv + (size_t)i * 16);
            wave_store_zero8(out_uv + (size_t)i * 16 + 8);
        }
        ok[i] = valid ? 1u : 0u;
    }
}

// ---------------------------------------------------------------- hashing to the curve (RFC 9380, curve25519_XMD:SHA-512_ELL2_RO_ / _NU_)
// The reference's MGAffinePoint.map_to_curve is the Elligator 2 map ed_ell2_map computes before its own change of model, and it has no
// failing inverse: it returns a point for every field element.  ed_ell2_map reports ok = false where the Edwards image has Z = 0: the
// Montgomery image has v = 0 or u = -1.  u = -1 is no rational point (above).  v = 0 is (0, 0) alone, reached by x2 = -A tv1 / d = 0,
// that is tv1 = 2 u^2 = 0: the input 0 and no other (x1 = -A / d is never 0, and for the input 0 gx1 = -486662 is not a square, so x2 is
// taken).  So ok = false means exactly "the image is (0, 0)", whose Edwards form is (0, -1).
DR_DEV EdPoint c25519_ell2_edwards(const F25& u) {
    bool ok;
    EdPoint q = ed_ell2_map(u, ok);
    const F25 one = F25::small(1), zero = F25::zero();
    q.x = select(ok, q.x, zero);
    q.y = select(ok, q.y, neg(one));
    q.z = select(ok, q.z, one);
    q.t = select(ok, q.t, zero);
    return q;
}
// out[i] = [8] (the sum of the images of item i's `per_item` field elements) (2: the uniform (RO) encoding, 1: the nonuniform one), or
// the sum itself when clear_cofactor = 0 (one element: the reference's map_to_curve).  us: n x per_item x 8 words (canonical, checked by
// the host), out: n x 16 words u || v, ident[i]: the identity flag.  Every canonical input has a value: there is no error output.
__global__ __launch_bounds__(ED_BLOCK) void k_curve25519_map_to_curve(const uint32_t* __restrict__ us, uint32_t* __restrict__ out_uv,
                                                                      uint32_t* __restrict__ ident, uint32_t n, uint32_t per_item,
                                                                      uint32_t clear_cofactor) {
    uint32_t i = blockIdx.x * ED_BLOCK + threadIdx.x;
    const bool live = i < n;
    if (!live) i = n - 1;
    EdPoint acc = ed_identity();
#pragma unroll 1
    for (uint32_t e = 0; e < per_item; e++)
        acc = ed_add(acc, c25519_ell2_edwards(wave_load_fe<Ed25519Curve>(us + ((size_t)i * per_item + e) * 8)));
    if (clear_cofactor) {
#pragma unroll 1
        for (int j = 0; j < 3; j++) acc = ed_dbl<true>(acc);
    }
    if (live) c25519_store(out_uv + (size_t)i * 16, ident + i, acc);
}

}  // namespace dr
