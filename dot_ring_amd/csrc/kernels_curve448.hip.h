// Curve448 kernels (DR_CURVE_CURVE448_RO / DR_CURVE_CURVE448_NU; the reference's specs/curve448.py): Montgomery affine points (u, v),
// 112 bytes u || v at the ABI, on the complete Edwards law of c448_law.hip.h (the curve birational to curve448; Ed448's own law is
// 4-isogenous and cannot serve).  Every kernel converts on loading, runs that law under the fixed 113-window schedule, and converts back
// on storing: one launch and one pass over memory per batch, as kernels_curve25519.hip.h does over the Ed25519 kernels.
//
// The identity has no affine coordinates and (0, 0) IS a point (order 2), so the scalar-multiplication kernels carry a per-item FLAG
// word beside the point in both directions (0 = the 28 words are the point, 1 = the identity; the words are ignored on input and zero
// on output); the host turns 112 bytes of 0xff into that flag and back (capi_suite.hpp, run_points).  The map writes the 0xff bytes
// itself, because its flag word says whether the item has a value at all.
//
// The schedule is wave_curve.hip.h's over Curve448Curve, which gives the law and the table forms; the memory forms (seven uint4 a point,
// seven uint2 a scalar) are that header's too.  The kernel bodies stay here: they carry the flag words.
// Included by capi_ed448.hip after kernels_ed448.hip.h: one unit per kernel header, and no second copy of the Ed448 kernels.
#pragma once
#include "c448_law.hip.h"
#include "kernels_ed448.hip.h"

namespace dr {

struct Curve448Curve : Limb28Curve<Fe448Consts> {
    using Point = M448Point;
    static constexpr int SCALAR_WORDS = W448, BLOCK = E448_BLOCK, WINDOWS = E448_WINDOWS;   // any k < 2^448
    static constexpr bool EXTENDED = false;
    DR_DEV static M448Point add(const M448Point& p, const M448Point& q) { return m448_add(p, q); }
    DR_DEV static M448Point dbl(const M448Point& p) { return m448_dbl(p); }
    DR_DEV static M448Point cneg(const M448Point& p, bool negate) { return m448_cneg(p, negate); }
    DR_DEV static M448Point identity() { return m448_identity(); }
};

// ---------------------------------------------------------------- memory forms
DR_DEV M448Point c448_load_term(const uint32_t* pt, uint32_t flag) {
    uint32_t u[W448], v[W448];
    wave_load_point_words(pt, u, v);
    return m448_load(unpack(u), unpack(v), flag != 0);
}
// u || v of a point (28 words); true for the identity, which stores zeros.  (0 : -1 : 1) stores (0, 0)
DR_DEV bool c448_store(uint32_t* out, const M448Point& p) {
    F448 u, v;
    const bool ident = m448_store(p, u, v);
    uint32_t uw[W448], vw[W448];
    pack(u, uw);
    pack(v, vw);
    wave_store_point_words(out, uw, vw);
    return ident;
}
DR_DEV void c448_store_fill(uint32_t* p, uint32_t word) {
    uint4* q = reinterpret_cast<uint4*>(p);
#pragma unroll
    for (int j = 0; j < E448_PT_WORDS / 4; j++) q[j] = make_uint4(word, word, word, word);
}

// out[i] = k[i] P[i].  pts: n x 28 words u || v canonical, ks: n x 14, id_in / id_out: n flag words, out: n x 28.  One lane per
// multiplication; the operand order is capi_suite.hpp's launch_points for a flagged suite.  The schedule of the (secret) scalar is
// wave_curve.hip.h's: 8 x 3 x 16 table words x 64 lanes x 4 = 98 304 bytes of LDS, one workgroup per CU.  (The body is wave_scalar_mul's
// with this file's load and store forms: a change to that template's lane handling belongs here too.)
__global__ __launch_bounds__(E448_BLOCK) void k_c448_scalar_mul(const uint32_t* __restrict__ pts, const uint32_t* __restrict__ ks,
                                                                const uint32_t* __restrict__ id_in, uint32_t* __restrict__ out,
                                                                uint32_t* __restrict__ id_out, uint32_t n) {
    __shared__ uint32_t tab[wave_table_words<Curve448Curve>()];
    const int lane = threadIdx.x;
    uint32_t i = blockIdx.x * E448_BLOCK + lane;
    const bool live = i < n;
    if (!live) i = n - 1;            // keep the wave converged; the duplicate result is not stored
    uint32_t k[W448];
    wave_load_words(ks + (size_t)i * W448, k);
    const M448Point P = c448_load_term(pts + (size_t)i * E448_PT_WORDS, id_in[i]);
    const M448Point acc = wave_scalar_mul_core<Curve448Curve>(tab, lane, P, k);
    if (live) id_out[i] = c448_store(out + (size_t)i * E448_PT_WORDS, acc) ? 1u : 0u;
}

// out[g] = sum_{j<m} k[g m + j] P[g m + j]: one lane per term (m padded to mpad, a power of two <= 64), folded with shuffles by the
// complete addition (terms that coincide or cancel need nothing special).  (The body is wave_msm_groups' with this file's load and store
// forms: a change to that template's lane handling or fold belongs here too.)
__global__ __launch_bounds__(E448_BLOCK) void k_c448_msm_groups(const uint32_t* __restrict__ pts, const uint32_t* __restrict__ ks,
                                                                const uint32_t* __restrict__ id_in, uint32_t* __restrict__ out,
                                                                uint32_t* __restrict__ id_out, uint32_t groups, uint32_t m, uint32_t mpad) {
    __shared__ uint32_t tab[wave_table_words<Curve448Curve>()];
    const int lane = threadIdx.x;
    const uint32_t per_block = E448_BLOCK / mpad;
    const uint32_t g = blockIdx.x * per_block + lane / mpad;
    const uint32_t j = lane % mpad;
    const bool live = g < groups && j < m;
    const size_t idx = live ? (size_t)g * m + j : 0;          // dead lanes recompute term 0 and are masked out
    uint32_t k[W448];
    wave_load_words(ks + idx * W448, k);
    const M448Point P = c448_load_term(pts + idx * E448_PT_WORDS, id_in[idx]);
    const M448Point r = wave_scalar_mul_core<Curve448Curve>(tab, lane, P, k);
    M448Point acc = live ? r : m448_identity();
#pragma unroll 1
    for (uint32_t s = mpad >> 1; s > 0; s >>= 1) acc = m448_add(acc, wave_shfl_down<Curve448Curve>(acc, s));
    if (g < groups && j == 0) id_out[g] = c448_store(out + (size_t)g * E448_PT_WORDS, acc) ? 1u : 0u;
}


// ---------------------------------------------------------------- the bucket method (dr_wide_msm): wave_msm.hip.h over Curve448Curve
// One MSM of n >= WIDE_PIP_FROM terms; the stages, their operands and the plan are that header's.  W448 scalar words, as they are.
// (the point is loaded as k_c448_msm_groups loads it: u || v with the flag word of the identity beside it)
__global__ __launch_bounds__(WMSM_BLOCK) void k_c448_msm_prepare(const uint32_t* __restrict__ pts, const uint32_t* __restrict__ id_in, uint32_t n,
                                                                uint32_t* __restrict__ table) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    wave_msm_put<Curve448Curve>(table, i, c448_load_term(pts + (size_t)i * E448_PT_WORDS, id_in[i]));
}
// (the sort looks at scalars only, and those are Ed448's 14 words: k_ed448_msm_sort)
__global__ __launch_bounds__(WMSM_BLOCK) void k_c448_msm_accumulate(const uint32_t* __restrict__ table, const uint32_t* __restrict__ sorted,
                                                                    const uint32_t* __restrict__ offsets, const uint32_t* __restrict__ counts,
                                                                    const uint32_t* __restrict__ perm, uint32_t* __restrict__ buckets, size_t nbuckets) {
    wave_msm_accumulate<Curve448Curve>(table, sorted, offsets, counts, perm, buckets, nbuckets);
}
__global__ __launch_bounds__(64) void k_c448_msm_accumulate_heavy(const uint32_t* __restrict__ table, const uint32_t* __restrict__ sorted,
                                                                  const uint32_t* __restrict__ offsets, const uint32_t* __restrict__ counts,
                                                                  uint32_t* __restrict__ buckets, size_t nbuckets) {
    wave_msm_accumulate_heavy<Curve448Curve>(table, sorted, offsets, counts, buckets, nbuckets);
}
__global__ __launch_bounds__(WMSM_BLOCK) void k_c448_msm_reduce(const uint32_t* __restrict__ buckets, size_t sets, uint32_t H, uint32_t L,
                                                                uint32_t* __restrict__ partial) {
    wave_msm_reduce<Curve448Curve>(buckets, sets, H, L, partial);
}
__global__ __launch_bounds__(WMSM_BLOCK) void k_c448_msm_fold(const uint32_t* __restrict__ partial, size_t sets, uint32_t T, uint32_t* __restrict__ setsum) {
    wave_msm_fold<Curve448Curve>(partial, sets, T, setsum);
}

// ---------------------------------------------------------------- hashing to the curve (RFC 9380, curve448_XOF:SHAKE256_ELL2_RO_ / _NU_)
// out[i] = [4 if clear] (the sum of the images of item i's `per_item` field elements) (2: the uniform (RO) encoding, 1: the nonuniform
// one).  us: n x per_item x 14 words (canonical, checked by the host), out: n x 28 words u || v.  ok[i] = 0 and 112 zero bytes exactly
// where an element has u^2 = 1 (the reference raises there); a sum that is the identity is ok = 1 and 112 bytes of 0xff.  clear = 0 with
// per_item = 1 is the reference's map_to_curve.  One lane per item; one exponentiation per element and one inversion per item.
__global__ __launch_bounds__(E448_BLOCK) void k_curve448_map_to_curve(const uint32_t* __restrict__ us, uint32_t* __restrict__ out_uv,
                                                                      uint32_t* __restrict__ ok, uint32_t n, uint32_t per_item, uint32_t clear) {
    uint32_t i = blockIdx.x * E448_BLOCK + threadIdx.x;
    const bool live = i < n;
    if (!live) i = n - 1;
    M448Point acc = m448_identity();
    bool good = true;
#pragma unroll 1
    for (uint32_t e = 0; e < per_item; e++) {
        uint32_t w[W448];
        wave_load_words(us + ((size_t)i * per_item + e) * W448, w);
        F448 N, D, v;
        bool has_value;
        m448_ell2(unpack(w), N, D, v, has_value);
        good = good && has_value;
        acc = m448_add(acc, m448_load_fraction(N, D, v));
    }
    if (clear) {
#pragma unroll 1
        for (int j = 0; j < 2; j++) acc = m448_dbl(acc);                     // the cofactor
    }
    if (live) {
        uint32_t* o = out_uv + (size_t)i * E448_PT_WORDS;
        const bool ident = c448_store(o, acc);
        if (!good) c448_store_fill(o, 0u);
        else if (ident) c448_store_fill(o, 0xffffffffu);
        ok[i] = good ? 1u : 0u;
    }
}

// Decoding (the reference's MGAffinePoint.string_to_point), one lane per 112-byte u || v.  CHECK = 0: both coordinates below p and
// v^2 = u^3 + A u^2 + u ((0, 0) and the points of order 4 pass; a record of 0xff bytes does not).  CHECK = 1: additionally n P = O by
// the fixed schedule over the public words of n (a decoded point is never the identity; (0, 0) has order 2 and fails).  out = the input
// and ok = 1, or 112 zero bytes and ok = 0.
template <int CHECK>
__global__ __launch_bounds__(E448_BLOCK) void k_c448_decode_points(const uint32_t* __restrict__ enc, uint32_t* __restrict__ out_uv,
                                                                   uint32_t* __restrict__ ok, uint32_t n) {
    __shared__ uint32_t tab[CHECK ? wave_table_words<Curve448Curve>() : 1];
    const int lane = threadIdx.x;
    uint32_t i = blockIdx.x * E448_BLOCK + lane;
    const bool live = i < n;
    if (!live) i = n - 1;
    uint32_t uw[W448], vw[W448];
    wave_load_point_words(enc + (size_t)i * E448_PT_WORDS, uw, vw);
    bool valid = below_p(uw) && below_p(vw);
    const F448 u = unpack(uw), v = unpack(vw);
    valid = valid && m448_on_curve(u, v);
    if constexpr (CHECK != 0) {
        const M448Point P = m448_load(u, v, false);
        uint32_t k[W448];
#pragma unroll
        for (int j = 0; j < W448; j++) k[j] = E448_ORDER[j];
        valid = m448_is_identity(wave_scalar_mul_core<Curve448Curve>(tab, lane, P, k)) && valid;
    }
    if (live) {
        if (valid) wave_store_point_words(out_uv + (size_t)i * E448_PT_WORDS, uw, vw);
        else wave_store_zero_words<E448_PT_WORDS>(out_uv + (size_t)i * E448_PT_WORDS);
        ok[i] = valid ? 1u : 0u;
    }
}

// Diagnostic (dr_curve448_law_selftest): wave_curve.hip.h's wave_law_selftest over Curve448Curve, the law on raw limb images
__global__ __launch_bounds__(64) void k_c448_law_selftest(const int32_t* __restrict__ pts, const uint32_t* __restrict__ ctl, uint32_t n, int32_t* __restrict__ out) {
    wave_law_selftest<Curve448Curve>(pts, ctl, n, out);
}

}  // namespace dr
