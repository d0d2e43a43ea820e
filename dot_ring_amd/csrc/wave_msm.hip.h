// The bucket method for ONE variable-base MSM as one set of templates over wave_curve.hip.h's description C of the curve (Point, add,
// cneg, identity, to_lds / from_lds, LDS_WORDS, EXTENDED) where kernels_te_msm.hip.h is the same method over Bandersnatch's own field:
//   the wide suites — P-384, P-521, Ed448, Curve448 — from WIDE_PIP_FROM terms (dr_wide_msm);
//   the 256-bit suites — Ed25519, Baby JubJub, P-256, secp256k1, and Curve25519 on Ed25519's stages — and BLS12-381's E(Fq) and E(Fq2)
//     from NARROW_PIP_FROM / BLSG2_PIP_FROM terms (dr_te_msm, dr_blsg1_msm, dr_blsg2_msm).
// Their kernel headers expand DR_WAVE_MSM_KERNELS or DR_WAVE_MSM_KERNELS_RECORDS below: one thin named __global__ per stage
// (kernels_curve448.hip.h writes its own out).
// The plan is msm_plan.hpp's plan_wide_msm, the digits are wide_recode.hip.h's, the host side is capi_wide_msm.hpp:
//   prepare      one lane per term: the ABI's point -> a projective RECORD of limb images (x, y, z and, where the description is
//                EXTENDED, t: 3 or 4 x LDS_WORDS words as to_lds gives them, padded to whole uint4).  Walks read records, so the
//                birational maps of Curve448 and Curve25519 and their exceptional points are paid once per term.  (The suites' kernels
//                load the point; wave_msm_put stores it.)
//   sort         one workgroup per bucket set (window, index group): histogram, scan and placement of the set's digits in LDS.  Entries
//                are the term index with the digit's sign in bit 31.
//   accumulate   one lane per bucket, in the order of a size-sorted permutation, walks its list with C::add, negating by C::cneg; lists
//                longer than TE_HEAVY_BUCKET are left to accumulate_heavy, where a whole wave strides over the list and folds its 64 sums
//                with wave_shfl_down.  All the laws are complete or unified: equal points, inverse pairs and identities in a list are
//                additions like any other.
//   reduce       per (set, chunk of L buckets): running sums + the chunk's offset multiple (double-and-add over the bits of the offset)
//   fold         one lane per set adds its chunk results; the W x G set sums leave the device as records (the wide suites, whose laws
//                compile for the host) or as the ABI's affine points (fold_affine: the suites whose host law runs over another form)
// The host combines index groups and windows with the suite's own law (a chain of ~bits doublings: one CPU core is far faster at that
// than one GPU lane).
//
// NOT a fixed schedule, exactly as dr_te_msm on Bandersnatch is not from 256 terms: which bucket a term goes to, how long a list is and
// which kernel walks it all depend on the scalars.  The provers' secret scalars never come here (they go through scalar_mul_batch and
// msm_groups); the verifiers' scalars are public.
#pragma once
#include "msm_plan.hpp"
#include "wave_curve.hip.h"

namespace dr {

constexpr int WMSM_SORT_BLOCK = 256;
constexpr int WMSM_BLOCK = 64;            // accumulate, reduce, fold: one wave per workgroup (the laws take 128 registers and more)

template <class C>
constexpr int wave_msm_record_words() { return ((C::EXTENDED ? 4 : 3) * C::LDS_WORDS + 3) & ~3; }

template <class C>
DR_DEV void wave_msm_put(uint32_t* __restrict__ recs, size_t idx, const typename C::Point& p) {
    constexpr int W = C::LDS_WORDS, N = C::EXTENDED ? 4 : 3, R = wave_msm_record_words<C>();
    [[maybe_unused]] uint32_t x[W], y[W], z[W], t[W], w[R];
    C::to_lds(p.x, x); C::to_lds(p.y, y); C::to_lds(p.z, z);
    if constexpr (C::EXTENDED) C::to_lds(p.t, t);
#pragma unroll
    for (int i = 0; i < W; i++) {
        w[i] = x[i]; w[W + i] = y[i]; w[2 * W + i] = z[i];
        if constexpr (C::EXTENDED) w[3 * W + i] = t[i];
    }
#pragma unroll
    for (int i = N * W; i < R; i++) w[i] = 0;
    wave_store_words(recs + idx * R, w);
}
template <class C>
DR_DEV typename C::Point wave_msm_get(const uint32_t* __restrict__ recs, size_t idx) {
    constexpr int W = C::LDS_WORDS, R = wave_msm_record_words<C>();
    [[maybe_unused]] uint32_t x[W], y[W], z[W], t[W], w[R];
    wave_load_words(recs + idx * R, w);
#pragma unroll
    for (int i = 0; i < W; i++) {
        x[i] = w[i]; y[i] = w[W + i]; z[i] = w[2 * W + i];
        if constexpr (C::EXTENDED) t[i] = w[3 * W + i];
    }
    typename C::Point p;
    p.x = C::from_lds(x); p.y = C::from_lds(y); p.z = C::from_lds(z);
    if constexpr (C::EXTENDED) p.t = C::from_lds(t);
    return p;
}

// the point half of wave_load_term: affine x || y (2 WORDS words, canonical); zero words are the identity where the ABI says so
template <class C>
DR_DEV typename C::Point wave_msm_load_point(const uint32_t* pt) {
    uint32_t x[C::WORDS], y[C::WORDS];
    wave_load_point_words(pt, x, y);
    [[maybe_unused]] uint32_t o = 0;
#pragma unroll
    for (int j = 0; j < C::WORDS; j++) o |= x[j] | y[j];
    typename C::Point r = C::from_affine(C::unpack(x), C::unpack(y));
    if constexpr (C::ZERO_IS_IDENTITY) {
        if (o == 0) r = C::identity();
    }
    return r;
}
template <class C>
DR_DEV void wave_msm_prepare(const uint32_t* __restrict__ pts, uint32_t n, uint32_t* __restrict__ table) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    wave_msm_put<C>(table, i, wave_msm_load_point<C>(pts + (size_t)i * (2 * C::WORDS)));
}

// ---------------------------------------------------------------- digits and sort
// exclusive scan over the workgroup's WMSM_SORT_BLOCK values; sums: one word per wave
DR_DEV uint32_t wave_msm_block_scan(uint32_t v, uint32_t* sums) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(inc, d, 64);
        if (lane >= d) inc += t;
    }
    if (lane == 63) sums[wv] = inc;
    __syncthreads();
    uint32_t base = 0;
    for (int j = 0; j < wv; j++) base += sums[j];
    return base + inc - v;
}
// Workgroup `set` = window w x index group g sorts the digits of window w of the terms [i_lo, i_hi) of its group by bucket: counts and
// offsets per bucket (offsets into `sorted`, where set s owns [s capacity, (s + 1) capacity)), entries = index | sign << 31.  Scalars
// are KW words each, used as they are; a lane reads the one or two words its window touches.  H <= WIDE_MAX_H, capacity >= i_hi - i_lo.
template <int KW>
DR_DEV void wave_msm_sort(const uint32_t* __restrict__ scalars, WideTiling wt, uint32_t n, uint32_t H, uint32_t groups, uint32_t capacity,
                          uint32_t* __restrict__ counts, uint32_t* __restrict__ offsets, uint32_t* __restrict__ sorted) {
    __shared__ uint32_t bins[WIDE_MAX_H];
    __shared__ uint32_t sums[WMSM_SORT_BLOCK / 64];
    const uint32_t set = blockIdx.x, g = set % groups;
    const int w = (int)(set / groups), start = wide_start(wt, w), width = wide_width(wt, w);
    const uint32_t i_lo = (uint32_t)(((uint64_t)g * n + groups - 1) / groups), i_hi = (uint32_t)(((uint64_t)(g + 1) * n + groups - 1) / groups);
    for (uint32_t j = threadIdx.x; j < H; j += WMSM_SORT_BLOCK) bins[j] = 0;
    __syncthreads();
    for (uint32_t i = i_lo + threadIdx.x; i < i_hi; i += WMSM_SORT_BLOCK) {
        const int32_t d = wide_digit(scalars + (size_t)i * KW, KW, start, width);
        if (d != 0) atomicAdd(&bins[(uint32_t)(d < 0 ? -d : d) - 1u], 1u);
    }
    __syncthreads();
    const uint32_t per = (H + WMSM_SORT_BLOCK - 1) / WMSM_SORT_BLOCK, lo = min(threadIdx.x * per, H), hi = min(lo + per, H);
    uint32_t local = 0;
    for (uint32_t j = lo; j < hi; j++) {
        const uint32_t c = bins[j];
        counts[(size_t)set * H + j] = c;
        local += c;
    }
    uint32_t run = wave_msm_block_scan(local, sums);
    const uint32_t base = set * capacity;
    for (uint32_t j = lo; j < hi; j++) {
        const uint32_t c = bins[j];
        bins[j] = run;                                  // becomes the placement cursor
        offsets[(size_t)set * H + j] = base + run;
        run += c;
    }
    __syncthreads();
    for (uint32_t i = i_lo + threadIdx.x; i < i_hi; i += WMSM_SORT_BLOCK) {
        const int32_t d = wide_digit(scalars + (size_t)i * KW, KW, start, width);
        if (d != 0) {
            const uint32_t pos = atomicAdd(&bins[(uint32_t)(d < 0 ? -d : d) - 1u], 1u);
            sorted[base + pos] = i | (d < 0 ? 0x80000000u : 0u);
        }
    }
}

// ---------------------------------------------------------------- accumulate
template <class C>
DR_DEV typename C::Point wave_msm_walk(const uint32_t* __restrict__ table, const uint32_t* __restrict__ sorted, uint32_t beg, uint32_t len,
                                       uint32_t first, uint32_t stride) {
    typename C::Point acc = C::identity();
#pragma unroll 1
    for (uint32_t p = first; p < len; p += stride) {
        const uint32_t e = sorted[beg + p];
        acc = C::add(acc, C::cneg(wave_msm_get<C>(table, e & 0x7fffffffu), (e >> 31) != 0));
    }
    return acc;
}
template <class C>
DR_DEV void wave_msm_accumulate(const uint32_t* __restrict__ table, const uint32_t* __restrict__ sorted, const uint32_t* __restrict__ offsets,
                                const uint32_t* __restrict__ counts, const uint32_t* __restrict__ perm, uint32_t* __restrict__ buckets,
                                size_t nbuckets) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nbuckets) return;
    const size_t b = perm[t];
    const uint32_t len = counts[b];
    if (len > TE_HEAVY_BUCKET) return;                               // the wave kernel takes it
    wave_msm_put<C>(buckets, b, wave_msm_walk<C>(table, sorted, offsets[b], len, 0, 1));
}
// one wave per bucket; returns at once unless the bucket is heavy
template <class C>
DR_DEV void wave_msm_accumulate_heavy(const uint32_t* __restrict__ table, const uint32_t* __restrict__ sorted, const uint32_t* __restrict__ offsets,
                                      const uint32_t* __restrict__ counts, uint32_t* __restrict__ buckets, size_t nbuckets) {
    const size_t b = blockIdx.x;
    if (b >= nbuckets) return;
    const uint32_t len = counts[b];
    if (len <= TE_HEAVY_BUCKET) return;
    typename C::Point acc = wave_msm_walk<C>(table, sorted, offsets[b], len, threadIdx.x, 64);
#pragma unroll 1
    for (unsigned d = 32; d >= 1; d >>= 1) acc = C::add(acc, wave_shfl_down<C>(acc, d));
    if (threadIdx.x == 0) wave_msm_put<C>(buckets, b, acc);
}

// ---------------------------------------------------------------- reduce and fold
// value of a bucket set = sum_j (j + 1) B_j.  Chunk [s, s + L): running sums give sum_j (j - s + 1) B_j and A = sum_j B_j; the chunk
// contributes that plus s A (double-and-add over the bits of s < H)
template <class C>
DR_DEV void wave_msm_reduce(const uint32_t* __restrict__ buckets, size_t sets, uint32_t H, uint32_t L, uint32_t* __restrict__ partial) {
    using Point = typename C::Point;
    const uint32_t T = H / L;
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= sets * T) return;
    const size_t set = gid / T;
    const uint32_t s = (uint32_t)(gid % T) * L;
    Point run = C::identity(), sum = C::identity();
#pragma unroll 1
    for (int j = (int)L - 1; j >= 0; j--) {
        run = C::add(run, wave_msm_get<C>(buckets, set * H + s + (uint32_t)j));
        sum = C::add(sum, run);
    }
    if (s != 0) {
        Point t = C::identity();
#pragma unroll 1
        for (int bit = 31 - __clz(s); bit >= 0; bit--) {
            t = C::dbl(t);
            if ((s >> bit) & 1) t = C::add(t, run);
        }
        sum = C::add(sum, t);
    }
    wave_msm_put<C>(partial, gid, sum);
}
template <class C>
DR_DEV typename C::Point wave_msm_fold_sum(const uint32_t* __restrict__ partial, size_t set, uint32_t T) {
    typename C::Point acc = wave_msm_get<C>(partial, set * T);
#pragma unroll 1
    for (uint32_t t = 1; t < T; t++) acc = C::add(acc, wave_msm_get<C>(partial, set * T + t));
    return acc;
}
template <class C>
DR_DEV void wave_msm_fold(const uint32_t* __restrict__ partial, size_t sets, uint32_t T, uint32_t* __restrict__ setsum) {
    const size_t set = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (set >= sets) return;
    wave_msm_put<C>(setsum, set, wave_msm_fold_sum<C>(partial, set, T));
}
// the same fold with the set sum stored as the ABI's affine point (2 WORDS canonical words: zero words for a Weierstrass identity, (0, 1)
// on an Edwards curve), for the suites whose host law is not over the device's limb form
template <class C>
DR_DEV void wave_msm_fold_affine(const uint32_t* __restrict__ partial, size_t sets, uint32_t T, uint32_t* __restrict__ setsum) {
    const size_t set = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (set >= sets) return;
    wave_store_affine<C>(setsum + set * (2 * C::WORDS), wave_msm_fold_sum<C>(partial, set, T));
}

// The stages' kernels k_NAME_msm_prepare, _sort, _accumulate, _accumulate_heavy, _reduce and _fold of a curve over its description C
// (scalars of C::SCALAR_WORDS words); each kernel header expands one of the two forms below once.
//   DR_WAVE_MSM_KERNELS          the fold stores affine points (NAME: ed, bjj, p256, secp256k1, blsg1, blsg2)
//   DR_WAVE_MSM_KERNELS_RECORDS  the fold stores records of limb images (NAME: p384, p521, ed448).  Curve448's stages stay written out in
//                                kernels_curve448.hip.h: its prepare takes the flag words and its sort is Ed448's.
#define DR_WAVE_MSM_KERNELS(NAME, C) DR_WAVE_MSM_KERNELS_FOLD(NAME, C, wave_msm_fold_affine)
#define DR_WAVE_MSM_KERNELS_RECORDS(NAME, C) DR_WAVE_MSM_KERNELS_FOLD(NAME, C, wave_msm_fold)
#define DR_WAVE_MSM_KERNELS_FOLD(NAME, C, FOLD)                                                                                                \
    __global__ __launch_bounds__(WMSM_BLOCK) void k_##NAME##_msm_prepare(const uint32_t* __restrict__ pts, uint32_t n, uint32_t* __restrict__ table) { \
        wave_msm_prepare<C>(pts, n, table);                                                                                                    \
    }                                                                                                                                          \
    __global__ __launch_bounds__(WMSM_SORT_BLOCK) void k_##NAME##_msm_sort(const uint32_t* __restrict__ scalars, WideTiling wt, uint32_t n, uint32_t H, \
                                                                           uint32_t groups, uint32_t capacity, uint32_t* __restrict__ counts,  \
                                                                           uint32_t* __restrict__ offsets, uint32_t* __restrict__ sorted) {    \
        wave_msm_sort<C::SCALAR_WORDS>(scalars, wt, n, H, groups, capacity, counts, offsets, sorted);                                          \
    }                                                                                                                                          \
    __global__ __launch_bounds__(WMSM_BLOCK) void k_##NAME##_msm_accumulate(const uint32_t* __restrict__ table, const uint32_t* __restrict__ sorted, \
                                                                            const uint32_t* __restrict__ offsets, const uint32_t* __restrict__ counts, \
                                                                            const uint32_t* __restrict__ perm, uint32_t* __restrict__ buckets, \
                                                                            size_t nbuckets) {                                                 \
        wave_msm_accumulate<C>(table, sorted, offsets, counts, perm, buckets, nbuckets);                                                       \
    }                                                                                                                                          \
    __global__ __launch_bounds__(64) void k_##NAME##_msm_accumulate_heavy(const uint32_t* __restrict__ table, const uint32_t* __restrict__ sorted, \
                                                                          const uint32_t* __restrict__ offsets, const uint32_t* __restrict__ counts, \
                                                                          uint32_t* __restrict__ buckets, size_t nbuckets) {                   \
        wave_msm_accumulate_heavy<C>(table, sorted, offsets, counts, buckets, nbuckets);                                                       \
    }                                                                                                                                          \
    __global__ __launch_bounds__(WMSM_BLOCK) void k_##NAME##_msm_reduce(const uint32_t* __restrict__ buckets, size_t sets, uint32_t H, uint32_t L, \
                                                                        uint32_t* __restrict__ partial) {                                      \
        wave_msm_reduce<C>(buckets, sets, H, L, partial);                                                                                      \
    }                                                                                                                                          \
    __global__ __launch_bounds__(WMSM_BLOCK) void k_##NAME##_msm_fold(const uint32_t* __restrict__ partial, size_t sets, uint32_t T,           \
                                                                      uint32_t* __restrict__ setsum) {                                         \
        FOLD<C>(partial, sets, T, setsum);                                                                                                     \
    }

}  // namespace dr
