// The one host path of every suite's single-launch entry points: the five 256-bit suites of capi_native256.hip (Ed25519, P-256, Baby JubJub,
// secp256k1, Curve25519) and the wide ones (capi_blsg1.hip, capi_blsg2.hip, capi_ed448.hip, capi_p521.hip, capi_p384.hip), whose coordinates do not fit 64-byte points.
// No kernel is defined here.  A unit describes its suite in one struct S and its entry points are calls of the templates below; every one
// of them is one io_round (capi_internal.hpp).  S has
//   fe_bytes, elem_bytes, pt_bytes, scalar_bytes, limb_bytes   a base-field element, a hashed element (elem_bytes / fe_bytes components),
//                                                              a point, a scalar, a raw limb image of the field selftest
//   max_map, max_points, max_decode                            batch limits (exclusive): map / encode, scalar_mul / msm_groups, decode / check
//   limit_first                                                msm_groups compares its sizes with max_points before it looks for null buffers
//   block, selftest_records; scalar_mul, msm_groups, field_selftest (kernels); k_scalar_mul, k_msm_groups, k_decode (launch names)
//   law_selftest (kernel), law_coords, law_slots               the diagnostic of the group law on raw limb images: the coordinates of a
//                                                              point (3, or 4 with t) and wave_curve.hip.h's WAVE_LAW_SLOTS
//   enc_bytes, rec_bytes, decode_gives_points, decode_checks_canonical   the flag-returning launch: an input, its zero-padded record on
//                                                              the device, whether points come back, whether inputs are field elements
//   canonical(p)                                               whether the fe_bytes at p are below the modulus
//   consts_ready(ctx)                                          device constants a decoder or the selftest needs (SuiteDefaults: none)
//   flagged                                                    the kernels carry an identity flag word beside each point (Curve25519, Curve448)
//   checks_scalars; scalars_ok(scalars, n), scalar_refusal     whether the suite bounds its scalars (P-521: below 2^521), the check and its text
//   map_flag_words(n, elems), map_launch(ctx, n, elems, per_item, clear)   the flag words of the map in io_c (the first n the items') and
//                                                              its launches, elements in io_a, points to io_b
// and a wide suite, for its hashing,
//   variant_ro, variant_nu, variant_names                      the two DR_CURVE_* ids, and how the refusal of another id spells them
//   hash_to_field(variant, salt, salt_len, msg, len, out)      RFC 9380 section 5 with the suite's own parameters
//   no_image                                                   the refusal of a message whose field elements have no image
// A suite without one of the operations leaves its members out: the templates are instantiated only where an entry point calls them.
// The caller has made the context current (use_ctx) before scalar_mul_batch and msm_groups; the other templates do it themselves.
// Secret scalars pass through io_a / io_b / io_c only (and G2's images through partial): what ctx_wipe_scratch covers.
#pragma once
#include "capi_internal.hpp"
#include "hostrecords.hpp"

namespace dri {

struct SuiteDefaults {
    static int consts_ready(dr_ctx*) { return DR_OK; }
    static constexpr bool flagged = false;
    static constexpr bool checks_scalars = false;      // true: run_points asks S::scalars_ok(scalars, n) before anything is uploaded
    // the bucket method (capi_wide_msm.hpp) as dr_wide_msm runs it: from WIDE_PIP_FROM terms, set sums out as records of limb images,
    // and the profile names of prepare, sort, accumulate, reduce and fold (none: the fold is timed with the reduction)
    static constexpr bool wide_affine = false;
    static constexpr size_t wide_from = dr::WIDE_PIP_FROM;
    static constexpr const char* wide_names[5] = {"k_wide_msm_prepare", "k_wide_msm_sort", "k_wide_msm_accumulate", "k_wide_msm_reduce", nullptr};
    // the law diagnostic's scratch in io_c per LANE of its launch, handed to the kernel as a fifth operand (G2: one record of the bucket
    // method, where the other curves' diagnostic goes through the LDS table)
    static constexpr size_t law_lane_bytes = 0;
};

// BLS12-381's base field element (48 bytes little-endian) below p: shared by the G1 and G2 suites
inline bool fq_canonical(const uint8_t* p) {
    uint64_t v[6];
    std::memcpy(v, p, 48);
    return !drh::Fq::geq_p(v);
}

template <class S>
int check_variant(int variant) {
    return variant == S::variant_ro || variant == S::variant_nu ? DR_OK : fail(DR_ERR_INVALID, std::string("variant must be ") + S::variant_names);
}
template <class S>
unsigned elems_of(int variant) { return variant == S::variant_nu ? 1 : 2; }
// `bytes` of base-field elements at p, each below the modulus
template <class S>
int check_canonical(const uint8_t* p, size_t bytes, const char* what) {
    for (size_t at = 0; at < bytes; at += S::fe_bytes)
        if (!S::canonical(p + at)) return fail(DR_ERR_INVALID, std::string(what) + " is not a canonical field element");
    return DR_OK;
}
inline int check_offsets(const uint64_t* off, const uint64_t* salt_off, size_t count, const char* refusal) {
    for (size_t i = 0; i < count; i++)
        if (off[i + 1] < off[i] || (salt_off && salt_off[i + 1] < salt_off[i])) return fail(DR_ERR_INVALID, refusal);
    return DR_OK;
}

template <class S>
int hash_to_field_batch(int variant, const uint8_t* msgs, const uint64_t* off, size_t count, uint8_t* out) {
    TRY(check_variant<S>(variant));
    if (count == 0) return DR_OK;
    if (!off || !out || (off[count] && !msgs)) return fail(DR_ERR_INVALID, "null buffer");
    TRY(check_offsets(off, nullptr, count, "message offsets must not decrease"));
    const size_t per = elems_of<S>(variant);
    drh::parallel_for(count, [&](size_t i) { S::hash_to_field(variant, nullptr, 0, msgs + off[i], off[i + 1] - off[i], out + S::elem_bytes * per * i); });
    return DR_OK;
}

// n items of per_item canonical elements at `us` (host): the suite's launches of the map, points and flags back
template <class S>
int map_round(dr_ctx* ctx, const uint8_t* us, size_t n, int per_item, int clear, uint8_t* out_xy, uint8_t* ok) {
    const size_t elems = n * (size_t)per_item;
    return io_round_flagged(ctx, {elems * S::elem_bytes, n * S::pt_bytes, S::map_flag_words(n, elems) * 4}, {{&ctx->io_a, 0, us, elems * S::elem_bytes}},
                            nullptr, [&] { return S::map_launch(ctx, n, elems, per_item, clear); }, {out_xy, &ctx->io_b, 0, n * S::pt_bytes}, n, ok);
}
template <class S>
int map_to_curve(dr_ctx* ctx, const uint8_t* us, size_t n, int per_item, int clear, uint8_t* out_xy, uint8_t* ok) {
    TRY(use_ctx(ctx));
    if (per_item != 1 && per_item != 2) return fail(DR_ERR_INVALID, "one (nonuniform) or two (uniform, RO) field elements per item");
    if (n == 0) return DR_OK;
    if (!us || !out_xy || !ok) return fail(DR_ERR_INVALID, "null buffer");
    if (n >= S::max_map) return fail(DR_ERR_INVALID, "batch too large");
    TRY(check_canonical<S>(us, n * (size_t)per_item * S::elem_bytes, "input"));
    return map_round<S>(ctx, us, n, per_item, clear, out_xy, ok);
}
template <class S>
int encode_to_curve_batch(dr_ctx* ctx, int variant, const uint8_t* msgs, const uint64_t* off, const uint8_t* salts, const uint64_t* salt_off,
                          size_t count, uint8_t* out_xy) {
    TRY(use_ctx(ctx));
    TRY(check_variant<S>(variant));
    if (count == 0) return DR_OK;
    if (!off || !out_xy || (off[count] && !msgs) || (salts && !salt_off)) return fail(DR_ERR_INVALID, "null buffer");
    if (count >= S::max_map) return fail(DR_ERR_INVALID, "batch too large");
    TRY(check_offsets(off, salts ? salt_off : nullptr, count, "offsets must not decrease"));
    const size_t per = elems_of<S>(variant);
    std::vector<uint8_t> us(count * per * S::elem_bytes), ok(count);
    drh::parallel_for(count, [&](size_t i) {
        S::hash_to_field(variant, salts ? salts + salt_off[i] : nullptr, salts ? salt_off[i + 1] - salt_off[i] : 0, msgs + off[i], off[i + 1] - off[i],
                         us.data() + S::elem_bytes * per * i);
    });
    TRY(map_round<S>(ctx, us.data(), count, (int)per, 1, out_xy, ok.data()));
    for (size_t i = 0; i < count; i++)
        if (!ok[i]) return fail(DR_ERR_INVALID, S::no_image);
    return DR_OK;
}

// The identity flags of a flagged suite's call when the caller spells them out (the dr_curve25519_* entry points; the dr_curve448_* ones do not): one byte per point in
// (null: none is the identity) and out.  Without them the identity travels inside the point, as pt_bytes of 0xff (drh::mont_is_identity).
struct IdentityFlags {
    const uint8_t* in = nullptr;
    uint8_t* out = nullptr;
};
// n points (coordinates checked) and n scalars to io_a / io_b, one launch (`go`, profiled as `name`) into io_c, n_out points back
template <class S, class F>
int run_points(dr_ctx* ctx, const char* name, const uint8_t* pts_xy, const uint8_t* scalars, size_t n, size_t n_out, uint8_t* out_xy, F&& go,
               const IdentityFlags* fl = nullptr) {
    if (!pts_xy || !scalars || !out_xy) return fail(DR_ERR_INVALID, "null buffer");
    if (n >= S::max_points) return fail(DR_ERR_INVALID, "batch too large");
    if constexpr (S::checks_scalars) {
        if (!S::scalars_ok(scalars, n)) return fail(DR_ERR_INVALID, S::scalar_refusal);
    }
    if constexpr (S::flagged) {
        // the identities among the points become flag words behind the points in io_a (their bytes zeros), and the flag words the kernel
        // leaves behind its results in io_c become identities again; with the caller's own flags (fl) the points go as they are, so that
        // a point of 0xff bytes is refused below like every other coordinate at or above p
        std::vector<uint8_t> clean;
        std::vector<uint32_t> flags_in, flags_out(n_out);
        drh::split_identities(pts_xy, n, S::pt_bytes, fl != nullptr, fl ? fl->in : nullptr, clean, flags_in);
        if (!clean.empty()) pts_xy = clean.data();
        TRY(check_canonical<S>(pts_xy, n * S::pt_bytes, "point coordinate"));
        TRY(io_round(ctx, {n * (S::pt_bytes + 4), n * S::scalar_bytes, n_out * (S::pt_bytes + 4)},
                     {{&ctx->io_a, 0, pts_xy, n * S::pt_bytes}, {&ctx->io_a, n * S::pt_bytes, flags_in.data(), n * 4}, {&ctx->io_b, 0, scalars, n * S::scalar_bytes}},
                     name, go, {{out_xy, &ctx->io_c, 0, n_out * S::pt_bytes}, {flags_out.data(), &ctx->io_c, n_out * S::pt_bytes, n_out * 4}}));
        for (size_t i = 0; i < n_out; i++) {
            if (fl) fl->out[i] = flags_out[i] ? 1 : 0;                         // (the kernel stored zero bytes)
            else if (flags_out[i]) std::memset(out_xy + S::pt_bytes * i, 0xff, S::pt_bytes);
        }
        return DR_OK;
    } else {
        TRY(check_canonical<S>(pts_xy, n * S::pt_bytes, "point coordinate"));
        return io_round(ctx, {n * S::pt_bytes, n * S::scalar_bytes, n_out * S::pt_bytes},
                        {{&ctx->io_a, 0, pts_xy, n * S::pt_bytes}, {&ctx->io_b, 0, scalars, n * S::scalar_bytes}}, name, go,
                        {{out_xy, &ctx->io_c, 0, n_out * S::pt_bytes}});
    }
}
// the kernels' operands: points in io_a, scalars in io_b, results in io_c; a flagged suite's flag words behind the n_in points and the
// n_out results
template <class S, class K, class... Tail>
void launch_points(dr_ctx* ctx, K kernel, size_t blocks, size_t n_in, size_t n_out, Tail... tail) {
    if constexpr (S::flagged)
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(S::block), 0, ctx->stream, ctx->io_a.as<uint32_t>(), ctx->io_b.as<uint32_t>(),
                           ctx->io_a.as<uint32_t>() + n_in * (S::pt_bytes / 4), ctx->io_c.as<uint32_t>(), ctx->io_c.as<uint32_t>() + n_out * (S::pt_bytes / 4),
                           tail...);
    else
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(S::block), 0, ctx->stream, ctx->io_a.as<uint32_t>(), ctx->io_b.as<uint32_t>(),
                           ctx->io_c.as<uint32_t>(), tail...);
}
template <class S>
int scalar_mul_batch(dr_ctx* ctx, const uint8_t* pts_xy, const uint8_t* scalars, size_t n, uint8_t* out_xy, const IdentityFlags* fl = nullptr) {
    if (n == 0) return DR_OK;
    return run_points<S>(ctx, S::k_scalar_mul, pts_xy, scalars, n, n, out_xy,
                         [&] { launch_points<S>(ctx, S::scalar_mul, div_up(n, S::block), n, n, (uint32_t)n); }, fl);
}
template <class S>
int msm_groups(dr_ctx* ctx, const uint8_t* pts_xy, const uint8_t* scalars, size_t groups, size_t m, uint8_t* out_xy, const IdentityFlags* fl = nullptr) {
    if (groups == 0) return DR_OK;
    if (m == 0 || m > 64) return fail(DR_ERR_INVALID, "group size must be in 1..64");
    if (S::limit_first && (groups >= S::max_points || groups * m >= S::max_points)) return fail(DR_ERR_INVALID, "batch too large");
    uint32_t mpad = 1;
    while (mpad < m) mpad <<= 1;
    const uint32_t per_block = S::block / mpad;
    return run_points<S>(ctx, S::k_msm_groups, pts_xy, scalars, groups * m, groups, out_xy, [&] {
        launch_points<S>(ctx, S::msm_groups, div_up(groups, per_block), groups * m, groups, (uint32_t)groups, (uint32_t)m, mpad);
    }, fl);
}

// The flag-returning launches (the decoders, G2's and Ed448's check_points): n inputs of S::enc_bytes to io_a, each zero-padded to
// S::rec_bytes, one launch (`go`, profiled as S::k_decode) with the flag words in io_c and, for a decoder, the points in io_b
template <class S, class F>
int flagged_round(dr_ctx* ctx, const uint8_t* in, size_t n, uint8_t* out_xy, uint8_t* ok, F&& go) {
    TRY(use_ctx(ctx));
    if (n == 0) return DR_OK;
    if (!in || (S::decode_gives_points && !out_xy) || !ok) return fail(DR_ERR_INVALID, "null buffer");
    if (n >= S::max_decode) return fail(DR_ERR_INVALID, "batch too large");
    TRY(S::consts_ready(ctx));
    if (S::decode_checks_canonical) TRY(check_canonical<S>(in, n * S::enc_bytes, "point coordinate"));
    std::vector<uint8_t> rec;
    if (S::rec_bytes != S::enc_bytes) {
        rec = drh::pad_records(in, n, S::enc_bytes, S::rec_bytes);
        in = rec.data();
    }
    return io_round_flagged(ctx, {n * S::rec_bytes, S::decode_gives_points ? n * S::pt_bytes : 0, n * 4}, {{&ctx->io_a, 0, in, n * S::rec_bytes}}, S::k_decode,
                            go, {S::decode_gives_points ? out_xy : nullptr, &ctx->io_b, 0, n * S::pt_bytes}, n, ok);
}
// ... with one of the suite's decoder kernels (points to io_b)
template <class S, class K>
int decode_points(dr_ctx* ctx, K kernel, const uint8_t* enc, size_t n, uint8_t* out_xy, uint8_t* ok) {
    return flagged_round<S>(ctx, enc, n, out_xy, ok, [&] {
        hipLaunchKernelGGL(kernel, dim3(div_up(n, S::block)), dim3(S::block), 0, ctx->stream, ctx->io_a.as<uint32_t>(), ctx->io_b.as<uint32_t>(),
                           ctx->io_c.as<uint32_t>(), (uint32_t)n);
    });
}

// n pairs of raw limb images in, S::selftest_records results of elem_bytes and one flag byte (the kernel's word, cut) per pair out; not profiled
template <class S>
int field_selftest(dr_ctx* ctx, const int32_t* a_limbs, const int32_t* b_limbs, size_t n, uint8_t* out, uint8_t* flags) {
    TRY(use_ctx(ctx));
    if (n == 0) return DR_OK;
    if (!a_limbs || !b_limbs || !out || !flags) return fail(DR_ERR_INVALID, "null buffer");
    if (n >= MAX_SELFTEST) return fail(DR_ERR_INVALID, "batch too large");
    TRY(S::consts_ready(ctx));
    constexpr size_t rec = (size_t)S::selftest_records * S::elem_bytes;
    return io_round_flagged(ctx, {n * 2 * S::limb_bytes, n * rec, n * 4},
                            {{&ctx->io_a, 0, a_limbs, n * S::limb_bytes}, {&ctx->io_a, n * S::limb_bytes, b_limbs, n * S::limb_bytes}}, nullptr, [&] {
        hipLaunchKernelGGL(S::field_selftest, dim3(div_up(n, 64)), dim3(64), 0, ctx->stream, ctx->io_a.as<int32_t>(),
                           (const int32_t*)(ctx->io_a.as<uint8_t>() + n * S::limb_bytes), (uint32_t)n, ctx->io_b.as<uint32_t>(), ctx->io_c.as<uint32_t>());
    }, {out, &ctx->io_b, 0, n * rec}, n, flags, false);
}

// wave_curve.hip.h's wave_law_selftest over the suite's curve: n records of S::law_coords coordinates for P and as many for Q, raw limb
// images of S::limb_bytes each, and n control words in; n x S::law_slots (wave_curve.hip.h's WAVE_LAW_SLOTS) points in the same form out; not profiled.
// A suite with law_lane_bytes gives a kernel of the same shape that takes its per-lane scratch (io_c) as a fifth operand.
template <class S>
int law_selftest(dr_ctx* ctx, const int32_t* points, const uint32_t* controls, size_t n, int32_t* out) {
    TRY(use_ctx(ctx));
    if (n == 0) return DR_OK;
    if (!points || !controls || !out) return fail(DR_ERR_INVALID, "null buffer");
    if (n >= MAX_SELFTEST) return fail(DR_ERR_INVALID, "batch too large");
    TRY(S::consts_ready(ctx));
    constexpr size_t pt = (size_t)S::law_coords * S::limb_bytes;
    return io_round(ctx, {n * (2 * pt + 4), n * S::law_slots * pt, (size_t)div_up(n, 64) * 64 * S::law_lane_bytes},
                    {{&ctx->io_a, 0, points, n * 2 * pt}, {&ctx->io_a, n * 2 * pt, controls, n * 4}}, nullptr, [&] {
        if constexpr (S::law_lane_bytes != 0)
            hipLaunchKernelGGL(S::law_selftest, dim3(div_up(n, 64)), dim3(64), 0, ctx->stream, ctx->io_a.as<int32_t>(),
                               (const uint32_t*)(ctx->io_a.as<uint8_t>() + n * 2 * pt), (uint32_t)n, ctx->io_b.as<int32_t>(), ctx->io_c.as<uint32_t>());
        else
            hipLaunchKernelGGL(S::law_selftest, dim3(div_up(n, 64)), dim3(64), 0, ctx->stream, ctx->io_a.as<int32_t>(),
                               (const uint32_t*)(ctx->io_a.as<uint8_t>() + n * 2 * pt), (uint32_t)n, ctx->io_b.as<int32_t>());
    }, {{out, &ctx->io_b, 0, n * S::law_slots * pt}});
}

}  // namespace dri
