// The host path of the wide suites (capi_blsg1.hip, capi_blsg2.hip, capi_ed448.hip): curves whose coordinates do not fit the 64-byte paths
// of capi_core.hip.  No kernel is defined here.  Each unit describes its suite in one struct S, named after capi_core.hip's Ed25519Suite
// where the meaning is the same, and its entry points are calls of the templates below.  S has
//   fe_bytes, elem_bytes, pt_bytes, scalar_bytes, limb_bytes   a base-field element, a hashed element (elem_bytes / fe_bytes components),
//                                                              a point, a scalar, a raw limb image of the field selftest
//   variant_ro, variant_nu, variant_names                      the two DR_CURVE_* ids, and how the refusal of another id spells them
//   max_map, max_points, max_decode                            batch limits (exclusive): map / encode, scalar_mul / msm_groups, decode / check
//   block, selftest_records; scalar_mul, msm_groups, field_selftest (kernels); k_scalar_mul, k_msm_groups, k_decode (launch names)
//   enc_bytes, rec_bytes, decode_gives_points, decode_checks_canonical   the flag-returning launch: an input, its zero-padded record on
//                                                              the device, whether points come back, whether inputs are field elements
//   canonical(p)                                               whether the fe_bytes at p are below the modulus
//   hash_to_field(variant, salt, salt_len, msg, len, out)      RFC 9380 section 5 with the suite's own parameters
//   map_flag_words(n, elems), map_launch(ctx, n, elems, per_item, clear)   the flag words of the map in io_c (the first n the items') and
//                                                              its launches, elements in io_a, points to io_b
//   no_image                                                   the refusal of a message whose field elements have no image
// A suite without one of the operations leaves its members out: the templates are instantiated only where an entry point calls them.
// Secret scalars pass through io_a / io_b / io_c only (and G2's images through partial): what ctx_wipe_scratch covers.
#pragma once
#include "capi_internal.hpp"

namespace dri {

constexpr size_t WIDE_MAX_SELFTEST = 1ull << 24;       // the field selftests' batch limit

// BLS12-381's base field element (48 bytes little-endian) below p: shared by the G1 and G2 suites
inline bool fq_canonical(const uint8_t* p) {
    uint64_t v[6];
    std::memcpy(v, p, 48);
    return !drh::Fq::geq_p(v);
}

template <class S>
int wide_check_variant(int variant) {
    return variant == S::variant_ro || variant == S::variant_nu ? DR_OK : fail(DR_ERR_INVALID, std::string("variant must be ") + S::variant_names);
}
template <class S>
unsigned wide_elems_of(int variant) { return variant == S::variant_nu ? 1 : 2; }
// `bytes` of base-field elements at p, each below the modulus
template <class S>
int wide_check_canonical(const uint8_t* p, size_t bytes, const char* what) {
    for (size_t at = 0; at < bytes; at += S::fe_bytes)
        if (!S::canonical(p + at)) return fail(DR_ERR_INVALID, std::string(what) + " is not a canonical field element");
    return DR_OK;
}
inline int wide_check_offsets(const uint64_t* off, const uint64_t* salt_off, size_t count, const char* refusal) {
    for (size_t i = 0; i < count; i++)
        if (off[i + 1] < off[i] || (salt_off && salt_off[i + 1] < salt_off[i])) return fail(DR_ERR_INVALID, refusal);
    return DR_OK;
}

template <class S>
int wide_hash_to_field_batch(int variant, const uint8_t* msgs, const uint64_t* off, size_t count, uint8_t* out) {
    TRY(wide_check_variant<S>(variant));
    if (count == 0) return DR_OK;
    if (!off || !out || (off[count] && !msgs)) return fail(DR_ERR_INVALID, "null buffer");
    TRY(wide_check_offsets(off, nullptr, count, "message offsets must not decrease"));
    const size_t per = wide_elems_of<S>(variant);
    drh::parallel_for(count, [&](size_t i) { S::hash_to_field(variant, nullptr, 0, msgs + off[i], off[i + 1] - off[i], out + S::elem_bytes * per * i); });
    return DR_OK;
}

// n items of per_item canonical elements at `us` (host): the suite's launches of the map, points and flags back
template <class S>
int wide_map(dr_ctx* ctx, const uint8_t* us, size_t n, int per_item, int clear, uint8_t* out_xy, uint8_t* ok) {
    const size_t elems = n * (size_t)per_item;
    TRY(ctx->io_a.reserve(elems * S::elem_bytes));
    TRY(ctx->io_b.reserve(n * S::pt_bytes));
    TRY(ctx->io_c.reserve(S::map_flag_words(n, elems) * 4));
    HIP_TRY(hipMemcpyAsync(ctx->io_a.p, us, elems * S::elem_bytes, hipMemcpyHostToDevice, ctx->stream));
    TRY(S::map_launch(ctx, n, elems, per_item, clear));
    return finish_flagged(ctx, out_xy, ctx->io_b.p, n * S::pt_bytes, ctx->io_c.p, n, ok);
}
template <class S>
int wide_map_to_curve(dr_ctx* ctx, const uint8_t* us, size_t n, int per_item, int clear, uint8_t* out_xy, uint8_t* ok) {
    TRY(use_ctx(ctx));
    if (per_item != 1 && per_item != 2) return fail(DR_ERR_INVALID, "one (nonuniform) or two (uniform, RO) field elements per item");
    if (n == 0) return DR_OK;
    if (!us || !out_xy || !ok) return fail(DR_ERR_INVALID, "null buffer");
    if (n >= S::max_map) return fail(DR_ERR_INVALID, "batch too large");
    TRY(wide_check_canonical<S>(us, n * (size_t)per_item * S::elem_bytes, "input"));
    return wide_map<S>(ctx, us, n, per_item, clear, out_xy, ok);
}
template <class S>
int wide_encode_to_curve_batch(dr_ctx* ctx, int variant, const uint8_t* msgs, const uint64_t* off, const uint8_t* salts, const uint64_t* salt_off,
                               size_t count, uint8_t* out_xy) {
    TRY(use_ctx(ctx));
    TRY(wide_check_variant<S>(variant));
    if (count == 0) return DR_OK;
    if (!off || !out_xy || (off[count] && !msgs) || (salts && !salt_off)) return fail(DR_ERR_INVALID, "null buffer");
    if (count >= S::max_map) return fail(DR_ERR_INVALID, "batch too large");
    TRY(wide_check_offsets(off, salts ? salt_off : nullptr, count, "offsets must not decrease"));
    const size_t per = wide_elems_of<S>(variant);
    std::vector<uint8_t> us(count * per * S::elem_bytes), ok(count);
    drh::parallel_for(count, [&](size_t i) {
        S::hash_to_field(variant, salts ? salts + salt_off[i] : nullptr, salts ? salt_off[i + 1] - salt_off[i] : 0, msgs + off[i], off[i + 1] - off[i],
                         us.data() + S::elem_bytes * per * i);
    });
    TRY(wide_map<S>(ctx, us.data(), count, (int)per, 1, out_xy, ok.data()));
    for (size_t i = 0; i < count; i++)
        if (!ok[i]) return fail(DR_ERR_INVALID, S::no_image);
    return DR_OK;
}

// n points (coordinates checked) and n scalars to io_a / io_b, one launch (`go`, profiled as `name`) into io_c, n_out points back
template <class S, class F>
int wide_run_points(dr_ctx* ctx, const char* name, const uint8_t* pts_xy, const uint8_t* scalars, size_t n, size_t n_out, uint8_t* out_xy, F&& go) {
    if (!pts_xy || !scalars || !out_xy) return fail(DR_ERR_INVALID, "null buffer");
    if (n >= S::max_points) return fail(DR_ERR_INVALID, "batch too large");
    TRY(wide_check_canonical<S>(pts_xy, n * S::pt_bytes, "point coordinate"));
    TRY(ctx->io_a.reserve(n * S::pt_bytes));
    TRY(ctx->io_b.reserve(n * S::scalar_bytes));
    TRY(ctx->io_c.reserve(n_out * S::pt_bytes));
    HIP_TRY(hipMemcpyAsync(ctx->io_a.p, pts_xy, n * S::pt_bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(ctx->io_b.p, scalars, n * S::scalar_bytes, hipMemcpyHostToDevice, ctx->stream));
    TRY(launch(ctx, name, go));
    HIP_TRY(hipMemcpyAsync(out_xy, ctx->io_c.p, n_out * S::pt_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (ctx->prof) TRY(prof_collect(ctx));
    return DR_OK;
}
template <class S>
int wide_scalar_mul_batch(dr_ctx* ctx, const uint8_t* pts_xy, const uint8_t* scalars, size_t n, uint8_t* out_xy) {
    TRY(use_ctx(ctx));
    if (n == 0) return DR_OK;
    return wide_run_points<S>(ctx, S::k_scalar_mul, pts_xy, scalars, n, n, out_xy, [&] {
        hipLaunchKernelGGL(S::scalar_mul, dim3(div_up(n, S::block)), dim3(S::block), 0, ctx->stream, ctx->io_a.as<uint32_t>(), ctx->io_b.as<uint32_t>(),
                           ctx->io_c.as<uint32_t>(), (uint32_t)n);
    });
}
template <class S>
int wide_msm_groups(dr_ctx* ctx, const uint8_t* pts_xy, const uint8_t* scalars, size_t groups, size_t m, uint8_t* out_xy) {
    TRY(use_ctx(ctx));
    if (groups == 0) return DR_OK;
    if (m == 0 || m > 64) return fail(DR_ERR_INVALID, "group size must be in 1..64");
    if (groups >= S::max_points || groups * m >= S::max_points) return fail(DR_ERR_INVALID, "batch too large");
    uint32_t mpad = 1;
    while (mpad < m) mpad <<= 1;
    const uint32_t per_block = S::block / mpad;
    return wide_run_points<S>(ctx, S::k_msm_groups, pts_xy, scalars, groups * m, groups, out_xy, [&] {
        hipLaunchKernelGGL(S::msm_groups, dim3(div_up(groups, per_block)), dim3(S::block), 0, ctx->stream, ctx->io_a.as<uint32_t>(),
                           ctx->io_b.as<uint32_t>(), ctx->io_c.as<uint32_t>(), (uint32_t)groups, (uint32_t)m, mpad);
    });
}

// The flag-returning launches (the G1 and Ed448 decoders, G2's check_points): n inputs of S::enc_bytes to io_a, each zero-padded to
// S::rec_bytes, one launch (`go`, profiled as S::k_decode) with the flag words in io_c and, for a decoder, the points in io_b
template <class S, class F>
int wide_flagged(dr_ctx* ctx, const uint8_t* in, size_t n, uint8_t* out_xy, uint8_t* ok, F&& go) {
    TRY(use_ctx(ctx));
    if (n == 0) return DR_OK;
    if (!in || (S::decode_gives_points && !out_xy) || !ok) return fail(DR_ERR_INVALID, "null buffer");
    if (n >= S::max_decode) return fail(DR_ERR_INVALID, "batch too large");
    if (S::decode_checks_canonical) TRY(wide_check_canonical<S>(in, n * S::enc_bytes, "point coordinate"));
    std::vector<uint8_t> rec;
    if (S::rec_bytes != S::enc_bytes) {
        rec.assign(n * S::rec_bytes, 0);
        for (size_t i = 0; i < n; i++) std::memcpy(rec.data() + S::rec_bytes * i, in + S::enc_bytes * i, S::enc_bytes);
        in = rec.data();
    }
    TRY(ctx->io_a.reserve(n * S::rec_bytes));
    if (S::decode_gives_points) TRY(ctx->io_b.reserve(n * S::pt_bytes));
    TRY(ctx->io_c.reserve(n * 4));
    HIP_TRY(hipMemcpyAsync(ctx->io_a.p, in, n * S::rec_bytes, hipMemcpyHostToDevice, ctx->stream));
    TRY(launch(ctx, S::k_decode, go));
    return finish_flagged(ctx, S::decode_gives_points ? out_xy : nullptr, ctx->io_b.p, n * S::pt_bytes, ctx->io_c.p, n, ok);
}

// n pairs of raw limb images in, S::selftest_records results of elem_bytes and one flag byte per pair out (not profiled)
template <class S>
int wide_field_selftest(dr_ctx* ctx, const int32_t* a_limbs, const int32_t* b_limbs, size_t n, uint8_t* out, uint8_t* flags) {
    TRY(use_ctx(ctx));
    if (n == 0) return DR_OK;
    if (!a_limbs || !b_limbs || !out || !flags) return fail(DR_ERR_INVALID, "null buffer");
    if (n >= WIDE_MAX_SELFTEST) return fail(DR_ERR_INVALID, "batch too large");
    constexpr size_t rec = (size_t)S::selftest_records * S::elem_bytes;
    TRY(ctx->io_a.reserve(n * 2 * S::limb_bytes));
    TRY(ctx->io_b.reserve(n * rec));
    TRY(ctx->io_c.reserve(n * 4));
    HIP_TRY(hipMemcpyAsync(ctx->io_a.p, a_limbs, n * S::limb_bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(ctx->io_a.as<uint8_t>() + n * S::limb_bytes, b_limbs, n * S::limb_bytes, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(S::field_selftest, dim3(div_up(n, 64)), dim3(64), 0, ctx->stream, ctx->io_a.as<int32_t>(),
                       (const int32_t*)(ctx->io_a.as<uint8_t>() + n * S::limb_bytes), (uint32_t)n, ctx->io_b.as<uint32_t>(), ctx->io_c.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    std::vector<uint32_t> fl(n);
    TRY(download_flagged(ctx, out, ctx->io_b.p, n * rec, ctx->io_c.p, fl));
    for (size_t i = 0; i < n; i++) flags[i] = (uint8_t)fl[i];
    return DR_OK;
}

}  // namespace dri
