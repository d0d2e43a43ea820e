// libdotring_hip.so — C ABI, part 8 of 11: the suites over p = 2^448 - 2^224 - 1.  Ed448 (DR_CURVE_ED448_RO / DR_CURVE_ED448_NU; the
// reference's specs/ed448.py) and Curve448 (DR_CURVE_CURVE448_RO / DR_CURVE_CURVE448_NU; specs/curve448.py).
// Field elements and coordinates are 56 bytes little-endian, canonical; points are affine, 112 bytes: Ed448's x || y with the identity
// (0, 1) as itself, Curve448's Montgomery u || v with the identity as 112 bytes of 0xff, in and out, at every dr_curve448_* entry point
// ((0, 0) is a point of that curve).  Scalars are 56 bytes used AS THEY ARE.  None of it goes through the 64-byte paths of capi_core.hip
// but through capi_suite.hpp.  The kernels are kernels_ed448.hip.h and kernels_curve448.hip.h over fe448.hip.h; the host does
// hash_to_field (expand_message_xof over SHAKE256, L = 84) on the worker threads and checks that inputs are canonical.  Scalars may be
// secret: they pass through io_a / io_b / io_c only, which ctx_wipe_scratch covers.
#include "capi_suite.hpp"
#include "capi_wide_msm.hpp"
#include "kernels_ed448.hip.h"
#include "kernels_curve448.hip.h"

using namespace dri;

namespace {

struct Ed448Suite : SuiteDefaults {
    static constexpr size_t fe_bytes = 56, elem_bytes = 56, pt_bytes = 112, scalar_bytes = 56, limb_bytes = 4 * dr::L448;
    static constexpr int variant_ro = DR_CURVE_ED448_RO, variant_nu = DR_CURVE_ED448_NU;
    static constexpr const char* variant_names = "DR_CURVE_ED448_RO or DR_CURVE_ED448_NU";
    static constexpr bool limit_first = true;
    static constexpr size_t max_map = 1ull << 28, max_points = 1ull << 29, max_decode = 1ull << 29;
    static constexpr auto scalar_mul = dr::k_ed448_scalar_mul;
    static constexpr auto msm_groups = dr::k_ed448_msm_groups;
    static constexpr auto field_selftest = dr::k_ed448_field_selftest;
    static constexpr auto law_selftest = dr::k_ed448_law_selftest;
    static constexpr int law_coords = 3, law_slots = dr::WAVE_LAW_SLOTS;
    static constexpr int block = dr::E448_BLOCK, selftest_records = dr::E448_SELFTEST_RECORDS;
    static constexpr const char *k_scalar_mul = "k_ed448_scalar_mul", *k_msm_groups = "k_ed448_msm_groups", *k_decode = "k_ed448_check_points";
    // the bucket method of dr_wide_msm (capi_wide_msm.hpp): the law on the host, the bits the tiling covers, the stages' kernels
    using Law = dr::E448Law;
    static constexpr int wide_bits = 449;
    DR_WAVE_MSM_STAGES_RECORDS(ed448);
    static constexpr size_t enc_bytes = pt_bytes, rec_bytes = pt_bytes;   // the decoder takes x || y as given: its kernel judges the range
    static constexpr bool decode_gives_points = true, decode_checks_canonical = false;
    // (a field element in {0, 1, p - 1}: kernels_ed448.hip.h, e448_ell2_map)
    static constexpr const char* no_image = "the map to the curve has no value for a message (Point is not on the curve)";
    static bool canonical(const uint8_t* p) {
        uint64_t v[7];
        std::memcpy(v, p, fe_bytes);
        for (int i = 6; i >= 0; i--)
            if (v[i] != drh::P448[i]) return v[i] < drh::P448[i];
        return false;
    }
    // RFC 9380 section 5.3.3: L = 84 bytes per element; the DST of the variant (the reference's hash_to_curve_dst: _RO_ replaced by _NU_)
    static void hash_to_field(int variant, const uint8_t* salt, size_t salt_len, const uint8_t* msg, size_t len, uint8_t* out) {
        const bool nu = variant == variant_nu;
        drh::hash_to_field_fe448(nu ? "QUUX-V01-CS02-with-edwards448_XOF:SHAKE256_ELL2_NU_" : "QUUX-V01-CS02-with-edwards448_XOF:SHAKE256_ELL2_RO_", 51,
                                 nu ? 1 : 2, salt, salt_len, msg, len, out);
    }
    static size_t map_flag_words(size_t n, size_t) { return n; }
    static int map_launch(dr_ctx* ctx, size_t n, size_t, int per_item, int clear) {
        return launch(ctx, "k_ed448_map_to_curve", [&] {
            hipLaunchKernelGGL(dr::k_ed448_map_to_curve, dim3(div_up(n, block)), dim3(block), 0, ctx->stream, ctx->io_a.as<uint32_t>(),
                               ctx->io_b.as<uint32_t>(), ctx->io_c.as<uint32_t>(), (uint32_t)n, (uint32_t)per_item, clear ? 1u : 0u);
        });
    }
};

// Curve448: the field, the widths and the limits are Ed448's; the kernels carry an identity flag word beside each point (flagged), which
// run_points makes of 112 bytes of 0xff and back.  The field selftest is Ed448's: there is none here; the law (c448_law.hip.h) has its own.
struct Curve448Suite : SuiteDefaults {
    static constexpr size_t fe_bytes = 56, elem_bytes = 56, pt_bytes = 112, scalar_bytes = 56, limb_bytes = 4 * dr::L448;
    static constexpr auto law_selftest = dr::k_c448_law_selftest;
    static constexpr int law_coords = 3, law_slots = dr::WAVE_LAW_SLOTS;
    static constexpr bool flagged = true;
    static constexpr int variant_ro = DR_CURVE_CURVE448_RO, variant_nu = DR_CURVE_CURVE448_NU;
    static constexpr const char* variant_names = "DR_CURVE_CURVE448_RO or DR_CURVE_CURVE448_NU";
    static constexpr bool limit_first = true;
    static constexpr size_t max_map = Ed448Suite::max_map, max_points = Ed448Suite::max_points, max_decode = Ed448Suite::max_decode;
    static constexpr auto scalar_mul = dr::k_c448_scalar_mul;
    static constexpr auto msm_groups = dr::k_c448_msm_groups;
    static constexpr int block = dr::E448_BLOCK;
    static constexpr const char *k_scalar_mul = "k_c448_scalar_mul", *k_msm_groups = "k_c448_msm_groups", *k_decode = "k_c448_decode_points";
    // the bucket method of dr_wide_msm (capi_wide_msm.hpp): the law on the host, the bits the tiling covers, the stages' kernels
    using Law = dr::M448Law;
    static constexpr int wide_bits = 449;
    static constexpr auto wide_prepare = dr::k_c448_msm_prepare;
    static constexpr auto wide_sort = dr::k_ed448_msm_sort;
    static constexpr auto wide_accumulate = dr::k_c448_msm_accumulate;
    static constexpr auto wide_accumulate_heavy = dr::k_c448_msm_accumulate_heavy;
    static constexpr auto wide_reduce = dr::k_c448_msm_reduce;
    static constexpr auto wide_fold = dr::k_c448_msm_fold;
    static constexpr size_t enc_bytes = pt_bytes, rec_bytes = pt_bytes;   // the decoder takes u || v as given: its kernel judges the range
    static constexpr bool decode_gives_points = true, decode_checks_canonical = false;
    // (a field element in {1, p - 1}: the reference's mod_inverse(0); c448_law.hip.h, m448_ell2)
    static constexpr const char* no_image = "the map to the curve has no value for a message (No inverse exists)";
    static bool canonical(const uint8_t* p) { return Ed448Suite::canonical(p); }
    static void hash_to_field(int variant, const uint8_t* salt, size_t salt_len, const uint8_t* msg, size_t len, uint8_t* out) {
        const bool nu = variant == variant_nu;
        drh::hash_to_field_fe448(nu ? "QUUX-V01-CS02-with-curve448_XOF:SHAKE256_ELL2_NU_" : "QUUX-V01-CS02-with-curve448_XOF:SHAKE256_ELL2_RO_", 49,
                                 nu ? 1 : 2, salt, salt_len, msg, len, out);
    }
    static size_t map_flag_words(size_t n, size_t) { return n; }
    static int map_launch(dr_ctx* ctx, size_t n, size_t, int per_item, int clear) {
        return launch(ctx, "k_curve448_map_to_curve", [&] {
            hipLaunchKernelGGL(dr::k_curve448_map_to_curve, dim3(div_up(n, block)), dim3(block), 0, ctx->stream, ctx->io_a.as<uint32_t>(),
                               ctx->io_b.as<uint32_t>(), ctx->io_c.as<uint32_t>(), (uint32_t)n, (uint32_t)per_item, clear ? 1u : 0u);
        });
    }
};

}  // namespace

int dr_ed448_hash_to_field_batch(int variant, const uint8_t* msgs, const uint64_t* off, size_t count, uint8_t* out) {
    return hash_to_field_batch<Ed448Suite>(variant, msgs, off, count, out);
}
int dr_ed448_map_to_curve(dr_ctx* ctx, const uint8_t* us, size_t n, int per_item, int clear, uint8_t* out_xy, uint8_t* ok) {
    return map_to_curve<Ed448Suite>(ctx, us, n, per_item, clear, out_xy, ok);
}
int dr_ed448_encode_to_curve_batch(dr_ctx* ctx, int variant, const uint8_t* msgs, const uint64_t* off, const uint8_t* salts,
                                   const uint64_t* salt_off, size_t count, uint8_t* out_xy) {
    return encode_to_curve_batch<Ed448Suite>(ctx, variant, msgs, off, salts, salt_off, count, out_xy);
}
int dr_ed448_scalar_mul_batch(dr_ctx* ctx, const uint8_t* pts_xy, const uint8_t* scalars, size_t n, uint8_t* out_xy) {
    TRY(use_ctx(ctx));
    return scalar_mul_batch<Ed448Suite>(ctx, pts_xy, scalars, n, out_xy);
}
int dr_ed448_msm_groups(dr_ctx* ctx, const uint8_t* pts_xy, const uint8_t* scalars, size_t groups, size_t m, uint8_t* out_xy) {
    TRY(use_ctx(ctx));
    return msm_groups<Ed448Suite>(ctx, pts_xy, scalars, groups, m, out_xy);
}
int dr_ed448_decode_points(dr_ctx* ctx, int check, const uint8_t* enc, size_t n, uint8_t* out_xy, uint8_t* ok) {
    return flagged_round<Ed448Suite>(ctx, enc, n, out_xy, ok, [&] {
        const auto kernel = check ? dr::k_ed448_check_points<1> : dr::k_ed448_check_points<0>;
        hipLaunchKernelGGL(kernel, dim3(div_up(n, dr::E448_BLOCK)), dim3(dr::E448_BLOCK), 0, ctx->stream, ctx->io_a.as<uint32_t>(),
                           ctx->io_b.as<uint32_t>(), ctx->io_c.as<uint32_t>(), (uint32_t)n);
    });
}
int dr_ed448_field_selftest(dr_ctx* ctx, const int32_t* a_limbs, const int32_t* b_limbs, size_t n, uint8_t* out, uint8_t* flags) {
    return field_selftest<Ed448Suite>(ctx, a_limbs, b_limbs, n, out, flags);
}
int dr_ed448_law_selftest(dr_ctx* ctx, const int32_t* points, const uint32_t* controls, size_t n, int32_t* out) {
    return law_selftest<Ed448Suite>(ctx, points, controls, n, out);
}

// dr_wide_msm for DR_CURVE_ED448_RO / _NU and DR_CURVE_CURVE448_RO / _NU (the dispatcher is capi_msm.hip's); Curve448's identity travels
// inside the point as 112 bytes of 0xff, in and out
int ed448_wide_msm(dr_ctx* ctx, const uint8_t* pts_xy, const uint8_t* scalars, size_t n, uint8_t* out_xy) {
    return wide_msm<Ed448Suite>(ctx, pts_xy, scalars, n, out_xy);
}
int curve448_wide_msm(dr_ctx* ctx, const uint8_t* pts_uv, const uint8_t* scalars, size_t n, uint8_t* out_uv) {
    return wide_msm<Curve448Suite>(ctx, pts_uv, scalars, n, out_uv);
}

// ---- Curve448: the identity is 112 bytes of 0xff at every one of them, in and out; there are no flag-byte parameters
int dr_curve448_hash_to_field_batch(int variant, const uint8_t* msgs, const uint64_t* off, size_t count, uint8_t* out) {
    return hash_to_field_batch<Curve448Suite>(variant, msgs, off, count, out);
}
int dr_curve448_map_to_curve(dr_ctx* ctx, const uint8_t* us, size_t n, int per_item, int clear, uint8_t* out_uv, uint8_t* ok) {
    return map_to_curve<Curve448Suite>(ctx, us, n, per_item, clear, out_uv, ok);
}
int dr_curve448_encode_to_curve_batch(dr_ctx* ctx, int variant, const uint8_t* msgs, const uint64_t* off, const uint8_t* salts,
                                      const uint64_t* salt_off, size_t count, uint8_t* out_uv) {
    return encode_to_curve_batch<Curve448Suite>(ctx, variant, msgs, off, salts, salt_off, count, out_uv);
}
int dr_curve448_scalar_mul_batch(dr_ctx* ctx, const uint8_t* pts_uv, const uint8_t* scalars, size_t n, uint8_t* out_uv) {
    TRY(use_ctx(ctx));
    return scalar_mul_batch<Curve448Suite>(ctx, pts_uv, scalars, n, out_uv);
}
int dr_curve448_msm_groups(dr_ctx* ctx, const uint8_t* pts_uv, const uint8_t* scalars, size_t groups, size_t m, uint8_t* out_uv) {
    TRY(use_ctx(ctx));
    return msm_groups<Curve448Suite>(ctx, pts_uv, scalars, groups, m, out_uv);
}
int dr_curve448_decode_points(dr_ctx* ctx, int check, const uint8_t* enc, size_t n, uint8_t* out_uv, uint8_t* ok) {
    return decode_points<Curve448Suite>(ctx, check ? dr::k_c448_decode_points<1> : dr::k_c448_decode_points<0>, enc, n, out_uv, ok);
}
int dr_curve448_law_selftest(dr_ctx* ctx, const int32_t* points, const uint32_t* controls, size_t n, int32_t* out) {
    return law_selftest<Curve448Suite>(ctx, points, controls, n, out);
}
