// libdotring_hip.so — C ABI, part 7 of 11: the BLS12_381_G2 suites (DR_CURVE_BLS12_381_G2 / DR_CURVE_BLS12_381_G2_NU; the reference's
// specs/bls12_381_G2.py).  Coordinates are elements of Fq2, c0 || c1, 48 + 48 bytes little-endian, canonical standard form; points are
// affine x || y, 192 bytes, 192 zero bytes the identity.  None of it goes through the 64-byte paths of capi_core.hip but through
// capi_suite.hpp.  The kernels are kernels_g2_h2c.hip.h (the complete projective law over fq2_28.hip.h); the host does hash_to_field
// (expand_message_xmd over SHA-256, m = 2, L = 64) on the worker threads and checks that inputs are canonical.  Scalars are 96 bytes used
// AS THEY ARE: E(Fq2) has order h2 r (762 bits), and its points need not lie in G2.  dr_blsg2_msm (kernels_g2_msm.hip.h: the bucket method
// of wave_msm.hip.h over G2hCurve, the host's end over g2_law.hpp) takes 32-byte scalars, as they are too.  Scalars on this curve are
// public: there is no VRF over it.
#include "capi_suite.hpp"
#include "capi_wide_msm.hpp"
#include "g2_law.hpp"
#include "kernels_g2_msm.hip.h"

using namespace dri;

namespace {

struct Blsg2Suite : SuiteDefaults {                     // (the flag-returning launch is check_points, which gives no points back)
    static constexpr size_t fe_bytes = 48, elem_bytes = 96, pt_bytes = 192, scalar_bytes = 96, limb_bytes = 4 * 2 * dr::L28;
    static constexpr int variant_ro = DR_CURVE_BLS12_381_G2, variant_nu = DR_CURVE_BLS12_381_G2_NU;
    static constexpr const char* variant_names = "DR_CURVE_BLS12_381_G2 or DR_CURVE_BLS12_381_G2_NU";
    static constexpr size_t max_map = 1ull << 28, max_points = 1ull << 28, max_decode = 1ull << 28;
    static constexpr bool limit_first = true;
    static constexpr auto scalar_mul = dr::k_blsg2_scalar_mul;
    static constexpr auto msm_groups = dr::k_blsg2_msm_groups<24>;
    static constexpr auto field_selftest = dr::k_blsg2_field_selftest;
    static constexpr auto law_selftest = dr::k_blsg2_law_selftest;
    static constexpr int law_coords = 3, law_slots = dr::WAVE_LAW_SLOTS;
    static constexpr size_t law_lane_bytes = 4 * (size_t)dr::wave_msm_record_words<dr::G2hCurve>();
    static constexpr int block = dr::G2H_BLOCK, selftest_records = dr::G2H_SELFTEST_RECORDS;
    static constexpr const char *k_scalar_mul = "k_blsg2_scalar_mul", *k_msm_groups = "k_blsg2_msm_groups", *k_decode = "k_blsg2_check_points";
    static constexpr size_t enc_bytes = pt_bytes, rec_bytes = pt_bytes;
    static constexpr bool decode_gives_points = false, decode_checks_canonical = true;
    // (no input reaches this: kernels_g2_h2c.hip.h, g2h_iso_map)
    static constexpr const char* no_image = "the map to the curve has no value for a message (an isogeny denominator vanishes)";
    static bool canonical(const uint8_t* p) { return fq_canonical(p); }
    // RFC 9380 section 5: m = 2 chunks of L = 64 bytes per element (256 bytes for RO, 128 for NU), element j = (e_2j, e_2j+1) = c0 || c1;
    // the DST of the variant (the `dst` fields of the RFC's vector files)
    static void hash_to_field(int variant, const uint8_t* salt, size_t salt_len, const uint8_t* msg, size_t len, uint8_t* out) {
        const bool nu = variant == variant_nu;
        drh::hash_to_field_fq(nu ? "QUUX-V01-CS02-with-BLS12381G2_XMD:SHA-256_SSWU_NU_" : "QUUX-V01-CS02-with-BLS12381G2_XMD:SHA-256_SSWU_RO_", 50,
                              nu ? 2 : 4, salt, salt_len, msg, len, out);
    }
    // the two launches of the map: every element's image through ctx->partial (a scratch buffer that ctx_wipe_scratch zeroes with the
    // rest), the per-element flags behind the per-item flags in io_c
    static size_t map_flag_words(size_t n, size_t elems) { return n + elems; }
    static int map_launch(dr_ctx* ctx, size_t n, size_t elems, int per_item, int clear) {
        TRY(ctx->partial.reserve(elems * dr::G2H_STAGE_WORDS * 4));
        uint32_t* ok_item = ctx->io_c.as<uint32_t>();
        uint32_t* ok_elem = ok_item + n;
        TRY(launch(ctx, "k_blsg2_map_iso", [&] {
            hipLaunchKernelGGL(dr::k_blsg2_map_iso, dim3(div_up(elems, block)), dim3(block), 0, ctx->stream, ctx->io_a.as<uint32_t>(),
                               ctx->partial.as<int32_t>(), ok_elem, (uint32_t)elems);
        }));
        return launch(ctx, "k_blsg2_sum_clear", [&] {
            hipLaunchKernelGGL(dr::k_blsg2_sum_clear, dim3(div_up(n, block)), dim3(block), 0, ctx->stream, ctx->partial.as<int32_t>(), ok_elem,
                               ctx->io_b.as<uint32_t>(), ok_item, (uint32_t)n, (uint32_t)per_item, clear ? 1u : 0u);
        });
    }
};

// dr_blsg2_msm (capi_wide_msm.hpp): the same suite with 32-byte scalars — msm_groups' kernel over 8-word scalars below BLSG2_PIP_FROM
// terms, from there on the bucket method over 257 tiled bits of scalars used as they are
struct Blsg2MsmSuite : Blsg2Suite {
    static constexpr size_t scalar_bytes = 32;
    static constexpr auto msm_groups = dr::k_blsg2_msm_groups<8>;
    using Law = dr::G2hLaw;
    using WideCurve = dr::G2hCurve;
    static constexpr int wide_bits = 257;
    static constexpr size_t wide_from = dr::BLSG2_PIP_FROM;
    DR_WAVE_MSM_STAGES(blsg2);
};

}  // namespace

int dr_blsg2_hash_to_field_batch(int variant, const uint8_t* msgs, const uint64_t* off, size_t count, uint8_t* out) {
    return hash_to_field_batch<Blsg2Suite>(variant, msgs, off, count, out);
}
int dr_blsg2_map_to_curve(dr_ctx* ctx, const uint8_t* us, size_t n, int per_item, int clear, uint8_t* out_xy, uint8_t* ok) {
    return map_to_curve<Blsg2Suite>(ctx, us, n, per_item, clear, out_xy, ok);
}
int dr_blsg2_encode_to_curve_batch(dr_ctx* ctx, int variant, const uint8_t* msgs, const uint64_t* off, const uint8_t* salts,
                                   const uint64_t* salt_off, size_t count, uint8_t* out_xy) {
    return encode_to_curve_batch<Blsg2Suite>(ctx, variant, msgs, off, salts, salt_off, count, out_xy);
}
int dr_blsg2_scalar_mul_batch(dr_ctx* ctx, const uint8_t* pts_xy, const uint8_t* scalars, size_t n, uint8_t* out_xy) {
    TRY(use_ctx(ctx));
    return scalar_mul_batch<Blsg2Suite>(ctx, pts_xy, scalars, n, out_xy);
}
int dr_blsg2_msm_groups(dr_ctx* ctx, const uint8_t* pts_xy, const uint8_t* scalars, size_t groups, size_t m, uint8_t* out_xy) {
    TRY(use_ctx(ctx));
    return msm_groups<Blsg2Suite>(ctx, pts_xy, scalars, groups, m, out_xy);
}
// ONE MSM of n terms: msm_groups in chunks of up to 64 folded on the host below BLSG2_PIP_FROM terms, the bucket method from there on.
// NOT a fixed schedule on either side of it: the scalars of this curve are public.
int dr_blsg2_msm(dr_ctx* ctx, int curve, const uint8_t* pts_xy, const uint8_t* scalars, size_t n, uint8_t* out_xy) {
    TRY(check_variant<Blsg2Suite>(curve));
    return wide_msm<Blsg2MsmSuite>(ctx, pts_xy, scalars, n, out_xy);
}
int dr_blsg2_check_points(dr_ctx* ctx, int subgroup, const uint8_t* pts_xy, size_t n, uint8_t* ok) {
    return flagged_round<Blsg2Suite>(ctx, pts_xy, n, nullptr, ok, [&] {
        const auto kernel = subgroup ? dr::k_blsg2_check_points<dr::G2H_CHECK_SUBGROUP> : dr::k_blsg2_check_points<dr::G2H_CHECK_CURVE>;
        hipLaunchKernelGGL(kernel, dim3(div_up(n, dr::G2H_BLOCK)), dim3(dr::G2H_BLOCK), 0, ctx->stream, ctx->io_a.as<uint32_t>(),
                           ctx->io_c.as<uint32_t>(), (uint32_t)n);
    });
}
int dr_blsg2_field_selftest(dr_ctx* ctx, const int32_t* a_limbs, const int32_t* b_limbs, size_t n, uint8_t* out, uint8_t* flags) {
    return field_selftest<Blsg2Suite>(ctx, a_limbs, b_limbs, n, out, flags);
}
int dr_blsg2_law_selftest(dr_ctx* ctx, const int32_t* points, const uint32_t* controls, size_t n, int32_t* out) {
    return law_selftest<Blsg2Suite>(ctx, points, controls, n, out);
}
