// libdotring_hip.so — C ABI, part 6 of 11: the BLS12_381_G1 suites (DR_CURVE_BLS12_381_G1 / DR_CURVE_BLS12_381_G1_NU; the reference's
// specs/bls12_381_G1.py).  The first curve here whose coordinates are 48 bytes: none of it goes through the 64-byte paths of
// capi_core.hip but through capi_suite.hpp — points are affine x || y, 48 + 48 bytes little-endian, canonical standard form, 96 zero bytes
// the identity.  The kernels are kernels_g1_h2c_entry.hip.h over kernels_g1_h2c.hip.h (the complete projective law over fq28.hip.h,
// wave_curve.hip.h's and sswu.hip.h's templates); the host does hash_to_field (expand_message_xmd over SHA-256, L = 64) on the worker
// threads and checks that inputs are canonical.  Scalars are 32 bytes used AS THEY ARE: E(Fq) has order h r, and its points need not lie
// in G1.
#include "capi_suite.hpp"
#include "capi_wide_msm.hpp"
#include "kernels_g1_h2c_entry.hip.h"
#include "narrow_law.hpp"

using namespace dri;

namespace {

struct Blsg1Suite : SuiteDefaults {
    static constexpr size_t fe_bytes = 48, elem_bytes = 48, pt_bytes = 96, scalar_bytes = 32, limb_bytes = 4 * dr::L28;
    static constexpr int variant_ro = DR_CURVE_BLS12_381_G1, variant_nu = DR_CURVE_BLS12_381_G1_NU;
    static constexpr const char* variant_names = "DR_CURVE_BLS12_381_G1 or DR_CURVE_BLS12_381_G1_NU";
    static constexpr bool limit_first = true;
    static constexpr size_t max_map = 1ull << 29, max_points = 1ull << 30, max_decode = 1ull << 30;
    static constexpr auto scalar_mul = dr::k_blsg1_scalar_mul;
    static constexpr auto msm_groups = dr::k_blsg1_msm_groups;
    static constexpr auto field_selftest = dr::k_blsg1_field_selftest;
    static constexpr auto law_selftest = dr::k_blsg1_law_selftest;
    static constexpr int law_coords = 3, law_slots = dr::WAVE_LAW_SLOTS;
    static constexpr int block = dr::G1H_BLOCK, selftest_records = dr::G1H_SELFTEST_RECORDS;
    static constexpr const char *k_scalar_mul = "k_blsg1_scalar_mul", *k_msm_groups = "k_blsg1_msm_groups", *k_decode = "k_blsg1_decode_points";
    static constexpr size_t enc_bytes = 49, rec_bytes = 52;               // each encoding zero-padded to 13 words
    static constexpr bool decode_gives_points = true, decode_checks_canonical = false;
    static constexpr const char* no_image = "the map to the curve has no value for a message (an isogeny denominator vanishes)";
    static bool canonical(const uint8_t* p) { return fq_canonical(p); }
    // dr_blsg1_msm (capi_wide_msm.hpp): the bucket method from NARROW_PIP_FROM terms on, over 257 tiled bits of scalars used as they are
    using Law = dr::G1hLaw;
    using WideCurve = dr::G1hCurve;
    static constexpr int wide_bits = 257;
    static constexpr size_t wide_from = dr::NARROW_PIP_FROM;
    DR_WAVE_MSM_STAGES(blsg1);
    // RFC 9380 section 5: L = 64 bytes per element, the DST of the variant (the `dst` fields of the RFC's vector files)
    static void hash_to_field(int variant, const uint8_t* salt, size_t salt_len, const uint8_t* msg, size_t len, uint8_t* out) {
        const bool nu = variant == variant_nu;
        drh::hash_to_field_fq(nu ? "QUUX-V01-CS02-with-BLS12381G1_XMD:SHA-256_SSWU_NU_" : "QUUX-V01-CS02-with-BLS12381G1_XMD:SHA-256_SSWU_RO_", 50,
                              nu ? 1 : 2, salt, salt_len, msg, len, out);
    }
    static size_t map_flag_words(size_t n, size_t) { return n; }
    static int map_launch(dr_ctx* ctx, size_t n, size_t, int per_item, int clear) {
        return launch(ctx, "k_blsg1_map_to_curve", [&] {
            hipLaunchKernelGGL(dr::k_blsg1_map_to_curve, dim3(div_up(n, block)), dim3(block), 0, ctx->stream, ctx->io_a.as<uint32_t>(),
                               ctx->io_b.as<uint32_t>(), ctx->io_c.as<uint32_t>(), (uint32_t)n, (uint32_t)per_item, clear ? 1u : 0u);
        });
    }
};

}  // namespace

int dr_blsg1_hash_to_field_batch(int variant, const uint8_t* msgs, const uint64_t* off, size_t count, uint8_t* out) {
    return hash_to_field_batch<Blsg1Suite>(variant, msgs, off, count, out);
}
int dr_blsg1_map_to_curve(dr_ctx* ctx, const uint8_t* us, size_t n, int per_item, int clear, uint8_t* out_xy, uint8_t* ok) {
    return map_to_curve<Blsg1Suite>(ctx, us, n, per_item, clear, out_xy, ok);
}
int dr_blsg1_encode_to_curve_batch(dr_ctx* ctx, int variant, const uint8_t* msgs, const uint64_t* off, const uint8_t* salts,
                                   const uint64_t* salt_off, size_t count, uint8_t* out_xy) {
    return encode_to_curve_batch<Blsg1Suite>(ctx, variant, msgs, off, salts, salt_off, count, out_xy);
}
int dr_blsg1_scalar_mul_batch(dr_ctx* ctx, const uint8_t* pts_xy, const uint8_t* scalars, size_t n, uint8_t* out_xy) {
    TRY(use_ctx(ctx));
    return scalar_mul_batch<Blsg1Suite>(ctx, pts_xy, scalars, n, out_xy);
}
int dr_blsg1_msm_groups(dr_ctx* ctx, const uint8_t* pts_xy, const uint8_t* scalars, size_t groups, size_t m, uint8_t* out_xy) {
    TRY(use_ctx(ctx));
    return msm_groups<Blsg1Suite>(ctx, pts_xy, scalars, groups, m, out_xy);
}
// ONE MSM of n terms: msm_groups in chunks of up to 64 folded on the host below NARROW_PIP_FROM terms, the bucket method from there on.
// NOT a fixed schedule from there on: secret scalars go through dr_blsg1_scalar_mul_batch and dr_blsg1_msm_groups.
int dr_blsg1_msm(dr_ctx* ctx, int curve, const uint8_t* pts_xy, const uint8_t* scalars, size_t n, uint8_t* out_xy) {
    TRY(check_variant<Blsg1Suite>(curve));
    return wide_msm<Blsg1Suite>(ctx, pts_xy, scalars, n, out_xy);
}
int dr_blsg1_decode_points(dr_ctx* ctx, int check, const uint8_t* enc, size_t n, uint8_t* out_xy, uint8_t* ok) {
    return flagged_round<Blsg1Suite>(ctx, enc, n, out_xy, ok, [&] {
        const auto kernel = check ? dr::k_blsg1_decode_points<dr::G1H_DEC_CHECK> : dr::k_blsg1_decode_points<dr::G1H_DEC_CODEC>;
        hipLaunchKernelGGL(kernel, dim3(div_up(n, dr::G1H_BLOCK)), dim3(dr::G1H_BLOCK), 0, ctx->stream, ctx->io_a.as<uint32_t>(),
                           ctx->io_b.as<uint32_t>(), ctx->io_c.as<uint32_t>(), (uint32_t)n);
    });
}
int dr_blsg1_field_selftest(dr_ctx* ctx, const int32_t* a_limbs, const int32_t* b_limbs, size_t n, uint8_t* out, uint8_t* flags) {
    return field_selftest<Blsg1Suite>(ctx, a_limbs, b_limbs, n, out, flags);
}
int dr_blsg1_law_selftest(dr_ctx* ctx, const int32_t* points, const uint32_t* controls, size_t n, int32_t* out) {
    return law_selftest<Blsg1Suite>(ctx, points, controls, n, out);
}
