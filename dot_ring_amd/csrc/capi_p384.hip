// libdotring_hip.so — C ABI, part 10 of 11: the P-384 suites (DR_CURVE_P384_RO / DR_CURVE_P384_NU; the reference's specs/p384.py).
// Field elements and coordinates are 48 bytes little-endian, canonical; points are affine x || y, 96 bytes, and 96 zero bytes are the
// identity, in and out ((0, 0) is not on the curve).  Scalars are 48 bytes used AS THEY ARE: the 97 windows of the schedule take every
// 384-bit value, so none is refused.  None of it goes through the 64-byte paths of capi_core.hip but through capi_suite.hpp.  The
// kernels are kernels_p384.hip.h over p384_law.hip.h and fp384.hip.h; the host does hash_to_field (expand_message_xmd over SHA-384,
// L = 72) on the worker threads and checks that inputs are canonical.  Scalars may be secret: they pass through io_a / io_b / io_c
// only, which ctx_wipe_scratch covers.
#include "capi_suite.hpp"
#include "capi_wide_msm.hpp"
#include "kernels_p384.hip.h"

using namespace dri;

namespace {

struct P384Suite : SuiteDefaults {
    static constexpr size_t fe_bytes = 48, elem_bytes = 48, pt_bytes = 96, scalar_bytes = 48, limb_bytes = 4 * dr::L384;
    static constexpr int variant_ro = DR_CURVE_P384_RO, variant_nu = DR_CURVE_P384_NU;
    static constexpr const char* variant_names = "DR_CURVE_P384_RO or DR_CURVE_P384_NU";
    static constexpr bool limit_first = true;
    static constexpr size_t max_map = 1ull << 28, max_points = 1ull << 28, max_decode = 1ull << 28;
    static constexpr auto scalar_mul = dr::k_p384_scalar_mul;
    static constexpr auto msm_groups = dr::k_p384_msm_groups;
    static constexpr auto field_selftest = dr::k_p384_field_selftest;
    static constexpr auto law_selftest = dr::k_p384_law_selftest;
    static constexpr int law_coords = 3, law_slots = dr::WAVE_LAW_SLOTS;
    static constexpr int block = dr::P384_BLOCK, selftest_records = dr::P384_SELFTEST_RECORDS;
    static constexpr const char *k_scalar_mul = "k_p384_scalar_mul", *k_msm_groups = "k_p384_msm_groups", *k_decode = "k_p384_decode_points";
    // the bucket method of dr_wide_msm (capi_wide_msm.hpp): the law on the host, the bits the tiling covers, the stages' kernels
    using Law = dr::P384Law;
    static constexpr int wide_bits = 385;
    DR_WAVE_MSM_STAGES_RECORDS(p384);
    // SEC1 compressed: 49 bytes, three zero bytes behind each on the device; the kernel judges the range of x, which is big-endian
    static constexpr size_t enc_bytes = 49, rec_bytes = 52;
    static constexpr bool decode_gives_points = true, decode_checks_canonical = false;
    static constexpr const char* no_image = "the map to the curve has no value for a message";     // (never: every element has an image)
    // the 48 bytes at p below the modulus
    static bool canonical(const uint8_t* p) {
        uint32_t w[12];
        std::memcpy(w, p, fe_bytes);
        return dr::below_p(w);
    }
    // RFC 9380 section 5.3.1: L = 72 bytes per element; the DST of the variant (the reference's hash_to_curve_dst: _RO_ replaced by _NU_)
    static void hash_to_field(int variant, const uint8_t* salt, size_t salt_len, const uint8_t* msg, size_t len, uint8_t* out) {
        const bool nu = variant == variant_nu;
        drh::hash_to_field_fp384(nu ? "QUUX-V01-CS02-with-P384_XMD:SHA-384_SSWU_NU_" : "QUUX-V01-CS02-with-P384_XMD:SHA-384_SSWU_RO_", 44, nu ? 1 : 2, salt,
                                 salt_len, msg, len, out);
    }
    static size_t map_flag_words(size_t n, size_t) { return n; }
    static int map_launch(dr_ctx* ctx, size_t n, size_t, int per_item, int clear) {
        return launch(ctx, "k_p384_map_to_curve", [&] {
            hipLaunchKernelGGL(dr::k_p384_map_to_curve, dim3(div_up(n, block)), dim3(block), 0, ctx->stream, ctx->io_a.as<uint32_t>(),
                               ctx->io_b.as<uint32_t>(), ctx->io_c.as<uint32_t>(), (uint32_t)n, (uint32_t)per_item, clear ? 1u : 0u);
        });
    }
};

}  // namespace

int dr_p384_hash_to_field_batch(int variant, const uint8_t* msgs, const uint64_t* off, size_t count, uint8_t* out) {
    return hash_to_field_batch<P384Suite>(variant, msgs, off, count, out);
}
int dr_p384_map_to_curve(dr_ctx* ctx, const uint8_t* us, size_t n, int per_item, int clear, uint8_t* out_xy, uint8_t* ok) {
    return map_to_curve<P384Suite>(ctx, us, n, per_item, clear, out_xy, ok);
}
int dr_p384_encode_to_curve_batch(dr_ctx* ctx, int variant, const uint8_t* msgs, const uint64_t* off, const uint8_t* salts,
                                  const uint64_t* salt_off, size_t count, uint8_t* out_xy) {
    return encode_to_curve_batch<P384Suite>(ctx, variant, msgs, off, salts, salt_off, count, out_xy);
}
int dr_p384_scalar_mul_batch(dr_ctx* ctx, const uint8_t* pts_xy, const uint8_t* scalars, size_t n, uint8_t* out_xy) {
    TRY(use_ctx(ctx));
    return scalar_mul_batch<P384Suite>(ctx, pts_xy, scalars, n, out_xy);
}
int dr_p384_msm_groups(dr_ctx* ctx, const uint8_t* pts_xy, const uint8_t* scalars, size_t groups, size_t m, uint8_t* out_xy) {
    TRY(use_ctx(ctx));
    return msm_groups<P384Suite>(ctx, pts_xy, scalars, groups, m, out_xy);
}
// dr_wide_msm for DR_CURVE_P384_RO / _NU (the dispatcher is capi_msm.hip's)
int p384_wide_msm(dr_ctx* ctx, const uint8_t* pts_xy, const uint8_t* scalars, size_t n, uint8_t* out_xy) {
    return wide_msm<P384Suite>(ctx, pts_xy, scalars, n, out_xy);
}
// check = 0 and check = 1 are one kernel (include/dotring_hip.h says why); the parameter is the suites' common signature
int dr_p384_decode_points(dr_ctx* ctx, int check, const uint8_t* enc, size_t n, uint8_t* out_xy, uint8_t* ok) {
    (void)check;
    return decode_points<P384Suite>(ctx, dr::k_p384_decode_points, enc, n, out_xy, ok);
}
int dr_p384_field_selftest(dr_ctx* ctx, const int32_t* a_limbs, const int32_t* b_limbs, size_t n, uint8_t* out, uint8_t* flags) {
    return field_selftest<P384Suite>(ctx, a_limbs, b_limbs, n, out, flags);
}
int dr_p384_law_selftest(dr_ctx* ctx, const int32_t* points, const uint32_t* controls, size_t n, int32_t* out) {
    return law_selftest<P384Suite>(ctx, points, controls, n, out);
}
