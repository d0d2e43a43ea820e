// libdotring_hip.so — C ABI, part 9 of 11: the P-521 suites (DR_CURVE_P521_RO / DR_CURVE_P521_NU; the reference's specs/p521.py).
// Field elements and coordinates are 68 bytes little-endian, canonical; points are affine x || y, 136 bytes, and 136 zero bytes are the
// identity, in and out ((0, 0) is not on the curve).  Scalars are 68 bytes below 2^521 used AS THEY ARE: the 131 windows of the schedule
// cover no more, so a larger one is refused here, on the host, before anything is uploaded.  None of it goes through the 64-byte paths of
// capi_core.hip but through capi_suite.hpp.  The kernels are kernels_p521.hip.h over p521_law.hip.h and fp521.hip.h; the host does
// hash_to_field (expand_message_xmd over SHA-512, L = 98) on the worker threads and checks that inputs are canonical.  Scalars may be
// secret: they pass through io_a / io_b / io_c only, which ctx_wipe_scratch covers.
#include "capi_suite.hpp"
#include "capi_wide_msm.hpp"
#include "kernels_p521.hip.h"

using namespace dri;

namespace {

struct P521Suite : SuiteDefaults {
    static constexpr size_t fe_bytes = 68, elem_bytes = 68, pt_bytes = 136, scalar_bytes = 68, limb_bytes = 4 * dr::L521;
    static constexpr int variant_ro = DR_CURVE_P521_RO, variant_nu = DR_CURVE_P521_NU;
    static constexpr const char* variant_names = "DR_CURVE_P521_RO or DR_CURVE_P521_NU";
    static constexpr bool limit_first = true;
    static constexpr size_t max_map = 1ull << 28, max_points = 1ull << 28, max_decode = 1ull << 28;
    static constexpr auto scalar_mul = dr::k_p521_scalar_mul;
    static constexpr auto msm_groups = dr::k_p521_msm_groups;
    static constexpr auto field_selftest = dr::k_p521_field_selftest;
    static constexpr auto law_selftest = dr::k_p521_law_selftest;
    static constexpr int law_coords = 3, law_slots = dr::WAVE_LAW_SLOTS;
    static constexpr int block = dr::P521_BLOCK, selftest_records = dr::P521_SELFTEST_RECORDS;
    static constexpr const char *k_scalar_mul = "k_p521_scalar_mul", *k_msm_groups = "k_p521_msm_groups", *k_decode = "k_p521_decode_points";
    // the bucket method of dr_wide_msm (capi_wide_msm.hpp): the law on the host, the bits the tiling covers, the stages' kernels
    using Law = dr::P521Law;
    static constexpr int wide_bits = 522;
    DR_WAVE_MSM_STAGES_RECORDS(p521);
    // SEC1 compressed: 67 bytes, a zero byte behind each on the device; the kernel judges the range of x, which is big-endian
    static constexpr size_t enc_bytes = 67, rec_bytes = 68;
    static constexpr bool decode_gives_points = true, decode_checks_canonical = false;
    static constexpr const char* no_image = "the map to the curve has no value for a message";     // (never: every element has an image)
    // the 68 bytes at p below p = 2^521 - 1: the top word is 0x1ff and the sixteen below it are all ones
    static bool canonical(const uint8_t* p) {
        uint32_t w[17];
        std::memcpy(w, p, fe_bytes);
        if (w[16] != 0x1ffu) return w[16] < 0x1ffu;
        for (int i = 0; i < 16; i++)
            if (w[i] != 0xffffffffu) return true;
        return false;
    }
    static constexpr bool checks_scalars = true;
    static constexpr const char* scalar_refusal = "scalar is not below 2^521";
    static bool scalars_ok(const uint8_t* scalars, size_t n) {
        for (size_t i = 0; i < n; i++) {
            const uint8_t* s = scalars + scalar_bytes * i;
            if (s[65] > 1 || s[66] || s[67]) return false;      // bits 521..543
        }
        return true;
    }
    // RFC 9380 section 5.3.1: L = 98 bytes per element; the DST of the variant (the reference's hash_to_curve_dst: _RO_ replaced by _NU_)
    static void hash_to_field(int variant, const uint8_t* salt, size_t salt_len, const uint8_t* msg, size_t len, uint8_t* out) {
        const bool nu = variant == variant_nu;
        drh::hash_to_field_fp521(nu ? "QUUX-V01-CS02-with-P521_XMD:SHA-512_SSWU_NU_" : "QUUX-V01-CS02-with-P521_XMD:SHA-512_SSWU_RO_", 44, nu ? 1 : 2, salt,
                                 salt_len, msg, len, out);
    }
    static size_t map_flag_words(size_t n, size_t) { return n; }
    static int map_launch(dr_ctx* ctx, size_t n, size_t, int per_item, int clear) {
        return launch(ctx, "k_p521_map_to_curve", [&] {
            hipLaunchKernelGGL(dr::k_p521_map_to_curve, dim3(div_up(n, block)), dim3(block), 0, ctx->stream, ctx->io_a.as<uint32_t>(),
                               ctx->io_b.as<uint32_t>(), ctx->io_c.as<uint32_t>(), (uint32_t)n, (uint32_t)per_item, clear ? 1u : 0u);
        });
    }
};

}  // namespace

int dr_p521_hash_to_field_batch(int variant, const uint8_t* msgs, const uint64_t* off, size_t count, uint8_t* out) {
    return hash_to_field_batch<P521Suite>(variant, msgs, off, count, out);
}
int dr_p521_map_to_curve(dr_ctx* ctx, const uint8_t* us, size_t n, int per_item, int clear, uint8_t* out_xy, uint8_t* ok) {
    return map_to_curve<P521Suite>(ctx, us, n, per_item, clear, out_xy, ok);
}
int dr_p521_encode_to_curve_batch(dr_ctx* ctx, int variant, const uint8_t* msgs, const uint64_t* off, const uint8_t* salts,
                                  const uint64_t* salt_off, size_t count, uint8_t* out_xy) {
    return encode_to_curve_batch<P521Suite>(ctx, variant, msgs, off, salts, salt_off, count, out_xy);
}
int dr_p521_scalar_mul_batch(dr_ctx* ctx, const uint8_t* pts_xy, const uint8_t* scalars, size_t n, uint8_t* out_xy) {
    TRY(use_ctx(ctx));
    return scalar_mul_batch<P521Suite>(ctx, pts_xy, scalars, n, out_xy);
}
int dr_p521_msm_groups(dr_ctx* ctx, const uint8_t* pts_xy, const uint8_t* scalars, size_t groups, size_t m, uint8_t* out_xy) {
    TRY(use_ctx(ctx));
    return msm_groups<P521Suite>(ctx, pts_xy, scalars, groups, m, out_xy);
}
// dr_wide_msm for DR_CURVE_P521_RO / _NU (the dispatcher is capi_msm.hip's)
int p521_wide_msm(dr_ctx* ctx, const uint8_t* pts_xy, const uint8_t* scalars, size_t n, uint8_t* out_xy) {
    return wide_msm<P521Suite>(ctx, pts_xy, scalars, n, out_xy);
}
// check = 0 and check = 1 are one kernel (include/dotring_hip.h says why); the parameter is the suites' common signature
int dr_p521_decode_points(dr_ctx* ctx, int check, const uint8_t* enc, size_t n, uint8_t* out_xy, uint8_t* ok) {
    (void)check;
    return decode_points<P521Suite>(ctx, dr::k_p521_decode_points, enc, n, out_xy, ok);
}
int dr_p521_field_selftest(dr_ctx* ctx, const int32_t* a_limbs, const int32_t* b_limbs, size_t n, uint8_t* out, uint8_t* flags) {
    return field_selftest<P521Suite>(ctx, a_limbs, b_limbs, n, out, flags);
}
int dr_p521_law_selftest(dr_ctx* ctx, const int32_t* points, const uint32_t* controls, size_t n, int32_t* out) {
    return law_selftest<P521Suite>(ctx, points, controls, n, out);
}
