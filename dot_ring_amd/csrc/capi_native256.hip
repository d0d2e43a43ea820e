// libdotring_hip.so — C ABI, part 11 of 11: the five native 256-bit suites, Ed25519 (kernels_ed25519.hip.h), P-256 (kernels_p256.hip.h),
// Baby JubJub (kernels_bjj.hip.h), secp256k1 (kernels_secp256k1.hip.h) and Curve25519 (kernels_curve25519.hip.h): their descriptions, their
// own entry points, and the seam through which capi_core.hip's dr_te_* paths and load_suite reach them (capi_internal.hpp).
// Every call runs on the kernels: there is no host route for these curves, and nothing here touches the BLS12-381 field of the other
// curves.  Secrets pass through io_a / io_b / io_c only, which ctx_wipe_scratch covers.  Points are affine x || y.  Each suite is one
// description below (its kernels, launch names, base field, identity and encoding widths) of the shape capi_suite.hpp lists; every
// operation is one of that header's templates over it.
#include "capi_suite.hpp"
#include "capi_wide_msm.hpp"
#include "narrow_law.hpp"
#include "kernels_ed25519.hip.h"
#include "kernels_curve25519.hip.h"
#include "kernels_p256.hip.h"
#include "kernels_secp256k1.hip.h"
#include "kernels_bjj.hip.h"

using namespace dri;

namespace {
// what the five descriptions share: 64-byte points, 32-byte scalars and field elements, nine-limb selftest images, the kernels' limits
template <class S>
struct Native256 : SuiteDefaults {
    static constexpr size_t fe_bytes = 32, elem_bytes = 32, pt_bytes = 64, scalar_bytes = 32, limb_bytes = 36;
    static constexpr int law_slots = dr::WAVE_LAW_SLOTS;
    static constexpr size_t max_map = 1ull << 30, max_points = 1ull << 31, max_decode = 1ull << 31;
    static constexpr bool limit_first = false, decode_gives_points = true, decode_checks_canonical = false;
    static bool canonical(const uint8_t* p) {
        uint64_t v[4];
        drh::load_le32(p, v);
        return !drh::Mod256::geq(v, S::field().m);
    }
    // the maps of RFC 9380 for n items of per_item (1 or 2) field elements each: one launch of the suite's map kernel (S::map, profiled as
    // S::k_map), the sum of each item's images out (on Ed25519 with the cofactor cleared)
    static size_t map_flag_words(size_t n, size_t) { return n; }
    static int map_launch(dr_ctx* ctx, size_t n, size_t, int per_item, int) {
        return launch(ctx, S::k_map, [&] {
            hipLaunchKernelGGL(S::map, dim3(div_up(n, S::block)), dim3(S::block), 0, ctx->stream, ctx->io_a.as<uint32_t>(), ctx->io_b.as<uint32_t>(),
                               ctx->io_c.as<uint32_t>(), (uint32_t)n, (uint32_t)per_item);
        });
    }
};
struct Ed25519Suite : Native256<Ed25519Suite> {
    static constexpr auto map = dr::k_ed25519_map_to_curve;
    static constexpr const char* k_map = "k_ed25519_map_to_curve";
    static constexpr auto scalar_mul = dr::k_ed_scalar_mul;
    static constexpr auto msm_groups = dr::k_ed_msm_groups;
    static constexpr auto dec_tai = dr::k_ed_decode_points<dr::ED_DEC_TAI>, dec_check = dr::k_ed_decode_points<dr::ED_DEC_CHECK>,
                          dec_codec = dr::k_ed_decode_points<dr::ED_DEC_CODEC>;
    static constexpr auto field_selftest = dr::k_fe25519_selftest;
    static constexpr auto law_selftest = dr::k_ed_law_selftest;
    static constexpr int law_coords = 4;
    static constexpr int block = dr::ED_BLOCK, selftest_records = dr::FE_SELFTEST_RECORDS;
    static constexpr const char *name = "Ed25519", *k_scalar_mul = "k_ed_scalar_mul", *k_msm_groups = "k_ed_msm_groups", *k_decode = "k_ed_decode_points";
    static const drh::Mod256& field() { return drh::mod_p25519(); }
    static constexpr size_t identity_y = 1, enc_bytes = 32, rec_bytes = 32, tai_bytes = 32;   // identity (0, identity_y); encoding, decoder record, try-and-increment candidate
    // the bucket method from NARROW_PIP_FROM terms on (native_msm): the host law, the device description, the tiled bits (the order's + 1)
    using Law = dr::Ed25519Law;
    using WideCurve = dr::Ed25519Curve;
    static constexpr int wide_bits = 254;
    DR_WAVE_MSM_STAGES(ed);
};
struct P256Suite : Native256<P256Suite> {
    static constexpr auto map = dr::k_p256_map_to_curve;
    static constexpr const char* k_map = "k_p256_map_to_curve";
    static constexpr auto scalar_mul = dr::k_p256_scalar_mul;
    static constexpr auto msm_groups = dr::k_p256_msm_groups;
    static constexpr auto dec_tai = dr::k_p256_decode_points<dr::P256_DEC_TAI>, dec_check = dr::k_p256_decode_points<dr::P256_DEC_CHECK>,
                          dec_codec = dr::k_p256_decode_points<dr::P256_DEC_CODEC>;
    static constexpr auto field_selftest = dr::k_p256_field_selftest;
    static constexpr auto law_selftest = dr::k_p256_law_selftest;
    static constexpr int law_coords = 3;
    static constexpr int block = dr::P256_BLOCK, selftest_records = dr::P256_SELFTEST_RECORDS;
    static constexpr const char *name = "P-256", *k_scalar_mul = "k_p256_scalar_mul", *k_msm_groups = "k_p256_msm_groups", *k_decode = "k_p256_decode_points";
    static const drh::Mod256& field() { return drh::mod_p256(); }
    static constexpr size_t identity_y = 0, enc_bytes = 33, rec_bytes = 36, tai_bytes = 33;   // 64 zero bytes are the identity; candidates carry the flag byte
    using Law = dr::P256Law;
    using WideCurve = dr::P256Curve;
    static constexpr int wide_bits = 257;
    DR_WAVE_MSM_STAGES(p256);
};
// P256_RO / P256_NU (curves 8 and 9): P-256's kernels with the plain SEC1 modes of its decoder (the reference's generic short
// Weierstrass encoding, not P256_TAI's; no string encodes the identity, so checking and codec-only decoding coincide and no entry point
// asks for the latter); no try-and-increment, so dec_tai is the checking decoder and tai_bytes never applies
struct P256Sec1Suite : P256Suite {
    static constexpr auto dec_tai = dr::k_p256_decode_points<dr::P256_DEC_SEC1>, dec_check = dr::k_p256_decode_points<dr::P256_DEC_SEC1>,
                          dec_codec = dr::k_p256_decode_points<dr::P256_DEC_SEC1>;
    static constexpr const char* name = "P-256 (RFC 9380)";
};
static_assert(P256Sec1Suite::dec_codec == P256Sec1Suite::dec_check, "one SEC1 decoder: a caller of either gets this format, never P256_TAI's");
// secp256k1 (curves 6 and 7): no try-and-increment, so dec_tai is the checking decoder again and encode_to_curve_msgs never takes that
// branch for these curves (they hash with k_secp256k1_map_to_curve)
struct Secp256k1Suite : Native256<Secp256k1Suite> {
    static constexpr auto map = dr::k_secp256k1_map_to_curve;
    static constexpr const char* k_map = "k_secp256k1_map_to_curve";
    static constexpr auto scalar_mul = dr::k_secp256k1_scalar_mul;
    static constexpr auto msm_groups = dr::k_secp256k1_msm_groups;
    static constexpr auto dec_tai = dr::k_secp256k1_decode_points<dr::K1_DEC_CHECK>, dec_check = dr::k_secp256k1_decode_points<dr::K1_DEC_CHECK>,
                          dec_codec = dr::k_secp256k1_decode_points<dr::K1_DEC_CODEC>;
    static constexpr auto field_selftest = dr::k_secp256k1_field_selftest;
    static constexpr auto law_selftest = dr::k_secp256k1_law_selftest;
    static constexpr int law_coords = 3;
    static constexpr int block = dr::K1_BLOCK, selftest_records = dr::K1_SELFTEST_RECORDS;
    static constexpr const char *name = "secp256k1", *k_scalar_mul = "k_secp256k1_scalar_mul", *k_msm_groups = "k_secp256k1_msm_groups",
                                *k_decode = "k_secp256k1_decode_points";
    static const drh::Mod256& field() { return drh::mod_psecp256k1(); }
    static constexpr size_t identity_y = 0, enc_bytes = 33, rec_bytes = 36, tai_bytes = 33;   // 64 zero bytes are the identity; no candidates are made
    using Law = dr::Secp256k1Law;
    using WideCurve = dr::Secp256k1Curve;
    static constexpr int wide_bits = 257;
    DR_WAVE_MSM_STAGES(secp256k1);
};
// Baby JubJub's square-root tables (BjjConsts) are built on the host once per process and copied to the device the first time a context
// decodes a point or runs the field selftest
int bjj_consts_build(dr::BjjConsts& h) {
    const drh::Mod256& F = drh::mod_pbn254();
    static const uint64_t R261[4] = {0x2fd4e1568fffff57ULL, 0x75bba827a494b01aULL, 0x5301fa84819caa80ULL, 0x0dc83629563d4475ULL};   // 2^261 mod p
    static const uint64_t Q[4] = {0x9b9709143e1f593fULL, 0x181585d2833e8487ULL, 0x131a029b85045b68ULL, 0x000000030644e72eULL};     // (p-1) / 2^28
    const uint64_t one[4] = {1, 0, 0, 0}, five[4] = {5, 0, 0, 0};
    uint64_t pm2[4];
    std::memcpy(pm2, F.m, 32);
    pm2[0] -= 2;                                               // (p = 1 mod 2^28: no borrow)
    auto put = [&](uint32_t (&w)[8], const uint64_t v[4]) {    // the device's Montgomery words of v
        uint64_t t[4];
        F.mul(v, R261, t);
        std::memcpy(w, t, 32);
    };
    auto mul = [&](const uint64_t a[4], const uint64_t b[4], uint64_t r[4]) { F.mul(a, b, r); };
    uint64_t c[4], c_inv[4];
    F.pow(five, Q, c);                                         // order 2^28
    F.pow(c, pm2, c_inv);
    for (int j = 0; j < 4; j++) {
        uint64_t step[4], hstep[4];                            // c^(-2^(7j)), c^(-2^(7j - 1)) (j = 0: c^-1, applied every other k)
        std::memcpy(step, c_inv, 32);
        for (int q = 0; q < 7 * j; q++) mul(step, step, step);
        std::memcpy(hstep, c_inv, 32);
        for (int q = 0; q < 7 * j - 1; q++) mul(hstep, hstep, hstep);
        uint64_t m[4], hh[4];
        std::memcpy(m, one, 32);
        std::memcpy(hh, one, 32);
        for (int k = 0; k < 128; k++) {
            if (j < 3) put(h.dl_mul[j][k], m);
            put(h.dl_half[j][k], hh);
            if (j > 0 || (k & 1)) mul(hh, hstep, hh);
            mul(m, step, m);
        }
    }
    uint64_t g3[4], v[4];
    std::memcpy(g3, c, 32);
    for (int q = 0; q < 21; q++) mul(g3, g3, g3);              // order 2^7
    std::vector<uint32_t> low(128);
    std::memcpy(v, one, 32);
    for (int k = 0; k < 128; k++) {
        low[k] = (uint32_t)v[0];
        mul(v, g3, v);
    }
    if (!(v[0] == 1 && v[1] == 0 && v[2] == 0 && v[3] == 0)) return fail(DR_ERR_DEVICE, "bad discrete-logarithm constants");
    for (uint32_t a = 0x9e3779b1u; a > 0x9e3779b1u - 2000000u; a -= 2) {
        std::memset(h.dl_map, 0xff, sizeof h.dl_map);
        std::vector<uint8_t> used(dr::BJJ_DL_SLOTS, 0);
        bool ok = true;
        for (int k = 0; k < 128 && ok; k++) {
            const uint32_t idx = (low[k] * a) >> 20;
            if (used[idx]) ok = false;
            used[idx] = 1;
            h.dl_map[idx] = (uint8_t)k;
        }
        if (ok) { h.dl_hash_mul = a; return DR_OK; }
    }
    return fail(DR_ERR_DEVICE, "no perfect hash for the discrete-logarithm table");
}
int bjj_consts_ready(dr_ctx* ctx) {
    if (ctx->bjj_ready) return DR_OK;
    static std::unique_ptr<dr::BjjConsts> host;                // 33 KB, the same for every context
    static int host_rc = [] { host = std::make_unique<dr::BjjConsts>(); return bjj_consts_build(*host); }();
    if (host_rc != DR_OK) return fail(DR_ERR_DEVICE, "bad Baby JubJub square-root constants");
    HIP_TRY(hipMemcpyToSymbolAsync(HIP_SYMBOL(dr::g_bjj_consts), host.get(), sizeof(dr::BjjConsts), 0, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->bjj_ready = true;
    return DR_OK;
}
struct BjjSuite : Native256<BjjSuite> {
    static constexpr auto scalar_mul = dr::k_bjj_scalar_mul;
    static constexpr auto msm_groups = dr::k_bjj_msm_groups;
    static constexpr auto dec_tai = dr::k_bjj_decode_points<dr::BJJ_DEC_TAI>, dec_check = dr::k_bjj_decode_points<dr::BJJ_DEC_CHECK>,
                          dec_codec = dr::k_bjj_decode_points<dr::BJJ_DEC_CODEC>;
    static constexpr auto field_selftest = dr::k_bjj_field_selftest;
    static constexpr auto law_selftest = dr::k_bjj_law_selftest;
    static constexpr int law_coords = 4;
    static constexpr int block = dr::BJJ_BLOCK, selftest_records = dr::BJJ_SELFTEST_RECORDS;
    static constexpr const char *name = "Baby JubJub", *k_scalar_mul = "k_bjj_scalar_mul", *k_msm_groups = "k_bjj_msm_groups", *k_decode = "k_bjj_decode_points";
    static const drh::Mod256& field() { return drh::mod_pbn254(); }
    static constexpr size_t identity_y = 1, enc_bytes = 32, rec_bytes = 32, tai_bytes = 32;
    static int consts_ready(dr_ctx* ctx) { return bjj_consts_ready(ctx); }
    using Law = dr::BjjLaw;
    using WideCurve = dr::BjjCurve;
    static constexpr int wide_bits = 252;
    DR_WAVE_MSM_STAGES(bjj);
};
// Curve25519_RO / Curve25519_NU (curves 13 and 14, kernels_curve25519.hip.h): Ed25519's group under Montgomery coordinates u || v, 64 bytes
// encoded as they are.  The kernels take and give an identity flag word per point (`flagged`); between the launches, where a point is 64
// bytes and nothing else, the identity is drh::mont_is_identity's 64 bytes of 0xff.  No try-and-increment: dec_tai is the checking decoder.
struct Curve25519Suite : Native256<Curve25519Suite> {
    static constexpr bool flagged = true;
    static constexpr auto scalar_mul = dr::k_c25519_scalar_mul;
    static constexpr auto msm_groups = dr::k_c25519_msm_groups;
    static constexpr auto dec_tai = dr::k_c25519_decode_points<dr::C25519_DEC_CHECK>, dec_check = dr::k_c25519_decode_points<dr::C25519_DEC_CHECK>,
                          dec_codec = dr::k_c25519_decode_points<dr::C25519_DEC_CODEC>;
    static constexpr int block = dr::ED_BLOCK;
    static constexpr const char *name = "Curve25519", *k_scalar_mul = "k_c25519_scalar_mul", *k_msm_groups = "k_c25519_msm_groups",
                                *k_decode = "k_c25519_decode_points";
    static const drh::Mod256& field() { return drh::mod_p25519(); }
    static constexpr size_t identity_y = 0, enc_bytes = 64, rec_bytes = 64, tai_bytes = 64;   // (identity_y does not apply: native_identity)
    // the bucket method: a prepare of its own (the map, once per term), then Ed25519's stages; the host converts the one result
    using Law = dr::C25519Law;
    using WideCurve = dr::Ed25519Curve;
    static constexpr int wide_bits = 254;
    static constexpr bool wide_affine = true;
    static constexpr auto wide_prepare = dr::k_c25519_msm_prepare;
    static constexpr auto wide_sort = dr::k_ed_msm_sort;
    static constexpr auto wide_accumulate = dr::k_ed_msm_accumulate;
    static constexpr auto wide_accumulate_heavy = dr::k_ed_msm_accumulate_heavy;
    static constexpr auto wide_reduce = dr::k_ed_msm_reduce;
    static constexpr auto wide_fold = dr::k_ed_msm_fold;
    static constexpr const char* wide_names[5] = {"k_c25519_msm_prepare", "k_ed_msm_sort", "k_ed_msm_accumulate", "k_ed_msm_reduce", "k_ed_msm_fold"};
    // Elligator 2, times the cofactor 8 unless `clear` is 0; every canonical input has a value, and the flag says that it is the identity
    static int map_launch(dr_ctx* ctx, size_t n, size_t, int per_item, int clear) {
        return launch(ctx, "k_curve25519_map_to_curve", [&] {
            hipLaunchKernelGGL(dr::k_curve25519_map_to_curve, dim3(div_up(n, block)), dim3(block), 0, ctx->stream, ctx->io_a.as<uint32_t>(),
                               ctx->io_b.as<uint32_t>(), ctx->io_c.as<uint32_t>(), (uint32_t)n, (uint32_t)per_item, clear ? 1u : 0u);
        });
    }
};
// the identity as the 64 bytes the host path carries: (0, identity_y), 64 zero bytes on the Weierstrass curves, 64 bytes of 0xff on Curve25519
template <class S>
void native_identity(uint8_t* xy) {
    if constexpr (S::flagged) {
        std::memset(xy, 0xff, 64);
    } else {
        std::memset(xy, 0, 64);
        xy[32] = (uint8_t)S::identity_y;
    }
}
// rc = f(S{}) for the description S of curve cv's native suite; false, f not called, for every other curve and an unknown id
template <class F>
bool on_native(int cv, int& rc, F&& f) {
    switch (drh::te_curve(cv) ? drh::te_curve(cv)->native : drh::NativeSuite::none) {
        case drh::NativeSuite::ed25519: rc = f(Ed25519Suite{}); return true;
        case drh::NativeSuite::p256:
            rc = drh::te_curve(cv)->sswu ? f(P256Sec1Suite{}) : f(P256Suite{});      // (ids 8 and 9: the SEC1 codec)
            return true;
        case drh::NativeSuite::bjj: rc = f(BjjSuite{}); return true;
        case drh::NativeSuite::secp256k1: rc = f(Secp256k1Suite{}); return true;
        case drh::NativeSuite::curve25519: rc = f(Curve25519Suite{}); return true;
        default: return false;
    }
}
// fixed bases through the grouped kernel, each group's terms the m bases: no window table.  te_fixed_base_groups checked the arguments.
template <class S>
int native_fixed_base_groups(S, dr_ctx* ctx, const uint8_t* bases_xy, const uint8_t* scalars, size_t groups, size_t m, uint8_t* out_xy) {
    std::vector<uint8_t> pts(groups * m * 64);
    for (size_t g = 0; g < groups; g++) std::memcpy(pts.data() + 64 * m * g, bases_xy, 64 * m);
    return msm_groups<S>(ctx, pts.data(), scalars, groups, m, out_xy);
}
// one MSM: groups of 64 terms in one launch, then the partial sums with scalar 1, 64 at a time, until one is left.  The host copy of
// the scalars is wiped after every launch, a failed one included.  From NARROW_PIP_FROM terms on: the bucket method
// (capi_wide_msm.hpp), on scalars reduced mod the group order here as load_scalar reduces them in the kernels — the digits are read
// from the words as they are, and on the curves with a cofactor sum (k_i mod n) P_i is what msm_groups returns for points with a
// torsion component.  NOT a fixed schedule: the provers' secret scalars go through scalar_mul_batch and msm_groups.
template <class S>
int native_msm(S, dr_ctx* ctx, const drh::Mod256& order, const uint8_t* pts_xy, const uint8_t* scalars, size_t n, uint8_t out_xy[64]) {
    if (n == 0) {
        native_identity<S>(out_xy);
        return DR_OK;
    }
    if (!pts_xy || !scalars) return fail(DR_ERR_INVALID, "null buffer");
    if (n >= dr::NARROW_PIP_FROM) {
        if (n >= S::max_points) return fail(DR_ERR_INVALID, "batch too large");
        std::vector<uint8_t> reduced(n * 32);
        const auto one = [&](size_t i) {
            uint64_t k[4];
            drh::load_le32(scalars + 32 * i, k);
            if (drh::Mod256::geq(k, order.m)) order.reduce_bytes(scalars + 32 * i, 32, false, k);
            drh::store_le32(k, reduced.data() + 32 * i);
            explicit_bzero(k, sizeof k);
        };
        if (n >= 4096) drh::parallel_for(n, one);
        else for (size_t i = 0; i < n; i++) one(i);
        const int rc = wide_msm_buckets<S>(ctx, pts_xy, reduced.data(), n, out_xy);
        explicit_bzero(reduced.data(), reduced.size());
        return rc;
    }
    std::vector<uint8_t> pts(pts_xy, pts_xy + n * 64), sc(scalars, scalars + n * 32), part;
    for (;;) {
        const size_t parts = (n + 63) / 64, m = parts == 1 ? n : 64;          // the last level: one group of the n <= 64 left
        pts.resize(parts * m * 64, 0);
        sc.resize(parts * m * 32, 0);
        for (size_t i = n; i < parts * m; i++) native_identity<S>(pts.data() + 64 * i);       // padding: 0 * identity
        part.resize(parts * 64);
        const int rc = msm_groups<S>(ctx, pts.data(), sc.data(), parts, m, parts == 1 ? out_xy : part.data());
        explicit_bzero(sc.data(), sc.size());
        if (rc != DR_OK || parts == 1) return rc;
        pts.swap(part);
        n = parts;
        sc.assign(n * 32, 0);
        for (size_t i = 0; i < n; i++) sc[32 * i] = 1;
    }
}
}  // namespace

// ---- the seam to capi_core.hip (capi_internal.hpp): each returns false and does nothing when cv is not a native suite's; otherwise rc
// is the call's result.  The caller has checked what its own function checks first.
bool native_scalar_mul_batch(int cv, int& rc, dr_ctx* ctx, const uint8_t* pts_xy, const uint8_t* scalars, size_t n, uint8_t* out_xy) {
    return on_native(cv, rc, [&](auto S) { return scalar_mul_batch<decltype(S)>(ctx, pts_xy, scalars, n, out_xy); });
}
bool native_msm_groups(int cv, int& rc, dr_ctx* ctx, const uint8_t* pts_xy, const uint8_t* scalars, size_t groups, size_t m, uint8_t* out_xy) {
    return on_native(cv, rc, [&](auto S) { return msm_groups<decltype(S)>(ctx, pts_xy, scalars, groups, m, out_xy); });
}
bool native_fixed_base_groups(int cv, int& rc, dr_ctx* ctx, const uint8_t* bases_xy, const uint8_t* scalars, size_t groups, size_t m, uint8_t* out_xy) {
    return on_native(cv, rc, [&](auto S) { return native_fixed_base_groups(S, ctx, bases_xy, scalars, groups, m, out_xy); });
}
bool native_msm(int cv, int& rc, dr_ctx* ctx, const uint8_t* pts_xy, const uint8_t* scalars, size_t n, uint8_t out_xy[64]) {
    return on_native(cv, rc, [&](auto S) { return native_msm(S, ctx, drh::te_curve(cv)->n, pts_xy, scalars, n, out_xy); });
}
bool native_decode_points(int cv, int& rc, dr_ctx* ctx, bool tai, const uint8_t* enc, size_t n, uint8_t* out_xy, uint8_t* ok) {
    return on_native(cv, rc, [&](auto S) { return decode_points<decltype(S)>(ctx, tai ? S.dec_tai : S.dec_check, enc, n, out_xy, ok); });
}
const NativeSuiteInfo* native_suite_info(int cv) {
    const NativeSuiteInfo* info = nullptr;
    int rc;
    on_native(cv, rc, [&](auto S) {
        static const NativeSuiteInfo of_s{S.enc_bytes, S.tai_bytes, S.identity_y, S.flagged, S.name};
        info = &of_s;
        return DR_OK;
    });
    return info;
}

// ---- the suites' own entry points
int dr_ed25519_decode_points(dr_ctx* ctx, int check, const uint8_t* enc, size_t n, uint8_t* out_xy, uint8_t* ok) {
    return decode_points<Ed25519Suite>(ctx, check ? Ed25519Suite::dec_check : Ed25519Suite::dec_codec, enc, n, out_xy, ok);
}
int dr_p256_decode_points(dr_ctx* ctx, int check, const uint8_t* enc, size_t n, uint8_t* out_xy, uint8_t* ok) {
    return decode_points<P256Suite>(ctx, check ? P256Suite::dec_check : P256Suite::dec_codec, enc, n, out_xy, ok);
}
int dr_bjj_decode_points(dr_ctx* ctx, int check, const uint8_t* enc, size_t n, uint8_t* out_xy, uint8_t* ok) {
    return decode_points<BjjSuite>(ctx, check ? BjjSuite::dec_check : BjjSuite::dec_codec, enc, n, out_xy, ok);
}
int dr_fe25519_ops_selftest(dr_ctx* ctx, const int32_t* a_limbs, const int32_t* b_limbs, size_t n, uint8_t* out, uint8_t* flags) {
    return field_selftest<Ed25519Suite>(ctx, a_limbs, b_limbs, n, out, flags);
}
int dr_p256_field_ops_selftest(dr_ctx* ctx, const int32_t* a_limbs, const int32_t* b_limbs, size_t n, uint8_t* out, uint8_t* flags) {
    return field_selftest<P256Suite>(ctx, a_limbs, b_limbs, n, out, flags);
}
int dr_secp256k1_decode_points(dr_ctx* ctx, int check, const uint8_t* enc, size_t n, uint8_t* out_xy, uint8_t* ok) {
    return decode_points<Secp256k1Suite>(ctx, check ? Secp256k1Suite::dec_check : Secp256k1Suite::dec_codec, enc, n, out_xy, ok);
}
int dr_secp256k1_field_selftest(dr_ctx* ctx, const int32_t* a_limbs, const int32_t* b_limbs, size_t n, uint8_t* out, uint8_t* flags) {
    return field_selftest<Secp256k1Suite>(ctx, a_limbs, b_limbs, n, out, flags);
}
int dr_secp256k1_map_to_curve(dr_ctx* ctx, const uint8_t* us, size_t n, int per_item, uint8_t* out_xy, uint8_t* ok) {
    return map_to_curve<Secp256k1Suite>(ctx, us, n, per_item, 1, out_xy, ok);
}
int dr_p256_map_to_curve(dr_ctx* ctx, const uint8_t* us, size_t n, int per_item, uint8_t* out_xy, uint8_t* ok) {
    return map_to_curve<P256Suite>(ctx, us, n, per_item, 1, out_xy, ok);
}
int dr_ed25519_map_to_curve(dr_ctx* ctx, const uint8_t* us, size_t n, int per_item, uint8_t* out_xy, uint8_t* ok) {
    return map_to_curve<Ed25519Suite>(ctx, us, n, per_item, 1, out_xy, ok);
}
// ---- Curve25519 (kernels_curve25519.hip.h): the entry points with the identity flags spelled out.  The flag bytes go straight to the
// kernels' flag words (IdentityFlags); a point whose flag is 0 must have canonical coordinates, 64 bytes of 0xff included.
int dr_curve25519_scalar_mul_batch(dr_ctx* ctx, const uint8_t* pts_uv, const uint8_t* id_in, const uint8_t* scalars, size_t n, uint8_t* out_uv,
                                   uint8_t* id_out) {
    TRY(use_ctx(ctx));
    if (n && !id_out) return fail(DR_ERR_INVALID, "null buffer");
    const IdentityFlags fl{id_in, id_out};
    return scalar_mul_batch<Curve25519Suite>(ctx, pts_uv, scalars, n, out_uv, &fl);
}
int dr_curve25519_msm_groups(dr_ctx* ctx, const uint8_t* pts_uv, const uint8_t* id_in, const uint8_t* scalars, size_t groups, size_t m,
                             uint8_t* out_uv, uint8_t* id_out) {
    TRY(use_ctx(ctx));
    if (m == 0 || m > 64) return fail(DR_ERR_INVALID, "group size must be in 1..64");
    if (groups >= (1ull << 31) || groups * m >= (1ull << 31)) return fail(DR_ERR_INVALID, "batch too large");
    if (groups && !id_out) return fail(DR_ERR_INVALID, "null buffer");
    const IdentityFlags fl{id_in, id_out};
    return msm_groups<Curve25519Suite>(ctx, pts_uv, scalars, groups, m, out_uv, &fl);
}
int dr_curve25519_decode_points(dr_ctx* ctx, int check, const uint8_t* enc, size_t n, uint8_t* out_uv, uint8_t* ok) {
    return decode_points<Curve25519Suite>(ctx, check ? Curve25519Suite::dec_check : Curve25519Suite::dec_codec, enc, n, out_uv, ok);
}
// n items of per_item (1 or 2) field elements: the sum of their Elligator 2 images, times the cofactor 8 unless clear_cofactor = 0; every
// canonical input has a value (id_out[i] = 1 where it is the identity, its 64 bytes then zeros)
int dr_curve25519_map_to_curve(dr_ctx* ctx, const uint8_t* us, size_t n, int per_item, int clear_cofactor, uint8_t* out_uv, uint8_t* id_out) {
    return map_to_curve<Curve25519Suite>(ctx, us, n, per_item, clear_cofactor, out_uv, id_out);
}
int dr_bjj_field_ops_selftest(dr_ctx* ctx, const int32_t* a_limbs, const int32_t* b_limbs, size_t n, uint8_t* out, uint8_t* flags) {
    return field_selftest<BjjSuite>(ctx, a_limbs, b_limbs, n, out, flags);
}
// the group laws on raw limb images (wave_curve.hip.h's wave_law_selftest; include/dotring_hip.h describes the records)
int dr_ed25519_law_selftest(dr_ctx* ctx, const int32_t* points, const uint32_t* controls, size_t n, int32_t* out) {
    return law_selftest<Ed25519Suite>(ctx, points, controls, n, out);
}
int dr_bjj_law_selftest(dr_ctx* ctx, const int32_t* points, const uint32_t* controls, size_t n, int32_t* out) {
    return law_selftest<BjjSuite>(ctx, points, controls, n, out);
}
int dr_p256_law_selftest(dr_ctx* ctx, const int32_t* points, const uint32_t* controls, size_t n, int32_t* out) {
    return law_selftest<P256Suite>(ctx, points, controls, n, out);
}
int dr_secp256k1_law_selftest(dr_ctx* ctx, const int32_t* points, const uint32_t* controls, size_t n, int32_t* out) {
    return law_selftest<Secp256k1Suite>(ctx, points, controls, n, out);
}
