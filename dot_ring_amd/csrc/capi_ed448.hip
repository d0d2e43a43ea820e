// libdotring_hip.so — C ABI, part 8 of 8: the Ed448 suites (DR_CURVE_ED448_RO / DR_CURVE_ED448_NU; the reference's specs/ed448.py).
// Field elements and coordinates are 56 bytes little-endian, canonical; points are affine x || y, 112 bytes, the identity (0, 1) as itself;
// scalars are 56 bytes used AS THEY ARE.  None of it goes through the 64-byte paths of capi_core.hip.  The kernels are
// kernels_ed448.hip.h over fe448.hip.h; the host does hash_to_field (expand_message_xof over SHAKE256, L = 84) on the worker threads and
// checks that inputs are canonical.  Scalars may be secret: they pass through io_a / io_b / io_c only, which ctx_wipe_scratch covers.
#include "capi_internal.hpp"
#include "hosthash.hpp"
#include "kernels_ed448.hip.h"

using namespace dri;

namespace {

constexpr size_t FE_BYTES = 56, PT_BYTES = 112, SCALAR_BYTES = 56, XOF_L = 84;

// p = 2^448 - 2^224 - 1 as seven 64-bit words: all ones but bit 224 (word 3, bit 32)
constexpr uint64_t P448[7] = {~0ull, ~0ull, ~0ull, 0xfffffffeffffffffull, ~0ull, ~0ull, ~0ull};

bool fe_canonical(const uint8_t* p) {
    uint64_t v[7];
    std::memcpy(v, p, FE_BYTES);
    for (int i = 6; i >= 0; i--)
        if (v[i] != P448[i]) return v[i] < P448[i];
    return false;
}
int check_fe_elems(const uint8_t* p, size_t count, const char* what) {
    for (size_t i = 0; i < count; i++)
        if (!fe_canonical(p + FE_BYTES * i)) return fail(DR_ERR_INVALID, std::string(what) + " is not a canonical field element");
    return DR_OK;
}
int check_variant(int variant) {
    return variant == DR_CURVE_ED448_RO || variant == DR_CURVE_ED448_NU ? DR_OK
                                                                         : fail(DR_ERR_INVALID, "variant must be DR_CURVE_ED448_RO or DR_CURVE_ED448_NU");
}
unsigned elems_of(int variant) { return variant == DR_CURVE_ED448_NU ? 1 : 2; }

// v (8 words, below 2^449 + 2^225) -= p while it is not below p (at most three times)
void fe_reduce_small(uint64_t (&v)[8]) {
    for (int pass = 0; pass < 3; pass++) {
        uint64_t d[8], borrow = 0;
        for (int i = 0; i < 8; i++) {
            const uint64_t pw = i < 7 ? P448[i] : 0;
            const unsigned __int128 t = (unsigned __int128)v[i] - pw - borrow;
            d[i] = (uint64_t)t;
            borrow = (uint64_t)(t >> 64) & 1;
        }
        if (!borrow) std::memcpy(v, d, sizeof d);
    }
}
// 84 big-endian bytes (672 bits) mod p -> 56 bytes little-endian: hi 2^448 + lo = lo + hi + hi 2^224 (hi of 224 bits)
void fe_reduce_be84(const uint8_t* in, uint8_t* out) {
    uint8_t le[88] = {0};
    for (size_t i = 0; i < XOF_L; i++) le[i] = in[XOF_L - 1 - i];
    uint64_t lo[8] = {0}, hi[8] = {0}, hs[8] = {0};
    std::memcpy(lo, le, 56);
    std::memcpy(hi, le + 56, 28);
    std::memcpy(reinterpret_cast<uint8_t*>(hs) + 28, le + 56, 28);      // hi << 224
    uint64_t v[8];
    unsigned __int128 c = 0;
    for (int i = 0; i < 8; i++) {
        c += (unsigned __int128)lo[i] + hi[i] + hs[i];
        v[i] = (uint64_t)c;
        c >>= 64;
    }
    fe_reduce_small(v);
    std::memcpy(out, v, FE_BYTES);
}
// RFC 9380 section 5.3.3 for these suites: expand_message_xof over SHAKE256 to count x 84 bytes (168 for RO, 84 for NU), each 84 bytes
// big-endian mod p; the DST of the variant (the reference's hash_to_curve_dst: _RO_ replaced by _NU_).  out: count x 56 bytes.
void hash_to_field(int variant, const uint8_t* salt, size_t salt_len, const uint8_t* msg, size_t len, uint8_t* out) {
    const unsigned count = elems_of(variant);
    static const char DST_RO[] = "QUUX-V01-CS02-with-edwards448_XOF:SHAKE256_ELL2_RO_", DST_NU[] = "QUUX-V01-CS02-with-edwards448_XOF:SHAKE256_ELL2_NU_";
    const char* dst = count == 2 ? DST_RO : DST_NU;
    const size_t dst_len = sizeof DST_RO - 1, L = XOF_L * count;
    drh::Shake256 h;
    if (salt_len) h.update(salt, salt_len);
    if (len) h.update(msg, len);
    const uint8_t lb[2] = {(uint8_t)(L >> 8), (uint8_t)L};
    h.update(lb, 2);
    h.update(dst, dst_len);
    const uint8_t dl = (uint8_t)dst_len;
    h.update(&dl, 1);
    uint8_t raw[2 * XOF_L];
    h.digest(raw, L);
    for (unsigned k = 0; k < count; k++) fe_reduce_be84(raw + XOF_L * k, out + FE_BYTES * k);
}

int map_to_curve(dr_ctx* ctx, const uint8_t* us, size_t n, int per_item, int clear, uint8_t* out_xy, uint8_t* ok) {
    const size_t elems = n * (size_t)per_item;
    TRY(ctx->io_a.reserve(elems * FE_BYTES));
    TRY(ctx->io_b.reserve(n * PT_BYTES));
    TRY(ctx->io_c.reserve(n * 4));
    HIP_TRY(hipMemcpyAsync(ctx->io_a.p, us, elems * FE_BYTES, hipMemcpyHostToDevice, ctx->stream));
    TRY(launch(ctx, "k_ed448_map_to_curve", [&] {
        hipLaunchKernelGGL(dr::k_ed448_map_to_curve, dim3(div_up(n, dr::E448_BLOCK)), dim3(dr::E448_BLOCK), 0, ctx->stream, ctx->io_a.as<uint32_t>(),
                           ctx->io_b.as<uint32_t>(), ctx->io_c.as<uint32_t>(), (uint32_t)n, (uint32_t)per_item, clear ? 1u : 0u);
    }));
    std::vector<uint32_t> flags(n);
    HIP_TRY(hipMemcpyAsync(out_xy, ctx->io_b.p, n * PT_BYTES, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(flags.data(), ctx->io_c.p, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (ctx->prof) TRY(prof_collect(ctx));
    for (size_t i = 0; i < n; i++) ok[i] = flags[i] ? 1 : 0;
    return DR_OK;
}

// n points (coordinates checked) and n scalars to io_a / io_b, one launch (`go`, profiled as `name`) into io_c, n_out points back
template <class F>
int run_points(dr_ctx* ctx, const char* name, const uint8_t* pts_xy, const uint8_t* scalars, size_t n, size_t n_out, uint8_t* out_xy, F&& go) {
    if (!pts_xy || !scalars || !out_xy) return fail(DR_ERR_INVALID, "null buffer");
    if (n >= (1ull << 29)) return fail(DR_ERR_INVALID, "batch too large");
    TRY(check_fe_elems(pts_xy, 2 * n, "a point coordinate"));
    TRY(ctx->io_a.reserve(n * PT_BYTES));
    TRY(ctx->io_b.reserve(n * SCALAR_BYTES));
    TRY(ctx->io_c.reserve(n_out * PT_BYTES));
    HIP_TRY(hipMemcpyAsync(ctx->io_a.p, pts_xy, n * PT_BYTES, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(ctx->io_b.p, scalars, n * SCALAR_BYTES, hipMemcpyHostToDevice, ctx->stream));
    TRY(launch(ctx, name, go));
    HIP_TRY(hipMemcpyAsync(out_xy, ctx->io_c.p, n_out * PT_BYTES, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (ctx->prof) TRY(prof_collect(ctx));
    return DR_OK;
}

}  // namespace

int dr_ed448_hash_to_field_batch(int variant, const uint8_t* msgs, const uint64_t* off, size_t count, uint8_t* out) {
    TRY(check_variant(variant));
    if (count == 0) return DR_OK;
    if (!off || !out || (off[count] && !msgs)) return fail(DR_ERR_INVALID, "null buffer");
    for (size_t i = 0; i < count; i++)
        if (off[i + 1] < off[i]) return fail(DR_ERR_INVALID, "message offsets must not decrease");
    const size_t per = elems_of(variant);
    drh::parallel_for(count, [&](size_t i) { hash_to_field(variant, nullptr, 0, msgs + off[i], off[i + 1] - off[i], out + FE_BYTES * per * i); });
    return DR_OK;
}

int dr_ed448_map_to_curve(dr_ctx* ctx, const uint8_t* us, size_t n, int per_item, int clear, uint8_t* out_xy, uint8_t* ok) {
    TRY(use_ctx(ctx));
    if (per_item != 1 && per_item != 2) return fail(DR_ERR_INVALID, "one (nonuniform) or two (uniform, RO) field elements per item");
    if (n == 0) return DR_OK;
    if (!us || !out_xy || !ok) return fail(DR_ERR_INVALID, "null buffer");
    if (n >= (1ull << 28)) return fail(DR_ERR_INVALID, "batch too large");
    TRY(check_fe_elems(us, n * (size_t)per_item, "an input"));
    return map_to_curve(ctx, us, n, per_item, clear, out_xy, ok);
}

int dr_ed448_encode_to_curve_batch(dr_ctx* ctx, int variant, const uint8_t* msgs, const uint64_t* off, const uint8_t* salts,
                                   const uint64_t* salt_off, size_t count, uint8_t* out_xy) {
    TRY(use_ctx(ctx));
    TRY(check_variant(variant));
    if (count == 0) return DR_OK;
    if (!off || !out_xy || (off[count] && !msgs) || (salts && !salt_off)) return fail(DR_ERR_INVALID, "null buffer");
    if (count >= (1ull << 28)) return fail(DR_ERR_INVALID, "batch too large");
    for (size_t i = 0; i < count; i++)
        if (off[i + 1] < off[i] || (salts && salt_off[i + 1] < salt_off[i])) return fail(DR_ERR_INVALID, "offsets must not decrease");
    const size_t per = elems_of(variant);
    std::vector<uint8_t> us(count * per * FE_BYTES), ok(count);
    drh::parallel_for(count, [&](size_t i) {
        hash_to_field(variant, salts ? salts + salt_off[i] : nullptr, salts ? salt_off[i + 1] - salt_off[i] : 0, msgs + off[i], off[i + 1] - off[i],
                      us.data() + FE_BYTES * per * i);
    });
    TRY(map_to_curve(ctx, us.data(), count, (int)per, 1, out_xy, ok.data()));
    for (size_t i = 0; i < count; i++)       // (a field element in {0, 1, p - 1}: kernels_ed448.hip.h, e448_ell2_map)
        if (!ok[i]) return fail(DR_ERR_INVALID, "the map to the curve has no value for a message (Point is not on the curve)");
    return DR_OK;
}

int dr_ed448_scalar_mul_batch(dr_ctx* ctx, const uint8_t* pts_xy, const uint8_t* scalars, size_t n, uint8_t* out_xy) {
    TRY(use_ctx(ctx));
    if (n == 0) return DR_OK;
    return run_points(ctx, "k_ed448_scalar_mul", pts_xy, scalars, n, n, out_xy, [&] {
        hipLaunchKernelGGL(dr::k_ed448_scalar_mul, dim3(div_up(n, dr::E448_BLOCK)), dim3(dr::E448_BLOCK), 0, ctx->stream, ctx->io_a.as<uint32_t>(),
                           ctx->io_b.as<uint32_t>(), ctx->io_c.as<uint32_t>(), (uint32_t)n);
    });
}

int dr_ed448_msm_groups(dr_ctx* ctx, const uint8_t* pts_xy, const uint8_t* scalars, size_t groups, size_t m, uint8_t* out_xy) {
    TRY(use_ctx(ctx));
    if (groups == 0) return DR_OK;
    if (m == 0 || m > 64) return fail(DR_ERR_INVALID, "group size must be in 1..64");
    if (groups >= (1ull << 29) || groups * m >= (1ull << 29)) return fail(DR_ERR_INVALID, "batch too large");
    uint32_t mpad = 1;
    while (mpad < m) mpad <<= 1;
    const uint32_t per_block = dr::E448_BLOCK / mpad;
    return run_points(ctx, "k_ed448_msm_groups", pts_xy, scalars, groups * m, groups, out_xy, [&] {
        hipLaunchKernelGGL(dr::k_ed448_msm_groups, dim3(div_up(groups, per_block)), dim3(dr::E448_BLOCK), 0, ctx->stream, ctx->io_a.as<uint32_t>(),
                           ctx->io_b.as<uint32_t>(), ctx->io_c.as<uint32_t>(), (uint32_t)groups, (uint32_t)m, mpad);
    });
}

int dr_ed448_decode_points(dr_ctx* ctx, int check, const uint8_t* enc, size_t n, uint8_t* out_xy, uint8_t* ok) {
    TRY(use_ctx(ctx));
    if (n == 0) return DR_OK;
    if (!enc || !out_xy || !ok) return fail(DR_ERR_INVALID, "null buffer");
    if (n >= (1ull << 29)) return fail(DR_ERR_INVALID, "batch too large");
    TRY(ctx->io_a.reserve(n * PT_BYTES));
    TRY(ctx->io_b.reserve(n * PT_BYTES));
    TRY(ctx->io_c.reserve(n * 4));
    HIP_TRY(hipMemcpyAsync(ctx->io_a.p, enc, n * PT_BYTES, hipMemcpyHostToDevice, ctx->stream));
    TRY(launch(ctx, "k_ed448_check_points", [&] {
        const auto kernel = check ? dr::k_ed448_check_points<1> : dr::k_ed448_check_points<0>;
        hipLaunchKernelGGL(kernel, dim3(div_up(n, dr::E448_BLOCK)), dim3(dr::E448_BLOCK), 0, ctx->stream, ctx->io_a.as<uint32_t>(),
                           ctx->io_b.as<uint32_t>(), ctx->io_c.as<uint32_t>(), (uint32_t)n);
    }));
    std::vector<uint32_t> flags(n);
    HIP_TRY(hipMemcpyAsync(out_xy, ctx->io_b.p, n * PT_BYTES, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(flags.data(), ctx->io_c.p, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (ctx->prof) TRY(prof_collect(ctx));
    for (size_t i = 0; i < n; i++) ok[i] = flags[i] ? 1 : 0;
    return DR_OK;
}

int dr_ed448_field_selftest(dr_ctx* ctx, const int32_t* a_limbs, const int32_t* b_limbs, size_t n, uint8_t* out, uint8_t* flags) {
    TRY(use_ctx(ctx));
    if (n == 0) return DR_OK;
    if (!a_limbs || !b_limbs || !out || !flags) return fail(DR_ERR_INVALID, "null buffer");
    if (n >= (1ull << 24)) return fail(DR_ERR_INVALID, "batch too large");
    constexpr size_t LIMB_BYTES = 4 * dr::L448, REC = (size_t)dr::E448_SELFTEST_RECORDS * FE_BYTES;
    TRY(ctx->io_a.reserve(n * 2 * LIMB_BYTES));
    TRY(ctx->io_b.reserve(n * REC));
    TRY(ctx->io_c.reserve(n * 4));
    HIP_TRY(hipMemcpyAsync(ctx->io_a.p, a_limbs, n * LIMB_BYTES, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(ctx->io_a.as<uint8_t>() + n * LIMB_BYTES, b_limbs, n * LIMB_BYTES, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(dr::k_ed448_field_selftest, dim3(div_up(n, 64)), dim3(64), 0, ctx->stream, ctx->io_a.as<int32_t>(),
                       (const int32_t*)(ctx->io_a.as<uint8_t>() + n * LIMB_BYTES), (uint32_t)n, ctx->io_b.as<uint32_t>(), ctx->io_c.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    std::vector<uint32_t> fl(n);
    HIP_TRY(hipMemcpyAsync(out, ctx->io_b.p, n * REC, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(fl.data(), ctx->io_c.p, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < n; i++) flags[i] = (uint8_t)fl[i];
    return DR_OK;
}
