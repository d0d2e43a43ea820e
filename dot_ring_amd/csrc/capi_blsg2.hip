// libdotring_hip.so — C ABI, part 7 of 8: the BLS12_381_G2 suites (DR_CURVE_BLS12_381_G2 / DR_CURVE_BLS12_381_G2_NU; the reference's
// specs/bls12_381_G2.py).  Coordinates are elements of Fq2, c0 || c1, 48 + 48 bytes little-endian, canonical standard form; points are
// affine x || y, 192 bytes, 192 zero bytes the identity.  None of it goes through the 64-byte paths of capi_core.hip.  The kernels are
// kernels_g2_h2c.hip.h (the complete projective law over fq2_28.hip.h); the host does hash_to_field (expand_message_xmd over SHA-256,
// m = 2, L = 64) on the worker threads and checks that inputs are canonical.  Scalars are 96 bytes used AS THEY ARE: E(Fq2) has order
// h2 r (762 bits), and its points need not lie in G2.
#include "capi_internal.hpp"
#include "kernels_g2_h2c.hip.h"

using namespace dri;

namespace {

constexpr size_t FQ_BYTES = 48, FQ2_BYTES = 96, PT_BYTES = 192, SCALAR_BYTES = 96;

bool fq_canonical(const uint8_t* p) {
    uint64_t v[6];
    std::memcpy(v, p, FQ_BYTES);
    return !drh::Fq::geq_p(v);
}
int check_fq_elems(const uint8_t* p, size_t count, const char* what) {
    for (size_t i = 0; i < count; i++)
        if (!fq_canonical(p + FQ_BYTES * i)) return fail(DR_ERR_INVALID, std::string(what) + " has a component that is not a canonical field element");
    return DR_OK;
}
int check_variant(int variant) {
    return variant == DR_CURVE_BLS12_381_G2 || variant == DR_CURVE_BLS12_381_G2_NU
               ? DR_OK
               : fail(DR_ERR_INVALID, "variant must be DR_CURVE_BLS12_381_G2 or DR_CURVE_BLS12_381_G2_NU");
}
unsigned elems_of(int variant) { return variant == DR_CURVE_BLS12_381_G2_NU ? 1 : 2; }

// 64 big-endian bytes mod p -> 48 bytes little-endian (capi_blsg1.hip's reduction: hi 2^384 + lo through two Montgomery products)
void fq_reduce_be64(const uint8_t* in, uint8_t* out) {
    drh::Fq lo = drh::Fq::zero(), hi = drh::Fq::zero(), r;
    for (int i = 0; i < 48; i++) lo.l[i / 8] |= (uint64_t)in[63 - i] << (8 * (i % 8));
    for (int i = 0; i < 16; i++) hi.l[i / 8] |= (uint64_t)in[15 - i] << (8 * (i % 8));
    std::memcpy(r.l, drh::FieldParams<6>::R2, sizeof r.l);
    (lo.to_mont() + hi.to_mont() * r).store_le(out);
}
// RFC 9380 section 5 for these suites: expand_message_xmd over SHA-256 (Z_pad 64 bytes) to count x m x L = count x 2 x 64 bytes (256 for
// RO, 128 for NU: 8 or 4 blocks), each 64 bytes big-endian mod p, element j = (e_2j, e_2j+1) = c0 || c1; the DST of the variant (the
// `dst` fields of the RFC's vector files).  out: count x 96 bytes little-endian.
void hash_to_field(int variant, const uint8_t* salt, size_t salt_len, const uint8_t* msg, size_t len, uint8_t* out) {
    const unsigned count = elems_of(variant);
    drh::Bytes dst;
    drh::put(dst, count == 2 ? "QUUX-V01-CS02-with-BLS12381G2_XMD:SHA-256_SSWU_RO_" : "QUUX-V01-CS02-with-BLS12381G2_XMD:SHA-256_SSWU_NU_", 50);
    drh::put8(dst, (uint8_t)dst.size());             // DST_prime = DST || len(DST)
    const size_t L = 128 * (size_t)count;
    uint8_t b0[32], prev[32], raw[256];
    const uint8_t zpad[64] = {0};
    drh::Sha256 h;
    h.update(zpad, 64);
    if (salt_len) h.update(salt, salt_len);
    if (len) h.update(msg, len);
    const uint8_t lb[3] = {(uint8_t)(L >> 8), (uint8_t)L, 0};
    h.update(lb, 3);
    h.update(dst.data(), dst.size());
    h.final(b0);
    for (size_t i = 1; 32 * (i - 1) < L; i++) {
        drh::Sha256 g;
        uint8_t x[32];
        for (size_t j = 0; j < 32; j++) x[j] = i == 1 ? b0[j] : (uint8_t)(b0[j] ^ prev[j]);
        g.update(x, 32);
        const uint8_t ib = (uint8_t)i;
        g.update(&ib, 1);
        g.update(dst.data(), dst.size());
        g.final(prev);
        std::memcpy(raw + 32 * (i - 1), prev, 32);
    }
    for (unsigned k = 0; k < 2 * count; k++) fq_reduce_be64(raw + 64 * k, out + FQ_BYTES * k);
}

// n items of per_item canonical Fq2 elements at `us` (host): the two launches of the map on the context's stream (images through
// ctx->partial, a scratch buffer that ctx_wipe_scratch zeroes with the rest), points and flags back
int map_to_curve(dr_ctx* ctx, const uint8_t* us, size_t n, int per_item, int clear, uint8_t* out_xy, uint8_t* ok) {
    const size_t elems = n * (size_t)per_item;
    TRY(ctx->io_a.reserve(elems * FQ2_BYTES));
    TRY(ctx->io_b.reserve(n * PT_BYTES));
    TRY(ctx->io_c.reserve((n + elems) * 4));
    TRY(ctx->partial.reserve(elems * dr::G2H_STAGE_WORDS * 4));
    uint32_t* ok_item = ctx->io_c.as<uint32_t>();
    uint32_t* ok_elem = ok_item + n;
    HIP_TRY(hipMemcpyAsync(ctx->io_a.p, us, elems * FQ2_BYTES, hipMemcpyHostToDevice, ctx->stream));
    TRY(launch(ctx, "k_blsg2_map_iso", [&] {
        hipLaunchKernelGGL(dr::k_blsg2_map_iso, dim3(div_up(elems, dr::G2H_BLOCK)), dim3(dr::G2H_BLOCK), 0, ctx->stream, ctx->io_a.as<uint32_t>(),
                           ctx->partial.as<int32_t>(), ok_elem, (uint32_t)elems);
    }));
    TRY(launch(ctx, "k_blsg2_sum_clear", [&] {
        hipLaunchKernelGGL(dr::k_blsg2_sum_clear, dim3(div_up(n, dr::G2H_BLOCK)), dim3(dr::G2H_BLOCK), 0, ctx->stream, ctx->partial.as<int32_t>(),
                           ok_elem, ctx->io_b.as<uint32_t>(), ok_item, (uint32_t)n, (uint32_t)per_item, clear ? 1u : 0u);
    }));
    std::vector<uint32_t> flags(n);
    HIP_TRY(hipMemcpyAsync(out_xy, ctx->io_b.p, n * PT_BYTES, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(flags.data(), ok_item, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (ctx->prof) TRY(prof_collect(ctx));
    for (size_t i = 0; i < n; i++) ok[i] = flags[i] ? 1 : 0;
    return DR_OK;
}

}  // namespace

int dr_blsg2_hash_to_field_batch(int variant, const uint8_t* msgs, const uint64_t* off, size_t count, uint8_t* out) {
    TRY(check_variant(variant));
    if (count == 0) return DR_OK;
    if (!off || !out || (off[count] && !msgs)) return fail(DR_ERR_INVALID, "null buffer");
    for (size_t i = 0; i < count; i++)
        if (off[i + 1] < off[i]) return fail(DR_ERR_INVALID, "message offsets must not decrease");
    const size_t per = elems_of(variant);
    drh::parallel_for(count, [&](size_t i) { hash_to_field(variant, nullptr, 0, msgs + off[i], off[i + 1] - off[i], out + FQ2_BYTES * per * i); });
    return DR_OK;
}

int dr_blsg2_map_to_curve(dr_ctx* ctx, const uint8_t* us, size_t n, int per_item, int clear, uint8_t* out_xy, uint8_t* ok) {
    TRY(use_ctx(ctx));
    if (per_item != 1 && per_item != 2) return fail(DR_ERR_INVALID, "one (nonuniform) or two (uniform, RO) field elements per item");
    if (n == 0) return DR_OK;
    if (!us || !out_xy || !ok) return fail(DR_ERR_INVALID, "null buffer");
    if (n >= (1ull << 28)) return fail(DR_ERR_INVALID, "batch too large");
    TRY(check_fq_elems(us, 2 * n * (size_t)per_item, "input"));
    return map_to_curve(ctx, us, n, per_item, clear, out_xy, ok);
}

int dr_blsg2_encode_to_curve_batch(dr_ctx* ctx, int variant, const uint8_t* msgs, const uint64_t* off, const uint8_t* salts,
                                   const uint64_t* salt_off, size_t count, uint8_t* out_xy) {
    TRY(use_ctx(ctx));
    TRY(check_variant(variant));
    if (count == 0) return DR_OK;
    if (!off || !out_xy || (off[count] && !msgs) || (salts && !salt_off)) return fail(DR_ERR_INVALID, "null buffer");
    if (count >= (1ull << 28)) return fail(DR_ERR_INVALID, "batch too large");
    for (size_t i = 0; i < count; i++)
        if (off[i + 1] < off[i] || (salts && salt_off[i + 1] < salt_off[i])) return fail(DR_ERR_INVALID, "offsets must not decrease");
    const size_t per = elems_of(variant);
    std::vector<uint8_t> us(count * per * FQ2_BYTES), ok(count);
    drh::parallel_for(count, [&](size_t i) {
        hash_to_field(variant, salts ? salts + salt_off[i] : nullptr, salts ? salt_off[i + 1] - salt_off[i] : 0, msgs + off[i], off[i + 1] - off[i],
                      us.data() + FQ2_BYTES * per * i);
    });
    TRY(map_to_curve(ctx, us.data(), count, (int)per, 1, out_xy, ok.data()));
    for (size_t i = 0; i < count; i++)       // (no input reaches this: kernels_g2_h2c.hip.h, g2h_iso_map)
        if (!ok[i]) return fail(DR_ERR_INVALID, "the map to the curve has no value for a message (an isogeny denominator vanishes)");
    return DR_OK;
}

int dr_blsg2_scalar_mul_batch(dr_ctx* ctx, const uint8_t* pts_xy, const uint8_t* scalars, size_t n, uint8_t* out_xy) {
    TRY(use_ctx(ctx));
    if (n == 0) return DR_OK;
    if (!pts_xy || !scalars || !out_xy) return fail(DR_ERR_INVALID, "null buffer");
    if (n >= (1ull << 28)) return fail(DR_ERR_INVALID, "batch too large");
    TRY(check_fq_elems(pts_xy, 4 * n, "point coordinate"));
    TRY(ctx->io_a.reserve(n * PT_BYTES));
    TRY(ctx->io_b.reserve(n * SCALAR_BYTES));
    TRY(ctx->io_c.reserve(n * PT_BYTES));
    HIP_TRY(hipMemcpyAsync(ctx->io_a.p, pts_xy, n * PT_BYTES, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(ctx->io_b.p, scalars, n * SCALAR_BYTES, hipMemcpyHostToDevice, ctx->stream));
    TRY(launch(ctx, "k_blsg2_scalar_mul", [&] {
        hipLaunchKernelGGL(dr::k_blsg2_scalar_mul, dim3(div_up(n, dr::G2H_BLOCK)), dim3(dr::G2H_BLOCK), 0, ctx->stream, ctx->io_a.as<uint32_t>(),
                           ctx->io_b.as<uint32_t>(), ctx->io_c.as<uint32_t>(), (uint32_t)n);
    }));
    HIP_TRY(hipMemcpyAsync(out_xy, ctx->io_c.p, n * PT_BYTES, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (ctx->prof) TRY(prof_collect(ctx));
    return DR_OK;
}

int dr_blsg2_check_points(dr_ctx* ctx, int subgroup, const uint8_t* pts_xy, size_t n, uint8_t* ok) {
    TRY(use_ctx(ctx));
    if (n == 0) return DR_OK;
    if (!pts_xy || !ok) return fail(DR_ERR_INVALID, "null buffer");
    if (n >= (1ull << 28)) return fail(DR_ERR_INVALID, "batch too large");
    TRY(check_fq_elems(pts_xy, 4 * n, "point coordinate"));
    TRY(ctx->io_a.reserve(n * PT_BYTES));
    TRY(ctx->io_c.reserve(n * 4));
    HIP_TRY(hipMemcpyAsync(ctx->io_a.p, pts_xy, n * PT_BYTES, hipMemcpyHostToDevice, ctx->stream));
    TRY(launch(ctx, "k_blsg2_check_points", [&] {
        const auto kernel = subgroup ? dr::k_blsg2_check_points<dr::G2H_CHECK_SUBGROUP> : dr::k_blsg2_check_points<dr::G2H_CHECK_CURVE>;
        hipLaunchKernelGGL(kernel, dim3(div_up(n, dr::G2H_BLOCK)), dim3(dr::G2H_BLOCK), 0, ctx->stream, ctx->io_a.as<uint32_t>(),
                           ctx->io_c.as<uint32_t>(), (uint32_t)n);
    }));
    std::vector<uint32_t> flags(n);
    HIP_TRY(hipMemcpyAsync(flags.data(), ctx->io_c.p, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (ctx->prof) TRY(prof_collect(ctx));
    for (size_t i = 0; i < n; i++) ok[i] = flags[i] ? 1 : 0;
    return DR_OK;
}

int dr_blsg2_field_selftest(dr_ctx* ctx, const int32_t* a_limbs, const int32_t* b_limbs, size_t n, uint8_t* out, uint8_t* flags) {
    TRY(use_ctx(ctx));
    if (n == 0) return DR_OK;
    if (!a_limbs || !b_limbs || !out || !flags) return fail(DR_ERR_INVALID, "null buffer");
    if (n >= (1ull << 24)) return fail(DR_ERR_INVALID, "batch too large");
    constexpr size_t LIMB_BYTES = 4 * 2 * dr::L28, REC = (size_t)dr::G2H_SELFTEST_RECORDS * FQ2_BYTES;
    TRY(ctx->io_a.reserve(n * 2 * LIMB_BYTES));
    TRY(ctx->io_b.reserve(n * REC));
    TRY(ctx->io_c.reserve(n * 4));
    HIP_TRY(hipMemcpyAsync(ctx->io_a.p, a_limbs, n * LIMB_BYTES, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(ctx->io_a.as<uint8_t>() + n * LIMB_BYTES, b_limbs, n * LIMB_BYTES, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(dr::k_blsg2_field_selftest, dim3(div_up(n, 64)), dim3(64), 0, ctx->stream, ctx->io_a.as<int32_t>(),
                       (const int32_t*)(ctx->io_a.as<uint8_t>() + n * LIMB_BYTES), (uint32_t)n, ctx->io_b.as<uint32_t>(), ctx->io_c.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    std::vector<uint32_t> fl(n);
    HIP_TRY(hipMemcpyAsync(out, ctx->io_b.p, n * REC, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(fl.data(), ctx->io_c.p, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < n; i++) flags[i] = (uint8_t)fl[i];
    return DR_OK;
}
