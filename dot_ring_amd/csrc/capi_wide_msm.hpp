// The host path of the bucket method (wave_msm.hip.h), once for every suite that has it: ONE variable-base MSM of n terms in the forms
// of the suite's msm_groups.
//   wide_msm<S>          dr_wide_msm for the four wide suites (capi_p384.hip, capi_p521.hip, capi_ed448.hip with Ed448 and Curve448) and
//                        dr_blsg1_msm (capi_blsg1.hip): below S::wide_from terms it launches msm_groups in chunks of up to 64 and folds the
//                        partial sums with the suite's law on the host; from there on wide_msm_buckets
//   wide_msm_buckets<S>  the bucket method by msm_plan.hpp's plan_wide_msm, the set sums combined on the host (wide_combine.hpp); also
//                        what native_msm (capi_native256.hip) calls from NARROW_PIP_FROM terms for the five 256-bit suites
// No kernel is defined here.  Beyond capi_suite.hpp's members a suite S gives
//   Law                                        the law as the host runs it, with the ABI's words <-> a point (P384Law, ...; narrow_law.hpp)
//   wide_bits                                  what the tiling covers: one bit more than a scalar can have (wide_recode.hip.h)
//   wide_prepare, wide_sort, wide_accumulate, wide_accumulate_heavy, wide_reduce, wide_fold   the stages' kernels
//   wide_affine, WideCurve                     the fold leaves affine ABI points, not records of limb images (the law is not over the
//                                              device's limbs), and the device description the record size comes from
//   wide_names                                 the launches' profile names (SuiteDefaults: k_wide_msm_*)
// The bucket path is NOT a fixed schedule (wave_msm.hip.h); secret scalars go through scalar_mul_batch and msm_groups.  Scalars travel as
// te_msm_pippenger's do: uploaded to ctx->scalars, digits and lists in the MSM workspaces — all of it what ctx_wipe_scratch covers.
#pragma once
#include "capi_suite.hpp"
#include "wave_msm.hip.h"
#include "wide_combine.hpp"

// The stage members of a suite whose six kernels are one expansion of wave_msm.hip.h's macros under NAME.
//   DR_WAVE_MSM_STAGES_RECORDS  after DR_WAVE_MSM_KERNELS_RECORDS (p384, p521, ed448): the six kernels; record set sums and the profile
//                               names k_wide_msm_* with the fold unnamed stay SuiteDefaults'
//   DR_WAVE_MSM_STAGES          after DR_WAVE_MSM_KERNELS (ed, bjj, p256, secp256k1, blsg1, blsg2): the same six, affine set sums, and
//                               each launch under its kernel's name
// (Curve448Suite and Curve25519Suite mix a prepare of their own with another suite's stages and list their members.)
#define DR_WAVE_MSM_STAGES_RECORDS(NAME)                                                                                               \
    static constexpr auto wide_prepare = dr::k_##NAME##_msm_prepare;                                                                   \
    static constexpr auto wide_sort = dr::k_##NAME##_msm_sort;                                                                         \
    static constexpr auto wide_accumulate = dr::k_##NAME##_msm_accumulate;                                                             \
    static constexpr auto wide_accumulate_heavy = dr::k_##NAME##_msm_accumulate_heavy;                                                 \
    static constexpr auto wide_reduce = dr::k_##NAME##_msm_reduce;                                                                     \
    static constexpr auto wide_fold = dr::k_##NAME##_msm_fold
#define DR_WAVE_MSM_STAGES(NAME)                                                                                                       \
    DR_WAVE_MSM_STAGES_RECORDS(NAME);                                                                                                  \
    static constexpr bool wide_affine = true;                                                                                          \
    static constexpr const char* wide_names[5] = {"k_" #NAME "_msm_prepare", "k_" #NAME "_msm_sort", "k_" #NAME "_msm_accumulate",      \
                                                  "k_" #NAME "_msm_reduce", "k_" #NAME "_msm_fold"}

namespace dri {

// the words of a device record and of what the fold leaves per set: a record of limb images, or (S::wide_affine) the ABI's affine point
template <class S>
constexpr size_t wide_rec_words() {
    if constexpr (S::wide_affine) return (size_t)dr::wave_msm_record_words<typename S::WideCurve>();
    else return (size_t)dr::wide_record_words<typename S::Law>();
}

// the bucket method itself: n >= the suite's threshold terms, no null buffer, n < S::max_points
template <class S>
int wide_msm_buckets(dr_ctx* ctx, const uint8_t* pts, const uint8_t* scalars, size_t n, uint8_t* out) {
    using Law = typename S::Law;
    using Point = typename Law::Point;
    constexpr size_t PW = S::pt_bytes / 4, REC = wide_rec_words<S>(), SUM = S::wide_affine ? PW : REC;
    static_assert(PW == 2 * (size_t)Law::WORDS, "a point is two coordinates");
    // the checks of run_points
    if constexpr (S::checks_scalars) {
        if (!S::scalars_ok(scalars, n)) return fail(DR_ERR_INVALID, S::scalar_refusal);
    }
    std::vector<uint8_t> clean;
    std::vector<uint32_t> flags_in;
    if constexpr (S::flagged) {
        drh::split_identities(pts, n, S::pt_bytes, false, nullptr, clean, flags_in);
        if (!clean.empty()) pts = clean.data();
    }
    TRY(check_canonical<S>(pts, n * S::pt_bytes, "point coordinate"));

    const dr::WideMsmPlan plan = dr::plan_wide_msm(n, S::wide_bits);
    const uint32_t H = plan.H, L = plan.L, T = plan.T, groups = plan.groups;
    const size_t sets = plan.sets, nbuckets = plan.nbuckets, per_set = plan.per_set;
    if (H > dr::WIDE_MAX_H || sets * per_set >= (1ull << 31) || nbuckets >= (1ull << 31)) return fail(DR_ERR_INVALID, "bad MSM size");
    hipStream_t st = ctx->stream;
    TRY(ctx->io_a.reserve(n * (S::pt_bytes + (S::flagged ? 4 : 0))));
    TRY(ctx->io_b.reserve(n * REC * 4));
    TRY(ctx->scalars.reserve(n * S::scalar_bytes));
    TRY(ctx->counts.reserve(nbuckets * 4));
    TRY(ctx->offsets.reserve((nbuckets + 1) * 4));
    TRY(ctx->sorted.reserve(sets * per_set * 4));
    TRY(ctx->buckets.reserve(nbuckets * REC * 4));
    TRY(ctx->partial.reserve(sets * T * REC * 4));
    TRY(ctx->winsum.reserve(sets * SUM * 4));
    HIP_TRY(hipMemcpyAsync(ctx->io_a.p, pts, n * S::pt_bytes, hipMemcpyHostToDevice, st));
    if constexpr (S::flagged) HIP_TRY(hipMemcpyAsync(ctx->io_a.as<uint8_t>() + n * S::pt_bytes, flags_in.data(), n * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ctx->scalars.p, scalars, n * S::scalar_bytes, hipMemcpyHostToDevice, st));
    TRY(launch(ctx, S::wide_names[0], [&] {
        if constexpr (S::flagged)
            hipLaunchKernelGGL(S::wide_prepare, dim3(div_up(n, dr::WMSM_BLOCK)), dim3(dr::WMSM_BLOCK), 0, st, ctx->io_a.as<uint32_t>(),
                               ctx->io_a.as<uint32_t>() + n * PW, (uint32_t)n, ctx->io_b.as<uint32_t>());
        else
            hipLaunchKernelGGL(S::wide_prepare, dim3(div_up(n, dr::WMSM_BLOCK)), dim3(dr::WMSM_BLOCK), 0, st, ctx->io_a.as<uint32_t>(), (uint32_t)n,
                               ctx->io_b.as<uint32_t>());
    }));
    TRY(launch(ctx, S::wide_names[1], [&] {
        hipLaunchKernelGGL(S::wide_sort, dim3((unsigned)sets), dim3(dr::WMSM_SORT_BLOCK), 0, st, ctx->scalars.as<uint32_t>(), plan.wt, (uint32_t)n, H,
                           groups, (uint32_t)per_set, ctx->counts.as<uint32_t>(), ctx->offsets.as<uint32_t>(), ctx->sorted.as<uint32_t>());
    }));
    TRY(bucket_size_order(ctx, nbuckets));              // counts -> perm, longest lists first
    TRY(launch(ctx, S::wide_names[2], [&] {
        hipLaunchKernelGGL(S::wide_accumulate, dim3(div_up(nbuckets, dr::WMSM_BLOCK)), dim3(dr::WMSM_BLOCK), 0, st, ctx->io_b.as<uint32_t>(),
                           ctx->sorted.as<uint32_t>(), ctx->offsets.as<uint32_t>(), ctx->counts.as<uint32_t>(), ctx->perm.as<uint32_t>(),
                           ctx->buckets.as<uint32_t>(), nbuckets);
        hipLaunchKernelGGL(S::wide_accumulate_heavy, dim3((unsigned)nbuckets), dim3(64), 0, st, ctx->io_b.as<uint32_t>(), ctx->sorted.as<uint32_t>(),
                           ctx->offsets.as<uint32_t>(), ctx->counts.as<uint32_t>(), ctx->buckets.as<uint32_t>(), nbuckets);
    }));
    const auto reduce = [&] {
        hipLaunchKernelGGL(S::wide_reduce, dim3(div_up(sets * T, dr::WMSM_BLOCK)), dim3(dr::WMSM_BLOCK), 0, st, ctx->buckets.as<uint32_t>(), sets, H, L,
                           ctx->partial.as<uint32_t>());
    };
    const auto fold = [&] {
        hipLaunchKernelGGL(S::wide_fold, dim3(div_up(sets, dr::WMSM_BLOCK)), dim3(dr::WMSM_BLOCK), 0, st, ctx->partial.as<uint32_t>(), sets, T,
                           ctx->winsum.as<uint32_t>());
    };
    if (S::wide_names[4]) {                             // the fold under a name of its own
        TRY(launch(ctx, S::wide_names[3], reduce));
        TRY(launch(ctx, S::wide_names[4], fold));
    } else {
        TRY(launch(ctx, S::wide_names[3], [&] { reduce(); fold(); }));
    }
    std::vector<uint32_t> recs(sets * SUM);
    HIP_TRY(hipMemcpyAsync(recs.data(), ctx->winsum.p, sets * SUM * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (ctx->prof) TRY(prof_collect(ctx));
    std::vector<Point> sums(sets);
    for (size_t s = 0; s < sets; s++) {
        if constexpr (S::wide_affine) sums[s] = Law::from_abi(recs.data() + s * SUM);
        else sums[s] = dr::wide_record_point<Law>(recs.data() + s * SUM);
    }
    uint32_t w[PW];
    Law::to_abi(dr::wide_combine<Law>(sums.data(), plan.wt, groups), w);
    std::memcpy(out, w, S::pt_bytes);
    return DR_OK;
}

// S::wide_from: the first size of the bucket method (WIDE_PIP_FROM, or NARROW_PIP_FROM for E(Fq))
template <class S>
int wide_msm(dr_ctx* ctx, const uint8_t* pts, const uint8_t* scalars, size_t n, uint8_t* out) {
    using Law = typename S::Law;
    using Point = typename Law::Point;
    constexpr size_t PW = S::pt_bytes / 4;
    TRY(use_ctx(ctx));
    if (!out) return fail(DR_ERR_INVALID, "null buffer");
    auto put = [&](const Point& p) {
        uint32_t w[PW];
        Law::to_abi(p, w);
        std::memcpy(out, w, S::pt_bytes);
    };
    auto get = [](const uint8_t* p) {
        uint32_t w[PW];
        std::memcpy(w, p, S::pt_bytes);
        return Law::from_abi(w);
    };
    if (n == 0) {
        put(Law::identity());
        return DR_OK;
    }
    if (!pts || !scalars) return fail(DR_ERR_INVALID, "null buffer");
    if (n >= S::max_points) return fail(DR_ERR_INVALID, "batch too large");
    if (n >= S::wide_from) return wide_msm_buckets<S>(ctx, pts, scalars, n, out);

    // whole chunks of 64 in one launch, the rest in a second one; msm_groups checks coordinates and scalars
    const size_t full = n / 64, rest = n % 64;
    std::vector<uint8_t> part((full + 1) * S::pt_bytes);
    if (full) TRY(msm_groups<S>(ctx, pts, scalars, full, 64, part.data()));
    if (rest) TRY(msm_groups<S>(ctx, pts + full * 64 * S::pt_bytes, scalars + full * 64 * S::scalar_bytes, 1, rest, part.data() + full * S::pt_bytes));
    Point acc = Law::identity();
    for (size_t i = 0; i < full + (rest ? 1 : 0); i++) acc = Law::add(acc, get(part.data() + i * S::pt_bytes));
    put(acc);
    return DR_OK;
}

}  // namespace dri
