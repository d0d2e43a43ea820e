// libdotring_hip.so — C ABI, part 2 of 11: the G1 Pippenger pipeline over kernels_g1.hip.h, seam B (SRS handles, MSM entry
// points, G1 codecs) and the pairing entry points.
#include "capi_internal.hpp"
#include "kernels_g1.hip.h"
#include "kernels_g1_claims.hip.h"
#include "kernels_te_msm.hip.h"

using namespace dri;

// the planner's knobs: DOTRING_MSM_WINDOW read at context creation (g_force_c), DOTRING_MSM_GROUPS and DOTRING_SRS_TILING once per process
static MsmKnobs msm_knobs() {
    static const int force_groups = std::getenv("DOTRING_MSM_GROUPS") ? std::atoi(std::getenv("DOTRING_MSM_GROUPS")) : 0;
    static const bool naf_tiling = !(std::getenv("DOTRING_SRS_TILING") && std::strcmp(std::getenv("DOTRING_SRS_TILING"), "rows") == 0);
    return MsmKnobs{g_force_c, force_groups, naf_tiling};
}

namespace {
int msm_reserve(dr_ctx* ctx, const MsmPlan& p) {
    const auto& b = p.bytes;
    for (const auto& r : {std::make_pair(&ctx->counts, b.counts), {&ctx->offsets, b.offsets}, {&ctx->tiles, b.tiles}, {&ctx->perm, b.perm},
                          {&ctx->cells, b.cells}, {&ctx->cell_off, b.cell_off}, {&ctx->buckets, b.buckets}, {&ctx->partial, b.partial},
                          {&ctx->winsum, b.winsum}, {&ctx->heavy, b.heavy}, {&ctx->sorted, b.sorted}, {&ctx->digits, b.digits},
                          {&ctx->cursor, b.cursor}, {&ctx->part_base, b.part_base}, {&ctx->result, b.result}})
        TRY(r.first->reserve(r.second));
    return DR_OK;
}

void exclusive_scan(dr_ctx* ctx, const uint32_t* in, uint32_t* out, size_t count) {
    hipStream_t st = ctx->stream;
    const unsigned nt = div_up(count, dr::SCAN_TILE);
    hipLaunchKernelGGL(dr::k_scan_tiles, dim3(nt), dim3(dr::SCAN_BLOCK), 0, st, in, out, ctx->tiles.as<uint32_t>(), count);
    hipLaunchKernelGGL(dr::k_scan_tile_sums, dim3(1), dim3(dr::SCAN_BLOCK), 0, st, ctx->tiles.as<uint32_t>(), nt, ctx->tiles.as<uint32_t>() + nt);
    hipLaunchKernelGGL(dr::k_scan_add, dim3(div_up(count, 256)), dim3(256), 0, st, out, ctx->tiles.as<uint32_t>(), count);
}

// Sorting the digits by bucket (counts, offsets, sorted).  A partition sort whose first try overfills a stream (few distinct scalars)
// sets the flag part_flag points to; the call then runs again with exact = true (kernels_g1.hip.h: k_g1_part_scatter).
int msm_sort(dr_ctx* ctx, const MsmPlan& p, const uint32_t* d_scalars, const MsmTable* tbl, bool exact, const uint32_t*& part_flag) {
    hipStream_t st = ctx->stream;
    if (p.sort == MsmSort::sets || p.sort == MsmSort::sets_staged) {
        dr::SortSetParams sp{};
        sp.n = (uint32_t)p.n; sp.batch = (uint32_t)p.batch; sp.H = p.H; sp.groups = p.groups; sp.single = p.single ? 1 : 0;
        sp.tbl_stride = p.single ? tbl->stride : 0; sp.tbl_offset = p.single ? tbl->offset : 0; sp.capacity = (uint32_t)p.per_set_digits;
        sp.short_from = p.single ? tbl->short_from : 0xffffffffu; sp.n_short = p.single ? std::min<uint32_t>(tbl->n_short, (uint32_t)p.n) : 0;
        sp.sets = (uint32_t)p.bsets; sp.fold = p.single && tbl->fold_sign ? 1 : 0; sp.n_pad = p.n_pad; sp.digits_per_set = p.digits_per_set;
        sp.mult = p.multiples; sp.tbl_block = 256u * sp.tbl_stride;
        return launch(ctx, "k_g1_sort_sets", [&] {
            const auto staged = p.H <= dr::SORT2_SMALL_H ? dr::k_g1_sort_sets_staged<dr::SORT2_SMALL_H, dr::SORT2_CAP_SMALL_H>
                                                         : dr::k_g1_sort_sets_staged<dr::SORT_MAX_H, dr::SORT2_CAP_LARGE_H>;
            if (p.sort == MsmSort::sets_staged && p.multiples > 1)      // (the non-adjacent form has at most 2^11 buckets per set)
                hipLaunchKernelGGL((dr::k_g1_sort_sets_staged<dr::SORT2_SMALL_H, dr::SORT2_CAP_SMALL_H, uint32_t>), dim3((unsigned)p.bsets),
                                   dim3(dr::SORT2_BLOCK), 0, st, d_scalars, p.wt, sp, ctx->digits.as<uint32_t>(), ctx->counts.as<uint32_t>(),
                                   ctx->offsets.as<uint32_t>(), ctx->sorted.as<uint32_t>());
            else if (p.sort == MsmSort::sets_staged)
                hipLaunchKernelGGL(staged, dim3((unsigned)p.bsets), dim3(dr::SORT2_BLOCK), 0, st, d_scalars, p.wt, sp, ctx->digits.as<uint16_t>(),
                                   ctx->counts.as<uint32_t>(), ctx->offsets.as<uint32_t>(), ctx->sorted.as<uint32_t>());
            else
                hipLaunchKernelGGL(dr::k_g1_sort_sets, dim3((unsigned)p.bsets), dim3(dr::SORT_BLOCK), 0, st, d_scalars, p.wt, sp,
                                   ctx->counts.as<uint32_t>(), ctx->offsets.as<uint32_t>(), ctx->sorted.as<uint32_t>());
        });
    }
    if (p.sort == MsmSort::partition) {
        dr::PartParams pp{};
        pp.n = (uint32_t)p.n; pp.H = p.H; pp.groups = p.groups; pp.P = p.part_p; pp.pshift = p.part_shift; pp.tile = p.part_tile;
        pp.tiles_per_set = p.part_tiles_per_set; pp.cap_part = p.part_cap; pp.capacity = (uint32_t)p.per_set_digits;
        pp.tbl_stride = tbl->stride; pp.tbl_offset = tbl->offset;
        for (int w = 0; w < p.wt.W; w++) pp.row[w] = p.wt.row[w];
        const size_t nparts = p.nparts();
        uint32_t* d_flag = ctx->cursor.as<uint32_t>() + nparts;
        const uint32_t* d_exact = nullptr;
        bool fits = true;
        if (exact) {     // the first try's fill counters (still in place) are exact whether or not a record fitted: pack the streams
            std::vector<uint32_t> fill(nparts), at(nparts);
            HIP_TRY(hipMemcpyAsync(fill.data(), ctx->cursor.p, nparts * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            uint64_t run = 0, most = 0;
            for (size_t q = 0; q < nparts; q++) { at[q] = (uint32_t)run; run += fill[q]; most = std::max<uint64_t>(most, fill[q]); }
            fits = most <= dr::PART_MAX_CHUNKS * (dr::PART_STAGE - dr::PART_SLACK) && run <= nparts * (uint64_t)pp.cap_part;
            if (fits) {
                HIP_TRY(hipMemcpyAsync(ctx->part_base.p, at.data(), nparts * 4, hipMemcpyHostToDevice, st));
                HIP_TRY(hipStreamSynchronize(st));               // `at` leaves scope
                d_exact = ctx->part_base.as<uint32_t>();
            }
        }
        if (fits) {
            HIP_TRY(hipMemsetAsync(ctx->cursor.p, 0, (nparts + 1) * 4, st));
            TRY(launch(ctx, "k_g1_part_scatter", [&] {
                hipLaunchKernelGGL(dr::k_g1_part_scatter, dim3((unsigned)(p.bsets * pp.tiles_per_set)), dim3(dr::PART_BLOCK), 0, st, d_scalars, p.wt, pp,
                                   ctx->cursor.as<uint32_t>(), d_exact, ctx->digits.as<uint2>());
            }));
            if (!exact) part_flag = d_flag;
            return launch(ctx, "k_g1_part_sort", [&] {
                hipLaunchKernelGGL(dr::k_g1_part_sort, dim3((unsigned)nparts), dim3(dr::PART_BLOCK), 0, st, ctx->digits.as<uint2>(),
                                   ctx->cursor.as<uint32_t>(), d_exact, pp, d_flag, ctx->counts.as<uint32_t>(), ctx->offsets.as<uint32_t>(),
                                   ctx->sorted.as<uint32_t>());
            });
        }
    }
    // global atomics (also a partition sort whose exact streams did not fit either: the plan's room covers it)
    HIP_TRY(hipMemsetAsync(ctx->counts.p, 0, p.nbuckets * 4, st));
    HIP_TRY(hipMemsetAsync(ctx->cursor.p, 0, p.nbuckets * 4, st));
    TRY(launch(ctx, "k_g1_digits", [&] {
        hipLaunchKernelGGL(dr::k_g1_digits, dim3(div_up(p.n * p.batch, 256)), dim3(256), 0, st, d_scalars, (uint32_t)p.n,
                           (uint32_t)p.batch, p.wt, p.single ? 1 : 0, p.groups, ctx->digits.as<int32_t>(), ctx->counts.as<uint32_t>());
    }));
    TRY(launch(ctx, "k_scan", [&] { exclusive_scan(ctx, ctx->counts.as<uint32_t>(), ctx->offsets.as<uint32_t>(), p.nbuckets); }));
    return launch(ctx, "k_g1_scatter", [&] {
        hipLaunchKernelGGL(dr::k_g1_scatter, dim3(div_up(p.ndigits, 256)), dim3(256), 0, st, ctx->digits.as<int32_t>(),
                           (uint32_t)p.n, p.windows, p.H, p.single ? p.wt.W : 0, p.wt, p.single ? tbl->stride : 0u, p.single ? tbl->offset : 0u,
                           p.groups, ctx->offsets.as<uint32_t>(), ctx->cursor.as<uint32_t>(), ctx->sorted.as<uint32_t>());
    });
}

// the bucket walk, over a size-ordered bucket permutation
int msm_accumulate(dr_ctx* ctx, const MsmPlan& p, const uint32_t* d_bases, uint32_t pt_words) {
    hipStream_t st = ctx->stream;
    const unsigned szblocks = p.szblocks;
    const size_t nbuckets = p.nbuckets, ncells = p.ncells;
    TRY(launch(ctx, "k_size_sort", [&] {
        hipLaunchKernelGGL(dr::k_size_hist, dim3(szblocks), dim3(dr::SZ_BLOCK), 0, st, ctx->counts.as<uint32_t>(), nbuckets, szblocks,
                           ctx->cells.as<uint32_t>());
        exclusive_scan(ctx, ctx->cells.as<uint32_t>(), ctx->cell_off.as<uint32_t>(), ncells);
        hipLaunchKernelGGL(dr::k_size_place, dim3(szblocks), dim3(dr::SZ_BLOCK), 0, st, ctx->counts.as<uint32_t>(), nbuckets, szblocks,
                           ctx->cell_off.as<uint32_t>(), ctx->perm.as<uint32_t>());
        // the launch's limit between the one-lane walk and the 16-lane walk, from the histogram (two words behind the cell offsets)
        hipLaunchKernelGGL(dr::k_size_pick, dim3(1), dim3(256), 0, st, ctx->cell_off.as<uint32_t>(), szblocks, nbuckets, ctx->cell_off.as<uint32_t>() + ncells);
    }));
    const uint32_t* d_pick = ctx->cell_off.as<uint32_t>() + ncells;
    return launch(ctx, "k_g1_accumulate", [&] {
        hipLaunchKernelGGL(dr::k_g1_accumulate, dim3(div_up(nbuckets, 256)), dim3(256), 0, st, d_bases, pt_words,
                           ctx->sorted.as<uint32_t>(), ctx->offsets.as<uint32_t>(), ctx->counts.as<uint32_t>(), ctx->perm.as<uint32_t>(), d_pick,
                           ctx->buckets.as<uint32_t>(), nbuckets);
        // lists of 256 entries or more (the lowest odd-multiple buckets of every set; skewed scalars): 16 lanes or a wave each; both
        // launches return at once when there are none
        hipLaunchKernelGGL(dr::k_g1_accumulate_long<16>, dim3(2048), dim3(64), 0, st, d_bases, pt_words, ctx->sorted.as<uint32_t>(),
                           ctx->offsets.as<uint32_t>(), ctx->counts.as<uint32_t>(), ctx->perm.as<uint32_t>(), ctx->cell_off.as<uint32_t>(),
                           szblocks, d_pick, ctx->buckets.as<uint32_t>());
        // lists of 1024 entries or more (equal scalars, 0 / 1 columns): segments spread over 2048 waves, then one wave per bucket folds
        // its segment sums
        hipLaunchKernelGGL(dr::k_g1_accumulate_heavy, dim3(dr::G1_HEAVY_SLOTS), dim3(64), 0, st, d_bases, pt_words, ctx->sorted.as<uint32_t>(),
                           ctx->offsets.as<uint32_t>(), ctx->counts.as<uint32_t>(), ctx->perm.as<uint32_t>(), ctx->cell_off.as<uint32_t>(),
                           szblocks, ctx->buckets.as<uint32_t>(), ctx->heavy.as<uint32_t>());
        hipLaunchKernelGGL(dr::k_g1_heavy_fold, dim3(256), dim3(64), 0, st, ctx->counts.as<uint32_t>(), ctx->perm.as<uint32_t>(),
                           ctx->cell_off.as<uint32_t>(), szblocks, ctx->heavy.as<uint32_t>(), ctx->buckets.as<uint32_t>());
    });
}

// bucket sets -> set values in winsum, or (V, S) pairs per workgroup in partial (wg_scan)
int msm_reduce(dr_ctx* ctx, const MsmPlan& p) {
    hipStream_t st = ctx->stream;
    const size_t bsets = p.bsets;
    const uint32_t H = p.H, T = p.T;
    uint32_t* const partial = ctx->partial.as<uint32_t>();
    if (p.reduce == MsmReduce::set_scan || p.reduce == MsmReduce::levels) {
        // first level: chunks of 16 buckets to (sum B, sum i B); the set scan folds that level's T results per set, the level-wise
        // reduction repeats it down to 16 per set.  Level outputs live in partial: [S | C] per level, sizes sets * H/16, sets * H/256, ...
        const uint32_t *in_s = ctx->buckets.as<uint32_t>(), *in_c = nullptr;
        uint32_t n = H;
        int level = 0;
        for (size_t off = 0; n > 16 && (level == 0 || p.reduce == MsmReduce::levels); n /= 16) {
            level++;
            const size_t cnt = bsets * (n / 16);
            uint32_t *out_s = partial + off * 48, *out_c = partial + (off + cnt) * 48;
            TRY(launch(ctx, "k_g1_reduce_chunks", [&] {
                if (in_c)
                    hipLaunchKernelGGL(dr::k_g1_reduce_level, dim3(div_up(cnt, 128)), dim3(128), 0, st, in_s, in_c, bsets, n, 16u, level, out_s, out_c);
                else
                    hipLaunchKernelGGL(dr::k_g1_reduce_level1, dim3(div_up(cnt, 128)), dim3(128), 0, st, in_s, bsets, n, 16u, out_s, out_c);
            }));
            in_s = out_s, in_c = out_c, off += 2 * cnt;
        }
        return launch(ctx, "k_g1_reduce_windows", [&] {
            if (p.reduce == MsmReduce::set_scan)
                hipLaunchKernelGGL(dr::k_g1_reduce_set_scan, dim3(div_up(bsets, dr::RS_BLOCK / (T / dr::RS_GROUP))), dim3(dr::RS_BLOCK), 0, st,
                                   in_s, in_c, bsets, T, p.wt.odd, ctx->winsum.as<uint32_t>());
            else
                hipLaunchKernelGGL(dr::k_g1_reduce_final, dim3(div_up(bsets, 64)), dim3(64), 0, st, in_s, in_c, bsets, n, level, ctx->winsum.as<uint32_t>());
        });
    }
    if (p.reduce == MsmReduce::wg_scan) {
        // one huge bucket set per index group: workgroups of ws_span buckets scan and fold themselves; msm_finish combines their pairs
        return launch(ctx, "k_g1_reduce_chunks", [&] {
            const uint32_t* in = ctx->buckets.as<uint32_t>();
            const dim3 grid((unsigned)p.wg_count), block(dr::WS_BLOCK);
            if (p.ws_per_lane == 8) hipLaunchKernelGGL(dr::k_g1_reduce_wg_scan<8>, grid, block, 0, st, in, partial);
            else if (p.ws_per_lane == 4) hipLaunchKernelGGL(dr::k_g1_reduce_wg_scan<4>, grid, block, 0, st, in, partial);
            else if (p.ws_per_lane == 2) hipLaunchKernelGGL(dr::k_g1_reduce_wg_scan<2>, grid, block, 0, st, in, partial);
            else hipLaunchKernelGGL(dr::k_g1_reduce_wg_scan<1>, grid, block, 0, st, in, partial);
        });
    }
    TRY(launch(ctx, "k_g1_reduce_chunks", [&] {
        hipLaunchKernelGGL(dr::k_g1_reduce_chunks, dim3(div_up(bsets * T, 128)), dim3(128), 0, st, ctx->buckets.as<uint32_t>(), bsets, H, p.L, partial);
    }));
    return launch(ctx, "k_g1_reduce_windows", [&] {
        if (p.reduce == MsmReduce::chunks_two_stage) {
            // thousands of chunk results per set (one huge MSM): fold 256 at a time first — 2 + 7 additions deep, then T / 256 values
            // per set — instead of T / 128 + 7 in one workgroup per set
            uint32_t* mid = partial + bsets * T * 48;
            hipLaunchKernelGGL(dr::k_g1_reduce_windows, dim3((unsigned)(bsets * (T / 256))), dim3(dr::RW_BLOCK), 0, st, partial, 256u, mid);
            hipLaunchKernelGGL(dr::k_g1_reduce_windows, dim3((unsigned)bsets), dim3(dr::RW_BLOCK), 0, st, mid, T / 256, ctx->winsum.as<uint32_t>());
        } else {
            hipLaunchKernelGGL(dr::k_g1_reduce_windows, dim3((unsigned)bsets), dim3(dr::RW_BLOCK), 0, st, partial, T, ctx->winsum.as<uint32_t>());
        }
    });
}

// set value = sum_g (V_g + span g S_g) over the set's workgroups (span = buckets per workgroup) from the (V, S) pairs `vs` of the
// workgroup scan (device form).  Segments of 16 workgroups are folded side by side on the worker threads — (v, r, w) = (sum V_g,
// sum S_g, sum (g - g0) S_g) by a running sum —, then sum_g g S_g = sum_s w_s + 16 sum_s s r_s is a second running sum over the
// segments (one 2^19-bucket set: 16 segments of ~50 group operations, then ~40).
std::vector<drh::G1> fold_scan_pairs(const MsmPlan& p, std::vector<drh::G1>& vs) {
    constexpr size_t SEG = 16;
    const size_t wg_per_set = p.wg_per_set, segs_per_set = (wg_per_set + SEG - 1) / SEG, nseg = p.bsets * segs_per_set;
    std::vector<drh::G1> seg_v(nseg), seg_r(nseg), seg_w(nseg);
    const std::function<void(size_t)> one_seg = [&](size_t t) {
        const size_t set = t / segs_per_set, g0 = (t % segs_per_set) * SEG, g1 = std::min(wg_per_set, g0 + SEG);
        drh::G1* q = vs.data() + 2 * (set * wg_per_set + g0);
        g1_dev_to_host(q, 2 * (g1 - g0));
        drh::G1 run = drh::G1::inf(), w = drh::G1::inf(), v = drh::G1::inf();
        for (size_t g = g1 - g0; g-- > 0;) {
            v = drh::g1_add(v, q[2 * g]);
            run = drh::g1_add(run, q[2 * g + 1]);
            if (g >= 1) w = drh::g1_add(w, run);                                               // w = sum_g (g - g0) S_g
        }
        seg_v[t] = v; seg_r[t] = run; seg_w[t] = w;
    };
    // a task is ~50 group operations (~40 us): one per worker thread (parallel_for would keep so few items on one thread)
    if (drh::WorkerPool* pool = drh::worker_pool()) pool->run(nseg, (unsigned)std::min<size_t>(nseg, drh::host_threads()), one_seg);
    else for (size_t t = 0; t < nseg; t++) one_seg(t);
    std::vector<drh::G1> set_sum(p.bsets);
    const std::function<void(size_t)> one_set = [&](size_t set) {
        drh::G1 v = drh::G1::inf(), w = drh::G1::inf(), run = drh::G1::inf(), sr = drh::G1::inf();
        for (size_t sg = segs_per_set; sg-- > 0;) {
            const size_t t = set * segs_per_set + sg;
            v = drh::g1_add(v, seg_v[t]);
            w = drh::g1_add(w, seg_w[t]);
            if (sg >= 1) { run = drh::g1_add(run, seg_r[t]); sr = drh::g1_add(sr, run); }       // sr = sum_s s r_s
        }
        for (int k = 0; k < 4; k++) sr = drh::g1_dbl(sr);                                       // x 16
        w = drh::g1_add(w, sr);
        for (uint32_t k = 1; k < p.ws_span; k <<= 1) w = drh::g1_dbl(w);                        // x span
        set_sum[set] = drh::g1_add(v, w);
    };
    if (drh::WorkerPool* pool = p.bsets > 1 ? drh::worker_pool() : nullptr) pool->run(p.bsets, (unsigned)std::min<size_t>(p.bsets, drh::host_threads()), one_set);
    else for (size_t set = 0; set < p.bsets; set++) one_set(set);
    return set_sum;
}

// plain bases: Horner over the window sums (255 doublings: ~50x faster on one CPU core than on one GPU lane)
drh::G1 host_horner(const std::vector<drh::G1>& ws, const dr::WindowTable& wt) {
    drh::G1 acc = ws[wt.W - 1];
    for (int w = wt.W - 2; w >= 0; w--) {
        for (int j = 0; j < wt.width[w]; j++) acc = drh::g1_dbl(acc);
        acc = drh::g1_add(acc, ws[w]);
    }
    return acc;
}

// the batched contract: results in ctx->result (XYZZ) for the device-side affine pass of msm_batch_results_to_bytes
int upload_results(dr_ctx* ctx, const std::vector<drh::G1>& results) {
    std::vector<drh::G1> up(results);
    g1_host_to_dev(up.data(), up.size());
    HIP_TRY(hipMemcpyAsync(ctx->result.p, up.data(), up.size() * 192, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return DR_OK;
}

// set values -> MSM values; overflow: the partition sort overfilled a stream (part_flag), the results are void and the call runs again
int msm_finish(dr_ctx* ctx, const MsmPlan& p, const uint32_t* part_flag, std::vector<drh::G1>& results, PhaseTrace& tr, bool& overflow) {
    static_assert(sizeof(drh::G1) == 192, "XYZZ layout");
    hipStream_t st = ctx->stream;
    if (p.finish == MsmFinish::device_copy) {            // the bucket-set sums ARE the MSM values
        HIP_TRY(hipMemcpyAsync(ctx->result.p, ctx->winsum.p, p.batch * 192, hipMemcpyDeviceToDevice, st));
        return DR_OK;
    }
    if (p.finish == MsmFinish::device_horner)            // results stay in ctx->result; msm_batch_results_to_bytes() finishes them
        return launch(ctx, "k_g1_horner", [&] {
            hipLaunchKernelGGL(dr::k_g1_horner, dim3(div_up(p.batch, 64)), dim3(64), 0, st, ctx->winsum.as<uint32_t>(),
                               (uint32_t)p.batch, p.wt, ctx->result.as<uint32_t>());
        });
    const bool pairs = p.reduce == MsmReduce::wg_scan;
    std::vector<drh::G1> sets(pairs ? 2 * p.wg_count : p.bsets);
    uint32_t part_overflow = 0;
    HIP_TRY(hipMemcpyAsync(sets.data(), pairs ? ctx->partial.p : ctx->winsum.p, sets.size() * 192, hipMemcpyDeviceToHost, st));
    if (part_flag) HIP_TRY(hipMemcpyAsync(&part_overflow, part_flag, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (pairs) tr.mark("gpu");
    if ((overflow = part_overflow != 0)) return DR_OK;
    if (pairs) sets = fold_scan_pairs(p, sets);
    else g1_dev_to_host(sets.data(), sets.size());
    if (p.finish == MsmFinish::host_horner) results[0] = host_horner(sets, p.wt);
    else {                                               // table mode: an MSM is the sum of its index groups' sets (<= 64 additions)
        for (size_t b = 0; b < p.batch; b++) {
            drh::G1 acc = drh::G1::inf();
            for (uint32_t g = 0; g < p.groups; g++) acc = drh::g1_add(acc, sets[b * p.groups + g]);
            results[b] = acc;
        }
        if (p.batch > 1) TRY(upload_results(ctx, results));
    }
    if (pairs) tr.mark("host_fold");
    return DR_OK;
}
}  // namespace

int msm_device(dr_ctx* ctx, const uint32_t* d_bases, const uint32_t* d_scalars, size_t n, size_t batch,
               std::vector<drh::G1>& results, const MsmTable* tbl) {
    results.assign(batch, drh::G1::inf());
    if (n == 0 || batch == 0) return DR_OK;
    if (n >= (1ull << 31)) return fail(DR_ERR_INVALID, "MSM size must be below 2^31");
    PhaseTrace tr("msm_device");                 // DOTRING_TRACE=1: where the wall time of a call goes
    const MsmPlan p = plan_msm(n, batch, tbl, msm_knobs());
    if (p.error) return fail(DR_ERR_INVALID, p.error);
    TRY(msm_reserve(ctx, p));
    bool overflow = false;
    const auto run = [&](bool exact, PhaseTrace& t) {      // exact: the second run of a call whose partition sort overfilled a stream
        const uint32_t* part_flag = nullptr;
        TRY(msm_sort(ctx, p, d_scalars, tbl, exact, part_flag));
        t.mark("sort");
        TRY(msm_accumulate(ctx, p, p.single ? tbl->table : d_bases, p.single ? tbl->pt_words : 24u));
        TRY(msm_reduce(ctx, p));
        t.mark("enqueue");
        return msm_finish(ctx, p, part_flag, results, t, overflow);
    };
    TRY(run(false, tr));
    if (overflow) {                              // (its own trace line, printed before the call's)
        PhaseTrace tr2("msm_device");
        TRY(run(true, tr2));
    }
    if (ctx->prof) TRY(prof_collect(ctx));
    return DR_OK;
}

MsmTable srs_table(const dr_srs* srs, size_t offset) {
    MsmTable t;
    if (srs->d_table) {
        t.table = srs->d_table;
        t.wt = srs->table_wt;
        t.pt_words = srs->table_pt_words;
        t.bit_rows = srs->table_bit_rows;
        t.naf_delta = srs->table_naf_delta;
        t.multiples = srs->table_multiples;
        t.stride = (uint32_t)srs->count;
        t.offset = (uint32_t)offset;
    }
    return t;
}

// MSM(s) with results written as BE affine records
int msm_to_bytes(dr_ctx* ctx, const uint32_t* d_bases, const uint32_t* d_scalars, size_t n, size_t batch, uint8_t* out_be_xy, int* is_inf,
                 const MsmTable* tbl) {
    std::vector<drh::G1> res;
    TRY(msm_device(ctx, d_bases, d_scalars, n, batch, res, tbl));
    if (batch == 1 || n == 0) {
        for (size_t b = 0; b < batch; b++) g1_result_to_bytes(res[b], out_be_xy + 96 * b, is_inf ? is_inf + b : nullptr);
        return DR_OK;
    }
    return msm_batch_results_to_bytes(ctx, batch, out_be_xy, is_inf);
}

// batch > 1: results were left in ctx->result (XYZZ).  The affine conversion is one 381-bit field inversion per
// result: on the GPU a division-step chain (divstep28.hip.h: ≈ 0.08 ms of pure latency per call, whatever the batch; 0.5 ms with
// the binary Euclid, 0.85 ms with the Fermat power before that).  (Downloading XYZZ and inverting on the worker threads was measured for whole
// batches: less GPU time but more wall time per 1024 proofs.)
int msm_batch_results_to_bytes(dr_ctx* ctx, size_t batch, uint8_t* out_be_xy, int* is_inf) {
    // a handful of results (a single proof's 4 witness commitments, 2 openings): the kernel's one inversion chain is 0.6 ms of
    // latency whatever the count, the host inverts in ~15 us each
    if (batch <= 16) {
        static_assert(sizeof(drh::G1) == 192, "XYZZ layout");
        std::vector<drh::G1> res(batch);
        HIP_TRY(hipMemcpyAsync(res.data(), ctx->result.p, batch * 192, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        if (ctx->prof) TRY(prof_collect(ctx));
        g1_dev_to_host(res.data(), res.size());
        drh::parallel_for(batch, [&](size_t b) { g1_result_to_bytes(res[b], out_be_xy + 96 * b, is_inf ? is_inf + b : nullptr); }, 1);    // an inversion each
        return DR_OK;
    }
    TRY(ctx->io_c.reserve(batch * 96));
    TRY(launch(ctx, "k_g1_results_affine", [&] {
        hipLaunchKernelGGL(dr::k_g1_results_affine, dim3(div_up(batch, 64)), dim3(64), 0, ctx->stream, ctx->result.as<uint32_t>(),
                           (uint32_t)batch, ctx->io_c.as<uint32_t>());
    }));
    std::vector<uint8_t> le(batch * 96);
    HIP_TRY(hipMemcpyAsync(le.data(), ctx->io_c.p, batch * 96, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (ctx->prof) TRY(prof_collect(ctx));
    for (size_t b = 0; b < batch; b++) {
        bool allz = true;
        for (int j = 0; j < 96; j++) if (le[96 * b + j]) { allz = false; break; }
        if (is_inf) is_inf[b] = allz ? 1 : 0;
        for (int j = 0; j < 48; j++) {
            out_be_xy[96 * b + j] = le[96 * b + 47 - j];
            out_be_xy[96 * b + 48 + j] = le[96 * b + 95 - j];
        }
    }
    return DR_OK;
}

void g1_result_to_bytes(const drh::G1& r, uint8_t* out96, int* is_inf) {
    drh::Fq ax, ay;
    if (!drh::g1_to_affine(r, ax, ay)) {
        std::memset(out96, 0, 96);
        if (is_inf) *is_inf = 1;
        return;
    }
    ax.store_be(out96);
    ay.store_be(out96 + 48);
    if (is_inf) *is_inf = 0;
}

// BE x||y records -> LE standard-form limbs (device converts to Montgomery). Validates range; infinity -> zeros.
int g1_be_to_le_limbs(const uint8_t* be, size_t m, std::vector<uint8_t>& le, bool check_curve) {
    le.resize(m * 96);
    for (size_t i = 0; i < m; i++) {
        const uint8_t* rec = be + 96 * i;
        uint8_t* dst = le.data() + 96 * i;
        bool inf = (rec[0] & 0x40) != 0;
        if (!inf) {
            bool allz = true;
            for (int j = 0; j < 96; j++) if (rec[j]) { allz = false; break; }
            inf = allz;
        }
        if (inf) { std::memset(dst, 0, 96); continue; }
        if (rec[0] & 0xe0) return fail(DR_ERR_INVALID, "invalid BLS12-381 G1 encoding");
        for (int j = 0; j < 48; j++) { dst[j] = rec[47 - j]; dst[48 + j] = rec[95 - j]; }
        drh::Fq x, y;
        if (!drh::Fq::load_le(x, dst) || !drh::Fq::load_le(y, dst + 48))
            return fail(DR_ERR_INVALID, "invalid BLS12-381 G1 encoding");
        if (check_curve && !drh::g1_on_curve(x, y)) return fail(DR_ERR_INVALID, "invalid BLS12-381 G1 encoding");
    }
    return DR_OK;
}


// ------------------------------------------------------------------------------- K4: twisted Edwards Pippenger
// One variable-base MSM on Bandersnatch / JubJub by the bucket method (kernels_te_msm.hip.h).  Bucket sets are
// (window, index group) pairs so that a few thousand terms still make tens of thousands of bucket lanes; digits, counting
// sort and size ordering are the G1 pipeline's kernels.  The W x G set sums come back to the host for the final combination.
namespace {
struct TeHost {                 // extended coordinates over the host field (same Montgomery form as the device's Fr)
    drh::Fr x, y, z, t;
};
TeHost te_host_identity() { return {drh::Fr::zero(), drh::Fr::one(), drh::Fr::one(), drh::Fr::zero()}; }
TeHost te_host_add(const TeHost& p, const TeHost& q, const drh::Fr& d, const drh::Fr& neg_a) {      // add-2008-hwcd, unified
    drh::Fr A = p.x * q.x, B = p.y * q.y, C = p.t * d * q.t, D = p.z * q.z;
    drh::Fr E = (p.x + p.y) * (q.x + q.y) - A - B, F = D - C, G = D + C, H = B + A * neg_a;
    return {E * F, G * H, F * G, E * H};
}
}  // namespace

// ctx->counts -> ctx->perm on ctx->stream: the buckets by list length, longest first, so that the lanes of a wave of a bucket walk have
// lists of about one length
int bucket_size_order(dr_ctx* ctx, size_t nbuckets) {
    hipStream_t st = ctx->stream;
    const unsigned szblocks = div_up(nbuckets, dr::SZ_TILE);
    const size_t ncells = (size_t)dr::SZ_CLASSES * szblocks;
    TRY(ctx->tiles.reserve((size_t)(div_up(ncells, dr::SCAN_TILE) + 1) * 4));
    TRY(ctx->perm.reserve(nbuckets * 4));
    TRY(ctx->cells.reserve(ncells * 4));
    TRY(ctx->cell_off.reserve(ncells * 4));
    return launch(ctx, "k_size_sort", [&] {
        hipLaunchKernelGGL(dr::k_size_hist, dim3(szblocks), dim3(dr::SZ_BLOCK), 0, st, ctx->counts.as<uint32_t>(), nbuckets, szblocks,
                           ctx->cells.as<uint32_t>());
        const unsigned nt = div_up(ncells, dr::SCAN_TILE);
        hipLaunchKernelGGL(dr::k_scan_tiles, dim3(nt), dim3(dr::SCAN_BLOCK), 0, st, ctx->cells.as<uint32_t>(), ctx->cell_off.as<uint32_t>(),
                           ctx->tiles.as<uint32_t>(), ncells);
        hipLaunchKernelGGL(dr::k_scan_tile_sums, dim3(1), dim3(dr::SCAN_BLOCK), 0, st, ctx->tiles.as<uint32_t>(), nt, ctx->tiles.as<uint32_t>() + nt);
        hipLaunchKernelGGL(dr::k_scan_add, dim3(div_up(ncells, 256)), dim3(256), 0, st, ctx->cell_off.as<uint32_t>(), ctx->tiles.as<uint32_t>(), ncells);
        hipLaunchKernelGGL(dr::k_size_place, dim3(szblocks), dim3(dr::SZ_BLOCK), 0, st, ctx->counts.as<uint32_t>(), nbuckets, szblocks,
                           ctx->cell_off.as<uint32_t>(), ctx->perm.as<uint32_t>());
    });
}

int te_msm_pippenger(dr_ctx* ctx, int cv, const uint8_t* pts_xy, const uint8_t* scalars, size_t n, uint8_t out_xy[64]) {
    TRY(use_ctx(ctx));
    const drh::TeCurveHost* cu = drh::te_curve(cv);
    if (!cu) return fail(DR_ERR_INVALID, "unknown curve id");
    if (n == 0 || n >= (1ull << 26)) return fail(DR_ERR_INVALID, "bad MSM size");
    // scalars mod n (253 / 252 bits: the signed recoding over 256-bit windows never carries out of the top)
    std::vector<uint8_t> ks(n * 32);
    auto red = [&](size_t i) {
        uint64_t k[4];
        cu->n.reduce_bytes(scalars + 32 * i, 32, false, k);
        drh::store_le32(k, ks.data() + 32 * i);
    };
    if (n >= 4096) drh::parallel_for(n, red);
    else for (size_t i = 0; i < n; i++) red(i);
    // window width, tiling, index groups and capacities: the plan (msm_plan.hpp, checked on the host by tests/native/te_msm_plan_check.cpp)
    const dr::TeMsmPlan plan = dr::plan_te_msm(n, (int)cu->scalar_bits);
    const dr::WindowTable& wt = plan.wt;
    const uint32_t H = plan.H, L = plan.L, T = plan.T, groups = plan.groups;
    const size_t sets = plan.sets, nbuckets = plan.nbuckets, per_set = plan.per_set;
    hipStream_t st = ctx->stream;
    TRY(ctx->io_a.reserve(n * 64));
    TRY(ctx->io_b.reserve(n * 96));
    TRY(ctx->scalars.reserve(n * 32));
    TRY(ctx->counts.reserve(nbuckets * 4));
    TRY(ctx->offsets.reserve((nbuckets + 1) * 4));
    TRY(ctx->sorted.reserve(sets * per_set * 4));
    TRY(ctx->buckets.reserve(nbuckets * 128));
    TRY(ctx->partial.reserve(sets * T * 128));
    TRY(ctx->winsum.reserve(sets * 128));
    HIP_TRY(hipMemcpyAsync(ctx->io_a.p, pts_xy, n * 64, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ctx->scalars.p, ks.data(), n * 32, hipMemcpyHostToDevice, st));
    dr::SortSetParams sp{};
    sp.n = (uint32_t)n; sp.batch = 1; sp.H = H; sp.groups = groups; sp.single = 0;
    sp.capacity = (uint32_t)per_set; sp.short_from = 0xffffffffu; sp.n_short = 0;
    TRY(launch(ctx, "k_te_msm_prepare", [&] {
        LAUNCH_CV(cv, dr::k_te_msm_prepare, dim3(div_up(n, 256)), dim3(256), 0, st, ctx->io_a.as<uint32_t>(), (uint32_t)n, ctx->io_b.as<uint32_t>());
    }));
    TRY(launch(ctx, "k_g1_sort_sets", [&] {
        hipLaunchKernelGGL(dr::k_g1_sort_sets, dim3((unsigned)sets), dim3(dr::SORT_BLOCK), 0, st, ctx->scalars.as<uint32_t>(), wt, sp,
                           ctx->counts.as<uint32_t>(), ctx->offsets.as<uint32_t>(), ctx->sorted.as<uint32_t>());
    }));
    TRY(bucket_size_order(ctx, nbuckets));
    TRY(launch(ctx, "k_te_msm_accumulate", [&] {
        LAUNCH_CV(cv, dr::k_te_msm_accumulate, dim3(div_up(nbuckets, 256)), dim3(256), 0, st, ctx->io_b.as<uint32_t>(), ctx->sorted.as<uint32_t>(),
                  ctx->offsets.as<uint32_t>(), ctx->counts.as<uint32_t>(), ctx->perm.as<uint32_t>(), ctx->buckets.as<uint32_t>(), nbuckets);
        LAUNCH_CV(cv, dr::k_te_msm_accumulate_heavy, dim3((unsigned)nbuckets), dim3(64), 0, st, ctx->io_b.as<uint32_t>(), ctx->sorted.as<uint32_t>(),
                  ctx->offsets.as<uint32_t>(), ctx->counts.as<uint32_t>(), ctx->buckets.as<uint32_t>(), nbuckets);
    }));
    TRY(launch(ctx, "k_te_msm_reduce", [&] {
        LAUNCH_CV(cv, dr::k_te_msm_reduce, dim3(div_up(sets * T, 128)), dim3(128), 0, st, ctx->buckets.as<uint32_t>(), sets, H, L,
                  ctx->partial.as<uint32_t>());
        LAUNCH_CV(cv, dr::k_te_msm_fold, dim3(div_up(sets, 64)), dim3(64), 0, st, ctx->partial.as<uint32_t>(), sets, T, ctx->winsum.as<uint32_t>());
    }));
    static_assert(sizeof(TeHost) == 128, "extended point layout");
    std::vector<TeHost> sums(sets);
    HIP_TRY(hipMemcpyAsync(sums.data(), ctx->winsum.p, sets * 128, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (ctx->prof) TRY(prof_collect(ctx));
    // device layout is X, Y, Z, T; TeHost is x, y, z, t in that order
    uint8_t D_LE[32];
    drh::store_le32(cu->d, D_LE);
    drh::Fr d, neg_a = drh::Fr::from_u64(cu->neg_a[0]);
    if (!drh::Fr::load_le(d, D_LE)) return fail(DR_ERR_DEVICE, "bad curve constant");
    TeHost acc = te_host_identity();
    for (int w = wt.W - 1; w >= 0; w--) {
        if (w != wt.W - 1)
            for (int j = 0; j < wt.width[w]; j++) acc = te_host_add(acc, acc, d, neg_a);
        for (uint32_t g = 0; g < groups; g++) acc = te_host_add(acc, sums[(size_t)w * groups + g], d, neg_a);
    }
    drh::Fr zi = acc.z.inv();
    (acc.x * zi).store_le(out_xy);
    (acc.y * zi).store_le(out_xy + 32);
    return DR_OK;
}

// One MSM on a wide suite: each suite's unit has the implementation (capi_wide_msm.hpp over its kernels), this selects by id
int dr_wide_msm(dr_ctx* ctx, int curve, const uint8_t* pts, const uint8_t* scalars, size_t n, uint8_t* out) {
    switch (curve) {
        case DR_CURVE_P384_RO: case DR_CURVE_P384_NU: return p384_wide_msm(ctx, pts, scalars, n, out);
        case DR_CURVE_P521_RO: case DR_CURVE_P521_NU: return p521_wide_msm(ctx, pts, scalars, n, out);
        case DR_CURVE_ED448_RO: case DR_CURVE_ED448_NU: return ed448_wide_msm(ctx, pts, scalars, n, out);
        case DR_CURVE_CURVE448_RO: case DR_CURVE_CURVE448_NU: return curve448_wide_msm(ctx, pts, scalars, n, out);
        default: return fail(DR_ERR_INVALID, "dr_wide_msm serves the P-384, P-521, Ed448 and Curve448 suites");
    }
}

void g1_launch_decompress(hipStream_t st, const uint8_t* d_enc, uint32_t* d_bases, uint32_t* d_ok, size_t n) {
    hipLaunchKernelGGL(dr::k_g1_decompress, dim3(div_up(n, 64)), dim3(64), 0, st, d_enc, d_bases, d_ok, (uint32_t)n);
}
void g1_launch_bases_to_mont(hipStream_t st, uint32_t* d_bases, size_t n) {
    hipLaunchKernelGGL(dr::k_g1_bases_to_mont, dim3(div_up(n, 256)), dim3(256), 0, st, d_bases, (uint32_t)n);
}
void g1_launch_bases_from_mont(hipStream_t st, const uint32_t* d_bases, uint32_t* d_out, size_t n) {
    hipLaunchKernelGGL(dr::k_g1_bases_from_mont, dim3(div_up(n, 256)), dim3(256), 0, st, d_bases, d_out, (uint32_t)n);
}

// Claim points and their sum tree (kernels_g1_claims.hip.h) over bases already on the device: `terms` = groups * stride terms, term t is
// scalars[t] on base h_idx[t] (null: base t); leaf g of component c sums terms [g * stride + off[c], + m[c]).  out_le: comps trees of
// 2 * Bp - 1 nodes each (heap order), affine standard-form little-endian x || y, zeros for the identity.  Works in io_a (indices),
// scalars, io_b (terms), io_c (nodes) and result (affine nodes) on the context's stream; the caller has made the context current.
size_t g1_claim_tree_padded(size_t groups) {
    size_t bp = 1;
    while (bp < groups) bp <<= 1;
    return bp;
}
int g1_claim_tree(dr_ctx* ctx, const uint32_t* d_bases, const uint32_t* h_idx, const uint8_t* h_scalars, size_t groups, size_t stride, size_t comps,
                  const uint32_t off[2], const uint32_t m[2], uint8_t* out_le) {
    if (groups == 0 || groups > 4096 || stride == 0 || stride > 64 || comps < 1 || comps > 2) return fail(DR_ERR_INVALID, "claim tree: 1..4096 groups of 1..64 terms");
    for (size_t c = 0; c < comps; c++)
        if ((size_t)off[c] + m[c] > stride) return fail(DR_ERR_INVALID, "claim tree: component outside its group");
    const size_t n = groups * stride, bp = g1_claim_tree_padded(groups), nodes = comps * (2 * bp - 1);
    hipStream_t st = ctx->stream;
    TRY(ctx->scalars.reserve(n * 32));
    TRY(ctx->io_b.reserve(n * 192));
    TRY(ctx->io_c.reserve(nodes * 192));
    TRY(ctx->result.reserve(nodes * 96));
    HIP_TRY(hipMemcpyAsync(ctx->scalars.p, h_scalars, n * 32, hipMemcpyHostToDevice, st));
    if (h_idx) {
        TRY(ctx->io_a.reserve(n * 4));
        HIP_TRY(hipMemcpyAsync(ctx->io_a.p, h_idx, n * 4, hipMemcpyHostToDevice, st));
    }
    dr::ClaimTreeShape sh{};
    sh.groups = (uint32_t)groups; sh.padded = (uint32_t)bp; sh.stride = (uint32_t)stride; sh.comps = (uint32_t)comps;
    for (size_t c = 0; c < comps; c++) { sh.off[c] = off[c]; sh.m[c] = m[c]; }
    TRY(launch(ctx, "k_g1_claim_terms", [&] {
        hipLaunchKernelGGL(dr::k_g1_claim_terms, dim3(div_up(n, 64)), dim3(64), 0, st, d_bases, h_idx ? ctx->io_a.as<uint32_t>() : nullptr,
                           ctx->scalars.as<uint32_t>(), (uint32_t)n, ctx->io_b.as<uint32_t>());
    }));
    const unsigned wgs = (unsigned)std::max<size_t>(1, bp / dr::CLAIM_TREE_WG);
    TRY(launch(ctx, "k_g1_claim_tree", [&] {
        hipLaunchKernelGGL(dr::k_g1_claim_tree, dim3(wgs, (unsigned)comps), dim3(dr::CLAIM_TREE_WG), 0, st, ctx->io_b.as<uint32_t>(), sh,
                           ctx->io_c.as<uint32_t>(), 0);
    }));
    if (wgs > 1)
        TRY(launch(ctx, "k_g1_claim_tree", [&] {
            hipLaunchKernelGGL(dr::k_g1_claim_tree, dim3(1, (unsigned)comps), dim3(dr::CLAIM_TREE_WG), 0, st, ctx->io_b.as<uint32_t>(), sh,
                               ctx->io_c.as<uint32_t>(), 1);
        }));
    TRY(launch(ctx, "k_g1_results_affine", [&] {
        hipLaunchKernelGGL(dr::k_g1_results_affine, dim3(div_up(nodes, 64)), dim3(64), 0, st, ctx->io_c.as<uint32_t>(), (uint32_t)nodes,
                           ctx->result.as<uint32_t>());
    }));
    HIP_TRY(hipMemcpyAsync(out_le, ctx->result.p, nodes * 96, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (ctx->prof) TRY(prof_collect(ctx));
    return DR_OK;
}

int dr_g1_claim_tree_selftest(dr_ctx* ctx, const uint8_t* pts_le_xy, const uint8_t* scalars, size_t groups, size_t m, uint8_t* out_nodes_le_xy,
                              uint8_t* out_inf) {
    return abi_guard("claim tree selftest", [&]() -> int {
        TRY(use_ctx(ctx));
        if (!pts_le_xy || !scalars || !out_nodes_le_xy || !out_inf) return fail(DR_ERR_INVALID, "null buffer");
        if (groups == 0 || groups > 4096 || m == 0 || m > 64) return fail(DR_ERR_INVALID, "1..4096 groups of 1..64 terms");
        const size_t n = groups * m;
        for (size_t i = 0; i < 2 * n; i++) {                                // coordinates below p: the device brings them to Montgomery form
            drh::Fq v;
            if (!drh::Fq::load_le(v, pts_le_xy + 48 * i)) return fail(DR_ERR_INVALID, "coordinate out of range");
        }
        TRY(ctx->buckets.reserve(n * 96));
        HIP_TRY(hipMemcpyAsync(ctx->buckets.p, pts_le_xy, n * 96, hipMemcpyHostToDevice, ctx->stream));
        g1_launch_bases_to_mont(ctx->stream, ctx->buckets.as<uint32_t>(), n);
        HIP_TRY(hipGetLastError());
        const uint32_t off[2] = {0, 0}, mm[2] = {(uint32_t)m, 0};
        TRY(g1_claim_tree(ctx, ctx->buckets.as<uint32_t>(), nullptr, scalars, groups, m, 1, off, mm, out_nodes_le_xy));
        const size_t nodes = 2 * g1_claim_tree_padded(groups) - 1;
        for (size_t k = 0; k < nodes; k++) {
            bool inf = true;
            for (int q = 0; q < 96; q++) if (out_nodes_le_xy[96 * k + q]) { inf = false; break; }
            out_inf[k] = inf ? 1 : 0;
        }
        return DR_OK;
    });
}

// ------------------------------------------------------------------------------- seam B
int dr_srs_load(dr_ctx* ctx, const uint8_t* g1_be_xy, size_t m, dr_srs** out) {
    TRY(use_ctx(ctx));
    if (!out) return fail(DR_ERR_INVALID, "null out pointer");
    *out = nullptr;
    if (!g1_be_xy || m == 0) return fail(DR_ERR_INVALID, "empty SRS");
    if (m >= (1ull << 31)) return fail(DR_ERR_INVALID, "SRS too large");
    std::vector<uint8_t> le;
    TRY(g1_be_to_le_limbs(g1_be_xy, m, le, /*check_curve=*/m <= 65536));
    dr_srs* s = new (std::nothrow) dr_srs();
    if (!s) return fail(DR_ERR_NOMEM, "out of host memory");
    s->device = ctx->device;
    s->count = m;
    hipError_t e = hipMalloc((void**)&s->d_bases, m * 96);
    if (e != hipSuccess) {
        delete s;
        return fail(DR_ERR_NOMEM, "hipMalloc for the SRS failed");
    }
    e = hipMemcpyAsync(s->d_bases, le.data(), m * 96, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(dr::k_g1_bases_to_mont, dim3(div_up(m, 256)), dim3(256), 0, ctx->stream, s->d_bases, (uint32_t)m);
        e = hipStreamSynchronize(ctx->stream);
    }
    if (e != hipSuccess) {
        (void)hipFree(s->d_bases);
        delete s;
        return fail(DR_ERR_DEVICE, std::string("SRS upload: ") + hipGetErrorString(e));
    }
    *out = s;
    return DR_OK;
}

int dr_srs_synthetic(dr_ctx* ctx, const uint8_t seed_be_xy[96], uint32_t first, size_t count, dr_srs** out) {
    TRY(use_ctx(ctx));
    if (!out || !seed_be_xy) return fail(DR_ERR_INVALID, "null argument");
    *out = nullptr;
    if (count == 0 || count >= (1ull << 31) || (uint64_t)first + count >= (1ull << 32) || first == 0)
        return fail(DR_ERR_INVALID, "bad synthetic SRS range");
    std::vector<uint8_t> le;
    TRY(g1_be_to_le_limbs(seed_be_xy, 1, le, true));
    dr_srs* s = new (std::nothrow) dr_srs();
    if (!s) return fail(DR_ERR_NOMEM, "out of host memory");
    s->device = ctx->device;
    s->count = count;
    uint32_t* d_seed = nullptr;
    hipError_t e = hipMalloc((void**)&s->d_bases, count * 96);
    if (e == hipSuccess) e = hipMalloc((void**)&d_seed, 96);
    if (e == hipSuccess) e = hipMemcpyAsync(d_seed, le.data(), 96, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(dr::k_g1_bases_to_mont, dim3(1), dim3(64), 0, ctx->stream, d_seed, 1u);
        hipLaunchKernelGGL(dr::k_g1_synth_bases, dim3(div_up(count, 128)), dim3(128), 0, ctx->stream, s->d_bases, (uint32_t)count, first, d_seed);
        e = hipStreamSynchronize(ctx->stream);
    }
    if (d_seed) (void)hipFree(d_seed);
    if (e != hipSuccess) {
        if (s->d_bases) (void)hipFree(s->d_bases);
        delete s;
        return fail(e == hipErrorOutOfMemory ? DR_ERR_NOMEM : DR_ERR_DEVICE, std::string("synthetic SRS: ") + hipGetErrorString(e));
    }
    *out = s;
    return DR_OK;
}

int dr_srs_powers(dr_ctx* ctx, const uint8_t base_be_xy[96], const uint8_t tau_le[32], size_t count, dr_srs** out) {
    TRY(use_ctx(ctx));
    if (!out || !base_be_xy || !tau_le) return fail(DR_ERR_INVALID, "null argument");
    *out = nullptr;
    if (count == 0 || count >= (1ull << 28)) return fail(DR_ERR_INVALID, "bad SRS size");
    drh::Fr tau;
    if (!drh::Fr::load_le(tau, tau_le)) return fail(DR_ERR_INVALID, "tau is not a canonical scalar");
    std::vector<uint8_t> le;
    TRY(g1_be_to_le_limbs(base_be_xy, 1, le, true));
    std::vector<uint8_t> pw(count * 32);
    drh::Fr t = drh::Fr::one();
    for (size_t i = 0; i < count; i++) {
        t.store_le(pw.data() + 32 * i);
        t = t * tau;
    }
    dr_srs* s = new (std::nothrow) dr_srs();
    if (!s) return fail(DR_ERR_NOMEM, "out of host memory");
    s->device = ctx->device;
    s->count = count;
    uint32_t *d_seed = nullptr, *d_pw = nullptr;
    hipError_t e = hipMalloc((void**)&s->d_bases, count * 96);
    if (e == hipSuccess) e = hipMalloc((void**)&d_seed, 96);
    if (e == hipSuccess) e = hipMalloc((void**)&d_pw, count * 32);
    if (e == hipSuccess) e = hipMemcpyAsync(d_seed, le.data(), 96, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_pw, pw.data(), count * 32, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(dr::k_g1_bases_to_mont, dim3(1), dim3(64), 0, ctx->stream, d_seed, 1u);
        hipLaunchKernelGGL(dr::k_g1_scalar_bases, dim3(div_up(count, 64)), dim3(64), 0, ctx->stream, s->d_bases, (uint32_t)count, d_pw, d_seed);
        e = hipStreamSynchronize(ctx->stream);
    }
    if (d_seed) (void)hipFree(d_seed);
    if (d_pw) (void)hipFree(d_pw);
    if (e != hipSuccess) {
        if (s->d_bases) (void)hipFree(s->d_bases);
        delete s;
        return fail(e == hipErrorOutOfMemory ? DR_ERR_NOMEM : DR_ERR_DEVICE, std::string("SRS powers: ") + hipGetErrorString(e));
    }
    *out = s;
    return DR_OK;
}

int dr_g2_mul(const uint8_t g2_be[192], const uint8_t scalar_le[32], uint8_t out_be[192]) {
    if (!g2_be || !scalar_le || !out_be) return fail(DR_ERR_INVALID, "null buffer");
    drh::G2Affine Q;
    Q.inf = false;
    if (!drh::Fq::load_be(Q.x.c1, g2_be) || !drh::Fq::load_be(Q.x.c0, g2_be + 48) || !drh::Fq::load_be(Q.y.c1, g2_be + 96) ||
        !drh::Fq::load_be(Q.y.c0, g2_be + 144) || !drh::g2_on_curve(Q))
        return fail(DR_ERR_INVALID, "invalid BLS12-381 G2 encoding");
    drh::G2Affine R = drh::g2_mul(Q, scalar_le);
    std::memset(out_be, 0, 192);
    if (R.inf) { out_be[0] = 0x40; return DR_OK; }
    R.x.c1.store_be(out_be);
    R.x.c0.store_be(out_be + 48);
    R.y.c1.store_be(out_be + 96);
    R.y.c0.store_be(out_be + 144);
    return DR_OK;
}

int dr_srs_download(dr_ctx* ctx, const dr_srs* srs, size_t offset, size_t count, uint8_t* out_be_xy) {
    TRY(use_ctx(ctx));
    if (!srs || !out_be_xy) return fail(DR_ERR_INVALID, "null argument");
    if (offset > srs->count || count > srs->count - offset) return fail(DR_ERR_INVALID, "range exceeds SRS size");
    if (count == 0) return DR_OK;
    TRY(ctx->io_a.reserve(count * 96));
    hipLaunchKernelGGL(dr::k_g1_bases_from_mont, dim3(div_up(count, 256)), dim3(256), 0, ctx->stream,
                       srs->d_bases + offset * 24, ctx->io_a.as<uint32_t>(), (uint32_t)count);
    std::vector<uint8_t> le(count * 96);
    HIP_TRY(hipMemcpyAsync(le.data(), ctx->io_a.p, count * 96, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < count; i++)
        for (int j = 0; j < 48; j++) {
            out_be_xy[96 * i + j] = le[96 * i + 47 - j];
            out_be_xy[96 * i + 48 + j] = le[96 * i + 95 - j];
        }
    return DR_OK;
}

int dr_srs_precompute(dr_ctx* ctx, dr_srs* srs, int window_bits) { return srs_precompute(ctx, srs, window_bits, true); }

// ... and, where the table gets a row per bit, the rows of a few small odd multiples of every base beside them (k_g1_bit_table): batched
// MSMs then write a digit as +-(2 t + 1) b and need fewer of them (msm_recode.hip.h: for_each_wnaf_multiple_digit).  multiples = 0: the
// library's default count, 8; -1: the count it recommends for batched proving (SRS_BATCH_MULTIPLES); DOTRING_SRS_MULTIPLES (1, 2, 4, 8,
// 16 or 32) overrides any of them.
int dr_srs_precompute_multiples(dr_ctx* ctx, dr_srs* srs, int window_bits, int multiples) {
    if (multiples != 0 && multiples != -1 && !multiples_ok((uint32_t)multiples))
        return fail(DR_ERR_INVALID, "multiples must be 0 (default), -1 (recommended for batched proving), 1, 2, 4, 8, 16 or 32");
    if (multiples == 0) multiples = SRS_DEFAULT_MULTIPLES;
    if (multiples == -1) multiples = SRS_BATCH_MULTIPLES;
    const char* env = std::getenv("DOTRING_SRS_MULTIPLES");          // read per call: a process may build tables of several shapes
    if (env && multiples_ok((uint32_t)std::atoi(env))) multiples = std::atoi(env);
    return srs_precompute(ctx, srs, window_bits, true, multiples);
}

// bit_rows = false: window rows only (the prover's summation-by-parts bases: a few hundred scalars per vector, most of them +-1 — short,
// uneven lists that gain nothing from a window less and measured 0.7 ms per batch slower with odd-multiple buckets)
int srs_precompute(dr_ctx* ctx, dr_srs* srs, int window_bits, bool allow_bit_rows, int multiples) {
    TRY(use_ctx(ctx));
    if (!srs) return fail(DR_ERR_INVALID, "null argument");
    if (srs->device != ctx->device) return fail(DR_ERR_INVALID, "SRS lives on another device");
    if (window_bits == 0) {
        if (srs->d_table) (void)hipFree(srs->d_table);
        srs->d_table = nullptr;
        return DR_OK;
    }
    if (!dr::table_window_ok(window_bits)) return fail(DR_ERR_INVALID, "window_bits must be in 7..22 (0 drops the table)");
    dr::WindowTable wt = dr::make_window_table(window_bits);
    if ((uint64_t)wt.W * srs->count >= (1ull << 31)) return fail(DR_ERR_INVALID, "window table too large");
    if (srs->d_table) (void)hipFree(srs->d_table);
    srs->d_table = nullptr;
    srs->table_bit_rows = false;
    srs->table_multiples = 1;
    // A small SRS gets a row for every bit (32 KB per base: 201 MB for the 6145 points of a 2048-point domain) — the window rows are a
    // subset of it, and batched MSMs may then recode the scalars in non-adjacent form (tiling_for).
    // DOTRING_SRS_BIT_ROWS_MB (default 512, 0 = never) bounds the table; the width of that form is chosen per call (tiling_for).
    static const size_t bit_rows_mb = std::getenv("DOTRING_SRS_BIT_ROWS_MB") ? (size_t)std::atol(std::getenv("DOTRING_SRS_BIT_ROWS_MB")) : 512;
    // One table point per 128-byte line (24 of 32 words used): a packed 96-byte record straddles two lines five times out of eight, and
    // the bucket walk — one random table point per addition — measured 1.1 % faster with a third fewer lines to fetch although the table is
    // a third larger (A/B on one box, three alternations: 40.50 - 40.63 against 40.85 - 41.17 ms per 1024 proofs).
    const uint32_t pt_words = 32;
    bool bit_rows = allow_bit_rows && window_bits <= 16 && (size_t)256 * srs->count * 4 * pt_words <= (bit_rows_mb << 20);
    // Blocks of rows for the odd multiples 3 P_i, 5 P_i, ... behind the first: as many of the count asked for as fit DOTRING_SRS_MULTIPLES_MB
    // (default SRS_MULTIPLES_MB, the whole table), the 2^31 sorted entries and the device's memory — half as many, and half again down to
    // none, otherwise: never an error.
    const char* mult_env = std::getenv("DOTRING_SRS_MULTIPLES_MB");
    const size_t mult_mb = mult_env ? (size_t)std::atol(mult_env) : SRS_MULTIPLES_MB;
    uint32_t mult = bit_rows && multiples_ok((uint32_t)multiples) ? (uint32_t)multiples : 1u;
    for (; mult > 1; mult /= 2) {
        const size_t bytes = (size_t)mult * 256 * srs->count * 4 * pt_words;
        if (bytes > (mult_mb << 20) || (uint64_t)mult * 256 * srs->count >= (1ull << 31)) continue;
        if (hipMalloc((void**)&srs->d_table, bytes) == hipSuccess) break;
        (void)hipGetLastError();
        srs->d_table = nullptr;
    }
    if (bit_rows && mult == 1 && hipMalloc((void**)&srs->d_table, (size_t)256 * srs->count * 4 * pt_words) != hipSuccess) {
        (void)hipGetLastError();                   // a device short of memory keeps the window rows (W rows instead of 256)
        srs->d_table = nullptr;
        bit_rows = false;
    }
    if (!bit_rows) HIP_TRY(hipMalloc((void**)&srs->d_table, (size_t)wt.W * srs->count * 4 * pt_words));
    srs->table_pt_words = pt_words;
    if (bit_rows) {
        for (int w = 0; w < wt.W; w++) wt.row[w] = wt.start[w];
        hipLaunchKernelGGL(dr::k_g1_bit_table, dim3(div_up(srs->count * mult, 128)), dim3(128), 0, ctx->stream, srs->d_bases, (uint32_t)srs->count, 256u,
                           pt_words, mult, srs->d_table);
        srs->table_bit_rows = true;
        srs->table_multiples = mult;
    } else {
        hipLaunchKernelGGL(dr::k_g1_window_table, dim3(div_up(srs->count, 128)), dim3(128), 0, ctx->stream, srs->d_bases, (uint32_t)srs->count, wt,
                           pt_words, srs->d_table);
    }
    hipError_t e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        (void)hipFree(srs->d_table);
        srs->d_table = nullptr;
        srs->table_multiples = 1;
        return fail(DR_ERR_DEVICE, std::string("window table: ") + hipGetErrorString(e));
    }
    srs->table_wt = wt;
    return DR_OK;
}

void dr_srs_destroy(dr_srs* srs) {
    if (!srs) return;
    (void)hipSetDevice(srs->device);
    for (auto& it : srs->lagrange_prefix) dr_srs_destroy(it.second);
    srs->lagrange_prefix.clear();
    if (srs->d_table) (void)hipFree(srs->d_table);
    if (srs->d_bases) (void)hipFree(srs->d_bases);
    delete srs;
}

size_t dr_srs_size(const dr_srs* srs) { return srs ? srs->count : 0; }

int dr_srs_table_info(const dr_srs* srs, size_t n, size_t batch, int info[6]) {
    if (!srs || !info) return fail(DR_ERR_INVALID, "null argument");
    for (int i = 0; i < 6; i++) info[i] = 0;
    if (!srs->d_table) return DR_OK;
    const MsmTable t = srs_table(srs, 0);
    const Tiling tl = tiling_for(t, n, batch, msm_knobs().naf_tiling);
    info[0] = srs->table_wt.cmax;
    info[1] = srs->table_bit_rows ? 256 : srs->table_wt.W;
    info[2] = tl.naf ? tl.slots : srs->table_wt.W;
    info[3] = tl.c;
    info[4] = tl.naf ? 2 : 0;
    info[5] = (int)std::lround(1000.0 * (tl.naf ? tl.digits : (double)srs->table_wt.W));
    return DR_OK;
}

// dr_srs_table_info's six values, then info[6] = the multipliers a digit of this (n, batch) may take (1: none), info[7] = the blocks of
// rows the table holds
int dr_srs_table_info_multiples(const dr_srs* srs, size_t n, size_t batch, int info[8]) {
    if (!srs || !info) return fail(DR_ERR_INVALID, "null argument");
    TRY(dr_srs_table_info(srs, n, batch, info));
    info[6] = info[7] = 0;
    if (!srs->d_table) return DR_OK;
    const MsmTable t = srs_table(srs, 0);
    const MsmPlan p = plan_msm(n, batch, &t, msm_knobs());
    info[6] = p.error ? 1 : (int)p.multiples;
    info[7] = (int)srs->table_multiples;
    return DR_OK;
}

int dr_g1_msm_batch_dev(dr_ctx* ctx, const dr_srs* srs, const void* d_scalars, size_t n, size_t batch, uint8_t* out_be_xy, int* is_inf) {
    TRY(use_ctx(ctx));
    if (!srs || !out_be_xy) return fail(DR_ERR_INVALID, "null argument");
    if (srs->device != ctx->device) return fail(DR_ERR_INVALID, "SRS lives on another device");
    if (n > srs->count) return fail(DR_ERR_INVALID, "polynomial degree exceeds SRS size");
    MsmTable t = srs_table(srs, 0);
    return msm_to_bytes(ctx, srs->d_bases, (const uint32_t*)d_scalars, n, batch, out_be_xy, is_inf, &t);
}

int dr_g1_msm_batch(dr_ctx* ctx, const dr_srs* srs, const uint8_t* scalars, size_t n, size_t batch, uint8_t* out_be_xy, int* is_inf) {
    TRY(use_ctx(ctx));
    if (n && batch && !scalars) return fail(DR_ERR_INVALID, "null buffer");
    TRY(ctx->scalars.reserve(n * batch * 32));
    if (n && batch) HIP_TRY(hipMemcpyAsync(ctx->scalars.p, scalars, n * batch * 32, hipMemcpyHostToDevice, ctx->stream));
    return dr_g1_msm_batch_dev(ctx, srs, ctx->scalars.p, n, batch, out_be_xy, is_inf);
}

int dr_g1_msm_dev(dr_ctx* ctx, const dr_srs* srs, size_t offset, const void* d_scalars, size_t n, uint8_t out_be_xy[96], int* is_inf) {
    TRY(use_ctx(ctx));
    if (!srs || !out_be_xy) return fail(DR_ERR_INVALID, "null argument");
    if (srs->device != ctx->device) return fail(DR_ERR_INVALID, "SRS lives on another device");
    if (offset > srs->count || n > srs->count - offset) return fail(DR_ERR_INVALID, "polynomial degree exceeds SRS size");
    std::vector<drh::G1> res;
    MsmTable t = srs_table(srs, offset);
    TRY(msm_device(ctx, srs->d_bases + offset * 24, (const uint32_t*)d_scalars, n, 1, res, &t));
    g1_result_to_bytes(res[0], out_be_xy, is_inf);
    return DR_OK;
}

int dr_g1_msm(dr_ctx* ctx, const dr_srs* srs, size_t offset, const uint8_t* scalars, size_t n, uint8_t out_be_xy[96], int* is_inf) {
    TRY(use_ctx(ctx));
    if (n && !scalars) return fail(DR_ERR_INVALID, "null buffer");
    TRY(ctx->scalars.reserve(n * 32));
    if (n) HIP_TRY(hipMemcpyAsync(ctx->scalars.p, scalars, n * 32, hipMemcpyHostToDevice, ctx->stream));
    return dr_g1_msm_dev(ctx, srs, offset, ctx->scalars.p, n, out_be_xy, is_inf);
}

int dr_g1_msm_points(dr_ctx* ctx, const uint8_t* pts_be_xy, const uint8_t* scalars, size_t n, uint8_t out_be_xy[96], int* is_inf) {
    TRY(use_ctx(ctx));
    if (!out_be_xy) return fail(DR_ERR_INVALID, "null argument");
    if (n == 0) {
        std::memset(out_be_xy, 0, 96);
        if (is_inf) *is_inf = 1;
        return DR_OK;
    }
    if (!pts_be_xy || !scalars) return fail(DR_ERR_INVALID, "null buffer");
    std::vector<uint8_t> le;
    TRY(g1_be_to_le_limbs(pts_be_xy, n, le, true));
    TRY(ctx->io_a.reserve(n * 96));
    TRY(ctx->scalars.reserve(n * 32));
    HIP_TRY(hipMemcpyAsync(ctx->io_a.p, le.data(), n * 96, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(ctx->scalars.p, scalars, n * 32, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(dr::k_g1_bases_to_mont, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, ctx->io_a.as<uint32_t>(), (uint32_t)n);
    std::vector<drh::G1> res;
    TRY(msm_device(ctx, ctx->io_a.as<uint32_t>(), ctx->scalars.as<uint32_t>(), n, 1, res));
    g1_result_to_bytes(res[0], out_be_xy, is_inf);
    return DR_OK;
}

int dr_g1_sum(const uint8_t* pts_be_xy, size_t n, uint8_t out_be_xy[96], int* is_inf) {
    if (!out_be_xy || (n && !pts_be_xy)) return fail(DR_ERR_INVALID, "null buffer");
    std::vector<uint8_t> le;
    TRY(g1_be_to_le_limbs(pts_be_xy, n, le, true));
    drh::G1 acc = drh::G1::inf();
    for (size_t i = 0; i < n; i++) {
        drh::G1 p;
        bool allz = true;
        for (int j = 0; j < 96; j++) if (le[96 * i + j]) { allz = false; break; }
        if (allz) continue;
        drh::Fq::load_le(p.x, le.data() + 96 * i);
        drh::Fq::load_le(p.y, le.data() + 96 * i + 48);
        p.zz = drh::Fq::one();
        p.zzz = drh::Fq::one();
        acc = drh::g1_add(acc, p);
    }
    g1_result_to_bytes(acc, out_be_xy, is_inf);
    return DR_OK;
}

namespace {
// prepared G2 points by their 192-byte encoding (a verifier key has two; a handful of SRS files per process)
// (shared ownership: verifiers run their Miller loops concurrently — two per verify, several verifying threads — and an entry evicted by one
//  thread must outlive the loop of another that is still reading it)
std::shared_ptr<const drh::G2Prepared> g2_prepared_cached(const uint8_t enc[192], const drh::G2Affine& q) {
    static std::mutex m;
    static std::vector<std::pair<std::array<uint8_t, 192>, std::shared_ptr<const drh::G2Prepared>>> cache;
    std::array<uint8_t, 192> key;
    std::memcpy(key.data(), enc, 192);
    std::lock_guard<std::mutex> lock(m);
    for (auto& e : cache) if (e.first == key) return e.second;
    if (cache.size() >= 16) cache.erase(cache.begin());
    cache.emplace_back(key, std::make_shared<const drh::G2Prepared>(drh::g2_prepare(q)));
    return cache.back().second;
}
int miller_product(const uint8_t* g1_be_xy, const uint8_t* g2_be, size_t n, drh::Fq12& f, bool prepared = true) {
    std::vector<uint8_t> le;
    TRY(g1_be_to_le_limbs(g1_be_xy, n, le, true));
    std::vector<drh::Fq> px, py;
    std::vector<drh::G2Affine> qs;
    std::vector<const drh::G2Prepared*> preps;
    std::vector<std::shared_ptr<const drh::G2Prepared>> held;           // keeps the cached entries alive for the duration of the loop
    for (size_t i = 0; i < n; i++) {
        const uint8_t* q = g2_be + 192 * i;
        drh::G2Affine Q;
        bool allz = true;
        for (int j = 0; j < 192; j++) if (q[j]) { allz = false; break; }
        Q.inf = allz || (q[0] & 0x40);
        bool p_inf = true;
        for (int j = 0; j < 96; j++) if (le[96 * i + j]) { p_inf = false; break; }
        if (Q.inf || p_inf) continue;                       // e(O, Q) = e(P, O) = 1
        // zcash layout: x.c1 || x.c0 || y.c1 || y.c0, 48-byte big-endian each (pcs/srs.py:78-88)
        if (!drh::Fq::load_be(Q.x.c1, q) || !drh::Fq::load_be(Q.x.c0, q + 48) || !drh::Fq::load_be(Q.y.c1, q + 96) ||
            !drh::Fq::load_be(Q.y.c0, q + 144) || !drh::g2_on_curve(Q))
            return fail(DR_ERR_INVALID, "invalid BLS12-381 G2 encoding");
        drh::Fq x, y;
        drh::Fq::load_le(x, le.data() + 96 * i);
        drh::Fq::load_le(y, le.data() + 96 * i + 48);
        px.push_back(x); py.push_back(y); qs.push_back(Q);
        if (prepared) {
            held.push_back(g2_prepared_cached(q, Q));
            preps.push_back(held.back().get());
        }
    }
    f = prepared ? drh::multi_miller_loop_prepared(px.data(), py.data(), preps.data(), preps.size())
                 : drh::multi_miller_loop(px.data(), py.data(), qs.data(), qs.size());
    return DR_OK;
}
}  // namespace

int dri::pairing_miller(const uint8_t* g1_be_xy, const uint8_t* g2_be, size_t n, drh::Fq12& f) { return miller_product(g1_be_xy, g2_be, n, f); }
bool dri::pairing_product_is_one(const drh::Fq12& f) { return drh::final_exponentiation_check(f) == drh::Fq12::one(); }

int dr_pairing_check(const uint8_t* g1_be_xy, const uint8_t* g2_be, size_t n, int* ok) {
    if (!ok || (n && (!g1_be_xy || !g2_be))) return fail(DR_ERR_INVALID, "null buffer");
    drh::Fq12 f;
    TRY(miller_product(g1_be_xy, g2_be, n, f));
    *ok = drh::final_exponentiation_check(f) == drh::Fq12::one() ? 1 : 0;
    return DR_OK;
}

// diagnostic: the check's Miller loop (prepared G2 points, sparse line products) against the plain affine one, and its
// final exponentiation (Frobenius maps + x-chain with cyclotomic squarings, exponent 3(p^12-1)/r) against the plain
// square-and-multiply one; *consistent = 1 iff the loops agree and fast == reference^3 for this product
int dr_pairing_selfcheck(const uint8_t* g1_be_xy, const uint8_t* g2_be, size_t n, int* consistent) {
    if (!consistent || (n && (!g1_be_xy || !g2_be))) return fail(DR_ERR_INVALID, "null buffer");
    drh::Fq12 f, f_plain;
    TRY(miller_product(g1_be_xy, g2_be, n, f));
    TRY(miller_product(g1_be_xy, g2_be, n, f_plain, false));            // affine Miller loop, slopes computed on the fly
    drh::Fq12 ref = drh::final_exponentiation(f_plain);
    *consistent = (f == f_plain && drh::final_exponentiation_check(f) == ref * ref * ref) ? 1 : 0;
    return DR_OK;
}

int dr_g1_compress(const uint8_t xy[96], int is_inf, uint8_t out[48]) {
    if (!xy || !out) return fail(DR_ERR_INVALID, "null buffer");
    bool inf = is_inf != 0 || (xy[0] & 0x40);
    if (!inf) {
        bool allz = true;
        for (int j = 0; j < 96; j++) if (xy[j]) { allz = false; break; }
        inf = allz;
    }
    if (inf) {
        std::memset(out, 0, 48);
        out[0] = 0xc0;
        return DR_OK;
    }
    drh::Fq x, y;
    if (!drh::Fq::load_be(x, xy) || !drh::Fq::load_be(y, xy + 48)) return fail(DR_ERR_INVALID, "invalid BLS12-381 G1 encoding");
    std::memcpy(out, xy, 48);
    out[0] |= 0x80;
    drh::Fq ys = y.from_mont(), nys = y.neg().from_mont();
    if (drh::Fq::gt_std(ys, nys)) out[0] |= 0x20;
    return DR_OK;
}

int dr_g1_decompress(const uint8_t in[48], uint8_t out_xy[96], int* is_inf) {
    if (!in || !out_xy) return fail(DR_ERR_INVALID, "null buffer");
    uint8_t flags = in[0] >> 5;
    if (!(flags & 4)) return fail(DR_ERR_INVALID, "invalid BLS12-381 G1 encoding");
    uint8_t xb[48];
    std::memcpy(xb, in, 48);
    xb[0] &= 0x1f;
    if (flags & 2) {
        bool allz = true;
        for (int j = 0; j < 48; j++) if (xb[j]) { allz = false; break; }
        if (!allz || (flags & 1)) return fail(DR_ERR_INVALID, "invalid BLS12-381 G1 encoding");
        std::memset(out_xy, 0, 96);
        if (is_inf) *is_inf = 1;
        return DR_OK;
    }
    drh::Fq x;
    if (!drh::Fq::load_be(x, xb)) return fail(DR_ERR_INVALID, "invalid BLS12-381 G1 encoding");
    drh::Fq rhs = x.sqr() * x + drh::Fq::from_u64(4);
    // p = 3 mod 4: y = rhs^((p+1)/4)
    static const uint64_t E[6] = {0xee7fbfffffffeaabULL, 0x07aaffffac54ffffULL, 0xd9cc34a83dac3d89ULL,
                                  0xd91dd2e13ce144afULL, 0x92c6e9ed90d2eb35ULL, 0x0680447a8e5ff9a6ULL};
    drh::Fq y = rhs.pow(E, 6);
    if (y.sqr() != rhs) return fail(DR_ERR_INVALID, "invalid BLS12-381 G1 encoding");
    drh::Fq ny = y.neg();
    bool y_larger = drh::Fq::gt_std(y.from_mont(), ny.from_mont());
    if (y_larger != ((flags & 1) != 0)) y = ny;
    std::memcpy(out_xy, xb, 48);
    y.store_be(out_xy + 48);
    if (is_inf) *is_inf = 0;
    return DR_OK;
}

// KZG.decompress_g1 for n points in one launch (zcash 48-byte encodings -> BE x||y records; ok[i] = 0 for malformed
// encodings, infinity decodes to an all-zero record with ok = 1)
int dr_g1_decompress_batch(dr_ctx* ctx, const uint8_t* enc, size_t n, uint8_t* out_be_xy, uint8_t* ok) {
    TRY(use_ctx(ctx));
    if (n == 0) return DR_OK;
    if (!enc || !out_be_xy || !ok) return fail(DR_ERR_INVALID, "null buffer");
    if (n >= (1ull << 28)) return fail(DR_ERR_INVALID, "batch too large");
    TRY(ctx->vfy_in.reserve(n * 48));
    TRY(ctx->vfy_bases.reserve(n * 96));
    TRY(ctx->vfy_std.reserve(n * 96));
    TRY(ctx->io_c.reserve(n * 4));
    hipStream_t st = ctx->stream;
    HIP_TRY(hipMemcpyAsync(ctx->vfy_in.p, enc, n * 48, hipMemcpyHostToDevice, st));
    TRY(launch(ctx, "k_g1_decompress", [&] {
        hipLaunchKernelGGL(dr::k_g1_decompress, dim3(div_up(n, 64)), dim3(64), 0, st, ctx->vfy_in.as<uint8_t>(), ctx->vfy_bases.as<uint32_t>(),
                           ctx->io_c.as<uint32_t>(), (uint32_t)n);
        hipLaunchKernelGGL(dr::k_g1_bases_from_mont, dim3(div_up(n, 256)), dim3(256), 0, st, ctx->vfy_bases.as<uint32_t>(), ctx->vfy_std.as<uint32_t>(),
                           (uint32_t)n);
    }));
    std::vector<uint8_t> le(n * 96);
    std::vector<uint32_t> flags(n);
    HIP_TRY(hipMemcpyAsync(le.data(), ctx->vfy_std.p, n * 96, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(flags.data(), ctx->io_c.p, n * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (ctx->prof) TRY(prof_collect(ctx));
    for (size_t i = 0; i < n; i++) {
        ok[i] = flags[i] ? 1 : 0;
        for (int j = 0; j < 48; j++) {
            out_be_xy[96 * i + j] = le[96 * i + 47 - j];
            out_be_xy[96 * i + 48 + j] = le[96 * i + 95 - j];
        }
    }
    return DR_OK;
}

int dr_fq_ops_selftest(dr_ctx* ctx, const int32_t* in, size_t n, int32_t* out) {
    TRY(use_ctx(ctx));
    if (n == 0) return DR_OK;
    if (!in || !out) return fail(DR_ERR_INVALID, "null buffer");
    if (n >= (1ull << 24)) return fail(DR_ERR_INVALID, "batch too large");
    const size_t in_bytes = n * dr::FQ_SELFTEST_IN_WORDS * 4, out_bytes = n * dr::FQ_SELFTEST_OUT_WORDS * 4;
    TRY(ctx->io_a.reserve(in_bytes));
    TRY(ctx->io_b.reserve(out_bytes));
    HIP_TRY(hipMemcpyAsync(ctx->io_a.p, in, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(dr::k_fq_ops_selftest, dim3(div_up(n, 64)), dim3(64), 0, ctx->stream, ctx->io_a.as<int32_t>(), (uint32_t)n,
                       ctx->io_b.as<int32_t>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, ctx->io_b.p, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return DR_OK;
}

int dr_g1_ops_selftest(dr_ctx* ctx, const uint32_t* in, size_t n, uint32_t* out) {
    TRY(use_ctx(ctx));
    if (n == 0) return DR_OK;
    if (!in || !out) return fail(DR_ERR_INVALID, "null buffer");
    if (n >= (1ull << 20)) return fail(DR_ERR_INVALID, "batch too large");
    const size_t in_bytes = n * dr::G1_SELFTEST_IN_WORDS * 4, out_bytes = n * dr::G1_SELFTEST_OUT_WORDS * 4;
    TRY(ctx->io_a.reserve(in_bytes));
    TRY(ctx->io_b.reserve(out_bytes));
    HIP_TRY(hipMemcpyAsync(ctx->io_a.p, in, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(dr::k_g1_ops_selftest, dim3(div_up(n, 64)), dim3(64), 0, ctx->stream, ctx->io_a.as<uint32_t>(), (uint32_t)n,
                       ctx->io_b.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, ctx->io_b.p, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return DR_OK;
}

int dr_g1_serialize_check(const uint8_t xy[96]) {
    std::vector<uint8_t> le;
    return g1_be_to_le_limbs(xy, 1, le, true);
}
