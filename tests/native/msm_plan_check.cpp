// Host check of dot_ring_amd/csrc/msm_plan.hpp — the plan msm_device executes for a G1 MSM call.
// Invariants over a sweep of sizes, batches, table shapes and knobs: the non-adjacent form only with the LDS sort and the set scan, bucket
// and digit counts below 2^32, the workgroup scan's sets divisible by its span, the table row bound.  Then the sort, reduction and finish
// path of every shape the GPU tests and bench.py name, so that a threshold edit which moves one of them shows here.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "msm_plan.hpp"

static int failures = 0;
#define CHECK(cond, ...)                                                  \
    do {                                                                  \
        if (!(cond)) {                                                    \
            if (failures++ < 20) {                                        \
                std::fprintf(stderr, "FAIL %s: ", #cond);                 \
                std::fprintf(stderr, __VA_ARGS__);                        \
                std::fprintf(stderr, "\n");                               \
            }                                                             \
        }                                                                 \
    } while (0)

static const uint32_t g_dummy = 0;

// what dr_srs_precompute builds for `count` bases: a row per bit for a small SRS (<= 16-bit windows, <= 512 MB at 128 bytes a point),
// otherwise a row per window; the summation-by-parts bases always take window rows (allow_bit_rows = false)
static MsmTable table(int bits, size_t count, bool allow_bit_rows = true) {
    MsmTable t;
    t.table = &g_dummy;
    t.wt = dr::make_window_table(bits);
    t.pt_words = 32;
    t.bit_rows = allow_bit_rows && bits <= 16 && (size_t)256 * count * 128 <= ((size_t)512 << 20);
    if (t.bit_rows) for (int w = 0; w < t.wt.W; w++) t.wt.row[w] = t.wt.start[w];
    t.stride = (uint32_t)count;
    return t;
}

static void check_invariants(size_t n, size_t batch, const MsmTable* tbl, const MsmKnobs& k) {
    const MsmPlan p = plan_msm(n, batch, tbl, k);
    if (p.error) return;
    const bool lds = p.sort == MsmSort::sets || p.sort == MsmSort::sets_staged;
    CHECK(!p.wt.odd || (lds && p.reduce == MsmReduce::set_scan), "n=%zu batch=%zu", n, batch);
    CHECK(!p.wt.odd || (tbl && tbl->bit_rows), "n=%zu batch=%zu", n, batch);
    CHECK(p.nbuckets < (1ull << 32) && p.ndigits < (1ull << 32), "n=%zu batch=%zu", n, batch);
    CHECK(p.nbuckets == p.bsets * p.H && p.T * p.L == p.H, "n=%zu batch=%zu", n, batch);
    if (p.reduce == MsmReduce::wg_scan) CHECK(p.ws_span && p.H % p.ws_span == 0 && p.wg_count == p.bsets * (p.H / p.ws_span), "n=%zu batch=%zu", n, batch);
    if (p.reduce == MsmReduce::set_scan) CHECK(p.L == 16 && p.T >= 8 && p.T <= 256 && p.bsets >= 256, "n=%zu batch=%zu", n, batch);
    if (p.single) CHECK(((uint64_t)p.wt.row[p.wt.W - 1] + p.wt.cmax + 1) * tbl->stride < (1ull << 31), "n=%zu batch=%zu", n, batch);
    if (p.sort == MsmSort::partition) CHECK(p.single && batch == 1 && p.wt.W <= 32 && p.part_cap && p.H >> p.part_shift <= p.part_p, "n=%zu", n);
    if (p.finish == MsmFinish::device_copy || p.finish == MsmFinish::device_horner) CHECK(batch > 1 && p.bytes.result == batch * 192, "batch=%zu", batch);
    CHECK(p.single == (p.finish == MsmFinish::group_sum || p.finish == MsmFinish::device_copy), "n=%zu batch=%zu", n, batch);
    // one workgroup sorts a set in LDS: its bins and its digits are bounded; staged rows are whole lines of u16 digits
    if (lds) CHECK(p.H <= dr::SORT_MAX_H && p.per_set_digits <= (1u << 20) && p.bsets * p.per_set_digits < (1ull << 32), "n=%zu batch=%zu", n, batch);
    if (p.sort == MsmSort::sets_staged) CHECK(p.n_pad % 8 == 0 && p.n_pad >= p.per_set_scalars && p.bytes.digits >= p.bsets * p.per_set_digits * 2, "n=%zu", n);
    // a partition sort's second pass may fall back to the global-atomic sort: its room must hold that sort too
    if (p.sort == MsmSort::partition)
        CHECK(p.bytes.digits >= p.ndigits * 4 && p.bytes.sorted >= p.ndigits * 4 && p.bytes.cursor >= std::max(p.nbuckets, p.nparts() + 1) * 4 &&
              p.bytes.sorted >= p.bsets * p.per_set_digits * 4, "n=%zu", n);
}

static const char* sort_name(MsmSort s) {
    return s == MsmSort::sets ? "sets" : s == MsmSort::sets_staged ? "sets_staged" : s == MsmSort::partition ? "partition" : "global";
}
static const char* reduce_name(MsmReduce r) {
    return r == MsmReduce::set_scan ? "set_scan" : r == MsmReduce::levels ? "levels" : r == MsmReduce::wg_scan ? "wg_scan"
         : r == MsmReduce::chunks ? "chunks" : "chunks_two_stage";
}
static const char* finish_name(MsmFinish f) {
    return f == MsmFinish::group_sum ? "group_sum" : f == MsmFinish::device_copy ? "device_copy" : f == MsmFinish::host_horner ? "host_horner"
         : "device_horner";
}

// the pinned path of one named shape; naf = the width of the non-adjacent form (0: window rows)
static void pin(const char* what, size_t n, size_t batch, const MsmTable* tbl, MsmSort sort, MsmReduce reduce, MsmFinish finish, int naf,
                const MsmKnobs& k = MsmKnobs{}) {
    const MsmPlan p = plan_msm(n, batch, tbl, k);
    const int got_naf = p.wt.odd ? p.wt.cmax : 0;
    const bool ok = !p.error && p.sort == sort && p.reduce == reduce && p.finish == finish && got_naf == naf;
    if (!ok && failures++ < 20)
        std::fprintf(stderr, "FAIL %s (n = %zu, batch = %zu): %s / %s / %s, non-adjacent width %d%s\n", what, n, batch, sort_name(p.sort),
                     reduce_name(p.reduce), finish_name(p.finish), got_naf, p.error ? " (error)" : "");
}

int main() {
    using S = MsmSort;
    using R = MsmReduce;
    using F = MsmFinish;
    // ---- invariants
    const std::vector<size_t> ns = {1, 2, 24, 63, 64, 96, 300, 513, 1000, 2048, 3000, 6144, 6145, 7172, 12288, 20000, 32768, 50000, 65536,
                                    (1 << 18) + 37, 1 << 20, 1 << 21};
    const std::vector<size_t> batches = {1, 2, 5, 32, 33, 64, 255, 256, 300, 1024, 2048, 2100, 4096, 8192, 16500, 20000};
    const std::vector<MsmKnobs> knobs = {MsmKnobs{}, MsmKnobs{0, 0, false}, MsmKnobs{12, 0, true}, MsmKnobs{0, 16, true}};
    size_t shapes = 0;
    for (const MsmKnobs& k : knobs)
        for (size_t n : ns)
            for (size_t batch : batches) {
                if ((double)n * batch > 3e9) continue;
                check_invariants(n, batch, nullptr, k);
                shapes++;
                for (int bits = dr::MIN_WINDOW; bits <= dr::MAX_TABLE_WINDOW; bits++)
                    for (size_t count : {n, (size_t)6145, (size_t)1 << 20}) {
                        if (count < n) continue;
                        for (int naf_delta : {-2, -1, 0, 1}) {
                            MsmTable t = table(bits, count);
                            t.naf_delta = naf_delta;
                            check_invariants(n, batch, &t, k);
                            shapes++;
                        }
                    }
            }

    // ---- the batched prover (RingVRF, ring 1024: domain N = 2048, 1024 proofs) over the shipped 6145-point SRS, 12-bit bit-row table:
    // the quotient commitments (3N + 1 coefficients) and the two openings per proof (3N) in width-13 non-adjacent form
    const MsmTable srs12 = table(12, 6145);
    pin("prover quotient", 6145, 1024, &srs12, S::sets_staged, R::set_scan, F::device_copy, 13);
    pin("prover openings", 6144, 2048, &srs12, S::sets_staged, R::set_scan, F::device_copy, 13);
    // DOTRING_SRS_TILING=rows: the same calls on the table's 12-bit window rows
    const MsmKnobs rows{0, 0, false};
    pin("prover quotient, rows", 6145, 1024, &srs12, S::sets_staged, R::set_scan, F::device_copy, 0, rows);
    pin("prover openings, rows", 6144, 2048, &srs12, S::sets_staged, R::set_scan, F::device_copy, 0, rows);
    // the witness commitments by summation by parts: 4 columns per proof over the N derived bases, 10-bit window rows
    const MsmTable ps10 = table(10, 2048, false);
    pin("summation by parts", 2048, 4096, &ps10, S::sets_staged, R::set_scan, F::device_copy, 0);
    // one proof (RingVRF.prove): 4, 1 and 2 commitments
    for (size_t b : {1, 2, 4}) pin("one proof", 6145, b, &srs12, b < 4 ? S::sets : S::sets_staged, R::wg_scan, F::group_sum, 0);

    // ---- test_gpu_kernels.py
    // test_g1_msm_many_bucket_sets_level_reduction: 24 points, thousands of MSMs over a bit-row table take the non-adjacent form and the
    // set scan — on window rows as well; the level-wise reduction needs more than 256 chunks per set (14-bit window rows and wider)
    const MsmTable lv12 = table(12, 24), lv9 = table(9, 24), lv14 = table(14, 24);
    pin("many sets 12 / 2100", 24, 2100, &lv12, S::sets, R::set_scan, F::device_copy, 11);
    pin("many sets 9 / 16500", 24, 16500, &lv9, S::sets, R::set_scan, F::device_copy, 9);
    pin("many sets 12 / 2100, rows", 24, 2100, &lv12, S::sets, R::set_scan, F::device_copy, 0, rows);
    pin("many sets 9 / 16500, rows", 24, 16500, &lv9, S::sets, R::set_scan, F::device_copy, 0, rows);
    pin("level reduction 14 / 2100, rows", 24, 2100, &lv14, S::sets, R::levels, F::device_copy, 0, rows);
    // test_g1_msm_window_rows_take_the_level_reduction: 20000 synthetic bases (too many for bit rows), 14- and 15-bit window rows
    const MsmTable w14 = table(14, 20000), w15 = table(15, 20000);
    pin("level reduction 14 / 600", 64, 600, &w14, S::sets, R::levels, F::device_copy, 0);
    pin("level reduction 15 / 300", 64, 300, &w15, S::global, R::levels, F::device_copy, 0);
    // test_g1_msm_batch_matches_singles: 5 MSMs over plain bases, Horner on the device
    pin("plain batch", 512, 5, nullptr, S::sets, R::chunks, F::device_horner, 0);
    // test_g1_msm_a_few_over_a_table_take_the_workgroup_scan: up to 32 MSMs the workgroup scan, 33 the chunk kernels — except 9 .. 32
    // MSMs of 2048 points over 10-bit windows, whose 512 buckets per set are fewer than the scan's span (4 buckets per lane x 256).
    // The sort: global atomics below 64 bucket sets, the LDS sort from there on, staged from 4096 digits per set.
    const struct { int bits; size_t n, batch; MsmSort sort; MsmReduce reduce; } few[] = {
        {9, 513, 1, S::global, R::wg_scan},    {9, 513, 5, S::global, R::wg_scan},    {9, 513, 8, S::sets, R::wg_scan},
        {9, 513, 32, S::sets, R::wg_scan},     {9, 513, 33, S::sets, R::chunks},
        {10, 2048, 1, S::global, R::wg_scan},  {10, 2048, 2, S::sets, R::wg_scan},    {10, 2048, 8, S::sets, R::wg_scan},
        {10, 2048, 9, S::sets, R::chunks},     {10, 2048, 32, S::sets, R::chunks},    {10, 2048, 33, S::sets, R::chunks},
        {12, 6145, 1, S::sets, R::wg_scan},    {12, 6145, 3, S::sets, R::wg_scan},    {12, 6145, 5, S::sets_staged, R::wg_scan},
        {12, 6145, 32, S::sets_staged, R::wg_scan}, {12, 6145, 33, S::sets_staged, R::chunks}};
    for (const auto& f : few) {
        const MsmTable t = table(f.bits, f.n);
        pin("a few over a table", f.n, f.batch, &t, f.sort, f.reduce, F::group_sum, 0);
    }
    // test_g1_msm_one_plain_call_takes_the_workgroup_scan: plain bases, window by size, Horner on the host
    for (size_t n : {300, 1000, 3000, 7172, 20000, 50000}) pin("one plain call", n, 1, nullptr, S::global, R::wg_scan, F::host_horner, 0);
    // test_g1_msm_partition_sort_skewed_and_ragged: 2^18 + 37 synthetic bases, 16- and 18-bit window rows
    for (int bits : {16, 18}) {
        const MsmTable t = table(bits, (1 << 18) + 37);
        pin("partition sort", (1 << 18) + 37, 1, &t, S::partition, R::wg_scan, F::group_sum, 0);
    }
    // test_g1_msm_batched_odd_multiple_buckets: the widths the test asserts through dr_srs_table_info, and 64 vectors on window rows
    const struct { int bits; size_t n, batch; int width; } odd[] = {{9, 96, 8192, 10}, {12, 1500, 1024, 13}, {12, 5000, 300, 13}};
    for (const auto& o : odd) {
        const MsmTable t = table(o.bits, o.n);
        const Tiling tl = tiling_for(t, o.n, o.batch, true);
        CHECK(tl.naf && tl.c == o.width && tl.slots == (256 + o.width - 1) / o.width, "odd multiples %zu / %zu", o.n, o.batch);
        pin("odd multiples", o.n, o.batch, &t, o.n == 96 ? S::sets : S::sets_staged, R::set_scan, F::device_copy, o.width);
        CHECK(!tiling_for(t, o.n, 64, true).naf && !tiling_for(t, o.n, o.batch, false).naf, "odd multiples %zu", o.n);
    }

    // ---- bench.py: the single MSMs over 16- and 20-bit window rows (BASELINE configs[2]), the verifier's folds over plain bases
    const MsmTable b16 = table(16, 1 << 16), b20 = table(20, 1 << 20);
    pin("bench 2^16", 1 << 16, 1, &b16, S::partition, R::wg_scan, F::group_sum, 0);
    pin("bench 2^20", 1 << 20, 1, &b20, S::partition, R::wg_scan, F::group_sum, 0);
    for (size_t n : {2048, 7172}) pin("verifier fold", n, 1, nullptr, S::global, R::wg_scan, F::host_horner, 0);

    if (failures) {
        std::fprintf(stderr, "%d failures\n", failures);
        return 1;
    }
    std::printf("msm plan ok: %zu shapes\n", shapes);
    return 0;
}
