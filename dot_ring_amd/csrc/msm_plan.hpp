// The plan of a G1 Pippenger call (msm_device, capi_msm.hip) and the kernel-geometry constants it depends on (kernels_g1.hip.h uses
// them from here), and the plan of a twisted Edwards Pippenger call (te_msm_pippenger: plan_te_msm) and of the wide suites' bucket
// method (dr_wide_msm, and dr_te_msm / dr_blsg1_msm on the 256-bit suites and E(Fq): plan_wide_msm).  Plain host C++ (no HIP): g++ builds
// it for tests/native/msm_plan_check.cpp, tests/native/te_msm_plan_check.cpp, tests/native/wide_msm_plan_check.cpp and
// tests/native/narrow_msm_host_check.cpp.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "dev_types.hpp"
#include "wide_recode.hip.h"

namespace dr {

// ---- kernel geometry (kernels_g1.hip.h)
constexpr int SCAN_BLOCK = 256, SCAN_ITEMS = 8, SCAN_TILE = SCAN_BLOCK * SCAN_ITEMS;   // exclusive scan
constexpr uint32_t SORT_MAX_H = 8192;                                                 // k_g1_sort_sets: bins of a set in LDS
constexpr int SORT2_BLOCK = 1024;                                                     // k_g1_sort_sets_staged
constexpr uint32_t SORT2_SLACK = 2048, SORT2_MAX_CHUNKS = 64;
constexpr uint32_t SORT2_CAP_SMALL_H = 36864, SORT2_CAP_LARGE_H = 28672, SORT2_SMALL_H = 2048;
constexpr int PART_BLOCK = 1024;                                                      // k_g1_part_scatter / k_g1_part_sort
constexpr uint32_t PART_TILE_ENTRIES = 32768, PART_MAX_P = 1024, PART_MAX_HP = 1024, PART_STAGE = 36864, PART_SLACK = 2048, PART_MAX_CHUNKS = 64;
constexpr int SZ_BLOCK = 256, SZ_ITEMS = 8, SZ_TILE = SZ_BLOCK * SZ_ITEMS, SZ_CLASSES = 256;   // bucket size sort
constexpr uint32_t G1_HEAVY_SLOTS = 2048;                 // grid of k_g1_accumulate_heavy: two waves per SIMD
constexpr int RS_BLOCK = 64, RS_GROUP = 4;                // k_g1_reduce_set_scan
constexpr int WS_BLOCK = 256;                             // k_g1_reduce_wg_scan

// ---- window widths: DOTRING_MSM_WINDOW may force one within [7, 16] (the range pick_window searches); fixed-base tables take [7, 22]
// (one bucket set per MSM: wider windows stay cheap)
constexpr int MIN_WINDOW = 7, MAX_WINDOW = 16, MAX_TABLE_WINDOW = 22;
inline bool forced_window_ok(int c) { return c >= MIN_WINDOW && c <= MAX_WINDOW; }
inline bool table_window_ok(int c) { return c >= MIN_WINDOW && c <= MAX_TABLE_WINDOW; }

// Scalars are reduced mod r (< 2^255) on the device and the 256 bits are tiled by W = ceil(256/c) windows of width cmax or cmax-1
// (see WindowTable).  Work ~ W*n mixed adds + W*2^(c-1)*(2 full adds) + per-chunk scalar multiplications; a full add costs ~1.4 mixed
// adds; pick the c minimising that, within [MIN_WINDOW, MAX_WINDOW] (W <= 37 fits the table).
inline int pick_window(size_t n) {
    int best = MIN_WINDOW;
    double best_cost = 1e300;
    for (int c = MIN_WINDOW; c <= MAX_WINDOW; c++) {
        int W = (256 + c - 1) / c;
        double cost = (double)W * ((double)n + 2.8 * (double)(1u << (c - 1)) + 40.0 * (double)((1u << (c - 1)) / 16 + 1));
        if (cost < best_cost) { best_cost = cost; best = c; }
    }
    return best;
}

// One small MSM over plain bases (the verifier's two folds of ~7 k and ~2 k points, KZG commits of a few thousand coefficients) is a
// latency chain, not a throughput problem: the lanes of a launch are far fewer than the chip holds, so what counts is the longest
// dependent chain — the bucket walk's ~(m + 3 sqrt(m)) mixed additions for m points per bucket, then the 4-bucket chunks' running sums
// and (c - 3)-bit double-and-add, then the fold.  In units of one dependent addition (~11 us mixed, ~15 us full on a lone wave):
inline int pick_window_latency(size_t n) {
    int best = 7;
    double best_t = 1e300;
    for (int c = 7; c <= 13; c++) {
        const int W = (256 + c - 1) / c;
        const double H = (double)(1u << (c - 1));
        if ((double)W * H > 131072.0) continue;
        const double m = (double)n / H;
        // (from 256 buckets per window on the reduction is the workgroup scan: 2 x buckets per lane + 17 additions, plan_msm)
        const double reduce = H >= 256.0 ? 15.0 * (2.0 * std::min(8.0, std::max(1.0, H / 1024.0)) + 17.0)
                                         : 15.0 * (8.0 + 1.5 * (c - 3)) + 15.0 * (std::log2(std::max(H / 4.0, 2.0)) + 4.0);
        const double t = 11.0 * (m + 3.0 * std::sqrt(m) + 1.0) + reduce;
        if (t < best_t) { best_t = t; best = c; }
    }
    return best;
}

inline WindowTable make_window_table(int c, int bits = 256) {      // `bits` scalar bits tiled by ceil(bits / c) windows of near-equal width
    WindowTable wt;
    wt.W = (bits + c - 1) / c;
    int base = bits / wt.W, rem = bits % wt.W;                     // `rem` windows of width base+1 (placed on top), the rest base
    wt.cmax = base + (rem ? 1 : 0);
    int bit = 0;
    for (int w = 0; w < wt.W; w++) {
        int width = base + (w >= wt.W - rem ? 1 : 0);
        wt.start[w] = (uint8_t)bit, wt.width[w] = (uint8_t)width, wt.row[w] = (uint8_t)w;
        bit += width;
    }
    wt.odd = 0;
    return wt;
}

// ---- the twisted Edwards Pippenger (te_msm_pippenger, capi_msm.hip; kernels_te_msm.hip.h): ONE variable-base MSM of n terms
// A bucket list longer than this is not walked by one lane but by a whole wave (k_te_msm_accumulate_heavy): skewed scalars — many
// equal ones, or values much shorter than the windows cover — put thousands of points into one bucket, and a single lane
// adding them one after the other would be the whole kernel's run time.
constexpr uint32_t TE_HEAVY_BUCKET = 64;
constexpr uint32_t TE_REDUCE_CHUNK = 8;                    // buckets per lane of k_te_msm_reduce

struct TeMsmPlan {
    int c = 0;                           // window width asked for; wt.cmax is the widest one of the tiling
    WindowTable wt{};
    uint32_t H = 0, L = 0, T = 0, groups = 1;   // buckets per set, per reduction chunk, chunks per set, index groups
    size_t sets = 0, nbuckets = 0, per_set = 0; // (window, group) bucket sets, all buckets, entries reserved per set in `sorted`
};

// scalar_bits: bits of the group order (253 on Bandersnatch, 252 on JubJub); scalars arrive reduced below it
inline TeMsmPlan plan_te_msm(size_t n, int scalar_bits) {
    TeMsmPlan p;
    // window width by size (the reference's rule grows the same way, bandersnatch.py:23-36)
    p.c = n < 4096 ? 7 : n < 16384 ? 8 : n < 65536 ? 9 : 10;
    // tile scalar_bits + 1 bits, not 256: a top window holding one or two live bits would put half of all points into one bucket
    p.wt = make_window_table(p.c, scalar_bits + 1);
    p.H = 1u << (p.wt.cmax - 1), p.L = TE_REDUCE_CHUNK, p.T = p.H / p.L;
    // index groups until a bucket holds ~8 points or 64 groups
    while (p.groups < 64 && n / ((size_t)p.groups * 2 * p.H) >= 8) p.groups *= 2;
    p.sets = (size_t)p.wt.W * p.groups, p.nbuckets = p.sets * p.H;
    p.per_set = (n + p.groups - 1) / p.groups;
    return p;
}

// ---- the bucket method of the wide suites (dr_wide_msm; wave_msm.hip.h, capi_wide_msm.hpp): ONE variable-base MSM of n terms on
// P-384, Ed448, Curve448 or P-521.  From WIDE_PIP_FROM terms on; below it the call launches msm_groups in chunks of up to 64.
constexpr size_t WIDE_PIP_FROM = 256;
constexpr uint32_t WIDE_MAX_H = 512;                       // wave_msm_sort: bins of a set in LDS (window widths up to 10)
// The same method under dr_te_msm for Ed25519, Baby JubJub, P-256, secp256k1 and Curve25519 and under dr_blsg1_msm for BLS12-381's
// E(Fq), from this many terms on.  At least 257: a dr_te_msm of 256 terms is recorded as two msm_groups launches
// (tests/golden/entry_surface_gpu.json).  The value is the smallest measured size at which the buckets beat msm_groups on all six
// curves.
constexpr size_t NARROW_PIP_FROM = 257;
// ... and under dr_blsg2_msm for BLS12-381's E(Fq2): the project's value for E(Fq); nothing else depends on it
constexpr size_t BLSG2_PIP_FROM = NARROW_PIP_FROM;

struct WideMsmPlan {
    int c = 0;                           // window width asked for; wide_cmax(wt) is the widest one of the tiling
    WideTiling wt{};
    uint32_t H = 0, L = 0, T = 0, groups = 1;   // buckets per set, per reduction chunk, chunks per set, index groups
    size_t sets = 0, nbuckets = 0, per_set = 0; // (window, group) bucket sets, all buckets, entries reserved per set in `sorted`
};

// bits: what the tiling covers, one more than the scalars can have (wide_recode.hip.h): 385 on P-384, 449 on Ed448 and Curve448, 522 on
// P-521; 254 on Ed25519 and Curve25519 and 252 on Baby JubJub (scalars reduced below the order), 257 on P-256, secp256k1 and E(Fq).  Width by size, index groups and chunks are plan_te_msm's rules: the walk and the reduction have the same shape
inline WideMsmPlan plan_wide_msm(size_t n, int bits) {
    WideMsmPlan p;
    p.c = n < 4096 ? 7 : n < 16384 ? 8 : n < 65536 ? 9 : 10;
    p.wt = make_wide_tiling(p.c, bits);
    p.H = 1u << (wide_cmax(p.wt) - 1), p.L = TE_REDUCE_CHUNK, p.T = p.H / p.L;
    while (p.groups < 64 && n / ((size_t)p.groups * 2 * p.H) >= 8) p.groups *= 2;
    p.sets = (size_t)p.wt.W * p.groups, p.nbuckets = p.sets * p.H;
    p.per_set = (n + p.groups - 1) / p.groups;
    return p;
}

}  // namespace dr

// Fixed-base table descriptor for msm_device (table == nullptr: plain bases, one bucket set per window).
struct MsmTable {
    const uint32_t* table = nullptr;
    dr::WindowTable wt{};
    uint32_t pt_words = 24;              // words per table record
    bool bit_rows = false;               // the table has a row per bit: a call may recode the scalars as it likes (non-adjacent form)
    int naf_delta = -2;                  // see dr_srs::table_naf_delta
    uint32_t multiples = 1;              // bit rows only: blocks of 256 rows, block t = the rows of (2 t + 1) * base (1, 2, 4, 8, 16 or 32)
    uint32_t stride = 0, offset = 0;
    uint32_t short_from = 0xffffffffu, n_short = 0;   // batched MSM: vectors from this index on are zero beyond n_short (sort hint)
    bool fold_sign = false;              // scalars above r / 2 enter as their negatives (difference columns: r - 1 becomes -1, one digit)
};

// the planner's environment knobs, read by the C API: DOTRING_MSM_WINDOW (force_c: the window of plain-base MSMs; 0 or out of range:
// by size), DOTRING_MSM_GROUPS (index groups of one table MSM; 0: by size), DOTRING_SRS_TILING=rows (naf_tiling = false: window rows)
struct MsmKnobs { int force_c = 0, force_groups = 0; bool naf_tiling = true; };

// fewer first-level chunks than this over all sets of a table MSM: chunks of 4 buckets instead of 16 (shorter dependent chains for
// launches that do not fill the chip)
// (2^15 since the end of round 4 — 256 sets of 2048 buckets: same-box sweeps of prove_batch at 256 / 384 / 512 proofs gave 20.7 / 28.4 / 32.9 ms with
//  2^17, 20.2 / 27.1 / 31.8 with 2^16, 19.6 / 26.6 / 31.6 with 2^15; 1024 proofs the same)
constexpr size_t L4_BELOW = (size_t)1 << 15;

// the tiling msm_device takes for `batch` MSMs of n points over this table: naf = width-c non-adjacent form (bit-row tables, hundreds of
// MSMs), otherwise the table's window rows; slots = digit rows per scalar, digits = expected non-zero digits per scalar
struct Tiling { bool naf; int c, slots; double digits; uint32_t multiples = 1; };

// Expected non-zero digits per uniformly random scalar of the non-adjacent form over a table with M = 2, 4, 8, 16, 32 odd multiples
// (msm_recode.hip.h: for_each_wnaf_multiple_digit), widths 9 .. 13: measured over 20 000 scalars by tests/native/recode_multiples_check.cpp
// (2, 4, 8) and tests/native/recode_multiples_wide_check.cpp (16, 32), which print this table
constexpr double NAF_MULTIPLE_DIGITS[5][5] = {{24.65, 23.20, 21.83, 20.54, 19.44}, {22.59, 21.40, 20.21, 19.07, 18.12}, {20.85, 19.83, 18.84, 17.87, 17.00},
                                              {19.36, 18.50, 17.64, 16.82, 16.02}, {18.06, 17.32, 16.60, 15.87, 15.15}};
inline bool multiples_ok(uint32_t m) { return m == 1 || m == 2 || m == 4 || m == 8 || m == 16 || m == 32; }
// the count dr_srs_precompute_multiples(.., 0) asks for
constexpr int SRS_DEFAULT_MULTIPLES = 8;
// the count dr_srs_precompute_multiples(.., -1) asks for, what the batched prover takes (the walk gathers
// from 6.4 GB at 98 % of its rate over 1.6 GB and has 8.8 % fewer entries; the sort pays 0.6 ms of the 2.7 ms won; 16 gained less)
constexpr int SRS_BATCH_MULTIPLES = 32;
// default of DOTRING_SRS_MULTIPLES_MB: the 6145-point table of a 2048-point domain at 32 blocks is 6145 MiB; the 12289 points of a
// 4096-point domain get 16 blocks under it (6145 MiB again; 32 would be 12289 MiB: raise the knob to take them)
constexpr size_t SRS_MULTIPLES_MB = 8192;

// A table with a row per bit and hundreds of MSMs (the batched prover): a digit may sit at ANY bit position, so every scalar is recoded
// in width-w non-adjacent form (msm_recode.hip.h: for_each_wnaf_digit): 256 / (w + 1) + ~0.55 odd digits on average — 18.8 for w = 13
// where 13-bit windows have 20 — into 2^(w-2) odd-multiple buckets per set (value of a set: sum_j (2j + 1) B_j).  Round 3 reached the
// same bucket count with 13-bit windows whose digits 2^k u went to bucket (u - 1) / 2 with the point of row start + k, which put every
// power of two of a window into bucket 0 and needed twin buckets and a merge kernel; the non-adjacent form has odd digits only and
// shares the bits at the top evenly, so the fullest bucket holds ~4x the average list and stays in the one-lane walk.
// Needs the per-set LDS sort and the set-scan reduction (hundreds of sets; with fewer the L = 4 latency reduction applies — plan_msm
// falls back to the window rows otherwise); w <= 13: the staged sort's u16 digit rows hold 11 bucket bits + 4 offset bits + sign.
// Among the widths that qualify the cheapest wins: n x digits bucket additions + ~1.5 addition-equivalents per bucket of the reduction
// (measured: level 1 + set scan per bucket against the walk's time per entry): w = 13 for the 3N = 6144-point vectors of domain 2048
// and the 12288 of domain 4096.
inline Tiling tiling_for(const MsmTable& t, size_t n, size_t batch, bool naf_tiling) {
    Tiling none{false, 0, 0, 0.0, 1};
    const uint32_t M = multiples_ok(t.multiples) ? t.multiples : 1;
    if (!t.table || !t.bit_rows || t.naf_delta == -1 || batch < 256 || n == 0 || !naf_tiling) return none;
    const int cn = t.wt.cmax;
    const int lo = t.naf_delta >= 0 ? cn + t.naf_delta : cn - 1, hi = t.naf_delta >= 0 ? cn + t.naf_delta : cn + 2;
    Tiling best = none;
    double best_cost = 0;
    for (int w = lo; w <= hi; w++) {
        if (w < 9 || w > 13) continue;
        const size_t H = (size_t)1 << (w - 2), slots = (256 + w - 1) / w;
        if (batch * (H / 16) < L4_BELOW) continue;
        if ((n + 64) * slots > ((size_t)1 << 20) || batch * (n + 64) * slots >= (1ull << 32)) continue;
        // (+ the evenly shared digits at the top and the end effects: 18.8 measured at w = 13)
        const double digits = M == 1 ? 256.0 / (w + 1) + 0.55 : NAF_MULTIPLE_DIGITS[w - 9][M == 2 ? 0 : M == 4 ? 1 : M == 8 ? 2 : M == 16 ? 3 : 4];
        if (t.naf_delta < 0 && (double)n * digits / (double)H > 160.0) continue;      // the fullest lists (~4x) stay near the one-lane limit
        // (1.5 addition-equivalents per bucket: with the widths 12 and 13 both admitted at ring 256 — 3N = 3072 terms, 1024 proofs — the
        //  narrower one saved 0.15 ms of reduction per step and cost 1.15 ms of walk; the 5.2 of the first fit priced the reduction at its
        //  issue rate, which launches of this size do not reach)
        const double cost = (double)n * digits + 1.5 * (double)H;
        if (!best.naf || cost < best_cost) { best = Tiling{true, w, (int)slots, digits, M}; best_cost = cost; }
    }
    return best;
}

// How the digits are sorted by bucket, how each bucket set is reduced to its value, and what becomes of the set values: summed per MSM
// on the host (group_sum: table mode, uploaded to ctx->result when batch > 1), the results themselves (device_copy), Horner over windows
enum class MsmSort { sets, sets_staged, partition, global };
enum class MsmReduce { set_scan, levels, wg_scan, chunks, chunks_two_stage };
enum class MsmFinish { group_sum, device_copy, host_horner, device_horner };

struct MsmPlan {
    const char* error = nullptr;         // set: the call cannot run (DR_ERR_INVALID)
    size_t n = 0, batch = 0;             // points per MSM, MSMs
    bool single = false;                 // over a fixed-base table: a bucket set per (MSM, index group) spans all windows
    dr::WindowTable wt{};                // the digit rows; wt.odd == 2: non-adjacent form with odd-multiple buckets
    uint32_t multiples = 1;              // non-adjacent form over a table with odd-multiple rows: digits +-(2 t + 1) b, t < multiples (u32 digit rows)
    uint32_t H = 0, L = 0, T = 0, groups = 1;   // buckets per set, per first-level chunk, chunks per set, index groups per MSM
    size_t windows = 0, bsets = 0, nbuckets = 0, ndigits = 0, per_set_scalars = 0, per_set_digits = 0;
    MsmSort sort = MsmSort::global;
    MsmReduce reduce = MsmReduce::chunks;
    MsmFinish finish = MsmFinish::group_sum;
    uint32_t n_pad = 0, digits_per_set = 0;                  // sets_staged: u16 digit row length and digits per set
    uint32_t part_p = 1, part_shift = 0;                     // partition: partitions per set, bucket >> part_shift = partition
    uint32_t part_tile = 0, part_tiles_per_set = 0, part_cap = 0;   // scalars per pass-A workgroup, its workgroups per set, stream room
    uint32_t ws_per_lane = 1, ws_span = 0;                   // wg_scan: buckets per lane and per workgroup, workgroups
    size_t wg_per_set = 0, wg_count = 0;
    size_t szblocks = 0, ncells = 0;     // size sort: workgroups and histogram cells
    struct { size_t counts, offsets, tiles, perm, cells, cell_off, buckets, partial, winsum, heavy, sorted, digits, cursor, part_base, result; }
        bytes{};                         // bytes of each ctx scratch buffer the call reserves (0: not used)
    size_t nparts() const { return bsets * (size_t)part_p; }
};

// the window tiling, index groups and reduction chunks of a call; allow_naf = false keeps a bit-row table's window rows
inline MsmPlan msm_shape(size_t n, size_t batch, const MsmTable* tbl, const MsmKnobs& k, bool allow_naf) {
    MsmPlan p;
    p.n = n, p.batch = batch, p.single = tbl != nullptr && tbl->table != nullptr;
    if (p.single) {
        const Tiling tl = allow_naf ? tiling_for(*tbl, n, batch, k.naf_tiling) : Tiling{false, 0, 0, 0.0, 1};
        if (tl.naf) {           // slots of the non-adjacent form: positions [c j, c j + c) of k << shift (msm_recode.hip.h: for_each_wnaf_digit)
            const int shift = tl.slots * tl.c - 256;
            p.wt.W = tl.slots, p.wt.cmax = tl.c, p.wt.odd = 2, p.multiples = tl.multiples;
            for (int j = 0; j < p.wt.W; j++)
                p.wt.start[j] = (uint8_t)(tl.c * j), p.wt.row[j] = (uint8_t)(j ? tl.c * j - shift : 0), p.wt.width[j] = (uint8_t)tl.c;
        } else {
            p.wt = tbl->wt;
        }
        p.H = 1u << (p.wt.cmax - (tl.naf ? 2 : 1));
    } else {
        const bool latency_bound = batch == 1 && n <= 32768;
        p.wt = dr::make_window_table(dr::forced_window_ok(k.force_c) ? k.force_c : latency_bound ? dr::pick_window_latency(n) : dr::pick_window(n));
        p.H = 1u << (p.wt.cmax - 1);
    }
    p.L = std::min<uint32_t>(p.H, 16u);
    // table mode: split the points of each MSM into index groups when one bucket set per MSM would leave lanes idle
    if (p.single) {
        // 8 waves per SIMD: finer slices balance better than 4 (2^20 bases: accumulate 3.98 -> 3.6 ms); below 2^19 points half of that —
        // every bucket is another lane-step of the reduction's chain, and the walk is short anyway (2^16 pairs over 16-bit windows:
        // 8 groups 0.875 ms, 16 groups 1.03, 2 groups 0.96)
        const size_t target_lanes = n >= ((size_t)1 << 19) ? 524288 : 262144;
        while (p.groups < 64 && batch * p.groups * (size_t)p.H < target_lanes && n / (p.groups * 2) >= 64) p.groups *= 2;
        if (k.force_groups > 0 && batch == 1 && n / (size_t)k.force_groups >= 64) p.groups = (uint32_t)k.force_groups;
    }
    p.windows = batch * (size_t)p.wt.W;                  // digit rows
    p.bsets = p.single ? batch * p.groups : p.windows;   // bucket sets
    // few bucket sets of moderate size (a single MSM over a window table): the reduction is a latency chain of 2L additions + a
    // log2(H)-bit double-and-add + the fold of H/L partial sums; L = 4 makes it ~40 % shorter
    // (one huge MSM, 16 groups x 32768 buckets: L stays 16 — measured 0.90 ms for the chunk kernel against 1.15 at L = 8 and 1.00
    //  at L = 4: every chunk pays a 15-bit double-and-add whatever its length)
    if (p.single && p.L == 16 && p.H >= 256 && p.H <= 4096 && p.bsets * (size_t)(p.H / 16) < L4_BELOW) p.L = 4;
    // the same for a small MSM over plain bases (the verifier's 2- and 11-point folds): 41 -> 16 dependent additions
    if (!p.single && p.L == 16 && p.H >= 16 && p.bsets * (size_t)(p.H / 16) < ((size_t)1 << 12)) p.L = 4;
    p.T = p.H / p.L;
    p.per_set_scalars = p.single ? (n + p.groups - 1) / p.groups : n;
    p.per_set_digits = p.single ? p.per_set_scalars * (size_t)p.wt.W : n;
    // small bucket sets fed by a bounded number of digits (the batched prover): one workgroup sorts a set entirely in LDS
    const bool lds_sort = p.H <= dr::SORT_MAX_H && p.bsets >= 64 && p.per_set_digits <= (1u << 20) && p.bsets * p.per_set_digits < (1ull << 32);
    p.sort = lds_sort ? MsmSort::sets : MsmSort::global;
    // many sets of <= 4096 buckets (every batched MSM of the prover): first level with 2 additions per bucket, then one workgroup per
    // set scans and folds its <= 256 chunk results
    const bool setscan = p.L == 16 && p.T >= 8 && p.T <= 256 && p.bsets >= 256;
    p.reduce = setscan ? MsmReduce::set_scan : MsmReduce::chunks;
    return p;
}

inline MsmPlan plan_msm(size_t n, size_t batch, const MsmTable* tbl, const MsmKnobs& k) {
    // the non-adjacent form needs the LDS sort and the set scan: a shape that would not get them keeps the table's window rows
    MsmPlan p = msm_shape(n, batch, tbl, k, true);
    if (p.wt.odd && !(p.sort == MsmSort::sets && p.reduce == MsmReduce::set_scan)) p = msm_shape(n, batch, tbl, k, false);
    const uint32_t H = p.H, T = p.T, W = (uint32_t)p.wt.W;
    const size_t bsets = p.bsets;
    // (a sorted entry is (t * 256 + row) * stride + i | sign << 31: the last block of a table with multiples counts from (multiples - 1) * 256)
    if (p.single && ((uint64_t)(p.multiples - 1) * 256 + p.wt.row[W - 1] + p.wt.cmax + 1) * tbl->stride >= (1ull << 31)) { p.error = "window table too large"; return p; }
    p.nbuckets = bsets * (size_t)H, p.ndigits = p.windows * n;
    if (p.nbuckets >= (1ull << 32) || p.ndigits >= (1ull << 32)) { p.error = "MSM batch too large for one launch (split the batch)"; return p; }

    // ---- sort
    if (p.sort == MsmSort::sets) {
        // sets of more than a few thousand entries: the sorted segment is assembled in LDS and written in whole lines
        const uint32_t stage_chunk = (H <= dr::SORT2_SMALL_H ? dr::SORT2_CAP_SMALL_H : dr::SORT2_CAP_LARGE_H) - dr::SORT2_SLACK;
        if (p.per_set_digits >= 4096 && p.per_set_digits / stage_chunk + 1 <= dr::SORT2_MAX_CHUNKS) {
            p.sort = MsmSort::sets_staged;
            p.n_pad = (uint32_t)((p.per_set_scalars + 7) & ~(size_t)7), p.digits_per_set = p.n_pad * (p.single ? W : 1u);
        }
    }
    // a few huge sets over a window table (one 2^20-point MSM): two-pass partition sort
    const size_t chunk = dr::PART_STAGE - dr::PART_SLACK;
    while (p.part_p < dr::PART_MAX_P && (H / p.part_p > dr::PART_MAX_HP || p.per_set_digits / p.part_p > chunk - chunk / 16)) p.part_p *= 2;
    while ((H >> p.part_shift) > p.part_p) p.part_shift++;
    if (p.sort == MsmSort::global && p.single && batch == 1 && W <= 32 && H >= p.part_p && H / p.part_p <= dr::PART_MAX_HP &&
        p.per_set_digits / p.part_p <= 48 * chunk && bsets * p.per_set_digits < (1ull << 32) && p.per_set_digits >= 65536) {
        p.sort = MsmSort::partition;
        p.part_tile = std::min<uint32_t>(2048, dr::PART_TILE_ENTRIES / W);
        p.part_tiles_per_set = (uint32_t)((p.per_set_scalars + p.part_tile - 1) / p.part_tile);
        p.part_cap = (uint32_t)std::min<size_t>(p.per_set_digits, std::max<size_t>(4 * p.per_set_digits / p.part_p, 65536));
    }

    // ---- reduction
    // many bucket sets (batched prover): level-wise reduction, 2 additions per entry and no scalar multiplications;
    // few sets (single MSMs): chunk sums + double-and-add, whose latency is one short chain
    const bool setscan = p.reduce == MsmReduce::set_scan;
    const bool leveled = p.L == 16 && H >= 256 && bsets * (size_t)(H / 16) >= ((size_t)1 << 18);
    // a single MSM over a wide window table (H >= 8192 buckets per index group): workgroup scan, (V, S) pairs to the host
    // buckets per lane of that scan: as few as keep the launch within one wave per SIMD (65536 lanes), at most 8
    // One plain MSM of a few thousand points (the batch verifier's folds, a single KZG.commit; ~22 windows of 256 .. 4096 buckets): the same
    // scan, four workgroups per window — 2 x buckets-per-lane + 17 additions deep where the chunk kernel (8 running-sum additions, a
    // double-and-add over the chunk index) and its fold were ~37: reduction 0.49 -> 0.3 ms of a 0.85 ms call.
    const bool plain_one = !p.single && batch == 1 && !setscan && !leveled && H >= 256 && !p.wt.odd;
    if (plain_one) p.ws_per_lane = std::min<uint32_t>(8u, std::max<uint32_t>(1u, H / 1024u));
    else while (p.ws_per_lane < 8 && bsets * (size_t)H > (size_t)65536 * p.ws_per_lane) p.ws_per_lane *= 2;
    p.ws_span = dr::WS_BLOCK * p.ws_per_lane;
    // ... and up to 32 MSMs over a window table whose launch does not fill the chip (RingVRF.prove of ONE proof: 1, 2 and 4 commitments,
    // up to 32 index groups of 512 .. 2048 buckets each; prove_batch of 8 / 16 / 32 proofs: 6.7 -> 6.5, 6.95 -> 6.4, 8.1 -> 7.6 ms): the
    // chunk kernel's chain there was 8 additions + an 11-bit double-and-add + the fold, ~0.65 ms per call; the scan is 19 additions deep
    const bool few_table = p.single && batch <= 32 && !setscan && !leveled && H >= 256 && !p.wt.odd && bsets * (size_t)H <= ((size_t)1 << 19);
    const bool wgscan = (plain_one || few_table || (!setscan && !leveled && p.single && batch == 1 && H >= 8192)) && H % p.ws_span == 0;
    p.wg_per_set = H / p.ws_span, p.wg_count = bsets * p.wg_per_set;
    if (!setscan) p.reduce = leveled ? MsmReduce::levels : wgscan ? MsmReduce::wg_scan
                           : T > 512 && T % 256 == 0 ? MsmReduce::chunks_two_stage : MsmReduce::chunks;
    // ---- results
    if (p.single) p.finish = wgscan || p.groups > 1 || batch == 1 ? MsmFinish::group_sum : MsmFinish::device_copy;
    else p.finish = batch == 1 ? MsmFinish::host_horner : MsmFinish::device_horner;

    // ---- workspace
    p.szblocks = (p.nbuckets + dr::SZ_TILE - 1) / dr::SZ_TILE, p.ncells = (size_t)dr::SZ_CLASSES * p.szblocks;
    auto& b = p.bytes;
    b.counts = b.perm = p.nbuckets * 4, b.offsets = (p.nbuckets + 1) * 4;
    b.tiles = (size_t)((std::max(p.ncells, p.nbuckets) + dr::SCAN_TILE - 1) / dr::SCAN_TILE + 1) * 4;
    b.cells = p.ncells * 4, b.cell_off = (p.ncells + 2) * 4;
    b.buckets = p.nbuckets * 192;
    size_t levels = 0;                                   // [S | C] per level, sizes sets * H/16, sets * H/256, ...
    for (uint32_t m = H; m > 16; m /= 16) levels += 2 * bsets * (m / 16);
    b.partial = std::max((bsets * T + bsets * (T / 256 + 1)) * 192, p.reduce == MsmReduce::set_scan ? 2 * bsets * T * 192
                         : p.reduce == MsmReduce::wg_scan ? 2 * p.wg_count * 192 : p.reduce == MsmReduce::levels ? levels * 192 : 0);
    b.winsum = bsets * 192;
    // segment sums of lists >= 1024 entries: sum_i ceil(len_i / seg) <= total / seg + n_heavy.  Up to 1024 heavy lists: seg >= 1024, so
    // total / 1024 + 1024; more of them: seg = 4096 and n_heavy <= total / 1024, so total / 4096 + total / 1024 (heavy_segment_size)
    b.heavy = (p.ndigits / 1024 + p.ndigits / 4096 + dr::G1_HEAVY_SLOTS / 2 + 64) * 192;
    // (a partition sort's room covers the global-atomic sort its second pass may fall back to; cursor: + fill counters, overflow flag)
    const bool global = p.sort == MsmSort::global, part = p.sort == MsmSort::partition;
    b.sorted = global ? p.ndigits * 4 : bsets * p.per_set_digits * 4;
    b.digits = global ? p.ndigits * 4 : part ? p.nparts() * p.part_cap * 8 : bsets * (size_t)p.digits_per_set * (p.multiples > 1 ? 4 : 2);
    b.cursor = global ? p.nbuckets * 4 : part ? std::max(p.nparts() + 1, p.nbuckets) * 4 : 0;
    b.part_base = part ? p.nparts() * 4 : 0;
    b.result = batch > 1 ? batch * 192 : 0;
    return p;
}
