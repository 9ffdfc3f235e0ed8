// qs_abi.hip -- implementation of the C-ABI declared in include/quartetscores_hip.h.
//
// Host-side orchestration only: validation of the flattened trees, device memory, kernel
// dispatch, and the O(#node pairs) finalisation of the scores. All O(m*C(n,4)) and O(C(n,4))
// work runs in the HIP kernels of qs_count.hip / qs_score.hip. There is no CPU fallback.
#include "../../include/quartetscores_hip.h"
#include "qs_common.hpp"
#include "qs_devbuf.hpp"
#include "qs_internal.hpp"

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <future>
#include <limits>
#include <memory>
#include <string>
#include <thread>
#include <vector>

using namespace qs;

struct EarlyPerm { std::vector<uint32_t> perm; uint32_t chunk = 0, cblock_in = 0, cgroup = 0; bool ok = false; };

struct qs_device_batch {
    DeviceBatch d;
    std::vector<uint32_t> fix_slot;   // depth clamp: slot (in the class-ordered batch) of the tree behind every correction unit, ascending
    std::vector<uint64_t> fix_work;   // n_fix + 1 prefix sums: triples x fourth leaves of every unit (what the split of a slice is planned from)
};

// the reference tree, flattened and indexed for scoring (build_ref)
struct RefHost {
    uint32_t n_nodes = 0, n = 0, n_inner = 0, root = 0;
    std::vector<int32_t> parent;
    std::vector<uint32_t> depth, nchild, inner_id, inner_node;
    std::vector<uint32_t> lca; // n*n
    std::vector<uint16_t> next; // n*n: for a < b the first a' > a with lca(a',b) != lca(a,b) (b if none): run ends of the score scan
    std::vector<uint32_t> leaf_node_in; // the caller's leaf_node array (cache key)
    std::vector<uint32_t> leaf_lo, leaf_cnt; // per node: its leaves are the lookup ids [leaf_lo, leaf_lo + leaf_cnt)
    bool bifurcating = false;
    bool root_deg2 = false;             // rooted Newick: the root has exactly two children
    std::vector<RootPairHost> root_pairs; // the node pairs (root, v) of such a tree, as the reference enumerates them
    uint32_t root_split = 0;            // ... and the number of taxa under the root's first child: lookup ids [0, root_split)
    uint64_t root_items = 0;
};

static int build_ref_shape(qs_ctx *c, const qs_ref_tree *ref, RefHost &R);

struct qs_ctx {
    uint32_t n = 0, count_bits = 32, flags = 0;
    int device = 0;
    hipStream_t stream = nullptr;
    uint32_t d_lo = 0, d_hi = 0;
    uint64_t rank_lo = 0, n_tuples = 0;
    void *table = nullptr;          // the context's own (table_mem) or the caller's (qs_table_attach)
    DevBuf<void> table_mem;         // qs_table_alloc
    uint64_t trees_counted = 0;
    uint32_t *wire_out = nullptr;   // qs_wire_attach: destination of QS_COUNT_WIRE16X2 (one word per tuple)
    uint64_t wire_trees = 0;        // trees accumulated in it
    // geometry
    DevBuf<uint32_t> dprefix, cprefix;
    uint32_t n_dblk = 0, total_tiles = 0;
    DevBuf<uint32_t> dprefix3, cprefix3; // tiling of count_bitslice3_kernel, every mode (16x8 tiles, d-blocks counted down from d_hi)
    uint32_t total_tiles3 = 0;
    // (a,b)-major launch order of count_bitslice3_kernel's tiles (tile_order below): launch slot -> tile id, built on
    // first use. Empty = (d,c)-major (identity).
    DevBuf<uint32_t> perm;
    bool perm_built = false;
    std::future<EarlyPerm> perm_early;                 // the launch order, started by qs_create before its first HIP call
    uint32_t tile_chunk = 2, tile_cblock = 32;         // a-block (pairs) per chunk / c values per c-block; chunk 0 = (d,c)-major (round 3: 4 | 16 -> 2 | 32, -1.5 %)
    uint32_t tile_cgroup = 0;                          // > 1: c innermost in groups of this many (the waves of a workgroup share M[ab], M[bd])
    // binary tiling, cooperative workgroups (count_bitslice4_kernel): launch slots in groups of 4 tiles of one (a-blocks,
    // b-block, d-block) with consecutive c (bit 31 = shadow tile: takes part, does not store), and the list of the tiles
    // that stay with count_bitslice3_kernel (diagonal tiles, tiles without a second a-block)
    DevBuf<uint32_t> perm_coop, perm_rest;
    uint32_t n_coop = 0, n_rest = 0;
    uint32_t tune_coop = 0;                            // QS_TUNE_COOP: 1 = cooperative workgroups on; 0 / 2 = off (the default: measured slower)
    std::vector<uint32_t> h_cp3, h_dp3;                // host copies of the prefix arrays
    // workspace
    DevBuf<void> panel;
    DevBuf<uint32_t> dev_flags; // [0] counter overflow, [1] score flags, [3] two-cell wire format: tuple sum mismatch
    std::vector<hipEvent_t> evs;   // QS_COUNT_TIMED: evs[0] = start, then one event after every kernel launch
    std::vector<uint8_t> ev_kind;  // per event after evs[0]: 0 = panel build, 1 = count kernel, 2 = depth-clamp corrections (clamp_fix_kernel),
                                   // 3 = no kernel of the step (the wait for the correction stream, the set-up of a new split), 4 = second count launch of a split slice
    std::vector<uint32_t> ev_from; // ... and the event its interval starts at (the one before it, unless a split slice says otherwise)
    uint32_t ev_used = 0;
    bool last_timed = false;
    // Split slices (run_launch): the corrections of the upper d-range run on fix_stream beside the count launch of the lower one.
    // split = the tilings of the two ranges for the d_mid they were last built for (launch orders: built with the first split launch).
    DevStream fix_stream;
    DevEvent fix_go, fix_done;     // fix_go: the upper range is stored (main stream); fix_done: its corrections are in (correction stream)
    struct Split {
        uint32_t d_mid = 0;                  // 0 = none built
        const uint32_t *perm_of = nullptr;   // the full launch order the two below were cut from (NULL: identity order, none needed)
        uint32_t n_dblk_hi = 0, tiles_hi = 0, n_dblk_lo = 0, tiles_lo = 0;
        DevBuf<uint32_t> dprefix_lo, perm_hi, perm_lo, filter_scratch;
        std::vector<uint32_t> h_dp_lo, h_perm_lo;
        DevEvent copied;                     // behind the copies out of the two host lists
        bool copied_valid = false;
    } split;
    uint32_t tune_fix_overlap = 1;           // QS_TUNE_FIX_OVERLAP
    uint32_t tune_fix_split_at = 0;          // QS_TUNE_FIX_SPLIT_AT (tests): d_mid of every split, 0 = planned
    uint32_t last_split = 0, last_splits = 0; // qs_last_count_split: d_mid of the last split slice of the last count, and how many there were
    // qs_set_tuning
    uint64_t tune_slice_bytes = 0; // 0 = automatic
    uint32_t tune_gather_impl = 0; // QS_IMPL_*
    uint32_t tune_panel_kernel = 0;
    uint32_t tune_cand_slots = kCand;  // candidate slots pass 2 fills per node pair (tests force overflows with fewer)
    int tune_score_kernel = 0;         // 0 = bundle kernel, 1 = scan kernel (QS_TUNE_SCORE_KERNEL)
    double tune_score_tol = 1e-12;     // pass 2 keeps triples whose device QIC is within this of the pair's minimum
    DevBuf<double> dev_logk;       // log(k) table of the device QIC (qs_score.hip), tbl_n entries
    uint32_t tbl_n = 0;
    // scoring view (qs_score_set_view): tuples [view_rank_lo, view_rank_lo + view_n) in caller-owned device memory
    const void *view_table = nullptr;
    uint32_t view_bits = 0;
    uint64_t view_rank_lo = 0, view_n = 0;
    std::string variant;
    std::string err;
    // the flattened reference tree of the last scoring call, its LCA matrix on the device (qs_score_pass1 / pass2 /
    // raw_qic / finish of one scoring run all get the same tree: built once, not three times)
    std::unique_ptr<RefHost> ref_cache;
    DevBuf<uint32_t> ref_lca_dev;
    DevBuf<uint16_t> ref_next_dev;
    DevBuf<void> root_pairs_dev;
    BundlePlan bundle[3];              // rounds of the score bundle kernel in pass 1 / pass 2 for [bundle_r0, bundle_r1) (plan_bundles); [2]: qs_taxon_support
    uint64_t bundle_r0[3] = {~0ull, ~0ull, ~0ull}, bundle_r1[3] = {~0ull, ~0ull, ~0ull};
    DevBuf<uint32_t> bundle_dev[3];    // plo[n] | pcnt[n] | rounds[2 R]
    int n_cu = 0;
    // tree batches go to the device through two pinned staging buffers on a copy stream of their own:
    // qs_batch_upload returns once the batch is in pinned memory, the copy of batch k+1 overlaps the counting of batch k
    hipStream_t copy_stream = nullptr;
    hipStream_t prep_stream = nullptr;           // qs_score_prepare: uploads of the scoring set-up go here instead of `stream` (which may hold count kernels)
    PinBuf<void> pin[2];
    hipEvent_t pin_ev[2] = {nullptr, nullptr};   // recorded after the last copy out of the buffer
    unsigned pin_next = 0;
    std::vector<BatchSlab> slabs;                // device slabs of freed batches, for the next uploads
    // qs_last_score_ms: phases of the last qs_score call (host clock, passes 1 / 2 by HIP events on the stream)
    float score_ms[6] = {0, 0, 0, 0, 0, 0};
    hipEvent_t score_ev[3] = {nullptr, nullptr, nullptr};
    uint64_t table_trees_hint = 0;               // QS_TUNE_TABLE_TREES: trees behind an attached / uploaded / viewed table
    // single-read scoring (qs_score): pass 1 logs candidate (node pair, triple) records, score_log_kernel filters them
    DevBuf<unsigned long long> score_log;        // log_cap records of 4 words + 1 word counter behind them
    uint64_t score_log_cap = 0;
    bool log_valid = false;                      // the candidate log holds the last qs_score_pass1 of (log_table, log_rank_lo, log_n_tuples, log_ref)
    const void *log_table = nullptr, *log_ref = nullptr;
    uint64_t log_rank_lo = 0, log_n_tuples = 0;
    double log_tol = 0.0;
    uint32_t tune_score_passes = 0;              // QS_TUNE_SCORE_PASSES: 0 = automatic (default), 1 = two passes over the table, 2 = single read
    DevBuf<void> score_acc;                      // qs_score's accumulators on the device + their pinned host copy (cached)
    PinBuf<void> score_acc_host;
    uint64_t last_score_estimate = 0;            // automatic single-read mode: predicted log records of the last qs_score (sample x S)
    uint64_t last_score_log = 0;                 // records the last single-read qs_score logged (0 = two passes were used)
    uint32_t tune_class_min = 1024;              // QS_TUNE_CLASS_MIN_TREES
    uint32_t tune_class_pct = 10;                // QS_TUNE_CLASS_PCT: a depth class below this share of the batch's trees is merged into the next one
    uint32_t tune_fuse = 1;                      // QS_TUNE_FUSE_CLASSES: classes of equal depth bits share ONE launch of the count kernel (qs_count_fused.hip)
    uint32_t tune_clamp_ppm = 20;                // QS_TUNE_DEPTH_CLAMP: corrections a tree may cost per depth bit it saves, in millionths of C(n,4); 0 = no clamp
    uint32_t tune_score_load = 0;                // QS_TUNE_SCORE_LOAD: 0 = a lane loads its row in 16-byte pieces, 1 = eight lanes load a row's chunk (LDS hand-over)
    uint32_t tune_score_dedupe = 1;              // QS_TUNE_SCORE_DEDUPE: the logging pass skips a quartet that repeats its node pair's last logged triple
    uint32_t tune_score_sample = 64u | 65536u;             // QS_TUNE_SCORE_SAMPLE: pre-pass of the single-read scoring (0 = none; S | by-round bit 16)
    uint64_t tune_score_log_cap = 0;             // QS_TUNE_SCORE_LOG_CAP: records the log may hold (0 = 8 M); tests force overflows
    DevBuf<uint16_t> remap_ids;                  // qs_table_remap / qs_table_restrict: src_id_of on the device (n entries)
    // qs_tree_agreement: the reference tree's inner nodes (>= 3 links) as id boundaries on the device, and the tree they came from
    std::vector<int32_t> agree_parent;
    std::vector<uint32_t> agree_leaf_node;
    DevBuf<uint32_t> agree_off;
    DevBuf<uint16_t> agree_bnd;
    DevBuf<uint8_t> agree_par;
    uint32_t agree_n_u = 0;
    // qs_taxon_placement: the cached reference tree's link lookups (dropped with ref_lca_dev), the walks of an n-taxon table and
    // the list of the last call; the host copies stay until the uploads on `stream` have read them
    std::vector<uint16_t> place_child, place_next, place_taxa;
    std::vector<uint32_t> place_tasks;
    DevBuf<uint16_t> place_child_dev, place_next_dev, place_taxa_dev;
    DevBuf<uint32_t> place_node_dev, place_tasks_dev;
    // qs_clade_placement: the walks in the numbering of the ids outside a clade (one list for every clade size) and the last call's
    // clades and workgroups, kept like the lists above
    std::vector<uint32_t> clade_tasks, clade_list;
    DevBuf<uint32_t> clade_tasks_dev, clade_list_dev;
};

static thread_local std::string g_create_err;   // per thread: qs_create of several contexts may run concurrently (multi_gpu.hpp)
// Tree groups (panel elements along the tree axis) per sub-batch of a batch of n_total groups.
// A batch is counted slice by slice: panel build + count kernel per slice, the first slice stores into the table, the
// others read-modify-write it. qs_set_tuning(QS_TUNE_PANEL_SLICE_BYTES) fixes the slice size in bytes (tests, sweeps).
//  * bit-sliced kernel in (a,b)-major tile order (the default): what must stay in an XCD's 4 MB L2 is the working set of
//    its concurrent tiles, which grows with the number of groups G of the slice (about 40 KB x G at 20-byte elements), not
//    with the panel's size; against that every extra slice costs one read + one write of the table. Measured optimum
//    (profiles/r02_experiments.md): 128-150 groups at 256 taxa (2 GB table), ~105 at 512 taxa (34 GB table; 3 slices
//    for 10000 trees: 401 ms, 2: 415, 5: 432, unsliced 440), >= 80 at 1024 taxa (34 GB table shard). Rule: 128 groups,
//    slices balanced (313 groups -> 3 x 105, not 128 + 128 + 57), at most 2 GiB of panel.
//  * (d,c)-major order and the byte-SWAR kernel: the whole slice has to stay in the 256 MiB Infinity Cache while every
//    wave streams through it: 96 MiB, but at least 32 groups (a tile's fixed cost needs that many steps to amortise),
//    capped at 384 MiB (round-1 measurements: 512 taxa 0.60 s at 100 MB, 0.72 s at 50 MB, 0.80 s unsliced).
static uint32_t slice_groups(const qs_ctx *c, size_t group_bytes, uint32_t n_total, bool ab_major) {
    size_t g;
    bool balance = false;
    if (c->tune_slice_bytes) g = (size_t)c->tune_slice_bytes / group_bytes;
    else if (ab_major) {
        // Every slice costs a pass over the table (read + write of every tuple), a larger slice a larger L2 working set. Measured
        // on the round-3 kernel (profiles/r03_experiments.md 14): 512 taxa x 30000 trees best at 256 groups per slice (670 MB;
        // 128: +3.5 %, 512: +0.7 %), 256 taxa x 100000 best at 512 groups (334 MB; 128: +3 %, 1024: +1.5 %), a 34 GB shard of 1024
        // taxa x 5000 trees best in ONE slice of 157 groups (1.65 GB; two slices: +5 %): 256 groups, but at least 350 MB worth.
        g = std::max<size_t>(256, (350ull << 20) / group_bytes);
        g = std::min<size_t>(g, std::max<size_t>(1, (4096ull << 20) / group_bytes));
        balance = true;
    }
    else g = std::min<size_t>(std::max<size_t>(96ull << 20, 32 * group_bytes), 384ull << 20) / group_bytes;
    g = std::min<size_t>(std::max<size_t>(g, 1), std::max<uint32_t>(n_total, 1));
    // (round 5: up to 1.5 slices' worth stays ONE slice -- 313 groups at configs[2] since the depth clamp put all 10000 trees in one
    // class: 301.5 ms in one slice against 308.1 ms in two of 157, the second pass over the table costs more than the larger L2 set)
    if (balance && !c->tune_slice_bytes && n_total <= g + g / 2) g = std::max<uint32_t>(n_total, 1);
    if (balance) { const size_t slices = (n_total + g - 1) / g; g = (n_total + slices - 1) / std::max<size_t>(slices, 1); }
    return (uint32_t)std::max<size_t>(g, 1);
}

// QS_COUNT_TIMED: an event after every kernel launch of the call (created on demand, re-used by later calls)
// The event goes onto the stream its kernel ran on (`on`; NULL pointer = the context's stream). Its interval starts at event
// `from` (index into evs), by default the event recorded before it.
constexpr uint32_t kEvPrev = ~0u;
static hipError_t mark(qs_ctx *c, int kind, const hipStream_t *on = nullptr, uint32_t from = kEvPrev) {
    if (c->ev_used == c->evs.size()) {
        hipEvent_t e;
        hipError_t rc = hipEventCreate(&e);
        if (rc != hipSuccess) return rc;
        c->evs.push_back(e); c->ev_kind.push_back(0); c->ev_from.push_back(0);
    }
    c->ev_kind[c->ev_used] = (uint8_t)kind;
    c->ev_from[c->ev_used] = from != kEvPrev ? from : (c->ev_used ? c->ev_used - 1 : 0);
    return hipEventRecord(c->evs[c->ev_used++], on ? *on : c->stream);
}

static int fail(qs_ctx *c, int code, const std::string &msg) {
    if (c) c->err = msg; else g_create_err = msg;
    return code;
}

#define QS_HIP(c, expr)                                                                                 \
    do {                                                                                                \
        hipError_t e__ = (expr);                                                                        \
        if (e__ != hipSuccess)                                                                          \
            return fail((c), e__ == hipErrorOutOfMemory ? QS_ERR_OOM : QS_ERR_HIP,                      \
                        std::string(#expr) + ": " + hipGetErrorString(e__));                            \
    } while (0)

extern "C" const char *qs_version(void) { return "quartetscores_amd 0.1.0 (gfx950)"; }

extern "C" const char *qs_last_error(const qs_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }

// (a,b)-major launch order of the tiles of count_bitslice3_kernel. The kernel decodes a tile id as (d-block k, c, tile
// inside c) -- the order in which the TABLE is contiguous. Walked in that order, the waves that run at the same time
// cover every (a,b) pair, so the private M[ab] loads (60 % of a wave's panel bytes) never hit in L2 and the launch is
// bound by the Infinity Cache (knock-out at 512 taxa: no panel loads = 45 % less time; profiles/r02_experiments.md).
// Here the launch slots are permuted: outermost the b-block Bk and a chunk of `chunk` a-blocks (pairs of a-blocks in
// the binary tiling) under it, then blocks of `cblock` values of c, then the d-blocks, then c inside the block,
// innermost the a-blocks of the chunk. Concurrent waves of an XCD (with xcd_remap each XCD walks a contiguous eighth of
// the slots) then share one chunk's M[ab] elements (8 b-rows x 16*chunk a's x the tree groups of the slice), the
// M[bd] elements of (Bk, d-block) and the M[xc] rows of the c-block, which stay in its 4 MB L2; per (c,d) a chunk still
// writes 8 contiguous runs of the table. Diagonal tiles follow at the end. 512 taxa x 10000 trees: 568 -> 401 ms,
// 256 taxa: -35 %. Shards with more than 2^26 tiles keep the (d,c)-major order (the slot array would be > 256 MB).
// Host part of the launch order: the (a,b)-major enumeration of the 16x8 tiles of count_bitslice3_kernel (two a-columns per lane in
// every instance since round 4) as launch slot -> tile id, checked to be a bijection. Pure host code (no context, no HIP):
// qs_create starts it on a helper thread BEFORE its first HIP call, so that in a fresh process the ~25 ms it takes at 512 taxa pass
// while the HIP runtime comes up (round 5: the CLI's first launch 25 ms earlier).
struct TilePermParams { uint32_t chunk, cblock_in, cgroup, d_hi, n_dblk, total; };
static bool build_tile_perm(const TilePermParams &P, const std::vector<uint32_t> &cp, const std::vector<uint32_t> &dp, std::vector<uint32_t> &perm,
                            std::string &err) {
    const uint32_t total = P.total, chunk = P.chunk, d_hi = P.d_hi, n_dblk = P.n_dblk;
    perm.clear();
    perm.reserve(total);
    auto T_of = [](uint32_t cc) { return (cc + 7) / 8; };
    const uint32_t cmax = d_hi >= 2 ? d_hi - 2 : 0;          // largest c of any tile
    const uint32_t Tmax = T_of(cmax);
    const uint32_t cblock = P.cblock_in ? P.cblock_in : cmax + 1;
    // off-diagonal tiles under b-block Bk. (Building the lists of several Bk on helper threads was tried: in the CLI, where 8 host
    // threads flatten the first batch at the same time, the set-up thread then was ready after 27-30 ms instead of 24.)
    auto emit_Bk = [&](uint32_t Bk, std::vector<uint32_t> &out) {
        // tile Bk^2/4 + j = a-blocks (2j, 2j+1)
        const uint32_t base = (Bk * Bk) / 4;
        const uint32_t nj = ((Bk + 1) * (Bk + 1)) / 4 - base;
        const uint32_t c_lo = std::max(2u, 8 * Bk + 1);      // T(c) > Bk
        for (uint32_t j0 = 0; j0 < nj; j0 += chunk) {
            const uint32_t j1 = std::min(nj, j0 + chunk);
            for (uint32_t cb = c_lo; cb <= cmax; cb += cblock)
                for (uint32_t k = 0; k < n_dblk; ++k) {
                    const uint32_t d1 = d_hi - k * kDB;
                    if (P.cgroup <= 1) {
                        for (uint32_t cc = cb; cc < cb + cblock && cc + 1 < d1; ++cc) {
                            const uint32_t id = dp[k] + cp[cc] + base;
                            for (uint32_t j = j0; j < j1; ++j) out.push_back(id + j);
                        }
                    } else {
                        // c innermost in groups of `cgroup`: the waves of a workgroup (consecutive slots) then hold the SAME
                        // (a-blocks, b-block, d-block) and consecutive c -- their M[ab] and M[bd] elements are identical
                        for (uint32_t c4 = cb; c4 < cb + cblock && c4 + 1 < d1; c4 += P.cgroup)
                            for (uint32_t j = j0; j < j1; ++j)
                                for (uint32_t cc = c4; cc < c4 + P.cgroup && cc < cb + cblock && cc + 1 < d1; ++cc)
                                    out.push_back(dp[k] + cp[cc] + base + j);
                    }
                }
        }
    };
    for (uint32_t Bk = 1; Bk < Tmax; ++Bk) emit_Bk(Bk, perm);
    for (uint32_t kd = 0; kd < (Tmax + 1) / 2; ++kd)          // diagonal tiles (two diagonal blocks each)
        for (uint32_t k = 0; k < n_dblk; ++k) {
            const uint32_t d1 = d_hi - k * kDB;
            for (uint32_t cc = 2; cc + 1 < d1; ++cc) {
                const uint32_t T = T_of(cc);
                if (kd < (T + 1) / 2) perm.push_back(dp[k] + cp[cc] + (T * T) / 4 + kd);
            }
        }
    if (perm.size() != total) { err = "tile order: enumeration does not match the tiling"; return false; }
    {   // every tile exactly once: a tile listed twice would be counted by two waves (a race on its tuples), one left out never
        std::vector<uint64_t> seen((total + 63) / 64, 0);   // (a bit per tile: 350 KB at 512 taxa, stays in the host's L2)
        for (uint32_t id : perm) {
            if (id >= total || ((seen[id >> 6] >> (id & 63)) & 1ull)) { err = "tile order: launch permutation is not a bijection"; return false; }
            seen[id >> 6] |= 1ull << (id & 63);
        }
    }
    return true;
}

static int tile_order(qs_ctx *c, const uint32_t **out) {
    *out = nullptr;
    if (c->perm_built) { *out = c->perm.get(); return QS_OK; }
    c->perm_built = true;
    const uint32_t total = c->total_tiles3;
    const uint32_t chunk = c->tile_chunk;
    if (chunk == 0 || total == 0 || total > (1u << 26)) {
        if (c->perm_early.valid()) c->perm_early.wait();
        return QS_OK;
    }
    const uint32_t d_hi = c->d_hi, n_dblk = c->n_dblk;
    const std::vector<uint32_t> &cp = c->h_cp3, &dp = c->h_dp3;
    const TilePermParams P{chunk, c->tile_cblock, c->tile_cgroup, d_hi, n_dblk, total};
    std::vector<uint32_t> perm;
    std::string perr;
    bool have = false;
    if (c->perm_early.valid()) {       // started by qs_create beside the HIP start-up
        EarlyPerm ep = c->perm_early.get();
        if (ep.ok && ep.chunk == P.chunk && ep.cblock_in == P.cblock_in && ep.cgroup == P.cgroup) { perm.swap(ep.perm); have = true; }
    }
    if (!have && !build_tile_perm(P, cp, dp, perm, perr)) return fail(c, QS_ERR_STATE, perr);
    auto T_of = [](uint32_t cc) { return (cc + 7) / 8; };
    const uint32_t cmax = d_hi >= 2 ? d_hi - 2 : 0;
    const uint32_t Tmax = T_of(cmax);
    const uint32_t cblock = c->tile_cblock ? c->tile_cblock : cmax + 1;
    // Off unless asked for (QS_TUNE_COOP = 1): measured on MI355X the real barrier per 32-tree step costs more than the
    // shared loads save (512 taxa x 10000 trees: 368 ms against 354 ms; profiles/r03_experiments.md)
    if (c->tune_coop == 1) {
        // Cooperative launch order: same nesting ((a,b)-major: b-block, chunk of a-block pairs, c-block, d-block), but
        // innermost FOUR consecutive c of one a-block pair -- one workgroup of count_bitslice4_kernel. A group short of
        // four valid c is filled with shadow copies of its first tile.
        std::vector<uint32_t> coop, rest;
        coop.reserve(total + total / 8);
        for (uint32_t Bk = 1; Bk < Tmax; ++Bk) {
            const uint32_t base = (Bk * Bk) / 4;
            const uint32_t nj = ((Bk + 1) * (Bk + 1)) / 4 - base;     // tiles under this b-block; the last one lacks a2 when Bk is odd
            const uint32_t nj2 = Bk / 2;                              // pairs (2j, 2j+1) with 2j+1 < Bk
            const uint32_t c_lo = std::max(2u, 8 * Bk + 1);
            for (uint32_t j0 = 0; j0 < nj2; j0 += chunk) {
                const uint32_t j1 = std::min(nj2, j0 + chunk);
                for (uint32_t cb = c_lo; cb <= cmax; cb += cblock)
                    for (uint32_t k = 0; k < n_dblk; ++k) {
                        const uint32_t d1 = d_hi - k * kDB;
                        for (uint32_t j = j0; j < j1; ++j)
                            for (uint32_t c4 = cb; c4 < cb + cblock && c4 + 1 < d1; c4 += 4) {
                                const uint32_t first = dp[k] + cp[c4] + base + j;
                                for (uint32_t cc = c4; cc < c4 + 4; ++cc)
                                    coop.push_back((cc < cb + cblock && cc + 1 < d1) ? dp[k] + cp[cc] + base + j : (first | 0x80000000u));
                            }
                    }
            }
            if (nj > nj2)                                            // the tile with a single a-block
                for (uint32_t k = 0; k < n_dblk; ++k) {
                    const uint32_t d1 = d_hi - k * kDB;
                    for (uint32_t cc = c_lo; cc + 1 < d1; ++cc) rest.push_back(dp[k] + cp[cc] + base + nj2);
                }
        }
        for (uint32_t kd = 0; kd < (Tmax + 1) / 2; ++kd)
            for (uint32_t k = 0; k < n_dblk; ++k) {
                const uint32_t d1 = d_hi - k * kDB;
                for (uint32_t cc = 2; cc + 1 < d1; ++cc) {
                    const uint32_t T = T_of(cc);
                    if (kd < (T + 1) / 2) rest.push_back(dp[k] + cp[cc] + (T * T) / 4 + kd);
                }
            }
        {   // coop (without shadows) and rest together: every tile exactly once
            std::vector<uint8_t> seen(total, 0);
            size_t real = 0;
            auto take = [&](uint32_t id) { if (id >= total || seen[id]) return false; seen[id] = 1; ++real; return true; };
            for (uint32_t id : coop) if (!(id & 0x80000000u) && !take(id)) return fail(c, QS_ERR_STATE, "tile order: cooperative list is not a partition");
            for (uint32_t id : rest) if (!take(id)) return fail(c, QS_ERR_STATE, "tile order: rest list is not a partition");
            if (real != total || coop.size() % 4) return fail(c, QS_ERR_STATE, "tile order: cooperative + rest lists do not cover the tiling");
        }
        if (!coop.empty()) {
            if (c->perm_coop.reserve(coop.size() * 4, nullptr) != hipSuccess || c->perm_rest.reserve(std::max<size_t>(rest.size(), 1) * 4, nullptr) != hipSuccess)
                return fail(c, QS_ERR_OOM, "hipMalloc tile order (cooperative lists)");
            if (hipMemcpyAsync(c->perm_coop.get(), coop.data(), coop.size() * 4, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
                (!rest.empty() && hipMemcpyAsync(c->perm_rest.get(), rest.data(), rest.size() * 4, hipMemcpyHostToDevice, c->stream) != hipSuccess) ||
                hipStreamSynchronize(c->stream) != hipSuccess) return fail(c, QS_ERR_HIP, "memcpy tile order (cooperative lists)");
            c->n_coop = (uint32_t)coop.size(); c->n_rest = (uint32_t)rest.size();
        }
    }
    if (c->perm.reserve(perm.size() * 4, nullptr) != hipSuccess) return fail(c, QS_ERR_OOM, "hipMalloc tile order");
    if (hipMemcpyAsync(c->perm.get(), perm.data(), perm.size() * 4, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess) return fail(c, QS_ERR_HIP, "memcpy tile order");
    *out = c->perm.get();
    return QS_OK;
}

// The launch-order lists depend on the tile-order tuning and on QS_TUNE_COOP: dropped here, tile_order rebuilds them on next use.
static int drop_tile_order(qs_ctx *c) {
    QS_HIP(c, hipSetDevice(c->device));
    QS_HIP(c, hipStreamSynchronize(c->stream));
    c->perm.reset(); c->perm_coop.reset(); c->perm_rest.reset();
    c->perm_built = false; c->n_coop = c->n_rest = 0;
    c->split.d_mid = 0;   // (cut from the order just dropped)
    return QS_OK;
}

extern "C" int qs_set_tuning(qs_ctx *c, uint32_t key, uint64_t value) {
    if (c) c->log_valid = false;   // (the table / view / tuning may change: a logged pass 1 no longer describes it)
    if (!c) return QS_ERR_ARG;
    switch (key) {
        case QS_TUNE_SCORE_CAND_SLOTS:
            if (value < 1 || value > (uint64_t)kCand) return fail(c, QS_ERR_ARG, "qs_set_tuning: QS_TUNE_SCORE_CAND_SLOTS takes 1..8");
            c->tune_cand_slots = (uint32_t)value; return QS_OK;
        case QS_TUNE_SCORE_KERNEL:
            if (value > 1) return fail(c, QS_ERR_ARG, "qs_set_tuning: QS_TUNE_SCORE_KERNEL takes 0 (bundle kernel) or 1 (scan kernel)");
            c->tune_score_kernel = (int)value; return QS_OK;
        case QS_TUNE_SCORE_TOL_EXP:
            if (value < 1 || value > 15) return fail(c, QS_ERR_ARG, "qs_set_tuning: QS_TUNE_SCORE_TOL_EXP takes 1..15 (tolerance 10^-value)");
            c->tune_score_tol = std::pow(10.0, -(double)value); return QS_OK;
        case QS_TUNE_TILE_ORDER:
            if (int rc = drop_tile_order(c)) return rc;
            c->tile_chunk = (uint32_t)(value & 0xFFFF); c->tile_cblock = (uint32_t)((value >> 16) & 0xFFFF); c->tile_cgroup = (uint32_t)((value >> 32) & 0xFF);
            return QS_OK;
        case QS_TUNE_PANEL_SLICE_BYTES: c->tune_slice_bytes = value; return QS_OK;
        case QS_TUNE_TABLE_TREES: c->table_trees_hint = value; return QS_OK;
        case QS_TUNE_SCORE_SAMPLE: {
            const uint64_t S = value & 0xFFFFu;
            if (value >> 17 || (value && (S < 2 || (S & (S - 1))))) return fail(c, QS_ERR_ARG, "qs_set_tuning: QS_TUNE_SCORE_SAMPLE takes 0 or a power of two in [2, 32768], optionally | 65536 (whole rounds)");
            c->tune_score_sample = (uint32_t)value; return QS_OK;
        }
        case QS_TUNE_CLASS_MIN_TREES: c->tune_class_min = (uint32_t)std::min<uint64_t>(value, 0xFFFFFFFFull); return QS_OK;
        case QS_TUNE_DEPTH_CLAMP: c->tune_clamp_ppm = (uint32_t)std::min<uint64_t>(value, 1000000ull); return QS_OK;
        case QS_TUNE_FUSE_CLASSES: c->tune_fuse = value ? 1u : 0u; return QS_OK;
        case QS_TUNE_FIX_OVERLAP: c->tune_fix_overlap = value ? 1u : 0u; return QS_OK;
        case QS_TUNE_FIX_SPLIT_AT:
            if (value > c->n) return fail(c, QS_ERR_ARG, "qs_set_tuning: QS_TUNE_FIX_SPLIT_AT takes 0 (planned) or a largest id up to n_taxa");
            c->tune_fix_split_at = (uint32_t)value; return QS_OK;
        case QS_TUNE_CLASS_PCT: if (value > 100) return fail(c, QS_ERR_ARG, "qs_set_tuning: QS_TUNE_CLASS_PCT takes 0 .. 100"); c->tune_class_pct = (uint32_t)value; return QS_OK;
        case QS_TUNE_SCORE_LOAD:
            if (value > 3) return fail(c, QS_ERR_ARG, "qs_set_tuning: QS_TUNE_SCORE_LOAD takes 0 .. 3");
            c->tune_score_load = (uint32_t)value;
            c->bundle_r0[0] = c->bundle_r0[1] = c->bundle_r1[0] = c->bundle_r1[1] = ~0ull;   // the rounds are planned per wave count, which the load mode sets
            return QS_OK;
        case QS_TUNE_SCORE_DEDUPE: c->tune_score_dedupe = value ? 1u : 0u; return QS_OK;
        case QS_TUNE_SCORE_LOG_CAP:
            if (value > (1ull << 26)) return fail(c, QS_ERR_ARG, "qs_set_tuning: QS_TUNE_SCORE_LOG_CAP takes at most 2^26 records");
            c->tune_score_log_cap = value; return QS_OK;
        case QS_TUNE_SCORE_PASSES:
            if (value > 2) return fail(c, QS_ERR_ARG, "qs_set_tuning: QS_TUNE_SCORE_PASSES takes 0 (automatic), 1 (two passes) or 2 (single read)");
            c->tune_score_passes = (uint32_t)value; return QS_OK;
        case QS_TUNE_COOP:
            if (value > 2) return fail(c, QS_ERR_ARG, "qs_set_tuning: QS_TUNE_COOP takes 0 (default: off), 1 (on) or 2 (off)");
            if (c->tune_coop != (uint32_t)value)
                if (int rc = drop_tile_order(c)) return rc;
            c->tune_coop = (uint32_t)value; return QS_OK;
        case QS_TUNE_GATHER_IMPL:
            if (value > QS_IMPL_BITSLICE) return fail(c, QS_ERR_ARG, "qs_set_tuning: QS_TUNE_GATHER_IMPL takes QS_IMPL_AUTO / _SWAR / _BITSLICE");
            c->tune_gather_impl = (uint32_t)value; return QS_OK;
        case QS_TUNE_PANEL_KERNEL:
            if (value > 1) return fail(c, QS_ERR_ARG, "qs_set_tuning: QS_TUNE_PANEL_KERNEL takes 0 (automatic) or 1 (general builder)");
            c->tune_panel_kernel = (uint32_t)value; return QS_OK;
        default: return fail(c, QS_ERR_ARG, "qs_set_tuning: unknown key");
    }
}

extern "C" int qs_create(qs_ctx **out, uint32_t n_taxa, uint32_t count_bits, uint32_t flags, int device, void *stream,
                         uint32_t d_lo, uint32_t d_hi) {
    if (!out) return fail(nullptr, QS_ERR_ARG, "qs_create: out is NULL");
    *out = nullptr;
    if (n_taxa < 4 || n_taxa > 4096) return fail(nullptr, QS_ERR_ARG, "qs_create: n_taxa must be in [4, 4096]");
    if (count_bits != 16 && count_bits != 32) return fail(nullptr, QS_ERR_ARG, "qs_create: count_bits must be 16 or 32");
    if (d_lo == 0 && d_hi == 0) d_hi = n_taxa;
    if (d_hi > n_taxa || d_lo >= d_hi) return fail(nullptr, QS_ERR_ARG, "qs_create: bad shard [d_lo, d_hi)");
    // Everything that needs no device first: the tile geometry and -- for large tilings, on a helper thread -- the launch order of the
    // binary tiling (build_tile_perm: ~25 ms at 512 taxa), so that in a fresh process it is computed while the first HIP call below
    // waits for the runtime to come up.
    qs_ctx *c = new qs_ctx();
    c->n = n_taxa; c->count_bits = count_bits; c->flags = flags; c->device = device;
    c->stream = (hipStream_t)stream;
    c->d_lo = d_lo; c->d_hi = d_hi;
    c->rank_lo = binom4(d_lo);
    c->n_tuples = binom4(d_hi) - binom4(d_lo);
    // tile geometry of the gather kernel
    std::vector<uint32_t> cp(n_taxa + 2, 0);
    for (uint32_t cc = 2; cc <= n_taxa; ++cc)
        cp[cc + 1] = cp[cc] + gather_tiles_for_c(cc);
    // note: cp[c] = tiles of all c' < c (c' >= 2)
    const uint32_t d_start = std::max(d_lo, 3u);
    c->n_dblk = d_hi > d_start ? (d_hi - d_start + kDB - 1) / kDB : 0;
    std::vector<uint32_t> dp(c->n_dblk + 1, 0);
    uint64_t tiles64 = 0;
    for (uint32_t k = 0; k < c->n_dblk; ++k) {
        uint32_t d0 = d_start + k * kDB, d1 = std::min(d0 + (uint32_t)kDB, d_hi);
        tiles64 += cp[d1 - 1]; // c in [2, d1-1)
        dp[k + 1] = (uint32_t)tiles64;
    }
    if (tiles64 >= (1ull << 31)) { delete c; return fail(nullptr, QS_ERR_UNSUPPORTED, "qs_create: shard too large for one launch; use a narrower [d_lo, d_hi)"); }
    c->total_tiles = dp[c->n_dblk];
    // the 16x8 tiles of count_bitslice3_kernel; block k = [max(d_start, d1 - 8), d1) with d1 = d_hi - 8k
    std::vector<uint32_t> cp3(n_taxa + 2, 0), dp3(c->n_dblk + 1, 0);
    {
        for (uint32_t cc = 2; cc <= n_taxa; ++cc) cp3[cc + 1] = cp3[cc] + bitslice3_tiles_for_c(cc);
        uint64_t t3 = 0;
        for (uint32_t k = 0; k < c->n_dblk; ++k) { t3 += cp3[d_hi - k * kDB - 1]; dp3[k + 1] = (uint32_t)t3; }
        if (t3 >= (1ull << 31)) { delete c; return fail(nullptr, QS_ERR_UNSUPPORTED, "qs_create: shard too large for one launch; use a narrower [d_lo, d_hi)"); }
        c->total_tiles3 = dp3[c->n_dblk];
        c->h_cp3 = cp3; c->h_dp3 = dp3;
    }
    if (c->total_tiles3 >= (1u << 20) && c->total_tiles3 <= (1u << 26) && c->tile_chunk) {
        const TilePermParams P{c->tile_chunk, c->tile_cblock, c->tile_cgroup, c->d_hi, c->n_dblk, c->total_tiles3};
        try {
            c->perm_early = std::async(std::launch::async, [P, cp3, dp3] {
                EarlyPerm ep; ep.chunk = P.chunk; ep.cblock_in = P.cblock_in; ep.cgroup = P.cgroup;
                std::string err;
                ep.ok = build_tile_perm(P, cp3, dp3, ep.perm, err);
                return ep;
            });
        } catch (...) { c->perm_early = std::future<EarlyPerm>(); }   // no thread to be had: tile_order builds it when asked
    }
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0) {
        delete c;   // (waits for the helper thread: a std::async future blocks in its destructor)
        return fail(nullptr, QS_ERR_NO_DEVICE,
                    "qs_create: no HIP device (this library has no CPU fallback; it needs a gfx950 GPU)");
    }
    if (device < 0 || device >= ndev) { delete c; return fail(nullptr, QS_ERR_ARG, "qs_create: bad device ordinal"); }
    if (hipSetDevice(device) != hipSuccess) { delete c; return fail(nullptr, QS_ERR_HIP, "qs_create: hipSetDevice"); }
    auto cleanup = [&](int code, const std::string &m) { qs_destroy(c); return fail(nullptr, code, m); };
    if (c->cprefix.reserve(cp.size() * 4, nullptr) != hipSuccess) return cleanup(QS_ERR_OOM, "hipMalloc cprefix");
    if (c->dprefix.reserve(dp.size() * 4, nullptr) != hipSuccess) return cleanup(QS_ERR_OOM, "hipMalloc dprefix");
    if (hipMemcpy(c->cprefix.get(), cp.data(), cp.size() * 4, hipMemcpyHostToDevice) != hipSuccess) return cleanup(QS_ERR_HIP, "memcpy cprefix");
    if (hipMemcpy(c->dprefix.get(), dp.data(), dp.size() * 4, hipMemcpyHostToDevice) != hipSuccess) return cleanup(QS_ERR_HIP, "memcpy dprefix");
    if (c->cprefix3.reserve(cp3.size() * 4, nullptr) != hipSuccess) return cleanup(QS_ERR_OOM, "hipMalloc cprefix3");
    if (c->dprefix3.reserve(dp3.size() * 4, nullptr) != hipSuccess) return cleanup(QS_ERR_OOM, "hipMalloc dprefix3");
    if (hipMemcpy(c->cprefix3.get(), cp3.data(), cp3.size() * 4, hipMemcpyHostToDevice) != hipSuccess) return cleanup(QS_ERR_HIP, "memcpy cprefix3");
    if (hipMemcpy(c->dprefix3.get(), dp3.data(), dp3.size() * 4, hipMemcpyHostToDevice) != hipSuccess) return cleanup(QS_ERR_HIP, "memcpy dprefix3");
    if (c->dev_flags.reserve(16, nullptr) != hipSuccess) return cleanup(QS_ERR_OOM, "hipMalloc flags");
    if (hipMemset(c->dev_flags.get(), 0, 16) != hipSuccess) return cleanup(QS_ERR_HIP, "memset flags");
    *out = c;
    return QS_OK;
}

// Every device and pinned buffer of the context is a DevBuf member and goes with `delete c`; what is left to do by hand is what
// has to happen before: wait for the copies out of the staging buffers, and release what the slab cache holds (BatchSlab is a
// plain struct shared with the launch code).
extern "C" void qs_destroy(qs_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    for (hipEvent_t e : c->evs) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->pin_ev) if (e) { (void)hipEventSynchronize(e); (void)hipEventDestroy(e); }
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    for (hipEvent_t e : c->score_ev) if (e) (void)hipEventDestroy(e);
    for (BatchSlab &sl : c->slabs) { (void)hipFree(sl.p); if (sl.last_use) (void)hipEventDestroy(sl.last_use); }
    delete c;
}

// Work the first qs_count_batch would otherwise do before its first launch, done ahead of time (the host calls this on its
// GPU-initialisation thread while the evaluation trees are still being parsed): the launch order of the bit-sliced count
// kernel for binary batches (12 M slots at 512 taxa: ~60 ms of host work + a 47 MB copy) and the pair-depth panel for a
// batch of n_trees_hint trees. Purely an optimisation: qs_count_batch builds whatever is missing. The reference does the
// equivalent set-up in the table's constructor (QuartetCounterLookup.hpp:245-273).
static size_t padded(size_t bytes) { return (bytes + 255) & ~(size_t)255; }   // the pieces of a staged batch start at 256-byte boundaries (Stager, below)
// pinned staging buffer `slot` holds `need` bytes, with a quarter to spare when it has to grow (nothing reads it then: the
// caller has waited for pin_ev[slot], or it has never been used)
static hipError_t ensure_pinned(qs_ctx *c, int slot, size_t need) {
    return c->pin[slot].bytes() >= need ? hipSuccess : c->pin[slot].reserve(need + need / 4 + 4096, nullptr);
}
static int prepare_staging(qs_ctx *c, uint64_t n_trees_hint);
extern "C" int qs_prepare(qs_ctx *c, uint64_t n_trees_hint) {
    if (!c) return QS_ERR_ARG;
    QS_HIP(c, hipSetDevice(c->device));
    // the staging allocations (two pinned buffers + a device slab: ~10 ms) on a helper thread beside the launch order (~15 ms of
    // host work): they touch different members of the context
    std::thread staging;
    if (n_trees_hint) {
        try { staging = std::thread([c, n_trees_hint] { (void)prepare_staging(c, n_trees_hint); }); }
        catch (...) { (void)prepare_staging(c, n_trees_hint); }   // (no thread to be had: do it here; nothing throws across the C boundary)
    }
    struct Join { std::thread &t; ~Join() { if (t.joinable()) t.join(); } } join_staging{staging};
    const uint32_t *order = nullptr;
    int rc = tile_order(c, &order);
    if (rc != QS_OK) return rc;
    if (n_trees_hint && !c->panel) {   // (no stream to wait for: there is no panel yet)
        const size_t group_bytes = (size_t)binom2(c->n) * 5 * 4;   // 5 planes: the common depth class
        const uint32_t groups = slice_groups(c, group_bytes, (uint32_t)std::min<uint64_t>((n_trees_hint + 31) / 32, 1u << 20), order != nullptr);
        if (c->panel.reserve((size_t)groups * group_bytes, nullptr) != hipSuccess) (void)hipGetLastError();   // not fatal here: the count reports it if it persists
    }
    return QS_OK;
}
static int prepare_staging(qs_ctx *c, uint64_t n_trees_hint) {
    if (hipSetDevice(c->device) != hipSuccess) { (void)hipGetLastError(); return QS_ERR_HIP; }
    {
        // both pinned staging buffers and one device slab for batches of that many full trees (qs_batch_upload's Stager
        // would allocate them on first use: hipHostMalloc + hipMalloc, tens of ms in front of the first count)
        const uint64_t nt = std::min<uint64_t>(n_trees_hint, 1u << 22);
        const size_t need = padded(((size_t)nt + 1) * 4) + 2 * padded((size_t)nt * c->n * 2) + padded((size_t)nt * 4);
        if (!c->copy_stream && hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking) != hipSuccess) { c->copy_stream = nullptr; (void)hipGetLastError(); return QS_ERR_HIP; }
        for (int slot = 0; slot < 2; ++slot)
            if (ensure_pinned(c, slot, need) != hipSuccess) (void)hipGetLastError();   // (the first upload asks again and reports it)
        bool have = false;
        for (const BatchSlab &sl : c->slabs) have = have || sl.cap >= need;
        if (!have && c->slabs.size() < 4) {
            BatchSlab sl;
            sl.cap = need + need / 4;
            if (hipMalloc(&sl.p, sl.cap) == hipSuccess) c->slabs.push_back(sl); else (void)hipGetLastError();
        }
    }
    // first use of the count kernels' code object (~5 ms of loading on MI355X: tools/modload_probe.py) here, beside the launch
    // order, instead of in front of the first count: one lookup of the quartet {0,1,2,3} on the copy stream
    if (c->table && c->n >= 4 && c->d_lo == 0) {
        DevBuf<char> scratch;
        if (scratch.reserve(64, nullptr) == hipSuccess) {
            const uint16_t ids[4] = {0, 1, 2, 3};
            if (hipMemcpyAsync(scratch.get(), ids, sizeof ids, hipMemcpyHostToDevice, c->copy_stream) == hipSuccess)
                (void)launch_lookup(c->copy_stream, c->n, c->d_lo, c->d_hi, c->rank_lo, c->table, (int)c->count_bits, 1, (const uint16_t *)scratch.get(),
                                    (uint64_t *)(scratch.get() + 16));
            (void)hipStreamSynchronize(c->copy_stream);
        }
        (void)hipGetLastError();
    }
    // the correction stream of split slices (QS_TUNE_FIX_OVERLAP) with its hardware queue, which the runtime opens with the stream's
    // first work: here instead of inside the first count
    if (c->tune_fix_overlap && c->fix_stream.ensure() == hipSuccess) {
        DevBuf<char> word;
        if (word.reserve(64, nullptr) == hipSuccess && hipMemsetAsync(word.get(), 0, 64, c->fix_stream.get()) == hipSuccess)
            (void)hipStreamSynchronize(c->fix_stream.get());
    }
    (void)hipGetLastError();
    return QS_OK;
}

// ---- table -------------------------------------------------------------------------------

extern "C" uint64_t qs_table_tuples(const qs_ctx *c) { return c ? c->n_tuples : 0; }
extern "C" uint64_t qs_table_bytes(const qs_ctx *c) { return c ? c->n_tuples * 3 * (c->count_bits / 8) : 0; }
extern "C" void *qs_table_device_ptr(const qs_ctx *c) { return c ? c->table : nullptr; }
extern "C" uint64_t qs_trees_counted(const qs_ctx *c) { return c ? c->trees_counted : 0; }

extern "C" int qs_table_alloc(qs_ctx *c) {
    if (c) c->log_valid = false;   // (the table / view / tuning may change: a logged pass 1 no longer describes it)
    if (!c) return QS_ERR_ARG;
    QS_HIP(c, hipSetDevice(c->device));
    if (c->table_mem) { c->table_mem.reset(); c->table = nullptr; }
    size_t bytes = (size_t)qs_table_bytes(c);
    size_t freeb = 0, total = 0;
    QS_HIP(c, hipMemGetInfo(&freeb, &total));
    if (bytes + (64u << 20) > freeb) return fail(c, QS_ERR_OOM, "Insufficient memory!");
    if (c->table_mem.reserve(bytes + 16, nullptr) != hipSuccess) { c->table = nullptr; return fail(c, QS_ERR_OOM, "Insufficient memory!"); }
    c->table = c->table_mem.get();
    c->trees_counted = 0;
    QS_HIP(c, hipMemsetAsync(c->table, 0, bytes + 16, c->stream));
    return QS_OK;
}

extern "C" int qs_table_attach(qs_ctx *c, void *device_ptr, uint64_t bytes) {
    if (c) c->log_valid = false;   // (the table / view / tuning may change: a logged pass 1 no longer describes it)
    if (!c) return QS_ERR_ARG;
    if (!device_ptr) {
        // detach: the caller takes its buffer back (e.g. to free a full table once its reduce-scattered shard is the scoring view)
        if (bytes != 0) return fail(c, QS_ERR_ARG, "qs_table_attach: NULL pointer with a size (detach = NULL, 0)");
        if (c->table_mem) return fail(c, QS_ERR_STATE, "qs_table_attach: detach of a table the context owns (qs_table_alloc)");
        QS_HIP(c, hipSetDevice(c->device));
        QS_HIP(c, hipStreamSynchronize(c->stream));   // nothing of this context may still be writing the buffer
        c->table = nullptr;
        return QS_OK;
    }
    // 16-bit cells are updated through their 32-bit word (packed half-word atomics of the scatter kernel, word-wise
    // collectives): the buffer must cover whole words
    const uint64_t need = (qs_table_bytes(c) + 3) & ~3ull;
    if (bytes < need) return fail(c, QS_ERR_ARG, "qs_table_attach: buffer smaller than qs_table_bytes() rounded up to a multiple of 4");
    if ((uintptr_t)device_ptr & 3) return fail(c, QS_ERR_ARG, "qs_table_attach: pointer must be 4-byte aligned");
    c->table_mem.reset();   // (the context's own table, if it had one)
    c->table = device_ptr;
    return QS_OK;
}

extern "C" int qs_table_clear(qs_ctx *c) {
    if (c) c->log_valid = false;   // (the table / view / tuning may change: a logged pass 1 no longer describes it)
    if (!c || !c->table) return fail(c, QS_ERR_STATE, "qs_table_clear: no table");
    QS_HIP(c, hipSetDevice(c->device));
    QS_HIP(c, hipMemsetAsync(c->table, 0, (size_t)qs_table_bytes(c), c->stream));
    c->trees_counted = 0;
    return QS_OK;
}

extern "C" int qs_table_download(qs_ctx *c, void *host_dst, uint64_t bytes) {
    if (!c || !c->table) return fail(c, QS_ERR_STATE, "qs_table_download: no table");
    if (bytes > qs_table_bytes(c)) return fail(c, QS_ERR_ARG, "qs_table_download: too many bytes");
    QS_HIP(c, hipSetDevice(c->device));
    QS_HIP(c, hipMemcpyAsync(host_dst, c->table, (size_t)bytes, hipMemcpyDeviceToHost, c->stream));
    QS_HIP(c, hipStreamSynchronize(c->stream));
    return QS_OK;
}

extern "C" int qs_table_upload(qs_ctx *c, const void *host_src, uint64_t bytes) {
    if (c) c->log_valid = false;   // (the table / view / tuning may change: a logged pass 1 no longer describes it)
    if (!c || !c->table) return fail(c, QS_ERR_STATE, "qs_table_upload: no table");
    if (bytes > qs_table_bytes(c)) return fail(c, QS_ERR_ARG, "qs_table_upload: too many bytes");
    QS_HIP(c, hipSetDevice(c->device));
    QS_HIP(c, hipMemcpyAsync(c->table, host_src, (size_t)bytes, hipMemcpyHostToDevice, c->stream));
    QS_HIP(c, hipStreamSynchronize(c->stream));
    return QS_OK;
}

extern "C" int qs_table_pack16(qs_ctx *c, void *dst_device, uint64_t dst_bytes) {
    if (!c || !c->table || !dst_device) return fail(c, QS_ERR_STATE, "qs_table_pack16: no table / NULL destination");
    if (c->count_bits != 32) return fail(c, QS_ERR_ARG, "qs_table_pack16: the table already has 16-bit cells");
    const uint64_t cells = c->n_tuples * 3, need = ((cells + 1) / 2) * 4;
    if (dst_bytes < need) return fail(c, QS_ERR_ARG, "qs_table_pack16: destination smaller than " + std::to_string(need) + " bytes");
    QS_HIP(c, hipSetDevice(c->device));
    QS_HIP(c, launch_pack16(c->stream, c->table, dst_device, cells, c->dev_flags.get()));
    return QS_OK;
}

extern "C" int qs_wire_attach(qs_ctx *c, void *dst_device, uint64_t dst_bytes) {
    if (c) c->log_valid = false;   // (the table / view / tuning may change: a logged pass 1 no longer describes it)
    if (!c) return QS_ERR_ARG;
    if (!dst_device) { c->wire_out = nullptr; c->wire_trees = 0; return QS_OK; }
    if (dst_bytes < c->n_tuples * 4) return fail(c, QS_ERR_ARG, "qs_wire_attach: destination smaller than " + std::to_string(c->n_tuples * 4) + " bytes");
    c->wire_out = (uint32_t *)dst_device;
    c->wire_trees = 0;
    return QS_OK;
}

extern "C" int qs_table_pack16x2(qs_ctx *c, void *dst_device, uint64_t dst_bytes) {
    if (!c || !c->table || !dst_device) return fail(c, QS_ERR_STATE, "qs_table_pack16x2: no table / NULL destination");
    if (c->count_bits != 32) return fail(c, QS_ERR_ARG, "qs_table_pack16x2: needs a 32-bit table");
    if (c->trees_counted > 0xFFFFull) return fail(c, QS_ERR_OVERFLOW, "qs_table_pack16x2: more than 65535 trees counted");
    if (dst_bytes < c->n_tuples * 4) return fail(c, QS_ERR_ARG, "qs_table_pack16x2: destination smaller than " + std::to_string(c->n_tuples * 4) + " bytes");
    QS_HIP(c, hipSetDevice(c->device));
    QS_HIP(c, launch_pack16x2(c->stream, c->table, dst_device, c->n_tuples, (uint32_t)c->trees_counted, c->dev_flags.get(), c->dev_flags.get() + 3));
    return QS_OK;
}

extern "C" int qs_unpack16x2(qs_ctx *c, const void *src_device, uint64_t n_tuples, uint32_t total_trees, void *dst_device) {
    if (c) c->log_valid = false;   // (the table / view / tuning may change: a logged pass 1 no longer describes it)
    if (!c || !src_device || !dst_device) return fail(c, QS_ERR_ARG, "qs_unpack16x2: NULL argument");
    if (total_trees > 0xFFFFu) return fail(c, QS_ERR_OVERFLOW, "qs_unpack16x2: more than 65535 trees");
    QS_HIP(c, hipSetDevice(c->device));
    QS_HIP(c, launch_unpack16x2(c->stream, src_device, dst_device, n_tuples, total_trees, c->dev_flags.get() + 3));
    return QS_OK;
}

// Two-cell wire format with 32-bit cells: (n0, n1) per tuple, for batches of binary trees holding all taxa whose total
// over the ranks reaches 65536 trees (8 bytes per quartet on the wire instead of 12).
extern "C" int qs_table_pack32x2(qs_ctx *c, void *dst_device, uint64_t dst_bytes) {
    if (!c || !c->table || !dst_device) return fail(c, QS_ERR_STATE, "qs_table_pack32x2: no table / NULL destination");
    if (c->count_bits != 32) return fail(c, QS_ERR_ARG, "qs_table_pack32x2: needs a 32-bit table");
    if (c->trees_counted > 0xFFFFFFFFull) return fail(c, QS_ERR_OVERFLOW, "qs_table_pack32x2: more than 2^32 - 1 trees counted");
    if (dst_bytes < c->n_tuples * 8) return fail(c, QS_ERR_ARG, "qs_table_pack32x2: destination smaller than " + std::to_string(c->n_tuples * 8) + " bytes");
    QS_HIP(c, hipSetDevice(c->device));
    QS_HIP(c, launch_pack32x2(c->stream, c->table, dst_device, c->n_tuples, (uint32_t)c->trees_counted, c->dev_flags.get() + 3));
    return QS_OK;
}

extern "C" int qs_unpack32x2(qs_ctx *c, const void *src_device, uint64_t n_tuples, uint64_t total_trees, void *dst_device) {
    if (c) c->log_valid = false;   // (the table / view / tuning may change: a logged pass 1 no longer describes it)
    if (!c || !src_device || !dst_device) return fail(c, QS_ERR_ARG, "qs_unpack32x2: NULL argument");
    if (total_trees > 0xFFFFFFFFull) return fail(c, QS_ERR_OVERFLOW, "qs_unpack32x2: more than 2^32 - 1 trees");
    QS_HIP(c, hipSetDevice(c->device));
    QS_HIP(c, launch_unpack32x2(c->stream, src_device, dst_device, n_tuples, (uint32_t)total_trees, c->dev_flags.get() + 3));
    return QS_OK;
}

extern "C" int qs_sum_words(qs_ctx *c, void *dst_device, const void *const *src_device, uint32_t n_src, uint64_t n_words) {
    if (c) c->log_valid = false;   // (a table may change under a logged pass 1)
    if (!c || (n_words && n_src && (!dst_device || !src_device))) return fail(c, QS_ERR_ARG, "qs_sum_words: NULL argument");
    if (n_src > 15) return fail(c, QS_ERR_ARG, "qs_sum_words: at most 15 sources");
    if ((uintptr_t)dst_device & 15) return fail(c, QS_ERR_ARG, "qs_sum_words: the destination must be 16-byte aligned");
    for (uint32_t k = 0; k < n_src; ++k)
        if (!src_device[k] || ((uintptr_t)src_device[k] & 15)) return fail(c, QS_ERR_ARG, "qs_sum_words: sources must be non-NULL and 16-byte aligned");
    QS_HIP(c, hipSetDevice(c->device));
    if (c->n_cu == 0) { int v = 0; QS_HIP(c, hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, c->device)); c->n_cu = std::max(1, v); }
    QS_HIP(c, launch_sum_words(c->stream, dst_device, src_device, n_src, n_words, c->n_cu));
    return QS_OK;   // asynchronous on the context's stream
}

// qs_table_remap (subset = false: a permutation of the same taxa, qs_remap.hip) and qs_table_restrict (subset = true: an injective
// map of dst's taxa into src's, qs_restrict.hip) differ in what they ask of the taxon counts and the id map and in the kernel they launch.
static int table_reindex(qs_ctx *dst, const qs_ctx *src, const uint16_t *src_id_of, bool subset) {
    const std::string fn = subset ? "qs_table_restrict: " : "qs_table_remap: ";
    if (dst) dst->log_valid = false;   // (the table changes: a logged pass 1 no longer describes it)
    if (!dst) return QS_ERR_ARG;
    if (!src || !src_id_of) return fail(dst, QS_ERR_ARG, fn + "NULL argument");
    if (dst == src) return fail(dst, QS_ERR_ARG, fn + "source and destination are the same context");
    if (dst->d_lo != 0 || dst->d_hi != dst->n || src->d_lo != 0 || src->d_hi != src->n)
        return fail(dst, QS_ERR_UNSUPPORTED, fn + "whole-table contexts only (no table shards)");
    if (subset ? dst->n > src->n : dst->n != src->n)
        return fail(dst, QS_ERR_ARG, fn + (subset ? "the destination has more taxa than the source" : "the contexts have different numbers of taxa"));
    if (dst->device != src->device) return fail(dst, QS_ERR_ARG, fn + "the contexts are on different devices");
    if (!dst->table || !src->table) return fail(dst, QS_ERR_STATE, fn + "the " + (src->table ? "destination" : "source") + " has no table");
    if (dst->table == src->table) return fail(dst, QS_ERR_ARG, fn + "source and destination share their table");
    if (dst->count_bits < src->count_bits) return fail(dst, QS_ERR_ARG, fn + "32-bit cells cannot be narrowed to 16 bits");
    std::vector<uint8_t> seen(src->n, 0);
    bool monotone = true;   // strictly increasing: the source ids of a destination 4-set are sorted as they come
    for (uint32_t i = 0; i < dst->n; ++i) {
        if (src_id_of[i] >= src->n || seen[src_id_of[i]])
            return fail(dst, QS_ERR_ARG, fn + (subset ? "src_id_of is not injective into [0, n_taxa of the source)" : "src_id_of is not a permutation of [0, n_taxa)"));
        seen[src_id_of[i]] = 1;
        if (i && src_id_of[i] < src_id_of[i - 1]) monotone = false;
    }
    QS_HIP(dst, hipSetDevice(dst->device));
    QS_HIP(dst, dst->remap_ids.reserve(4096 * sizeof(uint16_t), nullptr));
    if (src->stream != dst->stream) {   // the source's counting (or upload) first
        hipEvent_t ev = nullptr;
        QS_HIP(dst, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        hipError_t e = hipEventRecord(ev, src->stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(dst->stream, ev, 0);
        (void)hipEventDestroy(ev);
        QS_HIP(dst, e);
    }
    QS_HIP(dst, hipMemcpyAsync(dst->remap_ids.get(), src_id_of, dst->n * sizeof(uint16_t), hipMemcpyHostToDevice, dst->stream));
    if (subset)
        QS_HIP(dst, launch_table_restrict(dst->stream, src->table, (int)src->count_bits, dst->table, (int)dst->count_bits, dst->remap_ids.get(), dst->n, dst->n_tuples, monotone));
    else
        QS_HIP(dst, launch_table_remap(dst->stream, src->table, (int)src->count_bits, dst->table, (int)dst->count_bits, dst->remap_ids.get(), dst->n, dst->n_tuples));
    dst->trees_counted = src->trees_counted;   // sizes the log table and the 16-bit overflow guard of later counts
    return QS_OK;   // asynchronous on dst's stream
}

// The table of `src` in the lookup-id order of another reference tree over the same taxa (qs_remap.hip), so that one count
// serves several reference trees. The reference recounts per run: this replaces nothing there.
extern "C" int qs_table_remap(qs_ctx *dst, const qs_ctx *src, const uint16_t *src_id_of) { return table_reindex(dst, src, src_id_of, false); }

// The table of `src` over a subset of its taxa, in any id order (qs_restrict.hip): the table of the problem without the other taxa,
// because what a tree displays for a 4-set does not depend on its other taxa (a tree pruned below four taxa still counts towards
// trees-counted; scores never depend on it). The reference rejects a leaf it does not know and recounts per run: this replaces
// nothing there.
extern "C" int qs_table_restrict(qs_ctx *dst, const qs_ctx *src, const uint16_t *src_id_of) { return table_reindex(dst, src, src_id_of, true); }

// Per-tree quartet agreement of a batch with the reference tree (qs_agree.hip). The reference's links come from its depth-first id
// order: the children of an inner node split its id interval, ordered by their first id, and its parent link holds the other ids.
// The reference has no per-tree output: this replaces nothing there.
static int agree_ref_upload(qs_ctx *c, const qs_ref_tree *ref) {
    if (!ref || !ref->parent || !ref->leaf_node) return fail(c, QS_ERR_ARG, "qs_tree_agreement: NULL reference arrays");
    if (ref->n_taxa != c->n) return fail(c, QS_ERR_ARG, "qs_tree_agreement: the reference tree's n_taxa differs from the context");
    const uint32_t N = ref->n_nodes, n = ref->n_taxa;
    if (c->agree_off && c->agree_parent.size() == N && c->agree_leaf_node.size() == n &&
        memcmp(c->agree_parent.data(), ref->parent, (size_t)N * 4) == 0 && memcmp(c->agree_leaf_node.data(), ref->leaf_node, (size_t)n * 4) == 0)
        return QS_OK;
    RefHost R;
    if (int rc = build_ref_shape(c, ref, R)) return rc;
    // children of every node in id order
    std::vector<std::vector<uint32_t>> kids(N);
    for (uint32_t v = 0; v < N; ++v)
        if (R.parent[v] >= 0 && R.leaf_cnt[v]) kids[R.parent[v]].push_back(v);
    std::vector<uint32_t> off{0};
    std::vector<uint16_t> bnd;
    std::vector<uint8_t> par;
    for (uint32_t u = 0; u < N; ++u) {
        std::vector<uint32_t> &ks = kids[u];
        const uint32_t has_parent = R.parent[u] >= 0 ? 1u : 0u;
        if (ks.size() + has_parent < 3) continue;
        std::sort(ks.begin(), ks.end(), [&](uint32_t x, uint32_t y) { return R.leaf_lo[x] < R.leaf_lo[y]; });
        for (uint32_t v : ks) bnd.push_back((uint16_t)R.leaf_lo[v]);
        bnd.push_back((uint16_t)(R.leaf_lo[ks.back()] + R.leaf_cnt[ks.back()]));
        off.push_back((uint32_t)bnd.size());
        par.push_back((uint8_t)has_parent);
    }
    QS_HIP(c, hipSetDevice(c->device));
    QS_HIP(c, hipStreamSynchronize(c->stream));   // kernels of this context may still read the previous tree's arrays
    // The cache key goes BEFORE the first buffer: whatever fails below, the next call finds no tree cached and builds all three anew.
    c->agree_parent.clear(); c->agree_leaf_node.clear();
    c->agree_off.reset(); c->agree_bnd.reset(); c->agree_par.reset();   // (each tree gets arrays of its own size, as before)
    QS_HIP(c, c->agree_off.reserve(off.size() * 4, nullptr));
    QS_HIP(c, c->agree_bnd.reserve(std::max<size_t>(bnd.size(), 1) * 2, nullptr));
    QS_HIP(c, c->agree_par.reserve(std::max<size_t>(par.size(), 1), nullptr));
    QS_HIP(c, hipMemcpy(c->agree_off.get(), off.data(), off.size() * 4, hipMemcpyHostToDevice));
    if (!bnd.empty()) QS_HIP(c, hipMemcpy(c->agree_bnd.get(), bnd.data(), bnd.size() * 2, hipMemcpyHostToDevice));
    if (!par.empty()) QS_HIP(c, hipMemcpy(c->agree_par.get(), par.data(), par.size(), hipMemcpyHostToDevice));
    c->agree_n_u = (uint32_t)par.size();
    c->agree_parent.assign(ref->parent, ref->parent + N);
    c->agree_leaf_node.assign(ref->leaf_node, ref->leaf_node + n);
    return QS_OK;
}

extern "C" int qs_tree_agreement(qs_ctx *c, const qs_ref_tree *ref, const qs_device_batch *b, uint64_t *dst_device) {
    if (!c) return QS_ERR_ARG;
    if (!b || !dst_device) return fail(c, QS_ERR_ARG, "qs_tree_agreement: NULL argument");
    if (c->d_lo != 0 || c->d_hi != c->n)
        return fail(c, QS_ERR_UNSUPPORTED, "qs_tree_agreement: whole-table contexts only (no table shards)");
    if (reinterpret_cast<uintptr_t>(dst_device) % 8) return fail(c, QS_ERR_ARG, "qs_tree_agreement: dst_device is not 8-byte aligned");
    if (int rc = agree_ref_upload(c, ref)) return rc;
    const DeviceBatch &d = b->d;
    if (d.n_trees && !d.node_off) return fail(c, QS_ERR_STATE, "qs_tree_agreement: the batch was uploaded without node ranges");
    QS_HIP(c, hipSetDevice(c->device));
    if (d.ready) QS_HIP(c, hipStreamWaitEvent(c->stream, d.ready, 0));
    QS_HIP(c, launch_tree_agree(c->stream, d, c->n, d.max_tree_nodes, c->agree_off.get(), c->agree_bnd.get(), c->agree_par.get(), c->agree_n_u,
                                reinterpret_cast<unsigned long long *>(dst_device)));
    return QS_OK;   // asynchronous on the context's stream
}

// ---- issue probe: how fast does THIS device run the count kernel's instruction mix? ------------------------------------
// MI355X devices of one pool differ by several per cent in the clock they hold under a VALU-dense load (the guide measures up
// to 12 % between devices), more than a round of kernel work moves the headline. The probe runs the bare slot of the hot
// instance at B = 5 -- two magnitude comparisons of 6 planes sharing one operand (24 v_bitop3) + 4 v_bcnt with accumulate, all
// operands in registers -- at 4 waves per SIMD on every CU and returns nanoseconds per wave instruction and SIMD, the figure
// profiles/r03_valu_yardstick.txt calls the slot's cost (1.39-1.40 ns on the boxes it was written on). bench.py prints it
// beside its line so that lines from different boxes can be compared.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void issue_probe_kernel(const uint32_t *__restrict__ seed, uint32_t *__restrict__ out, uint32_t iters) {
    uint32_t l1[6], l2[6], r[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        l1[k] = seed[(threadIdx.x * 19u + k) & 1023u];
        l2[k] = seed[(threadIdx.x * 23u + k + 6) & 1023u];
        r[k] = seed[(threadIdx.x * 29u + k + 12) & 1023u];
    }
    uint32_t g1 = 0, t1 = 0, g2 = 0, t2 = 0, c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    for (uint32_t it = 0; it < iters; ++it) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int k = 0; k < 6; ++k) {       // the truth tables of cmp_planes (qs_count.hip): greater-than / less-than steps
                g1 = __builtin_amdgcn_bitop3_b32(l1[k], r[(k + u) % 6], g1, 0xb2);
                t1 = __builtin_amdgcn_bitop3_b32(l1[k], r[(k + u) % 6], t1, 0x8e);
                g2 = __builtin_amdgcn_bitop3_b32(l2[k], r[(k + u) % 6], g2, 0xb2);
                t2 = __builtin_amdgcn_bitop3_b32(l2[k], r[(k + u) % 6], t2, 0x8e);
            }
            c0 += (uint32_t)__builtin_popcount(g1); c1 += (uint32_t)__builtin_popcount(t1);
            c2 += (uint32_t)__builtin_popcount(g2); c3 += (uint32_t)__builtin_popcount(t2);
        }
    }
    out[blockIdx.x * blockDim.x + threadIdx.x] = c0 ^ c1 ^ c2 ^ c3;
}

extern "C" int qs_issue_probe(qs_ctx *c, uint32_t iterations, float *ns_per_instruction) {
    if (!c || !ns_per_instruction || iterations == 0) return fail(c, QS_ERR_ARG, "qs_issue_probe: bad argument");
    QS_HIP(c, hipSetDevice(c->device));
    if (c->n_cu == 0) { int v = 0; QS_HIP(c, hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, c->device)); c->n_cu = std::max(1, v); }
    const uint32_t blocks = (uint32_t)c->n_cu * 4u;              // 4 workgroups of 4 waves per CU = 4 waves per SIMD
    DevBuf<uint32_t> mem;
    QS_HIP(c, mem.reserve((1024 + (size_t)blocks * 256) * 4, nullptr));
    uint32_t *const buf = mem.get();
    std::vector<uint32_t> host(1024);
    uint32_t x = 0x9E3779B9u;
    for (uint32_t &w : host) { x ^= x << 13; x ^= x >> 17; x ^= x << 5; w = x; }   // random operands: all-zero words let the clock rise
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t e = hipMemcpyAsync(buf, host.data(), 4096, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    float ms = 0.f;
    if (e == hipSuccess) {
        hipLaunchKernelGGL(issue_probe_kernel, dim3(blocks), dim3(256), 0, c->stream, buf, buf + 1024, iterations);   // warm-up: clocks, code object
        e = hipEventRecord(e0, c->stream);
        if (e == hipSuccess) { hipLaunchKernelGGL(issue_probe_kernel, dim3(blocks), dim3(256), 0, c->stream, buf, buf + 1024, iterations); e = hipGetLastError(); }
        if (e == hipSuccess) e = hipEventRecord(e1, c->stream);
        if (e == hipSuccess) e = hipEventSynchronize(e1);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (e != hipSuccess) return fail(c, QS_ERR_HIP, std::string("qs_issue_probe: ") + hipGetErrorString(e));
    // per SIMD: 4 waves x iterations x 4 slots x 28 instructions
    *ns_per_instruction = ms * 1e6f / ((float)iterations * 4.f * 28.f * 4.f);
    return QS_OK;
}

// ---- batches -----------------------------------------------------------------------------

extern "C" void qs_batch_free(qs_ctx *c, qs_device_batch *b) {
    if (!b) return;
    if (c) (void)hipSetDevice(c->device);
    DeviceBatch &d = b->d;
    if (d.ready) { (void)hipEventSynchronize(d.ready); (void)hipEventDestroy(d.ready); }
    if (d.slab.p) {
        // kernels that read the batch may still be queued: remember where the compute stream stands and keep the slab
        bool kept = false;
        if (c && c->slabs.size() < 4) {
            if (!d.slab.last_use && hipEventCreateWithFlags(&d.slab.last_use, hipEventDisableTiming) != hipSuccess) d.slab.last_use = nullptr;
            if (d.slab.last_use && hipEventRecord(d.slab.last_use, c->stream) == hipSuccess) { c->slabs.push_back(d.slab); kept = true; }
        }
        if (!kept) { (void)hipFree(d.slab.p); if (d.slab.last_use) (void)hipEventDestroy(d.slab.last_use); }   // (hipFree waits for the device)
    }
    delete b;
}

// One batch's arrays are packed (256-byte aligned pieces) into a pinned staging buffer of the context and go to a device
// slab of the same layout with ONE copy on the copy stream. Slabs come from a small cache of the context: qs_batch_free
// records where the compute stream stands and hands the slab back, the next upload makes the copy stream wait for that
// point -- no hipMalloc / hipFree (a device-wide synchronisation) per batch, and no host thread ever waits for a kernel.
struct Stager {
    qs_ctx *c = nullptr; int slot = 0; size_t off = 0, need = 0; hipError_t err = hipSuccess;
    BatchSlab slab;
    hipError_t begin(qs_ctx *ctx, size_t bytes) {
        c = ctx; need = std::max<size_t>(bytes, 256); slot = (int)(c->pin_next++ & 1u);
        hipError_t e = hipSuccess;
        if (!c->copy_stream) e = hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking);
        if (e == hipSuccess && !c->pin_ev[slot]) e = hipEventCreateWithFlags(&c->pin_ev[slot], hipEventDisableTiming);
        else if (e == hipSuccess) e = hipEventSynchronize(c->pin_ev[slot]);      // its previous contents are on the device
        if (e == hipSuccess) e = ensure_pinned(c, slot, need);
        if (e != hipSuccess) return err = e;
        // device slab: the smallest cached one that is large enough, else a new one
        int best = -1;
        for (size_t i = 0; i < c->slabs.size(); ++i)
            if (c->slabs[i].cap >= need && (best < 0 || c->slabs[i].cap < c->slabs[(size_t)best].cap)) best = (int)i;
        if (best >= 0) { slab = c->slabs[(size_t)best]; c->slabs.erase(c->slabs.begin() + best); }
        else {
            slab = BatchSlab();
            slab.cap = need + need / 4;
            e = hipMalloc(&slab.p, slab.cap);
            if (e != hipSuccess) { slab = BatchSlab(); return err = e; }
        }
        if (slab.last_use) e = hipStreamWaitEvent(c->copy_stream, slab.last_use, 0);   // kernels of its previous batch
        return err = e;
    }
    template <typename T> T *put(const T *src, size_t count) {
        if (err != hipSuccess) return nullptr;
        const size_t bytes = count * sizeof(T);
        if (count) std::memcpy(static_cast<unsigned char *>(c->pin[slot].get()) + off, src, bytes);
        T *dev = reinterpret_cast<T *>(static_cast<unsigned char *>(slab.p) + off);
        off += padded(bytes);
        return dev;
    }
    // `ready` fires when the batch is on the device; the staging buffer is free again at the same moment
    hipError_t finish(hipEvent_t *ready) {
        if (err != hipSuccess) return err;
        err = hipMemcpyAsync(slab.p, c->pin[slot].get(), std::max<size_t>(off, 1), hipMemcpyHostToDevice, c->copy_stream);
        if (err == hipSuccess) err = hipEventCreateWithFlags(ready, hipEventDisableTiming);
        if (err == hipSuccess) err = hipEventRecord(*ready, c->copy_stream);
        if (err == hipSuccess) err = hipEventRecord(c->pin_ev[slot], c->copy_stream);
        return err;
    }
};

// ---- depth clamp (qs_count.hip clamp_fix_kernel): the plan -- "plan_depth_clamp" in qs_count.hip's comments and DESIGN.md = clamp_cost +
// clamp_choice below and the class rules of qs_batch_upload ------------------------------------------------------------------------
// (tree, quartet) corrections a tree costs when its LCA depths are cut at `cut`: the quartets with at least three leaves in one
// maximal run of tour-adjacent LCA depths >= cut (a subtree below a node of depth `cut`): C(s,3)(L - s) + C(s,4) per run of s
// leaves. ~0 when a run is longer than the kernel's LDS table takes. runs (optional): (first position, leaves) of every run.
constexpr uint32_t kClampMaxRun = 128;  // = kFixMaxRun of qs_count.hip
static uint64_t clamp_cost(const uint16_t *adj, uint32_t L, uint32_t cut, std::vector<std::pair<uint32_t, uint32_t>> *runs) {
    uint64_t cost = 0;
    for (uint32_t i = 0; i + 1 < L;) {
        if (adj[i] < cut) { ++i; continue; }
        uint32_t j = i;
        while (j + 1 < L && adj[j] >= cut) ++j;
        const uint64_t s_ = (uint64_t)(j - i) + 1;
        if (s_ >= 3) {
            if (s_ > kClampMaxRun) return ~0ull;
            cost += binom3(s_) * (L - s_) + binom4(s_);
            if (runs) runs->emplace_back(i, (uint32_t)s_);
        }
        i = j;
    }
    return cost;
}
static uint32_t depth_class_of(uint32_t depth) {   // depth bits of a tree's class: 4 .. 10, 11 = beyond the bit-sliced instances
    uint32_t bb = 1;
    while ((1u << bb) <= depth) ++bb;
    return bb <= 4 ? 4u : (bb <= 10 ? bb : 11u);
}
// The cheapest class (depth bits) a tree may be counted in: its own, or a lower one when the corrections of the cut stay within
// `budget_per_bit` (tree, quartet) pairs per bit saved -- soft: the rule for every tree; hard (16 x): for the trees of a class
// that would otherwise be too small to pay for its own pass over the table.
static void clamp_choice(const uint16_t *adj, uint32_t L, uint32_t own_bits, uint64_t budget_per_bit, uint8_t &soft, uint8_t &hard) {
    soft = hard = (uint8_t)own_bits;
    if (budget_per_bit == 0 || own_bits <= 4) return;
    for (uint32_t tb = 4; tb < own_bits; ++tb) {
        const uint64_t cost = clamp_cost(adj, L, (1u << tb) - 1u, nullptr);
        if (cost == ~0ull) continue;
        const uint64_t bits_saved = own_bits - tb;
        if (hard == own_bits && cost <= 16 * budget_per_bit * bits_saved) hard = (uint8_t)tb;
        if (cost <= budget_per_bit * bits_saved) { soft = (uint8_t)tb; return; }
    }
}

// ---- classes of a batch (host-only: qs_batch_upload and qs_class_plan) --------------------------------------------------------------
// What validation knows about every tree: its deepest LCA, the cheapest kernel mode that is exact for it, and the lowest depth class
// the clamp budget allows it (soft: the rule for every tree; hard: 16 x, for the trees of a class too small for a pass of its own).
struct TreeFacts { std::vector<uint16_t> depth; std::vector<uint8_t> mode, soft, hard; };
// deepest adjacent LCA and "fully resolved" of one tree from its adjacent-LCA depth sequence
static void tree_shape(const uint16_t *adj, uint32_t L, std::vector<uint32_t> &stack, uint32_t &depth, bool &binary) {
    stack.clear();
    uint32_t nodes = 0, zeros = 0;
    depth = 0;
    for (uint32_t i = 0; i + 1 < L; ++i) {
        const uint32_t dd = adj[i];
        depth = std::max(depth, dd);
        if (dd == 0) ++zeros;
        while (!stack.empty() && stack.back() > dd) stack.pop_back();
        if (stack.empty() || stack.back() < dd) { stack.push_back(dd); ++nodes; }
    }
    binary = L >= 3 && (zeros == 1 || zeros == 2) && (L - 1 - zeros) == nodes - 1;
}
struct ClassPlan {
    uint32_t n_classes = 0;
    uint32_t class_mode[DeviceBatch::kMaxClasses] = {0}, class_bits[DeviceBatch::kMaxClasses] = {0}, class_end[DeviceBatch::kMaxClasses] = {0},
             class_max_depth[DeviceBatch::kMaxClasses] = {0};
    std::vector<uint32_t> order;       // slot -> tree (empty = identity: one class)
    std::vector<uint8_t> bits, mode;   // per tree: depth bits and kernel mode of the class it is counted in
};
// Classes = (kernel mode, depth bits) per TREE. The bit-sliced kernel's work per (quartet, 32 trees) grows with the bits B
// of the class (2(B+1)+2 instructions for full binary trees, B >= 4) and with what the trees may contain: binary trees with
// missing taxa 2(B+1)+5, multifurcating trees 3(B+1)+3, both 3(B+1)+7. One deep, one multifurcating or one incomplete tree
// must not put the whole batch on the dearest instance (the reference's loop is shape-independent,
// QuartetCounterLookup.hpp:65-106), so trees are counted class by class: B = 4 .. 10 and "deeper" (byte-SWAR kernel, 16-bit
// depths) within each of the four modes. Every class costs at least one more panel slice = one more pass over the table, so a
// class that holds fewer than max(class_min, class_pct %) of the trees joins one that is exact for it: first a whole mode joins
// a more general mode that is present (binary_full -> binary_partial, general_full or partial; binary_partial, general_full
// -> partial), then -- depth clamp -- a small deep class goes DOWN where the corrections allow it, else a depth class joins
// the next deeper one of its mode.
// fuse (QS_TUNE_FUSE_CLASSES, round 6): classes of equal depth bits (up to kFusedMaxBits) run as segments of ONE launch (qs_count_fused.hip),
// so what costs a table pass is a depth-bits GROUP over all modes, not a class: no mode joins a dearer mode any more, and "too small
// for a pass of its own" is asked of the group.
static void plan_classes(uint32_t n, uint32_t nt, const uint32_t *leaf_off, const uint16_t *adj_depth, const TreeFacts &F, uint32_t class_min,
                         uint32_t class_pct, uint32_t clamp_ppm, ClassPlan &P, bool fuse = false) {
    {
        constexpr uint32_t top_bits = 10, deep = 11;   // depth class id = depth bits; `deep` = beyond the bit-sliced instances
        constexpr uint32_t kModes = 4, kBits = 12;
        // Depth clamp: a tree may sit in a class BELOW its own depth bits -- the panel builders cut its depths at the class's
        // largest value and clamp_fix_kernel adds the quartets the cut ties (qs_count.hip) -- when that costs less than the
        // instructions it saves (eff_soft: 2 of 2(B+1)+2 per bit and quartet against a few thousand atomics per tree).
        uint32_t cnt[kModes][kBits] = {{0}}, mx[kModes][kBits] = {{0}};
        std::vector<uint8_t> cls(nt);
        for (uint32_t t = 0; t < nt; ++t) {
            cls[t] = F.soft[t];
            cnt[F.mode[t]][cls[t]]++;
        }
        const uint32_t small = std::max<uint32_t>(class_min, (uint32_t)((uint64_t)nt * class_pct / 100));
        uint32_t mode_map[kModes] = {0, 1, 2, 3};
        auto total = [&](uint32_t mo) { uint32_t s_ = 0; for (uint32_t bb = 0; bb < kBits; ++bb) s_ += cnt[mo][bb]; return s_; };
        auto join_mode = [&](uint32_t from, std::initializer_list<uint32_t> into) {
            const uint32_t tf = total(from);
            if (tf == 0 || tf >= small) return;
            for (uint32_t to : into) {
                if (total(to) == 0) continue;
                for (uint32_t bb = 0; bb < kBits; ++bb) { cnt[to][bb] += cnt[from][bb]; mx[to][bb] = std::max(mx[to][bb], mx[from][bb]); cnt[from][bb] = 0; }
                mode_map[from] = to;
                return;
            }
        };
        if (!fuse) {
            join_mode(MODE_BINARY_FULL, {MODE_BINARY_PARTIAL, MODE_GENERAL_FULL, MODE_PARTIAL});
            join_mode(MODE_BINARY_PARTIAL, {MODE_PARTIAL});
            join_mode(MODE_GENERAL_FULL, {MODE_PARTIAL});
        }
        auto final_mode = [&](uint32_t mo) { while (mode_map[mo] != mo) mo = mode_map[mo]; return mo; };
        // trees that share the launch of class (mo, bb): the class itself, or -- fused launches -- every class with these depth bits
        auto size_at = [&](uint32_t mo, uint32_t bb) {
            if (!fuse || bb > (uint32_t)kFusedMaxBits) return cnt[mo][bb];
            uint32_t s_ = 0;
            for (uint32_t m2 = 0; m2 < kModes; ++m2) s_ += cnt[m2][bb];
            return s_;
        };
        // a class too small for a pass of its own: its trees go DOWN to a class that is large enough where the 16-fold budget allows
        // it (what is left joins the next deeper class below, as before)
        if (clamp_ppm)
            for (uint32_t t = 0; t < nt; ++t) {
                const uint32_t mo = final_mode(F.mode[t]), bb = cls[t];
                if (size_at(mo, bb) >= small || F.hard[t] >= bb) continue;
                for (uint32_t lo = bb - 1; lo >= F.hard[t] && lo >= 4; --lo)
                    if (size_at(mo, lo) >= small) { cnt[mo][bb]--; cnt[mo][lo]++; cls[t] = (uint8_t)lo; break; }
            }
        // ... and a class that is still small after that costs a launch of its own = one more pass over the table (10-20 ms at
        // 34 GB) plus the waves' fixed cost for a handful of trees: its trees go down at ANY finite price, as long as the sum stays
        // below what the pass would cost (5 % of C(n,4) corrections ~ 1.4e8 at 512 taxa)
        if (clamp_ppm)
            for (uint32_t mo = 0; mo < kModes; ++mo)
                for (uint32_t bb = top_bits; bb > 4; --bb) {
                    if (cnt[mo][bb] == 0 || size_at(mo, bb) >= small) continue;
                    // the class below to join: the nearest one that is large enough for a pass of its own, or -- in a batch whose
                    // classes are ALL small -- the nearest non-empty one that is at least as large as this one (joining the larger
                    // neighbour downwards beats the rule below, which would send the larger class up to this one's depth bits)
                    uint32_t lo = bb - 1;
                    while (lo > 4 && size_at(mo, lo) < small) --lo;
                    if (size_at(mo, lo) < small) {
                        lo = bb - 1;
                        while (lo > 4 && size_at(mo, lo) == 0) --lo;
                        if (size_at(mo, lo) == 0 || size_at(mo, lo) < size_at(mo, bb)) continue;   // nothing below that is worth joining
                    }
                    uint64_t total = 0;
                    bool finite = true;
                    std::vector<uint32_t> members;
                    for (uint32_t t = 0; t < nt && finite; ++t) {
                        if (final_mode(F.mode[t]) != mo || cls[t] != bb) continue;
                        const uint32_t base = leaf_off[t], L = leaf_off[t + 1] - base;
                        const uint64_t cost = clamp_cost(adj_depth + base, L, (1u << lo) - 1u, nullptr);
                        if (cost == ~0ull) finite = false; else { total += cost; members.push_back(t); }
                    }
                    if (!finite || total > binom4(n) / 20) continue;
                    for (uint32_t t : members) cls[t] = (uint8_t)lo;
                    cnt[mo][lo] += cnt[mo][bb]; cnt[mo][bb] = 0;
                }
        for (uint32_t t = 0; t < nt; ++t) { const uint32_t mo = final_mode(F.mode[t]); mx[mo][cls[t]] = std::max<uint32_t>(mx[mo][cls[t]], F.depth[t]); }
        uint32_t remap[kModes][kBits];
        for (uint32_t mo = 0; mo < kModes; ++mo) {
            for (uint32_t bb = 0; bb < kBits; ++bb) remap[mo][bb] = bb;
            for (uint32_t bb = 4; bb < top_bits; ++bb) {
                if (cnt[mo][bb] == 0 || size_at(mo, bb) >= small) continue;
                uint32_t up = bb + 1;
                while (up <= top_bits && size_at(mo, up) == 0) ++up;
                if (up > top_bits) continue;               // nothing above it among the bit-sliced classes of this mode (fused: of any mode)
                cnt[mo][up] += cnt[mo][bb]; mx[mo][up] = std::max(mx[mo][up], mx[mo][bb]); cnt[mo][bb] = 0; remap[mo][bb] = up;
            }
        }
        auto final_cls = [&](uint32_t mo, uint32_t k) { while (remap[mo][k] != k) k = remap[mo][k]; return k; };
        P.n_classes = 0;
        uint32_t run = 0, start[kModes][kBits] = {{0}};
        // launch order: the dearest instances first? No: by mode, then depth -- binary_full first (its first slice stores
        // instead of accumulating when the caller asks for QS_COUNT_OVERWRITE; any class may be the first)
        static const uint32_t mode_seq[kModes] = {MODE_BINARY_FULL, MODE_BINARY_PARTIAL, MODE_GENERAL_FULL, MODE_PARTIAL};
        for (uint32_t mi = 0; mi < kModes; ++mi) {
            const uint32_t mo = mode_seq[mi];
            for (uint32_t k = 4; k <= deep; ++k) {
                if (cnt[mo][k] == 0) continue;
                start[mo][k] = run; run += cnt[mo][k];
                P.class_mode[P.n_classes] = mo; P.class_bits[P.n_classes] = k; P.class_end[P.n_classes] = run; P.class_max_depth[P.n_classes] = mx[mo][k];
                P.n_classes++;
            }
        }
        P.bits.resize(nt); P.mode.resize(nt);
        for (uint32_t t = 0; t < nt; ++t) { const uint32_t mo = final_mode(F.mode[t]); P.mode[t] = (uint8_t)mo; P.bits[t] = (uint8_t)final_cls(mo, cls[t]); }
        P.order.clear();
        if (P.n_classes > 1) {
            P.order.resize(nt);
            for (uint32_t t = 0; t < nt; ++t) P.order[start[P.mode[t]][P.bits[t]]++] = t;
        }
    }
}

/* Host-only (no device call): the class plan of qs_batch_upload for the trees of `hb` on n_taxa taxa with the depth-clamp budget
 * `ppm` (QS_TUNE_DEPTH_CLAMP): per tree its own depth bits, the depth bits of the cheapest class the budget allows, and the
 * (tree, quartet) corrections that class costs. For tests and tools; qs_batch_upload applies the same functions. */
extern "C" int qs_depth_clamp_plan(uint32_t n_taxa, const qs_tree_batch *hb, uint32_t ppm, uint8_t *own_bits, uint8_t *class_bits,
                                   uint64_t *corrections) {
    if (!hb || !hb->leaf_off || (hb->n_trees && !hb->adj_depth) || n_taxa < 4) return QS_ERR_ARG;
    const uint64_t budget = (uint64_t)((double)binom4(n_taxa) * (double)ppm * 1e-6);
    for (uint32_t t = 0; t < hb->n_trees; ++t) {
        const uint32_t base = hb->leaf_off[t], L = hb->leaf_off[t + 1] - base;
        uint32_t depth = 0;
        for (uint32_t i = 0; i + 1 < L; ++i) depth = std::max<uint32_t>(depth, hb->adj_depth[base + i]);
        const uint32_t own = depth_class_of(depth);
        uint8_t soft, hard;
        clamp_choice(hb->adj_depth + base, L, own, budget, soft, hard);
        if (own_bits) own_bits[t] = (uint8_t)own;
        if (class_bits) class_bits[t] = soft;
        if (corrections) corrections[t] = soft < own ? clamp_cost(hb->adj_depth + base, L, (1u << soft) - 1u, nullptr) : 0;
    }
    return QS_OK;
}

/* Host-only: the classes qs_batch_upload forms for the trees of `hb` (which it does not validate) with the given floors and clamp
 * budget: per tree the kernel mode (0 binary_full, 1 general_full, 2 partial, 3 binary_partial) and depth bits of the class it is
 * counted in, and its slot in the class-ordered batch. */
extern "C" int qs_class_plan(uint32_t n_taxa, const qs_tree_batch *hb, uint32_t class_min_trees, uint32_t class_pct, uint32_t clamp_ppm,
                             uint8_t *mode_of_tree, uint8_t *bits_of_tree, uint32_t *slot_of_tree) {
    if (!hb || !hb->leaf_off || (hb->n_trees && !hb->adj_depth) || n_taxa < 4 || (class_pct & 0xFFu) > 100 || (class_pct & ~(0xFFu | QS_CLASS_PLAN_FUSED))) return QS_ERR_ARG;
    const uint32_t nt = hb->n_trees;
    const uint64_t budget = (uint64_t)((double)binom4(n_taxa) * (double)clamp_ppm * 1e-6);
    TreeFacts F;
    F.depth.resize(nt); F.mode.resize(nt); F.soft.resize(nt); F.hard.resize(nt);
    std::vector<uint32_t> stack;
    for (uint32_t t = 0; t < nt; ++t) {
        const uint32_t base = hb->leaf_off[t], L = hb->leaf_off[t + 1] - base;
        uint32_t depth = 0;
        bool binary = false;
        tree_shape(hb->adj_depth + base, L, stack, depth, binary);
        F.depth[t] = (uint16_t)depth;
        F.mode[t] = (uint8_t)(L == n_taxa ? (binary ? MODE_BINARY_FULL : MODE_GENERAL_FULL) : (binary ? MODE_BINARY_PARTIAL : MODE_PARTIAL));
        clamp_choice(hb->adj_depth + base, L, depth_class_of(depth), budget, F.soft[t], F.hard[t]);
    }
    ClassPlan P;
    plan_classes(n_taxa, nt, hb->leaf_off, hb->adj_depth, F, class_min_trees, class_pct & 0xFFu, clamp_ppm, P, (class_pct & QS_CLASS_PLAN_FUSED) != 0);
    for (uint32_t t = 0; t < nt; ++t) {
        if (mode_of_tree) mode_of_tree[t] = P.mode[t];
        if (bits_of_tree) bits_of_tree[t] = P.bits[t];
    }
    if (slot_of_tree) {
        if (P.order.empty()) for (uint32_t t = 0; t < nt; ++t) slot_of_tree[t] = t;
        else for (uint32_t sl = 0; sl < nt; ++sl) slot_of_tree[P.order[sl]] = sl;
    }
    return QS_OK;
}

/* Host-only: bounds[0..n_shards] of the largest taxon id d that cut the table into n_shards contiguous shards [bounds[k], bounds[k+1])
 * (contiguous rank ranges: the rank's leading term is C(s3,4), quartet_lookup_table.hpp:161-165).
 *   by = QS_SHARDS_BY_TUPLES: balanced by the tuples a shard HOLDS, C(d,4) (memory: configs[4], out-of-core runs);
 *   by = QS_SHARDS_BY_COST:   balanced by what the count kernel SPENDS on a shard -- the wave tiles of its d-blocks (blocks of 8
 *        largest ids aligned to the shard's top, the partial block at its bottom), each tile priced at (kShardTileOverhead + live
 *        d slots): fitted to the per-shard timings of profiles/r06_scaling_model.json within 2 %. The largest shard is minimal
 *        over all contiguous cuts (bisection on the bound, greedy from the top). */
constexpr double kShardTileOverhead = 4.0;
// count-kernel cost of the d-range [d_lo, d_hi) on n taxa in those units
struct TileCost {
    std::vector<double> T0, T1;   // T0[c] = sum of tiles(c') over c' < c, T1[c] = sum of tiles(c') * c'
    explicit TileCost(uint32_t n) : T0(n + 2, 0.0), T1(n + 2, 0.0) {
        for (uint32_t c = 0; c <= n; ++c) {
            const double t = c >= 2 ? (double)bitslice3_tiles_for_c(c) : 0.0;
            T0[c + 1] = T0[c] + t; T1[c + 1] = T1[c] + t * c;
        }
    }
    double operator()(uint32_t d_lo, uint32_t d_hi) const {
        d_lo = std::max(d_lo, 3u);
        double tot = 0.0;
        for (uint32_t d1 = d_hi; d1 > d_lo;) {
            const uint32_t d0 = d1 > d_lo + kDB ? d1 - kDB : d_lo, p = d1 - d0;
            // third ids below the block see all p slots; c inside the block sees the slots above it: d1 - 1 - c
            tot += (kShardTileOverhead + p) * T0[d0] + (kShardTileOverhead + (double)(d1 - 1)) * (T0[d1 - 1] - T0[d0]) - (T1[d1 - 1] - T1[d0]);
            d1 = d0;
        }
        return tot;
    }
    double tiles(uint32_t d_lo, uint32_t d_hi) const {   // wave tiles of the range (d-blocks counted down from d_hi)
        d_lo = std::max(d_lo, 3u);
        double t = 0.0;
        for (uint32_t d1 = d_hi; d1 > d_lo; d1 = d1 > d_lo + kDB ? d1 - kDB : d_lo) t += T0[d1 - 1];
        return t;
    }
};

/* Host-only: where a slice of the count step is split so that the depth-clamp corrections of the upper d-range run beside the count
 * launch of the lower one (run_launch). The count launch of [d_lo, d_mid) is priced with the tile cost model above, the corrections
 * of [d_mid, d_hi) as their share of the table's tuples; the answer is the SMALLEST d_mid (d-blocks aligned to d_hi) whose lower
 * count launch is modelled to last kFixCover times the upper corrections -- the upper launch keeps nearly all of the work.
 * Rates (MI355X, 512 taxa x 10000 binary trees, profiles/r06_cfg2_kernel_stats.csv): 284.8 ms for 3.67e7 cost units x 313 groups at
 * 4 depth bits (a chain of 2(B+1)+2 instructions; half as much again with the third comparison of the general modes), 1.9e10
 * corrections per second.
 * 16-bit cells: two tuples may share a 32-bit word, which the corrections' atomics work on; d_mid is then moved up by half a d-block
 * where needed, so that the upper range starts at a word boundary.
 * `keep`: a d_mid whose launch orders exist already; it is kept if it still covers the corrections and the lower launch stays below
 * the cap. Returns 0 = do not split: no corrections, a range too short, fewer than a wave population of tiles (kSplitMinTiles) in
 * the lower launch, or a lower launch of more than kSplitMaxShare of the count. model_ms (may be NULL) = modelled ms of the lower
 * count launch and of the upper corrections. */
constexpr double kCountMsPerUnitGroup = 284.8 / (36697698.0 * 313.0), kFixPerMs = 1.9e7, kFixCover = 1.5, kFixLaunchMs = 0.05, kSplitMaxShare = 0.4;
constexpr double kSplitMinTiles = 4096.0;   // 256 CUs x 4 SIMDs x 4 waves
extern "C" int qs_fix_overlap_plan(uint32_t n_taxa, uint32_t d_lo, uint32_t d_hi, uint32_t count_bits, uint32_t mode, uint32_t depth_bits,
                                   uint32_t n_groups, uint64_t corrections, uint32_t keep, double *model_ms) {
    if (n_taxa < 4 || n_taxa > 65535 || d_hi > n_taxa || d_lo >= d_hi || (count_bits != 16 && count_bits != 32) || mode > 3) return QS_ERR_ARG;
    if (model_ms) model_ms[0] = model_ms[1] = 0.0;
    const uint32_t d_start = std::max(d_lo, 3u);
    if (corrections == 0 || n_groups == 0 || d_hi < d_start + 2 * kDB) return 0;
    const TileCost cost(n_taxa);
    const bool gen = mode == MODE_GENERAL_FULL || mode == MODE_PARTIAL;
    const double B = (double)std::min(std::max(depth_bits, 4u), 10u);
    const double ms_per_unit = kCountMsPerUnitGroup * n_groups * (2.0 * (B + 1.0) + 2.0) / 12.0 * (gen ? 1.5 : 1.0);
    const double all = cost(d_start, d_hi) * ms_per_unit, tuples = (double)binom4(n_taxa);
    auto fix_ms = [&](uint32_t d_mid) { return (double)corrections * ((double)(binom4(d_hi) - binom4(d_mid)) / tuples) / kFixPerMs + kFixLaunchMs; };
    auto aligned = [&](uint32_t d_mid) { return count_bits == 32 || ((binom4(d_mid) - binom4(d_lo)) & 1ull) == 0; };
    auto fits = [&](uint32_t d_mid) {
        const double lo_ms = cost(d_start, d_mid) * ms_per_unit;
        return lo_ms >= kFixCover * fix_ms(d_mid) && lo_ms <= kSplitMaxShare * all && cost.tiles(d_start, d_mid) >= kSplitMinTiles;
    };
    uint32_t pick = 0;
    if (keep > d_start && keep < d_hi && aligned(keep) && fits(keep)) pick = keep;
    for (uint32_t j = (d_hi - d_start - 1) / kDB; !pick && j >= 1; --j) {
        uint32_t d_mid = d_hi - j * kDB;
        if (cost(d_start, d_mid) * ms_per_unit < kFixCover * fix_ms(d_mid)) continue;
        if (!aligned(d_mid)) d_mid += kDB / 2;   // (C(d,4) is even for d mod 8 in 0..3 and odd above: half a block changes the parity)
        if (!aligned(d_mid) || !fits(d_mid)) return 0;   // the smallest cover is too small or too large a launch: larger ones are no better
        pick = d_mid;
    }
    if (pick && model_ms) { model_ms[0] = cost(d_start, pick) * ms_per_unit; model_ms[1] = fix_ms(pick); }
    return (int)pick;
}

extern "C" int qs_shard_bounds(uint32_t n_taxa, uint32_t n_shards, uint32_t by, uint32_t *bounds) {
    if (!bounds || n_shards == 0 || n_taxa < 4 || n_taxa > 65535) return QS_ERR_ARG;
    const uint32_t n = n_taxa, K = n_shards;
    if (by == QS_SHARDS_BY_TUPLES) {
        const uint64_t total = binom4(n);
        bounds[0] = 0;
        for (uint32_t r = 1; r < K; ++r) {
            const uint64_t target = total / K * r;
            uint32_t d = bounds[r - 1];
            while (d < n && binom4(d) < target) ++d;
            bounds[r] = d;
        }
        bounds[K] = n;
        return QS_OK;
    }
    if (by != QS_SHARDS_BY_COST) return QS_ERR_ARG;
    const TileCost cost(n);
    auto cut = [&](double bound, uint32_t *out) {     // greedy from the top; true if K shards suffice (shards left over stay empty: [0, 0))
        uint32_t hi = n;
        if (out) out[K] = n;
        for (uint32_t k = K; k-- > 0;) {
            uint32_t lo = hi;
            while (lo > 0 && cost(lo - 1, hi) <= bound) --lo;   // (ids below 3 hold nothing: the cost stops growing, lo runs to 0)
            if (k == 0 && lo > 0) return false;
            if (out) out[k] = lo;
            hi = lo;
        }
        return true;
    };
    double lo_b = cost(0, n) / K, hi_b = cost(0, n);
    for (int it = 0; it < 60 && hi_b - lo_b > 1e-9 * hi_b; ++it) {
        const double mid = 0.5 * (lo_b + hi_b);
        if (cut(mid, nullptr)) hi_b = mid; else lo_b = mid;
    }
    if (!cut(hi_b, bounds)) return QS_ERR_STATE;
    // fewer useful shards than asked for (tiny n): the greedy cut leaves the EMPTY ones at the bottom as [0, 0); move them to the top as
    // [n, n) so that shard 0 (rank 0: the rank that writes the output) always holds quartets
    uint32_t e = 0;
    while (e < K && bounds[e + 1] == 0) ++e;
    if (e) {
        for (uint32_t k = 0; k + e <= K; ++k) bounds[k] = bounds[k + e];
        for (uint32_t k = K - e + 1; k <= K; ++k) bounds[k] = n;
    }
    return QS_OK;
}

extern "C" int qs_batch_upload(qs_ctx *c, const qs_tree_batch *hb, qs_device_batch **out) {
    if (!c || !hb || !out) return fail(c, QS_ERR_ARG, "qs_batch_upload: NULL argument");
    *out = nullptr;
    if (!hb->leaf_off || (hb->n_trees && (!hb->leaf_ids || !hb->adj_depth)))
        return fail(c, QS_ERR_ARG, "qs_batch_upload: leaf arrays missing");
    const uint32_t nt = hb->n_trees, n = c->n;
    // ---- validate (the reference dies on malformed input; we return a status) ----
    // Trees are independent: large batches are checked by a few host threads, the first error in tree order wins.
    struct Part { uint32_t max_depth = 0; bool all_full = true, all_binary = true; uint32_t err_tree = 0xFFFFFFFFu; std::string err; };
    std::vector<uint16_t> tree_depth(nt, 0); // deepest LCA of every tree
    std::vector<uint8_t> tree_mode(nt, 0);   // CountMode of every tree: the cheapest kernel instance that is exact for it
    std::vector<uint8_t> eff_soft(nt, 0), eff_hard(nt, 0);   // depth clamp: the lowest class (depth bits) the budget allows the tree (clamp_choice)
    const uint64_t clamp_budget = (uint64_t)((double)binom4(n) * (double)c->tune_clamp_ppm * 1e-6);
    auto check = [&](uint32_t t0, uint32_t t1, Part &P) {
        std::vector<uint32_t> stamp(n, 0xFFFFFFFFu);
        std::vector<uint32_t> stack;
        auto bad = [&](uint32_t t, const std::string &m) { P.err_tree = t; P.err = m; };
        for (uint32_t t = t0; t < t1; ++t) {
            if (hb->leaf_off[t + 1] < hb->leaf_off[t]) return bad(t, "qs_batch_upload: leaf_off not monotone");
            const uint32_t base = hb->leaf_off[t], L = hb->leaf_off[t + 1] - base;
            if (L > n) return bad(t, "qs_batch_upload: tree " + std::to_string(t) + " has more leaves than taxa");
            if (L != n) P.all_full = false;
            for (uint32_t i = 0; i < L; ++i) {
                const uint32_t id = hb->leaf_ids[base + i];
                if (id >= n) return bad(t, "qs_batch_upload: tree " + std::to_string(t) + ": taxon id out of range (unknown taxon)");
                if (stamp[id] == t) return bad(t, "qs_batch_upload: tree " + std::to_string(t) + ": duplicate taxon");
                stamp[id] = t;
            }
            // internal nodes from the adjacent-LCA depth sequence
            uint32_t depth = 0;
            bool binary = false;
            tree_shape(hb->adj_depth + base, L, stack, depth, binary);
            P.max_depth = std::max(P.max_depth, depth);
            tree_depth[t] = (uint16_t)depth;
            if (!binary) P.all_binary = false;
            tree_mode[t] = (uint8_t)(L == n ? (binary ? MODE_BINARY_FULL : MODE_GENERAL_FULL) : (binary ? MODE_BINARY_PARTIAL : MODE_PARTIAL));
            clamp_choice(hb->adj_depth + base, L, depth_class_of(tree_depth[t]), clamp_budget, eff_soft[t], eff_hard[t]);
        }
    };
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    const unsigned workers = nt >= 2048 ? std::min(8u, std::min(hw, nt / 1024)) : 1u;
    std::vector<Part> parts(workers);
    if (workers == 1) check(0, nt, parts[0]);
    else {
        std::vector<std::thread> pool;
        for (unsigned w = 0; w < workers; ++w)
            pool.emplace_back([&, w] { check((uint32_t)((uint64_t)nt * w / workers), (uint32_t)((uint64_t)nt * (w + 1) / workers), parts[w]); });
        for (auto &th : pool) th.join();
    }
    uint32_t max_depth = 0;
    bool all_full = true, all_binary = true;
    for (const Part &P : parts) { // parts are in tree order: the first one with an error holds the earliest bad tree
        if (P.err_tree != 0xFFFFFFFFu) return fail(c, QS_ERR_ARG, P.err);
        max_depth = std::max(max_depth, P.max_depth);
        all_full = all_full && P.all_full; all_binary = all_binary && P.all_binary;
    }
    qs_device_batch *b = new qs_device_batch();
    DeviceBatch &d = b->d;
    d.n_trees = nt;
    d.total_leaves = nt ? hb->leaf_off[nt] : 0;
    d.max_depth = max_depth; d.all_full = all_full && nt > 0; d.all_binary = all_binary && nt > 0;
    // classes = (kernel mode, depth bits) per tree: plan_classes above
    std::vector<uint32_t> order_host;
    std::vector<FixUnit> fix_units;
    ClassPlan plan;
    {
        TreeFacts F;
        F.depth.swap(tree_depth); F.mode.swap(tree_mode); F.soft.swap(eff_soft); F.hard.swap(eff_hard);
        plan_classes(n, nt, hb->leaf_off, hb->adj_depth, F, c->tune_class_min, c->tune_class_pct, c->tune_clamp_ppm, plan,
                     c->tune_fuse && c->tune_gather_impl != QS_IMPL_SWAR);
        tree_depth.swap(F.depth); tree_mode.swap(F.mode);
        d.n_classes = plan.n_classes;
        for (uint32_t k = 0; k < plan.n_classes; ++k) { d.class_mode[k] = plan.class_mode[k]; d.class_bits[k] = plan.class_bits[k]; d.class_end[k] = plan.class_end[k]; d.class_max_depth[k] = plan.class_max_depth[k]; }
        order_host = plan.order;
        constexpr uint32_t top_bits = 10;
        // correction units of the trees whose class holds fewer depth bits than they need, by slot (a slice of a class = a range of
        // slots = a range of units). One unit = one workgroup = a stretch of a run's triples worth ~32 K fourth leaves.
        if (c->tune_clamp_ppm) {
            std::vector<std::pair<uint32_t, uint32_t>> runs;
            auto emit = [&](uint32_t slot, uint32_t t) {
                const uint32_t fb = plan.bits[t];
                if (fb > top_bits || depth_class_of(tree_depth[t]) <= fb) return;
                const uint32_t base = hb->leaf_off[t], L = hb->leaf_off[t + 1] - base;
                runs.clear();
                const uint64_t cost = clamp_cost(hb->adj_depth + base, L, (1u << fb) - 1u, &runs);
                if (cost == ~0ull) return;   // cannot happen: the cut of a lower class was accepted, and runs only shrink with the cut
                d.fix_quartets += cost; d.clamped_trees++;
                const uint32_t per_unit = std::max<uint32_t>(1u, 32768u / std::max<uint32_t>(L, 1u));
                for (const auto &r : runs) {
                    const uint32_t triples = (uint32_t)binom3(r.second);
                    for (uint32_t t0 = 0; t0 < triples; t0 += per_unit) {
                        fix_units.push_back(FixUnit{t, r.first | (r.second << 16), t0, std::min(triples, t0 + per_unit)});
                        b->fix_slot.push_back(slot);
                        if (b->fix_work.empty()) b->fix_work.push_back(0);
                        b->fix_work.push_back(b->fix_work.back() + (uint64_t)(std::min(triples, t0 + per_unit) - t0) * (L > 3 ? L - 3 : 0));
                    }
                }
            };
            if (order_host.empty()) for (uint32_t t = 0; t < nt; ++t) emit(t, t);
            else for (uint32_t sl = 0; sl < nt; ++sl) emit(sl, order_host[sl]);
            d.n_fix = (uint32_t)fix_units.size();
        }
    }
    // scatter batches: the tree of every inner node, and a bounds check of the leaf ranges (host side, before any copy)
    const bool with_nodes = hb->node_off && hb->rng_off && hb->ranges;
    std::vector<uint32_t> node_tree;
    if (with_nodes) {
        d.n_nodes = hb->node_off[nt];
        d.n_links = hb->rng_off[d.n_nodes];
        node_tree.resize(d.n_nodes);
        for (uint32_t t = 0; t < nt; ++t) {
            const uint32_t L = hb->leaf_off[t + 1] - hb->leaf_off[t];
            d.max_tree_nodes = std::max(d.max_tree_nodes, hb->node_off[t + 1] - hb->node_off[t]);
            for (uint32_t v = hb->node_off[t]; v < hb->node_off[t + 1]; ++v) {
                node_tree[v] = t;
                for (uint32_t k = hb->rng_off[v]; k < hb->rng_off[v + 1]; ++k)
                    if (hb->ranges[2 * k] >= std::max(L, 1u) || hb->ranges[2 * k + 1] >= std::max(L, 1u)) {
                        qs_batch_free(c, b);
                        return fail(c, QS_ERR_ARG, "qs_batch_upload: range position out of bounds");
                    }
            }
        }
    }
    hipError_t e = hipSetDevice(c->device);
    Stager st;
    if (e == hipSuccess) {
        size_t need = padded(((size_t)nt + 1) * 4) + 2 * padded((size_t)d.total_leaves * 2) + padded(order_host.size() * 4) +
                      padded(fix_units.size() * sizeof(FixUnit));
        if (with_nodes) need += padded(((size_t)nt + 1) * 4) + padded(((size_t)d.n_nodes + 1) * 4) + padded((size_t)d.n_nodes * 4) + padded((size_t)2 * d.n_links * 2);
        e = st.begin(c, need);
    }
    if (e == hipSuccess) {
        d.leaf_off = st.put(hb->leaf_off, (size_t)nt + 1);
        d.leaf_ids = st.put(hb->leaf_ids, d.total_leaves);
        d.adj_depth = st.put(hb->adj_depth, d.total_leaves);
        if (!order_host.empty()) d.tree_order = st.put(order_host.data(), order_host.size());
        if (!fix_units.empty()) d.fix_units = st.put(fix_units.data(), fix_units.size());
        if (with_nodes) {
            d.node_off = st.put(hb->node_off, (size_t)nt + 1);
            d.rng_off = st.put(hb->rng_off, (size_t)d.n_nodes + 1);
            d.node_tree = st.put(node_tree.data(), d.n_nodes);
            d.ranges = st.put(hb->ranges, (size_t)2 * d.n_links);
        }
        e = st.finish(&d.ready);
    }
    d.slab = st.slab;
    if (e != hipSuccess) {
        qs_batch_free(c, b);
        return fail(c, e == hipErrorOutOfMemory ? QS_ERR_OOM : QS_ERR_HIP, std::string("qs_batch_upload: ") + hipGetErrorString(e));
    }
    *out = b;
    return QS_OK;
}

extern "C" uint32_t qs_batch_flags(const qs_device_batch *b) {
    if (!b) return 0;
    return (b->d.all_full ? QS_BATCH_ALL_TAXA : 0u) | (b->d.all_binary ? QS_BATCH_BINARY : 0u);
}

// corrections of the depth clamp for the trees in slots [slot_lo, slot_hi) of the batch whose largest id lies in [d_a, d_b), on
// stream s: after the count kernel that stored that range
static hipError_t clamp_fix_slots(qs_ctx *c, hipStream_t s, const qs_device_batch *b, uint32_t slot_lo, uint32_t slot_hi, uint32_t d_a, uint32_t d_b,
                                  int mode, uint32_t *wire) {
    const auto lo = std::lower_bound(b->fix_slot.begin(), b->fix_slot.end(), slot_lo), hi = std::lower_bound(lo, b->fix_slot.end(), slot_hi);
    if (lo == hi || d_a >= d_b) return hipSuccess;
    return launch_clamp_fix(s, b->d, b->d.fix_units + (lo - b->fix_slot.begin()), (uint32_t)(hi - lo), d_a, d_b,
                            c->rank_lo, c->table, (int)c->count_bits, mode, wire, c->dev_flags.get());
}
// ... and what they are modelled to cost: (tree, quartet) corrections over the whole table (an upper bound, see qs_batch_upload)
static uint64_t clamp_fix_work(const qs_device_batch *b, uint32_t slot_lo, uint32_t slot_hi) {
    const auto lo = std::lower_bound(b->fix_slot.begin(), b->fix_slot.end(), slot_lo), hi = std::lower_bound(lo, b->fix_slot.end(), slot_hi);
    return b->fix_work.empty() ? 0 : b->fix_work[hi - b->fix_slot.begin()] - b->fix_work[lo - b->fix_slot.begin()];
}

// the pair-depth panel holds `need` bytes (growing it waits for the launches that read the old one)
static int ensure_panel(qs_ctx *c, size_t need) {
    const hipError_t e = c->panel.reserve(need, &c->stream);   // exactly `need`: see run_launch
    if (e == hipErrorOutOfMemory) return fail(c, QS_ERR_OOM, "Insufficient memory! (pair-depth panel)");
    QS_HIP(c, e);   // (the wait for the stream)
    return QS_OK;
}

// The shard as a count kernel sees it: the 8x8 tiling of the byte-SWAR gather kernel, or (tiles16x8) the 16x8 tiling of the bit-sliced
// kernels with its launch order -- asked for here, so that a batch without a bit-sliced launch never builds it -- and, for a
// binary_full launch that is not fused (coop), the cooperative lists.
static int count_geometry(qs_ctx *c, bool tiles16x8, bool coop, CountGeometry &g) {
    g.n = c->n; g.d_lo = std::max(c->d_lo, 3u); g.d_hi = c->d_hi; g.rank_lo = c->rank_lo; g.n_dblk = c->n_dblk;
    if (!tiles16x8) { g.total_tiles = c->total_tiles; g.dprefix = c->dprefix.get(); g.cprefix = c->cprefix.get(); return QS_OK; }
    g.total_tiles = c->total_tiles3; g.dprefix = c->dprefix3.get(); g.cprefix = c->cprefix3.get();
    const int rc = tile_order(c, &g.perm);
    if (rc == QS_OK && coop) { g.perm_coop = c->perm_coop.get(); g.n_coop = c->n_coop; g.perm_rest = c->perm_rest.get(); g.n_rest = c->n_rest; }
    return rc;
}

// The 16x8 tiling `g` of the shard cut at d_mid into the tilings of [d_mid, d_hi) (hi: the leading d-blocks of g, so g's prefix
// array serves) and [d_lo, d_mid) (lo: d-blocks counted down from d_mid, a prefix array of its own), each with its launch order in
// the nesting of g's. Kept in the context for the d_mid they were built for.
static int split_geometry(qs_ctx *c, uint32_t d_mid, const CountGeometry &g, CountGeometry &hi, CountGeometry &lo, bool *rebuilt) {
    *rebuilt = false;
    qs_ctx::Split &S = c->split;
    const uint32_t d_start = g.d_lo;
    if (S.d_mid != d_mid || S.perm_of != g.perm) {
        // Everything goes onto the context's stream, behind the launches that may still read the old lists. The host waits only
        // where it rewrites what the device may still use: for the copies out of the host lists of an earlier split (the runtime may
        // read pageable memory after the call returns), and for the stream where a buffer has to grow. The first split of a context
        // finds neither.
        S.d_mid = 0;
        if (S.copied_valid) QS_HIP(c, hipEventSynchronize(S.copied.get()));
        S.copied_valid = false;
        S.n_dblk_hi = (g.d_hi - std::max(d_mid, d_start) + kDB - 1) / kDB;
        S.tiles_hi = c->h_dp3[S.n_dblk_hi];
        S.n_dblk_lo = d_mid > d_start ? (d_mid - d_start + kDB - 1) / kDB : 0;
        S.h_dp_lo.assign(S.n_dblk_lo + 1, 0);   // (host copies stay in the context: the asynchronous copies read them)
        for (uint32_t k = 0; k < S.n_dblk_lo; ++k) S.h_dp_lo[k + 1] = S.h_dp_lo[k] + c->h_cp3[d_mid - k * kDB - 1];
        S.tiles_lo = S.h_dp_lo[S.n_dblk_lo];
        if (S.dprefix_lo.reserve(S.h_dp_lo.size() * 4, &c->stream) != hipSuccess) return fail(c, QS_ERR_OOM, "hipMalloc split tiling");
        QS_HIP(c, hipMemcpyAsync(S.dprefix_lo.get(), S.h_dp_lo.data(), S.h_dp_lo.size() * 4, hipMemcpyHostToDevice, c->stream));
        if (g.perm) {
            // upper range: the shard's launch order without the tiles of the lower d-blocks -- its tiles are the ids below tiles_hi and
            // the nesting stays --, filtered on the device (12 M entries at 512 taxa: two short kernels instead of 25 ms of host work)
            if (S.perm_hi.reserve(std::max<size_t>(S.tiles_hi, 1) * 4, &c->stream) != hipSuccess ||
                S.filter_scratch.reserve(perm_filter_scratch_bytes(g.total_tiles), &c->stream) != hipSuccess)
                return fail(c, QS_ERR_OOM, "hipMalloc split tile order");
            QS_HIP(c, launch_perm_filter(c->stream, g.perm, g.total_tiles, S.tiles_hi, S.perm_hi.get(), S.tiles_hi, S.filter_scratch.get()));
            // lower range: a tiling of its own (d-blocks counted down from d_mid), a few per cent of the tiles: enumerated on the host
            std::string perr;
            const TilePermParams P_lo{c->tile_chunk, c->tile_cblock, c->tile_cgroup, d_mid, S.n_dblk_lo, S.tiles_lo};
            if (!build_tile_perm(P_lo, c->h_cp3, S.h_dp_lo, S.h_perm_lo, perr)) return fail(c, QS_ERR_STATE, perr);
            if (S.perm_lo.reserve(std::max<size_t>(S.h_perm_lo.size(), 1) * 4, &c->stream) != hipSuccess) return fail(c, QS_ERR_OOM, "hipMalloc split tile order");
            if (!S.h_perm_lo.empty()) QS_HIP(c, hipMemcpyAsync(S.perm_lo.get(), S.h_perm_lo.data(), S.h_perm_lo.size() * 4, hipMemcpyHostToDevice, c->stream));
        }
        QS_HIP(c, S.copied.ensure());
        QS_HIP(c, hipEventRecord(S.copied.get(), c->stream));
        S.copied_valid = true;
        S.perm_of = g.perm; S.d_mid = d_mid;
        *rebuilt = true;
    }
    hi = g; lo = g;
    hi.d_lo = std::max(d_mid, d_start); hi.n_dblk = S.n_dblk_hi; hi.total_tiles = S.tiles_hi; hi.perm = g.perm ? S.perm_hi.get() : nullptr;
    lo.d_hi = std::max(d_mid, d_start); lo.n_dblk = S.n_dblk_lo; lo.total_tiles = S.tiles_lo; lo.dprefix = S.dprefix_lo.get(); lo.perm = g.perm ? S.perm_lo.get() : nullptr;
    return QS_OK;
}

// One launch of a count kernel = 1..4 segments; a segment = one class's share of it: the slots [slot0, slot0 + trees) of the
// class-ordered batch in a panel of their own. (Classes = kernel mode x depth bits per TREE: qs_batch_upload.)
struct Seg {
    uint32_t slot0, trees;
    int mode;             // CountMode of the kernel instance
    bool part;            // panel elements carry a presence word
    uint32_t nw;          // bit-sliced: words per compact panel element
    uint32_t tpg;         // trees per group (= panel element along the tree axis): 32, byte-SWAR 16 / 8
    size_t group_bytes;   // bytes of one group: an element per pair
    uint32_t groups() const { return (trees + tpg - 1) / tpg; }
};
enum CountKernel { KERNEL_BITSLICE3, KERNEL_FUSED, KERNEL_SWAR };
struct Launch {
    CountKernel kernel;
    int bits;             // depth bits of the bit-sliced instance, panel bits (8 / 16) of the byte-SWAR kernel
    std::vector<Seg> segs;
};

static Seg bitslice_seg(const qs_ctx *c, uint32_t slot0, uint32_t trees, int mode, uint32_t depth_bits) {
    const bool part = mode == MODE_PARTIAL || mode == MODE_BINARY_PARTIAL;
    const uint32_t nw = std::max(depth_bits, 4u) + (part ? 1u : 0u);
    return Seg{slot0, trees, mode, part, nw, 32u, (size_t)binom2(c->n) * nw * 4};
}

// a class in the variant string: [mode.]bitslice_b<planes>x2[:trees] or [mode.]depth_u<panel bits>[:trees]; the wire format names the
// kernel family once, in front of its classes (family = false)
static std::string class_name(const Launch &L, const Seg &sg, bool family, const char *mode, bool with_trees) {
    std::string nm = L.kernel == KERNEL_SWAR ? "depth_u" + std::to_string(L.bits)
                                             : (family ? "bitslice_b" : "b") + std::to_string(std::max(L.bits, 4)) + "x2";
    if (mode) nm = std::string(mode) + "." + nm;
    if (with_trees) nm += ":" + std::to_string(sg.trees);
    return nm;
}

// Enqueue one launch, slice by slice (slice_groups over the concatenated group list [0, g_total) of its segments; slice [g0, g1)
// takes from every segment the groups that fall into it): panel build(s), count kernel, depth-clamp corrections, and with
// `timed` an event after each of the three. Into the table, or (wire != NULL) the two-cell wire words.
static int run_launch(qs_ctx *c, const qs_device_batch *b, const Launch &L, uint32_t *wire, bool timed, bool overwrite, bool &first) {
    const DeviceBatch &d = b->d;
    const bool bitsliced = L.kernel != KERNEL_SWAR;
    const int mode0 = L.segs[0].mode;
    CountGeometry g;
    int rc = count_geometry(c, bitsliced, L.kernel == KERNEL_BITSLICE3 && mode0 == MODE_BINARY_FULL, g);
    if (rc != QS_OK) return rc;
    uint32_t g_total = 0;
    size_t group_bytes = 0;
    for (const Seg &sg : L.segs) { g_total += sg.groups(); group_bytes = std::max(group_bytes, sg.group_bytes); }
    const uint32_t per_slice = slice_groups(c, group_bytes, g_total, g.perm != nullptr);
    // The segments of a slice lie one behind the other, each at a 256-byte boundary: only the gaps BETWEEN them need room. A launch
    // of one segment so asks for per_slice groups exactly -- what qs_prepare has allocated ahead for the common 5-plane class; a
    // byte more would make the CLI's first count wait for the stream, free that panel and allocate another.
    rc = ensure_panel(c, (size_t)per_slice * group_bytes + 256 * (L.segs.size() - 1));
    if (rc != QS_OK) return rc;
    // Split slices (QS_TUNE_FIX_OVERLAP): one d_mid for the launch, planned for a slice's groups and its share of the launch's
    // corrections. Not with the byte-SWAR kernel (no corrections), the cooperative lists, or where the plan says a split does not pay.
    uint32_t d_mid = 0;
    CountGeometry g_hi = g, g_lo = g;
    if (bitsliced && d.n_fix && c->tune_fix_overlap && !g.perm_coop) {
        uint64_t work = 0;
        for (const Seg &sg : L.segs) work += clamp_fix_work(b, sg.slot0, sg.slot0 + sg.trees);
        const uint32_t grp = std::min(per_slice, g_total), n_slices = (g_total + per_slice - 1) / per_slice;
        work = (work + n_slices - 1) / std::max(n_slices, 1u);
        if (c->tune_fix_split_at) d_mid = (work && c->tune_fix_split_at > c->d_lo && c->tune_fix_split_at < c->d_hi) ? c->tune_fix_split_at : 0;
        else {
            int gen = 0;
            for (const Seg &sg : L.segs) gen = gen || sg.mode == MODE_GENERAL_FULL || sg.mode == MODE_PARTIAL;
            const int pick = qs_fix_overlap_plan(c->n, c->d_lo, c->d_hi, c->count_bits, gen ? MODE_GENERAL_FULL : MODE_BINARY_FULL, (uint32_t)L.bits, grp, work, c->split.d_mid, nullptr);
            d_mid = pick > 0 ? (uint32_t)pick : 0;
        }
        if (d_mid) {
            QS_HIP(c, c->fix_stream.ensure());
            QS_HIP(c, c->fix_go.ensure());
            QS_HIP(c, c->fix_done.ensure());
            bool rebuilt = false;
            rc = split_geometry(c, d_mid, g, g_hi, g_lo, &rebuilt);
            if (rc != QS_OK) return rc;
            if (timed && rebuilt) QS_HIP(c, mark(c, 3));   // (the filter kernels and copies of a new split: not the next panel build's time)
        }
    }
    for (uint32_t g0 = 0; g0 < g_total; g0 += per_slice) {
        const uint32_t g1 = std::min(g_total, g0 + per_slice);
        // per CountMode, as the fused kernel takes them (a mode without trees in this slice: 0 groups)
        const void *seg_panel[4] = {nullptr, nullptr, nullptr, nullptr};
        uint32_t seg_groups[4] = {0, 0, 0, 0}, seg_trees[4] = {0, 0, 0, 0}, seg_slot[4] = {0, 0, 0, 0};
        size_t off = 0;
        uint32_t base = 0;
        for (const Seg &sg : L.segs) {
            const uint32_t a = std::max(g0, base), e_ = std::min(g1, base + sg.groups());
            base += sg.groups();
            if (a >= e_) continue;
            const uint32_t ga = a - (base - sg.groups()), nch = e_ - a;
            const uint32_t t0 = ga * sg.tpg, nt = std::min(nch * sg.tpg, sg.trees - t0);
            DeviceBatch sub = d;
            sub.slot0 = sg.slot0 + t0;        // slots [slot0, slot0 + nt) of the class-ordered batch
            sub.n_trees = nt;
            void *pp = (char *)c->panel.get() + off;
            if (bitsliced) QS_HIP(c, launch_build_bitpanel(c->stream, sub, c->n, sg.part, pp, nch, sg.nw, c->tune_panel_kernel == 1));
            else QS_HIP(c, launch_build_panel(c->stream, sub, c->n, L.bits, sg.part, pp, nch));
            seg_panel[sg.mode] = pp; seg_groups[sg.mode] = nch; seg_trees[sg.mode] = nt; seg_slot[sg.mode] = sub.slot0;
            off += ((size_t)nch * sg.group_bytes + 255) & ~(size_t)255;
        }
        if (timed) QS_HIP(c, mark(c, 0));
        const bool ow = overwrite && first;
        // a count launch over the tiling gg (the whole shard, or one d-range of a split slice)
        auto count_range = [&](const CountGeometry &gg) -> hipError_t {
            if (L.kernel == KERNEL_FUSED)
                return launch_count_bitslice3_fused(c->stream, gg, seg_panel, seg_groups, seg_trees, L.bits, c->table, (int)c->count_bits, c->dev_flags.get(), ow);
            if (L.kernel == KERNEL_BITSLICE3)
                return launch_count_bitslice3(c->stream, gg, seg_panel[mode0], L.bits, mode0, seg_groups[mode0], seg_trees[mode0], wire ? nullptr : c->table,
                                              wire ? 32 : (int)c->count_bits, c->dev_flags.get(), ow, wire);
            return launch_count_gather(c->stream, gg, seg_panel[mode0], L.bits, mode0, seg_groups[mode0], seg_trees[mode0], c->table, (int)c->count_bits, c->dev_flags.get(), ow);
        };
        // the corrections of the slice's trees in the d-range [d_a, d_b), on stream s
        auto fix_range = [&](hipStream_t s, uint32_t d_a, uint32_t d_b) -> hipError_t {
            for (int mo = 0; mo < 4; ++mo) {   // (the rule of the correction depends on the mode: a tied quartet sits in the third cell of a binary tree)
                const hipError_t e = seg_groups[mo] ? clamp_fix_slots(c, s, b, seg_slot[mo], seg_slot[mo] + seg_trees[mo], d_a, d_b, mo, wire) : hipSuccess;
                if (e != hipSuccess) return e;
            }
            return hipSuccess;
        };
        bool has_fix = false;   // (never the byte-SWAR kernel: its panel holds the trees' own depths)
        for (int mo = 0; mo < 4 && bitsliced && d.n_fix; ++mo) has_fix = has_fix || (seg_groups[mo] && clamp_fix_work(b, seg_slot[mo], seg_slot[mo] + seg_trees[mo]) > 0);
        // (with the first overwriting launch enqueued the old contents are gone: a later refusal must not leave their count behind)
        auto overwritten = [&] { if (ow) { if (wire) c->wire_trees = 0; else c->trees_counted = 0; } };
        first = false;
        if (has_fix && d_mid) {
            // THE ORDERING RULE of a split slice. A correction must land after the store of the cell it corrects, and a cell belongs to
            // exactly one of the two d-ranges (a d-range is one contiguous piece of the table), so:
            //   main stream:        count [d_mid, d_hi) -> fix_go -> count [d_lo, d_mid) -> corrections of [d_lo, d_mid) -> wait for fix_done
            //   correction stream:  wait for fix_go -> corrections of [d_mid, d_hi) -> fix_done
            // Kernels in flight together (the lower count launch and the upper corrections) work on disjoint ranges; everything later on
            // the main stream -- the next slice, the next class, whoever reads the table -- comes after both. Whatever fails once the
            // correction stream has work, the main stream still waits for it before the error is returned.
            const hipStream_t fs = c->fix_stream.get();
            QS_HIP(c, count_range(g_hi));
            overwritten();
            const uint32_t ev_hi = c->ev_used;
            if (timed) QS_HIP(c, mark(c, 1));
            QS_HIP(c, hipEventRecord(c->fix_go.get(), c->stream));
            QS_HIP(c, hipStreamWaitEvent(fs, c->fix_go.get(), 0));
            hipError_t e = fix_range(fs, g_hi.d_lo, g_hi.d_hi);
            if (e == hipSuccess && timed) e = mark(c, 2, &fs, ev_hi);
            const hipError_t e_done = hipEventRecord(c->fix_done.get(), fs);
            uint32_t ev_lo = 0;
            if (e == hipSuccess) e = count_range(g_lo);
            if (e == hipSuccess) { ev_lo = c->ev_used; if (timed) e = mark(c, 4, nullptr, ev_hi); }
            if (e == hipSuccess) e = fix_range(c->stream, g_lo.d_lo, g_lo.d_hi);
            if (e == hipSuccess && timed) e = mark(c, 2, nullptr, ev_lo);
            // the join: behind fix_done, or -- if that event could not be recorded -- once the correction stream has drained
            const hipError_t e_join = e_done == hipSuccess ? hipStreamWaitEvent(c->stream, c->fix_done.get(), 0) : hipStreamSynchronize(fs);
            QS_HIP(c, e);
            QS_HIP(c, e_done);
            QS_HIP(c, e_join);
            if (timed) QS_HIP(c, mark(c, 3));
            c->last_split = d_mid; ++c->last_splits;
        } else {
            QS_HIP(c, count_range(g));
            overwritten();
            if (timed) QS_HIP(c, mark(c, 1));
            if (has_fix) {
                QS_HIP(c, fix_range(c->stream, g.d_lo, g.d_hi));
                if (timed) QS_HIP(c, mark(c, 2));
            }
        }
    }
    return QS_OK;
}

// QS_COUNT_WIRE16X2: count a binary_full batch straight into the attached wire buffer (one word per tuple), class by class
static int count_batch_wire(qs_ctx *c, const qs_device_batch *b, uint32_t algo) {
    const DeviceBatch &d = b->d;
    if (!c->wire_out) return fail(c, QS_ERR_STATE, "QS_COUNT_WIRE16X2: no wire buffer (qs_wire_attach first)");
    const bool overwrite = (algo & QS_COUNT_OVERWRITE) != 0;
    const uint32_t base_algo = algo & 0xFFu;
    if (base_algo != QS_ALGO_AUTO && base_algo != QS_ALGO_GATHER) return fail(c, QS_ERR_ARG, "QS_COUNT_WIRE16X2 needs the gather algorithm");
    const bool timed = (algo & QS_COUNT_TIMED) != 0;
    QS_HIP(c, hipSetDevice(c->device));
    if (d.n_trees == 0) {
        if (overwrite) { QS_HIP(c, hipMemsetAsync(c->wire_out, 0, c->n_tuples * 4, c->stream)); c->wire_trees = 0; }
        return QS_OK;
    }
    if (!(d.all_full && d.all_binary))
        return fail(c, QS_ERR_STATE, "QS_COUNT_WIRE16X2: the batch is not made of binary trees that hold all taxa (count into the table and use qs_table_pack16)");
    if (d.ready) QS_HIP(c, hipStreamWaitEvent(c->stream, d.ready, 0));
    if ((overwrite ? 0 : c->wire_trees) + d.n_trees > 0xFFFFull)
        return fail(c, QS_ERR_OVERFLOW, "QS_COUNT_WIRE16X2: more than 65535 trees do not fit 16-bit cells");
    if (d.class_bits[d.n_classes - 1] > 10) return fail(c, QS_ERR_UNSUPPORTED, "QS_COUNT_WIRE16X2: tree depth needs more than 10 bits; count into the table instead");
    { const uint32_t *order; int rc_o = tile_order(c, &order); if (rc_o != QS_OK) return rc_o; }   // (a failure here leaves the last call's events as they were)
    c->ev_used = 0; c->last_split = c->last_splits = 0;
    if (timed) QS_HIP(c, mark(c, 0));
    bool first = true;
    c->variant = "gather/binary_full/bitslice_";
    for (uint32_t k = 0; k < d.n_classes; ++k) {
        const uint32_t s_lo = k ? d.class_end[k - 1] : 0;
        const Launch L{KERNEL_BITSLICE3, (int)d.class_bits[k], {bitslice_seg(c, s_lo, d.class_end[k] - s_lo, MODE_BINARY_FULL, d.class_bits[k])}};
        int rc = run_launch(c, b, L, c->wire_out, timed, overwrite, first);
        if (rc != QS_OK) return rc;
        c->variant += (k ? "+" : "") + class_name(L, L.segs[0], false, nullptr, d.n_classes > 1);
    }
    c->variant += "/wire_u16x2";
    if (d.n_fix) c->variant += "/clamp:" + std::to_string(d.clamped_trees);
    if (c->last_splits) c->variant += "/overlap:" + std::to_string(c->last_split);
    if (c->n_coop) c->variant += "/coop4";
    c->wire_trees = (overwrite ? 0 : c->wire_trees) + d.n_trees;
    c->last_timed = timed;
    return QS_OK;
}

extern "C" int qs_count_batch(qs_ctx *c, const qs_device_batch *b, uint32_t algo) {
    if (c) c->log_valid = false;   // (the table / view / tuning may change: a logged pass 1 no longer describes it)
    if (!c || !b) return fail(c, QS_ERR_ARG, "qs_count_batch: NULL argument");
    if (algo & QS_COUNT_WIRE16X2) return count_batch_wire(c, b, algo);
    if (!c->table) return fail(c, QS_ERR_STATE, "qs_count_batch: no table (qs_table_alloc / qs_table_attach first)");
    const DeviceBatch &d = b->d;
    QS_HIP(c, hipSetDevice(c->device));
    if (d.n_trees == 0) {
        if (algo & QS_COUNT_OVERWRITE) { // "discard the previous contents" holds for an empty batch too
            QS_HIP(c, hipMemsetAsync(c->table, 0, c->n_tuples * 3 * (c->count_bits / 8), c->stream));
            c->trees_counted = 0;
        }
        c->last_timed = false;
        return QS_OK;
    }
    if (c->count_bits == 16 && ((algo & QS_COUNT_OVERWRITE) ? 0 : c->trees_counted) + d.n_trees > 0xFFFFull)
        return fail(c, QS_ERR_OVERFLOW, "qs_count_batch: more than 65535 trees need count_bits = 32");
    if (d.ready) QS_HIP(c, hipStreamWaitEvent(c->stream, d.ready, 0));   // the batch's copies run on the copy stream
    const bool overwrite = (algo & QS_COUNT_OVERWRITE) != 0;
    const bool timed = (algo & QS_COUNT_TIMED) != 0;
    algo &= ~(QS_COUNT_OVERWRITE | QS_COUNT_TIMED);
    if (algo == QS_ALGO_AUTO) algo = QS_ALGO_GATHER;
    if (overwrite && algo != QS_ALGO_GATHER) return fail(c, QS_ERR_ARG, "qs_count_batch: QS_COUNT_OVERWRITE needs the gather algorithm");
    // (a call refused before its first launch leaves table and count as they were; run_launch resets trees_counted with the first
    // overwriting launch it enqueues, so that a refusal after it -- a later class too deep, a panel that cannot grow -- leaves no stale count)
    c->ev_used = 0; c->last_split = c->last_splits = 0;
    if (timed) QS_HIP(c, mark(c, 0));
    if (algo == QS_ALGO_GATHER) {
        static const char *mode_names[4] = {"binary_full", "general_full", "partial", "binary_partial"};
        // This function only chooses the launches (run_launch enqueues them). With QS_IMPL_SWAR the whole batch is one class of the
        // byte-SWAR kernel, in the mode the batch as a whole needs.
        const uint32_t top_bits = 10u;
        const bool all_swar = c->tune_gather_impl == QS_IMPL_SWAR;
        if (c->tune_gather_impl == QS_IMPL_BITSLICE)
            for (uint32_t k = 0; k < d.n_classes; ++k)
                if (d.class_bits[k] > top_bits) return fail(c, QS_ERR_UNSUPPORTED, "QS_IMPL_BITSLICE: tree depth needs more than 10 bits");
        const uint32_t n_cls = all_swar ? 1u : d.n_classes;
        bool first = true, mixed = false;
        for (uint32_t k = 1; k < n_cls; ++k) mixed = mixed || d.class_mode[k] != d.class_mode[0];
        const int batch_mode = !d.all_full ? MODE_PARTIAL : (d.all_binary ? MODE_BINARY_FULL : MODE_GENERAL_FULL);
        std::string names;
        bool any_coop = false;
        // several classes: "a:trees+b:trees", classes of several modes: "mode.a:trees+..."
        auto run_and_name = [&](const Launch &L) {
            const int rc = run_launch(c, b, L, nullptr, timed, overwrite, first);
            for (const Seg &sg : L.segs)
                if (rc == QS_OK) names += (names.empty() ? "" : "+") + class_name(L, sg, true, mixed ? mode_names[sg.mode] : nullptr, n_cls > 1);
            return rc;
        };
        auto slot_lo = [&](uint32_t k) { return k ? d.class_end[k - 1] : 0u; };
        // ---- fused launches (QS_TUNE_FUSE_CLASSES): the bit-sliced classes that share their depth bits run as segments of ONE launch
        // of count_bitslice3_fused_kernel -- one pass over the table, one wave prologue / epilogue, whatever the mix of modes ----
        std::vector<bool> done(n_cls, false);
        uint32_t fused_launch_groups = 0;
        for (uint32_t bb = 4; c->tune_fuse && !all_swar && bb <= (uint32_t)kFusedMaxBits; ++bb) {
            std::vector<uint32_t> ks;
            for (uint32_t k = 0; k < n_cls; ++k) if (std::max(d.class_bits[k], 4u) == bb) ks.push_back(k);
            // a lone binary_partial class at 4 or 5 bits takes the fused binary kernel too (with an empty binary_full segment): under the one
            // dispatch it needs 123 VGPRs and spills nothing at 4 waves per SIMD, where the one-class instance is held to 128 with 6-24
            // spilled: 512 taxa x 1500 trees with 10 % of the taxa dropped 64.95 -> 63.7 ms (profiles/r06_experiments.md 3)
            const bool lone_bp4 = ks.size() == 1 && bb <= 5 && d.class_mode[ks[0]] == MODE_BINARY_PARTIAL;   // (5 bits: 4 waves instead of the one-class instance's 3)
            if (ks.size() < 2 && !lone_bp4) continue;
            Launch L{KERNEL_FUSED, (int)bb, {}};
            for (uint32_t k : ks) { L.segs.push_back(bitslice_seg(c, slot_lo(k), d.class_end[k] - slot_lo(k), (int)d.class_mode[k], bb)); done[k] = true; }
            const int rc = run_and_name(L);
            if (rc != QS_OK) return rc;
            ++fused_launch_groups;
        }
        // ---- the other classes one by one: count_bitslice3_kernel on the compact panel, beyond its 10 depth bits the byte-SWAR kernel ----
        for (uint32_t k = 0; k < n_cls; ++k) {
            if (done[k]) continue;
            const uint32_t s_lo = all_swar ? 0u : slot_lo(k), trees = (all_swar ? d.n_trees : d.class_end[k]) - s_lo;
            const uint32_t depth_bits = all_swar ? 11u : d.class_bits[k];   // 11 = beyond the bit-sliced instances
            int mode = all_swar ? batch_mode : (int)d.class_mode[k];
            Launch L{KERNEL_BITSLICE3, (int)depth_bits, {}};
            if (depth_bits <= top_bits) L.segs.push_back(bitslice_seg(c, s_lo, trees, mode, depth_bits));
            else {
                // the byte-SWAR kernel has no binary_partial instance: such trees are exact under its partial mode
                if (mode == MODE_BINARY_PARTIAL) mode = MODE_PARTIAL;
                const bool part = mode == MODE_PARTIAL;
                const uint32_t cls_max_depth = all_swar ? d.max_depth : d.class_max_depth[k];
                if (cls_max_depth <= (part ? kMaxDepthU8Partial : kMaxDepthU8Full)) L.bits = 8;
                else if (cls_max_depth <= (part ? kMaxDepthU16Partial : kMaxDepthU16Full)) L.bits = 16;
                else return fail(c, QS_ERR_UNSUPPORTED, "qs_count_batch: tree depth " + std::to_string(cls_max_depth) + " exceeds the panel range; re-root the tree at its centre");
                L.kernel = KERNEL_SWAR;
                L.segs.push_back(Seg{s_lo, trees, mode, part, 0u, 16u / (uint32_t)(L.bits / 8), (size_t)binom2(c->n) * 16});   // 16 bytes per (pair, group)
            }
            const int rc = run_and_name(L);
            if (rc != QS_OK) return rc;
            // tiles with two a-blocks of binary_full classes: count_bitslice4_kernel (it carries at most 7 planes)
            any_coop = any_coop || (L.kernel == KERNEL_BITSLICE3 && mode == MODE_BINARY_FULL && c->n_coop && depth_bits <= 7);
        }
        const int one_mode = all_swar ? batch_mode : (int)d.class_mode[0];
        c->variant = std::string("gather/") + (mixed ? "mixed" : mode_names[(!all_swar && d.class_bits[0] > top_bits && one_mode == MODE_BINARY_PARTIAL) ? (int)MODE_PARTIAL : one_mode]) + "/" + names + "/count_u" + std::to_string(c->count_bits);
        if (fused_launch_groups) c->variant += "/fused:" + std::to_string(fused_launch_groups);   // depth-bits groups whose classes shared a launch (count_bitslice3_fused_kernel)
        if (any_coop) c->variant += "/coop4";
        if (!all_swar && d.n_fix) c->variant += "/clamp:" + std::to_string(d.clamped_trees);   // trees counted below their own depth bits + clamp_fix_kernel
        if (c->last_splits) c->variant += "/overlap:" + std::to_string(c->last_split);           // slices split at that largest id: corrections beside the lower count launch
    } else if (algo == QS_ALGO_SCATTER) {
        if (!d.node_off) return fail(c, QS_ERR_ARG, "qs_count_batch: QS_ALGO_SCATTER needs node_off/rng_off/ranges in the batch");
        if (c->n > 4096) return fail(c, QS_ERR_UNSUPPORTED, "scatter: n too large");
        QS_HIP(c, launch_count_scatter(c->stream, d, c->n, c->d_lo, c->d_hi, c->rank_lo, c->table, (int)c->count_bits, c->dev_flags.get()));
        if (timed) QS_HIP(c, mark(c, 1));
        c->variant = std::string("scatter/atomic/count_u") + std::to_string(c->count_bits);
    } else {
        return fail(c, QS_ERR_ARG, "qs_count_batch: unknown algo");
    }
    c->last_timed = timed;
    c->trees_counted = (overwrite ? 0 : c->trees_counted) + d.n_trees;
    return QS_OK;
}

extern "C" int qs_sync(qs_ctx *c) {
    if (!c) return QS_ERR_ARG;
    QS_HIP(c, hipSetDevice(c->device));
    QS_HIP(c, hipStreamSynchronize(c->stream));
    uint32_t fl[4] = {0, 0, 0, 0};
    QS_HIP(c, hipMemcpy(fl, c->dev_flags.get(), 16, hipMemcpyDeviceToHost));
    if (fl[0]) {
        (void)hipMemset(c->dev_flags.get(), 0, 4);
        return fail(c, QS_ERR_OVERFLOW, "count table overflow: a counter exceeded count_bits");
    }
    if (fl[3]) {
        (void)hipMemset(c->dev_flags.get() + 3, 0, 4);
        return fail(c, QS_ERR_STATE, "two-cell wire format: a tuple does not sum to the number of trees (the batch was not binary with all taxa)");
    }
    return QS_OK;
}

extern "C" int qs_count_trees(qs_ctx *c, const qs_tree_batch *batch, uint32_t algo) {
    qs_device_batch *b = nullptr;
    int rc = qs_batch_upload(c, batch, &b);
    if (rc != QS_OK) return rc;
    rc = qs_count_batch(c, b, algo);
    int rc2 = qs_sync(c);
    qs_batch_free(c, b);
    return rc != QS_OK ? rc : rc2;
}

extern "C" int qs_last_count_ms(qs_ctx *c, float out_ms[3]) {
    if (!c || !c->last_timed || c->ev_used < 2) return fail(c, QS_ERR_STATE, "qs_last_count_ms: the last qs_count_batch did not carry QS_COUNT_TIMED");
    QS_HIP(c, hipEventSynchronize(c->evs[c->ev_used - 1]));
    out_ms[0] = out_ms[1] = 0.f;
    for (uint32_t i = 1; i < c->ev_used; ++i) {
        float ms = 0.f;
        if (c->ev_kind[i] == 3) continue;      // (a wait for the correction stream or the set-up of a new split, not a kernel of the step)
        QS_HIP(c, hipEventElapsedTime(&ms, c->evs[c->ev_from[i]], c->evs[i]));
        out_ms[c->ev_kind[i] ? 1 : 0] += ms;   // (the depth-clamp corrections count as count-kernel time: qs_last_count_fix_ms has their share; those of a
                                               // split slice's upper range run beside its lower count launch, so the kernels may sum to more than [2])
    }
    QS_HIP(c, hipEventElapsedTime(&out_ms[2], c->evs[0], c->evs[c->ev_used - 1]));
    return QS_OK;
}

extern "C" int qs_last_count_launches(const qs_ctx *c) {
    if (!c || !c->last_timed) return 0;
    int k = 0;
    for (uint32_t i = 1; i < c->ev_used; ++i) k += c->ev_kind[i] == 1 ? 1 : 0;
    return k;
}

extern "C" float qs_last_count_fix_ms(qs_ctx *c) {
    if (!c || !c->last_timed || c->ev_used < 2) return 0.f;
    if (hipEventSynchronize(c->evs[c->ev_used - 1]) != hipSuccess) return 0.f;
    float sum = 0.f;
    for (uint32_t i = 1; i < c->ev_used; ++i) {
        float ms = 0.f;
        if (c->ev_kind[i] == 2 && hipEventElapsedTime(&ms, c->evs[c->ev_from[i]], c->evs[i]) == hipSuccess) sum += ms;
    }
    return sum;
}

extern "C" int qs_last_count_events(qs_ctx *c, float *ms, uint8_t *kind, int cap) {
    if (!c || !c->last_timed || c->ev_used < 2) return 0;
    if (hipEventSynchronize(c->evs[c->ev_used - 1]) != hipSuccess) return 0;
    int k = 0;
    for (uint32_t i = 1; i < c->ev_used && k < cap; ++i) {
        if (c->ev_kind[i] == 3) continue;   // (a wait for the correction stream or the set-up of a new split, not a kernel of the step)
        float t = 0.f;
        (void)hipEventElapsedTime(&t, c->evs[c->ev_from[i]], c->evs[i]);
        if (ms) ms[k] = t;
        if (kind) kind[k] = c->ev_kind[i] == 4 ? 1 : c->ev_kind[i];   // (the second count launch of a split slice is a count kernel)
        ++k;
    }
    return k;
}

extern "C" int qs_batch_clamp_info(const qs_device_batch *b, uint64_t out[3]) {
    if (!b || !out) return QS_ERR_ARG;
    out[0] = b->d.clamped_trees; out[1] = b->d.fix_quartets; out[2] = b->d.n_fix;
    return QS_OK;
}

extern "C" const char *qs_last_count_variant(const qs_ctx *c) { return c ? c->variant.c_str() : ""; }

extern "C" int qs_last_count_split(const qs_ctx *c, uint32_t *n_slices) {
    if (n_slices) *n_slices = c ? c->last_splits : 0;
    return c ? (int)c->last_split : 0;
}

extern "C" int qs_lookup(qs_ctx *c, uint64_t nq, const uint16_t *abcd, uint64_t *out3) {
    if (!c || !c->table) return fail(c, QS_ERR_STATE, "qs_lookup: no table");
    if (nq == 0) return QS_OK;
    if (!abcd || !out3) return fail(c, QS_ERR_ARG, "qs_lookup: NULL");
    for (uint64_t i = 0; i < nq * 4; ++i)
        if (abcd[i] >= c->n) return fail(c, QS_ERR_ARG, "qs_lookup: id out of range");
    QS_HIP(c, hipSetDevice(c->device));
    DevBuf<uint16_t> dq; DevBuf<uint64_t> dout;   // (freed on every way out; hipFree waits for the device)
    QS_HIP(c, dq.reserve(nq * 8, nullptr));
    if (dout.reserve(nq * 24, nullptr) != hipSuccess) return fail(c, QS_ERR_OOM, "qs_lookup: hipMalloc");
    hipError_t e = hipMemcpyAsync(dq.get(), abcd, nq * 8, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = launch_lookup(c->stream, c->n, c->d_lo, c->d_hi, c->rank_lo, c->table, (int)c->count_bits, nq, dq.get(), dout.get());
    if (e == hipSuccess) e = hipMemcpyAsync(out3, dout.get(), nq * 24, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, QS_ERR_HIP, std::string("qs_lookup: ") + hipGetErrorString(e));
    return QS_OK;
}

// ---- scoring -----------------------------------------------------------------------------

// QuartetScoreComputer.hpp:135-159, evaluated with the host's libm like the reference.
static double host_log_score(uint64_t q1, uint64_t q2, uint64_t q3) {
    if (q1 == 0 && q2 == 0 && q3 == 0) return 0;
    uint64_t sum = q1 + q2 + q3;
    double p1 = (double)q1 / sum, p2 = (double)q2 / sum, p3 = (double)q3 / sum;
    double qic = 1;
    if (p1 != 0) qic += p1 * std::log(p1) / std::log(3);
    if (p2 != 0) qic += p2 * std::log(p2) / std::log(3);
    if (p3 != 0) qic += p3 * std::log(p3) / std::log(3);
    return (q1 < q2 || q1 < q3) ? qic * -1 : qic;
}


// the checks of a flattened reference tree, its depths, children counts and the id interval of every node
static int build_ref_shape(qs_ctx *c, const qs_ref_tree *ref, RefHost &R) {
    if (!ref || !ref->parent || !ref->leaf_node) return fail(c, QS_ERR_ARG, "reference tree: NULL arrays");
    if (c && ref->n_taxa != c->n) return fail(c, QS_ERR_ARG, "reference tree: n_taxa differs from the context");
    const uint32_t N = ref->n_nodes, n = ref->n_taxa;
    if (N < n + 1 || N > 65535) return fail(c, QS_ERR_ARG, "reference tree: bad node count");
    R.n_nodes = N; R.n = n;
    R.parent.assign(ref->parent, ref->parent + N);
    R.nchild.assign(N, 0); R.depth.assign(N, 0);
    int root = -1;
    for (uint32_t v = 0; v < N; ++v) {
        int p = R.parent[v];
        if (p < 0) { if (root >= 0) return fail(c, QS_ERR_ARG, "reference tree: several roots"); root = (int)v; }
        else if ((uint32_t)p >= N || (uint32_t)p == v) return fail(c, QS_ERR_ARG, "reference tree: bad parent");
        else R.nchild[p]++;
    }
    if (root < 0) return fail(c, QS_ERR_ARG, "reference tree: no root");
    R.root = (uint32_t)root;
    // depths (parents may come after children in the numbering: iterate with memo)
    std::vector<int> dep(N, -1);
    dep[root] = 0;
    std::vector<uint32_t> chain;
    for (uint32_t v = 0; v < N; ++v) {
        chain.clear();
        uint32_t x = v;
        while (dep[x] < 0) { chain.push_back(x); x = (uint32_t)R.parent[x]; if (chain.size() > N) return fail(c, QS_ERR_ARG, "reference tree: cycle"); }
        int dd = dep[x];
        for (size_t i = chain.size(); i-- > 0;) dep[chain[i]] = ++dd;
    }
    for (uint32_t v = 0; v < N; ++v) R.depth[v] = (uint32_t)dep[v];
    std::vector<uint8_t> is_leaf_taxon(N, 0);
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t v = ref->leaf_node[i];
        if (v >= N || R.nchild[v] != 0 || is_leaf_taxon[v]) return fail(c, QS_ERR_ARG, "reference tree: leaf_node must list distinct leaves");
        is_leaf_taxon[v] = 1;
    }
    uint32_t n_leaf_nodes = 0;
    for (uint32_t v = 0; v < N; ++v) if (R.nchild[v] == 0) n_leaf_nodes++;
    if (n_leaf_nodes != n) return fail(c, QS_ERR_ARG, "reference tree: number of leaves differs from n_taxa");
    // depth-first order check: every node's leaves form one contiguous id interval
    std::vector<uint32_t> lo(N, 0xFFFFFFFFu), hi(N, 0), cnt(N, 0);
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t x = ref->leaf_node[i];
        for (;;) {
            lo[x] = std::min(lo[x], i); hi[x] = std::max(hi[x], i); cnt[x]++;
            if (R.parent[x] < 0) break;
            x = (uint32_t)R.parent[x];
        }
    }
    for (uint32_t v = 0; v < N; ++v)
        if (cnt[v] && hi[v] - lo[v] + 1 != cnt[v])
            return fail(c, QS_ERR_ARG, "reference tree: lookup ids are not in depth-first leaf order");
    // is_bifurcating: max over nodes of (degree - 1) == 2 (QuartetScoreComputer.hpp:760)
    uint32_t max_rank = 0;
    for (uint32_t v = 0; v < N; ++v) {
        uint32_t deg = R.nchild[v] + (R.parent[v] >= 0 ? 1 : 0);
        if (deg >= 1) max_rank = std::max(max_rank, deg - 1);
    }
    R.bifurcating = (max_rank == 2);
    R.leaf_lo = lo; R.leaf_cnt = cnt;
    return QS_OK;
}

static int build_ref(qs_ctx *c, const qs_ref_tree *ref, RefHost &R) {
    if (int rc = build_ref_shape(c, ref, R)) return rc;
    const uint32_t N = R.n_nodes, n = R.n;
    const std::vector<uint32_t> &lo = R.leaf_lo, &cnt = R.leaf_cnt;
    R.root_deg2 = R.nchild[R.root] == 2;
    R.inner_id.assign(N, 0xFFFFFFFFu);
    R.inner_node.clear();
    for (uint32_t v = 0; v < N; ++v)
        if (R.nchild[v] > 0) { R.inner_id[v] = (uint32_t)R.inner_node.size(); R.inner_node.push_back(v); }
    R.n_inner = (uint32_t)R.inner_node.size();
    // LCA of leaves with adjacent ids, then running minima per row
    std::vector<uint32_t> adj(n > 0 ? n - 1 : 0);
    for (uint32_t i = 0; i + 1 < n; ++i) {
        uint32_t x = ref->leaf_node[i], y = ref->leaf_node[i + 1];
        while (x != y) {
            if (R.depth[x] >= R.depth[y]) x = (uint32_t)R.parent[x]; else y = (uint32_t)R.parent[y];
        }
        adj[i] = x;
    }
    R.lca.assign((size_t)n * n, 0);
    for (uint32_t i = 0; i + 1 < n; ++i) {
        uint32_t cur = adj[i];
        for (uint32_t j = i + 1; j < n; ++j) {
            if (j > i + 1 && R.depth[adj[j - 1]] < R.depth[cur]) cur = adj[j - 1];
            uint32_t e = (R.depth[cur] << 16) | R.inner_id[cur];
            R.lca[(size_t)i * n + j] = e;
            R.lca[(size_t)j * n + i] = e;
        }
    }
    if (R.bifurcating && R.root_deg2) {
        // QuartetScoreComputer.hpp:390-410 for u = root: S1 = the root's other child subtree, S2 = the child subtree that
        // holds v, S3 / S4 = v's child subtrees in depth-first order; all of them intervals of lookup ids
        std::vector<std::vector<uint32_t>> kids(N);
        for (uint32_t v = 0; v < N; ++v) if (R.parent[v] >= 0) kids[(uint32_t)R.parent[v]].push_back(v);
        for (auto &k : kids) std::sort(k.begin(), k.end(), [&](uint32_t p_, uint32_t q_) { return lo[p_] < lo[q_]; });
        const uint32_t rx = kids[R.root][0], ry = kids[R.root][1];
        R.root_split = cnt[rx];
        for (uint32_t v = 0; v < N; ++v) {
            if (v == R.root || R.nchild[v] != 2) continue;
            const bool in_x = lo[v] >= lo[rx] && lo[v] < lo[rx] + cnt[rx];
            const uint32_t mine = in_x ? rx : ry, other = in_x ? ry : rx;
            RootPairHost P{};
            P.s1_lo = lo[other]; P.s1_n = cnt[other]; P.s2_lo = lo[mine]; P.s2_n = cnt[mine];
            P.s3_lo = lo[kids[v][0]]; P.s3_n = cnt[kids[v][0]]; P.s4_lo = lo[kids[v][1]]; P.s4_n = cnt[kids[v][1]];
            const uint32_t ir = R.inner_id[R.root], iv = R.inner_id[v];
            P.key = std::min(ir, iv) * R.n_inner + std::max(ir, iv);
            P.first = R.root_items;
            R.root_items += (uint64_t)P.s1_n * P.s2_n * P.s3_n * P.s4_n;
            R.root_pairs.push_back(P);
        }
    }
    R.next.assign((size_t)n * n, 0);
    for (uint32_t b = 1; b < n; ++b) {
        R.next[(size_t)b * n + (b - 1)] = (uint16_t)b;
        for (uint32_t a = b - 1; a-- > 0;)
            R.next[(size_t)b * n + a] = R.lca[(size_t)b * n + a] != R.lca[(size_t)b * n + a + 1] ? (uint16_t)(a + 1) : R.next[(size_t)b * n + a + 1];
    }
    return QS_OK;
}

// The context's cached reference tree (host arrays + LCA matrix on the device when want_dev); rebuilt only when the
// caller passes a different tree.
static int get_ref(qs_ctx *c, const qs_ref_tree *ref, bool want_dev, const RefHost **out) {
    if (!ref || !ref->parent || !ref->leaf_node) return fail(c, QS_ERR_ARG, "reference tree: NULL arrays");
    RefHost *R = c->ref_cache.get();
    const bool same = R && R->n_nodes == ref->n_nodes && R->n == ref->n_taxa &&
                      memcmp(R->parent.data(), ref->parent, (size_t)ref->n_nodes * 4) == 0 &&
                      memcmp(R->leaf_node_in.data(), ref->leaf_node, (size_t)ref->n_taxa * 4) == 0;
    if (!same) {
        std::unique_ptr<RefHost> fresh(new RefHost());
        int rc = build_ref(c, ref, *fresh);
        if (rc != QS_OK) return rc;
        fresh->leaf_node_in.assign(ref->leaf_node, ref->leaf_node + ref->n_taxa);
        if (c->ref_lca_dev) { (void)hipStreamSynchronize(c->stream); c->ref_lca_dev.reset(); c->ref_next_dev.reset(); c->root_pairs_dev.reset(); }
        if (c->place_child_dev) { (void)hipStreamSynchronize(c->stream); c->place_child_dev.reset(); c->place_next_dev.reset(); c->place_node_dev.reset(); }
        c->ref_cache = std::move(fresh);
        R = c->ref_cache.get();
        c->log_valid = false;
    }
    if (want_dev && !c->ref_lca_dev) {
        // The tree's device arrays are filled on the side and handed to the context together: ref_lca_dev says "all of them are
        // there", so a call that fails half-way leaves none behind (the context's own are empty here: nothing is held twice).
        DevBuf<uint32_t> lca; DevBuf<uint16_t> next; DevBuf<void> pairs;
        QS_HIP(c, lca.reserve(R->lca.size() * 4, nullptr));
        QS_HIP(c, next.reserve(R->next.size() * 2, nullptr));
        hipStream_t up = c->prep_stream ? c->prep_stream : c->stream;
        QS_HIP(c, hipMemcpyAsync(lca.get(), R->lca.data(), R->lca.size() * 4, hipMemcpyHostToDevice, up));
        QS_HIP(c, hipMemcpyAsync(next.get(), R->next.data(), R->next.size() * 2, hipMemcpyHostToDevice, up));
        if (!R->root_pairs.empty()) {
            QS_HIP(c, pairs.reserve(R->root_pairs.size() * sizeof(RootPairHost), nullptr));
            QS_HIP(c, hipMemcpyAsync(pairs.get(), R->root_pairs.data(), R->root_pairs.size() * sizeof(RootPairHost), hipMemcpyHostToDevice, up));
        }
        c->ref_lca_dev = std::move(lca); c->ref_next_dev = std::move(next); c->root_pairs_dev = std::move(pairs);
    }
    *out = R;
    return QS_OK;
}

// log(k) and 1/k for the integer arguments of the device QIC: every count and every tuple sum is at most the
// number of trees counted. Unknown (uploaded / attached tables, reduce-scattered shards): 65536 entries, larger
// values take the kernel's slow path.
static int ensure_score_tables(qs_ctx *c) {
    // every count and every tuple sum is at most the number of trees behind the table: what this context counted, or what
    // the caller says stands behind a reduced / uploaded / viewed table (QS_TUNE_TABLE_TREES)
    const uint64_t want64 = std::min<uint64_t>(std::max<uint64_t>(std::max(c->trees_counted, c->table_trees_hint) + 1, 65536), 1ull << 20);
    const uint32_t want = (uint32_t)want64;
    if (c->tbl_n >= want) return QS_OK;
    c->tbl_n = 0;   // (entries that are valid, not the capacity: set again once the new table is on the device)
    std::vector<double> lk(want);
    lk[0] = 0.0;
    for (uint32_t k = 1; k < want; ++k) lk[k] = std::log((double)k);
    QS_HIP(c, c->dev_logk.reserve((size_t)want * 8, &c->stream));
    {   // (not the null stream: that one waits for count kernels still running on `stream`)
        hipStream_t up = c->prep_stream ? c->prep_stream : c->stream;
        QS_HIP(c, hipMemcpyAsync(c->dev_logk.get(), lk.data(), (size_t)want * 8, hipMemcpyHostToDevice, up));
        QS_HIP(c, hipStreamSynchronize(up));
    }
    c->tbl_n = want;
    return QS_OK;
}

static void fill_score_device(const qs_ctx *c, const RefHost &R, const uint32_t *lca_dev, ScoreDevice &sd) {
    sd.logk = c->dev_logk.get(); sd.tbl_n = c->tbl_n;
    // as much of the log table as fits goes to LDS (every tuple sum of up to 15743 trees); larger arguments are range-checked
    sd.coop_load = c->tune_score_load;
    sd.lds_n = (uint32_t)std::min<uint64_t>(c->tbl_n, score_scan_max_lds_log((c->tune_score_load == 1 || c->tune_score_load == 3) && c->tune_score_kernel == 0));
    sd.ref_lca = lca_dev; sd.ref_next = c->ref_next_dev.get(); sd.n = c->n; sd.n_inner = R.n_inner; sd.d_lo = c->d_lo; sd.d_hi = c->d_hi;
    sd.rank_lo = c->rank_lo; sd.n_tuples = c->n_tuples; sd.table = c->table; sd.count_bits = (int)c->count_bits;
    if (c->view_table) { sd.rank_lo = c->view_rank_lo; sd.n_tuples = c->view_n; sd.table = const_cast<void *>(c->view_table); sd.count_bits = (int)c->view_bits; }
    sd.pair_sums = nullptr; sd.pair_min = nullptr; sd.pair_cand = nullptr; sd.flags = c->dev_flags.get() + 1;
    sd.cand_limit = c->tune_cand_slots; sd.list = nullptr; sd.list_count = nullptr; sd.list_cap = 0; sd.last_trip = nullptr;
    sd.frame = R.bifurcating ? 0 : 1;
    sd.root_split = (R.bifurcating && R.root_deg2) ? R.root_split : 0u;
    sd.bundle_plo = sd.bundle_pcnt = sd.bundle_rounds = nullptr; sd.n_rounds = 0; sd.sample = 0;
}

// the bundle kernel's rounds for the rank range sd covers (own table, table shard or view): planned on the host, cached;
// pass 3 = the per-taxon pass (qs_taxon_support: its own slot and wave count, whatever the score tuning says)
static int ensure_bundle_plan(qs_ctx *c, ScoreDevice &sd, int pass) {
    sd.bundle_plo = sd.bundle_pcnt = sd.bundle_rounds = nullptr; sd.n_rounds = 0;
    if (c->tune_score_kernel == 1 && pass != 3) return QS_OK;
    if (c->n_cu == 0) { int v = 0; QS_HIP(c, hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, c->device)); c->n_cu = std::max(1, v); }
    const int w = pass - 1;
    BundlePlan &plan = c->bundle[w];
    const uint64_t r0 = sd.rank_lo, r1 = sd.rank_lo + sd.n_tuples;
    if (c->bundle_r0[w] != r0 || c->bundle_r1[w] != r1 || !c->bundle_dev[w]) {
        // (a new plan gets a table of its own size, never the old one's memory: kernels on `stream` may read that while `up` writes)
        if (c->bundle_dev[w]) { QS_HIP(c, hipStreamSynchronize(c->stream)); c->bundle_dev[w].reset(); }
        plan_bundles(c->n, r0, r1, pass == 3 ? (uint32_t)kTaxonWaves : score_bundle_waves(pass, c->tune_score_load == 1 || c->tune_score_load == 3), plan);
        const size_t words = 2 * (size_t)c->n + plan.rounds.size();
        if (c->bundle_dev[w].reserve(std::max<size_t>(words, 1) * 4, nullptr) != hipSuccess) return fail(c, QS_ERR_OOM, "qs_score: round table of the bundle kernel");
        uint32_t *const dev = c->bundle_dev[w].get();
        hipStream_t up = c->prep_stream ? c->prep_stream : c->stream;
        QS_HIP(c, hipMemcpyAsync(dev, plan.plo.data(), (size_t)c->n * 4, hipMemcpyHostToDevice, up));
        QS_HIP(c, hipMemcpyAsync(dev + c->n, plan.pcnt.data(), (size_t)c->n * 4, hipMemcpyHostToDevice, up));
        if (!plan.rounds.empty())
            QS_HIP(c, hipMemcpyAsync(dev + 2 * (size_t)c->n, plan.rounds.data(), plan.rounds.size() * 4, hipMemcpyHostToDevice, up));
        QS_HIP(c, hipStreamSynchronize(up));   // (the host vectors may be re-planned by the next call)
        c->bundle_r0[w] = r0; c->bundle_r1[w] = r1;
    }
    sd.bundle_plo = c->bundle_dev[w].get(); sd.bundle_pcnt = sd.bundle_plo + c->n; sd.bundle_rounds = sd.bundle_plo + 2 * (size_t)c->n;
    sd.n_rounds = (uint32_t)(plan.rounds.size() / 2);
    return QS_OK;
}

// Per-taxon quartet support of this context's table against the reference tree (qs_taxon.hip). The reference has no such
// output: this replaces nothing there (the nearest is printRawQICScores, one text line per quartet).
extern "C" int qs_taxon_support(qs_ctx *c, const qs_ref_tree *ref, int64_t *dst_device) {
    if (!c) return QS_ERR_ARG;
    if (!dst_device) return fail(c, QS_ERR_ARG, "qs_taxon_support: NULL argument");
    if (reinterpret_cast<uintptr_t>(dst_device) % 8) return fail(c, QS_ERR_ARG, "qs_taxon_support: dst_device is not 8-byte aligned");
    if (!c->table) return fail(c, QS_ERR_STATE, "qs_taxon_support: no table");
    if (taxon_lds_bytes(c->n) > 160u * 1024u) return fail(c, QS_ERR_UNSUPPORTED, "qs_taxon_support: more than 3413 taxa (the accumulators of a workgroup live in LDS)");
    // every sum is at most C(n-1,3) x (largest count): the trees behind the table if known, else what a cell can hold
    const uint64_t cell_max = c->count_bits == 16 ? 0xFFFFull : 0xFFFFFFFFull;
    const uint64_t trees = std::max(c->trees_counted, c->table_trees_hint);
    const uint64_t max_count = trees ? std::min(trees, cell_max) : cell_max;
    const uint64_t per_taxon = c->n >= 4 ? (uint64_t)(c->n - 1) * (c->n - 2) / 2 * (c->n - 3) / 3 : 0;
    if (per_taxon && max_count > (uint64_t)INT64_MAX / per_taxon)
        return fail(c, QS_ERR_OVERFLOW, "qs_taxon_support: C(n-1,3) x the largest possible count exceeds 63 bits");
    QS_HIP(c, hipSetDevice(c->device));
    const RefHost *Rp = nullptr;
    if (int rc = get_ref(c, ref, true, &Rp)) return rc;
    ScoreDevice sd;
    fill_score_device(c, *Rp, c->ref_lca_dev.get(), sd);
    sd.rank_lo = c->rank_lo; sd.n_tuples = c->n_tuples; sd.table = c->table; sd.count_bits = (int)c->count_bits;   // the context's own table, not a scoring view
    sd.flags = nullptr;
    if (int rc = ensure_bundle_plan(c, sd, 3)) return rc;
    // (a context's table is cut by the largest id: it starts and ends at a row start, plan_bundles finds no partial rows)
    if (c->bundle[2].n_parts) return fail(c, QS_ERR_UNSUPPORTED, "qs_taxon_support: the table does not start and end at a row start");
    QS_HIP(c, hipMemsetAsync(dst_device, 0, (size_t)c->n * 6 * 8, c->stream));
    const bool wide = max_count >= (1ull << 32) / 192;   // 64 lanes x 3 counts in a 32-bit partial sum
    QS_HIP(c, launch_taxon_support(c->stream, sd, wide, c->n_cu, reinterpret_cast<unsigned long long *>(dst_device)));
    return QS_OK;   // asynchronous on the context's stream
}

// qs_taxon_placement: the link lookups of the cached reference tree on the device, beside its LCA matrix
static int ensure_place_ref(qs_ctx *c, const RefHost &R) {
    if (c->place_child_dev) return QS_OK;
    const uint32_t n = R.n;
    uint32_t max_depth = 0;
    for (uint32_t d : R.depth) max_depth = std::max(max_depth, d);
    // child[i][j] = the child of lca(i,j) that holds leaf j: j's ancestor one level below the LCA
    c->place_child.assign((size_t)n * n, 0);
    std::vector<uint32_t> at_depth(max_depth + 2, 0);
    for (uint32_t j = 0; j < n; ++j) {
        for (uint32_t v = R.leaf_node_in[j];; v = (uint32_t)R.parent[v]) { at_depth[R.depth[v]] = v; if (R.parent[v] < 0) break; }
        for (uint32_t i = 0; i < n; ++i)
            if (i != j) c->place_child[(size_t)i * n + j] = (uint16_t)at_depth[(R.lca[(size_t)i * n + j] >> 16) + 1];
    }
    // next[q][p], p < q: the end of the run of p over which lca(p,q) AND the child of it that holds p stay the same
    c->place_next.assign((size_t)n * n, 0);
    for (uint32_t q = 1; q < n; ++q) {
        const size_t o = (size_t)q * n;
        c->place_next[o + q - 1] = (uint16_t)q;
        for (uint32_t p = q - 1; p-- > 0;)
            c->place_next[o + p] = (R.lca[o + p] != R.lca[o + p + 1] || c->place_child[o + p] != c->place_child[o + p + 1]) ? (uint16_t)(p + 1) : c->place_next[o + p + 1];
    }
    DevBuf<uint16_t> child, next; DevBuf<uint32_t> node;
    QS_HIP(c, child.reserve(c->place_child.size() * 2, nullptr));
    QS_HIP(c, next.reserve(c->place_next.size() * 2, nullptr));
    QS_HIP(c, node.reserve(std::max<size_t>(R.inner_node.size(), 1) * 4, nullptr));
    QS_HIP(c, hipMemcpyAsync(child.get(), c->place_child.data(), c->place_child.size() * 2, hipMemcpyHostToDevice, c->stream));
    QS_HIP(c, hipMemcpyAsync(next.get(), c->place_next.data(), c->place_next.size() * 2, hipMemcpyHostToDevice, c->stream));
    QS_HIP(c, hipMemcpyAsync(node.get(), R.inner_node.data(), R.inner_node.size() * 4, hipMemcpyHostToDevice, c->stream));
    c->place_child_dev = std::move(child); c->place_next_dev = std::move(next); c->place_node_dev = std::move(node);
    return QS_OK;
}

// Link sums of the quartet placement of the listed taxa (qs_place.hip). The reference never asks where the evaluation trees would
// put a taxon: this replaces nothing there.
extern "C" int qs_taxon_placement(qs_ctx *c, const qs_ref_tree *ref, const uint16_t *taxa, uint32_t n_list, int64_t *dst_device) {
    if (!c) return QS_ERR_ARG;
    if (!dst_device) return fail(c, QS_ERR_ARG, "qs_taxon_placement: NULL argument");
    if (reinterpret_cast<uintptr_t>(dst_device) % 8) return fail(c, QS_ERR_ARG, "qs_taxon_placement: dst_device is not 8-byte aligned");
    if (!c->table) return fail(c, QS_ERR_STATE, "qs_taxon_placement: no table");
    // every sum is at most C(n-1,3) x (largest count): the trees behind the table if known, else what a cell can hold (as qs_taxon_support)
    const uint64_t cell_max = c->count_bits == 16 ? 0xFFFFull : 0xFFFFFFFFull;
    const uint64_t trees = std::max(c->trees_counted, c->table_trees_hint);
    const uint64_t max_count = trees ? std::min(trees, cell_max) : cell_max;
    const uint64_t per_taxon = c->n >= 4 ? (uint64_t)(c->n - 1) * (c->n - 2) / 2 * (c->n - 3) / 3 : 0;
    if (per_taxon && max_count > (uint64_t)INT64_MAX / per_taxon)
        return fail(c, QS_ERR_OVERFLOW, "qs_taxon_placement: C(n-1,3) x the largest possible count exceeds 63 bits");
    if (c->d_lo != 0 || c->d_hi != c->n) return fail(c, QS_ERR_UNSUPPORTED, "qs_taxon_placement: a table-shard context (the walks of a taxon cross every shard: use a whole-table one)");
    if (taxa ? n_list == 0 || n_list > c->n : n_list != c->n) return fail(c, QS_ERR_ARG, taxa ? "qs_taxon_placement: the list needs 1 .. n_taxa entries" : "qs_taxon_placement: n_list must be n_taxa when taxa is NULL");
    std::vector<uint16_t> list(n_list);
    {
        std::vector<uint8_t> seen(c->n, 0);
        for (uint32_t i = 0; i < n_list; ++i) {
            const uint32_t x = taxa ? taxa[i] : i;
            if (x >= c->n) return fail(c, QS_ERR_ARG, "qs_taxon_placement: taxon id out of range");
            if (seen[x]) return fail(c, QS_ERR_ARG, "qs_taxon_placement: taxon id " + std::to_string(x) + " is listed twice");
            seen[x] = 1; list[i] = (uint16_t)x;
        }
    }
    QS_HIP(c, hipSetDevice(c->device));
    const RefHost *Rp = nullptr;
    if (int rc = get_ref(c, ref, true, &Rp)) return rc;
    if (place_lds_bytes(Rp->n_nodes) > 160u * 1024u)
        return fail(c, QS_ERR_UNSUPPORTED, "qs_taxon_placement: more than 10240 nodes (the link sums of a workgroup live in LDS)");
    if (int rc = ensure_place_ref(c, *Rp)) return rc;
    if (c->n_cu == 0) { int v = 0; QS_HIP(c, hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, c->device)); c->n_cu = std::max(1, v); }
    if (!c->place_tasks_dev) {
        // a walk = (middle id q, 64 consecutive largest ids): q steps; the long ones first
        c->place_tasks.clear();
        for (uint32_t q = c->n - 2; q >= 1; --q)
            for (uint32_t g = 0; q + 1 + g * kWave < c->n; ++g) c->place_tasks.push_back(q | g << 16);
        QS_HIP(c, c->place_tasks_dev.reserve(c->place_tasks.size() * 4, nullptr));
        QS_HIP(c, hipMemcpyAsync(c->place_tasks_dev.get(), c->place_tasks.data(), c->place_tasks.size() * 4, hipMemcpyHostToDevice, c->stream));
    }
    if (list != c->place_taxa || !c->place_taxa_dev) {
        QS_HIP(c, hipStreamSynchronize(c->stream));   // (an earlier call's kernel and upload may still read the old list)
        c->place_taxa = list;
        QS_HIP(c, c->place_taxa_dev.reserve((size_t)c->n * 2, nullptr));
        QS_HIP(c, hipMemcpyAsync(c->place_taxa_dev.get(), c->place_taxa.data(), (size_t)n_list * 2, hipMemcpyHostToDevice, c->stream));
    }
    PlaceDevice pd;
    pd.ref_lca = c->ref_lca_dev.get(); pd.inner_node = c->place_node_dev.get(); pd.tasks = c->place_tasks_dev.get();
    pd.child = c->place_child_dev.get(); pd.next = c->place_next_dev.get(); pd.taxa = c->place_taxa_dev.get();
    pd.n = c->n; pd.n_nodes = Rp->n_nodes; pd.n_tasks = (uint32_t)c->place_tasks.size();
    pd.table = c->table; pd.count_bits = (int)c->count_bits;   // the context's own table, not a scoring view
    QS_HIP(c, hipMemsetAsync(dst_device, 0, (size_t)n_list * 2 * Rp->n_nodes * 8, c->stream));
    // 32-bit partial sums: a walk has q < n_taxa steps, so 4096 x (largest count) < 2^32 suffices only while n_taxa <= 4096
    // (qs_create's cap today; the LDS limit alone would allow more)
    const bool wide = max_count >= (1ull << 32) / 4096 || c->n > 4096;
    QS_HIP(c, launch_taxon_placement(c->stream, pd, n_list, wide, c->n_cu, reinterpret_cast<unsigned long long *>(dst_device)));
    return QS_OK;   // asynchronous on the context's stream
}

// Link sums of the quartet placement of the listed clades (qs_place_clade.hip): the clade below a node is pruned and regrafted, unchanged
// inside, on every edge outside it. The reference never asks where the evaluation trees would put a subtree: this replaces nothing there.
extern "C" int qs_clade_placement(qs_ctx *c, const qs_ref_tree *ref, const uint32_t *nodes, uint32_t n_list, int64_t *dst_device) {
    if (!c) return QS_ERR_ARG;
    if (!dst_device) return fail(c, QS_ERR_ARG, "qs_clade_placement: NULL argument");
    if (reinterpret_cast<uintptr_t>(dst_device) % 8) return fail(c, QS_ERR_ARG, "qs_clade_placement: dst_device is not 8-byte aligned");
    if (!c->table) return fail(c, QS_ERR_STATE, "qs_clade_placement: no table");
    if (!nodes || n_list == 0) return fail(c, QS_ERR_ARG, "qs_clade_placement: the list needs at least one node");
    // the list against the tree's shape, before anything touches the device
    const uint32_t n = c->n;
    std::vector<uint32_t> lo(n_list), hi(n_list);
    {
        RefHost S;
        if (int rc = build_ref_shape(c, ref, S)) return rc;
        std::vector<uint8_t> seen(S.n_nodes, 0);
        for (uint32_t i = 0; i < n_list; ++i) {
            const uint32_t v = nodes[i];
            if (v >= S.n_nodes) return fail(c, QS_ERR_ARG, "qs_clade_placement: node index out of range");
            if (v == S.root) return fail(c, QS_ERR_ARG, "qs_clade_placement: the root is not a clade to move");
            if (seen[v]) return fail(c, QS_ERR_ARG, "qs_clade_placement: node " + std::to_string(v) + " is listed twice");
            seen[v] = 1;
            lo[i] = S.leaf_lo[v]; hi[i] = lo[i] + S.leaf_cnt[v];
            if (n - S.leaf_cnt[v] < 3) return fail(c, QS_ERR_ARG, "qs_clade_placement: node " + std::to_string(v) + " leaves fewer than three taxa outside it");
        }
    }
    // every sum is at most |C| x C(n-|C|,3) x (largest count): the trees behind the table if known, else what a cell can hold (as qs_taxon_support)
    const uint64_t cell_max = c->count_bits == 16 ? 0xFFFFull : 0xFFFFFFFFull;
    const uint64_t trees = std::max(c->trees_counted, c->table_trees_hint);
    const uint64_t max_count = trees ? std::min(trees, cell_max) : cell_max;
    std::vector<uint64_t> cost(n_list);
    for (uint32_t i = 0; i < n_list; ++i) {
        const uint64_t s = hi[i] - lo[i], o = n - s;
        cost[i] = s * (o * (o - 1) / 2 * (o - 2) / 3);        // (n <= 65535: below 2^62)
        if (max_count > (uint64_t)INT64_MAX / cost[i])
            return fail(c, QS_ERR_OVERFLOW, "qs_clade_placement: |C| x C(n-|C|,3) x the largest possible count exceeds 63 bits for node " + std::to_string(nodes[i]));
    }
    if (c->d_lo != 0 || c->d_hi != c->n) return fail(c, QS_ERR_UNSUPPORTED, "qs_clade_placement: a table-shard context (the walks of a clade cross every shard: use a whole-table one)");
    if (place_lds_bytes(ref->n_nodes) > 160u * 1024u)
        return fail(c, QS_ERR_UNSUPPORTED, "qs_clade_placement: more than 10240 nodes (the link sums of a workgroup live in LDS)");
    QS_HIP(c, hipSetDevice(c->device));
    const RefHost *Rp = nullptr;
    if (int rc = get_ref(c, ref, true, &Rp)) return rc;
    if (int rc = ensure_place_ref(c, *Rp)) return rc;
    if (c->n_cu == 0) { int v = 0; QS_HIP(c, hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, c->device)); c->n_cu = std::max(1, v); }
    if (!c->clade_tasks_dev) {
        // a walk = (middle id, 64 consecutive largest ids) among the ids outside a clade, named by d = the outside ids above the middle
        // one: a clade with `o` taxa outside owns the entries with d <= o - 2, and the smallest d are its longest walks
        c->clade_tasks.clear();
        for (uint32_t d = 1; d + 2 <= n; ++d)
            for (uint32_t g = 0; g * kWave < d; ++g) c->clade_tasks.push_back(d | g << 16);
        QS_HIP(c, c->clade_tasks_dev.reserve(std::max<size_t>(c->clade_tasks.size(), 1) * 4, nullptr));
        QS_HIP(c, hipMemcpyAsync(c->clade_tasks_dev.get(), c->clade_tasks.data(), c->clade_tasks.size() * 4, hipMemcpyHostToDevice, c->stream));
    }
    // per clade: its x-slices and its share of about eight workgroups per CU, in proportion to its tuples
    // 32-bit register sums: a walk has at most n - |C| - 2 steps of `slice` tuples each, so (n - |C|) x slice x (largest count) < 2^32
    // keeps them exact; slices are shortened to stay below, and the 64-bit instance takes over where that would cut a clade
    // into slices of fewer than 16 taxa
    bool wide = false;
    for (uint32_t i = 0; i < n_list && !wide; ++i) {
        const uint64_t s = hi[i] - lo[i], cap = 0xFFFFFFFFull / (max_count * (n - s));
        wide = cap < std::min<uint64_t>(s, 16);
    }
    long double total_cost = 0;
    for (uint64_t v : cost) total_cost += (long double)v;
    const uint32_t budget = (uint32_t)c->n_cu * 8u;
    std::vector<uint32_t> list((size_t)n_list * 4), groups;
    for (uint32_t i = 0; i < n_list; ++i) {
        const uint32_t s = hi[i] - lo[i], o = n - s;
        uint64_t walks = 0;
        for (uint32_t d = 1; d + 2 <= o; ++d) walks += (d + kWave - 1) / kWave;
        uint32_t share = (uint32_t)std::min<long double>(65535.0L, std::max<long double>(1.0L, (long double)budget * (long double)cost[i] / total_cost + 0.5L));
        // about four items per wave of the share, from slices of at least 16 taxa
        uint64_t n_slices = std::max<uint64_t>(1, std::min<uint64_t>(s / 16, ((uint64_t)share * kPlaceWaves * 4 + walks - 1) / walks));
        uint32_t slice = (uint32_t)((s + n_slices - 1) / n_slices);
        if (!wide) slice = (uint32_t)std::min<uint64_t>(slice, 0xFFFFFFFFull / (max_count * o));
        n_slices = (s + slice - 1) / slice;
        share = (uint32_t)std::min<uint64_t>(share, (walks * n_slices + kPlaceWaves - 1) / kPlaceWaves);
        list[4 * (size_t)i] = lo[i]; list[4 * (size_t)i + 1] = hi[i]; list[4 * (size_t)i + 2] = slice; list[4 * (size_t)i + 3] = (uint32_t)walks;
        for (uint32_t k = 0; k < share; ++k) { groups.push_back(i); groups.push_back(k | share << 16); }
    }
    const uint32_t n_groups = (uint32_t)(groups.size() / 2);
    list.insert(list.end(), groups.begin(), groups.end());
    QS_HIP(c, hipStreamSynchronize(c->stream));   // (an earlier call's kernel and upload may still read the old lists)
    c->clade_list = std::move(list);
    QS_HIP(c, c->clade_list_dev.reserve(c->clade_list.size() * 4, nullptr));
    QS_HIP(c, hipMemcpyAsync(c->clade_list_dev.get(), c->clade_list.data(), c->clade_list.size() * 4, hipMemcpyHostToDevice, c->stream));
    CladeDevice cd;
    cd.ref_lca = c->ref_lca_dev.get(); cd.inner_node = c->place_node_dev.get(); cd.tasks = c->clade_tasks_dev.get();
    cd.clades = c->clade_list_dev.get(); cd.groups = cd.clades + (size_t)n_list * 4;
    cd.child = c->place_child_dev.get(); cd.next = c->place_next_dev.get();
    cd.n = c->n; cd.n_nodes = Rp->n_nodes;
    cd.table = c->table; cd.count_bits = (int)c->count_bits;   // the context's own table, not a scoring view
    QS_HIP(c, hipMemsetAsync(dst_device, 0, (size_t)n_list * 2 * Rp->n_nodes * 8, c->stream));
    QS_HIP(c, launch_clade_placement(c->stream, cd, n_groups, wide, reinterpret_cast<unsigned long long *>(dst_device)));
    return QS_OK;   // asynchronous on the context's stream
}

// Host-only: the link sums of one taxon -> the placement score of every edge, by the preorder recurrence S(v) = S(parent v) -
// W[N + parent v] + W[v] with S(root) = the sum of W over all parent links. No device, no context.
extern "C" int qs_placement_scores(const qs_ref_tree *ref, const int64_t *links_host, int64_t *scores_host) {
    if (!links_host || !scores_host) return fail(nullptr, QS_ERR_ARG, "qs_placement_scores: NULL argument");
    RefHost R;
    if (int rc = build_ref_shape(nullptr, ref, R)) return rc;
    const uint32_t N = R.n_nodes;
    std::vector<uint32_t> order(N);
    for (uint32_t v = 0; v < N; ++v) order[v] = v;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return R.depth[a] < R.depth[b]; });   // parents first
    int64_t tot_up = 0;
    for (uint32_t v = 0; v < N; ++v) tot_up += links_host[N + v];
    scores_host[R.root] = tot_up;
    for (uint32_t v : order) {
        if (v == R.root) continue;
        const uint32_t p = (uint32_t)R.parent[v];
        scores_host[v] = scores_host[p] - links_host[N + p] + links_host[v];
    }
    scores_host[R.root] = 0;
    return QS_OK;
}

extern "C" int qs_score_plan(uint32_t n_taxa, uint64_t rank_lo, uint64_t n_tuples, uint32_t *first_pair, uint32_t *n_pairs, uint64_t parts[4]) {
    if (!first_pair || !n_pairs || !parts || n_taxa < 4 || n_taxa > 65535) return QS_ERR_ARG;
    if (rank_lo > binom4(n_taxa) || n_tuples > binom4(n_taxa) - rank_lo) return QS_ERR_ARG;
    BundlePlan plan;
    plan_bundles(n_taxa, rank_lo, rank_lo + n_tuples, score_bundle_waves(1), plan);
    std::copy(plan.plo.begin(), plan.plo.end(), first_pair);
    std::copy(plan.pcnt.begin(), plan.pcnt.end(), n_pairs);
    for (int i = 0; i < 2; ++i) { parts[2 * i] = i < plan.n_parts ? plan.part_lo[i] : 0; parts[2 * i + 1] = i < plan.n_parts ? plan.part_n[i] : 0; }
    return QS_OK;
}

extern "C" uint64_t qs_score_pair_slots(const qs_ref_tree *ref) {
    if (!ref || !ref->parent || ref->n_nodes == 0) return 0;
    std::vector<uint32_t> nchild(ref->n_nodes, 0);
    for (uint32_t v = 0; v < ref->n_nodes; ++v)
        if (ref->parent[v] >= 0 && (uint32_t)ref->parent[v] < ref->n_nodes) nchild[ref->parent[v]]++;
    uint64_t ni = 0;
    for (uint32_t v = 0; v < ref->n_nodes; ++v) ni += nchild[v] > 0;
    return ni * ni;
}

extern "C" int qs_score_set_view(qs_ctx *c, const void *table_dev, uint32_t count_bits, uint64_t rank_lo, uint64_t n_tuples) {
    if (c) c->log_valid = false;   // (the table / view / tuning may change: a logged pass 1 no longer describes it)
    if (!c) return QS_ERR_ARG;
    if (!table_dev) { c->view_table = nullptr; c->view_bits = 0; c->view_rank_lo = c->view_n = 0; return QS_OK; }
    if (count_bits != 16 && count_bits != 32) return fail(c, QS_ERR_ARG, "qs_score_set_view: count_bits must be 16 or 32");
    if (rank_lo > binom4(c->n) || n_tuples > binom4(c->n) - rank_lo) return fail(c, QS_ERR_ARG, "qs_score_set_view: rank range outside C(n,4)");
    c->view_table = table_dev; c->view_bits = count_bits; c->view_rank_lo = rank_lo; c->view_n = n_tuples;
    return QS_OK;
}

// qs_score's accumulators on the device and their pinned host copy, cached in the context
static int ensure_score_accumulators(qs_ctx *c, size_t np) {
    const size_t need_dev = np * (size_t)(3 + 1 + kCand) * 8, need_host = np * (size_t)(3 + kCand) * 8;
    QS_HIP(c, c->score_acc.reserve(need_dev, &c->stream));
    QS_HIP(c, c->score_acc_host.reserve(need_host, &c->stream));
    return QS_OK;
}

// the candidate log of the single-read scoring: records, the counter word, one word per node pair (tie filter)
static bool ensure_score_log(qs_ctx *c, size_t np) {
    const uint64_t want_cap = c->tune_score_log_cap ? c->tune_score_log_cap : (1ull << 23);   // 8 M records = 256 MB
    // (the counter sits behind the records: another capacity is another layout, and a buffer of its own size as before)
    if (c->score_log && c->score_log_cap != want_cap) { (void)hipStreamSynchronize(c->stream); c->score_log.reset(); }
    c->score_log_cap = 0;
    if (c->score_log.reserve((want_cap * 4 + 1 + np) * 8, &c->stream) != hipSuccess) { (void)hipGetLastError(); return false; }   // no room for the log: two passes
    c->score_log_cap = want_cap;
    return true;
}

// Is the single-read scoring wanted for the tuples sd covers? The bundle kernel over whole rows (bundle[0]: the plan of pass 1);
// QS_TUNE_SCORE_PASSES: 0 = automatic (tables from 1 GB, if there is a sample to predict the log from), 1 = never, 2 = always.
static bool want_score_log(const qs_ctx *c, const ScoreDevice &sd) {
    const uint64_t scored_bytes = sd.n_tuples * 3 * (uint64_t)(sd.count_bits / 8);
    return c->tune_score_kernel == 0 && c->bundle[0].n_parts == 0 &&
           (c->tune_score_passes == 2 || (c->tune_score_passes == 0 && c->tune_score_sample != 0 && scored_bytes >= (1ull << 30)));
}

extern "C" int qs_score_pass1(qs_ctx *c, const qs_ref_tree *ref, int64_t *sums_dev, int64_t *min_dev) {
    if (!c || !sums_dev || !min_dev) return fail(c, QS_ERR_ARG, "qs_score_pass1: NULL");
    if (!c->table && !c->view_table) return fail(c, QS_ERR_STATE, "qs_score_pass1: no table");
    QS_HIP(c, hipSetDevice(c->device));
    const RefHost *Rp = nullptr;
    int rc = get_ref(c, ref, true, &Rp);
    if (rc != QS_OK) return rc;
    const RefHost &R = *Rp;
    const size_t np = (size_t)R.n_inner * R.n_inner;
    QS_HIP(c, hipMemsetAsync(sums_dev, 0, np * 3 * 8, c->stream));
    QS_HIP(c, hipMemsetAsync(min_dev, 0x7F, np * 8, c->stream));
    { int rc_t = ensure_score_tables(c); if (rc_t != QS_OK) return rc_t; }
    ScoreDevice sd;
    fill_score_device(c, R, c->ref_lca_dev.get(), sd);
    sd.pair_sums = (unsigned long long *)sums_dev; sd.pair_min = (long long *)min_dev;
    { int rc_b = ensure_bundle_plan(c, sd, 1); if (rc_b != QS_OK) return rc_b; }
    // Single-read scoring: this pass also LOGS every quartet whose device QIC is within the tolerance of the bound it knows for
    // its node pair (the pair's minimum in memory, lowered beforehand by a minima-only pre-pass over a sample of the table, and
    // the lane's own running minimum) -- a superset of the quartets within the tolerance of ANY later minimum <= this table's,
    // so the qs_score_pass2 that follows filters the log instead of reading the table again, also when its min_dev holds the
    // minima over several shards / GPUs (QuartetScoreComputer.hpp:417-469 evaluates log_score of every quartet once, too).
    // QS_TUNE_SCORE_PASSES: 0 = automatic (tables from 1 GB, whole rows, bundle kernel; a second sample predicts the log and
    // the pass runs plain when it would not hold), 1 = never, 2 = always (pass 2 reads the table if the log overflows).
    c->log_valid = false;
    c->last_score_estimate = 0;
    // (sd.n_rounds: pass 1's plan as ensure_bundle_plan has just left it -- a plan without rounds has nothing to log)
    bool logging = want_score_log(c, sd) && sd.n_rounds > 0 && ensure_score_log(c, np);
    if (logging) {
        sd.list = c->score_log.get(); sd.list_count = sd.list + 4 * c->score_log_cap; sd.list_cap = c->score_log_cap;
        QS_HIP(c, hipMemsetAsync(sd.list_count, 0, 8, c->stream));
        if (c->tune_score_dedupe) {   // the tie filter (one word per node pair behind the log's counter)
            sd.last_trip = sd.list_count + 1;
            QS_HIP(c, hipMemsetAsync(sd.last_trip, 0xFF, np * 8, c->stream));
        }
        if (c->tune_score_sample) {   // minima-only pre-pass over a sample of the table: the bound the logging pass starts from
            ScoreDevice pre = sd;
            pre.list = nullptr; pre.list_count = nullptr; pre.list_cap = 0; pre.sample = c->tune_score_sample;
            QS_HIP(c, launch_score_pass1(c->stream, pre, 0, c->n_cu, nullptr, nullptr, 0, 0.0));
            if (c->tune_score_passes != 2) {
                // automatic mode: a second, disjoint sample counts what the logging pass would log of it
                pre.list_count = sd.list_count; pre.sample = c->tune_score_sample | (1u << 17);
                QS_HIP(c, launch_score_pass1(c->stream, pre, 0, c->n_cu, nullptr, nullptr, 0, c->tune_score_tol));
                unsigned long long hits = 0;
                QS_HIP(c, hipMemcpyAsync(&hits, sd.list_count, 8, hipMemcpyDeviceToHost, c->stream));
                QS_HIP(c, hipStreamSynchronize(c->stream));
                c->last_score_estimate = hits * (c->tune_score_sample & 0xFFFFu);
                // The static bounds of the sample over-predict: the full pass also lowers the minima as it goes, a lane keeps its
                // own running minimum, and the tie filter has seen 64 x more of every node pair (measured, predicted / logged:
                // 12.6 M / 1.6 M at 512 taxa x 10000 random trees, 3.7 M / 0.75 M at 256 taxa, 19 M / 1.0 M at 512 taxa x 10000
                // reference + NNI trees; without the tie filter those predict 90 M and do overflow 8 M): go ahead up to 6 x the log.
                if ((double)c->last_score_estimate > 6.0 * (double)c->score_log_cap) {
                    logging = false;
                    sd.list = nullptr; sd.list_count = nullptr; sd.list_cap = 0;
                } else {
                    QS_HIP(c, hipMemsetAsync(sd.list_count, 0, 8, c->stream));
                    if (sd.last_trip) QS_HIP(c, hipMemsetAsync(sd.last_trip, 0xFF, np * 8, c->stream));   // (the estimate logged nothing)
                }
            }
        }
        // waves reserve whole chunks of records: what they leave unwritten must read as "no record" (key = all ones)
        if (logging) {
            QS_HIP(c, hipMemsetAsync(sd.list, 0xFF, (size_t)c->score_log_cap * 32, c->stream));
            c->log_valid = true;                 // until the table, the view or the tuning changes (invalidate_log)
            c->log_table = sd.table; c->log_rank_lo = sd.rank_lo; c->log_n_tuples = sd.n_tuples; c->log_ref = Rp; c->log_tol = c->tune_score_tol;
        }
    }
    QS_HIP(c, launch_score_pass1(c->stream, sd, c->tune_score_kernel, c->n_cu, c->bundle[0].part_lo, c->bundle[0].part_n, c->bundle[0].n_parts, c->tune_score_tol));
    // rooted reference (degree-2 root): the sums of the node pairs (root, v) as the reference enumerates them (quirk Q5)
    if (c->root_pairs_dev) QS_HIP(c, launch_root_pair_sums(c->stream, sd, c->root_pairs_dev.get(), (uint32_t)R.root_pairs.size(), R.root_items));
    return QS_OK;   // asynchronous on the context's stream
}

// Everything a first qs_score pays before its kernels -- reference tree + LCA matrix on the device, log table, the bundle
// kernel's round tables, the accumulators with their pinned host copy, the candidate log, the kernels' code objects' first
// use of the device-to-host copy path -- done ahead of time. Safe while count kernels of this context are still running (same
// host thread): the uploads go through the copy stream, nothing waits for `stream`. The CLI calls it after the last batch
// is enqueued, where the host would only wait: the scoring phase of 512 taxa x 10000 trees drops from 28 to ~15 ms.
extern "C" int qs_score_prepare(qs_ctx *c, const qs_ref_tree *ref, uint64_t n_trees_total) {
    if (!c || !ref) return fail(c, QS_ERR_ARG, "qs_score_prepare: NULL");
    QS_HIP(c, hipSetDevice(c->device));
    if (!c->copy_stream) QS_HIP(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
    // every exit path -- also the error returns below -- leaves the copy stream drained: what was uploaded through it is marked
    // present in the context, and the kernels of a later qs_score run on `stream`, which has no ordering against `copy_stream`
    struct Restore { qs_ctx *c; ~Restore() { c->prep_stream = nullptr; (void)hipStreamSynchronize(c->copy_stream); } } restore{c};
    c->prep_stream = c->copy_stream;
    const RefHost *Rp = nullptr;
    int rc = get_ref(c, ref, true, &Rp);
    if (rc != QS_OK) return rc;
    const size_t np = (size_t)Rp->n_inner * Rp->n_inner;
    if (np == 0) return fail(c, QS_ERR_ARG, "qs_score_prepare: bad reference tree");
    const uint64_t keep_hint = c->table_trees_hint;
    c->table_trees_hint = std::max<uint64_t>(c->table_trees_hint, n_trees_total);   // size the log table for the finished table
    rc = ensure_score_tables(c);
    c->table_trees_hint = keep_hint;
    if (rc != QS_OK) return rc;
    ScoreDevice sd;
    fill_score_device(c, *Rp, c->ref_lca_dev.get(), sd);
    rc = ensure_bundle_plan(c, sd, 1);
    if (rc == QS_OK) rc = ensure_bundle_plan(c, sd, 2);
    if (rc != QS_OK) return rc;
    rc = ensure_score_accumulators(c, np);
    if (rc != QS_OK) return rc;
    // (without pass 1's "the plan has rounds": sd holds pass 2's plan here, and a log that is never used costs only its memory)
    if (want_score_log(c, sd)) (void)ensure_score_log(c, np);
    for (hipEvent_t &e : c->score_ev) if (!e) QS_HIP(c, hipEventCreate(&e));
    // first use of the pinned accumulator copy by the device (the first device-to-host copy into freshly pinned memory took 7 ms)
    QS_HIP(c, hipMemcpyAsync(c->score_acc_host.get(), c->score_acc.get(), np * (size_t)(3 + kCand) * 8, hipMemcpyDeviceToHost, c->copy_stream));
    QS_HIP(c, hipStreamSynchronize(c->copy_stream));
    return QS_OK;
}

extern "C" int qs_score_pass2(qs_ctx *c, const qs_ref_tree *ref, const int64_t *min_dev, int64_t *cand_dev) {
    if (!c || !min_dev || !cand_dev) return fail(c, QS_ERR_ARG, "qs_score_pass2: NULL");
    if (!c->table && !c->view_table) return fail(c, QS_ERR_STATE, "qs_score_pass2: no table");
    QS_HIP(c, hipSetDevice(c->device));
    const RefHost *Rp = nullptr;
    int rc = get_ref(c, ref, true, &Rp);
    if (rc != QS_OK) return rc;
    const RefHost &R = *Rp;
    const size_t np = (size_t)R.n_inner * R.n_inner;
    QS_HIP(c, hipMemsetAsync(cand_dev, 0xFF, np * kCand * 8, c->stream));
    QS_HIP(c, hipMemsetAsync(c->dev_flags.get() + 1, 0, 4, c->stream));
    { int rc_t = ensure_score_tables(c); if (rc_t != QS_OK) return rc_t; }
    ScoreDevice sd;
    fill_score_device(c, R, c->ref_lca_dev.get(), sd);
    sd.pair_min = (long long *)min_dev; sd.pair_cand = (unsigned long long *)cand_dev;
    c->last_score_log = 0;
    if (c->log_valid && c->log_table == sd.table && c->log_rank_lo == sd.rank_lo && c->log_n_tuples == sd.n_tuples && c->log_ref == Rp &&
        c->log_tol == c->tune_score_tol) {
        // the preceding qs_score_pass1 over this very table logged its candidates: filter the log against min_dev
        c->log_valid = false;
        unsigned long long n_rec = 0;
        QS_HIP(c, hipMemcpyAsync(&n_rec, c->score_log.get() + 4 * c->score_log_cap, 8, hipMemcpyDeviceToHost, c->stream));
        QS_HIP(c, hipStreamSynchronize(c->stream));
        // A counter that reached the capacity is an overflow: waves reserve chunks of 64 records, the capacity is a multiple
        // of 64, so the counter can stop exactly AT the capacity while waves that found the log full at the start of a row
        // have skipped their hits without moving it. Only a log with room left is known to be complete.
        if (n_rec < c->score_log_cap) {
            sd.list = c->score_log.get(); sd.list_cap = c->score_log_cap;
            QS_HIP(c, launch_score_log(c->stream, sd, c->tune_score_tol, n_rec));
            c->last_score_log = n_rec;
            return QS_OK;
        }
        // (the log overflowed: read the table)
    }
    { int rc_b = ensure_bundle_plan(c, sd, 2); if (rc_b != QS_OK) return rc_b; }
    QS_HIP(c, launch_score_pass2(c->stream, sd, c->tune_score_tol, c->tune_score_kernel, c->n_cu, c->bundle[1].part_lo, c->bundle[1].part_n, c->bundle[1].n_parts));
    return QS_OK;   // asynchronous; node pairs whose slots did not suffice are marked in cand_dev (qs_score_overflow)
}

// Node pairs that pass 2 could not finish in their 8 packed slots (more than 8 distinct near-minimal triples, or a
// gcd-reduced count >= 2^21) carry kCandOverflow in their last slot. For those pairs the table is scanned once more
// and EVERY near-minimal quartet's (key, q1, q2, q3) is listed; the list is sorted and de-duplicated on the host and
// handed to qs_score_finish, which takes the exact minimum over it. The reference evaluates log_score for every
// quartet (QuartetScoreComputer.hpp:417-469), so any superset of the minimisers gives its result.
extern "C" int qs_score_overflow(qs_ctx *c, const qs_ref_tree *ref, const int64_t *min_dev, const int64_t *cand_dev,
                                 int64_t **list_out, uint64_t *n_out) {
    if (!c || !min_dev || !cand_dev || !list_out || !n_out) return fail(c, QS_ERR_ARG, "qs_score_overflow: NULL");
    *list_out = nullptr; *n_out = 0;
    QS_HIP(c, hipSetDevice(c->device));
    uint32_t fl = 0;
    QS_HIP(c, hipMemcpyAsync(&fl, c->dev_flags.get() + 1, 4, hipMemcpyDeviceToHost, c->stream));
    QS_HIP(c, hipStreamSynchronize(c->stream));
    if ((fl & 3u) == 0) return QS_OK;
    const RefHost *Rp = nullptr;
    int rc = get_ref(c, ref, true, &Rp);
    if (rc != QS_OK) return rc;
    ScoreDevice sd;
    fill_score_device(c, *Rp, c->ref_lca_dev.get(), sd);
    sd.pair_min = (long long *)const_cast<int64_t *>(min_dev); sd.pair_cand = (unsigned long long *)const_cast<int64_t *>(cand_dev);
    DevBuf<unsigned long long> cnt, list;
    QS_HIP(c, cnt.reserve(8, nullptr));
    uint64_t cap = 1ull << 20;
    std::vector<unsigned long long> host;
    for (int attempt = 0; attempt < 2; ++attempt) {
        if (list.reserve(cap * 32, nullptr) != hipSuccess) return fail(c, QS_ERR_OOM, "qs_score_overflow: list of " + std::to_string(cap) + " quartets does not fit");
        QS_HIP(c, hipMemsetAsync(cnt.get(), 0, 8, c->stream));
        sd.list = list.get(); sd.list_count = cnt.get(); sd.list_cap = cap;
        QS_HIP(c, launch_score_overflow_list(c->stream, sd, c->tune_score_tol));
        unsigned long long got = 0;
        QS_HIP(c, hipMemcpyAsync(&got, cnt.get(), 8, hipMemcpyDeviceToHost, c->stream));
        QS_HIP(c, hipStreamSynchronize(c->stream));
        if (got <= cap) {
            host.resize(got * 4);
            if (got) QS_HIP(c, hipMemcpy(host.data(), list.get(), got * 32, hipMemcpyDeviceToHost));
            break;
        }
        if (attempt == 1 || got > (1ull << 28)) return fail(c, QS_ERR_OVERFLOW, "qs_score_overflow: " + std::to_string(got) + " near-minimal quartets");
        cap = got;
    }
    // sort + unique the 4-word records
    const size_t n = host.size() / 4;
    std::vector<size_t> idx(n);
    for (size_t i = 0; i < n; ++i) idx[i] = i;
    auto less = [&](size_t x, size_t y) { return std::lexicographical_compare(&host[4 * x], &host[4 * x] + 4, &host[4 * y], &host[4 * y] + 4); };
    std::sort(idx.begin(), idx.end(), less);
    std::vector<unsigned long long> uniq;
    for (size_t i = 0; i < n; ++i)
        if (i == 0 || less(idx[i - 1], idx[i])) uniq.insert(uniq.end(), &host[4 * idx[i]], &host[4 * idx[i]] + 4);
    if (!uniq.empty()) {
        int64_t *out = (int64_t *)malloc(uniq.size() * 8);
        if (!out) return fail(c, QS_ERR_OOM, "qs_score_overflow: host list");
        memcpy(out, uniq.data(), uniq.size() * 8);
        *list_out = out; *n_out = uniq.size() / 4;
    }
    return QS_OK;
}

extern "C" void qs_free_host(void *p) { free(p); }

// QS_SCORE_SAVEMEM_LOOKUPS + a degree-2 reference root. For a node pair (root, v) the reference calls
// countQuartetOccurrences(a, b, c, d) with a in S1 (the root's other side), b in S2 = ALL leaves on v's side, c in S3, d in S4
// (v's child subtrees; QuartetScoreComputer.hpp:393-396,412-424): b repeats c or d. Its compact table sorts the ids
// (quartet_lookup_table.hpp:170-212) and the const get_tuple throws std::runtime_error("id = ..., but quartet_lookup_.size() =
// ...") when the index C(t1,4)+C(t2,3)+C(t3,2)+t4 of the sorted ids t1 >= t2 >= t3 >= t4 lies behind the table (:79-85), e.g.
// whenever the two largest are both n-1: for every rooted reference tree with 4 or more taxa some call does (proved case by
// case in DESIGN.md 1, checked on the unmodified header in tests/test_oracle_reftable.py). The exception is not caught
// anywhere in the reference: its run ends there. This finds the FIRST throwing call in the reference's sequential order
// (pairs by node index; a, b, c, d nested in that order, each ascending) without walking the O(n^4) calls: the index is
// monotone in every id, so the calls of a prefix throw iff the one with the largest remaining ids does.
static uint64_t dup_index(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {   // lookup_index_ on ids that may repeat
    uint32_t t[4] = {a, b, c, d};
    std::sort(t, t + 4);
    return binom4(t[3]) + binom3(t[2]) + binom2(t[1]) + t[0];
}
static bool first_compact_throw(const RefHost &R, uint64_t nq, uint64_t *id_out) {
    for (const RootPairHost &P : R.root_pairs) {
        if (!P.s1_n || !P.s3_n || !P.s4_n) continue;
        const uint32_t a_hi = P.s1_lo + P.s1_n - 1, c_hi = P.s3_lo + P.s3_n - 1, d_hi = P.s4_lo + P.s4_n - 1;
        // the largest index any call of this pair reaches: b repeats the largest c or the largest d
        if (std::max(dup_index(a_hi, c_hi, c_hi, d_hi), dup_index(a_hi, d_hi, c_hi, d_hi)) < nq) continue;
        for (uint32_t a = P.s1_lo; a <= a_hi; ++a) {
            if (std::max(dup_index(a, c_hi, c_hi, d_hi), dup_index(a, d_hi, c_hi, d_hi)) < nq) continue;
            for (uint32_t b = P.s2_lo; b < P.s2_lo + P.s2_n; ++b) {
                const bool in3 = b >= P.s3_lo && b <= c_hi, in4 = b >= P.s4_lo && b <= d_hi;
                if (in3) {            // calls (a, b, c = b, d), d ascending: a throwing d exists iff the largest throws
                    if (dup_index(a, b, b, d_hi) < nq) continue;
                    for (uint32_t d = P.s4_lo; d <= d_hi; ++d)
                        if (dup_index(a, b, b, d) >= nq) { *id_out = dup_index(a, b, b, d); return true; }
                } else if (in4) {     // calls (a, b, c, d = b), c ascending
                    if (dup_index(a, b, c_hi, b) < nq) continue;
                    for (uint32_t c = P.s3_lo; c <= c_hi; ++c)
                        if (dup_index(a, b, c, b) >= nq) { *id_out = dup_index(a, b, c, b); return true; }
                }
            }
        }
    }
    return false;
}
static int check_savemem_lookups(qs_ctx *c, const RefHost &R, uint32_t flags) {
    if (!(flags & QS_SCORE_SAVEMEM_LOOKUPS) || (flags & QS_SCORE_ROOT_AS_EDGE) || !R.bifurcating || !R.root_deg2) return QS_OK;
    const uint64_t nq = binom4(R.n);
    uint64_t id = 0;
    if (!first_compact_throw(R, nq, &id)) return QS_OK;
    return fail(c, QS_ERR_REFERENCE_THROWS, "id = " + std::to_string(id) + ", but quartet_lookup_.size() = " + std::to_string(nq));
}

// Host-only: what qs_score / qs_score_finish would refuse for this reference tree and these flags, found from the tree alone
// (before any counting): today the QS_SCORE_SAVEMEM_LOOKUPS + rooted-reference case. ctx may be NULL.
extern "C" int qs_score_check(qs_ctx *c, const qs_ref_tree *ref, uint32_t flags) {
    if (!ref) return fail(c, QS_ERR_ARG, "qs_score_check: NULL");
    RefHost local;
    const RefHost *Rp = &local;
    const int rc = c ? get_ref(c, ref, false, &Rp) : build_ref(nullptr, ref, local);
    if (rc != QS_OK) return rc;
    return check_savemem_lookups(c, *Rp, flags);
}

// Pure host: log_score of the O(#node pairs) candidates and sums with the host libm
// (QuartetScoreComputer.hpp:135-159), then the min-propagation along path(u,v) (:448-454, :472-489).
extern "C" int qs_score_finish(qs_ctx *c, const qs_ref_tree *ref, uint32_t flags, const int64_t *sums_host,
                               const int64_t *cand_host, uint32_t n_cand_parts, const int64_t *extra_host, uint64_t n_extra,
                               double *lqic, double *qpic, double *eqpic, int *is_bifurcating) {
    if (!sums_host || !cand_host || !lqic || n_cand_parts == 0) return fail(c, QS_ERR_ARG, "qs_score_finish: NULL");
    RefHost local;          // ctx == NULL: pure host use (no device, no cache)
    const RefHost *Rp = &local;
    int rc = c ? get_ref(c, ref, false, &Rp) : build_ref(nullptr, ref, local);
    if (rc != QS_OK) return rc;
    const RefHost &R = *Rp;
    const bool root_as_edge = (flags & QS_SCORE_ROOT_AS_EDGE) != 0;
    if (is_bifurcating) *is_bifurcating = R.bifurcating ? 1 : 0;
    { int rc_s = check_savemem_lookups(c, R, flags); if (rc_s != QS_OK) return rc_s; }
    if (R.bifurcating && (!qpic || !eqpic)) return fail(c, QS_ERR_ARG, "qs_score: qpic/eqpic required for a bifurcating reference");
    const size_t np = (size_t)R.n_inner * R.n_inner;
    const unsigned long long *sums = (const unsigned long long *)sums_host;
    const unsigned long long *cand = (const unsigned long long *)cand_host;
    // extra candidates (qs_score_overflow lists, any order): key -> range in a sorted copy
    std::vector<std::array<unsigned long long, 4>> extra;
    // A record flagged kListSwap / a slot flagged kCandSwap is a quartet the reference evaluates twice for a degree-2 root, the
    // second time with q2 and q3 exchanged (qs_score.hip root_swapped; QuartetScoreComputer.hpp:393-396,417-454): both orders
    // enter the minimum. QS_SCORE_ROOT_AS_EDGE does not reproduce the reference's root pairs, hence not this either.
    const bool both_orders = !root_as_edge;
    if (extra_host && n_extra) {
        extra.reserve(n_extra);
        for (uint64_t i = 0; i < n_extra; ++i) {
            const unsigned long long *e = (const unsigned long long *)extra_host + 4 * i;
            extra.push_back({e[0] & 0xFFFFFFFFull, e[1], e[2], e[3]});
            if ((e[0] & kListSwap) && both_orders) extra.push_back({e[0] & 0xFFFFFFFFull, e[1], e[3], e[2]});
        }
        std::sort(extra.begin(), extra.end());
    }
    const double inf = std::numeric_limits<double>::infinity();
    const uint32_t N = R.n_nodes;
    for (uint32_t v = 0; v < N; ++v) {
        lqic[v] = inf;
        if (R.bifurcating) { qpic[v] = inf; eqpic[v] = inf; }
    }
    // The O(#node pairs) finalisation runs on a few host threads for large references. Each thread folds a contiguous
    // range of iu (pairs are visited in (iu, iv) order) into private vectors; merging the ranges in order reproduces
    // the sequential result exactly, including which of two equal minima / which of two writers of a QP value wins.
    struct Local { std::vector<double> lq, qp, eqp; std::vector<uint8_t> qp_set; };
    auto fold = [&](uint32_t iu0, uint32_t iu1, Local &out) {
        out.lq.assign(N, inf);
        if (R.bifurcating) { out.qp.assign(N, inf); out.eqp.assign(N, inf); out.qp_set.assign(N, 0); }
        for (uint32_t iu = iu0; iu < iu1; ++iu)
            for (uint32_t iv = iu + 1; iv < R.n_inner; ++iv) {
                const size_t key = (size_t)iu * R.n_inner + iv;
                double lqmin = inf;
                bool any = false;
                for (uint32_t part = 0; part < n_cand_parts; ++part) {
                    const unsigned long long *cs = cand + ((size_t)part * np + key) * kCand;
                    for (int s = 0; s < kCand && cs[s] != kCandEmpty; ++s) {
                        if (cs[s] == kCandOverflow) continue;   // marker: this pair's full list is in `extra`
                        const uint64_t q1 = (cs[s] >> 42) & 0x1FFFFFu, q2 = (cs[s] >> 21) & 0x1FFFFFu, q3 = cs[s] & 0x1FFFFFu;
                        const double v = host_log_score(q1, q2, q3);
                        lqmin = std::min(lqmin, v);
                        if ((cs[s] & kCandSwap) && both_orders) lqmin = std::min(lqmin, host_log_score(q1, q3, q2));
                        any = true;
                    }
                }
                if (!extra.empty()) {
                    const std::array<unsigned long long, 4> lo_key = {(unsigned long long)key, 0, 0, 0};
                    for (auto it = std::lower_bound(extra.begin(), extra.end(), lo_key); it != extra.end() && (*it)[0] == key; ++it) {
                        lqmin = std::min(lqmin, host_log_score((*it)[1], (*it)[2], (*it)[3]));
                        any = true;
                    }
                }
                if (!any) continue; // pair owns no resolved quartet
                uint64_t p1 = sums[key * 3], p2 = sums[key * 3 + 1], p3 = sums[key * 3 + 2];
                if (!(flags & QS_SCORE_QP_EXACT64)) { p1 &= 0xFFFFFFFFull; p2 &= 0xFFFFFFFFull; p3 &= 0xFFFFFFFFull; } // QSC:382
                const double qp = host_log_score(p1, p2, p3);
                // walk the path u..v (edges are indexed by their child node)
                uint32_t x = R.inner_node[iu], y = R.inner_node[iv];
                uint32_t path_edges = 0, last_edge_a = 0, last_edge_b = 0;
                while (x != y) {
                    uint32_t e;
                    if (R.depth[x] >= R.depth[y]) { e = x; x = (uint32_t)R.parent[x]; }
                    else { e = y; y = (uint32_t)R.parent[y]; }
                    out.lq[e] = std::min(out.lq[e], lqmin);
                    if (R.bifurcating) out.eqp[e] = std::min(out.eqp[e], qp);
                    if (path_edges == 0) last_edge_a = e; else last_edge_b = e;
                    ++path_edges;
                }
                if (R.bifurcating) {
                    const bool through_deg2_root = root_as_edge && path_edges == 2 && x == R.root && R.nchild[R.root] == 2;
                    if (path_edges == 1) { out.qp[last_edge_a] = qp; out.qp_set[last_edge_a] = 1; }
                    else if (through_deg2_root) { out.qp[last_edge_a] = qp; out.qp[last_edge_b] = qp; out.qp_set[last_edge_a] = out.qp_set[last_edge_b] = 1; }
                }
            }
    };
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    const unsigned workers = R.n_inner >= 128 ? std::min(8u, hw) : 1u;
    std::vector<Local> parts(workers + 1);
    if (workers == 1) fold(0, R.n_inner, parts[0]);
    else {
        // ranges of iu with about the same number of pairs (row iu has n_inner - 1 - iu of them)
        std::vector<uint32_t> cut(workers + 1, R.n_inner);
        const uint64_t total = (uint64_t)R.n_inner * (R.n_inner - 1) / 2;
        uint64_t acc = 0;
        uint32_t w = 1;
        cut[0] = 0;
        for (uint32_t iu = 0; iu < R.n_inner && w < workers; ++iu) {
            acc += R.n_inner - 1 - iu;
            while (w < workers && acc >= total * w / workers) cut[w++] = iu + 1;
        }
        std::vector<std::thread> pool;
        for (unsigned k = 0; k < workers; ++k) pool.emplace_back([&, k] { fold(cut[k], cut[k + 1], parts[k]); });
        for (auto &th : pool) th.join();
    }
    if (R.bifurcating && R.root_deg2 && !root_as_edge) {
        // Reference-compatible handling of a degree-2 root (quirk Q5, QuartetScoreComputer.hpp:393-396,472-489): every
        // pair (root, v) has its own sums (root_pair_sums_kernel); QP-IC of the edge if v is a child of the root, EQP-IC
        // minimum along the path. (Pairs are visited with u = root first in the reference: these come before all others.)
        Local &L = parts[workers];
        L.lq.assign(N, inf); L.qp.assign(N, inf); L.eqp.assign(N, inf); L.qp_set.assign(N, 0);
        for (const RootPairHost &P : R.root_pairs) {
            uint64_t p1 = sums[(size_t)P.key * 3], p2 = sums[(size_t)P.key * 3 + 1], p3 = sums[(size_t)P.key * 3 + 2];
            if (!(flags & QS_SCORE_QP_EXACT64)) { p1 &= 0xFFFFFFFFull; p2 &= 0xFFFFFFFFull; p3 &= 0xFFFFFFFFull; }
            const double qp = host_log_score(p1, p2, p3);
            const uint32_t iu = P.key / R.n_inner, iv = P.key % R.n_inner;
            uint32_t v = R.inner_node[iu] == R.root ? R.inner_node[iv] : R.inner_node[iu];
            if ((uint32_t)R.parent[v] == R.root) { L.qp[v] = qp; L.qp_set[v] = 1; }
            for (uint32_t x = v; x != R.root; x = (uint32_t)R.parent[x]) L.eqp[x] = std::min(L.eqp[x], qp);
        }
        std::rotate(parts.begin(), parts.begin() + workers, parts.end());   // merged first
    } else parts.pop_back();
    for (const Local &L : parts) // in range order
        for (uint32_t v = 0; v < N; ++v) {
            lqic[v] = std::min(lqic[v], L.lq[v]);
            if (R.bifurcating) {
                eqpic[v] = std::min(eqpic[v], L.eqp[v]);
                if (L.qp_set[v]) qpic[v] = L.qp[v];
            }
        }
    return QS_OK;
}

extern "C" int qs_score(qs_ctx *c, const qs_ref_tree *ref, uint32_t flags, double *lqic, double *qpic, double *eqpic,
                        int *is_bifurcating) {
    if (!c || !lqic) return fail(c, QS_ERR_ARG, "qs_score: NULL");
    if (!c->table) return fail(c, QS_ERR_STATE, "qs_score: no table");
    if (c->d_lo != 0 || c->d_hi != c->n)
        return fail(c, QS_ERR_UNSUPPORTED, "qs_score: this context owns a table shard; use qs_score_pass1 / qs_score_pass2 / "
                                           "qs_score_finish with reductions over the shards in between");
    const size_t np = (size_t)qs_score_pair_slots(ref);
    if (np == 0) return fail(c, QS_ERR_ARG, "qs_score: bad reference tree");
    QS_HIP(c, hipSetDevice(c->device));
    using clk = std::chrono::steady_clock;
    auto ms_since = [](clk::time_point t) { return std::chrono::duration<float, std::milli>(clk::now() - t).count(); };
    const clk::time_point t_all = clk::now();
    for (hipEvent_t &e : c->score_ev) if (!e) QS_HIP(c, hipEventCreate(&e));
    for (float &x : c->score_ms) x = 0;
    // the accumulators (sums, minima, candidate slots: 24 MB at 512 taxa) and their pinned host copy live in the context: three
    // hipMalloc / hipFree pairs and a pageable 22 MB copy per call were 1 ms of a 15 ms call
    struct Ptr { void *p; } sums{nullptr}, mn{nullptr}, cand{nullptr};
    { int rc_a = ensure_score_accumulators(c, np); if (rc_a != QS_OK) return rc_a; }
    sums.p = c->score_acc.get(); mn.p = (char *)sums.p + np * 3 * 8; cand.p = (char *)sums.p + np * 4 * 8;
    {   // the cached pieces both passes need (reference tree + LCA matrix, log table, bundle plans): built here so that
        // the first call's set-up cost shows as its own phase and the events below bracket kernels only
        const RefHost *Rp = nullptr;
        int rc0 = get_ref(c, ref, true, &Rp);
        if (rc0 != QS_OK) return rc0;
        rc0 = check_savemem_lookups(c, *Rp, flags);      // (the reference throws during its scoring loop: before any kernel here)
        if (rc0 != QS_OK) return rc0;
        rc0 = ensure_score_tables(c);
        if (rc0 != QS_OK) return rc0;
    }
    c->score_ms[1] = ms_since(t_all);
    QS_HIP(c, hipEventRecord(c->score_ev[0], c->stream));
    int rc = qs_score_pass1(c, ref, (int64_t *)sums.p, (int64_t *)mn.p);     // (may log its candidates: see there)
    if (rc != QS_OK) return rc;
    QS_HIP(c, hipEventRecord(c->score_ev[1], c->stream));
    rc = qs_score_pass2(c, ref, (const int64_t *)mn.p, (int64_t *)cand.p);   // a filter over that log, or the second read
    if (rc != QS_OK) return rc;
    QS_HIP(c, hipEventRecord(c->score_ev[2], c->stream));
    const clk::time_point t_ov = clk::now();
    int64_t *extra = nullptr;
    uint64_t n_extra = 0;
    rc = qs_score_overflow(c, ref, (const int64_t *)mn.p, (const int64_t *)cand.p, &extra, &n_extra);   // synchronises the stream
    if (rc != QS_OK) return rc;
    struct FreeHost { int64_t *p; ~FreeHost() { free(p); } } free_extra{extra};
    // The accumulators come home through the COPY stream (the count stream is idle: qs_score_overflow has just synchronised
    // it). The first large device-to-host copy enqueued on a stream that has run kernels costs ~8 ms on the host, once per
    // stream (tools/d2h_cold.hip); a stream that only ever copies does not pay it -- that was most of a first call's
    // "wait + copies" phase.
    int64_t *hs = (int64_t *)c->score_acc_host.get(), *hc = hs + np * 3;
    if (!c->copy_stream) QS_HIP(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
    QS_HIP(c, hipMemcpyAsync(hs, sums.p, np * 3 * 8, hipMemcpyDeviceToHost, c->copy_stream));
    QS_HIP(c, hipMemcpyAsync(hc, cand.p, np * kCand * 8, hipMemcpyDeviceToHost, c->copy_stream));
    QS_HIP(c, hipStreamSynchronize(c->copy_stream));
    (void)hipEventElapsedTime(&c->score_ms[2], c->score_ev[0], c->score_ev[1]);
    (void)hipEventElapsedTime(&c->score_ms[3], c->score_ev[1], c->score_ev[2]);
    c->score_ms[4] = ms_since(t_ov);            // waiting for the passes + overflow pass (if any) + the accumulators' way back
    const clk::time_point t_fin = clk::now();
    rc = qs_score_finish(c, ref, flags, hs, hc, 1, extra, n_extra, lqic, qpic, eqpic, is_bifurcating);
    c->score_ms[5] = ms_since(t_fin);
    c->score_ms[0] = ms_since(t_all);
    return rc;
}

// Phases of the last qs_score call in ms: [0] whole call (host clock), [1] set-up (accumulator allocation, reference tree
// + LCA matrix, log table; near zero once cached), [2] pass 1 and [3] pass 2 (HIP events on the context's stream: kernels
// + the bundle plan of a first call), [4] host wait for the passes incl. overflow pass and device-to-host copies,
// [5] qs_score_finish (host libm + min-propagation).
// Records the candidate log of the most recent qs_score held (single-read mode); 0 = it took two passes over the table.
extern "C" uint64_t qs_last_score_log(const qs_ctx *c) { return c ? c->last_score_log : 0; }
extern "C" uint64_t qs_last_score_estimate(const qs_ctx *c) { return c ? c->last_score_estimate : 0; }

extern "C" int qs_last_score_ms(qs_ctx *c, float out_ms[6]) {
    if (!c || !out_ms) return QS_ERR_ARG;
    for (int i = 0; i < 6; ++i) out_ms[i] = c->score_ms[i];
    return QS_OK;
}

static int raw_qic_impl(qs_ctx *c, const qs_ref_tree *ref, uint64_t r0, uint64_t nq, uint8_t *topo, uint64_t *q, bool lex) {
    if (!c || !c->table) return fail(c, QS_ERR_STATE, "qs_raw_qic: no table");
    if (r0 + nq > c->n_tuples) return fail(c, QS_ERR_ARG, "qs_raw_qic: rank range outside this context's table");
    if (lex && (c->d_lo != 0 || c->d_hi != c->n)) return fail(c, QS_ERR_UNSUPPORTED, "qs_raw_qic_lex: needs the whole table (not a shard)");
    if (nq == 0) return QS_OK;
    QS_HIP(c, hipSetDevice(c->device));
    const RefHost *Rp = nullptr;
    int rc = get_ref(c, ref, true, &Rp);
    if (rc != QS_OK) return rc;
    const RefHost &R = *Rp;
    DevBuf<uint8_t> dt_mem; DevBuf<unsigned long long> dq_mem;   // (freed on every way out; hipFree waits for the device)
    QS_HIP(c, dt_mem.reserve(nq, nullptr));
    if (dq_mem.reserve(nq * 24, nullptr) != hipSuccess) return fail(c, QS_ERR_OOM, "qs_raw_qic: hipMalloc");
    uint8_t *const dt = dt_mem.get(); unsigned long long *const dq = dq_mem.get();
    { int rc_t = ensure_score_tables(c); if (rc_t != QS_OK) return rc_t; }
    ScoreDevice sd;
    fill_score_device(c, R, c->ref_lca_dev.get(), sd);
    sd.frame = 1; // printRawQICScores uses the multifurcating loop's argument order
    hipError_t e = lex ? launch_raw_qic_lex(c->stream, sd, r0, nq, dt, dq) : launch_raw_qic(c->stream, sd, r0, nq, dt, dq);
    if (e == hipSuccess) e = hipMemcpyAsync(topo, dt, nq, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(q, dq, nq * 24, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, QS_ERR_HIP, std::string("qs_raw_qic: ") + hipGetErrorString(e));
    return QS_OK;
}

extern "C" int qs_raw_qic(qs_ctx *c, const qs_ref_tree *ref, uint64_t r0, uint64_t nq, uint8_t *topo, uint64_t *q) {
    return raw_qic_impl(c, ref, r0, nq, topo, q, false);
}
extern "C" int qs_raw_qic_lex(qs_ctx *c, const qs_ref_tree *ref, uint64_t i0, uint64_t nq, uint8_t *topo, uint64_t *q) {
    return raw_qic_impl(c, ref, i0, nq, topo, q, true);
}
