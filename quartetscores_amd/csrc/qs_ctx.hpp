// qs_ctx.hpp -- what the files of the C-ABI layer share: the context, a device batch, the flattened reference tree, error
// reporting, and the few helpers one of them defines and another calls. Private to qs_abi*.hip and qs_probe.hip; no kernel file
// and not the host-only planning (qs_plan.hip) includes it.
#pragma once
#include "../../include/quartetscores_hip.h"
#include "qs_common.hpp"
#include "qs_devbuf.hpp"
#include "qs_internal.hpp"

#include <future>
#include <memory>
#include <string>
#include <vector>

namespace qs {

struct EarlyPerm { std::vector<uint32_t> perm; uint32_t chunk = 0, cblock_in = 0, cgroup = 0; bool ok = false; };

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

}  // namespace qs

// The two structs the public header names are global, as in C; their fields use the project's types unqualified, like every file
// that includes this one.
using namespace qs;

struct qs_device_batch {
    DeviceBatch d;
    std::vector<uint32_t> fix_slot;   // depth clamp: slot (in the class-ordered batch) of the tree behind every correction unit, ascending
    std::vector<uint64_t> fix_work;   // n_fix + 1 prefix sums: triples x fourth leaves of every unit (what the split of a slice is planned from)
};

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
    // (a,b)-major launch order of count_bitslice3_kernel's tiles (tile_order, qs_abi_count.hip): launch slot -> tile id, built on
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
    uint32_t tune_step_order = 0;            // QS_TUNE_STEP_ORDER: 0 = automatic, 1 = prefetch, 2 = late loads (binary_full instances that have a late variant)
    uint32_t tune_stage_six = 0;             // QS_TUNE_STAGE_SIX: 0 = automatic, 1 = the instances QS_TUNE_STEP_ORDER selects, 2 = the six-wave instance wherever it exists
    uint32_t last_six_waves = 0;             // waves per SIMD of the six-wave instance the last count ran (variant segment /dma<w> or /late<w>); 0 = none did
    uint32_t last_late_waves = 0;           // waves per SIMD of the late-load instance the last count ran (variant segment /late<w>); 0 = none did
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
    // qs_table_collapse: first_id and the species of every source id (host copy kept until the upload on `stream` has read it), and
    // the largest sum a cell of the collapsed table may hold (trees x the four largest groups; 0 = never collapsed into): cells
    // can exceed trees-counted then, which sizes the log table and the partial sums of the whole-table queries
    std::vector<uint16_t> collapse_ids;
    DevBuf<uint16_t> collapse_ids_dev;
    uint64_t collapse_max_count = 0;
    // qs_tree_agreement: the reference tree's inner nodes (>= 3 links) as id boundaries on the device, and the tree they came from
    std::vector<int32_t> agree_parent;
    std::vector<uint32_t> agree_leaf_node;
    DevBuf<uint32_t> agree_off;
    DevBuf<uint16_t> agree_bnd;
    DevBuf<uint8_t> agree_par;
    uint32_t agree_n_u = 0;
    // qs_tree_branch_support: the reference tree's internodes and child boundaries on the device (launch_tree_branch), and the tree they
    // came from; qs_branch_resample: the weights of the last call, kept until the upload on `stream` has read them
    std::vector<int32_t> tbranch_parent;
    std::vector<uint32_t> tbranch_leaf_node;
    DevBuf<uint32_t> tbranch_edges;
    DevBuf<uint16_t> tbranch_bnd;
    uint32_t tbranch_n_e = 0, tbranch_n_nodes = 0;
    int tbranch_frame = 0;
    std::vector<uint32_t> resample_weights;
    DevBuf<uint32_t> resample_weights_dev;
    // qs_tree_pair_agreement: the position maps and node orders of the last call's row trees (tree_pairs_work_words; grown, never shrunk)
    DevBuf<uint16_t> pair_pos;
    // qs_taxon_placement: the cached reference tree's link lookups (dropped with ref_lca_dev), the walks of an n-taxon table and
    // the list of the last call (both shared with qs_taxon_pair_support); the host copies stay until the uploads on `stream` have read them
    std::vector<uint16_t> place_child, place_next, place_taxa;
    std::vector<uint32_t> place_tasks;
    DevBuf<uint16_t> place_child_dev, place_next_dev, place_taxa_dev;
    DevBuf<uint32_t> place_node_dev, place_tasks_dev;
    // qs_branch_taxon_support: the cached reference tree's run ends on both sides of the diagonal, its words (par | inner_node | edge_key,
    // BranchDevice) and the internodes' numbers of 4-sets (dropped with ref_lca_dev), kept like the lists above; the node-pair sums and
    // minima of the score pass 1 behind the totals (grown, never shrunk)
    std::vector<uint16_t> branch_next;
    std::vector<uint32_t> branch_words;
    std::vector<unsigned long long> branch_quartets;
    DevBuf<uint16_t> branch_next_dev;
    DevBuf<uint32_t> branch_words_dev;
    DevBuf<unsigned long long> branch_quartets_dev;
    uint32_t branch_dup_from = 0xFFFFFFFFu, branch_dup_to = 0;
    DevBuf<unsigned long long> branch_sums;
    // qs_clade_placement: the walks in the numbering of the ids outside a clade (one list for every clade size) and the last call's
    // clades and workgroups, kept like the lists above
    std::vector<uint32_t> clade_tasks, clade_list;
    DevBuf<uint32_t> clade_tasks_dev, clade_list_dev;
    // qs_group_support: the label words of the last call (per pass of kGroupHyp hypotheses one word per taxon), kept like the lists above
    std::vector<uint32_t> group_labels;
    DevBuf<uint32_t> group_labels_dev;
};

namespace qs {

// ---- errors: qs_abi.hip ----
extern thread_local std::string g_create_err;   // the error of a failed qs_create (there is no context to hold it)
int fail(qs_ctx *c, int code, const std::string &msg);   // stores msg in c (NULL: in g_create_err), returns code

#define QS_HIP(c, expr)                                                                                 \
    do {                                                                                                \
        hipError_t e__ = (expr);                                                                        \
        if (e__ != hipSuccess)                                                                          \
            return fail((c), e__ == hipErrorOutOfMemory ? QS_ERR_OOM : QS_ERR_HIP,                      \
                        std::string(#expr) + ": " + hipGetErrorString(e__));                            \
    } while (0)

// ---- qs_abi.hip ----
int ensure_n_cu(qs_ctx *c);                  // c->n_cu holds the device's compute units (asked on first use)
uint64_t table_max_count(const qs_ctx *c);   // the largest count a cell of c's table may hold
size_t padded(size_t bytes);                 // the pieces of a staged batch start at 256-byte boundaries
hipError_t ensure_pinned(qs_ctx *c, int slot, size_t need);

// ---- launch order, slices, timing events: qs_abi_count.hip ----
int tile_order(qs_ctx *c, const uint32_t **out);
int drop_tile_order(qs_ctx *c);
uint32_t slice_groups(const qs_ctx *c, size_t group_bytes, uint32_t n_total, bool ab_major);
constexpr uint32_t kEvPrev = ~0u;   // mark: the interval starts at the event recorded before this one
hipError_t mark(qs_ctx *c, int kind, const hipStream_t *on = nullptr, uint32_t from = kEvPrev);

// ---- reference tree and score set-up: qs_abi_score.hip ----
int build_ref_shape(qs_ctx *c, const qs_ref_tree *ref, RefHost &R);
int get_ref(qs_ctx *c, const qs_ref_tree *ref, bool want_dev, const RefHost **out);
void fill_score_device(const qs_ctx *c, const RefHost &R, const uint32_t *lca_dev, ScoreDevice &sd);
int ensure_score_tables(qs_ctx *c);          // the log table of the device QIC for the trees behind c's table
int ensure_bundle_plan(qs_ctx *c, ScoreDevice &sd, int pass);

}  // namespace qs
