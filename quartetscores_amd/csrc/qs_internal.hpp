// qs_internal.hpp -- launcher interface between the C-ABI layer (qs_abi*.hip, qs_plan.hip) and the kernels.
#pragma once
#include <vector>

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qs_common.hpp"

namespace qs {

// Ranks are walked in blocks of consecutive values: the block's first rank is un-ranked once (f64 sqrt / cbrt,
// ~300 instructions), every other rank of the block from it: rank = C(d,4) + C(c,3) + (C(b,2) + a), so adding `off`
// to the pair rank and carrying into c (and d) is enough; unrank2 is a float sqrt and two corrections.
struct Ids4 { uint32_t a, b, c, d; };
__device__ __forceinline__ Ids4 decode_near(const Ids4 &base, uint32_t off) {
    Ids4 r;
    uint32_t c = base.c, d = base.d;
    uint64_t pr = binom2(base.b) + base.a + off;
    for (;;) {
        const uint64_t lim = binom2(c);
        if (pr < lim) break;
        pr -= lim;
        if (++c == d) { ++d; c = 2; }
    }
    unrank2((uint32_t)pr, r.a, r.b);
    r.c = c; r.d = d;
    return r;
}

// Panel element type / kernel mode of one batch
enum PanelBits { PANEL_U8 = 8, PANEL_U16 = 16 };
enum CountMode {
    MODE_BINARY_FULL = 0,  // every tree fully resolved and holding all n taxa: n2 = m - n0 - n1
    MODE_GENERAL_FULL = 1, // multifurcations possible, all taxa present
    MODE_PARTIAL = 2,      // taxa may be missing (flag bit in the panel), multifurcations possible
    MODE_BINARY_PARTIAL = 3 // every tree fully resolved, taxa may be missing (gene trees): n2 = (trees holding all four) - n0 - n1;
                            // bit-sliced kernel only (the byte-SWAR kernel takes such trees as MODE_PARTIAL)
};

// depth limits of the SWAR comparison (see qs_count.hip)
constexpr uint32_t kMaxDepthU8Full = 63;
constexpr uint32_t kMaxDepthU8Partial = 31;
constexpr uint32_t kMaxDepthU16Full = 16383;
constexpr uint32_t kMaxDepthU16Partial = 8191;

// device memory of one uploaded batch (all its arrays in one allocation); last_use: where the compute stream stood when
// the batch was freed (the slab is handed to a later upload, whose copy waits for it)
struct BatchSlab { void *p = nullptr; size_t cap = 0; hipEvent_t last_use = nullptr; };

// one workgroup of clamp_fix_kernel (qs_count.hip): the triples [t_lo, t_hi) (colex order) of the run of `run >> 16` leaves that
// starts at tour position `run & 0xFFFF` of tree `tree`
struct FixUnit { uint32_t tree, run, t_lo, t_hi; };

struct DeviceBatch {
    uint32_t n_trees = 0;
    uint32_t total_leaves = 0;
    uint32_t max_depth = 0;
    bool all_full = false;
    bool all_binary = false;
    // Trees are counted class by class. A class = (kernel mode of the tree -- binary / multifurcating x all taxa / missing
    // taxa --, bits of its deepest LCA), so that every tree runs the cheapest kernel instance that is exact for it: the
    // full binary trees of a batch keep the binary_full instance whatever else the batch holds. Slot s of the class-ordered
    // batch is tree tree_order[s]; class k holds the slots [class_end[k-1], class_end[k]), runs mode class_mode[k] and
    // needs class_bits[k] depth bits (> 10: byte-SWAR kernel). A sub-batch for the panel builders = slots
    // [slot0, slot0 + n_trees).
    uint32_t *tree_order = nullptr; // device, n_trees entries, or NULL = identity
    uint32_t slot0 = 0;
    uint32_t n_classes = 0;
    static constexpr uint32_t kMaxClasses = 32;   // 4 modes x 8 depth classes
    uint32_t class_bits[kMaxClasses] = {0}, class_end[kMaxClasses] = {0}, class_max_depth[kMaxClasses] = {0}, class_mode[kMaxClasses] = {0};
    uint32_t *leaf_off = nullptr;  // device
    uint16_t *leaf_ids = nullptr;  // device
    uint16_t *adj_depth = nullptr; // device
    // scatter-only
    uint32_t n_nodes = 0, n_links = 0;
    uint32_t *node_off = nullptr, *rng_off = nullptr, *node_tree = nullptr;
    uint16_t *ranges = nullptr;
    uint32_t max_tree_nodes = 0;    // most inner nodes of one tree (qs_tree_agreement's grid)
    // depth clamp (qs_plan.hip plan_depth_clamp): the correction units of the trees counted in a class below their own depth bits,
    // ordered by the tree's slot in the class-ordered batch (qs_device_batch::fix_slot = that slot per unit, host)
    FixUnit *fix_units = nullptr;   // device
    uint32_t n_fix = 0;
    uint64_t fix_quartets = 0;      // (tree, quartet) corrections of the whole batch
    uint32_t clamped_trees = 0;
    BatchSlab slab;                 // owns the arrays above
    hipEvent_t ready = nullptr;     // fires when the batch's arrays have arrived (copy stream); the count waits for it
};

struct CountGeometry {
    uint32_t n;          // taxa
    uint32_t d_lo, d_hi; // shard of the largest id
    uint64_t rank_lo;    // C(d_lo,4)
    uint32_t n_dblk;     // d-blocks
    uint32_t total_tiles;
    const uint32_t *dprefix; // device, n_dblk+1
    const uint32_t *cprefix; // device, n+1
    const uint32_t *perm = nullptr; // device, total_tiles: launch slot -> tile id (nullptr = identity); see qs_abi_count.hip tile_order
    // binary_full tiling only: the launch order split for count_bitslice4_kernel. perm_coop: n_coop slots (a multiple of 4;
    // every aligned group of 4 = tiles of one (a-blocks, b-block, d-block), bit 31 = shadow tile that must not store);
    // perm_rest: the n_rest tiles count_bitslice3_kernel still runs. NULL / 0 = everything through count_bitslice3_kernel.
    const uint32_t *perm_coop = nullptr, *perm_rest = nullptr;
    uint32_t n_coop = 0, n_rest = 0;
};

// qs_count.hip
hipError_t launch_build_panel(hipStream_t s, const DeviceBatch &b, uint32_t n, int panel_bits, bool partial, void *panel,
                              uint32_t n_chunks);
hipError_t launch_count_gather(hipStream_t s, const CountGeometry &g, const void *panel, int panel_bits, int mode,
                               uint32_t n_chunks, uint32_t m_trees, void *table, int count_bits, uint32_t *overflow_flag,
                               bool overwrite);
hipError_t launch_build_bitpanel(hipStream_t s, const DeviceBatch &b, uint32_t n, bool partial, void *panel, uint32_t n_groups,
                                 uint32_t compact_nw, // words per panel element: planes (>= 4) [+ presence word]
                                 bool force_general);
hipError_t launch_count_bitslice3(hipStream_t s, const CountGeometry &g, const void *panel, int depth_bits, int mode,
                                  uint32_t n_groups, uint32_t m_trees, void *table, int count_bits, uint32_t *overflow_flag,
                                  bool overwrite, uint32_t *wire, // wire != NULL (binary_full only): one word n0 | n1 << 16 per tuple instead of the table
                                  int order = 0);                 // step order of the instance: 0 = prefetch, 1 = late loads (bitslice3_late_waves != 0), 2 = the six-wave instance (bitslice3_six_waves != 0)
// waves per SIMD of the late-load instance of (mode, depth bits); 0 = the class has none
int bitslice3_late_waves(int mode, int depth_bits);
// ... and of the six-wave instance, whose order ("dma" or "late") names it in the variant string
int bitslice3_six_waves(int mode, int depth_bits);
const char *bitslice3_six_name();
// the classes of a mixed batch that share their depth bits in ONE launch (qs_count_fused.hip); seg_* are indexed by CountMode, a mode
// without trees in this launch has seg_groups = 0
constexpr int kFusedMaxBits = 7;
hipError_t launch_count_bitslice3_fused(hipStream_t s, const CountGeometry &g, const void *const seg_panel[4], const uint32_t seg_groups[4],
                                        const uint32_t seg_trees[4], int depth_bits, void *table, int count_bits, uint32_t *overflow_flag,
                                        bool overwrite);
hipError_t launch_clamp_fix(hipStream_t s, const DeviceBatch &b, const FixUnit *units, uint32_t n_units, uint32_t d_lo, uint32_t d_hi,
                            uint64_t rank_lo, void *table, int count_bits, int mode, uint32_t *wire, uint32_t *overflow_flag); // corrections of the depth clamp (after the class's count kernel)
// out[0 .. ) <- the entries of perm[0 .. n) below `limit`, in their order (at most out_cap are written); scratch: perm_filter_scratch_bytes(n)
size_t perm_filter_scratch_bytes(uint32_t n);
hipError_t launch_perm_filter(hipStream_t s, const uint32_t *perm, uint32_t n, uint32_t limit, uint32_t *out, uint32_t out_cap, uint32_t *scratch);
uint32_t bitslice3_tiles_for_c(uint32_t c); // wave tiles per (d-block, c) of count_bitslice3_kernel
hipError_t launch_count_scatter(hipStream_t s, const DeviceBatch &b, uint32_t n, uint32_t d_lo, uint32_t d_hi,
                                uint64_t rank_lo, void *table, int count_bits, uint32_t *overflow_flag);
hipError_t launch_pack16(hipStream_t s, const void *table_u32, void *dst, uint64_t n_cells, uint32_t *overflow_flag);
hipError_t launch_pack16x2(hipStream_t s, const void *table_u32, void *dst, uint64_t n_tuples, uint32_t trees,
                           uint32_t *overflow_flag, uint32_t *shape_flag);
hipError_t launch_unpack16x2(hipStream_t s, const void *src, void *dst_u16, uint64_t n_tuples, uint32_t trees, uint32_t *shape_flag);
hipError_t launch_pack32x2(hipStream_t s, const void *table_u32, void *dst, uint64_t n_tuples, uint32_t trees, uint32_t *shape_flag);
hipError_t launch_unpack32x2(hipStream_t s, const void *src, void *dst_u32, uint64_t n_tuples, uint32_t trees, uint32_t *shape_flag);
hipError_t launch_sum_words(hipStream_t s, void *dst, const void *const *src, uint32_t n_src, uint64_t n_words, int n_cu); // dst += sum of (peer) sources
hipError_t launch_lookup(hipStream_t s, uint32_t n, uint32_t d_lo, uint32_t d_hi, uint64_t rank_lo, const void *table,
                         int count_bits, uint64_t nq, const uint16_t *abcd_dev, uint64_t *out_dev);
// qs_remap.hip: dst (ids B) <- src (ids A); src_id_of_dev[i] = A-id of B-id i (a permutation of [0, n)); cell widths 32/32, 16/16 or 16 -> 32
hipError_t launch_table_remap(hipStream_t s, const void *src, int src_bits, void *dst, int dst_bits, const uint16_t *src_id_of_dev,
                              uint32_t n, uint64_t n_tuples);
// qs_restrict.hip: dst (n_dst taxa) <- the sub-table of src over the taxa src_id_of_dev[0 .. n_dst) (injective into src's ids); monotone:
// the map is strictly increasing (no sort, slots are the identity); cell widths as above
hipError_t launch_table_restrict(hipStream_t s, const void *src, int src_bits, void *dst, int dst_bits, const uint16_t *src_id_of_dev,
                                 uint32_t n_dst, uint64_t n_tuples, bool monotone);
// qs_collapse.hip: dst (n_dst species) <- the sums of src (n_src individuals) over one individual per species; ids_dev = first_id
// (n_dst + 1 entries) and, from entry 4097 on, the species of every source id; a sum beyond dst's cell width raises *overflow_flag
hipError_t launch_table_collapse(hipStream_t s, const void *src, int src_bits, void *dst, int dst_bits, const uint16_t *ids_dev,
                                 uint32_t n_dst, uint32_t n_src, uint32_t *overflow_flag);
// qs_agree.hip: per-tree quartet agreement with the reference (qs_tree_agreement); the reference's inner nodes with >= 3
// links as id boundaries (ref_off / ref_bnd, ref_par = has a parent link); dst = 4 words per tree of the batch
hipError_t launch_tree_agree(hipStream_t s, const DeviceBatch &b, uint32_t n, uint32_t max_tree_nodes, const uint32_t *ref_off,
                             const uint16_t *ref_bnd, const uint8_t *ref_par, uint32_t n_u, unsigned long long *dst);
// LDS plan of an agreement launch for n taxa: W words per bitmap, the link budget of one round, the inner nodes of one workgroup
void agree_plan(uint32_t n, uint32_t &W, uint32_t &cap, uint32_t &nb);
// qs_agree_pairs.hip: quartet agreement of the trees [r0, r1) of `rows` with the trees [c0, c1) of `cols` (qs_tree_pair_agreement);
// both batches uploaded with node ranges; upper: the two are one batch, pairs with column index <= row index are skipped; work =
// tree_pairs_work_words(...) 16-bit words of workspace (the row trees' position maps and node orders); dst = kPairWords words per pair,
// row-major, overwritten
constexpr int kPairWords = 5;     // concordant, discordant, resolved_row, resolved_col, shared
hipError_t launch_tree_pairs(hipStream_t s, const DeviceBatch &rows, uint32_t r0, uint32_t r1, const DeviceBatch &cols, uint32_t c0,
                             uint32_t c1, bool upper, uint32_t n, uint16_t *work, unsigned long long *dst);
inline size_t tree_pairs_work_words(const DeviceBatch &rows, uint32_t n_rows, uint32_t n) { return (size_t)n_rows * ((size_t)n + rows.max_tree_nodes); }
// qs_taxon.hip: per-taxon sums over the whole rows of the rank range of a ScoreDevice (qs_taxon_support); needs sd.bundle_* =
// plan_bundles with kTaxonWaves waves; dst = 6 words per taxon, zeroed beforehand; wide: counts may reach 2^32 / 192
struct ScoreDevice;
constexpr int kTaxonWaves = 12;   // waves per workgroup = consecutive b per round (the logging pass 1's count, qs_score.hip)
size_t taxon_lds_bytes(uint32_t n);
hipError_t launch_taxon_support(hipStream_t s, const ScoreDevice &sd, bool wide, int n_cu, unsigned long long *dst);
// qs_groups.hip: the six words of up to kGroupHyp group hypotheses over the whole rows of the rank range of a ScoreDevice
// (qs_group_support); needs sd.bundle_* = plan_bundles with kTaxonWaves waves (of sd only n, rank_lo, table, count_bits and the plan are
// read). labw[t] = the labels 0..4 of taxon t, hypothesis h in bits 4h .. 4h+3; split_mask bit h = hypothesis h is a split;
// dst = 6 words per hypothesis, zeroed beforehand; wide: counts may reach 2^32 / 192
constexpr int kGroupHyp = 8;      // hypotheses one read of the table serves
constexpr int kGroupWords = 6;    // quartets, F1, F2, F3, outvoted, uninformed
hipError_t launch_group_support(hipStream_t s, const ScoreDevice &sd, const uint32_t *labw, uint32_t split_mask, uint32_t n_hyp, bool wide,
                                int n_cu, unsigned long long *dst);
// The gathers of the tuples that hold a listed taxon (qs_taxon_walk.hpp), whole tables only: ref_lca as in ScoreDevice; tasks = q | group
// of 64 largest ids << 16, the walks of an n-taxon table, longest first; taxa = the listed ids, one row of dst each (zeroed beforehand)
struct GatherDevice {
    const uint32_t *ref_lca, *tasks;
    const uint16_t *taxa;
    uint32_t n, n_tasks;
    const void *table;
    int count_bits;
};
constexpr int kPlaceWaves = 4;
// qs_place.hip: link sums of the quartet placement of the listed taxa (qs_taxon_placement). child[i][j] = node of the child of lca(i,j)
// that holds leaf j; next[q][p], p < q = the first p' > p at which lca(p',q) or child[q][p'] differs (q if none); inner_node = node index
// of a compact inner id of ref_lca; dst = n_list rows of 2 x n_nodes words; wide: counts may reach 2^32 / 4096
struct PlaceDevice {
    GatherDevice g;
    const uint32_t *inner_node;
    const uint16_t *child, *next;
    uint32_t n_nodes;
};
size_t place_lds_bytes(uint32_t n_nodes);
hipError_t launch_taxon_placement(hipStream_t s, const PlaceDevice &pd, uint32_t n_list, bool wide, int n_cu, unsigned long long *dst);
// qs_taxon_pairs.hip: the eight words of every pair (x, j), x a listed taxon, over the 4-sets that hold both (qs_taxon_pair_support);
// needs nothing beyond the common fields; dst = n_list rows of n x 8 words; wide: counts may reach 2^32 / (4096 x 3)
constexpr int kPairFields = 8;    // n_rt, n_ra, T_rt, S_rt, T_ra, S_ra, T_all, S_all
size_t taxon_pairs_lds_bytes(uint32_t n);
hipError_t launch_taxon_pairs(hipStream_t s, const GatherDevice &pd, uint32_t n_list, bool wide, int n_cu, unsigned long long *dst);
// qs_branch_taxa.hip: per listed taxon x and internode the four words over the 4-sets around the internode that hold x
// (qs_branch_taxon_support). inner_node as in PlaceDevice. par[j] = compact inner id of the parent of inner node j (none: all ones);
// under a degree-2 root with two inner children par[second] = first, dup_from = the second's inner id and dup_to = the first's node
// (else dup_from = all ones). next[i][p] = the first p' > p at which lca(p',i) differs or p' - 1 or p' is i (n if none): run ends on
// both sides of the diagonal. frame as in ScoreDevice. dst = n_list rows of n_nodes x 4 words; wide: counts may reach 2^32 / 4096
struct BranchDevice {
    GatherDevice g;
    const uint32_t *inner_node, *par;
    const uint16_t *next;
    uint32_t n_nodes, n_inner, dup_from, dup_to;
    int frame;
};
constexpr int kBranchWords = 4;   // quartets, F1, F2, F3
size_t branch_taxa_lds_bytes(uint32_t n_inner);
hipError_t launch_branch_taxa(hipStream_t s, const BranchDevice &bd, uint32_t n_list, bool wide, int n_cu, unsigned long long *dst);
// ... and the same words over ALL 4-sets around every internode, picked from the node-pair sums of a score pass 1: edge_key[v] = the
// key of the node pair at the ends of the internode above node v (all ones: none), quartets[v] = its number of 4-sets
hipError_t launch_branch_totals(hipStream_t s, const unsigned long long *sums, const uint32_t *edge_key, const unsigned long long *quartets,
                                uint32_t n_nodes, unsigned long long *dst);
// qs_tree_branch.hip: per tree of the batch and internode of the reference the four words (4-sets inside the tree's taxa, q1, q2, q3)
// over the 4-sets around the internode (qs_tree_branch_support). edges = n_e records of kTreeBranchEdgeWords words: node of the lower
// end v, second node that gets the same words (all ones: none; under a degree-2 root its other inner child), offset into bnd and
// number of v's children, the same two of the upper end w, v's index among w's children (all ones: none, the two are the children of
// a degree-2 root) and whether w has a parent link. bnd = per inner node its children's first ids in id order and the id behind the
// last. frame as in ScoreDevice. dst = n_trees rows of n_nodes x 4 words, overwritten
constexpr int kTreeBranchEdgeWords = 8;
hipError_t launch_tree_branch(hipStream_t s, const DeviceBatch &b, uint32_t n, uint32_t max_tree_nodes, const uint32_t *edges, const uint16_t *bnd,
                              uint32_t n_e, uint32_t n_nodes, int frame, unsigned long long *dst);
// ... and dst[rep][cell] += sum over t of weights[rep][t] x rows[t][cell] (qs_branch_resample); weights on the device, n_rep x n_trees
hipError_t launch_branch_resample(hipStream_t s, const long long *rows, uint32_t n_trees, uint32_t cells, const uint32_t *weights, uint32_t n_rep,
                                  unsigned long long *dst);
// ... and dst[node] += (trees with q1 + q2 + q3 > 0, sum over them of floor(q_i x 2^40 / (q1 + q2 + q3)), i = 1..3) (qs_branch_frequencies)
hipError_t launch_branch_frequencies(hipStream_t s, const long long *rows, uint32_t n_trees, uint32_t n_nodes, unsigned long long *dst);
// qs_tree_taxa.hip: per tree of the batch and taxon id the four words (concordant, discordant, resolved in the tree, resolved in the
// reference) over the 4-sets of the tree's taxa that hold the taxon (qs_tree_taxon_agreement); the reference's nodes as for
// launch_tree_agree. dst = n_trees rows of n x 4 words, overwritten
constexpr int kTreeTaxaWords = 4;
// LDS plan of such a launch for n taxa: W words per bitmap, `flight` links of a node with their two difference arrays (diff_bytes in
// all) in LDS at once, the link bitmaps of one round (cap), the inner nodes of one workgroup (nb), the dynamic LDS of the launch
struct TreeTaxaPlan { uint32_t W, cap, nb, flight, diff_bytes, lds_bytes; };
bool tree_taxa_plan(uint32_t n, TreeTaxaPlan &p);   // false: more taxa than the plan supports (cap and lds_bytes are 0)
uint32_t tree_taxa_max_taxa();                      // the largest n that tree_taxa_plan accepts
hipError_t launch_tree_taxa(hipStream_t s, const DeviceBatch &b, uint32_t n, uint32_t max_tree_nodes, const uint32_t *ref_off,
                            const uint16_t *ref_bnd, const uint8_t *ref_par, uint32_t n_u, unsigned long long *dst);
// qs_place_clade.hip: link sums of the quartet placement of listed clades (qs_clade_placement); whole tables only. ref_lca, inner_node,
// child, next as in PlaceDevice. tasks = d | group of 64 largest ids << 16 by d ascending, in the numbering of the ids OUTSIDE a clade:
// the walk of the middle id n_outside - 1 - d (d = 1 ..: the longest walks first), so that the first clades[4 i + 3] entries are the walks
// of clade i whatever its size. clades = per listed clade lo, hi, x-slice length, walks. groups = per workgroup the clade's list index
// and (its number among the clade's workgroups | their count << 16). dst = one row of 2 x n_nodes words per clade, zeroed beforehand;
// wide: (n - |C|) x slice x (largest count) may reach 2^32
struct CladeDevice {
    const uint32_t *ref_lca, *inner_node, *tasks, *clades, *groups;
    const uint16_t *child, *next;
    uint32_t n, n_nodes;
    const void *table;
    int count_bits;
};
hipError_t launch_clade_placement(hipStream_t s, const CladeDevice &cd, uint32_t n_groups, bool wide, unsigned long long *dst);
size_t gather_lds_bytes(uint32_t d_hi);
uint32_t gather_tiles_for_c(uint32_t c); // workgroups of the gather kernel per (d-block, c)

// qs_score.hip
struct ScoreDevice {
    const uint32_t *ref_lca; // n*n: (depth << 16) | inner-node compact id, for leaf pairs (lookup ids)
    uint32_t n, n_inner;
    uint32_t d_lo, d_hi;
    uint64_t rank_lo, n_tuples;
    const void *table;
    int count_bits;
    unsigned long long *pair_sums; // n_inner*n_inner*3
    long long *pair_min;           // n_inner*n_inner (f64_to_sortable of the device QIC)
    unsigned long long *pair_cand; // n_inner*n_inner*kCand
    uint32_t cand_limit;           // candidate slots pass 2 may fill per node pair (kCand; smaller in tests)
    unsigned long long *list;      // pass 3 (qs_score_overflow): 4 words (key, q1, q2, q3) per near-minimal quartet of a marked pair;
                                   // pass 1 with list != NULL: the candidate log of the single-read scoring (same records)
    unsigned long long *list_count, list_cap;
    unsigned long long *last_trip; // logging pass 1: per node pair the packed (q1 << 42 | q2 << 21 | q3) of the record logged last for it (all
                                   // ones = none), or NULL: a quartet whose triple equals it is not logged again (ties at the bound)
    uint32_t *flags;               // [0] bit 0: a pair's candidate slots overflowed, bit 1: a reduced triple did not fit the packed slot
    const uint16_t *ref_next; // n*n: for a < b the first a' > a with lca(a',b) != lca(a,b), b if there is none
    const double *logk;            // log(k) (0 at k = 0) for k < tbl_n: integer arguments of the device QIC
    uint32_t tbl_n;
    uint32_t lds_n;                // leading entries of logk the scan kernel keeps in LDS
    const uint32_t *bundle_plo;    // bundle kernel (plan_bundles): per b the first pair index and the number of pairs (c,d) whose rows are scored
    const uint32_t *bundle_pcnt;
    const uint32_t *bundle_rounds; // n_rounds x (b / 16, pair group)
    uint32_t n_rounds;
    uint32_t coop_load;            // bundle kernel: 1 = a row's 96-byte chunk is loaded by eight lanes and handed over through LDS (QS_TUNE_SCORE_LOAD)
    uint32_t sample;               // pass 1, bundle kernel: 0 = every chunk; else the minima-only pre-pass of the single-read scoring:
                                   //    bits 0..15 = S (a power of two): one chunk (bit 16 clear) or one round (bit 16 set) in S
    uint32_t root_split;           // bifurcating reference with a degree-2 root: ids [0, root_split) lie under the root's first child (else 0);
                                   //    marks the quartets the reference evaluates in both (q2, q3) orders (qs_score.hip root_swapped)
    int frame;                     // 0: node-pair frame of processNodePair (QSC:417-431); 1: the (u,z|v,w) argument
                                   //    order of the multifurcating / raw-QIC loops (QSC:551-558, 661-668)
};
constexpr int kCand = 8;
constexpr unsigned long long kCandEmpty = ~0ull;
constexpr unsigned long long kCandOverflow = ~0ull - 1; // in the LAST slot of a node pair: its slots did not suffice (qs_score_overflow)
constexpr unsigned long long kCandSwap = 1ull << 63;    // candidate slot flag: the reference also evaluates log_score(q1, q3, q2) for it (degree-2 root)
constexpr unsigned long long kListSwap = 1ull << 32;    // the same flag in the key word of a (key, q1, q2, q3) record (candidate log, overflow lists)
uint32_t score_scan_max_lds_log(bool coop_load = false);
// kernel: 0 = bundle kernel (a wave walks 64 rows with the same b in lockstep; needs sd.bundle_* = plan_bundles of the
// rank range, and the partial rows at its ends, which go through the scan kernel), 1 = scan kernel (lane = 8 consecutive ranks)
struct BundlePlan { std::vector<uint32_t> plo, pcnt, rounds; uint64_t part_lo[2], part_n[2]; int n_parts; };
void plan_bundles(uint32_t n, uint64_t r0, uint64_t r1, uint32_t waves, BundlePlan &out);
uint32_t score_bundle_waves(int pass, bool coop_load = false);   // waves per workgroup (= consecutive b per round) of the bundle kernel in pass 1 / 2; cooperative loads: their own count
hipError_t launch_score_pass1(hipStream_t s, const ScoreDevice &sd, int kernel, int n_cu, const uint64_t *part_lo, const uint64_t *part_n, int n_parts, double tol = 0.0);
hipError_t launch_score_log(hipStream_t s, const ScoreDevice &sd, double tol, unsigned long long n_rec); // single-read scoring: filter pass 1's candidate log (sd.list)
hipError_t launch_score_pass2(hipStream_t s, const ScoreDevice &sd, double tol, int kernel, int n_cu, const uint64_t *part_lo, const uint64_t *part_n, int n_parts);
hipError_t launch_score_overflow_list(hipStream_t s, const ScoreDevice &sd, double tol);
// sums of the node pairs (degree-2 root, v): pairs_dev = RootPairHost records (qs_abi_score.hip), total = number of (v,a,b,c,d) items
struct RootPairHost { uint32_t s1_lo, s1_n, s2_lo, s2_n, s3_lo, s3_n, s4_lo, s4_n, key, pad; unsigned long long first; };
hipError_t launch_root_pair_sums(hipStream_t s, const ScoreDevice &sd, const void *pairs_dev, uint32_t n_pairs, uint64_t total);
hipError_t launch_raw_qic(hipStream_t s, const ScoreDevice &sd, uint64_t r0, uint64_t nq, uint8_t *topo_dev,
                          unsigned long long *q_dev);
hipError_t launch_raw_qic_lex(hipStream_t s, const ScoreDevice &sd, uint64_t i0, uint64_t nq, uint8_t *topo_dev,
                              unsigned long long *q_dev);

} // namespace qs
