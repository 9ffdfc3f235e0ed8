// qs_plan.hip -- host-only planning behind the C-ABI: the launch order of the count kernel's tiles, the depth-clamp plan, the classes
// of a batch, where a slice is split, the shard bounds, the score plan. Plain functions of their arguments: no context, no device call.
#include "../../include/quartetscores_hip.h"
#include "qs_common.hpp"
#include "qs_internal.hpp"
#include "qs_plan.hpp"

#include <algorithm>
#include <initializer_list>
#include <string>
#include <utility>
#include <vector>

using namespace qs;

// Host part of the launch order: the (a,b)-major enumeration of the 16x8 tiles of count_bitslice3_kernel (two a-columns per lane in
// every instance since round 4) as launch slot -> tile id, checked to be a bijection. Pure host code (no context, no HIP):
// qs_create starts it on a helper thread BEFORE its first HIP call, so that in a fresh process the ~25 ms it takes at 512 taxa pass
// while the HIP runtime comes up (round 5: the CLI's first launch 25 ms earlier).
bool qs::build_tile_perm(const TilePermParams &P, const std::vector<uint32_t> &cp, const std::vector<uint32_t> &dp, std::vector<uint32_t> &perm,
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

// ---- depth clamp (qs_count.hip clamp_fix_kernel): the plan -- "plan_depth_clamp" in qs_count.hip's comments and DESIGN.md = clamp_cost +
// clamp_choice below and the class rules of qs_batch_upload ------------------------------------------------------------------------
// (tree, quartet) corrections a tree costs when its LCA depths are cut at `cut`: the quartets with at least three leaves in one
// maximal run of tour-adjacent LCA depths >= cut (a subtree below a node of depth `cut`): C(s,3)(L - s) + C(s,4) per run of s
// leaves. ~0 when a run is longer than the kernel's LDS table takes. runs (optional): (first position, leaves) of every run.
constexpr uint32_t kClampMaxRun = 128;  // = kFixMaxRun of qs_count.hip
uint64_t qs::clamp_cost(const uint16_t *adj, uint32_t L, uint32_t cut, std::vector<std::pair<uint32_t, uint32_t>> *runs) {
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
uint32_t qs::depth_class_of(uint32_t depth) {   // depth bits of a tree's class: 4 .. 10, 11 = beyond the bit-sliced instances
    uint32_t bb = 1;
    while ((1u << bb) <= depth) ++bb;
    return bb <= 4 ? 4u : (bb <= 10 ? bb : 11u);
}
// The cheapest class (depth bits) a tree may be counted in: its own, or a lower one when the corrections of the cut stay within
// `budget_per_bit` (tree, quartet) pairs per bit saved -- soft: the rule for every tree; hard (16 x): for the trees of a class
// that would otherwise be too small to pay for its own pass over the table.
void qs::clamp_choice(const uint16_t *adj, uint32_t L, uint32_t own_bits, uint64_t budget_per_bit, uint8_t &soft, uint8_t &hard) {
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
// deepest adjacent LCA and "fully resolved" of one tree from its adjacent-LCA depth sequence
void qs::tree_shape(const uint16_t *adj, uint32_t L, std::vector<uint32_t> &stack, uint32_t &depth, bool &binary) {
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
void qs::plan_classes(uint32_t n, uint32_t nt, const uint32_t *leaf_off, const uint16_t *adj_depth, const TreeFacts &F, uint32_t class_min,
                      uint32_t class_pct, uint32_t clamp_ppm, ClassPlan &P, bool fuse) {
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

// ---- group hypotheses: what a label pattern asserts and how many 4-sets of the whole table it counts ------------------------------
bool qs::group_classify(uint32_t n, const uint8_t *labels, uint32_t n_hyp, uint8_t *kind, uint64_t *quartets, std::string &err) {
    for (uint32_t h = 0; h < n_hyp; ++h) {
        uint64_t cnt[5] = {0, 0, 0, 0, 0};
        const uint8_t *row = labels + (size_t)h * n;
        for (uint32_t t = 0; t < n; ++t) {
            if (row[t] > 4) { err = "hypothesis " + std::to_string(h) + ": taxon " + std::to_string(t) + " carries label " + std::to_string(row[t]) + " (labels are 0..4)"; return false; }
            cnt[row[t]]++;
        }
        const std::string who = "hypothesis " + std::to_string(h) + ": ";
        if (cnt[3] || cnt[4]) {   // a quad: S1 S2 | S3 S4
            for (uint32_t l = 1; l <= 4; ++l)
                if (!cnt[l]) { err = who + "no taxon carries label " + std::to_string(l) + " (a quad hypothesis needs labels 1, 2, 3 and 4)"; return false; }
            if (kind) kind[h] = 0;
            if (quartets) quartets[h] = cnt[1] * cnt[2] * cnt[3] * cnt[4];
        } else {                  // a split: S1 | S2
            for (uint32_t l = 1; l <= 2; ++l)
                if (cnt[l] < 2) {
                    err = who + (cnt[l] ? "only one taxon carries label " : "no taxon carries label ") + std::to_string(l) + " (a split hypothesis needs two taxa on either side)";
                    return false;
                }
            if (kind) kind[h] = 1;
            if (quartets) quartets[h] = binom2(cnt[1]) * binom2(cnt[2]);
        }
    }
    return true;
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
