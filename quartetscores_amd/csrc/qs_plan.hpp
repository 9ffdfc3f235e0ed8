// qs_plan.hpp -- host-only planning of the count step (qs_plan.hip): what qs_abi.hip and qs_abi_count.hip call of it. No context,
// no device.
#pragma once
#include "qs_internal.hpp"

#include <stdint.h>
#include <string>
#include <utility>
#include <vector>

namespace qs {

// ---- launch order ----
struct TilePermParams { uint32_t chunk, cblock_in, cgroup, d_hi, n_dblk, total; };
bool build_tile_perm(const TilePermParams &P, const std::vector<uint32_t> &cp, const std::vector<uint32_t> &dp, std::vector<uint32_t> &perm,
                     std::string &err);

// ---- depth clamp ----
uint64_t clamp_cost(const uint16_t *adj, uint32_t L, uint32_t cut, std::vector<std::pair<uint32_t, uint32_t>> *runs);
uint32_t depth_class_of(uint32_t depth);
void clamp_choice(const uint16_t *adj, uint32_t L, uint32_t own_bits, uint64_t budget_per_bit, uint8_t &soft, uint8_t &hard);

// ---- classes of a batch ----
// What validation knows about every tree: its deepest LCA, the cheapest kernel mode that is exact for it, and the lowest depth class
// the clamp budget allows it (soft: the rule for every tree; hard: 16 x, for the trees of a class too small for a pass of its own).
struct TreeFacts { std::vector<uint16_t> depth; std::vector<uint8_t> mode, soft, hard; };
void tree_shape(const uint16_t *adj, uint32_t L, std::vector<uint32_t> &stack, uint32_t &depth, bool &binary);
struct ClassPlan {
    uint32_t n_classes = 0;
    uint32_t class_mode[DeviceBatch::kMaxClasses] = {0}, class_bits[DeviceBatch::kMaxClasses] = {0}, class_end[DeviceBatch::kMaxClasses] = {0},
             class_max_depth[DeviceBatch::kMaxClasses] = {0};
    std::vector<uint32_t> order;       // slot -> tree (empty = identity: one class)
    std::vector<uint8_t> bits, mode;   // per tree: depth bits and kernel mode of the class it is counted in
};
void plan_classes(uint32_t n, uint32_t nt, const uint32_t *leaf_off, const uint16_t *adj_depth, const TreeFacts &F, uint32_t class_min,
                  uint32_t class_pct, uint32_t clamp_ppm, ClassPlan &P, bool fuse = false);

// ---- group hypotheses (qs_group_check, qs_group_support) ----
// labels[h * n + t] in 0..4 for n_hyp hypotheses over n taxa: kind (0 quad: labels 1..4 all occur; 1 split: only 1 and 2, each on at
// least two taxa) and the whole-table number of counted 4-sets of each. false: err names the first hypothesis that is neither.
bool group_classify(uint32_t n, const uint8_t *labels, uint32_t n_hyp, uint8_t *kind, uint64_t *quartets, std::string &err);

}  // namespace qs
