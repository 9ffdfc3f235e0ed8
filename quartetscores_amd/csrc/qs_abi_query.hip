// qs_abi_query.hip -- what reads a finished table and is not the score: per-taxon, per-pair and per-branch-and-taxon support, taxon and clade placement, per-tree
// agreement, per-tree-and-taxon agreement and per-tree support of every branch with its resampling (against a reference tree; these
// read the trees, not a table),
// the agreement of the evaluation trees with each other and the support of taxon groups (against none). Host code only; the kernels are
// in qs_taxon.hip, qs_taxon_pairs.hip, qs_branch_taxa.hip, qs_place.hip, qs_place_clade.hip, qs_agree.hip, qs_tree_taxa.hip,
// qs_tree_branch.hip, qs_agree_pairs.hip and qs_groups.hip.
#include "qs_ctx.hpp"
#include "qs_plan.hpp"

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

using namespace qs;

// The refusals the table queries share. Every entry point calls them in an order of its own, which its callers see (a 3000-taxon shard
// is refused for its taxa, not for being a shard): they are not one prologue.
static int need_args(qs_ctx *c, const char *who, bool all_given) {
    return all_given ? QS_OK : fail(c, QS_ERR_ARG, std::string(who) + ": NULL argument");
}
static int need_aligned(qs_ctx *c, const char *who, const void *p, const char *name = "dst_device") {
    return reinterpret_cast<uintptr_t>(p) % 8 ? fail(c, QS_ERR_ARG, std::string(who) + ": " + name + " is not 8-byte aligned") : QS_OK;
}
static int need_table(qs_ctx *c, const char *who) { return c->table ? QS_OK : fail(c, QS_ERR_STATE, std::string(who) + ": no table"); }
static int need_whole_table(qs_ctx *c, const char *who, const char *unit) {
    if (c->d_lo == 0 && c->d_hi == c->n) return QS_OK;
    return fail(c, QS_ERR_UNSUPPORTED, std::string(who) + ": a table-shard context (the walks of a " + unit + " cross every shard: use a whole-table one)");
}
// every sum over the 4-sets that hold one taxon is at most C(n-1,3) x (largest count): the trees behind the table if known, else what
// a cell can hold
static int need_taxon_sums_fit(qs_ctx *c, const char *who, uint64_t max_count) {
    const uint64_t per_taxon = c->n >= 4 ? (uint64_t)(c->n - 1) * (c->n - 2) / 2 * (c->n - 3) / 3 : 0;
    if (per_taxon && max_count > (uint64_t)INT64_MAX / per_taxon)
        return fail(c, QS_ERR_OVERFLOW, std::string(who) + ": C(n-1,3) x the largest possible count exceeds 63 bits");
    return QS_OK;
}

// Per-taxon quartet support of this context's table against the reference tree (qs_taxon.hip). The reference has no such
// output: this replaces nothing there (the nearest is printRawQICScores, one text line per quartet).
extern "C" int qs_taxon_support(qs_ctx *c, const qs_ref_tree *ref, int64_t *dst_device) {
    if (!c) return QS_ERR_ARG;
    const char *who = "qs_taxon_support";
    if (int rc = need_args(c, who, dst_device)) return rc;
    if (int rc = need_aligned(c, who, dst_device)) return rc;
    if (int rc = need_table(c, who)) return rc;
    if (taxon_lds_bytes(c->n) > 160u * 1024u) return fail(c, QS_ERR_UNSUPPORTED, "qs_taxon_support: more than 3413 taxa (the accumulators of a workgroup live in LDS)");
    const uint64_t max_count = table_max_count(c);
    if (int rc = need_taxon_sums_fit(c, who, max_count)) return rc;
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

// Host-only: kind and whole-table number of counted 4-sets of every hypothesis, or the first malformed one (qs_plan.hip group_classify).
extern "C" int qs_group_check(uint32_t n_taxa, const uint8_t *labels, uint32_t n_hyp, uint8_t *kind_out, uint64_t *quartets_out) {
    if (!labels) return fail(nullptr, QS_ERR_ARG, "qs_group_check: NULL argument");
    if (n_hyp == 0) return fail(nullptr, QS_ERR_ARG, "qs_group_check: n_hyp must be at least 1");
    if (n_taxa < 4 || n_taxa > 65535) return fail(nullptr, QS_ERR_ARG, "qs_group_check: n_taxa must be 4 .. 65535");
    std::string err;
    if (!group_classify(n_taxa, labels, n_hyp, kind_out, quartets_out, err)) return fail(nullptr, QS_ERR_ARG, "qs_group_check: " + err);
    return QS_OK;
}

// The six words of every group hypothesis over this context's table (qs_groups.hip). Replaces nothing in the reference; the nearest is
// the metaquartet sum of processNodePair, which knows only the four subtrees beside a node pair of the reference tree.
extern "C" int qs_group_support(qs_ctx *c, const uint8_t *labels, uint32_t n_hyp, int64_t *dst_device) {
    if (!c) return QS_ERR_ARG;
    const char *who = "qs_group_support";
    if (int rc = need_args(c, who, labels && dst_device)) return rc;
    if (int rc = need_aligned(c, who, dst_device)) return rc;
    if (n_hyp == 0) return fail(c, QS_ERR_ARG, "qs_group_support: n_hyp must be at least 1");
    if (int rc = need_table(c, who)) return rc;
    const uint32_t n = c->n;
    std::vector<uint8_t> kind(n_hyp);
    std::vector<uint64_t> quartets(n_hyp);
    {
        std::string err;
        if (!group_classify(n, labels, n_hyp, kind.data(), quartets.data(), err)) return fail(c, QS_ERR_ARG, "qs_group_support: " + err);
    }
    // every sum is at most (counted 4-sets of the whole table) x (largest count): the trees behind the table if known, else what a cell can hold
    const uint64_t max_count = table_max_count(c);
    for (uint32_t h = 0; h < n_hyp; ++h)
        if (quartets[h] && max_count > (uint64_t)INT64_MAX / quartets[h])
            return fail(c, QS_ERR_OVERFLOW, "qs_group_support: the counted 4-sets x the largest possible count exceed 63 bits for hypothesis " + std::to_string(h));
    QS_HIP(c, hipSetDevice(c->device));
    ScoreDevice sd{};
    sd.n = n; sd.d_lo = c->d_lo; sd.d_hi = c->d_hi;
    sd.rank_lo = c->rank_lo; sd.n_tuples = c->n_tuples; sd.table = c->table; sd.count_bits = (int)c->count_bits;   // the context's own table, not a scoring view
    if (int rc = ensure_bundle_plan(c, sd, 3)) return rc;   // (the per-taxon pass' rounds: the same rows, the same waves)
    // (a context's table is cut by the largest id: it starts and ends at a row start, plan_bundles finds no partial rows)
    if (c->bundle[2].n_parts) return fail(c, QS_ERR_UNSUPPORTED, "qs_group_support: the table does not start and end at a row start");
    const uint32_t n_pass = (n_hyp + kGroupHyp - 1) / kGroupHyp;
    QS_HIP(c, hipStreamSynchronize(c->stream));   // (an earlier call's kernels and upload may still read the old label words)
    c->group_labels.assign((size_t)n_pass * n, 0u);
    for (uint32_t h = 0; h < n_hyp; ++h) {
        uint32_t *w = c->group_labels.data() + (size_t)(h / kGroupHyp) * n;
        for (uint32_t t = 0; t < n; ++t) w[t] |= (uint32_t)labels[(size_t)h * n + t] << (4 * (h % kGroupHyp));
    }
    QS_HIP(c, c->group_labels_dev.reserve(c->group_labels.size() * 4, nullptr));
    QS_HIP(c, hipMemcpyAsync(c->group_labels_dev.get(), c->group_labels.data(), c->group_labels.size() * 4, hipMemcpyHostToDevice, c->stream));
    QS_HIP(c, hipMemsetAsync(dst_device, 0, (size_t)n_hyp * kGroupWords * 8, c->stream));
    const bool wide = max_count >= (1ull << 32) / 192;   // the per-taxon pass' rule: 64 lanes x 3 counts in a 32-bit partial sum
    for (uint32_t p = 0; p < n_pass; ++p) {
        const uint32_t h0 = p * kGroupHyp, nh = std::min<uint32_t>(kGroupHyp, n_hyp - h0);
        uint32_t split_mask = 0;
        for (uint32_t i = 0; i < nh; ++i) split_mask |= (uint32_t)kind[h0 + i] << i;
        QS_HIP(c, launch_group_support(c->stream, sd, c->group_labels_dev.get() + (size_t)p * n, split_mask, nh, wide, c->n_cu,
                                       reinterpret_cast<unsigned long long *>(dst_device) + (size_t)h0 * kGroupWords));
    }
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

// qs_taxon_placement, qs_taxon_pair_support: the caller's list (NULL = all taxa in id order) checked and copied
static int check_taxon_list(qs_ctx *c, const char *who, const uint16_t *taxa, uint32_t n_list, std::vector<uint16_t> &list) {
    const std::string w(who);
    if (taxa ? n_list == 0 || n_list > c->n : n_list != c->n) return fail(c, QS_ERR_ARG, w + (taxa ? ": the list needs 1 .. n_taxa entries" : ": n_list must be n_taxa when taxa is NULL"));
    list.resize(n_list);
    std::vector<uint8_t> seen(c->n, 0);
    for (uint32_t i = 0; i < n_list; ++i) {
        const uint32_t x = taxa ? taxa[i] : i;
        if (x >= c->n) return fail(c, QS_ERR_ARG, w + ": taxon id out of range");
        if (seen[x]) return fail(c, QS_ERR_ARG, w + ": taxon id " + std::to_string(x) + " is listed twice");
        seen[x] = 1; list[i] = (uint16_t)x;
    }
    return QS_OK;
}

// ... and the walks of an n-taxon table and that list on the device
static int ensure_place_walks(qs_ctx *c, const std::vector<uint16_t> &list) {
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
        QS_HIP(c, hipMemcpyAsync(c->place_taxa_dev.get(), c->place_taxa.data(), list.size() * 2, hipMemcpyHostToDevice, c->stream));
    }
    return QS_OK;
}

// ... and what every gather over that list reads (after ensure_place_walks)
static GatherDevice gather_device(const qs_ctx *c) {
    GatherDevice g;
    g.ref_lca = c->ref_lca_dev.get(); g.tasks = c->place_tasks_dev.get(); g.taxa = c->place_taxa_dev.get();
    g.n = c->n; g.n_tasks = (uint32_t)c->place_tasks.size();
    g.table = c->table; g.count_bits = (int)c->count_bits;   // the context's own table, not a scoring view
    return g;
}

// Link sums of the quartet placement of the listed taxa (qs_place.hip). The reference never asks where the evaluation trees would
// put a taxon: this replaces nothing there.
extern "C" int qs_taxon_placement(qs_ctx *c, const qs_ref_tree *ref, const uint16_t *taxa, uint32_t n_list, int64_t *dst_device) {
    if (!c) return QS_ERR_ARG;
    const char *who = "qs_taxon_placement";
    if (int rc = need_args(c, who, dst_device)) return rc;
    if (int rc = need_aligned(c, who, dst_device)) return rc;
    if (int rc = need_table(c, who)) return rc;
    const uint64_t max_count = table_max_count(c);
    if (int rc = need_taxon_sums_fit(c, who, max_count)) return rc;
    if (int rc = need_whole_table(c, who, "taxon")) return rc;
    std::vector<uint16_t> list;
    if (int rc = check_taxon_list(c, who, taxa, n_list, list)) return rc;
    QS_HIP(c, hipSetDevice(c->device));
    const RefHost *Rp = nullptr;
    if (int rc = get_ref(c, ref, true, &Rp)) return rc;
    if (place_lds_bytes(Rp->n_nodes) > 160u * 1024u)
        return fail(c, QS_ERR_UNSUPPORTED, "qs_taxon_placement: more than 10240 nodes (the link sums of a workgroup live in LDS)");
    if (int rc = ensure_place_ref(c, *Rp)) return rc;
    if (int rc = ensure_n_cu(c)) return rc;
    if (int rc = ensure_place_walks(c, list)) return rc;
    PlaceDevice pd;
    pd.g = gather_device(c);
    pd.inner_node = c->place_node_dev.get(); pd.child = c->place_child_dev.get(); pd.next = c->place_next_dev.get();
    pd.n_nodes = Rp->n_nodes;
    QS_HIP(c, hipMemsetAsync(dst_device, 0, (size_t)n_list * 2 * Rp->n_nodes * 8, c->stream));
    // 32-bit partial sums: a walk has q < n_taxa steps, so 4096 x (largest count) < 2^32 suffices only while n_taxa <= 4096
    // (qs_create's cap today; the LDS limit alone would allow more)
    const bool wide = max_count >= (1ull << 32) / 4096 || c->n > 4096;
    QS_HIP(c, launch_taxon_placement(c->stream, pd, n_list, wide, c->n_cu, reinterpret_cast<unsigned long long *>(dst_device)));
    return QS_OK;   // asynchronous on the context's stream
}

// The eight words of every pair (listed taxon, other taxon) over the 4-sets that hold both (qs_taxon_pairs.hip). The reference has no
// output per pair of taxa: this replaces nothing there.
extern "C" int qs_taxon_pair_support(qs_ctx *c, const qs_ref_tree *ref, const uint16_t *taxa, uint32_t n_list, int64_t *dst_device) {
    if (!c) return QS_ERR_ARG;
    const char *who = "qs_taxon_pair_support";
    if (int rc = need_args(c, who, dst_device)) return rc;
    if (int rc = need_aligned(c, who, dst_device)) return rc;
    if (int rc = need_table(c, who)) return rc;
    if (taxon_pairs_lds_bytes(c->n) > 160u * 1024u) return fail(c, QS_ERR_UNSUPPORTED, "qs_taxon_pair_support: more than 2560 taxa (the accumulators of a workgroup live in LDS)");
    if (int rc = need_whole_table(c, who, "taxon")) return rc;
    std::vector<uint16_t> list;
    if (int rc = check_taxon_list(c, who, taxa, n_list, list)) return rc;
    // (a word is at most C(n-2,2) x 3 x (largest count) < 2^23 x 2^34: no overflow to refuse)
    const uint64_t max_count = table_max_count(c);
    QS_HIP(c, hipSetDevice(c->device));
    const RefHost *Rp = nullptr;
    if (int rc = get_ref(c, ref, true, &Rp)) return rc;
    if (int rc = ensure_n_cu(c)) return rc;
    if (int rc = ensure_place_walks(c, list)) return rc;
    const GatherDevice pd = gather_device(c);
    QS_HIP(c, hipMemsetAsync(dst_device, 0, (size_t)n_list * c->n * kPairFields * 8, c->stream));
    // 32-bit partial sums: a walk has q < 4096 steps of up to three counts each
    const bool wide = max_count >= (1ull << 32) / (4096 * 3);
    QS_HIP(c, launch_taxon_pairs(c->stream, pd, n_list, wide, c->n_cu, reinterpret_cast<unsigned long long *>(dst_device)));
    return QS_OK;   // asynchronous on the context's stream
}

// qs_branch_taxon_support: the internodes of the cached reference tree on the device, beside its LCA matrix
static int ensure_branch_ref(qs_ctx *c, const RefHost &R) {
    if (c->branch_next_dev) return QS_OK;
    const uint32_t n = R.n, N = R.n_nodes, NI = R.n_inner, none = 0xFFFFFFFFu;
    // next[i][p]: the end of the run of p over which lca(p,i) stays the same, on either side of the diagonal (a run ends in front of i
    // and behind it: the sorted order of a 4-set changes there)
    c->branch_next.assign((size_t)n * n, 0);
    for (uint32_t i = 0; i < n; ++i) {
        const size_t o = (size_t)i * n;
        c->branch_next[o + n - 1] = (uint16_t)n;
        for (uint32_t p = n - 1; p-- > 0;)
            c->branch_next[o + p] = (R.lca[o + p] != R.lca[o + p + 1] || p == i || p + 1 == i) ? (uint16_t)(p + 1) : c->branch_next[o + p + 1];
    }
    // the internode above a node v: both ends inner nodes; under a degree-2 root its two inner children are the ends of one
    std::vector<std::vector<uint32_t>> kids(N);
    for (uint32_t v = 0; v < N; ++v)
        if (R.parent[v] >= 0) kids[(uint32_t)R.parent[v]].push_back(v);
    for (auto &k : kids) std::sort(k.begin(), k.end(), [&](uint32_t a, uint32_t b) { return R.leaf_lo[a] < R.leaf_lo[b]; });
    auto pairs_of_links = [&](uint32_t v, uint32_t without, bool up) {   // sum over two different links of v of the product of their sizes
        uint64_t s = 0, s2 = 0;
        for (uint32_t k : kids[v]) if (k != without) { s += R.leaf_cnt[k]; s2 += (uint64_t)R.leaf_cnt[k] * R.leaf_cnt[k]; }
        if (up && R.parent[v] >= 0) { const uint64_t o = n - R.leaf_cnt[v]; s += o; s2 += o * o; }
        return (s * s - s2) / 2;
    };
    c->branch_words.assign((size_t)2 * NI + N, none);
    uint32_t *par = c->branch_words.data(), *node = par + NI, *edge_key = node + NI;
    c->branch_quartets.assign(N, 0);
    c->branch_dup_from = none; c->branch_dup_to = 0;
    for (uint32_t j = 0; j < NI; ++j) node[j] = R.inner_node[j];
    const bool merged = R.root_deg2 && R.nchild[kids[R.root][0]] > 0 && R.nchild[kids[R.root][1]] > 0;
    for (uint32_t v = 0; v < N; ++v) {
        if (R.nchild[v] == 0 || R.parent[v] < 0) continue;
        const uint32_t u = (uint32_t)R.parent[v];
        uint32_t w = u;                    // the other end
        uint64_t there;                    // pairs of links at the other end
        if (u == R.root && R.root_deg2) {
            if (!merged) continue;
            w = kids[u][0] == v ? kids[u][1] : kids[u][0];
            there = pairs_of_links(w, none, false);
            if (v == kids[u][1]) { par[R.inner_id[v]] = R.inner_id[w]; c->branch_dup_from = R.inner_id[v]; c->branch_dup_to = w; }
        } else {
            there = pairs_of_links(u, v, true);
            par[R.inner_id[v]] = R.inner_id[u];
        }
        const uint32_t iv = R.inner_id[v], iw = R.inner_id[w];
        edge_key[v] = std::min(iv, iw) * NI + std::max(iv, iw);
        c->branch_quartets[v] = pairs_of_links(v, none, false) * there;
    }
    DevBuf<uint16_t> next; DevBuf<uint32_t> words; DevBuf<unsigned long long> quartets;
    QS_HIP(c, next.reserve(c->branch_next.size() * 2, nullptr));
    QS_HIP(c, words.reserve(c->branch_words.size() * 4, nullptr));
    QS_HIP(c, quartets.reserve(c->branch_quartets.size() * 8, nullptr));
    QS_HIP(c, hipMemcpyAsync(next.get(), c->branch_next.data(), c->branch_next.size() * 2, hipMemcpyHostToDevice, c->stream));
    QS_HIP(c, hipMemcpyAsync(words.get(), c->branch_words.data(), c->branch_words.size() * 4, hipMemcpyHostToDevice, c->stream));
    QS_HIP(c, hipMemcpyAsync(quartets.get(), c->branch_quartets.data(), c->branch_quartets.size() * 8, hipMemcpyHostToDevice, c->stream));
    c->branch_next_dev = std::move(next); c->branch_words_dev = std::move(words); c->branch_quartets_dev = std::move(quartets);
    return QS_OK;
}

// The four words (4-sets, F1, F2, F3) of every internode of the reference tree over the 4-sets around it that hold a listed taxon
// (qs_branch_taxa.hip), and over all 4-sets around it (the adjacent node pairs of one score pass 1 over the context's own table). The
// reference never asks what a branch's support would be without one taxon: this replaces nothing there.
extern "C" int qs_branch_taxon_support(qs_ctx *c, const qs_ref_tree *ref, const uint16_t *taxa, uint32_t n_list, int64_t *rows_device,
                                       int64_t *totals_device) {
    if (!c) return QS_ERR_ARG;
    const char *who = "qs_branch_taxon_support";
    if (int rc = need_args(c, who, rows_device)) return rc;
    for (const void *p : {(const void *)rows_device, (const void *)totals_device})
        if (int rc = need_aligned(c, who, p, "rows_device / totals_device")) return rc;
    if (int rc = need_table(c, who)) return rc;
    const uint64_t max_count = table_max_count(c);
    if (int rc = need_taxon_sums_fit(c, who, max_count)) return rc;   // (the bound of qs_taxon_support for a row; the totals are the score's sums)
    if (int rc = need_whole_table(c, who, "taxon")) return rc;
    std::vector<uint16_t> list;
    if (int rc = check_taxon_list(c, who, taxa, n_list, list)) return rc;
    QS_HIP(c, hipSetDevice(c->device));
    const RefHost *Rp = nullptr;
    if (int rc = get_ref(c, ref, true, &Rp)) return rc;
    if (branch_taxa_lds_bytes(Rp->n_inner) > 160u * 1024u)
        return fail(c, QS_ERR_UNSUPPORTED, "qs_branch_taxon_support: more than 4551 inner nodes (the sums of a workgroup live in LDS)");
    if (int rc = ensure_branch_ref(c, *Rp)) return rc;
    if (int rc = ensure_n_cu(c)) return rc;
    if (int rc = ensure_place_walks(c, list)) return rc;
    const uint32_t NI = Rp->n_inner, N = Rp->n_nodes;
    BranchDevice bd;
    bd.g = gather_device(c);
    bd.par = c->branch_words_dev.get(); bd.inner_node = bd.par + NI; bd.next = c->branch_next_dev.get();
    bd.n_nodes = N; bd.n_inner = NI;
    bd.dup_from = c->branch_dup_from; bd.dup_to = c->branch_dup_to;
    bd.frame = Rp->bifurcating ? 0 : 1;   // (fill_score_device: the order of (q1,q2,q3) qs_score uses without flags)
    QS_HIP(c, hipMemsetAsync(rows_device, 0, (size_t)n_list * N * kBranchWords * 8, c->stream));
    const bool wide = max_count >= (1ull << 32) / 4096 || c->n > 4096;   // the rule of qs_taxon_placement
    QS_HIP(c, launch_branch_taxa(c->stream, bd, n_list, wide, c->n_cu, reinterpret_cast<unsigned long long *>(rows_device)));
    if (totals_device) {
        // one streaming read: the exact 64-bit sums per node pair of a plain pass 1 (no candidate log, no view, no sums of the pairs
        // (degree-2 root, v)) into a buffer of this call's own; the adjacent pairs are the internodes
        const size_t np = (size_t)NI * NI;
        QS_HIP(c, c->branch_sums.reserve(np * 4 * 8, &c->stream));
        unsigned long long *sums = c->branch_sums.get();
        QS_HIP(c, hipMemsetAsync(sums, 0, np * 3 * 8, c->stream));
        QS_HIP(c, hipMemsetAsync(sums + np * 3, 0x7F, np * 8, c->stream));
        if (int rc = ensure_score_tables(c)) return rc;
        ScoreDevice sd;
        fill_score_device(c, *Rp, c->ref_lca_dev.get(), sd);
        sd.rank_lo = c->rank_lo; sd.n_tuples = c->n_tuples; sd.table = c->table; sd.count_bits = (int)c->count_bits;
        sd.pair_sums = sums; sd.pair_min = reinterpret_cast<long long *>(sums + np * 3);
        if (int rc = ensure_bundle_plan(c, sd, 1)) return rc;
        QS_HIP(c, launch_score_pass1(c->stream, sd, c->tune_score_kernel, c->n_cu, c->bundle[0].part_lo, c->bundle[0].part_n, c->bundle[0].n_parts, c->tune_score_tol));
        QS_HIP(c, launch_branch_totals(c->stream, sums, bd.inner_node + NI, c->branch_quartets_dev.get(), N, reinterpret_cast<unsigned long long *>(totals_device)));
    }
    return QS_OK;   // asynchronous on the context's stream
}

// Link sums of the quartet placement of the listed clades (qs_place_clade.hip): the clade below a node is pruned and regrafted, unchanged
// inside, on every edge outside it. The reference never asks where the evaluation trees would put a subtree: this replaces nothing there.
extern "C" int qs_clade_placement(qs_ctx *c, const qs_ref_tree *ref, const uint32_t *nodes, uint32_t n_list, int64_t *dst_device) {
    if (!c) return QS_ERR_ARG;
    const char *who = "qs_clade_placement";
    if (int rc = need_args(c, who, dst_device)) return rc;
    if (int rc = need_aligned(c, who, dst_device)) return rc;
    if (int rc = need_table(c, who)) return rc;
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
    const uint64_t max_count = table_max_count(c);
    std::vector<uint64_t> cost(n_list);
    for (uint32_t i = 0; i < n_list; ++i) {
        const uint64_t s = hi[i] - lo[i], o = n - s;
        cost[i] = s * (o * (o - 1) / 2 * (o - 2) / 3);        // (n <= 65535: below 2^62)
        if (max_count > (uint64_t)INT64_MAX / cost[i])
            return fail(c, QS_ERR_OVERFLOW, "qs_clade_placement: |C| x C(n-|C|,3) x the largest possible count exceeds 63 bits for node " + std::to_string(nodes[i]));
    }
    if (int rc = need_whole_table(c, who, "clade")) return rc;
    if (place_lds_bytes(ref->n_nodes) > 160u * 1024u)
        return fail(c, QS_ERR_UNSUPPORTED, "qs_clade_placement: more than 10240 nodes (the link sums of a workgroup live in LDS)");
    QS_HIP(c, hipSetDevice(c->device));
    const RefHost *Rp = nullptr;
    if (int rc = get_ref(c, ref, true, &Rp)) return rc;
    if (int rc = ensure_place_ref(c, *Rp)) return rc;
    if (int rc = ensure_n_cu(c)) return rc;
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

// Per-tree quartet agreement of a batch with the reference tree (qs_agree.hip). The reference's links come from its depth-first id
// order: the children of an inner node split its id interval, ordered by their first id, and its parent link holds the other ids.
// The reference has no per-tree output: this replaces nothing there.
static int agree_ref_upload(qs_ctx *c, const qs_ref_tree *ref, const char *who = "qs_tree_agreement") {
    if (!ref || !ref->parent || !ref->leaf_node) return fail(c, QS_ERR_ARG, std::string(who) + ": NULL reference arrays");
    if (ref->n_taxa != c->n) return fail(c, QS_ERR_ARG, std::string(who) + ": the reference tree's n_taxa differs from the context");
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

// Host-only: the LDS plan of qs_tree_taxon_agreement for n_taxa (qs_tree_taxa.hip tree_taxa_plan) and the largest n_taxa it supports.
extern "C" int qs_tree_taxa_plan(uint32_t n_taxa, uint32_t out[7]) {
    if (!out) return fail(nullptr, QS_ERR_ARG, "qs_tree_taxa_plan: NULL argument");
    TreeTaxaPlan p;
    const bool ok = tree_taxa_plan(n_taxa, p);
    const uint32_t words[7] = {p.W, p.cap, p.nb, p.flight, p.diff_bytes, p.lds_bytes, tree_taxa_max_taxa()};
    std::copy(words, words + 7, out);
    return ok ? QS_OK : fail(nullptr, QS_ERR_UNSUPPORTED, "qs_tree_taxa_plan: more than " + std::to_string(tree_taxa_max_taxa()) + " taxa");
}

// Per tree of a batch and per taxon the tree holds the quartet agreement with the reference tree over the 4-sets that hold the taxon
// (qs_tree_taxa.hip). The reference's nodes are qs_tree_agreement's upload, cached per context. The reference has no output per tree
// and none per taxon: this replaces nothing there.
extern "C" int qs_tree_taxon_agreement(qs_ctx *c, const qs_ref_tree *ref, const qs_device_batch *b, int64_t *dst_device) {
    if (!c) return QS_ERR_ARG;
    const char *who = "qs_tree_taxon_agreement";
    if (int rc = need_args(c, who, b && dst_device)) return rc;
    if (c->d_lo != 0 || c->d_hi != c->n)
        return fail(c, QS_ERR_UNSUPPORTED, "qs_tree_taxon_agreement: whole-table contexts only (no table shards)");
    if (int rc = need_aligned(c, who, dst_device)) return rc;
    TreeTaxaPlan plan;
    if (!tree_taxa_plan(c->n, plan))
        return fail(c, QS_ERR_UNSUPPORTED, "qs_tree_taxon_agreement: more than " + std::to_string(tree_taxa_max_taxa()) +
                                               " taxa (the difference arrays of a workgroup live in LDS beside its bitmaps)");
    if (int rc = agree_ref_upload(c, ref, who)) return rc;
    const DeviceBatch &d = b->d;
    if (d.n_trees && !d.node_off) return fail(c, QS_ERR_STATE, "qs_tree_taxon_agreement: the batch was uploaded without node ranges");
    QS_HIP(c, hipSetDevice(c->device));
    if (d.ready) QS_HIP(c, hipStreamWaitEvent(c->stream, d.ready, 0));
    QS_HIP(c, launch_tree_taxa(c->stream, d, c->n, d.max_tree_nodes, c->agree_off.get(), c->agree_bnd.get(), c->agree_par.get(), c->agree_n_u,
                               reinterpret_cast<unsigned long long *>(dst_device)));
    return QS_OK;   // asynchronous on the context's stream
}

// Quartet agreement of the trees of one batch with those of another, or of a batch with itself (qs_agree_pairs.hip). The reference never
// compares the evaluation trees with each other: this replaces nothing there.
extern "C" int qs_tree_pair_agreement(qs_ctx *c, const qs_device_batch *rows, uint32_t r0, uint32_t r1, const qs_device_batch *cols,
                                      uint32_t c0, uint32_t c1, uint32_t flags, uint64_t *dst_device) {
    if (!c) return QS_ERR_ARG;
    if (!rows || !cols || !dst_device) return fail(c, QS_ERR_ARG, "qs_tree_pair_agreement: NULL argument");
    if (c->d_lo != 0 || c->d_hi != c->n)
        return fail(c, QS_ERR_UNSUPPORTED, "qs_tree_pair_agreement: whole-table contexts only (no table shards)");
    if (reinterpret_cast<uintptr_t>(dst_device) % 8) return fail(c, QS_ERR_ARG, "qs_tree_pair_agreement: dst_device is not 8-byte aligned");
    if (flags & ~QS_PAIRS_UPPER) return fail(c, QS_ERR_ARG, "qs_tree_pair_agreement: unknown flag");
    if ((flags & QS_PAIRS_UPPER) && rows != cols) return fail(c, QS_ERR_ARG, "qs_tree_pair_agreement: QS_PAIRS_UPPER needs rows and cols to be the same batch");
    const DeviceBatch &dr = rows->d, &dc = cols->d;
    if (r0 > r1 || r1 > dr.n_trees) return fail(c, QS_ERR_ARG, "qs_tree_pair_agreement: the row range is not within the batch");
    if (c0 > c1 || c1 > dc.n_trees) return fail(c, QS_ERR_ARG, "qs_tree_pair_agreement: the column range is not within the batch");
    if ((dr.n_trees && !dr.node_off) || (dc.n_trees && !dc.node_off))
        return fail(c, QS_ERR_STATE, "qs_tree_pair_agreement: a batch was uploaded without node ranges");
    const uint64_t n_pairs = (uint64_t)(r1 - r0) * (c1 - c0);
    if (n_pairs > (1ull << 28)) return fail(c, QS_ERR_ARG, "qs_tree_pair_agreement: more than 2^28 pairs in one call");
    if (n_pairs == 0) return QS_OK;
    QS_HIP(c, hipSetDevice(c->device));
    QS_HIP(c, c->pair_pos.reserve(tree_pairs_work_words(dr, r1 - r0, c->n) * sizeof(uint16_t), &c->stream));
    if (dr.ready) QS_HIP(c, hipStreamWaitEvent(c->stream, dr.ready, 0));
    if (dc.ready && rows != cols) QS_HIP(c, hipStreamWaitEvent(c->stream, dc.ready, 0));
    QS_HIP(c, launch_tree_pairs(c->stream, dr, r0, r1, dc, c0, c1, (flags & QS_PAIRS_UPPER) != 0, c->n, c->pair_pos.get(),
                                reinterpret_cast<unsigned long long *>(dst_device)));
    return QS_OK;   // asynchronous on the context's stream
}

// Per tree of a batch the quartet support of every internode of the reference tree (qs_tree_branch.hip). The internodes are
// qs_branch_taxon_support's: both ends inner nodes, the edge through a degree-2 root once, standing at both its inner children. The
// reference sums over the trees before it looks at a branch: this replaces nothing there.
static int tree_branch_ref_upload(qs_ctx *c, const qs_ref_tree *ref) {
    if (!ref || !ref->parent || !ref->leaf_node) return fail(c, QS_ERR_ARG, "qs_tree_branch_support: NULL reference arrays");
    if (ref->n_taxa != c->n) return fail(c, QS_ERR_ARG, "qs_tree_branch_support: the reference tree's n_taxa differs from the context");
    const uint32_t N = ref->n_nodes, n = ref->n_taxa, none = 0xFFFFFFFFu;
    if (c->tbranch_edges && c->tbranch_parent.size() == N && c->tbranch_leaf_node.size() == n &&
        memcmp(c->tbranch_parent.data(), ref->parent, (size_t)N * 4) == 0 && memcmp(c->tbranch_leaf_node.data(), ref->leaf_node, (size_t)n * 4) == 0)
        return QS_OK;
    RefHost R;
    if (int rc = build_ref_shape(c, ref, R)) return rc;
    std::vector<std::vector<uint32_t>> kids(N);
    for (uint32_t v = 0; v < N; ++v)
        if (R.parent[v] >= 0) kids[(uint32_t)R.parent[v]].push_back(v);
    std::vector<uint32_t> boff(N, 0), edges;
    std::vector<uint16_t> bnd;
    for (uint32_t v = 0; v < N; ++v) {
        if (kids[v].empty()) continue;
        std::sort(kids[v].begin(), kids[v].end(), [&](uint32_t x, uint32_t y) { return R.leaf_lo[x] < R.leaf_lo[y]; });
        boff[v] = (uint32_t)bnd.size();
        for (uint32_t k : kids[v]) bnd.push_back((uint16_t)R.leaf_lo[k]);
        bnd.push_back((uint16_t)(R.leaf_lo[v] + R.leaf_cnt[v]));
    }
    const bool root_deg2 = R.nchild[R.root] == 2;
    const bool merged = root_deg2 && R.nchild[kids[R.root][0]] > 0 && R.nchild[kids[R.root][1]] > 0;
    for (uint32_t v = 0; v < N; ++v) {
        if (R.nchild[v] == 0 || R.parent[v] < 0) continue;
        const uint32_t u = (uint32_t)R.parent[v];
        uint32_t w = u, dup = none, iv = none, par = R.parent[u] >= 0 ? 1u : 0u;
        if (u == R.root && root_deg2) {
            if (!merged || v != kids[u][0]) continue;   // the edge through the root: one record, written to both children
            w = dup = kids[u][1]; par = 0;
        } else {
            iv = (uint32_t)(std::find(kids[u].begin(), kids[u].end(), v) - kids[u].begin());
        }
        const uint32_t rec[kTreeBranchEdgeWords] = {v, dup, boff[v], R.nchild[v], boff[w], R.nchild[w], iv, par};
        edges.insert(edges.end(), rec, rec + kTreeBranchEdgeWords);
    }
    QS_HIP(c, hipSetDevice(c->device));
    QS_HIP(c, hipStreamSynchronize(c->stream));   // kernels of this context may still read the previous tree's arrays
    // (the cache key goes before the first buffer, as in agree_ref_upload)
    c->tbranch_parent.clear(); c->tbranch_leaf_node.clear();
    c->tbranch_edges.reset(); c->tbranch_bnd.reset();
    QS_HIP(c, c->tbranch_edges.reserve(std::max<size_t>(edges.size(), 1) * 4, nullptr));
    QS_HIP(c, c->tbranch_bnd.reserve(std::max<size_t>(bnd.size(), 1) * 2, nullptr));
    if (!edges.empty()) QS_HIP(c, hipMemcpy(c->tbranch_edges.get(), edges.data(), edges.size() * 4, hipMemcpyHostToDevice));
    if (!bnd.empty()) QS_HIP(c, hipMemcpy(c->tbranch_bnd.get(), bnd.data(), bnd.size() * 2, hipMemcpyHostToDevice));
    c->tbranch_n_e = (uint32_t)(edges.size() / kTreeBranchEdgeWords);
    c->tbranch_n_nodes = N;
    c->tbranch_frame = R.bifurcating ? 0 : 1;   // (fill_score_device: the order of (q1,q2,q3) qs_score uses without flags)
    c->tbranch_parent.assign(ref->parent, ref->parent + N);
    c->tbranch_leaf_node.assign(ref->leaf_node, ref->leaf_node + n);
    return QS_OK;
}

extern "C" int qs_tree_branch_support(qs_ctx *c, const qs_ref_tree *ref, const qs_device_batch *b, int64_t *dst_device) {
    if (!c) return QS_ERR_ARG;
    const char *who = "qs_tree_branch_support";
    if (int rc = need_args(c, who, b && dst_device)) return rc;
    if (c->d_lo != 0 || c->d_hi != c->n)
        return fail(c, QS_ERR_UNSUPPORTED, "qs_tree_branch_support: whole-table contexts only (no table shards)");
    if (int rc = need_aligned(c, who, dst_device)) return rc;
    if (int rc = tree_branch_ref_upload(c, ref)) return rc;
    const DeviceBatch &d = b->d;
    if (d.n_trees && !d.node_off) return fail(c, QS_ERR_STATE, "qs_tree_branch_support: the batch was uploaded without node ranges");
    QS_HIP(c, hipSetDevice(c->device));
    if (d.ready) QS_HIP(c, hipStreamWaitEvent(c->stream, d.ready, 0));
    QS_HIP(c, launch_tree_branch(c->stream, d, c->n, d.max_tree_nodes, c->tbranch_edges.get(), c->tbranch_bnd.get(), c->tbranch_n_e,
                                 c->tbranch_n_nodes, c->tbranch_frame, reinterpret_cast<unsigned long long *>(dst_device)));
    return QS_OK;   // asynchronous on the context's stream
}

// Weighted sums over the trees of the rows of qs_tree_branch_support, one per replicate of a bootstrap over the trees; dst is ADDED to.
extern "C" int qs_branch_resample(qs_ctx *c, const int64_t *rows_device, uint32_t n_trees, uint32_t n_nodes, const uint32_t *weights_host,
                                  uint32_t n_rep, int64_t *dst_device) {
    if (!c) return QS_ERR_ARG;
    const char *who = "qs_branch_resample";
    if (int rc = need_args(c, who, rows_device && weights_host && dst_device)) return rc;
    if (int rc = need_aligned(c, who, dst_device)) return rc;
    if (int rc = need_aligned(c, who, rows_device, "rows_device")) return rc;
    if ((uint64_t)n_nodes * kBranchWords > 0xFFFFFFFFull) return fail(c, QS_ERR_ARG, "qs_branch_resample: n_nodes x 4 must fit 32 bits");
    // a word of a row is at most C(n,4): every replicate's sum stays below 2^63 if (sum of its weights) x C(n,4) does
    const uint64_t n = c->n, quads = n >= 4 ? n * (n - 1) / 2 * (n - 2) / 3 * (n - 3) / 4 : 0;
    for (uint32_t r = 0; r < n_rep; ++r) {
        uint64_t s = 0;
        for (uint32_t t = 0; t < n_trees; ++t) s += weights_host[(size_t)r * n_trees + t];
        if (quads && s > (uint64_t)INT64_MAX / quads)
            return fail(c, QS_ERR_OVERFLOW, "qs_branch_resample: (sum of the weights) x C(n,4) exceeds 63 bits for replicate " + std::to_string(r));
    }
    if (n_trees == 0 || n_rep == 0 || n_nodes == 0) return QS_OK;
    QS_HIP(c, hipSetDevice(c->device));
    QS_HIP(c, hipStreamSynchronize(c->stream));   // (an earlier call's upload may still read the old weights)
    c->resample_weights.assign(weights_host, weights_host + (size_t)n_rep * n_trees);
    QS_HIP(c, c->resample_weights_dev.reserve(c->resample_weights.size() * 4, nullptr));
    QS_HIP(c, hipMemcpyAsync(c->resample_weights_dev.get(), c->resample_weights.data(), c->resample_weights.size() * 4, hipMemcpyHostToDevice, c->stream));
    QS_HIP(c, launch_branch_resample(c->stream, reinterpret_cast<const long long *>(rows_device), n_trees, n_nodes * kBranchWords,
                                     c->resample_weights_dev.get(), n_rep, reinterpret_cast<unsigned long long *>(dst_device)));
    return QS_OK;   // asynchronous on the context's stream
}

// Per node the number of trees that resolve a 4-set around its internode and the sums of their normalised frequencies in 2^-40 units
// (the inputs of the local posterior); dst is ADDED to.
extern "C" int qs_branch_frequencies(qs_ctx *c, const int64_t *rows_device, uint32_t n_trees, uint32_t n_nodes, int64_t *dst_device) {
    if (!c) return QS_ERR_ARG;
    const char *who = "qs_branch_frequencies";
    if (int rc = need_args(c, who, rows_device && dst_device)) return rc;
    if (int rc = need_aligned(c, who, dst_device)) return rc;
    if (int rc = need_aligned(c, who, rows_device, "rows_device")) return rc;
    if (n_nodes > (1u << 21)) return fail(c, QS_ERR_ARG, "qs_branch_frequencies: more than 2^21 nodes (a tree of 4096 taxa has fewer than 2^13)");
    // a tree adds at most 2^40 to a sum: below 2^23 trees per call and in all, every sum stays below 2^63
    if (n_trees >= (1u << 23)) return fail(c, QS_ERR_OVERFLOW, "qs_branch_frequencies: 2^23 trees or more (the sums of 2^40-scaled frequencies could leave 63 bits)");
    if (n_trees == 0 || n_nodes == 0) return QS_OK;
    QS_HIP(c, hipSetDevice(c->device));
    QS_HIP(c, launch_branch_frequencies(c->stream, reinterpret_cast<const long long *>(rows_device), n_trees, n_nodes,
                                        reinterpret_cast<unsigned long long *>(dst_device)));
    return QS_OK;   // asynchronous on the context's stream
}
