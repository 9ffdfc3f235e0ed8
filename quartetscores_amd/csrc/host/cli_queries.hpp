// cli_queries.hpp -- the device side of the CLI's outputs beyond the annotated tree: the one helper through which every output gets
// its words from the count table (table_query), the writers above it, the three hook structs that work behind every batch's count
// (PerTree, TreeBranches, TreeTaxa) and the rescoring of further trees from the same table (--also-ref, --without-taxa). The lines themselves
// come from cli_reports.hpp.
#pragma once

#include "cli_args.hpp"
#include "cli_reports.hpp"
#include "synth.hpp"

#include <chrono>
#include <memory>

namespace qsh {

void write_annotated(const Tree &tree, const std::string &path, const EdgeScores &sc);   // (QuartetScores.cpp)

// `words` 64-bit words of device memory for the output `flag`, and their way back to the host
template <typename T>
void reserve_words(const std::string &flag, int device, qs::DevBuf<T> &buf, size_t words) {
    if (hipSetDevice(device) != hipSuccess || buf.reserve(words * 8, nullptr) != hipSuccess) throw std::runtime_error(flag + ": Insufficient memory!");
}
template <typename T>
void download_words(const std::string &flag, T *dst, const T *src, size_t words) {
    if (words && hipMemcpy(dst, src, words * 8, hipMemcpyDeviceToHost) != hipSuccess) throw std::runtime_error(flag + ": download failed");
}

// One query of the counted (or loaded) table for the output `flag`: `words` words allocated, launch(dst) behind the context's
// stream, one qs_sync, one download
template <typename Launch>
std::vector<int64_t> table_query(qs_ctx *ctx, int device, const std::string &flag, size_t words, Launch launch) {
    qs::DevBuf<int64_t> dev;
    reserve_words(flag, device, dev, words);
    if (launch(dev.get()) != QS_OK || qs_sync(ctx) != QS_OK) throw std::runtime_error(flag + ": " + qs_last_error(ctx));
    std::vector<int64_t> w(words);
    download_words(flag, w.data(), dev.get(), words);
    return w;
}

// --per-taxon: one qs_taxon_support, 6 words per taxon
inline void write_per_taxon(qs_ctx *ctx, const RefFlat &ref, const Args &a) {
    const qs_ref_tree rt = ref_view(ref);
    const std::vector<int64_t> w = table_query(ctx, a.dev.device, "--per-taxon", 6 * ref.names.size(), [&](int64_t *dst) { return qs_taxon_support(ctx, &rt, dst); });
    TsvFile f(a.per_taxon, kPerTaxonHeader);
    per_taxon_lines(f.f, ref, w.data());
    f.close();
}

// --place-taxa / --place-clades: one qs_taxon_placement / qs_clade_placement for the listed taxa / nodes, 2 x n_nodes link sums each,
// and per row qs_placement_scores in front of its line
template <typename Id, typename Launch, typename Line>
void write_placements(qs_ctx *ctx, const RefFlat &ref, int device, const std::string &flag, const std::string &path, const char *header,
                      const std::vector<Id> &ids, Launch launch, Line line) {
    const size_t N = ref.parent.size();
    const qs_ref_tree rt = ref_view(ref);
    const std::vector<int64_t> w = table_query(ctx, device, flag, ids.size() * 2 * N, [&](int64_t *dst) { return launch(&rt, ids.data(), (uint32_t)ids.size(), dst); });
    const RefShape S(ref);
    S.need_preorder(flag);
    TsvFile f(path, header);
    std::vector<int64_t> score(N);
    for (size_t k = 0; k < ids.size(); ++k) {
        if (qs_placement_scores(&rt, &w[k * 2 * N], score.data()) != QS_OK) throw std::runtime_error(flag + ": " + qs_last_error(nullptr));
        line(f.f, S, k, score.data());
    }
    f.close();
}
inline void write_place_taxa(qs_ctx *ctx, const RefFlat &ref, const Args &a) {
    write_placements(ctx, ref, a.dev.device, "--place-taxa", a.place_taxa, kPlaceTaxaHeader, a.place_ids,
                     [&](const qs_ref_tree *rt, const uint16_t *ids, uint32_t L, int64_t *dst) { return qs_taxon_placement(ctx, rt, ids, L, dst); },
                     [&](std::ostream &os, const RefShape &S, size_t k, const int64_t *score) { place_taxa_line(os, ref, S, a.place_ids[k], score); });
}
inline void write_place_clades(qs_ctx *ctx, const RefFlat &ref, const Args &a) {
    write_placements(ctx, ref, a.dev.device, "--place-clades", a.place_clades, kPlaceCladesHeader, a.place_nodes,
                     [&](const qs_ref_tree *rt, const uint32_t *nodes, uint32_t L, int64_t *dst) { return qs_clade_placement(ctx, rt, nodes, L, dst); },
                     [&](std::ostream &os, const RefShape &S, size_t k, const int64_t *score) { place_clades_line(os, ref, S, k, a.place_nodes[k], score); });
}

// --test-groups: one qs_group_support, 6 words per hypothesis
inline void write_test_groups(qs_ctx *ctx, const Args &a) {
    const size_t H = a.group_names.size();
    const std::vector<int64_t> w = table_query(ctx, a.dev.device, "--test-groups", 6 * H, [&](int64_t *dst) { return qs_group_support(ctx, a.group_labels.data(), (uint32_t)H, dst); });
    TsvFile f(a.test_groups, kTestGroupsHeader);
    test_groups_lines(f.f, a.group_names, a.group_kind.data(), w.data());
    f.close();
}

// --taxon-pairs: one qs_taxon_pair_support for the listed taxa, a row of n x 8 words each
inline void write_taxon_pairs(qs_ctx *ctx, const RefFlat &ref, const Args &a) {
    const std::vector<uint16_t> &ids = a.pair_ids;
    const qs_ref_tree rt = ref_view(ref);
    const std::vector<int64_t> w = table_query(ctx, a.dev.device, "--taxon-pairs", ids.size() * ref.names.size() * 8,
                                               [&](int64_t *dst) { return qs_taxon_pair_support(ctx, &rt, ids.data(), (uint32_t)ids.size(), dst); });
    TsvFile f(a.taxon_pairs, kTaxonPairsHeader);
    taxon_pairs_lines(f.f, ref, ids, w.data());
    f.close();
}

// --drop-one: one qs_branch_taxon_support for the listed taxa, a row of n_nodes x 4 words each and the totals behind them
inline void write_drop_one(qs_ctx *ctx, const RefFlat &ref, const Args &a) {
    const std::vector<uint16_t> &ids = a.drop_ids;
    const size_t rows = ids.size() * ref.parent.size() * 4;
    const qs_ref_tree rt = ref_view(ref);
    const std::vector<int64_t> w = table_query(ctx, a.dev.device, "--drop-one", rows + ref.parent.size() * 4,
                                               [&](int64_t *dst) { return qs_branch_taxon_support(ctx, &rt, ids.data(), (uint32_t)ids.size(), dst, dst + rows); });
    TsvFile f(a.drop_one, kDropOneHeader);
    drop_one_lines(f.f, ref, RefShape(ref), ids, w.data(), w.data() + rows);
    f.close();
}

// --per-tree: qs_tree_agreement behind every batch's count into one device buffer of 4 x m words, downloaded once after the last
// qs_sync; taxa per tree from the flattened batches
struct PerTree {
    const Args &a;
    size_t m;
    RefFlat ref;
    qs::DevBuf<uint64_t> dev;
    std::vector<uint64_t> counts;
    std::vector<uint32_t> taxa;
    PerTree(const Args &args, size_t trees, const Tree &referenceTree, DeviceOptions &opt) : a(args), m(trees), ref(flatten_reference(referenceTree)), taxa(trees, 0) {
        opt.per_tree = a.per_tree;
        add_after_count(opt, [this](qs_ctx *ctx, const qs_device_batch *db, size_t i0, const BatchFlat &b) {
            if (!dev) reserve_words("--per-tree", a.dev.device, dev, std::max<size_t>(1, 4 * m));
            for (uint32_t t = 0; t < b.n_trees; ++t) taxa[i0 + t] = b.leaf_off[t + 1] - b.leaf_off[t];
            const qs_ref_tree rt = ref_view(ref);
            if (qs_tree_agreement(ctx, &rt, db, dev.get() + 4 * i0) != QS_OK) throw std::runtime_error(qs_last_error(ctx));
        });
        add_after_sync(opt, [this](qs_ctx *) {
            counts.assign(4 * m, 0);
            download_words("--per-tree", counts.data(), dev.get(), 4 * m);
        });
    }
    void write() const {
        TsvFile f(a.per_tree, kPerTreeHeader);
        per_tree_lines(f.f, m, taxa.data(), counts.data());
        f.close();
    }
};

// --branch-trees / --bootstrap / --local-pp: qs_tree_branch_support behind every batch's count into one device buffer of (trees of the
// batch) x n_nodes x 4 words, shared by the three outputs. --branch-trees downloads every batch and writes its lines as it comes;
// --bootstrap adds the batch to the sums of every replicate with its slice of the replicates' weights (qs_branch_resample; row 0 of the
// weights is all ones: the unweighted sums behind the qpic column); --local-pp adds the batch's normalised frequencies to n_nodes x 4
// words (qs_branch_frequencies). Both sums are downloaded once behind the final qs_sync. No buffer grows with m on the device.
struct TreeBranches {
    const Args &a;
    size_t m;
    RefFlat ref;
    RefShape shape;
    qs::DevBuf<int64_t> rows, sums, freq;
    std::vector<uint32_t> weights, slice;   // [1 + reps][m]; the columns of one batch
    std::vector<int64_t> host, totals, freq_totals;
    TsvFile lines;
    static bool wanted(const Args &a) { return !a.branch_trees.empty() || !a.bootstrap.empty() || !a.local_pp.empty(); }
    // zeroed sums of an output, allocated with its first batch
    void zeroed(const char *flag, qs::DevBuf<int64_t> &buf, size_t words) const {
        if (buf) return;
        reserve_words(flag, a.dev.device, buf, std::max<size_t>(1, words));
        if (hipMemset(buf.get(), 0, words * 8) != hipSuccess || hipDeviceSynchronize() != hipSuccess) throw std::runtime_error(std::string(flag) + ": Insufficient memory!");
    }
    TreeBranches(const Args &args, size_t trees, const Tree &referenceTree, DeviceOptions &opt) : a(args), m(trees), ref(flatten_reference(referenceTree)), shape(ref) {
        opt.tree_branches = true;
        const size_t N = ref.parent.size(), reps = a.bootstrap_reps;
        if (!a.branch_trees.empty()) lines.open(a.branch_trees, kBranchTreesHeader);
        if (!a.bootstrap.empty()) {
            // replicate r draws m tree indices; its weights are their multiplicities
            weights.assign((1 + reps) * m, 0);
            std::fill(weights.begin(), weights.begin() + (std::ptrdiff_t)m, 1u);
            for (uint32_t r = 0; r < reps; ++r) {
                Rng rng(a.bootstrap_seed, r);
                for (size_t i = 0; i < m; ++i) weights[(size_t)(1 + r) * m + rng.below((uint32_t)m)]++;
            }
        }
        add_after_count(opt, [this, N, reps](qs_ctx *ctx, const qs_device_batch *db, size_t i0, const BatchFlat &b) {
            const size_t k = b.n_trees, words = k * N * 4;
            reserve_words("--branch-trees / --bootstrap / --local-pp", a.dev.device, rows, std::max<size_t>(1, words));
            const qs_ref_tree rt = ref_view(ref);
            if (qs_tree_branch_support(ctx, &rt, db, rows.get()) != QS_OK) throw std::runtime_error(qs_last_error(ctx));
            if (!a.bootstrap.empty()) {
                zeroed("--bootstrap", sums, (1 + reps) * N * 4);
                slice.resize((1 + reps) * k);
                for (size_t r = 0; r <= reps; ++r) std::copy_n(weights.begin() + (std::ptrdiff_t)(r * m + i0), k, slice.begin() + (std::ptrdiff_t)(r * k));
                if (qs_branch_resample(ctx, rows.get(), (uint32_t)k, (uint32_t)N, slice.data(), (uint32_t)(1 + reps), sums.get()) != QS_OK) throw std::runtime_error(qs_last_error(ctx));
            }
            if (!a.local_pp.empty()) {
                zeroed("--local-pp", freq, N * 4);
                if (qs_branch_frequencies(ctx, rows.get(), (uint32_t)k, (uint32_t)N, freq.get()) != QS_OK) throw std::runtime_error(qs_last_error(ctx));
            }
            if (a.branch_trees.empty()) return;   // (the next batch's rows come behind this one's sums on the context's stream)
            // the lines are written as the batch comes: the device is waited for here, which this output pays for and no other
            if (qs_sync(ctx) != QS_OK) throw std::runtime_error(qs_last_error(ctx));
            host.resize(words);
            download_words("--branch-trees", host.data(), rows.get(), words);
            branch_trees_lines(lines.f, shape, i0, k, host.data());
            lines.check();
        });
        add_after_sync(opt, [this, N, reps](qs_ctx *) {
            if (!a.local_pp.empty()) {
                freq_totals.assign(N * 4, 0);
                download_words("--local-pp", freq_totals.data(), freq.get(), freq ? freq_totals.size() : 0);
            }
            if (a.bootstrap.empty()) return;
            totals.assign((1 + reps) * N * 4, 0);
            download_words("--bootstrap", totals.data(), sums.get(), sums ? totals.size() : 0);
        });
    }
    void write() {
        if (!a.branch_trees.empty()) lines.close();
        if (!a.local_pp.empty()) {
            TsvFile f(a.local_pp, kLocalPpHeader);
            local_pp_lines(f.f, shape, a.local_pp_lambda, freq_totals.data());
            f.close();
        }
        if (a.bootstrap.empty()) return;
        TsvFile f(a.bootstrap, kBootstrapHeader);
        bootstrap_lines(f.f, shape, a.bootstrap_reps, totals.data());
        f.close();
    }
};

// --tree-taxa: qs_tree_taxon_agreement behind every batch's count into one device buffer of (trees of the batch) x n x 4 words; every
// batch is waited for and downloaded and its lines are written as it comes, which this output pays for and no other: no buffer grows
// with m, on the device or on the host
struct TreeTaxa {
    const Args &a;
    RefFlat ref;
    qs::DevBuf<int64_t> rows;
    std::vector<int64_t> host;
    std::vector<uint8_t> keep;
    TsvFile lines;
    TreeTaxa(const Args &args, const Tree &referenceTree, DeviceOptions &opt) : a(args), ref(flatten_reference(referenceTree)), keep(ref.names.size(), 0) {
        opt.tree_branches = true;   // (the batches carry their node ranges)
        for (uint16_t x : a.tree_taxa_ids) keep[x] = 1;
        lines.open(a.tree_taxa, kTreeTaxaHeader);
        add_after_count(opt, [this](qs_ctx *ctx, const qs_device_batch *db, size_t i0, const BatchFlat &b) {
            const size_t k = b.n_trees, words = k * ref.names.size() * 4;
            reserve_words("--tree-taxa", a.dev.device, rows, std::max<size_t>(1, words));
            const qs_ref_tree rt = ref_view(ref);
            if (qs_tree_taxon_agreement(ctx, &rt, db, rows.get()) != QS_OK || qs_sync(ctx) != QS_OK) throw std::runtime_error(std::string("--tree-taxa: ") + qs_last_error(ctx));
            host.resize(words);
            download_words("--tree-taxa", host.data(), rows.get(), words);
            tree_taxa_lines(lines.f, ref, i0, k, b.leaf_off.data(), b.leaf_ids.data(), host.data(), keep, a.tree_taxa_min_gain_given ? &a.tree_taxa_min_gain : nullptr);
            lines.check();
        });
    }
    void write() { lines.close(); }
};

// --also-ref / --without-taxa, after the primary tree's output is written: one further tree scored from the same count table. The
// two differ in how the table reaches `ctx` (prepare: re-indexed, or cut down to the kept taxa) and share what is said and written.
struct Rescoring {
    const Args &a;
    const Tree &tree;
    RefFlat flat;
    std::vector<uint16_t> src_id_of;   // the tree's lookup ids in the numbering of the -r tree
    std::chrono::steady_clock::time_point begin = std::chrono::steady_clock::now();
    Rescoring(const Args &args, const Tree &t, const RefFlat &primary, const std::string &intro) : a(args), tree(t) {
        std::cout << intro << " from the same count table.\n";
        flat = flatten_reference(tree);
        src_id_of.resize(flat.names.size());
        for (size_t i = 0; i < flat.names.size(); ++i) src_id_of[i] = (uint16_t)primary.name_to_id.at(flat.names[i]);
    }
    static long long us_since(std::chrono::steady_clock::time_point t) {
        return std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t).count();
    }
    // `did` ("Remapped") the table through `call` since `since`; then the scores of the tree from `ctx` and its annotated file
    void finish(qs_ctx *ctx, const char *did, const char *call, const std::string &label, std::chrono::steady_clock::time_point since, const std::string &out) const {
        const long long step_us = us_since(since);
        std::cout << did << " the count table in " << step_us << " microseconds.\n";
        if (a.dev.trace) std::fprintf(stderr, "[trace] %s for %s: %.2f ms\n", call, label.c_str(), step_us / 1000.0);
        const EdgeScores sc = score_table(ctx, ref_view(flat), score_flags(a.dev));
        std::cout << (sc.bifurcating ? "The reference tree is bifurcating.\n" : "The reference tree is multifurcating.\n");
        write_annotated(tree, out, sc);
        std::cout << "Finished computing scores.\n";
        std::cout << "It took: " << us_since(begin) << " microseconds." << std::endl;
    }
};

// --also-ref: the table of -r re-indexed into `table`'s context (allocated before the counting) per further reference tree
inline void score_also_refs(const Args &a, qs_ctx *src, const RefFlat &primary, qs_ctx *table) {
    for (const AlsoRef &x : a.also) {
        const Rescoring r(a, x.tree, primary, "Scoring the reference tree " + x.ref);
        if (qs_table_remap(table, src, r.src_id_of.data()) != QS_OK || qs_sync(table) != QS_OK) throw std::runtime_error(qs_last_error(table));
        r.finish(table, "Remapped", "qs_table_remap", x.ref, r.begin, x.out);
    }
}

// --without-taxa: per set a context of the kept taxa on `table` (allocated before the counting for the largest of them) and the count
// table cut down into it
inline void score_without_taxa(const Args &a, qs_ctx *src, const RefFlat &primary, uint32_t bits, const qs::DevBuf<char> &table) {
    for (const WithoutTaxa &x : a.without) {
        const Rescoring r(a, x.tree, primary, "Scoring the reference tree without " + std::to_string(x.drop.size()) + " taxa (" + x.names + ")");
        qs_ctx *ctx = nullptr;
        if (qs_create(&ctx, (uint32_t)r.flat.names.size(), bits, QS_FLAG_NONE, a.dev.device, nullptr, 0, 0) != QS_OK) throw std::runtime_error(qs_last_error(nullptr));
        struct Guard { qs_ctx *c; ~Guard() { qs_destroy(c); } } guard{ctx};   // (waits for the context's stream; the table stays the caller's)
        if (qs_table_attach(ctx, table.get(), table.bytes()) != QS_OK) throw std::runtime_error(qs_last_error(ctx));
        const auto attached = std::chrono::steady_clock::now();   // the restrict alone is timed, not the set-up in front of it
        if (qs_table_restrict(ctx, src, r.src_id_of.data()) != QS_OK || qs_sync(ctx) != QS_OK) throw std::runtime_error(qs_last_error(ctx));
        r.finish(ctx, "Restricted", "qs_table_restrict", x.names, attached, x.out);
    }
}

} // namespace qsh
