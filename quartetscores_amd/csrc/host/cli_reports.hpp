// cli_reports.hpp -- everything of the CLI's TSV outputs that needs no device: the shape of the -r tree (RefShape), the placement
// summary, the %.6f formatter, the file sink and the lines of every output from the 64-bit words the device gave. No HIP header is
// included, so that a sanitizer build can drive it alone (tools/asan_cli_reports.cpp); the calls that produce the words are in
// cli_queries.hpp.
#pragma once

#include "flatten.hpp"
#include "local_pp.hpp"
#include "quartet_math.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <fstream>
#include <ostream>
#include <set>
#include <stdexcept>
#include <string>
#include <vector>

namespace qsh {

// A figure as the files show it: %.6f, or nan / inf; a ratio is nan where its denominator is 0
struct Fixed6 {
    char text[64];
    explicit Fixed6(double v) {
        if (std::isnan(v)) std::snprintf(text, sizeof text, "nan");
        else if (std::isinf(v)) std::snprintf(text, sizeof text, "inf");   // (--local-pp's length where f1 reaches en + 2L - 1)
        else std::snprintf(text, sizeof text, "%.6f", v);
    }
    Fixed6(int64_t num, int64_t den) : Fixed6(den ? (double)num / (double)den : std::nan("")) {}
};
inline std::ostream &operator<<(std::ostream &os, const Fixed6 &f) { return os << f.text; }

// A TSV file: opened with its header, closed by close(); both say "cannot write PATH" where the stream fails
struct TsvFile {
    std::string path;
    std::ofstream f;
    TsvFile() = default;
    TsvFile(const std::string &p, const char *header) { open(p, header); }
    void open(const std::string &p, const char *header) {
        path = p;
        f.open(path);
        check();
        f << header;
    }
    void check() const { if (!f) throw std::runtime_error("cannot write " + path); }
    void close() { f.close(); check(); }
};

// The shape of a flattened reference tree that the outputs need: root, depth and links of every node, the lookup ids [lo, hi) below
// it, its children in id order, and the internodes as the per-branch outputs list them (tests/branch_taxon_model.py): the edges (child
// node v, other end w) in node order -- the internode through a degree-2 root once, at the child that holds lookup id 0
struct RefShape {
    struct Edge { size_t v, w; bool through_root; };
    size_t n = 0, root = 0;
    bool preorder = true;   // parents are numbered before their children
    std::vector<uint32_t> depth, links;
    std::vector<size_t> lo, hi;
    std::vector<std::vector<size_t>> kids;
    std::vector<Edge> edges;
    explicit RefShape(const RefFlat &ref) : n(ref.names.size()) {
        const size_t N = ref.parent.size();
        depth.assign(N, 0); links.assign(N, 0); lo.assign(N, n); hi.assign(N, 0); kids.resize(N);
        for (size_t v = 0; v < N; ++v) {
            const int32_t p = ref.parent[v];
            if (p < 0) { root = v; continue; }
            if ((size_t)p >= v) preorder = false;
            links[v] += 1; links[(size_t)p] += 1; kids[(size_t)p].push_back(v);
        }
        std::vector<size_t> order;   // parents first, whatever the numbering
        if (N) order.push_back(root);
        for (size_t k = 0; k < order.size(); ++k)
            for (size_t c : kids[order[k]]) { depth[c] = depth[order[k]] + 1; order.push_back(c); }
        for (size_t i = 0; i < n; ++i) { lo[ref.leaf_node[i]] = i; hi[ref.leaf_node[i]] = i + 1; }
        for (size_t k = order.size(); k-- > 1;) {
            const size_t v = order[k], p = (size_t)ref.parent[v];
            lo[p] = std::min(lo[p], lo[v]); hi[p] = std::max(hi[p], hi[v]);
        }
        for (auto &k : kids) std::sort(k.begin(), k.end(), [&](size_t x, size_t y) { return lo[x] < lo[y]; });
        for (size_t v = 0; v < N; ++v) {
            if (v == root || kids[v].empty()) continue;
            const size_t u = (size_t)ref.parent[v];
            if (u == root && kids[u].size() == 2) {
                const size_t o = kids[u][0] == v ? kids[u][1] : kids[u][0];
                if (!kids[o].empty() && v == kids[u][0]) edges.push_back({v, o, true});
            } else edges.push_back({v, u, false});
        }
    }
    size_t nodes() const { return lo.size(); }
    size_t below(size_t v) const { return hi[v] - lo[v]; }
    bool holds(size_t v, size_t x) const { return lo[v] <= x && x < hi[v]; }
    // the placement outputs walk the tree by node number
    void need_preorder(const std::string &flag) const {
        if (!preorder) throw std::runtime_error(flag + ": the reference tree is not numbered in preorder");
    }
};

// Where the evaluation trees would put the part of the -r tree below the node `moved` (a leaf: --place-taxa, an inner node:
// --place-clades), from the score of every edge as its position (qs_placement_scores; tests/placement_model.py and
// tests/clade_placement_model.py define the columns). edge[v] says whether the edge above v is a position at all; lookup ids at or
// above `from` count `by` less, which numbers the taxa that stay. A position = the edges that induce the same bipartition of those.
struct Placement {
    int64_t current, best;
    size_t n_best, node, distance;
};
inline Placement summarise_placement(const RefFlat &ref, const RefShape &S, size_t moved, const std::vector<uint8_t> &edge, size_t from, size_t by,
                                     const int64_t *score) {
    const size_t N = S.nodes();
    const int64_t n = (int64_t)S.n;
    // the position of the edge above v: the id interval, in the numbering of the taxa that stay, of the side without the smallest of them
    std::vector<int64_t> key(N);
    for (size_t v = 0; v < N; ++v) {
        int64_t a = (int64_t)(S.lo[v] - (S.lo[v] >= from ? by : 0)), b = (int64_t)(S.hi[v] - (S.hi[v] >= from ? by : 0));
        if (a == 0 && b > 0) { a = b; b = n - (int64_t)by; }
        key[v] = b > a ? a * n + b : 0;
    }
    const size_t u = (size_t)ref.parent[moved];
    if (S.links[u] == 3)   // the moved edge and the two other edges at its parent are one position
        for (size_t v = 0; v < N; ++v) if (v != moved && ref.parent[v] == (int32_t)u) { key[moved] = key[v]; break; }
    int64_t best = INT64_MIN;
    for (size_t v = 0; v < N; ++v) if (edge[v]) best = std::max(best, score[v]);
    std::set<int64_t> top;
    int64_t first_top = -1;
    for (size_t v = 0; v < N; ++v) if (edge[v] && score[v] == best) { if (top.empty()) first_top = key[v]; top.insert(key[v]); }
    const int64_t current = score[moved];
    const int64_t pick = current == best ? key[moved] : first_top;
    size_t node = 0;
    for (size_t v = 0; v < N; ++v) if (edge[v] && key[v] == pick) { node = v; break; }
    auto walk = [&](size_t a, size_t b) {   // nodes on the path from a to b, both inclusive
        std::vector<size_t> left{a}, right{b};
        while (left.back() != right.back()) {
            if (S.depth[left.back()] >= S.depth[right.back()]) left.push_back((size_t)ref.parent[left.back()]);
            else right.push_back((size_t)ref.parent[right.back()]);
        }
        left.insert(left.end(), right.rbegin() + 1, right.rend());
        return left;
    };
    size_t dist = 0;
    if (pick != key[moved]) {
        const std::vector<size_t> to_child = walk(u, node), to_parent = walk(u, (size_t)ref.parent[node]);
        for (size_t v : to_parent.size() < to_child.size() ? to_parent : to_child) dist += S.links[v] - (v == u) >= 3;
    }
    return {current, best, top.size(), node, dist};
}
inline std::ostream &operator<<(std::ostream &os, const Placement &p) {   // current best gain n_best best_node (best_lo best_hi follow)
    return os << p.current << '\t' << p.best << '\t' << (p.best - p.current) << '\t' << p.n_best << '\t' << p.node;
}

constexpr const char *kPlaceTaxaHeader = "taxon\tname\tcurrent\tbest\tgain\tn_best\tbest_node\tbest_lo\tbest_hi\tdistance\n";
// --place-taxa: the line of taxon x from the scores of its positions; every edge but the root's is one
inline void place_taxa_line(std::ostream &os, const RefFlat &ref, const RefShape &S, size_t x, const int64_t *score) {
    std::vector<uint8_t> edge(S.nodes(), 1);
    if (!edge.empty()) edge[S.root] = 0;
    const Placement p = summarise_placement(ref, S, ref.leaf_node[x], edge, x + 1, 1, score);
    os << x << '\t' << ref.names[x] << '\t' << p << '\t' << S.lo[p.node] << '\t' << S.hi[p.node] << '\t' << p.distance << '\n';
}

constexpr const char *kPlaceCladesHeader = "clade\tnode\tlo\thi\tsize\tcurrent\tbest\tgain\tn_best\tbest_node\tbest_lo\tbest_hi\tdistance\n";
// --place-clades: the line of the k-th listed clade, the subtree below node c; the edges outside the clade and its own are positions
inline void place_clades_line(std::ostream &os, const RefFlat &ref, const RefShape &S, size_t k, size_t c, const int64_t *score) {
    const size_t cl = S.lo[c], ch = S.hi[c];
    std::vector<uint8_t> edge(S.nodes());
    for (size_t v = 0; v < edge.size(); ++v) edge[v] = v != S.root && !(v != c && S.lo[v] >= cl && S.hi[v] <= ch);
    const Placement p = summarise_placement(ref, S, c, edge, ch, ch - cl, score);
    os << k << '\t' << c << '\t' << cl << '\t' << ch << '\t' << (ch - cl) << '\t' << p << '\t' << S.lo[p.node] << '\t' << S.hi[p.node] << '\t' << p.distance << '\n';
}

constexpr const char *kPerTreeHeader = "tree\ttaxa\tquartets\tconcordant\tdiscordant\teval_only\tref_only\tunresolved\tconcordance\n";
// --per-tree: one line per tree from its number of taxa and its four words (concordant, discordant, resolved in it, resolved in -r)
inline void per_tree_lines(std::ostream &os, size_t m, const uint32_t *taxa, const uint64_t *counts) {
    for (size_t t = 0; t < m; ++t) {
        const uint64_t n = taxa[t], c = counts[4 * t], d = counts[4 * t + 1], re = counts[4 * t + 2], rr = counts[4 * t + 3];
        const uint64_t q = c4(n), eo = re - c - d, ro = rr - c - d;
        os << t << '\t' << n << '\t' << q << '\t' << c << '\t' << d << '\t' << eo << '\t' << ro << '\t' << (q - c - d - eo - ro) << '\t'
           << Fixed6((int64_t)c, (int64_t)(c + d)) << '\n';
    }
}

constexpr const char *kPerTaxonHeader = "taxon\tname\tquartets\tref_resolved\tconcordant\tdiscordant\teval_only\toutvoted\tuninformed\tconcordance\tconcordance_without\n";
// --per-taxon: one line per taxon from its six words
inline void per_taxon_lines(std::ostream &os, const RefFlat &ref, const int64_t *w) {
    const size_t n = ref.names.size();
    int64_t conc = 0, disc = 0;   // of the whole table: every quartet is in four taxa's sums
    for (size_t x = 0; x < n; ++x) { conc += w[6 * x + 1]; disc += w[6 * x + 2]; }
    conc /= 4; disc /= 4;
    const uint64_t quartets = n < 4 ? 0 : (uint64_t)(n - 1) * (n - 2) * (n - 3) / 6;
    for (size_t x = 0; x < n; ++x) {
        const int64_t *v = &w[6 * x];
        os << x << '\t' << ref.names[x] << '\t' << quartets;
        for (int k = 0; k < 6; ++k) os << '\t' << v[k];
        os << '\t' << Fixed6(v[1], v[1] + v[2]) << '\t' << Fixed6(conc - v[1], conc - v[1] + disc - v[2]) << '\n';
    }
}

constexpr const char *kTaxonPairsHeader = "a\tb\tname_a\tname_b\tquartets\tref_together\tref_apart\ttogether\tapart\taffinity\tkept\tjoined\n";
// --taxon-pairs: one line per pair a < b with a listed taxon from the rows of n x 8 words of the listed taxa (tests/taxon_pair_model.py
// defines the columns; the matrix is symmetric: a pair's words come from the row of whichever of the two is listed)
inline void taxon_pairs_lines(std::ostream &os, const RefFlat &ref, const std::vector<uint16_t> &ids, const int64_t *w) {
    const size_t n = ref.names.size();
    std::vector<int64_t> row_of(n, -1);
    for (size_t k = 0; k < ids.size(); ++k) row_of[ids[k]] = (int64_t)k;
    const uint64_t quartets = n < 4 ? 0 : (uint64_t)(n - 2) * (n - 3) / 2;
    for (size_t a = 0; a < n; ++a)
        for (size_t b = a + 1; b < n; ++b) {
            if (row_of[a] < 0 && row_of[b] < 0) continue;
            const int64_t *v = row_of[a] >= 0 ? &w[((size_t)row_of[a] * n + b) * 8] : &w[((size_t)row_of[b] * n + a) * 8];
            os << a << '\t' << b << '\t' << ref.names[a] << '\t' << ref.names[b] << '\t' << quartets << '\t' << v[0] << '\t' << v[1] << '\t' << v[6] << '\t'
               << (v[7] - v[6]) << '\t' << Fixed6(v[6], v[7]) << '\t' << Fixed6(v[2], v[3]) << '\t' << Fixed6(v[4], v[5]) << '\n';
        }
}

constexpr const char *kDropOneHeader = "taxon\tname\tnode\tlo\thi\tgroup\tquartets\tq1\tq2\tq3\tqpic\tqpic_without\tdelta\n";
// --drop-one: one line per listed taxon and internode from the taxon's row of n_nodes x 4 words and the totals of the same layout
// (tests/branch_taxon_model.py defines the columns)
inline void drop_one_lines(std::ostream &os, const RefFlat &ref, const RefShape &S, const std::vector<uint16_t> &ids, const int64_t *w, const int64_t *totals) {
    const size_t N = S.nodes();
    // taxa in x's link at the node `end`, whose link towards `away` (N = none) is the edge itself
    auto link_size = [&](size_t end, size_t x, size_t away) {
        for (size_t k : S.kids[end])
            if (k != away && S.holds(k, x)) return S.below(k);
        return S.n - S.below(end);   // the parent's side
    };
    for (size_t k = 0; k < ids.size(); ++k) {
        const size_t x = ids[k];
        for (const RefShape::Edge &e : S.edges) {
            const int64_t *r = &w[(k * N + e.v) * 4], *t = totals + e.v * 4;
            const size_t group = S.holds(e.v, x) ? link_size(e.v, x, N) : e.through_root ? link_size(e.w, x, N) : link_size(e.w, x, e.v);
            const double full = raw_log_score((size_t)t[1], (size_t)t[2], (size_t)t[3]), none = std::nan("");
            const double rest = t[0] - r[0] > 0 ? raw_log_score((size_t)(t[1] - r[1]), (size_t)(t[2] - r[2]), (size_t)(t[3] - r[3])) : none;
            os << x << '\t' << ref.names[x] << '\t' << e.v << '\t' << S.lo[e.v] << '\t' << S.hi[e.v] << '\t' << group << '\t' << r[0] << '\t' << r[1] << '\t'
               << r[2] << '\t' << r[3] << '\t' << Fixed6(full) << '\t' << Fixed6(rest) << '\t' << Fixed6(rest - full) << '\n';
        }
    }
}

constexpr const char *kTestGroupsHeader = "name\tkind\tquartets\tq1\tq2\tq3\toutvoted\tuninformed\tsupport\tqpic\n";
// --test-groups: one line per hypothesis from its six words; kind 0 = quad, else split
inline void test_groups_lines(std::ostream &os, const std::vector<std::string> &names, const uint8_t *kind, const int64_t *w) {
    for (size_t h = 0; h < names.size(); ++h) {
        const int64_t *v = &w[6 * h];
        const bool split = kind[h] != 0;
        os << names[h] << '\t' << (split ? "split" : "quad");
        for (int k = 0; k < 6; ++k) os << '\t' << v[k];
        os << '\t' << Fixed6(v[1], v[1] + v[2] + v[3]) << '\t' << Fixed6(split ? std::nan("") : raw_log_score((size_t)v[1], (size_t)v[2], (size_t)v[3])) << '\n';
    }
}

constexpr const char *kBranchTreesHeader = "tree\tnode\tlo\thi\tpresent\tq1\tq2\tq3\tconcordance\n";
// --branch-trees: the lines of the k trees of a batch, the first of which is tree i0, from their k x n_nodes x 4 words; lines with
// present = 0 are left out
inline void branch_trees_lines(std::ostream &os, const RefShape &S, size_t i0, size_t k, const int64_t *words) {
    for (size_t t = 0; t < k; ++t)
        for (const RefShape::Edge &e : S.edges) {
            const int64_t *w = &words[(t * S.nodes() + e.v) * 4];
            if (w[0] == 0) continue;
            os << (i0 + t) << '\t' << e.v << '\t' << S.lo[e.v] << '\t' << S.hi[e.v] << '\t' << w[0] << '\t' << w[1] << '\t' << w[2] << '\t' << w[3] << '\t'
               << Fixed6(w[1], w[1] + w[2] + w[3]) << '\n';
        }
}

constexpr const char *kTreeTaxaHeader = "tree\ttaxon\tname\tquartets\tconcordant\tdiscordant\teval_only\tref_only\tunresolved\tconcordance\ttree_concordance\tconcordance_without\tgain\n";
// --tree-taxa: the lines of the k trees of a batch, the first of which is tree i0, from their leaf lists and their k x n x 4 words
// (concordant, discordant, resolved in the tree, resolved in -r, over the 4-sets of the tree that hold the taxon): per tree of at least
// four taxa one line per taxon it holds, in id order; keep[x] = 0 leaves taxon x out, min_gain (where given) the lines below it and
// those whose gain is nan
inline void tree_taxa_lines(std::ostream &os, const RefFlat &ref, size_t i0, size_t k, const uint32_t *leaf_off, const uint16_t *leaf_ids, const int64_t *words,
                            const std::vector<uint8_t> &keep, const double *min_gain) {
    const size_t n = ref.names.size();
    const auto ratio = [](int64_t num, int64_t den) { return den ? (double)num / (double)den : std::nan(""); };
    std::vector<uint16_t> ids;
    for (size_t t = 0; t < k; ++t) {
        ids.assign(leaf_ids + leaf_off[t], leaf_ids + leaf_off[t + 1]);
        const uint64_t L = ids.size();
        if (L < 4) continue;
        std::sort(ids.begin(), ids.end());
        const int64_t *w = &words[t * n * 4];
        int64_t conc = 0, disc = 0;   // of the whole tree: every 4-set is in four taxa's words
        for (uint16_t x : ids) { conc += w[4 * x]; disc += w[4 * x + 1]; }
        conc /= 4; disc /= 4;
        const double tree_conc = ratio(conc, conc + disc);
        const uint64_t quartets = (L - 1) * (L - 2) * (L - 3) / 6;
        for (uint16_t x : ids) {
            const int64_t c = w[4 * x], d = w[4 * x + 1], eo = w[4 * x + 2] - c - d, ro = w[4 * x + 3] - c - d;
            const double without = ratio(conc - c, conc - c + disc - d), gain = without - tree_conc;
            if (!keep[x] || (min_gain && !(gain >= *min_gain))) continue;
            os << (i0 + t) << '\t' << x << '\t' << ref.names[x] << '\t' << quartets << '\t' << c << '\t' << d << '\t' << eo << '\t' << ro << '\t'
               << ((int64_t)quartets - c - d - eo - ro) << '\t' << Fixed6(c, c + d) << '\t' << Fixed6(tree_conc) << '\t' << Fixed6(without) << '\t' << Fixed6(gain) << '\n';
        }
    }
}

constexpr const char *kBootstrapHeader = "node\tlo\thi\tqpic\tmean\tsd\tlo95\thi95\treps\n";
// --bootstrap: one line per internode from the sums [1 + B][n_nodes][4]: row 0 unweighted, rows 1 .. B the replicates (B >= 1)
inline void bootstrap_lines(std::ostream &os, const RefShape &S, size_t B, const int64_t *totals) {
    std::vector<double> vals(B);
    for (const RefShape::Edge &e : S.edges) {
        auto score = [&](size_t r) { const int64_t *w = &totals[(r * S.nodes() + e.v) * 4]; return raw_log_score((size_t)w[1], (size_t)w[2], (size_t)w[3]); };
        double total = 0.0, dev2 = 0.0;   // plain double sums in replicate order
        for (size_t r = 0; r < B; ++r) { vals[r] = score(1 + r); total += vals[r]; }
        const double mean = total / (double)B;
        for (size_t r = 0; r < B; ++r) dev2 += (vals[r] - mean) * (vals[r] - mean);
        std::sort(vals.begin(), vals.end());
        os << e.v << '\t' << S.lo[e.v] << '\t' << S.hi[e.v] << '\t' << Fixed6(score(0)) << '\t' << Fixed6(mean) << '\t' << Fixed6(std::sqrt(dev2 / (double)B)) << '\t'
           << Fixed6(vals[(size_t)std::floor(0.025 * (double)(B - 1))]) << '\t' << Fixed6(vals[(size_t)std::ceil(0.975 * (double)(B - 1))]) << '\t' << B << '\n';
    }
}

constexpr const char *kLocalPpHeader = "node\tlo\thi\ten\tf1\tf2\tf3\tpp1\tpp2\tpp3\tlength\tpolytomy_p\n";
// --local-pp: one line per internode from the four words of its node: integers as they are, f_i = Z_i / 2^40 and local_pp.hpp's five
inline void local_pp_lines(std::ostream &os, const RefShape &S, double lambda, const int64_t *freq) {
    for (const RefShape::Edge &e : S.edges) {
        const int64_t *w = &freq[e.v * 4];
        // (no 4-set lies around a branch that does not leave two of the tree's n taxa on either side: it is written as en = 0 is)
        const bool splits = S.n > 1 && S.below(e.v) >= 2 && S.n - S.below(e.v) >= 2;
        double cols[8] = {(double)w[1] / 1099511627776.0, (double)w[2] / 1099511627776.0, (double)w[3] / 1099511627776.0};
        local_pp(splits ? w[0] : 0, w + 1, lambda, cols + 3);
        os << e.v << '\t' << S.lo[e.v] << '\t' << S.hi[e.v] << '\t' << w[0];
        for (double c : cols) os << '\t' << Fixed6(c);
        os << '\n';
    }
}

} // namespace qsh
