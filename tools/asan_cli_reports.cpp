// sanitizer driver for the host side of the CLI's TSV outputs (cli_reports.hpp; AddressSanitizer + UBSan, CPU only): RefShape, the
// placement summary and the lines of every output from synthetic words, on the reference trees where the index arithmetic is at its
// limit, and a few lines worked out by hand. A wrong line aborts, and so does every sanitizer report (-fno-sanitize-recover=all).
//   make -C tools asan && tools/bin/asan_cli_reports
#include "cli_reports.hpp"
#include "flatten.hpp"
#include "newick.hpp"

#include <cstdlib>
#include <sstream>
using namespace qsh;

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); std::abort(); } } while (0)

static RefFlat flat(const std::string &newick) {
    Tree t;
    NewickReader rr(newick);
    CHECK(rr.next(t));
    return flatten_reference(t);
}

// every line of `text` has as many columns as `header`; returns the number of lines
static size_t columns_match(const char *header, const std::string &text) {
    const std::string h = header;
    const auto tabs = std::count(h.begin(), h.end(), '\t');
    CHECK(text.empty() || text.back() == '\n');
    std::istringstream in(text);
    size_t lines = 0;
    for (std::string line; std::getline(in, line); ++lines) CHECK(std::count(line.begin(), line.end(), '\t') == tabs && !line.empty() && line.back() != '\t');
    return lines;
}

static uint64_t mix(uint64_t x) { x ^= x >> 31; x *= 0x9E3779B97F4A7C15ull; x ^= x >> 29; return x; }

struct Expect { size_t internodes, through_root; };

static void drive(const std::string &newick, Expect want) {
    const RefFlat ref = flat(newick);
    const RefShape S(ref);
    const size_t n = ref.names.size(), N = S.nodes();
    CHECK(S.preorder && S.n == n && N == ref.parent.size() && S.lo[S.root] == 0 && S.hi[S.root] == n && S.depth[S.root] == 0);
    size_t through = 0;
    for (const RefShape::Edge &e : S.edges) {
        CHECK(e.v < N && e.w < N && !S.kids[e.v].empty() && S.below(e.v) >= 2);
        through += e.through_root;
        if (e.through_root) CHECK(S.lo[e.v] == 0 && (size_t)ref.parent[e.w] == S.root);
    }
    CHECK(S.edges.size() == want.internodes && through == want.through_root);
    for (size_t v = 0; v < N; ++v) {
        CHECK(S.lo[v] < S.hi[v] && S.hi[v] <= n && S.links[v] == S.kids[v].size() + (v != S.root));
        for (size_t k = 1; k < S.kids[v].size(); ++k) CHECK(S.hi[S.kids[v][k - 1]] == S.lo[S.kids[v][k]]);
    }

    // the placement of every taxon and of every clade with three taxa outside it, under scores that put the best position at the
    // moved edge, elsewhere, everywhere at once and wherever a hash says
    std::vector<int64_t> score(N);
    for (int pattern = 0; pattern < 4 + (int)N; ++pattern) {
        for (size_t v = 0; v < N; ++v) score[v] = pattern == 0 ? 7 : pattern == 1 ? (int64_t)v : pattern == 2 ? -(int64_t)v : pattern == 3 ? (int64_t)(mix(v + n) % 5) : (int64_t)(v == (size_t)(pattern - 4));
        std::ostringstream taxa, clades;
        for (size_t x = 0; x < n; ++x) {
            place_taxa_line(taxa, ref, S, x, score.data());
            if (pattern == 0) {   // one score everywhere: the taxon stays, and every position is a best one
                std::vector<uint8_t> edge(N, 1);
                edge[S.root] = 0;
                const Placement p = summarise_placement(ref, S, ref.leaf_node[x], edge, x + 1, 1, score.data());
                CHECK(p.current == 7 && p.best == 7 && p.distance == 0 && p.n_best >= 1 && p.node < N);
            }
        }
        size_t placed = 0;
        for (size_t c = 0; c < N; ++c)
            if (c != S.root && !S.kids[c].empty() && n - S.below(c) >= 3) place_clades_line(clades, ref, S, placed++, c, score.data());
        CHECK(columns_match(kPlaceTaxaHeader, taxa.str()) == n && columns_match(kPlaceCladesHeader, clades.str()) == placed);
    }

    // the outputs per internode: rows of n_nodes x 4 words per taxon, tree or replicate
    std::vector<uint16_t> all(n), some, none;
    for (size_t i = 0; i < n; ++i) { all[i] = (uint16_t)i; if (i % 3 == 1) some.push_back((uint16_t)i); }
    for (const std::vector<uint16_t> &ids : {all, some, none}) {
        const size_t L = ids.size();
        std::vector<int64_t> rows((L + 1) * N * 4), pairs(L * n * 8);
        for (size_t v = 0; v < N; ++v)
            for (size_t c = 0; c < 4; ++c) {
                int64_t total = 0;
                for (size_t k = 0; k < L; ++k) total += rows[(k * N + v) * 4 + c] = (int64_t)(mix(k * 131 + v * 7 + c) % 4);   // (a taxon's row may hold all of an internode's 4-sets)
                rows[(L * N + v) * 4 + c] = v % 2 ? total : total + 3;
            }
        for (size_t i = 0; i < pairs.size(); i += 8) {
            int64_t *w = &pairs[i];
            w[0] = (int64_t)(mix(i) % 3); w[1] = (int64_t)(mix(i + 1) % 3); w[3] = (int64_t)(mix(i + 2) % 4); w[2] = w[3] / 2; w[5] = (int64_t)(mix(i + 3) % 4); w[4] = w[5] / 3;
            w[6] = w[2] + w[4]; w[7] = w[3] + w[5];
        }
        std::ostringstream drop, tp;
        drop_one_lines(drop, ref, S, ids, rows.data(), rows.data() + L * N * 4);
        taxon_pairs_lines(tp, ref, ids, pairs.data());
        CHECK(columns_match(kDropOneHeader, drop.str()) == L * S.edges.size());
        CHECK(columns_match(kTaxonPairsHeader, tp.str()) == n * (n - 1) / 2 - (n - L) * (n - L - 1) / 2);
    }
    for (size_t k : {size_t(0), size_t(1), size_t(5)}) {
        std::vector<int64_t> words(k * N * 4);
        for (size_t i = 0; i < words.size(); ++i) words[i] = (int64_t)(mix(i) % 3);
        std::ostringstream lines;
        branch_trees_lines(lines, S, 40, k, words.data());
        size_t present = 0;
        for (size_t t = 0; t < k; ++t) for (const RefShape::Edge &e : S.edges) present += words[(t * N + e.v) * 4] != 0;
        CHECK(columns_match(kBranchTreesHeader, lines.str()) == present);
    }
    for (size_t B : {size_t(1), size_t(2), size_t(41)}) {
        std::vector<int64_t> totals((1 + B) * N * 4);
        for (size_t i = 0; i < totals.size(); ++i) totals[i] = (int64_t)(mix(i + B) % 9) * (i % 5 != 0);
        std::ostringstream lines;
        bootstrap_lines(lines, S, B, totals.data());
        CHECK(columns_match(kBootstrapHeader, lines.str()) == S.edges.size());
    }
    for (double lambda : {0.5, 1e-3, 40.0}) {
        std::vector<int64_t> freq(N * 4);
        for (size_t v = 0; v < N; ++v) {   // en trees, their fractions in units of 2^-40: none, all on the first, spread
            const int64_t en = (int64_t)(v % 4) * 3, unit = int64_t(1) << 40;
            freq[4 * v] = en; freq[4 * v + 1] = v % 3 == 0 ? en * unit : en * unit / 2; freq[4 * v + 2] = v % 3 == 0 ? 0 : en * unit / 3; freq[4 * v + 3] = en * unit - freq[4 * v + 1] - freq[4 * v + 2];
        }
        std::ostringstream lines;
        local_pp_lines(lines, S, lambda, freq.data());
        CHECK(columns_match(kLocalPpHeader, lines.str()) == S.edges.size());
    }

    // the outputs per taxon, tree and hypothesis
    std::vector<int64_t> six(6 * n);
    for (size_t i = 0; i < six.size(); ++i) six[i] = (int64_t)(mix(i) % 4) * 4;
    std::ostringstream pt, grp, tree;
    per_taxon_lines(pt, ref, six.data());
    CHECK(columns_match(kPerTaxonHeader, pt.str()) == n);
    std::vector<int64_t> zeros(6 * n, 0);
    pt.str("");
    per_taxon_lines(pt, ref, zeros.data());   // nothing resolved: both ratios nan
    CHECK(columns_match(kPerTaxonHeader, pt.str()) == n && pt.str().find("nan\tnan\n") != std::string::npos);
    const std::vector<std::string> names{"first", "second", "third"};
    const uint8_t kind[3] = {0, 1, 0};
    test_groups_lines(grp, names, kind, six.data());
    CHECK(columns_match(kTestGroupsHeader, grp.str()) == 3);
    test_groups_lines(grp, {}, nullptr, nullptr);
    const uint32_t taxa[4] = {0, 3, 4, (uint32_t)n};
    const uint64_t counts[16] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 1, 1, 0, 0, 0, 0};
    per_tree_lines(tree, 4, taxa, counts);
    per_tree_lines(tree, 0, nullptr, nullptr);
    CHECK(columns_match(kPerTreeHeader, tree.str()) == 4);

    // --tree-taxa: a batch of four trees -- all taxa, three taxa (no line), every second taxon in any order, none -- with every taxon
    // kept, one kept and under a threshold no gain reaches
    std::vector<uint32_t> leaf_off{0};
    std::vector<uint16_t> leaf_ids;
    for (size_t x = 0; x < n; ++x) leaf_ids.push_back((uint16_t)x);
    leaf_off.push_back((uint32_t)leaf_ids.size());
    for (size_t x = 0; x < 3; ++x) leaf_ids.push_back((uint16_t)(n - 1 - x));
    leaf_off.push_back((uint32_t)leaf_ids.size());
    for (size_t x = n; x-- > 0;) if (x % 2 == 0) leaf_ids.push_back((uint16_t)x);
    const size_t half = leaf_ids.size() - leaf_off.back();
    leaf_off.push_back((uint32_t)leaf_ids.size());
    leaf_off.push_back((uint32_t)leaf_ids.size());
    std::vector<int64_t> tw(4 * n * 4);
    for (size_t i = 0; i < tw.size(); i += 4) { tw[i] = (int64_t)(mix(i) % 3) * 4; tw[i + 1] = (int64_t)(mix(i + 1) % 2) * 4; tw[i + 2] = tw[i] + tw[i + 1] + 1; tw[i + 3] = tw[i] + tw[i + 1]; }
    std::vector<uint8_t> keep_all(n, 1), keep_one(n, 0);
    keep_one[0] = 1;
    const double never = 2.0;
    std::ostringstream tt, one, nothing;
    tree_taxa_lines(tt, ref, 7, 4, leaf_off.data(), leaf_ids.data(), tw.data(), keep_all, nullptr);
    tree_taxa_lines(one, ref, 7, 4, leaf_off.data(), leaf_ids.data(), tw.data(), keep_one, nullptr);
    tree_taxa_lines(nothing, ref, 7, 4, leaf_off.data(), leaf_ids.data(), tw.data(), keep_all, &never);
    tree_taxa_lines(nothing, ref, 0, 0, leaf_off.data(), nullptr, nullptr, keep_all, nullptr);
    CHECK(columns_match(kTreeTaxaHeader, tt.str()) == n + (half >= 4 ? half : 0) && columns_match(kTreeTaxaHeader, one.str()) == 1 + (half >= 4) && nothing.str().empty());
    CHECK(tt.str().rfind("7\t0\t", 0) == 0 && (half < 4 || tt.str().find("\n9\t0\t") != std::string::npos) && tt.str().find("\n8\t") == std::string::npos);
}

// Lines worked out by hand on (((t0,t1),t2),t3,t4,(t5,t6,t7)): nodes in preorder 0 = root, 1 = ((t0,t1),t2), 2 = (t0,t1), 3 4 5 = t0 t1
// t2, 6 7 = t3 t4, 8 = (t5,t6,t7), 9 10 11 = t5 t6 t7. Node 1 has degree 3, so t2 and the clade (t0,t1) each share one position with
// the two other edges at it, and the node is no node on the way once either is taken out.
static void fixed_lines() {
    const RefFlat ref = flat("(((t0,t1),t2),t3,t4,(t5,t6,t7));");
    const RefShape S(ref);
    CHECK(S.nodes() == 12 && ref.leaf_node[2] == 5 && ref.leaf_node[6] == 10 && S.lo[8] == 5 && S.hi[8] == 8);
    std::vector<int64_t> score(12, 0);
    std::ostringstream taxon, same, clade, drop;
    // t2 is best placed on the edge above t6, ids [6, 7): one best position, and the root and node 8 lie between
    score[10] = 1;
    place_taxa_line(taxon, ref, S, 2, score.data());
    CHECK(taxon.str() == "2\tt2\t0\t1\t1\t1\t10\t6\t7\t2\n");
    // the best edge is the one above node 1, which is t2's own position: reported there, ids [0, 3), distance 0
    score.assign(12, 0);
    score[1] = score[2] = score[5] = 4;
    place_taxa_line(same, ref, S, 2, score.data());
    CHECK(same.str() == "2\tt2\t4\t4\t0\t1\t1\t0\t3\t0\n");
    // the clade (t0,t1), node 2, ids [0, 2), scores 3 where it is and 5 on the edge above t4, ids [4, 5): the root lies between
    score.assign(12, 0);
    score[2] = 3; score[7] = 5;
    place_clades_line(clade, ref, S, 0, 2, score.data());
    CHECK(clade.str() == "0\t2\t0\t2\t2\t3\t5\t2\t1\t7\t4\t5\t1\n");
    // --drop-one of t2 at the internodes above nodes 1, 2 and 8. Above node 1 t2 is alone in its link at a node of degree 3 and holds
    // all 5 of the internode's 4-sets: nan. Above node 2 it is alone in its link at the far end (group 1); sums (3, 3, 0) give
    // 1 - ln 2 / ln 3 = 0.369070, without its (2, 0, 0) the sums (1, 3, 0) give -(1 + (ln 0.25 / 4 + 3 ln 0.75 / 4) / ln 3) = -0.488140.
    // Above node 8 it is one of the 3 taxa below node 1 and in none of the 4-sets.
    std::vector<int64_t> words(2 * 12 * 4, 0);
    auto set = [&](size_t row, size_t v, std::vector<int64_t> w) { std::copy(w.begin(), w.end(), words.begin() + (std::ptrdiff_t)((row * 12 + v) * 4)); };
    set(0, 1, {5, 5, 0, 0}); set(1, 1, {5, 5, 0, 0});
    set(0, 2, {2, 2, 0, 0}); set(1, 2, {6, 3, 3, 0});
    set(1, 8, {4, 4, 0, 0});
    drop_one_lines(drop, ref, S, {2}, words.data(), words.data() + 12 * 4);
    CHECK(drop.str() == "2\tt2\t1\t0\t3\t1\t5\t5\t0\t0\t1.000000\tnan\tnan\n"
                        "2\tt2\t2\t0\t2\t1\t2\t2\t0\t0\t0.369070\t-0.488140\t-0.857211\n"
                        "2\tt2\t8\t5\t8\t3\t0\t0\t0\t0\t1.000000\t1.000000\t0.000000\n");
    // --tree-taxa of the tree ((((B,C),D),E),(A,F)) against (((((A,B),C),D),E),F): A holds the 10 discordant 4-sets, every other taxon 4
    // concordant and 6 discordant ones; the tree has 5 and 10, without A 5 of 5, without another taxon 1 of 5
    const RefFlat six = flat("(((((A,B),C),D),E),F);");
    const uint32_t leaf_off[2] = {0, 6};
    const uint16_t leaf_ids[6] = {1, 2, 3, 4, 0, 5};
    std::vector<int64_t> w{0, 10, 10, 10};
    for (int x = 1; x < 6; ++x) w.insert(w.end(), {4, 6, 10, 10});
    std::ostringstream all, rogue;
    const double G = 0.5;
    tree_taxa_lines(all, six, 3, 1, leaf_off, leaf_ids, w.data(), std::vector<uint8_t>(6, 1), nullptr);
    tree_taxa_lines(rogue, six, 3, 1, leaf_off, leaf_ids, w.data(), std::vector<uint8_t>(6, 1), &G);
    CHECK(rogue.str() == "3\t0\tA\t10\t0\t10\t0\t0\t0\t0.000000\t0.333333\t1.000000\t0.666667\n");
    CHECK(all.str().rfind(rogue.str(), 0) == 0 && all.str().find("3\t1\tB\t10\t4\t6\t0\t0\t0\t0.400000\t0.333333\t0.200000\t-0.133333\n") == rogue.str().size());
}

static void formats_and_sink() {
    CHECK(std::string(Fixed6(1, 3).text) == "0.333333" && std::string(Fixed6(0, 0).text) == "nan" && std::string(Fixed6(5, 0).text) == "nan");
    CHECK(std::string(Fixed6(-0.25).text) == "-0.250000" && std::string(Fixed6(std::nan("")).text) == "nan" && std::string(Fixed6(-std::nan("")).text) == "nan");
    CHECK(std::string(Fixed6(HUGE_VAL).text) == "inf" && std::string(Fixed6(1e300).text).size() == 63);   // (the longest number is cut, not overrun)
    const std::string path = "asan_cli_reports.tsv";
    {
        TsvFile f(path, "a\tb\n");
        f.f << 1 << '\t' << 2 << '\n';
        f.close();
    }
    std::ifstream in(path);
    std::stringstream got;
    got << in.rdbuf();
    CHECK(got.str() == "a\tb\n1\t2\n");
    std::remove(path.c_str());
    bool threw = false;
    try { TsvFile f("no-such-directory/x.tsv", "a\n"); } catch (const std::runtime_error &e) { threw = std::string(e.what()) == "cannot write no-such-directory/x.tsv"; }
    CHECK(threw);
}

int main() {
    drive("((t0,t1),t2,t3);", {1, 0});                               // 4 taxa
    drive("(t0,t1,t2,t3,t4);", {0, 0});                              // a star: no internode
    drive("(t0,t1,(t2,(t3,(t4,(t5,t6)))));", {4, 0});                // a caterpillar
    drive("(t0,((t1,t2),(t3,t4)));", {2, 0});                        // a degree-2 root beside a leaf: no internode through the root
    drive("((t0,t1),((t2,t3),(t4,t5)));", {3, 1});                   // a degree-2 root between two inner nodes: that internode once
    drive("(((t0,t1),t2),t3,t4,(t5,t6,t7));", {3, 0});               // a clade whose parent has degree 3; taxa alone beside such a node
    fixed_lines();
    formats_and_sink();
    std::puts("asan_cli_reports: ok");
    return 0;
}
