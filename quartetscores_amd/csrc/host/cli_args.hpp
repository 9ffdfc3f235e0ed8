// cli_args.hpp -- the command line of QuartetScores: its options (Args), the usage text, parse() driven by one table of option
// descriptions, the registry of output files from which every "needs ...", "already exists" and "is also another output file"
// refusal derives (check_output), and what each option checks beyond that before the device is touched.
#pragma once

#include "QuartetScoreComputer.hpp"
#include "cli_reports.hpp"
#include "table_shards.hpp"

#include <algorithm>
#include <map>
#include <sstream>
#include <cerrno>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <iostream>
#include <set>
#include <string>
#include <unistd.h>
#include <vector>

namespace qsh {

// true when something in the environment says "a tool rides along that flushes at exit"
inline bool wrapped_by_tool() {
    const char *pre = std::getenv("LD_PRELOAD");
    if (pre && *pre) return true;
    if (std::getenv("HSA_TOOLS_LIB")) return true;
    for (char **e = ::environ; e && *e; ++e) {
        const std::string kv = *e;
        if (kv.rfind("ROCP_", 0) == 0 || kv.rfind("ROCPROFILER_", 0) == 0 || kv.rfind("ROCTRACER_", 0) == 0 || kv.rfind("ASAN_OPTIONS", 0) == 0 ||
            kv.rfind("LLVM_PROFILE_FILE", 0) == 0 || kv.rfind("GCOV_PREFIX", 0) == 0) return true;
    }
    return false;
}

// --also-ref: a further reference tree and the file its annotated tree goes to
struct AlsoRef {
    std::string ref, out;
    Tree tree;
};

// --without-taxa: a file of taxon labels to drop and the file the annotated pruned -r tree goes to
struct WithoutTaxa {
    std::string names, out;
    std::set<std::string> drop;
    Tree tree;   // the -r tree without them
};

struct Args {
    std::string ref, eval, out, raw, raw_bin;
    std::string per_tree;   // --per-tree FILE: quartet agreement of every evaluation tree with -r (TSV)
    std::string tree_distances;   // --tree-distances FILE: quartet agreement and distance of every pair of evaluation trees (TSV)
    std::string per_taxon;  // --per-taxon FILE: quartet support per taxon of -r from the count table (TSV)
    std::string place_taxa; // --place-taxa FILE: quartet placement of the taxa of -r from the count table (TSV)
    std::string place_only; // --place-only NAMES: a file of the taxon labels to place (default: all)
    std::vector<uint16_t> place_ids;   // the lookup ids to place, ascending (check_taxon_list_output)
    std::string taxon_pairs;      // --taxon-pairs FILE: quartet support of the taxon pairs of -r from the count table (TSV)
    std::string taxon_pairs_only; // --taxon-pairs-only NAMES: a file of the taxon labels whose pairs are written (default: all)
    std::vector<uint16_t> pair_ids;    // the lookup ids whose rows are computed, ascending (check_taxon_list_output)
    std::string drop_one;         // --drop-one FILE: QP-IC of every internode of -r without each single taxon, from the count table (TSV)
    std::string drop_one_only;    // --drop-one-only NAMES: a file of the taxon labels to drop (default: all)
    std::vector<uint16_t> drop_ids;    // the lookup ids whose rows are computed, ascending (check_taxon_list_output)
    std::string branch_trees;     // --branch-trees FILE: per evaluation tree the quartet support of every internode of -r (TSV)
    std::string bootstrap;        // --bootstrap FILE: QP-IC of every internode of -r under a bootstrap over the evaluation trees (TSV)
    uint32_t bootstrap_reps = 100;   // --bootstrap-reps B
    uint64_t bootstrap_seed = 1;     // --bootstrap-seed S
    bool bootstrap_reps_given = false, bootstrap_seed_given = false;
    std::string tree_taxa;        // --tree-taxa FILE: per evaluation tree the quartet agreement of every taxon it holds with -r (TSV)
    std::string tree_taxa_only;   // --tree-taxa-only NAMES: a file of the taxon labels whose lines are written (default: all)
    std::vector<uint16_t> tree_taxa_ids;   // the lookup ids whose lines are written, ascending (check_taxon_list_output)
    double tree_taxa_min_gain = 0.0;       // --tree-taxa-min-gain G: only the lines with gain >= G
    bool tree_taxa_min_gain_given = false;
    std::string local_pp;         // --local-pp FILE: local posterior, coalescent length and polytomy test of every internode of -r (TSV)
    double local_pp_lambda = 0.5; // --local-pp-lambda L
    bool local_pp_lambda_given = false;
    std::string place_clades;      // --place-clades FILE: quartet placement of the clades of -r from the count table (TSV)
    std::string place_clades_only; // --place-clades-only SPEC: a file of the clades to place, one per line (default: every eligible inner clade)
    std::vector<uint32_t> place_nodes; // the nodes to place, in output order (check_place_clades)
    std::string test_groups_spec, test_groups;   // --test-groups SPEC FILE: quartet support of the taxon groups of SPEC from the count table (TSV)
    std::vector<std::string> group_names;        // the hypotheses of SPEC in its order (check_test_groups): name, labels [hypothesis][taxon], kind
    std::vector<uint8_t> group_labels, group_kind;
    std::vector<AlsoRef> also;
    std::vector<WithoutTaxa> without;
    std::string species_map;   // --species-map FILE: the evaluation trees' leaves are individuals of the species of -r (check_species_map -> dev.species)
    size_t threads = 0;
    bool verbose = false, savemem = false, raw_rank_order = false, fail_fast = false, clean_exit = false, fast_exit = false;
    int table_shards = -1;   // -1 = off (the whole table on the device); 0 = as many as the device's free memory asks for; K = K shards, one after the other (table_shards.hpp)
    int spill = 0;           // ShardedTableQuartetScoreComputer::Spill
    int gpus = 0;   // 0 = the single-GPU path; N >= 1 = N GPUs of this node: tree-sharded + one table collective (multi_gpu.hpp) or table-sharded (table_shards.hpp)
    std::string mode = "auto";   // --mode with --gpus N: tree | table | auto (the model of table_shards.hpp prefer_table_shards)
    DeviceOptions dev;
};

inline void usage(std::ostream &os) {
    os << "USAGE:\n   QuartetScores  [-s] [-v] [-t <uint>] [-q <string>] -o <string> -e <string> -r <string> [--version] [-h]\n"
          "   -r, --ref      Path to the reference tree\n"
          "   -e, --eval     Path to the evaluation trees\n"
          "   -o, --output   Path to the annotated newick output file (for lqic/qpic/eqpic scores)\n"
          "   -q, --qic      Path to the file where to write the raw QIC scores for each quartet\n"
          "   -t, --threads  Maximum number of host threads for parsing the evaluation trees (0 = all)\n"
          "   -v, --verbose  Verbose mode\n"
          "   -s, --savemem  Consume less memory (the GPU table is always the compact one; with a ROOTED reference tree the run\n"
          "                  ends with the reference's own std::runtime_error, see --root-as-edge; a note says so before the\n"
          "                  counting starts, --fail-fast ends the run there)\n"
          "   --device N     HIP device ordinal (default 0)\n"
          "   --gpus N       count on N GPUs of this node (devices --device .. --device+N-1)\n"
          "   --mode M       with --gpus: tree = the evaluation trees are split over the GPUs and the count tables combined with one\n"
          "                  reduction over xGMI; table = every GPU counts ALL trees into its shard of the table (by largest taxon\n"
          "                  id): no table collective, no communicator; auto (default) = table unless -q / --qic-binary need the\n"
          "                  whole table on one device or the table collective is the cheaper of the two (many trees, small table)\n"
          "   --reduce R     with --gpus: rccl (default: one RCCL reduce-scatter / all-reduce) | p2p (this one process maps its\n"
          "                  peers' memory and every GPU sums its chunk with plain loads: no communicator to create)\n"
          "   --comm-overlap 0|1  with --gpus, rccl: count while the communicators are being created (default 0: the first launch waits for them)\n"
          "   --algo A       gather (default) | scatter\n"
          "   --exact-qp     64-bit QP sums instead of the reference's 32-bit wrap\n"
          "   --qic-rank-order  -q lines in the order of the count table instead of the reference's loop order\n"
          "   --trace        time stamps of the counting pipeline on stderr\n"
          "   --clean-exit   tear the HIP runtime down before exiting (default: exit right after the output is written,\n"
          "                  unless LD_PRELOAD or a profiler's ROCP_* / ROCPROFILER_* / HSA_TOOLS_LIB environment is set)\n"
          "   --fast-exit    exit right after the output is written even under such a wrapper\n"
          "   --root-as-edge rooted reference tree: score the two root edges as one internode (the reference's\n"
          "                  own handling of a degree-2 root is the default)\n"
          "   --table-shards K  the count table in K shards by largest taxon id (0 = as many as the free device memory asks for):\n"
          "                  alone: a table larger than the device's memory passes through ONE GPU shard by shard;\n"
          "                  with --gpus N: shard s lives on GPU s mod N, every GPU counts all trees into its shard(s), no\n"
          "                  table collective (1024 taxa, 273 GB: --gpus 8 --table-shards 8). --gpus N alone switches to this\n"
          "                  mode by itself when the table does not fit one GPU\n"
          "   --spill M      with --table-shards: host (keep finished shards in host memory) | recount (count every shard a\n"
          "                  second time for the second scoring pass) | auto (host if it fits MemAvailable; default)\n"
          "   --save-table F write the count table to F after counting\n"
          "   --load-table F read the count table from F instead of counting (-e is still needed for m)\n"
          "   --qic-binary F raw per-quartet QIC as a binary file (topology byte + double per quartet, in rank order)\n"
          "   --also-ref REF OUT  (repeatable) score the reference tree REF as well and write its annotated tree to OUT: the count\n"
          "                  table of -r is re-indexed into REF's taxon order instead of counting again. REF must hold the same\n"
          "                  taxa as -r; one GPU with the whole table (not with --gpus / --table-shards); works with --load-table\n"
          "   --without-taxa NAMES OUT  (repeatable) score the -r tree without the taxa listed in NAMES (one label per line, as parsed and\n"
          "                  unquoted; blank lines are skipped) as well and write the annotated pruned tree to OUT: the count table is cut\n"
          "                  down to the kept taxa instead of pruning every tree and counting again. At least four taxa must remain; one\n"
          "                  GPU with the whole table (not with --gpus / --table-shards); works with --load-table, --per-tree, --per-taxon\n"
          "                  (both still the full -r tree) and beside --also-ref (whose trees are not pruned)\n"
          "   --species-map FILE  the evaluation trees hold several individuals (alleles, samples) per species and the -r tree one leaf\n"
          "                  per species: FILE maps them in ASTRAL's format, one line per species, species:ind1,ind2,... (blank lines and\n"
          "                  lines that start with # are skipped, surrounding blanks trimmed; a leaf of -r without a line is a species\n"
          "                  with one individual of the same name). The trees are counted under the individuals' ids and the count table\n"
          "                  is summed into the species' table on the device: a 4-set of species counts every choice of one individual\n"
          "                  per species (the multi-individual quartet score). Scores, -q and every output that reads the count table\n"
          "                  (--per-taxon, --place-taxa, --place-clades, --test-groups, --taxon-pairs, --drop-one, --without-taxa,\n"
          "                  --also-ref) then work on the species; --save-table writes the species' table, which a later --load-table\n"
          "                  run WITHOUT the map resumes on. At most 4096 individuals, at least 4 species; one GPU that counts (not\n"
          "                  with --gpus / --table-shards / --load-table) and not with the outputs computed from the trees themselves\n"
          "                  (--per-tree, --tree-distances, --branch-trees, --bootstrap, --local-pp, --tree-taxa)\n"
          "   --per-tree F   write the quartet agreement of every evaluation tree with the -r tree to F (TSV, one line per tree in\n"
          "                  -e order after a header: tree taxa quartets concordant discordant eval_only ref_only unresolved\n"
          "                  concordance); computed on the device behind the counting; one GPU that counts (not with --gpus /\n"
          "                  --table-shards / --load-table)\n"
          "   --tree-distances F  write the quartet agreement of every PAIR of evaluation trees to F (TSV, one line per pair a < b in\n"
          "                  row-major order of their -e numbers after a header: a b taxa quartets concordant discordant a_only b_only\n"
          "                  unresolved concordance distance). taxa = the taxa both trees hold, quartets = the 4-sets of those; both\n"
          "                  trees are restricted to them. distance = (discordant + a_only + b_only) / quartets, the normalised quartet\n"
          "                  distance that takes \"unresolved\" as a topology of its own; nan where quartets = 0. Needs no -r tree beyond\n"
          "                  its taxon names; computed on the device after the counting, m (m - 1) / 2 lines for m trees; one GPU that\n"
          "                  counts (not with --gpus / --table-shards / --load-table); works with --per-tree and beside the other outputs\n"
          "   --per-taxon F  write, per taxon of the -r tree, the support its quartets get from the count table to F (TSV, one line per\n"
          "                  taxon in lookup-id order after a header: taxon name quartets ref_resolved concordant discordant eval_only\n"
          "                  outvoted uninformed concordance concordance_without); one more read of the table on the device; a taxon\n"
          "                  whose concordance_without lies clearly above the others' is a rogue taxon; one GPU with the whole table\n"
          "                  (not with --gpus / --table-shards); works with --load-table, --also-ref (still the -r tree) and --per-tree\n"
          "   --place-taxa F write, per taxon of the -r tree, where the evaluation trees would put it to F (TSV, one line per taxon in\n"
          "                  lookup-id order after a header: taxon name current best gain n_best best_node best_lo best_hi distance).\n"
          "                  The score of a position = the sum, over the quartets that hold the taxon, of the count of the topology the\n"
          "                  -r tree shows with the taxon attached there; current = at its own edge, best = the largest over all edges,\n"
          "                  n_best = positions that attain it (one clearly better position: a misplaced taxon; none: an unstable one),\n"
          "                  best_node / [best_lo, best_hi) = node index and lookup ids below the edge of the reported position,\n"
          "                  distance = nodes between the two positions (0 = where it is, 1 = an NNI away). One gather over the table per\n"
          "                  taxon; one GPU with the whole table (not with --gpus / --table-shards); works with --load-table, --per-taxon,\n"
          "                  --per-tree, --also-ref and --without-taxa (always the full -r tree)\n"
          "   --place-only NAMES  with --place-taxa: place only the taxa listed in NAMES (one label per line, as for --without-taxa)\n"
          "   --place-clades F  write, per inner clade of the -r tree, where the evaluation trees would put the whole clade to F (TSV, one\n"
          "                  line per clade in node order after a header: clade node lo hi size current best gain n_best best_node best_lo\n"
          "                  best_hi distance). The clade (the subtree below `node`, lookup ids [lo, hi)) is pruned and regrafted, unchanged\n"
          "                  inside, on every edge outside it: one subtree-prune-and-regraft move per position. The score of a position =\n"
          "                  the sum, over the quartets with exactly one taxon of the clade, of the count of the topology the -r tree shows\n"
          "                  with the clade there (the other quartets do not see the move); the columns as for --place-taxa with the clade\n"
          "                  in the taxon's place (distance 1 = an NNI of the clade). Every inner clade with at least three taxa outside it\n"
          "                  is placed; one GPU with the whole table (not with --gpus / --table-shards); works with --load-table and\n"
          "                  beside the other outputs (always the full -r tree)\n"
          "   --place-clades-only SPEC  with --place-clades: place only the clades of SPEC, in its order: one clade per line, given as one\n"
          "                  or more labels separated by tabs = the smallest subtree of the -r tree, as rooted in its file, that holds\n"
          "                  them all (one label: that leaf)\n"
          "   --test-groups SPEC F  write the quartet support of user-defined taxon groups to F (TSV, one line per hypothesis of SPEC in\n"
          "                  its order after a header: name kind quartets q1 q2 q3 outvoted uninformed support qpic). SPEC holds one\n"
          "                  hypothesis per line (blank lines and lines that start with # are skipped): NAME<TAB>G1<TAB>G2<TAB>G3<TAB>G4\n"
          "                  asserts the branch G1 G2 | G3 G4 (kind quad), NAME<TAB>G1<TAB>G2 the bipartition G1 | G2 (kind split); a\n"
          "                  group is a comma-separated list of leaf labels of the -r tree, the groups of a line share no label, and one\n"
          "                  group of a split may be * = every taxon the other group does not name (is the named group monophyletic?).\n"
          "                  Labels that contain a tab or a comma cannot be named. quartets = the 4-sets with one taxon of each group\n"
          "                  (split: two of either); q1 = how often the evaluation trees show the asserted resolution of them, q2 and q3\n"
          "                  the two others; outvoted = 4-sets where another resolution is the most frequent, uninformed = 4-sets no\n"
          "                  tree resolves; support = q1 / (q1 + q2 + q3); qpic = the QP-IC of (q1, q2, q3), for the four subtrees beside\n"
          "                  an edge of a binary -r tree that edge's qp-ic with --exact-qp. In a split line the division of the\n"
          "                  discordant counts into q2 and q3 follows the order of the taxa in the -r tree and means nothing (only\n"
          "                  q2 + q3 does), and qpic is nan. The groups need not be clades of any tree; one more read of the table on the\n"
          "                  device per eight hypotheses; one GPU with the whole table (not with --gpus / --table-shards); works with\n"
          "                  --load-table and beside every other output\n"
          "   --taxon-pairs F  write, per pair of taxa of the -r tree, how the evaluation trees pair the two to F (TSV, one line per pair\n"
          "                  a < b of lookup ids, row by row, after a header: a b name_a name_b quartets ref_together ref_apart together\n"
          "                  apart affinity kept joined). Over the quartets = C(n-2,2) 4-sets that hold both taxa: ref_together /\n"
          "                  ref_apart = 4-sets in which the -r tree puts the two together / resolves them apart; together / apart = how\n"
          "                  often the evaluation trees show them together / show anything else; affinity = together / (together + apart);\n"
          "                  kept = the same ratio over the ref_together 4-sets, joined = over the ref_apart ones (nan where there is\n"
          "                  none). A pair whose joined stands out attracts each other against the -r tree (introgression, paralogy,\n"
          "                  long-branch attraction, a misplaced pair); the matrix is the quartet neighbourliness of the taxa. One gather\n"
          "                  over the table per taxon; one GPU with the whole table (not with --gpus / --table-shards); works with\n"
          "                  --load-table and beside every other output\n"
          "   --taxon-pairs-only NAMES  with --taxon-pairs: write only the pairs with a taxon listed in NAMES (one label per line, as for\n"
          "                  --place-only)\n"
          "   --drop-one F   write, per taxon and internal branch of the -r tree, what the branch's QP-IC would be without that taxon to F\n"
          "                  (TSV, after a header one line per taxon in id order and branch in node order: taxon name node lo hi group\n"
          "                  quartets q1 q2 q3 qpic qpic_without delta). [lo, hi) = the lookup ids below the branch, group = the number of\n"
          "                  taxa in the taxon's subtree beside the branch; quartets q1 q2 q3 = the 4-sets around the branch that hold the\n"
          "                  taxon and their share of the three sums behind QP-IC; qpic = the branch's QP-IC from exact sums, qpic_without\n"
          "                  = the same without the 4-sets that hold the taxon (nan where none is left: the taxon is alone beside a\n"
          "                  branching of degree 3, the branch dissolves with it), delta = qpic_without - qpic: a taxon with a large\n"
          "                  positive delta drags the branch down. A rooted -r tree's branch through the root is written once. LQ-IC and\n"
          "                  EQP-IC are minima and have no such decomposition. One gather over the table per taxon and one read of it;\n"
          "                  one GPU with the whole table (not with --gpus / --table-shards); works with --load-table and beside every\n"
          "                  other output\n"
          "   --drop-one-only NAMES  with --drop-one: write only the taxa listed in NAMES (one label per line, as for --place-only)\n"
          "   --branch-trees F  write, per evaluation tree and internal branch of the -r tree, how the tree resolves the 4-sets around that\n"
          "                  branch to F (TSV, after a header one line per tree in -e order and branch in node order: tree node lo hi present\n"
          "                  q1 q2 q3 concordance). [lo, hi) = the lookup ids below the branch; present = the 4-sets around the branch whose\n"
          "                  four taxa the tree holds; q1 = how many of them it shows as the -r tree does, q2 and q3 the two other\n"
          "                  resolutions, in the order of --drop-one's sums (the q1 q2 q3 of all trees add up to them); concordance =\n"
          "                  q1 / (q1 + q2 + q3), nan where the tree resolves none. Lines with present = 0 are left out; a rooted -r\n"
          "                  tree's branch through the root is written once. Which gene trees contradict this branch: computed on the\n"
          "                  device behind the counting from the trees themselves; one GPU that counts (not with --gpus / --table-shards /\n"
          "                  --load-table); works beside every other output\n"
          "   --bootstrap F  write, per internal branch of the -r tree, its QP-IC under a bootstrap over the evaluation trees to F (TSV,\n"
          "                  one line per branch in node order after a header: node lo hi qpic mean sd lo95 hi95 reps). qpic = the\n"
          "                  branch's QP-IC from exact sums (--drop-one's qpic); a replicate draws as many trees as there are, with\n"
          "                  replacement, and its QP-IC is that of the redrawn trees' sums: a reweighting of the per-tree sums of\n"
          "                  --branch-trees, not a recount. mean and sd (of the population) are over the replicates, lo95 / hi95 their\n"
          "                  2.5 % / 97.5 % points (the sorted values at floor(0.025 (B-1)) and ceil(0.975 (B-1))). One GPU that counts\n"
          "                  (not with --gpus / --table-shards / --load-table); works with --branch-trees and beside every other output\n"
          "   --bootstrap-reps B  with --bootstrap: the number of replicates (default 100)\n"
          "   --bootstrap-seed S  with --bootstrap: the seed of the resampling (default 1); the same seed gives the same file\n"
          "   --local-pp F   write, per internal branch of the -r tree, its local posterior probability, its length in coalescent units\n"
          "                  and the polytomy test to F (TSV, one line per branch in node order after a header: node lo hi en f1 f2 f3\n"
          "                  pp1 pp2 pp3 length polytomy_p). Every evaluation tree gives the FRACTIONS of the 4-sets around the branch\n"
          "                  that it resolves as the -r tree does and as the two alternatives (--branch-trees' q1 q2 q3 over their sum), so\n"
          "                  a tree that lacks half the taxa weighs as much as a complete one; en = the trees that resolve any, f1 f2 f3 =\n"
          "                  the sums of the fractions (exact in units of 2^-40). pp1 = the posterior of the branch, pp2 pp3 = of its two\n"
          "                  alternatives in the order of q2 q3 (Sayyari & Mirarab 2016), length = -ln(3/2 (1 - f1 / (en + 2L - 1))), 0\n"
          "                  where f1 / (en + 2L - 1) <= 1/3 and inf where it is >= 1, polytomy_p = the p-value of the chi-square test of\n"
          "                  f1 = f2 = f3 (2 degrees of freedom; Sayyari & Mirarab 2018). nan where en = 0. The model assumes a binary\n"
          "                  branch: where the -r tree's branch ends in a node of degree above 3 the figures are written as computed from\n"
          "                  the sums over all pairs of its groups. One GPU that counts (not with --gpus / --table-shards /\n"
          "                  --load-table), fewer than 2^23 evaluation trees; works with --branch-trees / --bootstrap and beside every\n"
          "                  other output\n"
          "   --local-pp-lambda L  with --local-pp: the rate of the prior on branch lengths, L > 0 (default 0.5)\n"
          "   --tree-taxa F  write, per evaluation tree and taxon the tree holds, how the 4-sets of the tree that hold the taxon agree with\n"
          "                  the -r tree to F (TSV, after a header one line per tree in -e order and taxon in lookup-id order: tree taxon name\n"
          "                  quartets concordant discordant eval_only ref_only unresolved concordance tree_concordance concordance_without\n"
          "                  gain). quartets = C(L-1,3) for a tree of L taxa; the counts as in --per-tree, over the 4-sets that hold the\n"
          "                  taxon; concordance = concordant / (concordant + discordant); tree_concordance = the tree's own (--per-tree's\n"
          "                  figure); concordance_without = the tree's concordance over the 4-sets that do NOT hold the taxon; gain =\n"
          "                  concordance_without - tree_concordance: how much the tree's agreement with the -r tree rises when this one\n"
          "                  leaf is taken out of this one tree (one contaminated, paralogous or misaligned sequence). nan where a\n"
          "                  denominator is 0; trees with fewer than four taxa write no line. The full file has (trees x taxa) lines.\n"
          "                  Computed on the device behind the counting from the trees themselves, written batch by batch; one GPU that\n"
          "                  counts (not with --gpus / --table-shards / --load-table), at most 1277 taxa; works with --per-tree,\n"
          "                  --branch-trees, --bootstrap, --local-pp and beside every other output\n"
          "   --tree-taxa-only NAMES  with --tree-taxa: write only the lines of the taxa listed in NAMES (one label per line, as for\n"
          "                  --place-only)\n"
          "   --tree-taxa-min-gain G  with --tree-taxa: write only the lines with gain >= G (lines whose gain is nan are dropped): the\n"
          "                  list of rogue leaves\n";
}

// One option of the command line. `text` is how messages name it (its name unless a row says otherwise); the target is the member that
// fits the kind. `check`, where a row has one, sees the value after `str` has taken it, stores what the row keeps elsewhere and returns
// what is wrong with it ("" = nothing). A TWO's text is what it takes ("REF OUT"), `dash` says whether a second value that starts with
// '-' counts as missing, and `two` stores the pair.
struct Option {
    enum Kind { SWITCH, STRING, UNSIGNED, TWO } kind;
    const char *name, *alias, *text;
    bool *on = nullptr;
    std::string *str = nullptr;
    std::function<void(unsigned long)> num;
    std::function<std::string(const char *)> check;
    std::function<void(const char *, const char *)> two;
    bool dash = false;
};

inline std::vector<Option> options(Args &a) {
    auto row = [](Option::Kind kind, const char *name, const char *alias, const char *text) { Option o; o.kind = kind; o.name = name; o.alias = alias; o.text = text ? text : name; return o; };
    auto sw = [&](const char *name, bool *on, const char *alias = nullptr) { Option o = row(Option::SWITCH, name, alias, nullptr); o.on = on; return o; };
    auto str = [&](const char *name, std::string *s, const char *alias = nullptr, const char *text = nullptr) { Option o = row(Option::STRING, name, alias, text); o.str = s; return o; };
    auto checked = [&](const char *name, std::string *s, std::function<std::string(const char *)> check) { Option o = str(name, s); o.check = std::move(check); return o; };
    auto num = [&](const char *name, std::function<void(unsigned long)> f, const char *alias = nullptr, const char *text = nullptr) { Option o = row(Option::UNSIGNED, name, alias, text); o.num = std::move(f); return o; };
    auto two = [&](const char *name, const char *takes, bool dash, std::function<void(const char *, const char *)> store) { Option o = row(Option::TWO, name, nullptr, takes); o.dash = dash; o.two = std::move(store); return o; };
    return {
        str("-r", &a.ref, "--ref", "-r (--ref)"), str("-e", &a.eval, "--eval", "-e (--eval)"), str("-o", &a.out, "--output", "-o (--output)"),
        str("-q", &a.raw, "--qic", "-q (--qic)"), num("-t", [&a](unsigned long v) { a.threads = v; }, "--threads", "-t (--threads)"),
        sw("-v", &a.verbose, "--verbose"), sw("-s", &a.savemem, "--savemem"),
        num("--gpus", [&a](unsigned long v) { a.gpus = (int)v; }), num("--table-shards", [&a](unsigned long v) { a.table_shards = (int)v; }),
        num("--device", [&a](unsigned long v) { a.dev.device = (int)v; }), num("--comm-overlap", [&a](unsigned long v) { a.dev.comm_overlap = v != 0; }),
        num("--bootstrap-reps", [&a](unsigned long v) { a.bootstrap_reps = (uint32_t)std::min<unsigned long>(v, 0xFFFFFFFFul); a.bootstrap_reps_given = true; }),
        num("--bootstrap-seed", [&a](unsigned long v) { a.bootstrap_seed = v; a.bootstrap_seed_given = true; }),
        sw("--exact-qp", &a.dev.qp_exact64), sw("--root-as-edge", &a.dev.root_as_edge), sw("--fail-fast", &a.fail_fast), sw("--clean-exit", &a.clean_exit),
        sw("--fast-exit", &a.fast_exit), sw("--gpus-on-one-device", &a.dev.gpus_on_one_device), sw("--trace", &a.dev.trace), sw("--qic-rank-order", &a.raw_rank_order),
        str("--save-table", &a.dev.save_table), str("--load-table", &a.dev.load_table), str("--qic-binary", &a.raw_bin), str("--per-tree", &a.per_tree),
        str("--tree-distances", &a.tree_distances), str("--per-taxon", &a.per_taxon), str("--place-taxa", &a.place_taxa), str("--place-only", &a.place_only),
        str("--taxon-pairs", &a.taxon_pairs), str("--taxon-pairs-only", &a.taxon_pairs_only), str("--drop-one", &a.drop_one), str("--drop-one-only", &a.drop_one_only),
        str("--branch-trees", &a.branch_trees), str("--bootstrap", &a.bootstrap), str("--local-pp", &a.local_pp), str("--place-clades", &a.place_clades),
        str("--place-clades-only", &a.place_clades_only), str("--tree-taxa", &a.tree_taxa), str("--tree-taxa-only", &a.tree_taxa_only),
        str("--species-map", &a.species_map),
        checked("--tree-taxa-min-gain", nullptr, [&a](const char *v) -> std::string {
            char *end = nullptr;
            a.tree_taxa_min_gain = std::strtod(v, &end);
            if (end == v || *end != '\0' || !std::isfinite(a.tree_taxa_min_gain))
                return std::string("Couldn't read argument value from string '") + v + "' for arg --tree-taxa-min-gain (a number)";
            a.tree_taxa_min_gain_given = true;
            return "";
        }),
        checked("--spill", nullptr, [&a](const char *v) -> std::string {
            const std::string sv = v;
            a.spill = sv == "host" ? ShardedTableQuartetScoreComputer::SPILL_HOST : sv == "recount" ? ShardedTableQuartetScoreComputer::SPILL_RECOUNT : ShardedTableQuartetScoreComputer::SPILL_AUTO;
            return sv == "host" || sv == "recount" || sv == "auto" ? "" : "--spill takes host, recount or auto";
        }),
        checked("--algo", nullptr, [&a](const char *v) -> std::string { a.dev.algo = std::string(v) == "scatter" ? QS_ALGO_SCATTER : QS_ALGO_GATHER; return ""; }),
        checked("--mode", &a.mode, [&a](const char *) -> std::string { return a.mode != "auto" && a.mode != "tree" && a.mode != "table" ? "--mode takes auto, tree or table" : ""; }),
        checked("--reduce", &a.dev.reduce, [&a](const char *) -> std::string { return a.dev.reduce != "rccl" && a.dev.reduce != "p2p" ? "--reduce takes rccl or p2p" : ""; }),
        checked("--local-pp-lambda", nullptr, [&a](const char *v) -> std::string {
            char *end = nullptr;
            a.local_pp_lambda = std::strtod(v, &end);
            if (end == v || *end != '\0' || !std::isfinite(a.local_pp_lambda) || !(a.local_pp_lambda > 0.0))
                return std::string("Couldn't read argument value from string '") + v + "' for arg --local-pp-lambda (a positive number)";
            a.local_pp_lambda_given = true;
            return "";
        }),
        two("--test-groups", "SPEC FILE", false, [&a](const char *spec, const char *file) { a.test_groups_spec = spec; a.test_groups = file; }),
        two("--also-ref", "REF OUT", true, [&a](const char *ref, const char *out) { AlsoRef x; x.ref = ref; x.out = out; a.also.push_back(std::move(x)); }),
        two("--without-taxa", "NAMES OUT", true, [&a](const char *names, const char *out) { WithoutTaxa x; x.names = names; x.out = out; a.without.push_back(std::move(x)); })};
}

// returns 0 ok, 1 error (message printed like the reference prints TCLAP::ArgException), 2 exit quietly
inline int parse(int argc, char **argv, Args &a) {
    const std::vector<Option> table = options(a);
    auto fail = [](const std::string &what) { std::cerr << "ERROR: " << what << std::endl; return 1; };
    for (int i = 1; i < argc; ++i) {
        const std::string f = argv[i];
        if (f == "--version") { std::cout << argv[0] << "  version: 1.0.1 (" << qs_version() << ")" << std::endl; return 2; }
        if (f == "-h" || f == "--help") { usage(std::cout); return 2; }
        const Option *o = nullptr;
        for (const Option &x : table)
            if (f == x.name || (x.alias && f == x.alias)) { o = &x; break; }
        if (!o) return fail("Couldn't find match for argument for arg " + f);
        if (o->kind == Option::SWITCH) { *o->on = true; continue; }
        if (o->kind == Option::TWO) {
            if (i + 2 >= argc || (o->dash && argv[i + 2][0] == '-')) return fail("Missing a value for this argument! for arg " + f + " (it takes two: " + o->text + ")");
            o->two(argv[i + 1], argv[i + 2]);
            i += 2;
            continue;
        }
        if (i + 1 >= argc) return fail(std::string("Missing a value for this argument! for arg ") + o->text);
        const char *v = argv[++i];
        if (o->str) *o->str = v;
        if (o->kind == Option::UNSIGNED) {
            // a malformed number is reported like the other argument errors (tclap: "Couldn't read argument value from string"), not
            // an uncaught std::invalid_argument
            char *end = nullptr;
            errno = 0;
            const unsigned long val = std::strtoul(v, &end, 10);
            if (end == v || *end != '\0' || errno != 0 || v[0] == '-') return fail(std::string("Couldn't read argument value from string '") + v + "' for arg " + o->text);
            o->num(val);
        }
        const std::string wrong = o->check ? o->check(v) : std::string();
        if (!wrong.empty()) return fail(wrong);
    }
    const char *missing = a.ref.empty() ? "-r (--ref)" : a.eval.empty() ? "-e (--eval)" : a.out.empty() ? "-o (--output)" : nullptr;
    if (missing) return fail(std::string("Required argument missing: for arg ") + missing);
    // A wrapper that flushes in its exit handlers (rocprofv3, a tracer, a coverage or sanitizer runtime) would lose its output to the
    // fast exit: with a preloaded library or a profiler's environment the ordinary return is the default (--fast-exit overrides)
    if (!a.clean_exit && !a.fast_exit && wrapped_by_tool()) a.clean_exit = true;
    return 0;
}

// What an output option needs of the run
enum class Needs {
    NOTHING,        // written on every route
    WHOLE_TABLE,    // read from the count table: the whole table on one GPU
    COUNTED_TREES,  // computed from the trees behind their count: trees counted on one GPU
};

// One row per output option: its flag, its FILE (empty = not given), what it needs, and the companion option `only` that restricts it
struct Output {
    const char *flag;
    const std::string &path;
    Needs needs;
    const char *only_flag;
    const std::string *only;
};

inline std::vector<Output> output_registry(const Args &a) {
    return {{"-o", a.out, Needs::NOTHING, nullptr, nullptr},
            {"-q", a.raw, Needs::NOTHING, nullptr, nullptr},
            {"--qic-binary", a.raw_bin, Needs::NOTHING, nullptr, nullptr},
            {"--save-table", a.dev.save_table, Needs::NOTHING, nullptr, nullptr},
            {"--per-tree", a.per_tree, Needs::COUNTED_TREES, nullptr, nullptr},
            {"--tree-distances", a.tree_distances, Needs::COUNTED_TREES, nullptr, nullptr},
            {"--per-taxon", a.per_taxon, Needs::WHOLE_TABLE, nullptr, nullptr},
            {"--place-taxa", a.place_taxa, Needs::WHOLE_TABLE, "--place-only", &a.place_only},
            {"--place-clades", a.place_clades, Needs::WHOLE_TABLE, "--place-clades-only", &a.place_clades_only},
            {"--test-groups", a.test_groups, Needs::WHOLE_TABLE, nullptr, nullptr},
            {"--taxon-pairs", a.taxon_pairs, Needs::WHOLE_TABLE, "--taxon-pairs-only", &a.taxon_pairs_only},
            {"--drop-one", a.drop_one, Needs::WHOLE_TABLE, "--drop-one-only", &a.drop_one_only},
            {"--branch-trees", a.branch_trees, Needs::COUNTED_TREES, nullptr, nullptr},
            {"--bootstrap", a.bootstrap, Needs::COUNTED_TREES, nullptr, nullptr},
            {"--local-pp", a.local_pp, Needs::COUNTED_TREES, nullptr, nullptr},
            {"--tree-taxa", a.tree_taxa, Needs::COUNTED_TREES, "--tree-taxa-only", &a.tree_taxa_only}};
}

// Every output file of the command line with the option that names it; an option that was not given has an empty path
inline std::vector<std::pair<std::string, std::string>> output_files(const Args &a) {
    std::vector<std::pair<std::string, std::string>> files;
    for (const Output &o : output_registry(a)) files.emplace_back(o.flag, o.path);
    for (const AlsoRef &x : a.also) files.emplace_back("--also-ref", x.out);
    for (const WithoutTaxa &x : a.without) files.emplace_back("--without-taxa", x.out);
    return files;
}

// The registry's row of the output option `flag`
inline Output output_row(const Args &a, const std::string &flag) {
    for (const Output &o : output_registry(a))
        if (flag == o.flag) return o;
    throw std::logic_error(flag + " is not an output option");
}

// The output option `flag` of the registry, before the device is touched: its companion needs it, and where it is given the run must
// offer what it needs and its FILE must neither be another output of the command line nor exist. Returns whether it is given.
inline bool check_output(const Args &a, const std::string &flag) {
    const Output o = output_row(a, flag);
    if (o.path.empty()) {
        if (o.only && !o.only->empty()) throw std::runtime_error(std::string(o.only_flag) + " needs " + flag + " FILE");
        return false;
    }
    const bool split = a.gpus > 0 || a.table_shards >= 0;
    if (o.needs == Needs::WHOLE_TABLE && split) throw std::runtime_error(flag + " needs the whole count table on one GPU: omit --gpus / --table-shards");
    if (o.needs == Needs::COUNTED_TREES && (split || !a.dev.load_table.empty()))
        throw std::runtime_error(flag + " needs the evaluation trees counted on one GPU: omit --gpus / --table-shards / --load-table");
    if (o.needs == Needs::COUNTED_TREES && !a.species_map.empty())
        throw std::runtime_error(flag + " compares every evaluation tree with the -r tree leaf by leaf, and with --species-map the trees hold individuals, the -r tree species: omit one of the two");
    for (const auto &e : output_files(a))
        if (e.first != flag && e.second == o.path) throw std::runtime_error(flag + ": " + o.path + " is also another output file");
    if (std::ifstream(o.path).good()) throw std::runtime_error(flag + ": the output file " + o.path + " already exists");
    return true;
}

// the -r tree
inline Tree read_reference(const Args &a) {
    Tree primary;
    const std::string text = slurp(a.ref);
    NewickReader rr(text);
    if (!rr.next(primary)) throw std::runtime_error("empty reference tree file");
    return primary;
}

// --species-map FILE: everything before the device is touched -- the routes that cannot take it are refused, the file parses against
// the leaves of -r (each message names the offending label), and the layout of the individuals is left in a.dev.species
inline void check_species_map(Args &a) {
    if (a.species_map.empty()) return;
    const std::string what = "--species-map " + a.species_map + ": ";
    if (!a.dev.load_table.empty())
        throw std::runtime_error("--species-map does not work with --load-table: a saved table holds no names, and the table a --species-map run saves is the species' table already (load it without the map)");
    if (a.gpus > 0 || a.table_shards >= 0)
        throw std::runtime_error("--species-map needs the individuals' whole count table on one GPU: omit --gpus / --table-shards");
    const RefFlat rf = flatten_reference(read_reference(a));
    auto trimmed = [](const std::string &t) {
        const size_t b = t.find_first_not_of(" \t\r"), e = t.find_last_not_of(" \t\r");
        return b == std::string::npos ? std::string() : t.substr(b, e - b + 1);
    };
    std::map<std::string, std::vector<std::string>> listed;   // species -> its individuals in file order
    std::map<std::string, std::string> owner;                 // individual -> species
    std::istringstream lines(slurp(a.species_map));
    size_t line_no = 0;
    for (std::string line; std::getline(lines, line);) {
        ++line_no;
        const std::string at = what + "line " + std::to_string(line_no) + ": ";
        line = trimmed(line);
        if (line.empty() || line[0] == '#') continue;
        const size_t colon = line.find(':');
        if (colon == std::string::npos) throw std::runtime_error(at + "no ':' in '" + line + "'");
        const std::string species = trimmed(line.substr(0, colon));
        if (species.empty()) throw std::runtime_error(at + "no species name in front of ':'");
        if (!rf.name_to_id.count(species)) throw std::runtime_error(at + "the species '" + species + "' is not a leaf of the reference tree " + a.ref);
        if (listed.count(species)) throw std::runtime_error(at + "the species '" + species + "' has two lines");
        std::vector<std::string> &inds = listed[species];
        const std::string rest = line.substr(colon + 1);
        if (trimmed(rest).empty()) throw std::runtime_error(at + "the species '" + species + "' has an empty individual list");
        for (size_t from = 0;;) {
            const size_t comma = rest.find(',', from);
            const std::string ind = trimmed(rest.substr(from, comma == std::string::npos ? std::string::npos : comma - from));
            if (ind.empty()) throw std::runtime_error(at + "the species '" + species + "' lists an empty individual name");
            const auto ins = owner.emplace(ind, species);
            if (!ins.second) throw std::runtime_error(at + "the individual '" + ind + "' is listed twice (species '" + ins.first->second + "' and '" + species + "')");
            inds.push_back(ind);
            if (comma == std::string::npos) break;
            from = comma + 1;
        }
    }
    for (const auto &kv : owner)
        if (rf.name_to_id.count(kv.first) && !listed.count(kv.first))
            throw std::runtime_error(what + "the individual '" + kv.first + "' of species '" + kv.second + "' has the name of the unlisted species '" + kv.first + "'");
    if (rf.names.size() < 4) throw std::runtime_error(what + "fewer than 4 species (" + std::to_string(rf.names.size()) + ") in the reference tree " + a.ref);
    auto sp = std::make_shared<SpeciesLayout>();
    std::vector<uint64_t> sizes;
    sp->first_id.push_back(0);
    for (const std::string &species : rf.names) {
        const auto it = listed.find(species);
        if (it == listed.end()) sp->names.push_back(species);
        else sp->names.insert(sp->names.end(), it->second.begin(), it->second.end());
        if (sp->names.size() > 4096)
            throw std::runtime_error(what + "more than 4096 individuals in all (reached at the species '" + species + "')");
        sizes.push_back(sp->names.size() - sp->first_id.back());
        sp->first_id.push_back((uint16_t)sp->names.size());
    }
    for (size_t i = 0; i < sp->names.size(); ++i) sp->name_to_id[sp->names[i]] = (uint32_t)i;
    std::sort(sizes.begin(), sizes.end());
    for (size_t k = sizes.size() - 4; k < sizes.size(); ++k) sp->top4 *= sizes[k];
    a.dev.species = sp;
}

// A NAMES file (--without-taxa, --place-only): one label per line, as parsed and unquoted; surrounding blanks go, blank lines are skipped,
// a repeated label counts once. Returns the labels; `what` prefixes the message for a label the -r tree lacks.
inline std::set<std::string> read_taxon_names(const std::string &path, const RefFlat &rf, const std::string &ref_path, const std::string &what) {
    std::set<std::string> names;
    std::istringstream lines(slurp(path));
    for (std::string line; std::getline(lines, line);) {
        const size_t b = line.find_first_not_of(" \t\r"), e = line.find_last_not_of(" \t\r");
        if (b == std::string::npos) continue;
        const std::string name = line.substr(b, e - b + 1);
        if (!rf.name_to_id.count(name)) throw std::runtime_error(what + "the taxon " + name + " is not in the reference tree " + ref_path);
        names.insert(name);
    }
    if (names.empty()) throw std::runtime_error(what + "the list of taxa is empty");
    return names;
}

// --X FILE [--X-only NAMES], an output per listed taxon of -r (--place-taxa, --taxon-pairs, --drop-one): beyond check_output, refused
// where NAMES holds a label the -r tree lacks; returns the lookup ids to compute, ascending (all without NAMES; none without FILE)
inline std::vector<uint16_t> check_taxon_list_output(const Args &a, const std::string &flag) {
    if (!check_output(a, flag)) return {};
    const Output o = output_row(a, flag);
    const RefFlat rf = flatten_reference(read_reference(a));
    std::set<uint16_t> ids;
    if (o.only->empty()) {
        for (size_t i = 0; i < rf.names.size(); ++i) ids.insert((uint16_t)i);
    } else {
        for (const std::string &name : read_taxon_names(*o.only, rf, a.ref, std::string(o.only_flag) + " " + *o.only + ": ")) ids.insert((uint16_t)rf.name_to_id.at(name));
    }
    return std::vector<uint16_t>(ids.begin(), ids.end());
}

// The OUT of an --also-ref / --without-taxa, `what` in front of the message: refused where it exists or is one of `taken`, which it joins
inline void check_second_tree_file(const std::string &what, const std::string &out, std::set<std::string> &taken) {
    if (!taken.insert(out).second) throw std::runtime_error(what + "the output file " + out + " is given twice");
    if (std::ifstream(out).good()) throw std::runtime_error(what + "the output file " + out + " already exists");
}

// --also-ref: everything that needs no GPU, before the device is touched -- the files parse, every tree holds exactly the
// taxa of -r, no OUT exists or repeats -o or another OUT, and qs_score_check passes for every tree with the run's flags
inline void check_also_refs(Args &a) {
    if (a.also.empty()) return;
    if (a.gpus > 0 || a.table_shards >= 0)
        throw std::runtime_error("--also-ref works on one GPU with the whole table: omit --gpus / --table-shards");
    Tree primary = read_reference(a);
    const RefFlat rf = flatten_reference(primary);
    const std::set<std::string> names(rf.names.begin(), rf.names.end());
    std::set<std::string> outs;
    for (const Output &o : output_registry(a))
        if (!std::strcmp(o.flag, "-o")) outs.insert(o.path);   // of the registry, an OUT is held against the annotated tree alone
    for (AlsoRef &x : a.also) {
        check_second_tree_file("--also-ref " + x.ref + ": ", x.out, outs);
        const std::string text = slurp(x.ref);
        NewickReader rr(text);
        if (!rr.next(x.tree)) throw std::runtime_error("--also-ref " + x.ref + ": empty reference tree file");
        const RefFlat fx = flatten_reference(x.tree);
        const std::set<std::string> other(fx.names.begin(), fx.names.end());
        std::string missing, extra;
        for (const std::string &s : names) if (!other.count(s)) missing += (missing.empty() ? "" : ", ") + s;
        for (const std::string &s : other) if (!names.count(s)) extra += (extra.empty() ? "" : ", ") + s;
        if (!missing.empty() || !extra.empty())
            throw std::runtime_error("--also-ref " + x.ref + ": the taxa differ from those of the reference tree " + a.ref + " (missing: " +
                                     (missing.empty() ? "none" : missing) + "; extra: " + (extra.empty() ? "none" : extra) + ")");
        const qs_ref_tree rt = ref_view(fx);
        if (qs_score_check(nullptr, &rt, score_flags(a.dev)) != QS_OK) throw std::runtime_error("--also-ref " + x.ref + ": " + qs_last_error(nullptr));
    }
}

// --without-taxa: everything that needs no GPU, before the device is touched -- every name is a taxon of -r, at least one is dropped
// and four are kept, no OUT exists or repeats another output, and qs_score_check passes for every pruned tree with the run's flags
inline void check_without_taxa(Args &a) {
    if (a.without.empty()) return;
    if (a.gpus > 0 || a.table_shards >= 0)
        throw std::runtime_error("--without-taxa works on one GPU with the whole table: omit --gpus / --table-shards");
    Tree primary = read_reference(a);
    const RefFlat rf = flatten_reference(primary);
    std::set<std::string> outs;
    // of the registry, an OUT is held against the outputs every route writes and --per-tree / --per-taxon (given or not: an empty OUT
    // is refused with them); every other output holds its own FILE against the OUTs (check_output)
    for (const Output &o : output_registry(a))
        if (o.needs == Needs::NOTHING || !std::strcmp(o.flag, "--per-tree") || !std::strcmp(o.flag, "--per-taxon")) outs.insert(o.path);
    for (const AlsoRef &x : a.also) outs.insert(x.out);
    for (WithoutTaxa &x : a.without) {
        const std::string what = "--without-taxa " + x.names + ": ";
        check_second_tree_file(what, x.out, outs);
        x.drop = read_taxon_names(x.names, rf, a.ref, what);
        if (rf.names.size() < x.drop.size() + 4)
            throw std::runtime_error(what + "fewer than four taxa are left (" + std::to_string(rf.names.size() - x.drop.size()) + " of " + std::to_string(rf.names.size()) + ")");
        prune(primary, x.drop, x.tree);
        const RefFlat fx = flatten_reference(x.tree);
        const qs_ref_tree rt = ref_view(fx);
        if (qs_score_check(nullptr, &rt, score_flags(a.dev)) != QS_OK) throw std::runtime_error(what + qs_last_error(nullptr));
    }
}

// --branch-trees / --bootstrap / --local-pp: beyond check_output, their companions need them and a bootstrap needs a replicate
inline void check_tree_branches(const Args &a) {
    if (a.bootstrap.empty() && (a.bootstrap_reps_given || a.bootstrap_seed_given)) throw std::runtime_error("--bootstrap-reps / --bootstrap-seed need --bootstrap FILE");
    if (a.local_pp.empty() && a.local_pp_lambda_given) throw std::runtime_error("--local-pp-lambda needs --local-pp FILE");
    for (const char *flag : {"--branch-trees", "--bootstrap", "--local-pp"}) check_output(a, flag);
    if (!a.bootstrap.empty() && a.bootstrap_reps == 0) throw std::runtime_error("--bootstrap-reps must be at least 1");
}

// --tree-taxa: beyond check_taxon_list_output, its second companion needs it and the -r tree must be within the limit of the device's
// plan (qs_tree_taxa_plan, host-only); leaves the lookup ids to write in a.tree_taxa_ids
inline void check_tree_taxa(Args &a) {
    if (a.tree_taxa.empty() && a.tree_taxa_min_gain_given) throw std::runtime_error("--tree-taxa-min-gain needs --tree-taxa FILE");
    a.tree_taxa_ids = check_taxon_list_output(a, "--tree-taxa");
    if (a.tree_taxa.empty()) return;
    const size_t n = flatten_reference(read_reference(a)).names.size();
    uint32_t plan[7];
    if (qs_tree_taxa_plan((uint32_t)n, plan) != QS_OK)
        throw std::runtime_error("--tree-taxa: the reference tree " + a.ref + " has " + std::to_string(n) + " taxa, the device plan supports at most " + std::to_string(plan[6]));
}

// --place-clades: beyond check_output, refused where a line of --place-clades-only names a label the -r tree lacks, the whole tree, a
// clade with fewer than three taxa outside it or a clade an earlier line names; leaves the nodes to place in a.place_nodes
inline void check_place_clades(Args &a) {
    if (!check_output(a, "--place-clades")) return;
    Tree primary = read_reference(a);
    const RefFlat rf = flatten_reference(primary);
    const RefShape S(rf);
    S.need_preorder("--place-clades");
    const size_t n = rf.names.size(), N = rf.parent.size();
    if (a.place_clades_only.empty()) {
        for (size_t v = 0; v < N; ++v)
            if (v != S.root && !S.kids[v].empty() && n - S.below(v) >= 3) a.place_nodes.push_back((uint32_t)v);
        if (a.place_nodes.empty()) throw std::runtime_error("--place-clades: the reference tree " + a.ref + " has no inner clade with at least three taxa outside it");
        return;
    }
    std::map<uint32_t, size_t> line_of;
    std::istringstream lines(slurp(a.place_clades_only));
    size_t line_no = 0;
    for (std::string line; std::getline(lines, line);) {
        ++line_no;
        const std::string what = "--place-clades-only " + a.place_clades_only + " line " + std::to_string(line_no) + ": ";
        if (line.find_first_not_of(" \t\r") == std::string::npos) continue;
        size_t first = n, last = 0;
        std::istringstream fields(line);
        for (std::string field; std::getline(fields, field, '\t');) {
            const size_t b = field.find_first_not_of(" \r"), e = field.find_last_not_of(" \r");
            if (b == std::string::npos) continue;
            const std::string name = field.substr(b, e - b + 1);
            const auto it = rf.name_to_id.find(name);
            if (it == rf.name_to_id.end()) throw std::runtime_error(what + "the taxon " + name + " is not in the reference tree " + a.ref);
            first = std::min<size_t>(first, it->second); last = std::max<size_t>(last, it->second);
        }
        // the smallest subtree that holds all labels: from the first label's leaf upwards until the last label is below as well
        size_t v = rf.leaf_node[first];
        while (!(S.holds(v, first) && S.holds(v, last))) v = (size_t)rf.parent[v];
        if (v == S.root) throw std::runtime_error(what + "the smallest subtree that holds these labels is the whole reference tree");
        if (n - S.below(v) < 3) throw std::runtime_error(what + "the clade leaves fewer than three taxa outside it (" + std::to_string(n - S.below(v)) + ")");
        const auto ins = line_of.emplace((uint32_t)v, line_no);
        if (!ins.second) throw std::runtime_error(what + "the same clade as line " + std::to_string(ins.first->second));
        a.place_nodes.push_back((uint32_t)v);
    }
    if (a.place_nodes.empty()) throw std::runtime_error("--place-clades-only " + a.place_clades_only + ": the list of clades is empty");
}

// --test-groups: beyond check_output, every line of SPEC parses against the labels of -r, and qs_group_check accepts the patterns;
// leaves the hypotheses in a.group_names / a.group_labels / a.group_kind
inline void check_test_groups(Args &a) {
    if (!check_output(a, "--test-groups")) return;
    Tree primary = read_reference(a);
    const RefFlat rf = flatten_reference(primary);
    const size_t n = rf.names.size();
    auto trimmed = [](const std::string &t) {
        const size_t b = t.find_first_not_of(" \r"), e = t.find_last_not_of(" \r");
        return b == std::string::npos ? std::string() : t.substr(b, e - b + 1);
    };
    std::istringstream lines(slurp(a.test_groups_spec));
    size_t line_no = 0;
    for (std::string line; std::getline(lines, line);) {
        ++line_no;
        const std::string what = "--test-groups " + a.test_groups_spec + " line " + std::to_string(line_no) + ": ";
        const size_t first = line.find_first_not_of(" \t\r");
        if (first == std::string::npos || line[first] == '#') continue;
        if (!line.empty() && line.back() == '\r') line.pop_back();
        std::vector<std::string> cols;
        for (size_t at = 0;;) {
            const size_t tab = line.find('\t', at);
            cols.push_back(line.substr(at, tab == std::string::npos ? std::string::npos : tab - at));
            if (tab == std::string::npos) break;
            at = tab + 1;
        }
        if (cols.size() != 3 && cols.size() != 5)
            throw std::runtime_error(what + "a hypothesis needs a name and two or four groups, found " + std::to_string(cols.size() - 1) + " group(s)");
        std::vector<uint8_t> row(n, 0);
        size_t star = 0, stars = 0;
        for (size_t k = 1; k < cols.size(); ++k)
            if (trimmed(cols[k]) == "*") { star = k; ++stars; }
        if (stars && (cols.size() != 3 || stars > 1)) throw std::runtime_error(what + "'*' may stand for one group of a split only");
        for (size_t k = 1; k < cols.size(); ++k) {
            if (k == star) continue;
            if (trimmed(cols[k]).empty()) throw std::runtime_error(what + "group " + std::to_string(k) + " is empty");
            std::istringstream members(cols[k]);
            for (std::string member; std::getline(members, member, ',');) {
                const std::string name = trimmed(member);
                const auto it = rf.name_to_id.find(name);
                if (it == rf.name_to_id.end()) throw std::runtime_error(what + "unknown taxon '" + name + "' in group " + std::to_string(k) + " (not in the reference tree " + a.ref + ")");
                if (row[it->second]) throw std::runtime_error(what + "taxon '" + name + "' is in two groups (or twice in one)");
                row[it->second] = (uint8_t)k;
            }
        }
        if (star) for (uint8_t &l : row) if (!l) l = (uint8_t)star;
        if (cols.size() == 3)
            for (uint8_t k = 1; k <= 2; ++k) {
                const size_t members = (size_t)std::count(row.begin(), row.end(), k);
                if (members == 0) throw std::runtime_error(what + "group " + std::to_string(k) + " is empty");
                if (members < 2) throw std::runtime_error(what + "group " + std::to_string(k) + " of a split needs at least two taxa");
            }
        a.group_names.push_back(cols[0]);
        a.group_labels.insert(a.group_labels.end(), row.begin(), row.end());
    }
    if (a.group_names.empty()) throw std::runtime_error("--test-groups " + a.test_groups_spec + ": no hypothesis in the file");
    a.group_kind.assign(a.group_names.size(), 0);
    if (qs_group_check((uint32_t)n, a.group_labels.data(), (uint32_t)a.group_names.size(), a.group_kind.data(), nullptr) != QS_OK)
        throw std::runtime_error("--test-groups " + a.test_groups_spec + ": " + qs_last_error(nullptr));
}

} // namespace qsh
