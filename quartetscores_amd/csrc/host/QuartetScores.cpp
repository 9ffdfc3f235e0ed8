// QuartetScores.cpp -- command-line driver of the MI355X engine; keeps the reference's CLI surface
// (QuartetScores.cpp:48-79: -r -e -o required, -q -t -v -s optional) and stdout protocol.
//
//   QuartetScores -r ref.nwk -e eval.nwk -o out.nwk [-q raw.txt] [-t N] [-v] [-s]
//                 [--device N] [--algo gather|scatter] [--exact-qp] [--qic-binary raw.bin]
//
// -t sets the number of host threads that parse + flatten the evaluation trees (the reference's OpenMP
// threads counted quartets; here that happens on the GPU). -s/--savemem does not change the table: the GPU table
// is always the compact C(n,4)x3 layout with semantic (1x) counts. It selects the reference's compact-table lookups
// where those differ observably: with a ROOTED reference tree the reference's table throws (quartet_lookup_table.hpp:79-85)
// and the run ends with that error, here as there (QS_SCORE_SAVEMEM_LOOKUPS).
// --save-table / --load-table write / read the raw count table (resume without recounting).
// --also-ref REF OUT (repeatable) scores further reference trees over the same taxa from the same count table: the table is
// re-indexed into REF's lookup-id order (qs_table_remap) instead of being counted again.
// --without-taxa NAMES OUT (repeatable) scores the -r tree without the taxa listed in NAMES from the same count table: the tree is
// pruned (newick.hpp prune) and the table cut down to the kept taxa (qs_table_restrict) instead of pruning every tree and recounting.
// --place-taxa FILE [--place-only NAMES] writes where the evaluation trees would put every (listed) taxon of the -r tree: the quartet
// score of each edge as a position of the taxon, from the same count table (qs_taxon_placement, qs_placement_scores).
// --place-clades FILE [--place-clades-only SPEC] does the same for whole clades of the -r tree, pruned and regrafted unchanged inside
// (qs_clade_placement, qs_placement_scores).
// --test-groups SPEC FILE writes how often the evaluation trees show each of the three resolutions around branches the user names as
// taxon groups -- four groups S1 S2 | S3 S4 or a bipartition S1 | S2 --, whether or not the -r tree has them, from the same count
// table (qs_group_check, qs_group_support).
// --taxon-pairs FILE [--taxon-pairs-only NAMES] writes, per pair of taxa of the -r tree, how often the evaluation trees put the two
// together against the other two taxa of a 4-set, beside what the -r tree shows for the same 4-sets (qs_taxon_pair_support).
// --drop-one FILE [--drop-one-only NAMES] writes, per taxon and internode of the -r tree, the internode's QP-IC without that taxon, from
// the same count table (qs_branch_taxon_support).
#include "QuartetScoreComputer.hpp"
#include "multi_gpu.hpp"
#include "table_shards.hpp"
#include "synth.hpp"
#include "tree_distances.hpp"
#include "local_pp.hpp"

#include <algorithm>
#include <cerrno>
#include <cmath>
#include <map>
#include <set>
#include <sstream>
#include <cstdlib>
#include <unistd.h>
#include <chrono>
#include <cstring>
#include <fstream>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

using namespace qsh;

namespace {

bool fast_exit_forced = false;
// true when something in the environment says "a tool rides along that flushes at exit"
bool wrapped_by_tool() {
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
    size_t threads = 0;
    bool verbose = false, savemem = false, raw_rank_order = false, fail_fast = false, clean_exit = false;
    int table_shards = -1;   // -1 = off (the whole table on the device); 0 = as many as the device's free memory asks for; K = K shards, one after the other (table_shards.hpp)
    int spill = 0;           // ShardedTableQuartetScoreComputer::Spill
    int gpus = 0;   // 0 = the single-GPU path; N >= 1 = N GPUs of this node: tree-sharded + one table collective (multi_gpu.hpp) or table-sharded (table_shards.hpp)
    std::string mode = "auto";   // --mode with --gpus N: tree | table | auto (the model of table_shards.hpp prefer_table_shards)
    DeviceOptions dev;
};

void usage(std::ostream &os) {
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
          "   --local-pp-lambda L  with --local-pp: the rate of the prior on branch lengths, L > 0 (default 0.5)\n";
}

// returns 0 ok, 1 error (message printed like the reference prints TCLAP::ArgException), 2 exit quietly
int parse(int argc, char **argv, Args &a) {
    auto need = [&](int &i, const char *flag) -> const char * {
        if (i + 1 >= argc) {
            std::cerr << "ERROR: Missing a value for this argument! for arg " << flag << std::endl;
            return nullptr;
        }
        return argv[++i];
    };
    // numeric flag values: a malformed one is reported like the other argument errors (tclap: "Couldn't read argument
    // value from string"), not an uncaught std::invalid_argument
    auto number = [&](const char *text, const char *flag, unsigned long &out) {
        char *end = nullptr;
        errno = 0;
        const unsigned long val = std::strtoul(text, &end, 10);
        if (end == text || *end != '\0' || errno != 0 || text[0] == '-') {
            std::cerr << "ERROR: Couldn't read argument value from string '" << text << "' for arg " << flag << std::endl;
            return false;
        }
        out = val;
        return true;
    };
    unsigned long num = 0;
    for (int i = 1; i < argc; ++i) {
        std::string f = argv[i];
        const char *v = nullptr;
        if (f == "-r" || f == "--ref") { if (!(v = need(i, "-r (--ref)"))) return 1; a.ref = v; }
        else if (f == "-e" || f == "--eval") { if (!(v = need(i, "-e (--eval)"))) return 1; a.eval = v; }
        else if (f == "-o" || f == "--output") { if (!(v = need(i, "-o (--output)"))) return 1; a.out = v; }
        else if (f == "-q" || f == "--qic") { if (!(v = need(i, "-q (--qic)"))) return 1; a.raw = v; }
        else if (f == "-t" || f == "--threads") { if (!(v = need(i, "-t (--threads)")) || !number(v, "-t (--threads)", num)) return 1; a.threads = num; }
        else if (f == "-v" || f == "--verbose") a.verbose = true;
        else if (f == "-s" || f == "--savemem") a.savemem = true;
        else if (f == "--gpus") { if (!(v = need(i, "--gpus")) || !number(v, "--gpus", num)) return 1; a.gpus = (int)num; }
        else if (f == "--table-shards") { if (!(v = need(i, "--table-shards")) || !number(v, "--table-shards", num)) return 1; a.table_shards = (int)num; }
        else if (f == "--spill") {
            if (!(v = need(i, "--spill"))) return 1;
            const std::string sv = v;
            if (sv == "host") a.spill = ShardedTableQuartetScoreComputer::SPILL_HOST;
            else if (sv == "recount") a.spill = ShardedTableQuartetScoreComputer::SPILL_RECOUNT;
            else if (sv == "auto") a.spill = ShardedTableQuartetScoreComputer::SPILL_AUTO;
            else { std::cerr << "ERROR: --spill takes host, recount or auto" << std::endl; return 1; }
        }
        else if (f == "--device") { if (!(v = need(i, "--device")) || !number(v, "--device", num)) return 1; a.dev.device = (int)num; }
        else if (f == "--algo") {
            if (!(v = need(i, "--algo"))) return 1;
            a.dev.algo = std::string(v) == "scatter" ? QS_ALGO_SCATTER : QS_ALGO_GATHER;
        } else if (f == "--exact-qp") a.dev.qp_exact64 = true;
        else if (f == "--root-as-edge") a.dev.root_as_edge = true;
        else if (f == "--mode") {
            if (!(v = need(i, "--mode"))) return 1;
            a.mode = v;
            if (a.mode != "auto" && a.mode != "tree" && a.mode != "table") { std::cerr << "ERROR: --mode takes auto, tree or table" << std::endl; return 1; }
        }
        else if (f == "--fail-fast") a.fail_fast = true;
        else if (f == "--clean-exit") a.clean_exit = true;
        else if (f == "--fast-exit") fast_exit_forced = true;
        else if (f == "--reduce") {
            if (!(v = need(i, "--reduce"))) return 1;
            a.dev.reduce = v;
            if (a.dev.reduce != "rccl" && a.dev.reduce != "p2p") { std::cerr << "ERROR: --reduce takes rccl or p2p" << std::endl; return 1; }
        }
        else if (f == "--gpus-on-one-device") a.dev.gpus_on_one_device = true;
        else if (f == "--comm-overlap") { if (!(v = need(i, "--comm-overlap")) || !number(v, "--comm-overlap", num)) return 1; a.dev.comm_overlap = num != 0; }
        else if (f == "--trace") a.dev.trace = true;
        else if (f == "--qic-rank-order") a.raw_rank_order = true;
        else if (f == "--save-table") { if (!(v = need(i, "--save-table"))) return 1; a.dev.save_table = v; }
        else if (f == "--qic-binary") { if (!(v = need(i, "--qic-binary"))) return 1; a.raw_bin = v; }
        else if (f == "--per-tree") { if (!(v = need(i, "--per-tree"))) return 1; a.per_tree = v; }
        else if (f == "--tree-distances") { if (!(v = need(i, "--tree-distances"))) return 1; a.tree_distances = v; }
        else if (f == "--per-taxon") { if (!(v = need(i, "--per-taxon"))) return 1; a.per_taxon = v; }
        else if (f == "--place-taxa") { if (!(v = need(i, "--place-taxa"))) return 1; a.place_taxa = v; }
        else if (f == "--taxon-pairs") { if (!(v = need(i, "--taxon-pairs"))) return 1; a.taxon_pairs = v; }
        else if (f == "--taxon-pairs-only") { if (!(v = need(i, "--taxon-pairs-only"))) return 1; a.taxon_pairs_only = v; }
        else if (f == "--drop-one") { if (!(v = need(i, "--drop-one"))) return 1; a.drop_one = v; }
        else if (f == "--drop-one-only") { if (!(v = need(i, "--drop-one-only"))) return 1; a.drop_one_only = v; }
        else if (f == "--branch-trees") { if (!(v = need(i, "--branch-trees"))) return 1; a.branch_trees = v; }
        else if (f == "--bootstrap") { if (!(v = need(i, "--bootstrap"))) return 1; a.bootstrap = v; }
        else if (f == "--bootstrap-reps") { if (!(v = need(i, "--bootstrap-reps")) || !number(v, "--bootstrap-reps", num)) return 1; a.bootstrap_reps = (uint32_t)std::min<unsigned long>(num, 0xFFFFFFFFul); a.bootstrap_reps_given = true; }
        else if (f == "--bootstrap-seed") { if (!(v = need(i, "--bootstrap-seed")) || !number(v, "--bootstrap-seed", num)) return 1; a.bootstrap_seed = num; a.bootstrap_seed_given = true; }
        else if (f == "--local-pp") { if (!(v = need(i, "--local-pp"))) return 1; a.local_pp = v; }
        else if (f == "--local-pp-lambda") {
            if (!(v = need(i, "--local-pp-lambda"))) return 1;
            char *end = nullptr;
            a.local_pp_lambda = std::strtod(v, &end);
            if (end == v || *end != '\0' || !std::isfinite(a.local_pp_lambda) || !(a.local_pp_lambda > 0.0)) {
                std::cerr << "ERROR: Couldn't read argument value from string '" << v << "' for arg --local-pp-lambda (a positive number)" << std::endl;
                return 1;
            }
            a.local_pp_lambda_given = true;
        }
        else if (f == "--place-only") { if (!(v = need(i, "--place-only"))) return 1; a.place_only = v; }
        else if (f == "--place-clades") { if (!(v = need(i, "--place-clades"))) return 1; a.place_clades = v; }
        else if (f == "--place-clades-only") { if (!(v = need(i, "--place-clades-only"))) return 1; a.place_clades_only = v; }
        else if (f == "--test-groups") {
            if (i + 2 >= argc) {
                std::cerr << "ERROR: Missing a value for this argument! for arg --test-groups (it takes two: SPEC FILE)" << std::endl;
                return 1;
            }
            a.test_groups_spec = argv[++i];
            a.test_groups = argv[++i];
        }
        else if (f == "--load-table") { if (!(v = need(i, "--load-table"))) return 1; a.dev.load_table = v; }
        else if (f == "--also-ref") {
            if (i + 2 >= argc || argv[i + 2][0] == '-') {
                std::cerr << "ERROR: Missing a value for this argument! for arg --also-ref (it takes two: REF OUT)" << std::endl;
                return 1;
            }
            AlsoRef x;
            x.ref = argv[++i];
            x.out = argv[++i];
            a.also.push_back(std::move(x));
        }
        else if (f == "--without-taxa") {
            if (i + 2 >= argc || argv[i + 2][0] == '-') {
                std::cerr << "ERROR: Missing a value for this argument! for arg --without-taxa (it takes two: NAMES OUT)" << std::endl;
                return 1;
            }
            WithoutTaxa x;
            x.names = argv[++i];
            x.out = argv[++i];
            a.without.push_back(std::move(x));
        }
        else if (f == "--version") { std::cout << argv[0] << "  version: 1.0.1 (" << qs_version() << ")" << std::endl; return 2; }
        else if (f == "-h" || f == "--help") { usage(std::cout); return 2; }
        else { std::cerr << "ERROR: Couldn't find match for argument for arg " << f << std::endl; return 1; }
    }
    const char *missing = a.ref.empty() ? "-r (--ref)" : a.eval.empty() ? "-e (--eval)" : a.out.empty() ? "-o (--output)" : nullptr;
    if (missing) { std::cerr << "ERROR: Required argument missing: for arg " << missing << std::endl; return 1; }
    // A wrapper that flushes in its exit handlers (rocprofv3, a tracer, a coverage or sanitizer runtime) would lose its output to the
    // fast exit: with a preloaded library or a profiler's environment the ordinary return is the default (--fast-exit overrides)
    if (!a.clean_exit && !fast_exit_forced && wrapped_by_tool()) a.clean_exit = true;
    return 0;
}

// annotated Newick: per edge "qp-ic:X;lq-ic:Y;eqp-ic:Z" via std::to_string, parts omitted when +inf;
// the qp-ic guard tests the LQ value like the reference (quartet_newick_writer.hpp:164-187, quirk Q6)
void write_annotated(const Tree &tree, const std::string &path, const std::vector<double> &lqic, const std::vector<double> &qpic,
                     const std::vector<double> &eqpic) {
    const double inf = std::numeric_limits<double>::infinity();
    auto comment = [&](size_t v) -> std::string {
        if (v == 0) return std::string();
        const size_t e = v - 1;
        std::string s;
        auto add = [&](const std::string &part) { if (!s.empty()) s += ";"; s += part; };
        if (!qpic.empty() && lqic[e] != inf) add("qp-ic:" + std::to_string(qpic[e]));
        if (lqic[e] != inf) add("lq-ic:" + std::to_string(lqic[e]));
        if (!eqpic.empty() && eqpic[e] != inf) add("eqp-ic:" + std::to_string(eqpic[e]));
        return s;
    };
    std::ofstream out(path);
    if (!out) throw std::runtime_error("cannot write " + path);
    out << write_newick(tree, comment) << "\n";
}

std::set<std::string> read_taxon_names(const std::string &path, const RefFlat &rf, const std::string &ref_path, const std::string &what);

// the -r tree
Tree read_reference(const Args &a) {
    Tree primary;
    const std::string text = slurp(a.ref);
    NewickReader rr(text);
    if (!rr.next(primary)) throw std::runtime_error("empty reference tree file");
    return primary;
}

// Every output file of the command line with the option that names it; an option that was not given has an empty path
std::vector<std::pair<std::string, std::string>> output_files(const Args &a) {
    std::vector<std::pair<std::string, std::string>> files{
        {"-o", a.out}, {"-q", a.raw}, {"--qic-binary", a.raw_bin}, {"--save-table", a.dev.save_table}, {"--per-tree", a.per_tree},
        {"--tree-distances", a.tree_distances}, {"--per-taxon", a.per_taxon}, {"--place-taxa", a.place_taxa}, {"--place-clades", a.place_clades},
        {"--test-groups", a.test_groups}, {"--taxon-pairs", a.taxon_pairs}, {"--drop-one", a.drop_one}, {"--branch-trees", a.branch_trees},
        {"--bootstrap", a.bootstrap}, {"--local-pp", a.local_pp}};
    for (const AlsoRef &x : a.also) files.emplace_back("--also-ref", x.out);
    for (const WithoutTaxa &x : a.without) files.emplace_back("--without-taxa", x.out);
    return files;
}

std::string output_file(const Args &a, const std::string &flag) {
    for (const auto &e : output_files(a))
        if (e.first == flag) return e.second;
    return "";
}

// The FILE of `flag` (given): refused where another output of the command line goes to the same path, and where it exists
void check_output_file(const Args &a, const std::string &flag) {
    const std::string path = output_file(a, flag);
    for (const auto &e : output_files(a))
        if (e.first != flag && e.second == path) throw std::runtime_error(flag + ": " + path + " is also another output file");
    if (std::ifstream(path).good()) throw std::runtime_error(flag + ": the output file " + path + " already exists");
}

// --X FILE [--X-only NAMES], an output per listed taxon of -r (--place-taxa, --taxon-pairs, --drop-one): refused before the device is
// touched where the whole table is not on one GPU, where FILE exists or is another output, and where NAMES holds a label the -r tree
// lacks; returns the lookup ids to compute, ascending (all without NAMES; none without FILE)
std::vector<uint16_t> check_taxon_list_output(const Args &a, const std::string &flag, const std::string &only_flag, const std::string &only) {
    if (output_file(a, flag).empty()) {
        if (!only.empty()) throw std::runtime_error(only_flag + " needs " + flag + " FILE");
        return {};
    }
    if (a.gpus > 0 || a.table_shards >= 0) throw std::runtime_error(flag + " needs the whole count table on one GPU: omit --gpus / --table-shards");
    check_output_file(a, flag);
    const RefFlat rf = flatten_reference(read_reference(a));
    std::set<uint16_t> ids;
    if (only.empty()) {
        for (size_t i = 0; i < rf.names.size(); ++i) ids.insert((uint16_t)i);
    } else {
        for (const std::string &name : read_taxon_names(only, rf, a.ref, only_flag + " " + only + ": ")) ids.insert((uint16_t)rf.name_to_id.at(name));
    }
    return std::vector<uint16_t>(ids.begin(), ids.end());
}

// --also-ref: everything that needs no GPU, before the device is touched -- the files parse, every tree holds exactly the
// taxa of -r, no OUT exists or repeats -o or another OUT, and qs_score_check passes for every tree with the run's flags
void check_also_refs(Args &a) {
    if (a.also.empty()) return;
    if (a.gpus > 0 || a.table_shards >= 0)
        throw std::runtime_error("--also-ref works on one GPU with the whole table: omit --gpus / --table-shards");
    Tree primary = read_reference(a);
    const RefFlat rf = flatten_reference(primary);
    const std::set<std::string> names(rf.names.begin(), rf.names.end());
    std::set<std::string> outs{a.out};
    for (AlsoRef &x : a.also) {
        if (!outs.insert(x.out).second) throw std::runtime_error("--also-ref " + x.ref + ": the output file " + x.out + " is given twice");
        if (std::ifstream(x.out).good()) throw std::runtime_error("--also-ref " + x.ref + ": the output file " + x.out + " already exists");
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

// A NAMES file (--without-taxa, --place-only): one label per line, as parsed and unquoted; surrounding blanks go, blank lines are skipped,
// a repeated label counts once. Returns the labels; `what` prefixes the message for a label the -r tree lacks.
std::set<std::string> read_taxon_names(const std::string &path, const RefFlat &rf, const std::string &ref_path, const std::string &what) {
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

// --without-taxa: everything that needs no GPU, before the device is touched -- every name is a taxon of -r, at least one is dropped
// and four are kept, no OUT exists or repeats another output, and qs_score_check passes for every pruned tree with the run's flags
void check_without_taxa(Args &a) {
    if (a.without.empty()) return;
    if (a.gpus > 0 || a.table_shards >= 0)
        throw std::runtime_error("--without-taxa works on one GPU with the whole table: omit --gpus / --table-shards");
    Tree primary = read_reference(a);
    const RefFlat rf = flatten_reference(primary);
    std::set<std::string> outs{a.out, a.raw, a.raw_bin, a.dev.save_table, a.per_tree, a.per_taxon};
    for (const AlsoRef &x : a.also) outs.insert(x.out);
    for (WithoutTaxa &x : a.without) {
        const std::string what = "--without-taxa " + x.names + ": ";
        if (!outs.insert(x.out).second) throw std::runtime_error(what + "the output file " + x.out + " is given twice");
        if (std::ifstream(x.out).good()) throw std::runtime_error(what + "the output file " + x.out + " already exists");
        x.drop = read_taxon_names(x.names, rf, a.ref, what);
        if (rf.names.size() < x.drop.size() + 4)
            throw std::runtime_error(what + "fewer than four taxa are left (" + std::to_string(rf.names.size() - x.drop.size()) + " of " + std::to_string(rf.names.size()) + ")");
        prune(primary, x.drop, x.tree);
        const RefFlat fx = flatten_reference(x.tree);
        const qs_ref_tree rt = ref_view(fx);
        if (qs_score_check(nullptr, &rt, score_flags(a.dev)) != QS_OK) throw std::runtime_error(what + qs_last_error(nullptr));
    }
}

// --per-tree: refused before the device is touched where no trees are counted on one GPU, and where FILE exists or is another output
void check_per_tree(const Args &a) {
    if (a.per_tree.empty()) return;
    if (a.gpus > 0 || a.table_shards >= 0 || !a.dev.load_table.empty())
        throw std::runtime_error("--per-tree needs the evaluation trees counted on one GPU: omit --gpus / --table-shards / --load-table");
    check_output_file(a, "--per-tree");
}

// --tree-distances: refused like --per-tree, before the device is touched
void check_tree_distances(const Args &a) {
    if (a.tree_distances.empty()) return;
    if (a.gpus > 0 || a.table_shards >= 0 || !a.dev.load_table.empty())
        throw std::runtime_error("--tree-distances needs the evaluation trees counted on one GPU: omit --gpus / --table-shards / --load-table");
    check_output_file(a, "--tree-distances");
}

// --per-tree: qs_tree_agreement behind every batch's count into one device buffer of 4 x m words, downloaded once after the last
// qs_sync; taxa per tree from the flattened batches
struct PerTree {
    size_t m = 0;
    int device = 0;
    qs::DevBuf<uint64_t> dev;
    std::vector<uint64_t> counts;
    std::vector<uint32_t> taxa;
    void hook(DeviceOptions &opt, const RefFlat &ref) {
        taxa.assign(m, 0);
        add_after_count(opt, [this, &ref](qs_ctx *ctx, const qs_device_batch *db, size_t i0, const BatchFlat &b) {
            if (!dev) {
                if (hipSetDevice(device) != hipSuccess || dev.reserve(std::max<size_t>(1, 4 * m) * 8, nullptr) != hipSuccess)
                    throw std::runtime_error("--per-tree: Insufficient memory!");
            }
            for (uint32_t t = 0; t < b.n_trees; ++t) taxa[i0 + t] = b.leaf_off[t + 1] - b.leaf_off[t];
            const qs_ref_tree rt = ref_view(ref);
            if (qs_tree_agreement(ctx, &rt, db, dev.get() + 4 * i0) != QS_OK) throw std::runtime_error(qs_last_error(ctx));
        });
        add_after_sync(opt, [this](qs_ctx *) {
            counts.assign(4 * m, 0);
            if (m && hipMemcpy(counts.data(), dev.get(), 4 * m * 8, hipMemcpyDeviceToHost) != hipSuccess)
                throw std::runtime_error("--per-tree: download failed");
        });
    }
    void write(const std::string &path) const {
        std::ofstream f(path);
        if (!f) throw std::runtime_error("cannot write " + path);
        f << "tree\ttaxa\tquartets\tconcordant\tdiscordant\teval_only\tref_only\tunresolved\tconcordance\n";
        char conc[64];
        for (size_t t = 0; t < m; ++t) {
            const uint64_t n = taxa[t], c = counts[4 * t], d = counts[4 * t + 1], re = counts[4 * t + 2], rr = counts[4 * t + 3];
            const uint64_t q = c4(n);
            const uint64_t eo = re - c - d, ro = rr - c - d;
            if (c + d) std::snprintf(conc, sizeof conc, "%.6f", (double)c / (double)(c + d));
            else std::snprintf(conc, sizeof conc, "nan");
            f << t << '\t' << n << '\t' << q << '\t' << c << '\t' << d << '\t' << eo << '\t' << ro << '\t' << (q - c - d - eo - ro) << '\t' << conc << '\n';
        }
        if (!f) throw std::runtime_error("cannot write " + path);
    }
};

// --per-taxon: refused before the device is touched where the whole table is not on one GPU, and where FILE exists or is another output
void check_per_taxon(const Args &a) {
    if (a.per_taxon.empty()) return;
    if (a.gpus > 0 || a.table_shards >= 0)
        throw std::runtime_error("--per-taxon needs the whole count table on one GPU: omit --gpus / --table-shards");
    check_output_file(a, "--per-taxon");
}

// --per-taxon: one qs_taxon_support over the counted (or loaded) table, 6 x n words downloaded, one TSV line per taxon
void write_per_taxon(qs_ctx *ctx, const RefFlat &ref, int device, const std::string &path) {
    const size_t n = ref.names.size();
    const qs_ref_tree rt = ref_view(ref);
    qs::DevBuf<int64_t> dev;
    if (hipSetDevice(device) != hipSuccess || dev.reserve(6 * n * 8, nullptr) != hipSuccess) throw std::runtime_error("--per-taxon: Insufficient memory!");
    if (qs_taxon_support(ctx, &rt, dev.get()) != QS_OK || qs_sync(ctx) != QS_OK) throw std::runtime_error(std::string("--per-taxon: ") + qs_last_error(ctx));
    std::vector<int64_t> w(6 * n);
    if (hipMemcpy(w.data(), dev.get(), 6 * n * 8, hipMemcpyDeviceToHost) != hipSuccess) throw std::runtime_error("--per-taxon: download failed");
    int64_t conc = 0, disc = 0;   // of the whole table: every quartet is in four taxa's sums
    for (size_t x = 0; x < n; ++x) { conc += w[6 * x + 1]; disc += w[6 * x + 2]; }
    conc /= 4; disc /= 4;
    std::ofstream f(path);
    if (!f) throw std::runtime_error("cannot write " + path);
    f << "taxon\tname\tquartets\tref_resolved\tconcordant\tdiscordant\teval_only\toutvoted\tuninformed\tconcordance\tconcordance_without\n";
    const uint64_t quartets = n < 4 ? 0 : (uint64_t)(n - 1) * (n - 2) * (n - 3) / 6;
    auto ratio = [](int64_t c, int64_t d, char (&buf)[64]) {
        if (c + d) std::snprintf(buf, sizeof buf, "%.6f", (double)c / (double)(c + d));
        else std::snprintf(buf, sizeof buf, "nan");
    };
    char own[64], without[64];
    for (size_t x = 0; x < n; ++x) {
        const int64_t *v = &w[6 * x];
        ratio(v[1], v[2], own);
        ratio(conc - v[1], disc - v[2], without);
        f << x << '\t' << ref.names[x] << '\t' << quartets;
        for (int k = 0; k < 6; ++k) f << '\t' << v[k];
        f << '\t' << own << '\t' << without << '\n';
    }
    if (!f) throw std::runtime_error("cannot write " + path);
}

// The shape of a flattened reference tree that the placement outputs need: nodes are numbered in preorder (parents first)
struct PlaceShape {
    size_t root = 0;
    std::vector<uint32_t> depth, links;
    std::vector<int64_t> lo, hi;   // the lookup ids below a node: [lo, hi)
    PlaceShape(const RefFlat &ref, const char *flag) {
        const size_t n = ref.names.size(), N = ref.parent.size();
        depth.assign(N, 0); links.assign(N, 0); lo.assign(N, (int64_t)n); hi.assign(N, 0);
        for (size_t v = 0; v < N; ++v) {
            const int32_t p = ref.parent[v];
            if (p < 0) { root = v; continue; }
            if ((size_t)p >= v) throw std::runtime_error(std::string(flag) + ": the reference tree is not numbered in preorder");
            depth[v] = depth[p] + 1; links[v] += 1; links[p] += 1;
        }
        for (size_t i = 0; i < n; ++i) { lo[ref.leaf_node[i]] = (int64_t)i; hi[ref.leaf_node[i]] = (int64_t)i + 1; }
        for (size_t v = N; v-- > 0;)
            if (ref.parent[v] >= 0) { const size_t p = (size_t)ref.parent[v]; lo[p] = std::min(lo[p], lo[v]); hi[p] = std::max(hi[p], hi[v]); }
    }
};

// --place-taxa: one qs_taxon_placement over the counted (or loaded) table for the listed taxa, their link sums downloaded, per taxon
// qs_placement_scores and the columns (tests/placement_model.py defines them): a position = the edges that induce the same
// bipartition of the other taxa
void write_place_taxa(qs_ctx *ctx, const RefFlat &ref, int device, const std::string &path, const std::vector<uint16_t> &ids) {
    const size_t n = ref.names.size(), N = ref.parent.size(), L = ids.size();
    const qs_ref_tree rt = ref_view(ref);
    qs::DevBuf<int64_t> dev;
    if (hipSetDevice(device) != hipSuccess || dev.reserve(L * 2 * N * 8, nullptr) != hipSuccess) throw std::runtime_error("--place-taxa: Insufficient memory!");
    if (qs_taxon_placement(ctx, &rt, ids.data(), (uint32_t)L, dev.get()) != QS_OK || qs_sync(ctx) != QS_OK)
        throw std::runtime_error(std::string("--place-taxa: ") + qs_last_error(ctx));
    std::vector<int64_t> w(L * 2 * N);
    if (hipMemcpy(w.data(), dev.get(), w.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) throw std::runtime_error("--place-taxa: download failed");
    const PlaceShape S(ref, "--place-taxa");
    const size_t root = S.root;
    const std::vector<uint32_t> &depth = S.depth, &links = S.links;
    const std::vector<int64_t> &lo = S.lo, &hi = S.hi;
    auto walk = [&](size_t a, size_t b) {   // nodes on the path from a to b, both inclusive
        std::vector<size_t> left{a}, right{b};
        while (left.back() != right.back()) {
            if (depth[left.back()] >= depth[right.back()]) left.push_back((size_t)ref.parent[left.back()]);
            else right.push_back((size_t)ref.parent[right.back()]);
        }
        left.insert(left.end(), right.rbegin() + 1, right.rend());
        return left;
    };
    std::ofstream f(path);
    if (!f) throw std::runtime_error("cannot write " + path);
    f << "taxon\tname\tcurrent\tbest\tgain\tn_best\tbest_node\tbest_lo\tbest_hi\tdistance\n";
    std::vector<int64_t> score(N), key(N);
    for (size_t k = 0; k < L; ++k) {
        const int64_t x = ids[k];
        if (qs_placement_scores(&rt, &w[k * 2 * N], score.data()) != QS_OK) throw std::runtime_error(std::string("--place-taxa: ") + qs_last_error(nullptr));
        // the position of the edge above v: the id interval, in the others' numbering, of the side without the smallest other taxon
        for (size_t v = 0; v < N; ++v) {
            int64_t a = lo[v] - (lo[v] > x), b = hi[v] - (hi[v] > x);
            if (a == 0 && b > 0) { a = b; b = (int64_t)n - 1; }
            key[v] = b > a ? a * (int64_t)n + b : 0;
        }
        const size_t own = ref.leaf_node[x], u = (size_t)ref.parent[own];
        if (links[u] == 3)   // the taxon's pendant edge and the two other edges at its parent are one position
            for (size_t v = 0; v < N; ++v) if (v != own && ref.parent[v] == (int32_t)u) { key[own] = key[v]; break; }
        int64_t best = INT64_MIN;
        for (size_t v = 0; v < N; ++v) if (v != root) best = std::max(best, score[v]);
        std::set<int64_t> top;
        int64_t first_top = -1;
        for (size_t v = 0; v < N; ++v) if (v != root && score[v] == best) { if (top.empty()) first_top = key[v]; top.insert(key[v]); }
        const int64_t current = score[own];
        const int64_t pick = current == best ? key[own] : first_top;
        size_t node = 0;
        for (size_t v = 0; v < N; ++v) if (v != root && key[v] == pick) { node = v; break; }
        size_t dist = 0;
        if (pick != key[own]) {
            const std::vector<size_t> to_child = walk(u, node), to_parent = walk(u, (size_t)ref.parent[node]);
            for (size_t v : to_parent.size() < to_child.size() ? to_parent : to_child) dist += links[v] - (v == u) >= 3;
        }
        f << x << '\t' << ref.names[x] << '\t' << current << '\t' << best << '\t' << (best - current) << '\t' << top.size() << '\t' << node << '\t'
          << lo[node] << '\t' << hi[node] << '\t' << dist << '\n';
    }
    if (!f) throw std::runtime_error("cannot write " + path);
}

// --taxon-pairs: one qs_taxon_pair_support over the counted (or loaded) table for the listed taxa, their rows of n x 8 words downloaded,
// one TSV line per pair a < b with a listed taxon (tests/taxon_pair_model.py defines the columns; the matrix is symmetric: a pair's
// words come from the row of whichever of the two is listed)
void write_taxon_pairs(qs_ctx *ctx, const RefFlat &ref, int device, const std::string &path, const std::vector<uint16_t> &ids) {
    const size_t n = ref.names.size(), L = ids.size();
    const qs_ref_tree rt = ref_view(ref);
    qs::DevBuf<int64_t> dev;
    if (hipSetDevice(device) != hipSuccess || dev.reserve(L * n * 8 * 8, nullptr) != hipSuccess) throw std::runtime_error("--taxon-pairs: Insufficient memory!");
    if (qs_taxon_pair_support(ctx, &rt, ids.data(), (uint32_t)L, dev.get()) != QS_OK || qs_sync(ctx) != QS_OK)
        throw std::runtime_error(std::string("--taxon-pairs: ") + qs_last_error(ctx));
    std::vector<int64_t> w(L * n * 8);
    if (hipMemcpy(w.data(), dev.get(), w.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) throw std::runtime_error("--taxon-pairs: download failed");
    std::vector<int64_t> row_of(n, -1);
    for (size_t k = 0; k < L; ++k) row_of[ids[k]] = (int64_t)k;
    std::ofstream f(path);
    if (!f) throw std::runtime_error("cannot write " + path);
    f << "a\tb\tname_a\tname_b\tquartets\tref_together\tref_apart\ttogether\tapart\taffinity\tkept\tjoined\n";
    const uint64_t quartets = n < 4 ? 0 : (uint64_t)(n - 2) * (n - 3) / 2;
    auto ratio = [](int64_t num, int64_t den, char (&buf)[64]) {   // (as --per-taxon's concordance)
        if (den) std::snprintf(buf, sizeof buf, "%.6f", (double)num / (double)den);
        else std::snprintf(buf, sizeof buf, "nan");
    };
    char affinity[64], kept[64], joined[64];
    for (size_t a = 0; a < n; ++a)
        for (size_t b = a + 1; b < n; ++b) {
            if (row_of[a] < 0 && row_of[b] < 0) continue;
            const int64_t *v = row_of[a] >= 0 ? &w[((size_t)row_of[a] * n + b) * 8] : &w[((size_t)row_of[b] * n + a) * 8];
            ratio(v[6], v[7], affinity);
            ratio(v[2], v[3], kept);
            ratio(v[4], v[5], joined);
            f << a << '\t' << b << '\t' << ref.names[a] << '\t' << ref.names[b] << '\t' << quartets << '\t' << v[0] << '\t' << v[1] << '\t' << v[6] << '\t'
              << (v[7] - v[6]) << '\t' << affinity << '\t' << kept << '\t' << joined << '\n';
        }
    if (!f) throw std::runtime_error("cannot write " + path);
}

// The internodes of the -r tree as the per-branch outputs list them (tests/branch_taxon_model.py): the id interval below every node, its
// children in id order, and the edges (child node, other end) in node order -- the internode through a degree-2 root once, at the child
// that holds lookup id 0
struct Internodes {
    struct Edge { size_t v, w; bool through_root; };
    std::vector<size_t> lo, hi;
    std::vector<std::vector<size_t>> kids;
    std::vector<Edge> edges;
    explicit Internodes(const RefFlat &ref) {
        const size_t n = ref.names.size(), N = ref.parent.size();
        lo.assign(N, n); hi.assign(N, 0); kids.resize(N);
        for (size_t i = 0; i < n; ++i)
            for (int64_t v = ref.leaf_node[i]; v >= 0; v = ref.parent[(size_t)v]) { lo[(size_t)v] = std::min(lo[(size_t)v], i); hi[(size_t)v] = std::max(hi[(size_t)v], i + 1); }
        size_t root = 0;
        for (size_t v = 0; v < N; ++v) {
            if (ref.parent[v] >= 0) kids[(size_t)ref.parent[v]].push_back(v);
            else root = v;
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
};

// --drop-one: one qs_branch_taxon_support over the counted (or loaded) table for the listed taxa, their rows of n_nodes x 4 words and
// the totals downloaded, one TSV line per taxon and internode (tests/branch_taxon_model.py defines the columns; the internode through a
// degree-2 root once, at the child that holds lookup id 0)
void write_drop_one(qs_ctx *ctx, const RefFlat &ref, int device, const std::string &path, const std::vector<uint16_t> &ids) {
    const size_t n = ref.names.size(), N = ref.parent.size(), L = ids.size();
    const qs_ref_tree rt = ref_view(ref);
    qs::DevBuf<int64_t> dev;
    if (hipSetDevice(device) != hipSuccess || dev.reserve((L + 1) * N * 4 * 8, nullptr) != hipSuccess) throw std::runtime_error("--drop-one: Insufficient memory!");
    if (qs_branch_taxon_support(ctx, &rt, ids.data(), (uint32_t)L, dev.get(), dev.get() + L * N * 4) != QS_OK || qs_sync(ctx) != QS_OK)
        throw std::runtime_error(std::string("--drop-one: ") + qs_last_error(ctx));
    std::vector<int64_t> w((L + 1) * N * 4);
    if (hipMemcpy(w.data(), dev.get(), w.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) throw std::runtime_error("--drop-one: download failed");
    const int64_t *totals = w.data() + L * N * 4;
    const Internodes in(ref);
    const std::vector<size_t> &lo = in.lo, &hi = in.hi;
    const std::vector<std::vector<size_t>> &kids = in.kids;
    const std::vector<Internodes::Edge> &edges = in.edges;
    // taxa in x's link at the node `end`, whose link towards `away` (N = none) is the edge itself
    auto link_size = [&](size_t end, size_t x, size_t away) {
        for (size_t k : kids[end])
            if (k != away && lo[k] <= x && x < hi[k]) return hi[k] - lo[k];
        return n - (hi[end] - lo[end]);   // the parent's side
    };
    std::ofstream f(path);
    if (!f) throw std::runtime_error("cannot write " + path);
    f << "taxon\tname\tnode\tlo\thi\tgroup\tquartets\tq1\tq2\tq3\tqpic\tqpic_without\tdelta\n";
    char qpic[64], without[64], delta[64];
    for (size_t k = 0; k < L; ++k) {
        const size_t x = ids[k];
        for (const Internodes::Edge &e : edges) {
            const int64_t *r = &w[(k * N + e.v) * 4], *t = totals + e.v * 4;
            const bool below = lo[e.v] <= x && x < hi[e.v];
            const size_t group = below ? link_size(e.v, x, N) : e.through_root ? link_size(e.w, x, N) : link_size(e.w, x, e.v);
            const double full = raw_log_score((size_t)t[1], (size_t)t[2], (size_t)t[3]);
            std::snprintf(qpic, sizeof qpic, "%.6f", full);
            if (t[0] - r[0] > 0) {
                const double rest = raw_log_score((size_t)(t[1] - r[1]), (size_t)(t[2] - r[2]), (size_t)(t[3] - r[3]));
                std::snprintf(without, sizeof without, "%.6f", rest);
                std::snprintf(delta, sizeof delta, "%.6f", rest - full);
            } else {
                std::snprintf(without, sizeof without, "nan");
                std::snprintf(delta, sizeof delta, "nan");
            }
            f << x << '\t' << ref.names[x] << '\t' << e.v << '\t' << lo[e.v] << '\t' << hi[e.v] << '\t' << group << '\t' << r[0] << '\t' << r[1] << '\t'
              << r[2] << '\t' << r[3] << '\t' << qpic << '\t' << without << '\t' << delta << '\n';
        }
    }
    if (!f) throw std::runtime_error("cannot write " + path);
}

// --branch-trees / --bootstrap / --local-pp: refused like --per-tree, before the device is touched
void check_tree_branches(const Args &a) {
    if (a.bootstrap.empty() && (a.bootstrap_reps_given || a.bootstrap_seed_given)) throw std::runtime_error("--bootstrap-reps / --bootstrap-seed need --bootstrap FILE");
    if (a.local_pp.empty() && a.local_pp_lambda_given) throw std::runtime_error("--local-pp-lambda needs --local-pp FILE");
    for (const char *flag : {"--branch-trees", "--bootstrap", "--local-pp"}) {
        if (output_file(a, flag).empty()) continue;
        if (a.gpus > 0 || a.table_shards >= 0 || !a.dev.load_table.empty())
            throw std::runtime_error(std::string(flag) + " needs the evaluation trees counted on one GPU: omit --gpus / --table-shards / --load-table");
        check_output_file(a, flag);
    }
    if (!a.bootstrap.empty() && a.bootstrap_reps == 0) throw std::runtime_error("--bootstrap-reps must be at least 1");
}

// --branch-trees / --bootstrap / --local-pp: qs_tree_branch_support behind every batch's count into one device buffer of (trees of the
// batch) x n_nodes x 4 words, shared by the three outputs. --branch-trees downloads every batch and writes its lines as it comes;
// --bootstrap adds the batch to the sums of every replicate with its slice of the replicates' weights (qs_branch_resample; row 0 of the
// weights is all ones: the unweighted sums behind the qpic column); --local-pp adds the batch's normalised frequencies to n_nodes x 4
// words (qs_branch_frequencies). Both sums are downloaded once behind the final qs_sync. No buffer grows with m on the device.
struct TreeBranches {
    size_t m = 0, n_taxa = 0;
    int device = 0;
    std::string lines_path, boot_path, pp_path;
    uint32_t reps = 0;
    uint64_t seed = 1;
    double lambda = 0.5;
    qs::DevBuf<int64_t> rows, sums, freq;
    std::vector<uint32_t> weights, slice;   // [1 + reps][m]; the columns of one batch
    std::vector<int64_t> host, totals, freq_totals;
    std::ofstream lines;
    std::unique_ptr<Internodes> in;
    void hook(DeviceOptions &opt, const RefFlat &ref) {
        opt.tree_branches = true;
        in.reset(new Internodes(ref));
        n_taxa = ref.names.size();
        const size_t N = ref.parent.size();
        if (!lines_path.empty()) {
            lines.open(lines_path);
            if (!lines) throw std::runtime_error("cannot write " + lines_path);
            lines << "tree\tnode\tlo\thi\tpresent\tq1\tq2\tq3\tconcordance\n";
        }
        if (!boot_path.empty()) {
            // replicate r draws m tree indices; its weights are their multiplicities
            weights.assign((size_t)(1 + reps) * m, 0);
            std::fill(weights.begin(), weights.begin() + (std::ptrdiff_t)m, 1u);
            for (uint32_t r = 0; r < reps; ++r) {
                Rng rng(seed, r);
                for (size_t i = 0; i < m; ++i) weights[(size_t)(1 + r) * m + rng.below((uint32_t)m)]++;
            }
        }
        add_after_count(opt, [this, &ref, N](qs_ctx *ctx, const qs_device_batch *db, size_t i0, const BatchFlat &b) {
            const size_t k = b.n_trees, words = k * N * 4;
            if (hipSetDevice(device) != hipSuccess || rows.reserve(std::max<size_t>(1, words) * 8, nullptr) != hipSuccess)
                throw std::runtime_error("--branch-trees / --bootstrap / --local-pp: Insufficient memory!");
            const qs_ref_tree rt = ref_view(ref);
            if (qs_tree_branch_support(ctx, &rt, db, rows.get()) != QS_OK) throw std::runtime_error(qs_last_error(ctx));
            if (!boot_path.empty()) {
                const size_t sum_words = (size_t)(1 + reps) * N * 4;
                if (!sums) {
                    if (sums.reserve(std::max<size_t>(1, sum_words) * 8, nullptr) != hipSuccess || hipMemset(sums.get(), 0, sum_words * 8) != hipSuccess || hipDeviceSynchronize() != hipSuccess)
                        throw std::runtime_error("--bootstrap: Insufficient memory!");
                }
                slice.resize((size_t)(1 + reps) * k);
                for (size_t r = 0; r <= reps; ++r) std::copy_n(weights.begin() + (std::ptrdiff_t)(r * m + i0), k, slice.begin() + (std::ptrdiff_t)(r * k));
                if (qs_branch_resample(ctx, rows.get(), (uint32_t)k, (uint32_t)N, slice.data(), 1 + reps, sums.get()) != QS_OK) throw std::runtime_error(qs_last_error(ctx));
            }
            if (!pp_path.empty()) {
                if (!freq) {
                    if (freq.reserve(std::max<size_t>(1, N * 4) * 8, nullptr) != hipSuccess || hipMemset(freq.get(), 0, N * 4 * 8) != hipSuccess || hipDeviceSynchronize() != hipSuccess)
                        throw std::runtime_error("--local-pp: Insufficient memory!");
                }
                if (qs_branch_frequencies(ctx, rows.get(), (uint32_t)k, (uint32_t)N, freq.get()) != QS_OK) throw std::runtime_error(qs_last_error(ctx));
            }
            if (lines_path.empty()) return;   // (the next batch's rows come behind this one's sums on the context's stream)
            // the lines are written as the batch comes: the device is waited for here, which this output pays for and no other
            if (qs_sync(ctx) != QS_OK) throw std::runtime_error(qs_last_error(ctx));
            host.resize(words);
            if (words && hipMemcpy(host.data(), rows.get(), words * 8, hipMemcpyDeviceToHost) != hipSuccess) throw std::runtime_error("--branch-trees: download failed");
            char conc[64];
            for (size_t t = 0; t < k; ++t)
                for (const Internodes::Edge &e : in->edges) {
                    const int64_t *w = &host[(t * N + e.v) * 4];
                    if (w[0] == 0) continue;
                    const int64_t s = w[1] + w[2] + w[3];
                    if (s) std::snprintf(conc, sizeof conc, "%.6f", (double)w[1] / (double)s);
                    else std::snprintf(conc, sizeof conc, "nan");
                    lines << (i0 + t) << '\t' << e.v << '\t' << in->lo[e.v] << '\t' << in->hi[e.v] << '\t' << w[0] << '\t' << w[1] << '\t' << w[2] << '\t' << w[3] << '\t' << conc << '\n';
                }
            if (!lines) throw std::runtime_error("cannot write " + lines_path);
        });
        add_after_sync(opt, [this, N](qs_ctx *) {
            if (!pp_path.empty()) {
                freq_totals.assign(N * 4, 0);
                if (freq && hipMemcpy(freq_totals.data(), freq.get(), freq_totals.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) throw std::runtime_error("--local-pp: download failed");
            }
            if (boot_path.empty()) return;
            totals.assign((size_t)(1 + reps) * N * 4, 0);
            if (sums && hipMemcpy(totals.data(), sums.get(), totals.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) throw std::runtime_error("--bootstrap: download failed");
        });
    }
    void write() {
        if (!lines_path.empty()) {
            lines.close();
            if (!lines) throw std::runtime_error("cannot write " + lines_path);
        }
        write_local_pp();
        if (boot_path.empty()) return;
        const size_t N = in->lo.size(), B = reps;
        std::ofstream f(boot_path);
        if (!f) throw std::runtime_error("cannot write " + boot_path);
        f << "node\tlo\thi\tqpic\tmean\tsd\tlo95\thi95\treps\n";
        std::vector<double> vals(B);
        char text[5][64];
        for (const Internodes::Edge &e : in->edges) {
            auto score = [&](size_t r) { const int64_t *w = &totals[(r * N + e.v) * 4]; return raw_log_score((size_t)w[1], (size_t)w[2], (size_t)w[3]); };
            double total = 0.0, dev2 = 0.0;   // plain double sums in replicate order
            for (size_t r = 0; r < B; ++r) { vals[r] = score(1 + r); total += vals[r]; }
            const double mean = total / (double)B;
            for (size_t r = 0; r < B; ++r) dev2 += (vals[r] - mean) * (vals[r] - mean);
            std::sort(vals.begin(), vals.end());
            const double cols[5] = {score(0), mean, std::sqrt(dev2 / (double)B), vals[(size_t)std::floor(0.025 * (double)(B - 1))], vals[(size_t)std::ceil(0.975 * (double)(B - 1))]};
            for (int i = 0; i < 5; ++i) std::snprintf(text[i], sizeof text[i], "%.6f", cols[i]);
            f << e.v << '\t' << in->lo[e.v] << '\t' << in->hi[e.v] << '\t' << text[0] << '\t' << text[1] << '\t' << text[2] << '\t' << text[3] << '\t' << text[4] << '\t' << B << '\n';
        }
        if (!f) throw std::runtime_error("cannot write " + boot_path);
    }
    // one line per internode from the four words of its node: integers as they are, f_i = Z_i / 2^40 and local_pp.hpp's five as %.6f
    void write_local_pp() {
        if (pp_path.empty()) return;
        const size_t n = n_taxa;
        std::ofstream f(pp_path);
        if (!f) throw std::runtime_error("cannot write " + pp_path);
        f << "node\tlo\thi\ten\tf1\tf2\tf3\tpp1\tpp2\tpp3\tlength\tpolytomy_p\n";
        char text[8][64];
        for (const Internodes::Edge &e : in->edges) {
            const int64_t *w = &freq_totals[e.v * 4];
            // (no 4-set lies around a branch that does not leave two of the tree's n taxa on either side: it is written as en = 0 is)
            const size_t below = in->hi[e.v] - in->lo[e.v];
            const bool splits = n > 1 && below >= 2 && n - below >= 2;
            double cols[8] = {(double)w[1] / 1099511627776.0, (double)w[2] / 1099511627776.0, (double)w[3] / 1099511627776.0};
            local_pp(splits ? w[0] : 0, w + 1, lambda, cols + 3);
            for (int i = 0; i < 8; ++i) {
                if (std::isnan(cols[i])) std::snprintf(text[i], sizeof text[i], "nan");
                else if (std::isinf(cols[i])) std::snprintf(text[i], sizeof text[i], "inf");   // (the length where f1 reaches en + 2L - 1)
                else std::snprintf(text[i], sizeof text[i], "%.6f", cols[i]);
            }
            f << e.v << '\t' << in->lo[e.v] << '\t' << in->hi[e.v] << '\t' << w[0];
            for (int i = 0; i < 8; ++i) f << '\t' << text[i];
            f << '\n';
        }
        if (!f) throw std::runtime_error("cannot write " + pp_path);
    }
};

// --place-clades: refused before the device is touched where the whole table is not on one GPU, where FILE exists or is another output,
// and where a line of --place-clades-only names a label the -r tree lacks, the whole tree, a clade with fewer than three taxa outside it
// or a clade an earlier line names; leaves the nodes to place in a.place_nodes
void check_place_clades(Args &a) {
    if (a.place_clades.empty()) {
        if (!a.place_clades_only.empty()) throw std::runtime_error("--place-clades-only needs --place-clades FILE");
        return;
    }
    if (a.gpus > 0 || a.table_shards >= 0)
        throw std::runtime_error("--place-clades needs the whole count table on one GPU: omit --gpus / --table-shards");
    check_output_file(a, "--place-clades");
    Tree primary = read_reference(a);
    const RefFlat rf = flatten_reference(primary);
    const PlaceShape S(rf, "--place-clades");
    const size_t n = rf.names.size(), N = rf.parent.size();
    std::vector<uint32_t> nchild(N, 0);
    for (size_t v = 0; v < N; ++v) if (rf.parent[v] >= 0) nchild[rf.parent[v]]++;
    if (a.place_clades_only.empty()) {
        for (size_t v = 0; v < N; ++v)
            if (v != S.root && nchild[v] && n - (size_t)(S.hi[v] - S.lo[v]) >= 3) a.place_nodes.push_back((uint32_t)v);
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
        int64_t first = (int64_t)n, last = -1;
        std::istringstream fields(line);
        for (std::string field; std::getline(fields, field, '\t');) {
            const size_t b = field.find_first_not_of(" \r"), e = field.find_last_not_of(" \r");
            if (b == std::string::npos) continue;
            const std::string name = field.substr(b, e - b + 1);
            const auto it = rf.name_to_id.find(name);
            if (it == rf.name_to_id.end()) throw std::runtime_error(what + "the taxon " + name + " is not in the reference tree " + a.ref);
            first = std::min(first, (int64_t)it->second); last = std::max(last, (int64_t)it->second);
        }
        // the smallest subtree that holds all labels: from the first label's leaf upwards until the last label is below as well
        size_t v = rf.leaf_node[(size_t)first];
        while (!(S.lo[v] <= first && last < S.hi[v])) v = (size_t)rf.parent[v];
        if (v == S.root) throw std::runtime_error(what + "the smallest subtree that holds these labels is the whole reference tree");
        if (n - (size_t)(S.hi[v] - S.lo[v]) < 3)
            throw std::runtime_error(what + "the clade leaves fewer than three taxa outside it (" + std::to_string(n - (size_t)(S.hi[v] - S.lo[v])) + ")");
        const auto ins = line_of.emplace((uint32_t)v, line_no);
        if (!ins.second) throw std::runtime_error(what + "the same clade as line " + std::to_string(ins.first->second));
        a.place_nodes.push_back((uint32_t)v);
    }
    if (a.place_nodes.empty()) throw std::runtime_error("--place-clades-only " + a.place_clades_only + ": the list of clades is empty");
}

// --place-clades: one qs_clade_placement over the counted (or loaded) table for the listed nodes, their link sums downloaded, per clade
// qs_placement_scores and the columns (tests/clade_placement_model.py defines them): a position = the edges outside the clade that
// induce the same bipartition of the taxa outside it
void write_place_clades(qs_ctx *ctx, const RefFlat &ref, int device, const std::string &path, const std::vector<uint32_t> &nodes) {
    const size_t n = ref.names.size(), N = ref.parent.size(), L = nodes.size();
    const qs_ref_tree rt = ref_view(ref);
    qs::DevBuf<int64_t> dev;
    if (hipSetDevice(device) != hipSuccess || dev.reserve(L * 2 * N * 8, nullptr) != hipSuccess) throw std::runtime_error("--place-clades: Insufficient memory!");
    if (qs_clade_placement(ctx, &rt, nodes.data(), (uint32_t)L, dev.get()) != QS_OK || qs_sync(ctx) != QS_OK)
        throw std::runtime_error(std::string("--place-clades: ") + qs_last_error(ctx));
    std::vector<int64_t> w(L * 2 * N);
    if (hipMemcpy(w.data(), dev.get(), w.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) throw std::runtime_error("--place-clades: download failed");
    const PlaceShape S(ref, "--place-clades");
    auto walk = [&](size_t a, size_t b) {   // nodes on the path from a to b, both inclusive
        std::vector<size_t> left{a}, right{b};
        while (left.back() != right.back()) {
            if (S.depth[left.back()] >= S.depth[right.back()]) left.push_back((size_t)ref.parent[left.back()]);
            else right.push_back((size_t)ref.parent[right.back()]);
        }
        left.insert(left.end(), right.rbegin() + 1, right.rend());
        return left;
    };
    std::ofstream f(path);
    if (!f) throw std::runtime_error("cannot write " + path);
    f << "clade\tnode\tlo\thi\tsize\tcurrent\tbest\tgain\tn_best\tbest_node\tbest_lo\tbest_hi\tdistance\n";
    std::vector<int64_t> score(N), key(N);
    std::vector<uint8_t> edge(N);
    for (size_t k = 0; k < L; ++k) {
        const size_t c = nodes[k];
        const int64_t cl = S.lo[c], ch = S.hi[c], size = ch - cl;
        if (qs_placement_scores(&rt, &w[k * 2 * N], score.data()) != QS_OK) throw std::runtime_error(std::string("--place-clades: ") + qs_last_error(nullptr));
        // the edges outside the clade and its own; the position of the edge above v: the id interval, in the numbering of the taxa
        // outside the clade, of the side without the smallest of them
        for (size_t v = 0; v < N; ++v) {
            edge[v] = v != S.root && !(v != c && S.lo[v] >= cl && S.hi[v] <= ch);
            int64_t a = S.lo[v] - (S.lo[v] >= ch ? size : 0), b = S.hi[v] - (S.hi[v] >= ch ? size : 0);
            if (a == 0 && b > 0) { a = b; b = (int64_t)n - size; }
            key[v] = b > a ? a * (int64_t)n + b : 0;
        }
        const size_t u = (size_t)ref.parent[c];
        if (S.links[u] == 3)   // the clade's own edge and the two other edges at its parent are one position
            for (size_t v = 0; v < N; ++v) if (v != c && ref.parent[v] == (int32_t)u) { key[c] = key[v]; break; }
        int64_t best = INT64_MIN;
        for (size_t v = 0; v < N; ++v) if (edge[v]) best = std::max(best, score[v]);
        std::set<int64_t> top;
        int64_t first_top = -1;
        for (size_t v = 0; v < N; ++v) if (edge[v] && score[v] == best) { if (top.empty()) first_top = key[v]; top.insert(key[v]); }
        const int64_t current = score[c];
        const int64_t pick = current == best ? key[c] : first_top;
        size_t node = 0;
        for (size_t v = 0; v < N; ++v) if (edge[v] && key[v] == pick) { node = v; break; }
        size_t dist = 0;
        if (pick != key[c]) {
            const std::vector<size_t> to_child = walk(u, node), to_parent = walk(u, (size_t)ref.parent[node]);
            for (size_t v : to_parent.size() < to_child.size() ? to_parent : to_child) dist += S.links[v] - (v == u) >= 3;
        }
        f << k << '\t' << c << '\t' << cl << '\t' << ch << '\t' << size << '\t' << current << '\t' << best << '\t' << (best - current) << '\t' << top.size()
          << '\t' << node << '\t' << S.lo[node] << '\t' << S.hi[node] << '\t' << dist << '\n';
    }
    if (!f) throw std::runtime_error("cannot write " + path);
}

// --also-ref, after the primary tree's output is written: its table re-indexed into `table`'s context (allocated before the
// counting), scored and written per further reference tree
void score_also_refs(const Args &a, qs_ctx *src, const RefFlat &primary, qs_ctx *table) {
    for (const AlsoRef &x : a.also) {
        const auto begin = std::chrono::steady_clock::now();
        std::cout << "Scoring the reference tree " << x.ref << " from the same count table.\n";
        const RefFlat fx = flatten_reference(x.tree);
        std::vector<uint16_t> src_id_of(fx.names.size());
        for (size_t i = 0; i < fx.names.size(); ++i) src_id_of[i] = (uint16_t)primary.name_to_id.at(fx.names[i]);
        if (qs_table_remap(table, src, src_id_of.data()) != QS_OK || qs_sync(table) != QS_OK) throw std::runtime_error(qs_last_error(table));
        const auto remapped = std::chrono::steady_clock::now();
        const auto remap_us = std::chrono::duration_cast<std::chrono::microseconds>(remapped - begin).count();
        std::cout << "Remapped the count table in " << remap_us << " microseconds.\n";
        if (a.dev.trace) std::fprintf(stderr, "[trace] qs_table_remap for %s: %.2f ms\n", x.ref.c_str(), remap_us / 1000.0);
        const EdgeScores sc = score_table(table, ref_view(fx), score_flags(a.dev));
        std::cout << (sc.bifurcating ? "The reference tree is bifurcating.\n" : "The reference tree is multifurcating.\n");
        write_annotated(x.tree, x.out, sc.lq, sc.qp, sc.eqp);
        std::cout << "Finished computing scores.\n";
        std::cout << "It took: " << std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - begin).count()
                  << " microseconds." << std::endl;
    }
}

// --without-taxa, after the primary tree's output is written: per set a context of the kept taxa on `table` (allocated before the
// counting for the largest of them), the count table cut down into it, scored and written
void score_without_taxa(const Args &a, qs_ctx *src, const RefFlat &primary, uint32_t bits, const qs::DevBuf<char> &table) {
    for (const WithoutTaxa &x : a.without) {
        const auto begin = std::chrono::steady_clock::now();
        std::cout << "Scoring the reference tree without " << x.drop.size() << " taxa (" << x.names << ") from the same count table.\n";
        const RefFlat fx = flatten_reference(x.tree);
        std::vector<uint16_t> src_id_of(fx.names.size());
        for (size_t i = 0; i < fx.names.size(); ++i) src_id_of[i] = (uint16_t)primary.name_to_id.at(fx.names[i]);
        qs_ctx *ctx = nullptr;
        if (qs_create(&ctx, (uint32_t)fx.names.size(), bits, QS_FLAG_NONE, a.dev.device, nullptr, 0, 0) != QS_OK) throw std::runtime_error(qs_last_error(nullptr));
        struct Guard { qs_ctx *c; ~Guard() { qs_destroy(c); } } guard{ctx};   // (waits for the context's stream; the table stays the caller's)
        if (qs_table_attach(ctx, table.get(), table.bytes()) != QS_OK) throw std::runtime_error(qs_last_error(ctx));
        const auto attached = std::chrono::steady_clock::now();   // the restrict alone is timed, not the set-up in front of it
        if (qs_table_restrict(ctx, src, src_id_of.data()) != QS_OK || qs_sync(ctx) != QS_OK) throw std::runtime_error(qs_last_error(ctx));
        const auto restrict_us = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - attached).count();
        std::cout << "Restricted the count table in " << restrict_us << " microseconds.\n";
        if (a.dev.trace) std::fprintf(stderr, "[trace] qs_table_restrict for %s: %.2f ms\n", x.names.c_str(), restrict_us / 1000.0);
        const EdgeScores sc = score_table(ctx, ref_view(fx), score_flags(a.dev));
        std::cout << (sc.bifurcating ? "The reference tree is bifurcating.\n" : "The reference tree is multifurcating.\n");
        write_annotated(x.tree, x.out, sc.lq, sc.qp, sc.eqp);
        std::cout << "Finished computing scores.\n";
        std::cout << "It took: " << std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - begin).count()
                  << " microseconds." << std::endl;
    }
}

// --test-groups: everything that needs no GPU, before the device is touched -- the whole table is on one GPU, FILE neither exists nor is
// another output, every line of SPEC parses against the labels of -r, and qs_group_check accepts the patterns; leaves the hypotheses in
// a.group_names / a.group_labels / a.group_kind
void check_test_groups(Args &a) {
    if (a.test_groups.empty()) return;
    if (a.gpus > 0 || a.table_shards >= 0)
        throw std::runtime_error("--test-groups needs the whole count table on one GPU: omit --gpus / --table-shards");
    check_output_file(a, "--test-groups");
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

// --test-groups: one qs_group_support over the counted (or loaded) table, 6 words per hypothesis downloaded, one TSV line each
void write_test_groups(qs_ctx *ctx, int device, const Args &a) {
    const size_t H = a.group_names.size();
    qs::DevBuf<int64_t> dev;
    if (hipSetDevice(device) != hipSuccess || dev.reserve(6 * H * 8, nullptr) != hipSuccess) throw std::runtime_error("--test-groups: Insufficient memory!");
    if (qs_group_support(ctx, a.group_labels.data(), (uint32_t)H, dev.get()) != QS_OK || qs_sync(ctx) != QS_OK)
        throw std::runtime_error(std::string("--test-groups: ") + qs_last_error(ctx));
    std::vector<int64_t> w(6 * H);
    if (hipMemcpy(w.data(), dev.get(), 6 * H * 8, hipMemcpyDeviceToHost) != hipSuccess) throw std::runtime_error("--test-groups: download failed");
    std::ofstream f(a.test_groups);
    if (!f) throw std::runtime_error("cannot write " + a.test_groups);
    f << "name\tkind\tquartets\tq1\tq2\tq3\toutvoted\tuninformed\tsupport\tqpic\n";
    char support[64], qpic[64];
    for (size_t h = 0; h < H; ++h) {
        const int64_t *v = &w[6 * h];
        const bool split = a.group_kind[h] != 0;
        if (v[1] + v[2] + v[3]) std::snprintf(support, sizeof support, "%.6f", (double)v[1] / (double)(v[1] + v[2] + v[3]));
        else std::snprintf(support, sizeof support, "nan");
        if (split) std::snprintf(qpic, sizeof qpic, "nan");
        else std::snprintf(qpic, sizeof qpic, "%.6f", raw_log_score((size_t)v[1], (size_t)v[2], (size_t)v[3]));
        f << a.group_names[h] << '\t' << (split ? "split" : "quad");
        for (int k = 0; k < 6; ++k) f << '\t' << v[k];
        f << '\t' << support << '\t' << qpic << '\n';
    }
    if (!f) throw std::runtime_error("cannot write " + a.test_groups);
}

// --gpus N: trees split over N GPUs, one collective on the table, sharded scoring (multi_gpu.hpp)
void run_multi(const Tree &referenceTree, const Args &a, size_t m, uint32_t count_bits, std::vector<double> &lqic,
               std::vector<double> &qpic, std::vector<double> &eqpic) {
    if (!a.dev.load_table.empty() || !a.dev.save_table.empty()) throw std::runtime_error("--save-table / --load-table work on one GPU (omit --gpus)");
    const bool need_full = !a.raw.empty() || !a.raw_bin.empty();   // the -q dump walks the whole table on one GPU
    MultiGpuQuartetScoreComputer mg(referenceTree, a.eval, m, count_bits, a.gpus, need_full, a.dev);
    lqic = mg.scores.lq; qpic = mg.scores.qp; eqpic = mg.scores.eqp;
    if (!a.raw.empty()) print_raw_qic_scores(mg.context0(), mg.reference(), a.raw, a.dev.ingest_threads, a.raw_rank_order);
    if (!a.raw_bin.empty()) print_raw_qic_binary(mg.context0(), mg.reference(), a.raw_bin);
}

// --table-shards K [--gpus N]: the table cut into K shards by the largest taxon id, shard s on GPU s mod N; every GPU counts
// all trees into its shard(s), no table collective (table_shards.hpp; BASELINE configs[4] = --gpus 8 --table-shards 8)
void run_sharded(const Tree &referenceTree, const Args &a, size_t m, uint32_t count_bits, int shards, int gpus, std::vector<double> &lqic,
                 std::vector<double> &qpic, std::vector<double> &eqpic) {
    if (!a.dev.load_table.empty() || !a.dev.save_table.empty() || !a.raw.empty() || !a.raw_bin.empty())
        throw std::runtime_error("--table-shards: -q / --qic-binary / --save-table / --load-table need the whole table on one device");
    ShardedTableQuartetScoreComputer st(referenceTree, a.eval, m, count_bits, shards, (ShardedTableQuartetScoreComputer::Spill)a.spill, a.dev, gpus);
    lqic = st.scores.lq; qpic = st.scores.qp; eqpic = st.scores.eqp;
}

template <typename CINT>
void run(const Tree &referenceTree, const Args &a, size_t m, std::vector<double> &lqic, std::vector<double> &qpic,
         std::vector<double> &eqpic) {
    const uint32_t bits = sizeof(CINT) <= 2 ? 16u : 32u;
    size_t n = 0;
    for (size_t v = 0; v < referenceTree.node_count(); ++v) n += referenceTree.is_leaf(v);
    const uint64_t bytes = c4(n) * 3 * (bits / 8);
    const int gpus = std::max(1, a.gpus);
    if (a.table_shards >= 0 || a.gpus > 0) {
        // shards one device's free memory asks for (0 / unset = automatic); with --gpus N at least one shard per GPU
        const int needed = ShardedTableQuartetScoreComputer::shards_needed(bytes, a.dev.device);
        if (a.table_shards > 0) return run_sharded(referenceTree, a, m, bits, a.table_shards, gpus, lqic, qpic, eqpic);
        if (needed > 1) {
            if (a.gpus > 0 && a.table_shards < 0)
                std::cout << "The count table (" << bytes << " bytes) does not fit one GPU: table-sharded mode instead of tree-sharded.\n";
            return run_sharded(referenceTree, a, m, bits, std::max(needed, gpus), gpus, lqic, qpic, eqpic);
        }
        if (a.gpus > 0 && a.table_shards == 0) return run_sharded(referenceTree, a, m, bits, gpus, gpus, lqic, qpic, eqpic);
    }
    if (a.gpus > 1 && a.table_shards < 0) {
        // N GPUs, the table fits one of them: tree- or table-sharded. The count work per GPU is the same either way;
        // the table-sharded mode needs no collective and no communicator, the tree-sharded one keeps the whole table on GPU 0
        // (which -q / --qic-binary / --save-table walk).
        const bool need_whole = !a.raw.empty() || !a.raw_bin.empty() || !a.dev.save_table.empty() || !a.dev.load_table.empty();
        double coll_ms = 0.0, extra_ms = 0.0;
        const bool model_table = ShardedTableQuartetScoreComputer::prefer_table_shards((uint32_t)n, m, gpus, a.dev.reduce == "rccl", coll_ms, extra_ms);
        // (--gpus-on-one-device without --mode stays the test hook of the tree-sharded reductions it was written for)
        const bool table = !need_whole && (a.mode == "table" || (a.mode == "auto" && model_table && !a.dev.gpus_on_one_device));
        if (a.mode == "table" && need_whole) std::cout << "--mode table: -q / --qic-binary / --save-table / --load-table need the whole table on one device; tree-sharded mode instead.\n";
        if (table) {
            std::cout << "Table-sharded counting on " << gpus << " GPUs (" << (a.mode == "table" ? "--mode table" : "auto")
                      << ": table collective ~" << coll_ms << " ms against ~" << extra_ms << " ms of replicated panel build and imbalance).\n";
            return run_sharded(referenceTree, a, m, bits, gpus, gpus, lqic, qpic, eqpic);
        }
    }
    if (a.gpus > 0) return run_multi(referenceTree, a, m, bits, lqic, qpic, eqpic);
    // --also-ref: the second table is allocated before anything is counted, so that a table that fits once but not twice is
    // reported now and not after the counting
    qs_ctx *also_table = nullptr;
    struct AlsoTable { qs_ctx *&c; bool keep; ~AlsoTable() { if (!keep) qs_destroy(c); } } also_guard{also_table, !a.clean_exit};
    if (!a.also.empty()) {
        if (ShardedTableQuartetScoreComputer::shards_needed(bytes, a.dev.device) > 1)
            throw std::runtime_error("--also-ref needs the whole count table (" + std::to_string(bytes) + " bytes) on one GPU");
        if (qs_create(&also_table, (uint32_t)n, bits, QS_FLAG_NONE, a.dev.device, nullptr, 0, 0) != QS_OK) throw std::runtime_error(qs_last_error(nullptr));
        if (qs_table_alloc(also_table) != QS_OK) throw std::runtime_error(std::string("--also-ref: ") + qs_last_error(also_table));
        trace_mark(a.dev, "main: --also-ref table allocated");
    }
    // --without-taxa: likewise one table for the largest set of kept taxa, which every set's context attaches in its turn
    std::unique_ptr<qs::DevBuf<char>> without_holder(new qs::DevBuf<char>());
    qs::DevBuf<char> &without_table = *without_holder;
    if (!a.without.empty()) {
        size_t kept = 0;
        for (const WithoutTaxa &x : a.without) kept = std::max(kept, x.tree.leaf_count());
        // qs_table_bytes of a context of `kept` taxa (C(kept,4) tuples of three cells; computed here because no such context exists
        // yet) plus qs_table_alloc's 16 bytes of padding: qs_table_attach checks the size against qs_table_bytes for every set
        const size_t need = (size_t)(c4(kept) * 3 * (bits / 8)) + 16;
        size_t freeb = 0, total = 0;
        hip_ok(hipSetDevice(a.dev.device), "--without-taxa: hipSetDevice");
        hip_ok(hipMemGetInfo(&freeb, &total), "--without-taxa: hipMemGetInfo");
        if (need + bytes + (64u << 20) > freeb || without_table.reserve(need, nullptr) != hipSuccess)   // (the -r tree's table comes on top)
            throw std::runtime_error("--without-taxa: Insufficient memory!");
        trace_mark(a.dev, "main: --without-taxa table allocated");
    }
    // (without --clean-exit the computer is never destroyed: freeing a 17-34 GB table and the context is work the exiting process
    // leaves to the driver -- main ends with std::_Exit once the output is written)
    PerTree per_tree;
    DeviceOptions dev = a.dev;
    const RefFlat per_tree_ref = a.per_tree.empty() ? RefFlat() : flatten_reference(referenceTree);
    if (!a.per_tree.empty()) {
        per_tree.m = m;
        per_tree.device = a.dev.device;
        dev.per_tree = a.per_tree;
        per_tree.hook(dev, per_tree_ref);
    }
    TreeBranches tree_branches;
    const bool want_branches = !a.branch_trees.empty() || !a.bootstrap.empty() || !a.local_pp.empty();
    const RefFlat tree_branches_ref = want_branches ? flatten_reference(referenceTree) : RefFlat();
    if (want_branches) {
        tree_branches.m = m;
        tree_branches.device = a.dev.device;
        tree_branches.lines_path = a.branch_trees;
        tree_branches.boot_path = a.bootstrap;
        tree_branches.reps = a.bootstrap_reps;
        tree_branches.seed = a.bootstrap_seed;
        tree_branches.pp_path = a.local_pp;
        tree_branches.lambda = a.local_pp_lambda;
        tree_branches.hook(dev, tree_branches_ref);
    }
    TreeDistances tree_distances;
    if (!a.tree_distances.empty()) {
        dev.tree_distances = a.tree_distances;
        tree_distances.hook(dev);
    }
    std::unique_ptr<QuartetScoreComputer<CINT>> holder(new QuartetScoreComputer<CINT>(referenceTree, a.eval, m, a.verbose, a.savemem, dev));
    QuartetScoreComputer<CINT> &qsc = *holder;
    lqic = qsc.getLQICScores();
    qpic = qsc.getQPICScores();
    eqpic = qsc.getEQPICScores();
    qsc.raw_threads = a.dev.ingest_threads;
    qsc.raw_rank_order = a.raw_rank_order;
    if (!a.raw.empty()) qsc.printRawQICScores(a.raw);
    if (!a.raw_bin.empty()) qsc.printRawQICBinary(a.raw_bin);
    if (!a.per_tree.empty()) per_tree.write(a.per_tree);
    if (!a.tree_distances.empty()) tree_distances.write(qsc.context(), a.dev.device, a.tree_distances);
    if (want_branches) tree_branches.write();
    if (!a.per_taxon.empty()) write_per_taxon(qsc.context(), qsc.reference(), a.dev.device, a.per_taxon);
    if (!a.place_taxa.empty()) write_place_taxa(qsc.context(), qsc.reference(), a.dev.device, a.place_taxa, a.place_ids);
    if (!a.place_clades.empty()) write_place_clades(qsc.context(), qsc.reference(), a.dev.device, a.place_clades, a.place_nodes);
    if (!a.test_groups.empty()) write_test_groups(qsc.context(), a.dev.device, a);
    if (!a.taxon_pairs.empty()) write_taxon_pairs(qsc.context(), qsc.reference(), a.dev.device, a.taxon_pairs, a.pair_ids);
    if (!a.drop_one.empty()) write_drop_one(qsc.context(), qsc.reference(), a.dev.device, a.drop_one, a.drop_ids);
    if (!a.also.empty() || !a.without.empty()) {   // the primary tree's output first, exactly as without --also-ref / --without-taxa
        write_annotated(referenceTree, a.out, lqic, qpic, eqpic);
        score_also_refs(a, qsc.context(), qsc.reference(), also_table);
        score_without_taxa(a, qsc.context(), qsc.reference(), bits, without_table);
    }
    if (!a.clean_exit) { (void)holder.release(); (void)without_holder.release(); }
}

} // namespace

int main(int argc, char *argv[]) {
    auto begin = std::chrono::steady_clock::now();
    Args a;
    int pr = parse(argc, argv, a);
    if (pr == 1) return 1;
    if (pr == 2) return 0;
    a.dev.savemem_lookups = a.savemem;   // -s: the reference's compact table behind the lookups of a rooted reference tree

    std::ifstream infile(a.out);
    if (infile.good()) {
        std::cout << "ERROR: The specified output file already exists.\n";
        return 1;
    }
    try {
        check_also_refs(a);
        check_without_taxa(a);
        check_per_tree(a);
        check_tree_distances(a);
        check_tree_branches(a);
        check_per_taxon(a);
        a.place_ids = check_taxon_list_output(a, "--place-taxa", "--place-only", a.place_only);
        check_place_clades(a);
        check_test_groups(a);
        a.pair_ids = check_taxon_list_output(a, "--taxon-pairs", "--taxon-pairs-only", a.taxon_pairs_only);
        a.drop_ids = check_taxon_list_output(a, "--drop-one", "--drop-one-only", a.drop_one_only);
    } catch (const std::exception &e) {
        std::cerr << "ERROR: " << e.what() << std::endl;
        return 1;
    }
    a.dev.ingest_threads = (unsigned)a.threads;
    trace_mark(a.dev, "main: arguments parsed");
    // HIP start-up (~0.1-0.2 s: driver, device, code objects) begins NOW on a helper thread, while this thread reads and
    // splits the Newick files; the counter's own set-up thread then finds the runtime initialised
    std::thread hip_start([&a] { qs_ctx *probe = nullptr; if (qs_create(&probe, 4, 16, QS_FLAG_NONE, a.dev.device, nullptr, 0, 0) == QS_OK) qs_destroy(probe); trace_mark(a.dev, "hip thread: runtime initialised"); });
    struct Joiner { std::thread &t; ~Joiner() { if (t.joinable()) t.join(); } } hip_start_join{hip_start};

    try {
        std::string refText = slurp(a.ref);
        NewickReader rr(refText);
        Tree referenceTree;
        if (!rr.next(referenceTree)) throw std::runtime_error("empty reference tree file");

        if (a.verbose) {
            for (size_t v = 0; v < referenceTree.node_count(); ++v)
                if (referenceTree.is_leaf(v)) std::cout << referenceTree.name[v] << " " << v << "\n";
            std::cout << std::endl;
        }

        // What the scoring will refuse because of the reference tree alone is known before anything is counted (qs_score_check,
        // host-only): `-s` with a rooted reference tree. The reference program counts first and dies in its scoring loop; this run
        // says so NOW and then does the same -- or ends at once with --fail-fast.
        if (a.savemem) {
            const RefFlat rf0 = flatten_reference(referenceTree);
            const qs_ref_tree rt0 = ref_view(rf0);
            if (qs_score_check(nullptr, &rt0, QS_SCORE_SAVEMEM_LOOKUPS | (a.dev.root_as_edge ? QS_SCORE_ROOT_AS_EDGE : 0u)) == QS_ERR_REFERENCE_THROWS) {
                const std::string what = qs_last_error(nullptr);
                if (a.fail_fast) throw std::runtime_error(what);
                std::cerr << "Note: -s with a rooted reference tree: the reference program ends in its scoring loop with \"" << what
                          << "\" after it has counted, and so will this run (--fail-fast ends it now).\n";
            }
        }

        std::vector<double> lqic, qpic, eqpic;
        size_t m = countEvalTrees(a.eval);
        if (!a.local_pp.empty() && m >= (size_t(1) << 23)) throw std::runtime_error("--local-pp: 2^23 evaluation trees or more are not supported (the sums of 2^40-scaled frequencies could leave 63 bits)");
        trace_mark(a.dev, "main: evaluation file read and split into trees");
        // (round 5: no join of the HIP start-up here -- the counter's GPU set-up thread simply blocks in its first HIP call until the
        // runtime is up, while THIS thread already flattens the first batch: 25-30 ms of the start-up leave the critical path)
        // counter width by m as in QuartetScores.cpp:115-147 (u8 is widened to the GPU's 16-bit cells)
        if (m < (size_t(1) << 8)) run<uint8_t>(referenceTree, a, m, lqic, qpic, eqpic);
        else if (m < (size_t(1) << 16)) run<uint16_t>(referenceTree, a, m, lqic, qpic, eqpic);
        else if (m < (size_t(1) << 32)) run<uint32_t>(referenceTree, a, m, lqic, qpic, eqpic);
        else throw std::runtime_error("more than 2^32 evaluation trees are not supported");

        if (a.also.empty() && a.without.empty()) write_annotated(referenceTree, a.out, lqic, qpic, eqpic);   // (else: written by run())
    } catch (const std::exception &e) {
        std::cerr << "ERROR: " << e.what() << std::endl;
        if (a.savemem && std::string(e.what()).rfind("id = ", 0) == 0)
            std::cerr << "       (-s with a rooted reference tree: the reference's memory-efficient table throws this std::runtime_error for the\n"
                         "       node pairs of the root, quartet_lookup_table.hpp:79-85, and its run ends here as well. Without -s the root's\n"
                         "       pairs are scored like the reference's runtime-efficient table scores them; --root-as-edge treats the root as\n"
                         "       a point on one edge.)\n";
        return 1;
    }

    auto end = std::chrono::steady_clock::now();
    std::cout << "Elapsed time: " << std::chrono::duration_cast<std::chrono::microseconds>(end - begin).count()
              << " microseconds." << std::endl;
    if (!a.clean_exit) {
        // Everything the run produces is written and closed. What is left is tearing down the HIP runtime (and RCCL): tens of
        // milliseconds of a 0.5 s run that buy nothing -- the driver reclaims the process' device memory either way.
        // --clean-exit keeps the ordinary return (profilers and sanitizers flush in their exit handlers).
        std::cout.flush(); std::cerr.flush(); std::fflush(nullptr);
        if (hip_start.joinable()) hip_start.join();
        std::_Exit(0);
    }
    return 0;
}
