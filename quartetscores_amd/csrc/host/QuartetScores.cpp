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
// --species-map FILE takes evaluation trees with several individuals per species of the -r tree: they are counted under the individuals'
// ids and the table is summed into the species' table on the device (qs_table_collapse); everything after works on the species.
// --drop-one FILE [--drop-one-only NAMES] writes, per taxon and internode of the -r tree, the internode's QP-IC without that taxon, from
// the same count table (qs_branch_taxon_support).
//
// The file holds main, the choice of the route (one GPU, --gpus N, --table-shards K) and the annotated tree. The options, their table,
// the registry of output files and the checks before the device is touched are in cli_args.hpp; what queries the device for an output
// in cli_queries.hpp; what turns the downloaded words into lines, host only, in cli_reports.hpp.
#include "QuartetScoreComputer.hpp"
#include "multi_gpu.hpp"
#include "table_shards.hpp"
#include "tree_distances.hpp"
#include "cli_args.hpp"
#include "cli_queries.hpp"

#include <algorithm>
#include <chrono>
#include <fstream>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

using namespace qsh;

// annotated Newick: per edge "qp-ic:X;lq-ic:Y;eqp-ic:Z" via std::to_string, parts omitted when +inf;
// the qp-ic guard tests the LQ value like the reference (quartet_newick_writer.hpp:164-187, quirk Q6)
void qsh::write_annotated(const Tree &tree, const std::string &path, const EdgeScores &sc) {
    const double inf = std::numeric_limits<double>::infinity();
    auto comment = [&](size_t v) -> std::string {
        if (v == 0) return std::string();
        const size_t e = v - 1;
        std::string s;
        auto add = [&](const std::string &part) { if (!s.empty()) s += ";"; s += part; };
        if (!sc.qp.empty() && sc.lq[e] != inf) add("qp-ic:" + std::to_string(sc.qp[e]));
        if (sc.lq[e] != inf) add("lq-ic:" + std::to_string(sc.lq[e]));
        if (!sc.eqp.empty() && sc.eqp[e] != inf) add("eqp-ic:" + std::to_string(sc.eqp[e]));
        return s;
    };
    std::ofstream out(path);
    if (!out) throw std::runtime_error("cannot write " + path);
    out << write_newick(tree, comment) << "\n";
}

namespace {

// --gpus N: trees split over N GPUs, one collective on the table, sharded scoring (multi_gpu.hpp)
EdgeScores run_multi(const Tree &referenceTree, const Args &a, size_t m, uint32_t count_bits) {
    if (!a.dev.load_table.empty() || !a.dev.save_table.empty()) throw std::runtime_error("--save-table / --load-table work on one GPU (omit --gpus)");
    const bool need_full = !a.raw.empty() || !a.raw_bin.empty();   // the -q dump walks the whole table on one GPU
    MultiGpuQuartetScoreComputer mg(referenceTree, a.eval, m, count_bits, a.gpus, need_full, a.dev);
    if (!a.raw.empty()) print_raw_qic_scores(mg.context0(), mg.reference(), a.raw, a.dev.ingest_threads, a.raw_rank_order);
    if (!a.raw_bin.empty()) print_raw_qic_binary(mg.context0(), mg.reference(), a.raw_bin);
    return mg.scores;
}

// --table-shards K [--gpus N]: the table cut into K shards by the largest taxon id, shard s on GPU s mod N; every GPU counts
// all trees into its shard(s), no table collective (table_shards.hpp; BASELINE configs[4] = --gpus 8 --table-shards 8)
EdgeScores run_sharded(const Tree &referenceTree, const Args &a, size_t m, uint32_t count_bits, int shards, int gpus) {
    if (!a.dev.load_table.empty() || !a.dev.save_table.empty() || !a.raw.empty() || !a.raw_bin.empty())
        throw std::runtime_error("--table-shards: -q / --qic-binary / --save-table / --load-table need the whole table on one device");
    ShardedTableQuartetScoreComputer st(referenceTree, a.eval, m, count_bits, shards, (ShardedTableQuartetScoreComputer::Spill)a.spill, a.dev, gpus);
    return st.scores;
}

template <typename CINT>
EdgeScores run(const Tree &referenceTree, const Args &a, size_t m) {
    uint32_t bits = sizeof(CINT) <= 2 ? 16u : 32u;
    size_t n = 0;
    for (size_t v = 0; v < referenceTree.node_count(); ++v) n += referenceTree.is_leaf(v);
    // The width of the table that is scored, and with it of the --also-ref / --without-taxa tables cut from it, is not always m's: the
    // species' table of --species-map is widened where m x (the four largest groups) leaves 16 bits, and a table saved by such a run
    // is loaded at the width its size implies (single-GPU route only; the others refuse both options)
    uint32_t scored_bits = 0;
    if (a.dev.species) scored_bits = species_table_bits(bits, m, *a.dev.species);
    else if (!a.dev.load_table.empty() && a.gpus == 0 && a.table_shards < 0) {
        scored_bits = saved_table_bits(a.dev.load_table, n);
        if (!scored_bits) throw std::runtime_error("--load-table: size does not match this reference tree (neither its 16-bit nor its 32-bit table)");
    }
    const uint64_t bytes = c4(n) * 3 * (bits / 8);
    const int gpus = std::max(1, a.gpus);
    if (a.table_shards >= 0 || a.gpus > 0) {
        // shards one device's free memory asks for (0 / unset = automatic); with --gpus N at least one shard per GPU
        const int needed = ShardedTableQuartetScoreComputer::shards_needed(bytes, a.dev.device);
        if (a.table_shards > 0) return run_sharded(referenceTree, a, m, bits, a.table_shards, gpus);
        if (needed > 1) {
            if (a.gpus > 0 && a.table_shards < 0)
                std::cout << "The count table (" << bytes << " bytes) does not fit one GPU: table-sharded mode instead of tree-sharded.\n";
            return run_sharded(referenceTree, a, m, bits, std::max(needed, gpus), gpus);
        }
        if (a.gpus > 0 && a.table_shards == 0) return run_sharded(referenceTree, a, m, bits, gpus, gpus);
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
            return run_sharded(referenceTree, a, m, bits, gpus, gpus);
        }
    }
    if (a.gpus > 0) return run_multi(referenceTree, a, m, bits);
    // --also-ref: the second table is allocated before anything is counted, so that a table that fits once but not twice is
    // reported now and not after the counting
    if (scored_bits) bits = scored_bits;   // (from here on: the tables re-indexed out of the scored one)
    const uint64_t scored_bytes = c4(n) * 3 * (bits / 8);
    qs_ctx *also_table = nullptr;
    struct AlsoTable { qs_ctx *&c; bool keep; ~AlsoTable() { if (!keep) qs_destroy(c); } } also_guard{also_table, !a.clean_exit};
    if (!a.also.empty()) {
        if (ShardedTableQuartetScoreComputer::shards_needed(scored_bytes, a.dev.device) > 1)
            throw std::runtime_error("--also-ref needs the whole count table (" + std::to_string(scored_bytes) + " bytes) on one GPU");
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
        if (need + scored_bytes + (64u << 20) > freeb || without_table.reserve(need, nullptr) != hipSuccess)   // (the -r tree's table comes on top)
            throw std::runtime_error("--without-taxa: Insufficient memory!");
        trace_mark(a.dev, "main: --without-taxa table allocated");
    }
    // the outputs that work behind every batch's count hook themselves into the options, in this order
    DeviceOptions dev = a.dev;
    dev.table_bits = scored_bits;
    std::unique_ptr<PerTree> per_tree;
    if (!a.per_tree.empty()) per_tree.reset(new PerTree(a, m, referenceTree, dev));
    std::unique_ptr<TreeBranches> tree_branches;
    if (TreeBranches::wanted(a)) tree_branches.reset(new TreeBranches(a, m, referenceTree, dev));
    std::unique_ptr<TreeTaxa> tree_taxa;
    if (!a.tree_taxa.empty()) tree_taxa.reset(new TreeTaxa(a, referenceTree, dev));
    TreeDistances tree_distances;
    if (!a.tree_distances.empty()) {
        dev.tree_distances = a.tree_distances;
        tree_distances.hook(dev);
    }
    // (without --clean-exit the computer is never destroyed: freeing a 17-34 GB table and the context is work the exiting process
    // leaves to the driver -- main ends with std::_Exit once the output is written)
    std::unique_ptr<QuartetScoreComputer<CINT>> holder(new QuartetScoreComputer<CINT>(referenceTree, a.eval, m, a.verbose, a.savemem, dev));
    QuartetScoreComputer<CINT> &qsc = *holder;
    EdgeScores sc;
    sc.lq = qsc.getLQICScores();
    sc.qp = qsc.getQPICScores();
    sc.eqp = qsc.getEQPICScores();
    qsc.raw_threads = a.dev.ingest_threads;
    qsc.raw_rank_order = a.raw_rank_order;
    if (!a.raw.empty()) qsc.printRawQICScores(a.raw);
    if (!a.raw_bin.empty()) qsc.printRawQICBinary(a.raw_bin);
    if (per_tree) per_tree->write();
    if (!a.tree_distances.empty()) tree_distances.write(qsc.context(), a.dev.device, a.tree_distances);
    if (tree_branches) tree_branches->write();
    if (tree_taxa) tree_taxa->write();
    if (!a.per_taxon.empty()) write_per_taxon(qsc.context(), qsc.reference(), a);
    if (!a.place_taxa.empty()) write_place_taxa(qsc.context(), qsc.reference(), a);
    if (!a.place_clades.empty()) write_place_clades(qsc.context(), qsc.reference(), a);
    if (!a.test_groups.empty()) write_test_groups(qsc.context(), a);
    if (!a.taxon_pairs.empty()) write_taxon_pairs(qsc.context(), qsc.reference(), a);
    if (!a.drop_one.empty()) write_drop_one(qsc.context(), qsc.reference(), a);
    if (!a.also.empty() || !a.without.empty()) {   // the primary tree's output first, exactly as without --also-ref / --without-taxa
        write_annotated(referenceTree, a.out, sc);
        score_also_refs(a, qsc.context(), qsc.reference(), also_table);
        score_without_taxa(a, qsc.context(), qsc.reference(), bits, without_table);
    }
    if (!a.clean_exit) { (void)holder.release(); (void)without_holder.release(); }
    return sc;
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
    try {   // (the order decides which message a command line sees that trips two checks)
        check_species_map(a);
        check_also_refs(a);
        check_without_taxa(a);
        check_output(a, "--per-tree");
        check_output(a, "--tree-distances");
        check_tree_branches(a);
        check_output(a, "--per-taxon");
        a.place_ids = check_taxon_list_output(a, "--place-taxa");
        check_place_clades(a);
        check_test_groups(a);
        a.pair_ids = check_taxon_list_output(a, "--taxon-pairs");
        a.drop_ids = check_taxon_list_output(a, "--drop-one");
        check_tree_taxa(a);
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
        const Tree referenceTree = read_reference(a);

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

        size_t m = countEvalTrees(a.eval);
        if (!a.local_pp.empty() && m >= (size_t(1) << 23)) throw std::runtime_error("--local-pp: 2^23 evaluation trees or more are not supported (the sums of 2^40-scaled frequencies could leave 63 bits)");
        trace_mark(a.dev, "main: evaluation file read and split into trees");
        // (round 5: no join of the HIP start-up here -- the counter's GPU set-up thread simply blocks in its first HIP call until the
        // runtime is up, while THIS thread already flattens the first batch: 25-30 ms of the start-up leave the critical path)
        // counter width by m as in QuartetScores.cpp:115-147 (u8 is widened to the GPU's 16-bit cells)
        if (m >= (size_t(1) << 32)) throw std::runtime_error("more than 2^32 evaluation trees are not supported");
        const EdgeScores sc = m < (size_t(1) << 8) ? run<uint8_t>(referenceTree, a, m) : m < (size_t(1) << 16) ? run<uint16_t>(referenceTree, a, m) : run<uint32_t>(referenceTree, a, m);

        if (a.also.empty() && a.without.empty()) write_annotated(referenceTree, a.out, sc);   // (else: written by run())
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
