// host_common.hpp -- what the three routes of the CLI (one GPU, --gpus N, --table-shards K) share above the C-ABI: the options,
// the views of the flattened trees, the count loop of one context (BatchQueue) and the two-round sharded scoring (ScoreFold).
#pragma once

#include "../../../include/quartetscores_hip.h"
#include "../qs_devbuf.hpp"
#include "flatten.hpp"
#include "quartet_math.hpp"

#include <chrono>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

namespace qsh {

// --species-map: the individuals behind the species of the -r tree in counting order -- species in lookup-id order, individuals in
// map order within a species; species i owns the counting ids [first_id[i], first_id[i + 1]) (qs_table_collapse)
struct SpeciesLayout {
    std::vector<std::string> names;
    std::unordered_map<std::string, uint32_t> name_to_id;
    std::vector<uint16_t> first_id;
    uint64_t top4 = 1;   // the product of the four largest groups: a collapsed cell is at most m times this
};

struct DeviceOptions {
    int device = 0;
    uint32_t algo = QS_ALGO_AUTO;
    size_t batch_trees = 8192;   // trees per device batch = 256 groups of 32 = one panel slice = one launch of the count kernel per depth
                                 // class (each launch reads and writes the whole table once); batch k+1 is parsed and flattened on the
                                 // host threads while batch k counts
    size_t first_batch_trees = 2048;   // ... and only the FIRST batch's parse is exposed: it is a small one (the device starts after
                                 // ~1/4 of the time; 512 taxa x 10000 trees: counting phase 0.43 -> 0.39 s at -t 8)
    unsigned ingest_threads = 0; // host threads that parse + flatten (0 = hardware concurrency); the CLI's -t
    bool qp_exact64 = false;
    bool root_as_edge = false;   // QS_SCORE_ROOT_AS_EDGE: a degree-2 root as a subdivision of one edge (not the reference's quirk Q5)
    bool savemem_lookups = false; // QS_SCORE_SAVEMEM_LOOKUPS (the CLI's -s): a rooted reference tree ends the run with the
                                 // std::runtime_error the reference's compact table throws (quartet_lookup_table.hpp:79-85)
    std::string reduce = "rccl"; // --gpus N: "rccl" (ncclReduceScatter / ncclAllReduce) or "p2p" (peer access, no communicator: multi_gpu.hpp)
    bool gpus_on_one_device = false; // test hook of --reduce p2p: the N "GPUs" are N contexts on device `device`
    bool comm_overlap = false;   // --gpus N, rccl: count while ncclCommInitAll runs (false: the first launch waits for the communicators)
    std::string load_table, save_table; // count-table persistence
    bool trace = false;          // --trace: time stamps of the counting pipeline on stderr
    std::shared_ptr<const SpeciesLayout> species;   // --species-map FILE: count under the individuals' ids, then collapse into the species' table
    uint32_t table_bits = 0;     // cell width of the table the run scores where the number of trees does not decide it (0 = it does): the species'
                                 // table of --species-map (m x the four largest groups), a --load-table file (its size)
    std::string per_tree;        // --per-tree FILE: batches carry their node ranges (qs_tree_agreement reads them)
    std::string tree_distances;  // --tree-distances FILE: likewise (qs_tree_pair_agreement reads them)
    bool tree_branches = false;  // --branch-trees / --bootstrap / --local-pp / --tree-taxa: likewise (qs_tree_branch_support, qs_tree_taxon_agreement read them)
    // called behind every batch's qs_count_batch (first tree of the batch, the flattened batch) and behind the final qs_sync;
    // several features share them through add_after_count / add_after_sync
    std::function<void(qs_ctx *, const qs_device_batch *, size_t, const BatchFlat &)> after_count;
    std::function<void(qs_ctx *)> after_sync;
};

// one more callback behind those the option already holds, in the order they were added
inline void add_after_count(DeviceOptions &opt, std::function<void(qs_ctx *, const qs_device_batch *, size_t, const BatchFlat &)> f) {
    if (!opt.after_count) { opt.after_count = std::move(f); return; }
    auto first = std::move(opt.after_count);
    opt.after_count = [first, f](qs_ctx *ctx, const qs_device_batch *db, size_t i0, const BatchFlat &b) { first(ctx, db, i0, b); f(ctx, db, i0, b); };
}
inline void add_after_sync(DeviceOptions &opt, std::function<void(qs_ctx *)> f) {
    if (!opt.after_sync) { opt.after_sync = std::move(f); return; }
    auto first = std::move(opt.after_sync);
    opt.after_sync = [first, f](qs_ctx *ctx) { first(ctx); f(ctx); };
}

// --trace: "[trace] +12.3 ms  what" relative to the first call (process start for practical purposes)
inline void trace_mark(const DeviceOptions &opt, const char *what) {
    if (!opt.trace) return;
    static const auto t0 = std::chrono::steady_clock::now();
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    std::fprintf(stderr, "[trace] +%8.1f ms  %s\n", ms, what);
}

inline void hip_ok(hipError_t e, const char *what) { if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e)); }

// the devices used are opt.device .. opt.device + n_gpus - 1 (--gpus-on-one-device, a test hook: all on opt.device)
inline void check_device_range(const DeviceOptions &opt, int n_gpus, int ndev) {
    if (n_gpus < 1 || opt.device < 0 || opt.device + (opt.gpus_on_one_device ? 1 : n_gpus) > ndev)
        throw std::runtime_error("--gpus " + std::to_string(n_gpus) + " from --device " + std::to_string(opt.device) + ": " + std::to_string(ndev) + " device(s) visible");
}

// the C-ABI's views of the flattened trees (they point into their argument)
inline qs_ref_tree ref_view(const RefFlat &r) {
    qs_ref_tree rt;
    rt.n_nodes = (uint32_t)r.parent.size(); rt.n_taxa = (uint32_t)r.names.size();
    rt.parent = r.parent.data(); rt.leaf_node = r.leaf_node.data();
    return rt;
}
inline qs_tree_batch batch_view(const BatchFlat &b, bool want_ranges) {   // ranges: read by the scatter kernel and the per-tree agreement
    qs_tree_batch hb;
    hb.n_trees = b.n_trees; hb.leaf_off = b.leaf_off.data(); hb.leaf_ids = b.leaf_ids.data(); hb.adj_depth = b.adj_depth.data();
    hb.node_off = want_ranges ? b.node_off.data() : nullptr; hb.rng_off = want_ranges ? b.rng_off.data() : nullptr;
    hb.ranges = b.ranges.data();
    return hb;
}
inline uint32_t score_flags(const DeviceOptions &o) {
    return (o.qp_exact64 ? QS_SCORE_QP_EXACT64 : QS_SCORE_QP_WRAP32) | (o.root_as_edge ? QS_SCORE_ROOT_AS_EDGE : 0u) |
           (o.savemem_lookups ? QS_SCORE_SAVEMEM_LOOKUPS : 0u);
}

struct EdgeScores {
    std::vector<double> lq, qp, eqp; // per edge (edge e = edge above node e + 1, preorder), qp / eqp empty for a multifurcating reference
    bool bifurcating = false;
};
inline EdgeScores edge_scores(const std::vector<double> &lq, const std::vector<double> &qp, const std::vector<double> &eqp, bool bif) {
    EdgeScores s;
    s.bifurcating = bif;
    s.lq.assign(lq.begin() + 1, lq.end());
    if (bif) { s.qp.assign(qp.begin() + 1, qp.end()); s.eqp.assign(eqp.begin() + 1, eqp.end()); }
    return s;
}
// qs_score on a context that holds the whole table
inline EdgeScores score_table(qs_ctx *ctx, const qs_ref_tree &rt, uint32_t flags) {
    std::vector<double> lq(rt.n_nodes), qp(rt.n_nodes), eqp(rt.n_nodes);
    int bif = 0;
    if (qs_score(ctx, &rt, flags, lq.data(), qp.data(), eqp.data(), &bif) != QS_OK) throw std::runtime_error(qs_last_error(ctx));
    return edge_scores(lq, qp, eqp, bif != 0);
}

// The count loop of one context: at most two device batches alive, the one being counted and the one being uploaded. Freeing is
// cheap (the library keeps the device slab for the next upload and orders its reuse behind the kernels). A queue that goes away
// without release() -- an exception -- waits for the device and frees what is left.
class BatchQueue {
public:
    explicit BatchQueue(qs_ctx *ctx) : ctx_(ctx) {}
    BatchQueue(BatchQueue &&o) noexcept : ctx_(o.ctx_), live_(std::move(o.live_)) { o.ctx_ = nullptr; o.live_.clear(); }
    ~BatchQueue() { if (ctx_) { (void)qs_sync(ctx_); release(); } }
    // the batch is copied into pinned staging memory here (`b` may go away); the copy to the device runs on the library's copy
    // stream while the previous batch is still being counted; the count is asynchronous
    qs_device_batch *submit(const BatchFlat &b, bool want_ranges, uint32_t algo) {
        const qs_tree_batch hb = batch_view(b, want_ranges);
        if (live_.size() == 2) { qs_batch_free(ctx_, live_.front()); live_.erase(live_.begin()); }
        qs_device_batch *db = nullptr;
        if (qs_batch_upload(ctx_, &hb, &db) != QS_OK) fail();
        live_.push_back(db);
        if (qs_count_batch(ctx_, db, algo) != QS_OK) fail();
        return db;
    }
    void sync() { if (qs_sync(ctx_) != QS_OK) fail(); }
    void release() {   // after sync(): the batches are freed, the queue is done
        for (auto *db : live_) qs_batch_free(ctx_, db);
        live_.clear();
        ctx_ = nullptr;
    }
    void finish() { sync(); release(); }

private:
    qs_ctx *ctx_;
    std::vector<qs_device_batch *> live_;
    [[noreturn]] void fail() const { throw std::runtime_error(qs_last_error(ctx_)); }
};

// the device accumulators of the sharded scoring on the current device `dev`: sums, minima, candidates, allocated in this order
struct ScoreAcc {
    int dev;
    qs::DevBuf<int64_t> sums, mins, cand;
    ScoreAcc(int device, size_t P) : dev(device) {
        if (sums.reserve(P * 3 * 8, nullptr) != hipSuccess || mins.reserve(P * 8, nullptr) != hipSuccess ||
            cand.reserve(P * QS_SCORE_CAND_SLOTS * 8, nullptr) != hipSuccess)
            throw std::runtime_error("Insufficient memory!");
    }
    ~ScoreAcc() { (void)hipSetDevice(dev); }   // (runs in front of the buffers' hipFree)
};

// Scoring a table that exists only in parts (shards of one table, or one shard per GPU): pass 1 per part, the per-node-pair sums
// (wrapping 64-bit) and minima folded on the host, pass 2 per part against the GLOBAL minima, the candidate slots and overflow
// lists collected, qs_score_finish once on the host. P = qs_score_pair_slots.
class ScoreFold {
public:
    std::vector<int64_t> sums, mins, cand, extra;
    explicit ScoreFold(size_t P = 0, size_t n_parts = 0)
        : sums(P * 3, 0), mins(P, INT64_MAX), cand(n_parts * P * QS_SCORE_CAND_SLOTS), P_(P), n_parts_(n_parts) {}

    void pass1_launch(qs_ctx *ctx, const qs_ref_tree &rt, ScoreAcc &acc) const {
        if (qs_score_pass1(ctx, &rt, acc.sums.get(), acc.mins.get()) != QS_OK) throw std::runtime_error(qs_last_error(ctx));
    }
    void pass1_fold(const ScoreAcc &acc) {
        ScoreFold part(P_);
        hip_ok(hipMemcpy(part.sums.data(), acc.sums.get(), P_ * 3 * 8, hipMemcpyDeviceToHost), "copy of the score sums");
        hip_ok(hipMemcpy(part.mins.data(), acc.mins.get(), P_ * 8, hipMemcpyDeviceToHost), "copy of the score minima");
        merge(part);
    }
    void merge(const ScoreFold &o) {   // SUM of the sums, MIN of the minima (a few MB)
        for (size_t i = 0; i < P_ * 3; ++i) sums[i] = (int64_t)((uint64_t)sums[i] + (uint64_t)o.sums[i]);
        for (size_t i = 0; i < P_; ++i) mins[i] = std::min(mins[i], o.mins[i]);
    }
    void upload_mins(ScoreAcc &acc) const { hip_ok(hipMemcpy(acc.mins.get(), mins.data(), P_ * 8, hipMemcpyHostToDevice), "copy of the minima"); }
    void pass2_launch(qs_ctx *ctx, const qs_ref_tree &rt, ScoreAcc &acc) const {
        if (qs_score_pass2(ctx, &rt, acc.mins.get(), acc.cand.get()) != QS_OK) throw std::runtime_error(qs_last_error(ctx));
    }
    // the part's overflow list joins `extra`, its candidate slots go to slot `part` of `into` (another fold, or this one)
    void pass2_collect(qs_ctx *ctx, const qs_ref_tree &rt, ScoreAcc &acc, size_t part, ScoreFold &into) {
        int64_t *list = nullptr;
        uint64_t k = 0;
        if (qs_score_overflow(ctx, &rt, acc.mins.get(), acc.cand.get(), &list, &k) != QS_OK) throw std::runtime_error(qs_last_error(ctx));
        if (k) { extra.insert(extra.end(), list, list + 4 * k); qs_free_host(list); }
        const size_t slots = P_ * QS_SCORE_CAND_SLOTS;
        hip_ok(hipMemcpy(into.cand.data() + part * slots, acc.cand.get(), slots * 8, hipMemcpyDeviceToHost), "copy of the candidates");
    }
    EdgeScores finish(qs_ctx *ctx, const qs_ref_tree &rt, uint32_t flags) const {   // ctx may be NULL (host only)
        std::vector<double> lq(rt.n_nodes), qp(rt.n_nodes), eqp(rt.n_nodes);
        int bif = 0;
        if (qs_score_finish(ctx, &rt, flags, sums.data(), cand.data(), (uint32_t)n_parts_, extra.empty() ? nullptr : extra.data(), extra.size() / 4,
                            lq.data(), qp.data(), eqp.data(), &bif) != QS_OK)
            throw std::runtime_error(qs_last_error(ctx));
        return edge_scores(lq, qp, eqp, bif != 0);
    }

private:
    size_t P_, n_parts_;
};

} // namespace qsh
