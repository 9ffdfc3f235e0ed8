// qs_abi_score.hip -- scoring through the C-ABI: the flattened reference tree and its cache, the score passes over the table with their
// set-up, the host finish. Host code only; the kernels are in qs_score.hip.
#include "qs_ctx.hpp"

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <thread>
#include <vector>

using namespace qs;

// ---- scoring -----------------------------------------------------------------------------

// QuartetScoreComputer.hpp:135-159, evaluated with the host's libm like the reference.
static double host_log_score(uint64_t q1, uint64_t q2, uint64_t q3) {
    if (q1 == 0 && q2 == 0 && q3 == 0) return 0;
    uint64_t sum = q1 + q2 + q3;
    double p1 = (double)q1 / sum, p2 = (double)q2 / sum, p3 = (double)q3 / sum;
    double qic = 1;
    if (p1 != 0) qic += p1 * std::log(p1) / std::log(3);
    if (p2 != 0) qic += p2 * std::log(p2) / std::log(3);
    if (p3 != 0) qic += p3 * std::log(p3) / std::log(3);
    return (q1 < q2 || q1 < q3) ? qic * -1 : qic;
}


// the checks of a flattened reference tree, its depths, children counts and the id interval of every node
int qs::build_ref_shape(qs_ctx *c, const qs_ref_tree *ref, RefHost &R) {
    if (!ref || !ref->parent || !ref->leaf_node) return fail(c, QS_ERR_ARG, "reference tree: NULL arrays");
    if (c && ref->n_taxa != c->n) return fail(c, QS_ERR_ARG, "reference tree: n_taxa differs from the context");
    const uint32_t N = ref->n_nodes, n = ref->n_taxa;
    if (N < n + 1 || N > 65535) return fail(c, QS_ERR_ARG, "reference tree: bad node count");
    R.n_nodes = N; R.n = n;
    R.parent.assign(ref->parent, ref->parent + N);
    R.nchild.assign(N, 0); R.depth.assign(N, 0);
    int root = -1;
    for (uint32_t v = 0; v < N; ++v) {
        int p = R.parent[v];
        if (p < 0) { if (root >= 0) return fail(c, QS_ERR_ARG, "reference tree: several roots"); root = (int)v; }
        else if ((uint32_t)p >= N || (uint32_t)p == v) return fail(c, QS_ERR_ARG, "reference tree: bad parent");
        else R.nchild[p]++;
    }
    if (root < 0) return fail(c, QS_ERR_ARG, "reference tree: no root");
    R.root = (uint32_t)root;
    // depths (parents may come after children in the numbering: iterate with memo)
    std::vector<int> dep(N, -1);
    dep[root] = 0;
    std::vector<uint32_t> chain;
    for (uint32_t v = 0; v < N; ++v) {
        chain.clear();
        uint32_t x = v;
        while (dep[x] < 0) { chain.push_back(x); x = (uint32_t)R.parent[x]; if (chain.size() > N) return fail(c, QS_ERR_ARG, "reference tree: cycle"); }
        int dd = dep[x];
        for (size_t i = chain.size(); i-- > 0;) dep[chain[i]] = ++dd;
    }
    for (uint32_t v = 0; v < N; ++v) R.depth[v] = (uint32_t)dep[v];
    std::vector<uint8_t> is_leaf_taxon(N, 0);
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t v = ref->leaf_node[i];
        if (v >= N || R.nchild[v] != 0 || is_leaf_taxon[v]) return fail(c, QS_ERR_ARG, "reference tree: leaf_node must list distinct leaves");
        is_leaf_taxon[v] = 1;
    }
    uint32_t n_leaf_nodes = 0;
    for (uint32_t v = 0; v < N; ++v) if (R.nchild[v] == 0) n_leaf_nodes++;
    if (n_leaf_nodes != n) return fail(c, QS_ERR_ARG, "reference tree: number of leaves differs from n_taxa");
    // depth-first order check: every node's leaves form one contiguous id interval
    std::vector<uint32_t> lo(N, 0xFFFFFFFFu), hi(N, 0), cnt(N, 0);
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t x = ref->leaf_node[i];
        for (;;) {
            lo[x] = std::min(lo[x], i); hi[x] = std::max(hi[x], i); cnt[x]++;
            if (R.parent[x] < 0) break;
            x = (uint32_t)R.parent[x];
        }
    }
    for (uint32_t v = 0; v < N; ++v)
        if (cnt[v] && hi[v] - lo[v] + 1 != cnt[v])
            return fail(c, QS_ERR_ARG, "reference tree: lookup ids are not in depth-first leaf order");
    // is_bifurcating: max over nodes of (degree - 1) == 2 (QuartetScoreComputer.hpp:760)
    uint32_t max_rank = 0;
    for (uint32_t v = 0; v < N; ++v) {
        uint32_t deg = R.nchild[v] + (R.parent[v] >= 0 ? 1 : 0);
        if (deg >= 1) max_rank = std::max(max_rank, deg - 1);
    }
    R.bifurcating = (max_rank == 2);
    R.leaf_lo = lo; R.leaf_cnt = cnt;
    return QS_OK;
}

static int build_ref(qs_ctx *c, const qs_ref_tree *ref, RefHost &R) {
    if (int rc = build_ref_shape(c, ref, R)) return rc;
    const uint32_t N = R.n_nodes, n = R.n;
    const std::vector<uint32_t> &lo = R.leaf_lo, &cnt = R.leaf_cnt;
    R.root_deg2 = R.nchild[R.root] == 2;
    R.inner_id.assign(N, 0xFFFFFFFFu);
    R.inner_node.clear();
    for (uint32_t v = 0; v < N; ++v)
        if (R.nchild[v] > 0) { R.inner_id[v] = (uint32_t)R.inner_node.size(); R.inner_node.push_back(v); }
    R.n_inner = (uint32_t)R.inner_node.size();
    // LCA of leaves with adjacent ids, then running minima per row
    std::vector<uint32_t> adj(n > 0 ? n - 1 : 0);
    for (uint32_t i = 0; i + 1 < n; ++i) {
        uint32_t x = ref->leaf_node[i], y = ref->leaf_node[i + 1];
        while (x != y) {
            if (R.depth[x] >= R.depth[y]) x = (uint32_t)R.parent[x]; else y = (uint32_t)R.parent[y];
        }
        adj[i] = x;
    }
    R.lca.assign((size_t)n * n, 0);
    for (uint32_t i = 0; i + 1 < n; ++i) {
        uint32_t cur = adj[i];
        for (uint32_t j = i + 1; j < n; ++j) {
            if (j > i + 1 && R.depth[adj[j - 1]] < R.depth[cur]) cur = adj[j - 1];
            uint32_t e = (R.depth[cur] << 16) | R.inner_id[cur];
            R.lca[(size_t)i * n + j] = e;
            R.lca[(size_t)j * n + i] = e;
        }
    }
    if (R.bifurcating && R.root_deg2) {
        // QuartetScoreComputer.hpp:390-410 for u = root: S1 = the root's other child subtree, S2 = the child subtree that
        // holds v, S3 / S4 = v's child subtrees in depth-first order; all of them intervals of lookup ids
        std::vector<std::vector<uint32_t>> kids(N);
        for (uint32_t v = 0; v < N; ++v) if (R.parent[v] >= 0) kids[(uint32_t)R.parent[v]].push_back(v);
        for (auto &k : kids) std::sort(k.begin(), k.end(), [&](uint32_t p_, uint32_t q_) { return lo[p_] < lo[q_]; });
        const uint32_t rx = kids[R.root][0], ry = kids[R.root][1];
        R.root_split = cnt[rx];
        for (uint32_t v = 0; v < N; ++v) {
            if (v == R.root || R.nchild[v] != 2) continue;
            const bool in_x = lo[v] >= lo[rx] && lo[v] < lo[rx] + cnt[rx];
            const uint32_t mine = in_x ? rx : ry, other = in_x ? ry : rx;
            RootPairHost P{};
            P.s1_lo = lo[other]; P.s1_n = cnt[other]; P.s2_lo = lo[mine]; P.s2_n = cnt[mine];
            P.s3_lo = lo[kids[v][0]]; P.s3_n = cnt[kids[v][0]]; P.s4_lo = lo[kids[v][1]]; P.s4_n = cnt[kids[v][1]];
            const uint32_t ir = R.inner_id[R.root], iv = R.inner_id[v];
            P.key = std::min(ir, iv) * R.n_inner + std::max(ir, iv);
            P.first = R.root_items;
            R.root_items += (uint64_t)P.s1_n * P.s2_n * P.s3_n * P.s4_n;
            R.root_pairs.push_back(P);
        }
    }
    R.next.assign((size_t)n * n, 0);
    for (uint32_t b = 1; b < n; ++b) {
        R.next[(size_t)b * n + (b - 1)] = (uint16_t)b;
        for (uint32_t a = b - 1; a-- > 0;)
            R.next[(size_t)b * n + a] = R.lca[(size_t)b * n + a] != R.lca[(size_t)b * n + a + 1] ? (uint16_t)(a + 1) : R.next[(size_t)b * n + a + 1];
    }
    return QS_OK;
}

// The context's cached reference tree (host arrays + LCA matrix on the device when want_dev); rebuilt only when the
// caller passes a different tree.
int qs::get_ref(qs_ctx *c, const qs_ref_tree *ref, bool want_dev, const RefHost **out) {
    if (!ref || !ref->parent || !ref->leaf_node) return fail(c, QS_ERR_ARG, "reference tree: NULL arrays");
    RefHost *R = c->ref_cache.get();
    const bool same = R && R->n_nodes == ref->n_nodes && R->n == ref->n_taxa &&
                      memcmp(R->parent.data(), ref->parent, (size_t)ref->n_nodes * 4) == 0 &&
                      memcmp(R->leaf_node_in.data(), ref->leaf_node, (size_t)ref->n_taxa * 4) == 0;
    if (!same) {
        std::unique_ptr<RefHost> fresh(new RefHost());
        int rc = build_ref(c, ref, *fresh);
        if (rc != QS_OK) return rc;
        fresh->leaf_node_in.assign(ref->leaf_node, ref->leaf_node + ref->n_taxa);
        if (c->ref_lca_dev) { (void)hipStreamSynchronize(c->stream); c->ref_lca_dev.reset(); c->ref_next_dev.reset(); c->root_pairs_dev.reset(); }
        if (c->place_child_dev) { (void)hipStreamSynchronize(c->stream); c->place_child_dev.reset(); c->place_next_dev.reset(); c->place_node_dev.reset(); }
        if (c->branch_next_dev) { (void)hipStreamSynchronize(c->stream); c->branch_next_dev.reset(); c->branch_words_dev.reset(); c->branch_quartets_dev.reset(); }
        c->ref_cache = std::move(fresh);
        R = c->ref_cache.get();
        c->log_valid = false;
    }
    if (want_dev && !c->ref_lca_dev) {
        // The tree's device arrays are filled on the side and handed to the context together: ref_lca_dev says "all of them are
        // there", so a call that fails half-way leaves none behind (the context's own are empty here: nothing is held twice).
        DevBuf<uint32_t> lca; DevBuf<uint16_t> next; DevBuf<void> pairs;
        QS_HIP(c, lca.reserve(R->lca.size() * 4, nullptr));
        QS_HIP(c, next.reserve(R->next.size() * 2, nullptr));
        hipStream_t up = c->prep_stream ? c->prep_stream : c->stream;
        QS_HIP(c, hipMemcpyAsync(lca.get(), R->lca.data(), R->lca.size() * 4, hipMemcpyHostToDevice, up));
        QS_HIP(c, hipMemcpyAsync(next.get(), R->next.data(), R->next.size() * 2, hipMemcpyHostToDevice, up));
        if (!R->root_pairs.empty()) {
            QS_HIP(c, pairs.reserve(R->root_pairs.size() * sizeof(RootPairHost), nullptr));
            QS_HIP(c, hipMemcpyAsync(pairs.get(), R->root_pairs.data(), R->root_pairs.size() * sizeof(RootPairHost), hipMemcpyHostToDevice, up));
        }
        c->ref_lca_dev = std::move(lca); c->ref_next_dev = std::move(next); c->root_pairs_dev = std::move(pairs);
    }
    *out = R;
    return QS_OK;
}

// log(k) and 1/k for the integer arguments of the device QIC: every count and every tuple sum is at most the
// number of trees counted. Unknown (uploaded / attached tables, reduce-scattered shards): 65536 entries, larger
// values take the kernel's slow path.
int qs::ensure_score_tables(qs_ctx *c) {
    // every count and every tuple sum is at most the number of trees behind the table: what this context counted, or what
    // the caller says stands behind a reduced / uploaded / viewed table (QS_TUNE_TABLE_TREES)
    const uint64_t want64 = std::min<uint64_t>(std::max<uint64_t>(std::min<uint64_t>(std::max(std::max(c->trees_counted, c->table_trees_hint), c->collapse_max_count), 1ull << 20) + 1, 65536), 1ull << 20);
    const uint32_t want = (uint32_t)want64;
    if (c->tbl_n >= want) return QS_OK;
    c->tbl_n = 0;   // (entries that are valid, not the capacity: set again once the new table is on the device)
    std::vector<double> lk(want);
    lk[0] = 0.0;
    for (uint32_t k = 1; k < want; ++k) lk[k] = std::log((double)k);
    QS_HIP(c, c->dev_logk.reserve((size_t)want * 8, &c->stream));
    {   // (not the null stream: that one waits for count kernels still running on `stream`)
        hipStream_t up = c->prep_stream ? c->prep_stream : c->stream;
        QS_HIP(c, hipMemcpyAsync(c->dev_logk.get(), lk.data(), (size_t)want * 8, hipMemcpyHostToDevice, up));
        QS_HIP(c, hipStreamSynchronize(up));
    }
    c->tbl_n = want;
    return QS_OK;
}

void qs::fill_score_device(const qs_ctx *c, const RefHost &R, const uint32_t *lca_dev, ScoreDevice &sd) {
    sd.logk = c->dev_logk.get(); sd.tbl_n = c->tbl_n;
    // as much of the log table as fits goes to LDS (every tuple sum of up to 15743 trees); larger arguments are range-checked
    sd.coop_load = c->tune_score_load;
    sd.lds_n = (uint32_t)std::min<uint64_t>(c->tbl_n, score_scan_max_lds_log((c->tune_score_load == 1 || c->tune_score_load == 3) && c->tune_score_kernel == 0));
    sd.ref_lca = lca_dev; sd.ref_next = c->ref_next_dev.get(); sd.n = c->n; sd.n_inner = R.n_inner; sd.d_lo = c->d_lo; sd.d_hi = c->d_hi;
    sd.rank_lo = c->rank_lo; sd.n_tuples = c->n_tuples; sd.table = c->table; sd.count_bits = (int)c->count_bits;
    if (c->view_table) { sd.rank_lo = c->view_rank_lo; sd.n_tuples = c->view_n; sd.table = const_cast<void *>(c->view_table); sd.count_bits = (int)c->view_bits; }
    sd.pair_sums = nullptr; sd.pair_min = nullptr; sd.pair_cand = nullptr; sd.flags = c->dev_flags.get() + 1;
    sd.cand_limit = c->tune_cand_slots; sd.list = nullptr; sd.list_count = nullptr; sd.list_cap = 0; sd.last_trip = nullptr;
    sd.frame = R.bifurcating ? 0 : 1;
    sd.root_split = (R.bifurcating && R.root_deg2) ? R.root_split : 0u;
    sd.bundle_plo = sd.bundle_pcnt = sd.bundle_rounds = nullptr; sd.n_rounds = 0; sd.sample = 0;
}

// the bundle kernel's rounds for the rank range sd covers (own table, table shard or view): planned on the host, cached;
// pass 3 = the per-taxon pass (qs_taxon_support: its own slot and wave count, whatever the score tuning says)
int qs::ensure_bundle_plan(qs_ctx *c, ScoreDevice &sd, int pass) {
    sd.bundle_plo = sd.bundle_pcnt = sd.bundle_rounds = nullptr; sd.n_rounds = 0;
    if (c->tune_score_kernel == 1 && pass != 3) return QS_OK;
    if (int rc = ensure_n_cu(c)) return rc;
    const int w = pass - 1;
    BundlePlan &plan = c->bundle[w];
    const uint64_t r0 = sd.rank_lo, r1 = sd.rank_lo + sd.n_tuples;
    if (c->bundle_r0[w] != r0 || c->bundle_r1[w] != r1 || !c->bundle_dev[w]) {
        // (a new plan gets a table of its own size, never the old one's memory: kernels on `stream` may read that while `up` writes)
        if (c->bundle_dev[w]) { QS_HIP(c, hipStreamSynchronize(c->stream)); c->bundle_dev[w].reset(); }
        plan_bundles(c->n, r0, r1, pass == 3 ? (uint32_t)kTaxonWaves : score_bundle_waves(pass, c->tune_score_load == 1 || c->tune_score_load == 3), plan);
        const size_t words = 2 * (size_t)c->n + plan.rounds.size();
        if (c->bundle_dev[w].reserve(std::max<size_t>(words, 1) * 4, nullptr) != hipSuccess) return fail(c, QS_ERR_OOM, "qs_score: round table of the bundle kernel");
        uint32_t *const dev = c->bundle_dev[w].get();
        hipStream_t up = c->prep_stream ? c->prep_stream : c->stream;
        QS_HIP(c, hipMemcpyAsync(dev, plan.plo.data(), (size_t)c->n * 4, hipMemcpyHostToDevice, up));
        QS_HIP(c, hipMemcpyAsync(dev + c->n, plan.pcnt.data(), (size_t)c->n * 4, hipMemcpyHostToDevice, up));
        if (!plan.rounds.empty())
            QS_HIP(c, hipMemcpyAsync(dev + 2 * (size_t)c->n, plan.rounds.data(), plan.rounds.size() * 4, hipMemcpyHostToDevice, up));
        QS_HIP(c, hipStreamSynchronize(up));   // (the host vectors may be re-planned by the next call)
        c->bundle_r0[w] = r0; c->bundle_r1[w] = r1;
    }
    sd.bundle_plo = c->bundle_dev[w].get(); sd.bundle_pcnt = sd.bundle_plo + c->n; sd.bundle_rounds = sd.bundle_plo + 2 * (size_t)c->n;
    sd.n_rounds = (uint32_t)(plan.rounds.size() / 2);
    return QS_OK;
}

extern "C" int qs_score_set_view(qs_ctx *c, const void *table_dev, uint32_t count_bits, uint64_t rank_lo, uint64_t n_tuples) {
    if (c) c->log_valid = false;   // (the table / view / tuning may change: a logged pass 1 no longer describes it)
    if (!c) return QS_ERR_ARG;
    if (!table_dev) { c->view_table = nullptr; c->view_bits = 0; c->view_rank_lo = c->view_n = 0; return QS_OK; }
    if (count_bits != 16 && count_bits != 32) return fail(c, QS_ERR_ARG, "qs_score_set_view: count_bits must be 16 or 32");
    if (rank_lo > binom4(c->n) || n_tuples > binom4(c->n) - rank_lo) return fail(c, QS_ERR_ARG, "qs_score_set_view: rank range outside C(n,4)");
    c->view_table = table_dev; c->view_bits = count_bits; c->view_rank_lo = rank_lo; c->view_n = n_tuples;
    return QS_OK;
}

// qs_score's accumulators on the device and their pinned host copy, cached in the context
static int ensure_score_accumulators(qs_ctx *c, size_t np) {
    const size_t need_dev = np * (size_t)(3 + 1 + kCand) * 8, need_host = np * (size_t)(3 + kCand) * 8;
    QS_HIP(c, c->score_acc.reserve(need_dev, &c->stream));
    QS_HIP(c, c->score_acc_host.reserve(need_host, &c->stream));
    return QS_OK;
}

// the candidate log of the single-read scoring: records, the counter word, one word per node pair (tie filter)
static bool ensure_score_log(qs_ctx *c, size_t np) {
    const uint64_t want_cap = c->tune_score_log_cap ? c->tune_score_log_cap : (1ull << 23);   // 8 M records = 256 MB
    // (the counter sits behind the records: another capacity is another layout, and a buffer of its own size as before)
    if (c->score_log && c->score_log_cap != want_cap) { (void)hipStreamSynchronize(c->stream); c->score_log.reset(); }
    c->score_log_cap = 0;
    if (c->score_log.reserve((want_cap * 4 + 1 + np) * 8, &c->stream) != hipSuccess) { (void)hipGetLastError(); return false; }   // no room for the log: two passes
    c->score_log_cap = want_cap;
    return true;
}

// Is the single-read scoring wanted for the tuples sd covers? The bundle kernel over whole rows (bundle[0]: the plan of pass 1);
// QS_TUNE_SCORE_PASSES: 0 = automatic (tables from 1 GB, if there is a sample to predict the log from), 1 = never, 2 = always.
static bool want_score_log(const qs_ctx *c, const ScoreDevice &sd) {
    const uint64_t scored_bytes = sd.n_tuples * 3 * (uint64_t)(sd.count_bits / 8);
    return c->tune_score_kernel == 0 && c->bundle[0].n_parts == 0 &&
           (c->tune_score_passes == 2 || (c->tune_score_passes == 0 && c->tune_score_sample != 0 && scored_bytes >= (1ull << 30)));
}

extern "C" int qs_score_pass1(qs_ctx *c, const qs_ref_tree *ref, int64_t *sums_dev, int64_t *min_dev) {
    if (!c || !sums_dev || !min_dev) return fail(c, QS_ERR_ARG, "qs_score_pass1: NULL");
    if (!c->table && !c->view_table) return fail(c, QS_ERR_STATE, "qs_score_pass1: no table");
    QS_HIP(c, hipSetDevice(c->device));
    const RefHost *Rp = nullptr;
    int rc = get_ref(c, ref, true, &Rp);
    if (rc != QS_OK) return rc;
    const RefHost &R = *Rp;
    const size_t np = (size_t)R.n_inner * R.n_inner;
    QS_HIP(c, hipMemsetAsync(sums_dev, 0, np * 3 * 8, c->stream));
    QS_HIP(c, hipMemsetAsync(min_dev, 0x7F, np * 8, c->stream));
    { int rc_t = ensure_score_tables(c); if (rc_t != QS_OK) return rc_t; }
    ScoreDevice sd;
    fill_score_device(c, R, c->ref_lca_dev.get(), sd);
    sd.pair_sums = (unsigned long long *)sums_dev; sd.pair_min = (long long *)min_dev;
    { int rc_b = ensure_bundle_plan(c, sd, 1); if (rc_b != QS_OK) return rc_b; }
    // Single-read scoring: this pass also LOGS every quartet whose device QIC is within the tolerance of the bound it knows for
    // its node pair (the pair's minimum in memory, lowered beforehand by a minima-only pre-pass over a sample of the table, and
    // the lane's own running minimum) -- a superset of the quartets within the tolerance of ANY later minimum <= this table's,
    // so the qs_score_pass2 that follows filters the log instead of reading the table again, also when its min_dev holds the
    // minima over several shards / GPUs (QuartetScoreComputer.hpp:417-469 evaluates log_score of every quartet once, too).
    // QS_TUNE_SCORE_PASSES: 0 = automatic (tables from 1 GB, whole rows, bundle kernel; a second sample predicts the log and
    // the pass runs plain when it would not hold), 1 = never, 2 = always (pass 2 reads the table if the log overflows).
    c->log_valid = false;
    c->last_score_estimate = 0;
    // (sd.n_rounds: pass 1's plan as ensure_bundle_plan has just left it -- a plan without rounds has nothing to log)
    bool logging = want_score_log(c, sd) && sd.n_rounds > 0 && ensure_score_log(c, np);
    if (logging) {
        sd.list = c->score_log.get(); sd.list_count = sd.list + 4 * c->score_log_cap; sd.list_cap = c->score_log_cap;
        QS_HIP(c, hipMemsetAsync(sd.list_count, 0, 8, c->stream));
        if (c->tune_score_dedupe) {   // the tie filter (one word per node pair behind the log's counter)
            sd.last_trip = sd.list_count + 1;
            QS_HIP(c, hipMemsetAsync(sd.last_trip, 0xFF, np * 8, c->stream));
        }
        if (c->tune_score_sample) {   // minima-only pre-pass over a sample of the table: the bound the logging pass starts from
            ScoreDevice pre = sd;
            pre.list = nullptr; pre.list_count = nullptr; pre.list_cap = 0; pre.sample = c->tune_score_sample;
            QS_HIP(c, launch_score_pass1(c->stream, pre, 0, c->n_cu, nullptr, nullptr, 0, 0.0));
            if (c->tune_score_passes != 2) {
                // automatic mode: a second, disjoint sample counts what the logging pass would log of it
                pre.list_count = sd.list_count; pre.sample = c->tune_score_sample | (1u << 17);
                QS_HIP(c, launch_score_pass1(c->stream, pre, 0, c->n_cu, nullptr, nullptr, 0, c->tune_score_tol));
                unsigned long long hits = 0;
                QS_HIP(c, hipMemcpyAsync(&hits, sd.list_count, 8, hipMemcpyDeviceToHost, c->stream));
                QS_HIP(c, hipStreamSynchronize(c->stream));
                c->last_score_estimate = hits * (c->tune_score_sample & 0xFFFFu);
                // The static bounds of the sample over-predict: the full pass also lowers the minima as it goes, a lane keeps its
                // own running minimum, and the tie filter has seen 64 x more of every node pair (measured, predicted / logged:
                // 12.6 M / 1.6 M at 512 taxa x 10000 random trees, 3.7 M / 0.75 M at 256 taxa, 19 M / 1.0 M at 512 taxa x 10000
                // reference + NNI trees; without the tie filter those predict 90 M and do overflow 8 M): go ahead up to 6 x the log.
                if ((double)c->last_score_estimate > 6.0 * (double)c->score_log_cap) {
                    logging = false;
                    sd.list = nullptr; sd.list_count = nullptr; sd.list_cap = 0;
                } else {
                    QS_HIP(c, hipMemsetAsync(sd.list_count, 0, 8, c->stream));
                    if (sd.last_trip) QS_HIP(c, hipMemsetAsync(sd.last_trip, 0xFF, np * 8, c->stream));   // (the estimate logged nothing)
                }
            }
        }
        // waves reserve whole chunks of records: what they leave unwritten must read as "no record" (key = all ones)
        if (logging) {
            QS_HIP(c, hipMemsetAsync(sd.list, 0xFF, (size_t)c->score_log_cap * 32, c->stream));
            c->log_valid = true;                 // until the table, the view or the tuning changes (invalidate_log)
            c->log_table = sd.table; c->log_rank_lo = sd.rank_lo; c->log_n_tuples = sd.n_tuples; c->log_ref = Rp; c->log_tol = c->tune_score_tol;
        }
    }
    QS_HIP(c, launch_score_pass1(c->stream, sd, c->tune_score_kernel, c->n_cu, c->bundle[0].part_lo, c->bundle[0].part_n, c->bundle[0].n_parts, c->tune_score_tol));
    // rooted reference (degree-2 root): the sums of the node pairs (root, v) as the reference enumerates them (quirk Q5)
    if (c->root_pairs_dev) QS_HIP(c, launch_root_pair_sums(c->stream, sd, c->root_pairs_dev.get(), (uint32_t)R.root_pairs.size(), R.root_items));
    return QS_OK;   // asynchronous on the context's stream
}

// Everything a first qs_score pays before its kernels -- reference tree + LCA matrix on the device, log table, the bundle
// kernel's round tables, the accumulators with their pinned host copy, the candidate log, the kernels' code objects' first
// use of the device-to-host copy path -- done ahead of time. Safe while count kernels of this context are still running (same
// host thread): the uploads go through the copy stream, nothing waits for `stream`. The CLI calls it after the last batch
// is enqueued, where the host would only wait: the scoring phase of 512 taxa x 10000 trees drops from 28 to ~15 ms.
extern "C" int qs_score_prepare(qs_ctx *c, const qs_ref_tree *ref, uint64_t n_trees_total) {
    if (!c || !ref) return fail(c, QS_ERR_ARG, "qs_score_prepare: NULL");
    QS_HIP(c, hipSetDevice(c->device));
    if (!c->copy_stream) QS_HIP(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
    // every exit path -- also the error returns below -- leaves the copy stream drained: what was uploaded through it is marked
    // present in the context, and the kernels of a later qs_score run on `stream`, which has no ordering against `copy_stream`
    struct Restore { qs_ctx *c; ~Restore() { c->prep_stream = nullptr; (void)hipStreamSynchronize(c->copy_stream); } } restore{c};
    c->prep_stream = c->copy_stream;
    const RefHost *Rp = nullptr;
    int rc = get_ref(c, ref, true, &Rp);
    if (rc != QS_OK) return rc;
    const size_t np = (size_t)Rp->n_inner * Rp->n_inner;
    if (np == 0) return fail(c, QS_ERR_ARG, "qs_score_prepare: bad reference tree");
    const uint64_t keep_hint = c->table_trees_hint;
    c->table_trees_hint = std::max<uint64_t>(c->table_trees_hint, n_trees_total);   // size the log table for the finished table
    rc = ensure_score_tables(c);
    c->table_trees_hint = keep_hint;
    if (rc != QS_OK) return rc;
    ScoreDevice sd;
    fill_score_device(c, *Rp, c->ref_lca_dev.get(), sd);
    rc = ensure_bundle_plan(c, sd, 1);
    if (rc == QS_OK) rc = ensure_bundle_plan(c, sd, 2);
    if (rc != QS_OK) return rc;
    rc = ensure_score_accumulators(c, np);
    if (rc != QS_OK) return rc;
    // (without pass 1's "the plan has rounds": sd holds pass 2's plan here, and a log that is never used costs only its memory)
    if (want_score_log(c, sd)) (void)ensure_score_log(c, np);
    for (hipEvent_t &e : c->score_ev) if (!e) QS_HIP(c, hipEventCreate(&e));
    // first use of the pinned accumulator copy by the device (the first device-to-host copy into freshly pinned memory took 7 ms)
    QS_HIP(c, hipMemcpyAsync(c->score_acc_host.get(), c->score_acc.get(), np * (size_t)(3 + kCand) * 8, hipMemcpyDeviceToHost, c->copy_stream));
    QS_HIP(c, hipStreamSynchronize(c->copy_stream));
    return QS_OK;
}

extern "C" int qs_score_pass2(qs_ctx *c, const qs_ref_tree *ref, const int64_t *min_dev, int64_t *cand_dev) {
    if (!c || !min_dev || !cand_dev) return fail(c, QS_ERR_ARG, "qs_score_pass2: NULL");
    if (!c->table && !c->view_table) return fail(c, QS_ERR_STATE, "qs_score_pass2: no table");
    QS_HIP(c, hipSetDevice(c->device));
    const RefHost *Rp = nullptr;
    int rc = get_ref(c, ref, true, &Rp);
    if (rc != QS_OK) return rc;
    const RefHost &R = *Rp;
    const size_t np = (size_t)R.n_inner * R.n_inner;
    QS_HIP(c, hipMemsetAsync(cand_dev, 0xFF, np * kCand * 8, c->stream));
    QS_HIP(c, hipMemsetAsync(c->dev_flags.get() + 1, 0, 4, c->stream));
    { int rc_t = ensure_score_tables(c); if (rc_t != QS_OK) return rc_t; }
    ScoreDevice sd;
    fill_score_device(c, R, c->ref_lca_dev.get(), sd);
    sd.pair_min = (long long *)min_dev; sd.pair_cand = (unsigned long long *)cand_dev;
    c->last_score_log = 0;
    if (c->log_valid && c->log_table == sd.table && c->log_rank_lo == sd.rank_lo && c->log_n_tuples == sd.n_tuples && c->log_ref == Rp &&
        c->log_tol == c->tune_score_tol) {
        // the preceding qs_score_pass1 over this very table logged its candidates: filter the log against min_dev
        c->log_valid = false;
        unsigned long long n_rec = 0;
        QS_HIP(c, hipMemcpyAsync(&n_rec, c->score_log.get() + 4 * c->score_log_cap, 8, hipMemcpyDeviceToHost, c->stream));
        QS_HIP(c, hipStreamSynchronize(c->stream));
        // A counter that reached the capacity is an overflow: waves reserve chunks of 64 records, the capacity is a multiple
        // of 64, so the counter can stop exactly AT the capacity while waves that found the log full at the start of a row
        // have skipped their hits without moving it. Only a log with room left is known to be complete.
        if (n_rec < c->score_log_cap) {
            sd.list = c->score_log.get(); sd.list_cap = c->score_log_cap;
            QS_HIP(c, launch_score_log(c->stream, sd, c->tune_score_tol, n_rec));
            c->last_score_log = n_rec;
            return QS_OK;
        }
        // (the log overflowed: read the table)
    }
    { int rc_b = ensure_bundle_plan(c, sd, 2); if (rc_b != QS_OK) return rc_b; }
    QS_HIP(c, launch_score_pass2(c->stream, sd, c->tune_score_tol, c->tune_score_kernel, c->n_cu, c->bundle[1].part_lo, c->bundle[1].part_n, c->bundle[1].n_parts));
    return QS_OK;   // asynchronous; node pairs whose slots did not suffice are marked in cand_dev (qs_score_overflow)
}

// Node pairs that pass 2 could not finish in their 8 packed slots (more than 8 distinct near-minimal triples, or a
// gcd-reduced count >= 2^21) carry kCandOverflow in their last slot. For those pairs the table is scanned once more
// and EVERY near-minimal quartet's (key, q1, q2, q3) is listed; the list is sorted and de-duplicated on the host and
// handed to qs_score_finish, which takes the exact minimum over it. The reference evaluates log_score for every
// quartet (QuartetScoreComputer.hpp:417-469), so any superset of the minimisers gives its result.
extern "C" int qs_score_overflow(qs_ctx *c, const qs_ref_tree *ref, const int64_t *min_dev, const int64_t *cand_dev,
                                 int64_t **list_out, uint64_t *n_out) {
    if (!c || !min_dev || !cand_dev || !list_out || !n_out) return fail(c, QS_ERR_ARG, "qs_score_overflow: NULL");
    *list_out = nullptr; *n_out = 0;
    QS_HIP(c, hipSetDevice(c->device));
    uint32_t fl = 0;
    QS_HIP(c, hipMemcpyAsync(&fl, c->dev_flags.get() + 1, 4, hipMemcpyDeviceToHost, c->stream));
    QS_HIP(c, hipStreamSynchronize(c->stream));
    if ((fl & 3u) == 0) return QS_OK;
    const RefHost *Rp = nullptr;
    int rc = get_ref(c, ref, true, &Rp);
    if (rc != QS_OK) return rc;
    ScoreDevice sd;
    fill_score_device(c, *Rp, c->ref_lca_dev.get(), sd);
    sd.pair_min = (long long *)const_cast<int64_t *>(min_dev); sd.pair_cand = (unsigned long long *)const_cast<int64_t *>(cand_dev);
    DevBuf<unsigned long long> cnt, list;
    QS_HIP(c, cnt.reserve(8, nullptr));
    uint64_t cap = 1ull << 20;
    std::vector<unsigned long long> host;
    for (int attempt = 0; attempt < 2; ++attempt) {
        if (list.reserve(cap * 32, nullptr) != hipSuccess) return fail(c, QS_ERR_OOM, "qs_score_overflow: list of " + std::to_string(cap) + " quartets does not fit");
        QS_HIP(c, hipMemsetAsync(cnt.get(), 0, 8, c->stream));
        sd.list = list.get(); sd.list_count = cnt.get(); sd.list_cap = cap;
        QS_HIP(c, launch_score_overflow_list(c->stream, sd, c->tune_score_tol));
        unsigned long long got = 0;
        QS_HIP(c, hipMemcpyAsync(&got, cnt.get(), 8, hipMemcpyDeviceToHost, c->stream));
        QS_HIP(c, hipStreamSynchronize(c->stream));
        if (got <= cap) {
            host.resize(got * 4);
            if (got) QS_HIP(c, hipMemcpy(host.data(), list.get(), got * 32, hipMemcpyDeviceToHost));
            break;
        }
        if (attempt == 1 || got > (1ull << 28)) return fail(c, QS_ERR_OVERFLOW, "qs_score_overflow: " + std::to_string(got) + " near-minimal quartets");
        cap = got;
    }
    // sort + unique the 4-word records
    const size_t n = host.size() / 4;
    std::vector<size_t> idx(n);
    for (size_t i = 0; i < n; ++i) idx[i] = i;
    auto less = [&](size_t x, size_t y) { return std::lexicographical_compare(&host[4 * x], &host[4 * x] + 4, &host[4 * y], &host[4 * y] + 4); };
    std::sort(idx.begin(), idx.end(), less);
    std::vector<unsigned long long> uniq;
    for (size_t i = 0; i < n; ++i)
        if (i == 0 || less(idx[i - 1], idx[i])) uniq.insert(uniq.end(), &host[4 * idx[i]], &host[4 * idx[i]] + 4);
    if (!uniq.empty()) {
        int64_t *out = (int64_t *)malloc(uniq.size() * 8);
        if (!out) return fail(c, QS_ERR_OOM, "qs_score_overflow: host list");
        memcpy(out, uniq.data(), uniq.size() * 8);
        *list_out = out; *n_out = uniq.size() / 4;
    }
    return QS_OK;
}

extern "C" void qs_free_host(void *p) { free(p); }

// QS_SCORE_SAVEMEM_LOOKUPS + a degree-2 reference root. For a node pair (root, v) the reference calls
// countQuartetOccurrences(a, b, c, d) with a in S1 (the root's other side), b in S2 = ALL leaves on v's side, c in S3, d in S4
// (v's child subtrees; QuartetScoreComputer.hpp:393-396,412-424): b repeats c or d. Its compact table sorts the ids
// (quartet_lookup_table.hpp:170-212) and the const get_tuple throws std::runtime_error("id = ..., but quartet_lookup_.size() =
// ...") when the index C(t1,4)+C(t2,3)+C(t3,2)+t4 of the sorted ids t1 >= t2 >= t3 >= t4 lies behind the table (:79-85), e.g.
// whenever the two largest are both n-1: for every rooted reference tree with 4 or more taxa some call does (proved case by
// case in DESIGN.md 1, checked on the unmodified header in tests/test_oracle_reftable.py). The exception is not caught
// anywhere in the reference: its run ends there. This finds the FIRST throwing call in the reference's sequential order
// (pairs by node index; a, b, c, d nested in that order, each ascending) without walking the O(n^4) calls: the index is
// monotone in every id, so the calls of a prefix throw iff the one with the largest remaining ids does.
static uint64_t dup_index(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {   // lookup_index_ on ids that may repeat
    uint32_t t[4] = {a, b, c, d};
    std::sort(t, t + 4);
    return binom4(t[3]) + binom3(t[2]) + binom2(t[1]) + t[0];
}
static bool first_compact_throw(const RefHost &R, uint64_t nq, uint64_t *id_out) {
    for (const RootPairHost &P : R.root_pairs) {
        if (!P.s1_n || !P.s3_n || !P.s4_n) continue;
        const uint32_t a_hi = P.s1_lo + P.s1_n - 1, c_hi = P.s3_lo + P.s3_n - 1, d_hi = P.s4_lo + P.s4_n - 1;
        // the largest index any call of this pair reaches: b repeats the largest c or the largest d
        if (std::max(dup_index(a_hi, c_hi, c_hi, d_hi), dup_index(a_hi, d_hi, c_hi, d_hi)) < nq) continue;
        for (uint32_t a = P.s1_lo; a <= a_hi; ++a) {
            if (std::max(dup_index(a, c_hi, c_hi, d_hi), dup_index(a, d_hi, c_hi, d_hi)) < nq) continue;
            for (uint32_t b = P.s2_lo; b < P.s2_lo + P.s2_n; ++b) {
                const bool in3 = b >= P.s3_lo && b <= c_hi, in4 = b >= P.s4_lo && b <= d_hi;
                if (in3) {            // calls (a, b, c = b, d), d ascending: a throwing d exists iff the largest throws
                    if (dup_index(a, b, b, d_hi) < nq) continue;
                    for (uint32_t d = P.s4_lo; d <= d_hi; ++d)
                        if (dup_index(a, b, b, d) >= nq) { *id_out = dup_index(a, b, b, d); return true; }
                } else if (in4) {     // calls (a, b, c, d = b), c ascending
                    if (dup_index(a, b, c_hi, b) < nq) continue;
                    for (uint32_t c = P.s3_lo; c <= c_hi; ++c)
                        if (dup_index(a, b, c, b) >= nq) { *id_out = dup_index(a, b, c, b); return true; }
                }
            }
        }
    }
    return false;
}
static int check_savemem_lookups(qs_ctx *c, const RefHost &R, uint32_t flags) {
    if (!(flags & QS_SCORE_SAVEMEM_LOOKUPS) || (flags & QS_SCORE_ROOT_AS_EDGE) || !R.bifurcating || !R.root_deg2) return QS_OK;
    const uint64_t nq = binom4(R.n);
    uint64_t id = 0;
    if (!first_compact_throw(R, nq, &id)) return QS_OK;
    return fail(c, QS_ERR_REFERENCE_THROWS, "id = " + std::to_string(id) + ", but quartet_lookup_.size() = " + std::to_string(nq));
}

// Host-only: what qs_score / qs_score_finish would refuse for this reference tree and these flags, found from the tree alone
// (before any counting): today the QS_SCORE_SAVEMEM_LOOKUPS + rooted-reference case. ctx may be NULL.
extern "C" int qs_score_check(qs_ctx *c, const qs_ref_tree *ref, uint32_t flags) {
    if (!ref) return fail(c, QS_ERR_ARG, "qs_score_check: NULL");
    RefHost local;
    const RefHost *Rp = &local;
    const int rc = c ? get_ref(c, ref, false, &Rp) : build_ref(nullptr, ref, local);
    if (rc != QS_OK) return rc;
    return check_savemem_lookups(c, *Rp, flags);
}

// Pure host: log_score of the O(#node pairs) candidates and sums with the host libm
// (QuartetScoreComputer.hpp:135-159), then the min-propagation along path(u,v) (:448-454, :472-489).
extern "C" int qs_score_finish(qs_ctx *c, const qs_ref_tree *ref, uint32_t flags, const int64_t *sums_host,
                               const int64_t *cand_host, uint32_t n_cand_parts, const int64_t *extra_host, uint64_t n_extra,
                               double *lqic, double *qpic, double *eqpic, int *is_bifurcating) {
    if (!sums_host || !cand_host || !lqic || n_cand_parts == 0) return fail(c, QS_ERR_ARG, "qs_score_finish: NULL");
    RefHost local;          // ctx == NULL: pure host use (no device, no cache)
    const RefHost *Rp = &local;
    int rc = c ? get_ref(c, ref, false, &Rp) : build_ref(nullptr, ref, local);
    if (rc != QS_OK) return rc;
    const RefHost &R = *Rp;
    const bool root_as_edge = (flags & QS_SCORE_ROOT_AS_EDGE) != 0;
    if (is_bifurcating) *is_bifurcating = R.bifurcating ? 1 : 0;
    { int rc_s = check_savemem_lookups(c, R, flags); if (rc_s != QS_OK) return rc_s; }
    if (R.bifurcating && (!qpic || !eqpic)) return fail(c, QS_ERR_ARG, "qs_score: qpic/eqpic required for a bifurcating reference");
    const size_t np = (size_t)R.n_inner * R.n_inner;
    const unsigned long long *sums = (const unsigned long long *)sums_host;
    const unsigned long long *cand = (const unsigned long long *)cand_host;
    // extra candidates (qs_score_overflow lists, any order): key -> range in a sorted copy
    std::vector<std::array<unsigned long long, 4>> extra;
    // A record flagged kListSwap / a slot flagged kCandSwap is a quartet the reference evaluates twice for a degree-2 root, the
    // second time with q2 and q3 exchanged (qs_score.hip root_swapped; QuartetScoreComputer.hpp:393-396,417-454): both orders
    // enter the minimum. QS_SCORE_ROOT_AS_EDGE does not reproduce the reference's root pairs, hence not this either.
    const bool both_orders = !root_as_edge;
    if (extra_host && n_extra) {
        extra.reserve(n_extra);
        for (uint64_t i = 0; i < n_extra; ++i) {
            const unsigned long long *e = (const unsigned long long *)extra_host + 4 * i;
            extra.push_back({e[0] & 0xFFFFFFFFull, e[1], e[2], e[3]});
            if ((e[0] & kListSwap) && both_orders) extra.push_back({e[0] & 0xFFFFFFFFull, e[1], e[3], e[2]});
        }
        std::sort(extra.begin(), extra.end());
    }
    const double inf = std::numeric_limits<double>::infinity();
    const uint32_t N = R.n_nodes;
    for (uint32_t v = 0; v < N; ++v) {
        lqic[v] = inf;
        if (R.bifurcating) { qpic[v] = inf; eqpic[v] = inf; }
    }
    // The O(#node pairs) finalisation runs on a few host threads for large references. Each thread folds a contiguous
    // range of iu (pairs are visited in (iu, iv) order) into private vectors; merging the ranges in order reproduces
    // the sequential result exactly, including which of two equal minima / which of two writers of a QP value wins.
    struct Local { std::vector<double> lq, qp, eqp; std::vector<uint8_t> qp_set; };
    auto fold = [&](uint32_t iu0, uint32_t iu1, Local &out) {
        out.lq.assign(N, inf);
        if (R.bifurcating) { out.qp.assign(N, inf); out.eqp.assign(N, inf); out.qp_set.assign(N, 0); }
        for (uint32_t iu = iu0; iu < iu1; ++iu)
            for (uint32_t iv = iu + 1; iv < R.n_inner; ++iv) {
                const size_t key = (size_t)iu * R.n_inner + iv;
                double lqmin = inf;
                bool any = false;
                for (uint32_t part = 0; part < n_cand_parts; ++part) {
                    const unsigned long long *cs = cand + ((size_t)part * np + key) * kCand;
                    for (int s = 0; s < kCand && cs[s] != kCandEmpty; ++s) {
                        if (cs[s] == kCandOverflow) continue;   // marker: this pair's full list is in `extra`
                        const uint64_t q1 = (cs[s] >> 42) & 0x1FFFFFu, q2 = (cs[s] >> 21) & 0x1FFFFFu, q3 = cs[s] & 0x1FFFFFu;
                        const double v = host_log_score(q1, q2, q3);
                        lqmin = std::min(lqmin, v);
                        if ((cs[s] & kCandSwap) && both_orders) lqmin = std::min(lqmin, host_log_score(q1, q3, q2));
                        any = true;
                    }
                }
                if (!extra.empty()) {
                    const std::array<unsigned long long, 4> lo_key = {(unsigned long long)key, 0, 0, 0};
                    for (auto it = std::lower_bound(extra.begin(), extra.end(), lo_key); it != extra.end() && (*it)[0] == key; ++it) {
                        lqmin = std::min(lqmin, host_log_score((*it)[1], (*it)[2], (*it)[3]));
                        any = true;
                    }
                }
                if (!any) continue; // pair owns no resolved quartet
                uint64_t p1 = sums[key * 3], p2 = sums[key * 3 + 1], p3 = sums[key * 3 + 2];
                if (!(flags & QS_SCORE_QP_EXACT64)) { p1 &= 0xFFFFFFFFull; p2 &= 0xFFFFFFFFull; p3 &= 0xFFFFFFFFull; } // QSC:382
                const double qp = host_log_score(p1, p2, p3);
                // walk the path u..v (edges are indexed by their child node)
                uint32_t x = R.inner_node[iu], y = R.inner_node[iv];
                uint32_t path_edges = 0, last_edge_a = 0, last_edge_b = 0;
                while (x != y) {
                    uint32_t e;
                    if (R.depth[x] >= R.depth[y]) { e = x; x = (uint32_t)R.parent[x]; }
                    else { e = y; y = (uint32_t)R.parent[y]; }
                    out.lq[e] = std::min(out.lq[e], lqmin);
                    if (R.bifurcating) out.eqp[e] = std::min(out.eqp[e], qp);
                    if (path_edges == 0) last_edge_a = e; else last_edge_b = e;
                    ++path_edges;
                }
                if (R.bifurcating) {
                    const bool through_deg2_root = root_as_edge && path_edges == 2 && x == R.root && R.nchild[R.root] == 2;
                    if (path_edges == 1) { out.qp[last_edge_a] = qp; out.qp_set[last_edge_a] = 1; }
                    else if (through_deg2_root) { out.qp[last_edge_a] = qp; out.qp[last_edge_b] = qp; out.qp_set[last_edge_a] = out.qp_set[last_edge_b] = 1; }
                }
            }
    };
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    const unsigned workers = R.n_inner >= 128 ? std::min(8u, hw) : 1u;
    std::vector<Local> parts(workers + 1);
    if (workers == 1) fold(0, R.n_inner, parts[0]);
    else {
        // ranges of iu with about the same number of pairs (row iu has n_inner - 1 - iu of them)
        std::vector<uint32_t> cut(workers + 1, R.n_inner);
        const uint64_t total = (uint64_t)R.n_inner * (R.n_inner - 1) / 2;
        uint64_t acc = 0;
        uint32_t w = 1;
        cut[0] = 0;
        for (uint32_t iu = 0; iu < R.n_inner && w < workers; ++iu) {
            acc += R.n_inner - 1 - iu;
            while (w < workers && acc >= total * w / workers) cut[w++] = iu + 1;
        }
        std::vector<std::thread> pool;
        for (unsigned k = 0; k < workers; ++k) pool.emplace_back([&, k] { fold(cut[k], cut[k + 1], parts[k]); });
        for (auto &th : pool) th.join();
    }
    if (R.bifurcating && R.root_deg2 && !root_as_edge) {
        // Reference-compatible handling of a degree-2 root (quirk Q5, QuartetScoreComputer.hpp:393-396,472-489): every
        // pair (root, v) has its own sums (root_pair_sums_kernel); QP-IC of the edge if v is a child of the root, EQP-IC
        // minimum along the path. (Pairs are visited with u = root first in the reference: these come before all others.)
        Local &L = parts[workers];
        L.lq.assign(N, inf); L.qp.assign(N, inf); L.eqp.assign(N, inf); L.qp_set.assign(N, 0);
        for (const RootPairHost &P : R.root_pairs) {
            uint64_t p1 = sums[(size_t)P.key * 3], p2 = sums[(size_t)P.key * 3 + 1], p3 = sums[(size_t)P.key * 3 + 2];
            if (!(flags & QS_SCORE_QP_EXACT64)) { p1 &= 0xFFFFFFFFull; p2 &= 0xFFFFFFFFull; p3 &= 0xFFFFFFFFull; }
            const double qp = host_log_score(p1, p2, p3);
            const uint32_t iu = P.key / R.n_inner, iv = P.key % R.n_inner;
            uint32_t v = R.inner_node[iu] == R.root ? R.inner_node[iv] : R.inner_node[iu];
            if ((uint32_t)R.parent[v] == R.root) { L.qp[v] = qp; L.qp_set[v] = 1; }
            for (uint32_t x = v; x != R.root; x = (uint32_t)R.parent[x]) L.eqp[x] = std::min(L.eqp[x], qp);
        }
        std::rotate(parts.begin(), parts.begin() + workers, parts.end());   // merged first
    } else parts.pop_back();
    for (const Local &L : parts) // in range order
        for (uint32_t v = 0; v < N; ++v) {
            lqic[v] = std::min(lqic[v], L.lq[v]);
            if (R.bifurcating) {
                eqpic[v] = std::min(eqpic[v], L.eqp[v]);
                if (L.qp_set[v]) qpic[v] = L.qp[v];
            }
        }
    return QS_OK;
}

extern "C" int qs_score(qs_ctx *c, const qs_ref_tree *ref, uint32_t flags, double *lqic, double *qpic, double *eqpic,
                        int *is_bifurcating) {
    if (!c || !lqic) return fail(c, QS_ERR_ARG, "qs_score: NULL");
    if (!c->table) return fail(c, QS_ERR_STATE, "qs_score: no table");
    if (c->d_lo != 0 || c->d_hi != c->n)
        return fail(c, QS_ERR_UNSUPPORTED, "qs_score: this context owns a table shard; use qs_score_pass1 / qs_score_pass2 / "
                                           "qs_score_finish with reductions over the shards in between");
    const size_t np = (size_t)qs_score_pair_slots(ref);
    if (np == 0) return fail(c, QS_ERR_ARG, "qs_score: bad reference tree");
    QS_HIP(c, hipSetDevice(c->device));
    using clk = std::chrono::steady_clock;
    auto ms_since = [](clk::time_point t) { return std::chrono::duration<float, std::milli>(clk::now() - t).count(); };
    const clk::time_point t_all = clk::now();
    for (hipEvent_t &e : c->score_ev) if (!e) QS_HIP(c, hipEventCreate(&e));
    for (float &x : c->score_ms) x = 0;
    // the accumulators (sums, minima, candidate slots: 24 MB at 512 taxa) and their pinned host copy live in the context: three
    // hipMalloc / hipFree pairs and a pageable 22 MB copy per call were 1 ms of a 15 ms call
    struct Ptr { void *p; } sums{nullptr}, mn{nullptr}, cand{nullptr};
    { int rc_a = ensure_score_accumulators(c, np); if (rc_a != QS_OK) return rc_a; }
    sums.p = c->score_acc.get(); mn.p = (char *)sums.p + np * 3 * 8; cand.p = (char *)sums.p + np * 4 * 8;
    {   // the cached pieces both passes need (reference tree + LCA matrix, log table, bundle plans): built here so that
        // the first call's set-up cost shows as its own phase and the events below bracket kernels only
        const RefHost *Rp = nullptr;
        int rc0 = get_ref(c, ref, true, &Rp);
        if (rc0 != QS_OK) return rc0;
        rc0 = check_savemem_lookups(c, *Rp, flags);      // (the reference throws during its scoring loop: before any kernel here)
        if (rc0 != QS_OK) return rc0;
        rc0 = ensure_score_tables(c);
        if (rc0 != QS_OK) return rc0;
    }
    c->score_ms[1] = ms_since(t_all);
    QS_HIP(c, hipEventRecord(c->score_ev[0], c->stream));
    int rc = qs_score_pass1(c, ref, (int64_t *)sums.p, (int64_t *)mn.p);     // (may log its candidates: see there)
    if (rc != QS_OK) return rc;
    QS_HIP(c, hipEventRecord(c->score_ev[1], c->stream));
    rc = qs_score_pass2(c, ref, (const int64_t *)mn.p, (int64_t *)cand.p);   // a filter over that log, or the second read
    if (rc != QS_OK) return rc;
    QS_HIP(c, hipEventRecord(c->score_ev[2], c->stream));
    const clk::time_point t_ov = clk::now();
    int64_t *extra = nullptr;
    uint64_t n_extra = 0;
    rc = qs_score_overflow(c, ref, (const int64_t *)mn.p, (const int64_t *)cand.p, &extra, &n_extra);   // synchronises the stream
    if (rc != QS_OK) return rc;
    struct FreeHost { int64_t *p; ~FreeHost() { free(p); } } free_extra{extra};
    // The accumulators come home through the COPY stream (the count stream is idle: qs_score_overflow has just synchronised
    // it). The first large device-to-host copy enqueued on a stream that has run kernels costs ~8 ms on the host, once per
    // stream (tools/d2h_cold.hip); a stream that only ever copies does not pay it -- that was most of a first call's
    // "wait + copies" phase.
    int64_t *hs = (int64_t *)c->score_acc_host.get(), *hc = hs + np * 3;
    if (!c->copy_stream) QS_HIP(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
    QS_HIP(c, hipMemcpyAsync(hs, sums.p, np * 3 * 8, hipMemcpyDeviceToHost, c->copy_stream));
    QS_HIP(c, hipMemcpyAsync(hc, cand.p, np * kCand * 8, hipMemcpyDeviceToHost, c->copy_stream));
    QS_HIP(c, hipStreamSynchronize(c->copy_stream));
    (void)hipEventElapsedTime(&c->score_ms[2], c->score_ev[0], c->score_ev[1]);
    (void)hipEventElapsedTime(&c->score_ms[3], c->score_ev[1], c->score_ev[2]);
    c->score_ms[4] = ms_since(t_ov);            // waiting for the passes + overflow pass (if any) + the accumulators' way back
    const clk::time_point t_fin = clk::now();
    rc = qs_score_finish(c, ref, flags, hs, hc, 1, extra, n_extra, lqic, qpic, eqpic, is_bifurcating);
    c->score_ms[5] = ms_since(t_fin);
    c->score_ms[0] = ms_since(t_all);
    return rc;
}

// Phases of the last qs_score call in ms: [0] whole call (host clock), [1] set-up (accumulator allocation, reference tree
// + LCA matrix, log table; near zero once cached), [2] pass 1 and [3] pass 2 (HIP events on the context's stream: kernels
// + the bundle plan of a first call), [4] host wait for the passes incl. overflow pass and device-to-host copies,
// [5] qs_score_finish (host libm + min-propagation).
// Records the candidate log of the most recent qs_score held (single-read mode); 0 = it took two passes over the table.
extern "C" uint64_t qs_last_score_log(const qs_ctx *c) { return c ? c->last_score_log : 0; }
extern "C" uint64_t qs_last_score_estimate(const qs_ctx *c) { return c ? c->last_score_estimate : 0; }

extern "C" int qs_last_score_ms(qs_ctx *c, float out_ms[6]) {
    if (!c || !out_ms) return QS_ERR_ARG;
    for (int i = 0; i < 6; ++i) out_ms[i] = c->score_ms[i];
    return QS_OK;
}

static int raw_qic_impl(qs_ctx *c, const qs_ref_tree *ref, uint64_t r0, uint64_t nq, uint8_t *topo, uint64_t *q, bool lex) {
    if (!c || !c->table) return fail(c, QS_ERR_STATE, "qs_raw_qic: no table");
    if (r0 + nq > c->n_tuples) return fail(c, QS_ERR_ARG, "qs_raw_qic: rank range outside this context's table");
    if (lex && (c->d_lo != 0 || c->d_hi != c->n)) return fail(c, QS_ERR_UNSUPPORTED, "qs_raw_qic_lex: needs the whole table (not a shard)");
    if (nq == 0) return QS_OK;
    QS_HIP(c, hipSetDevice(c->device));
    const RefHost *Rp = nullptr;
    int rc = get_ref(c, ref, true, &Rp);
    if (rc != QS_OK) return rc;
    const RefHost &R = *Rp;
    DevBuf<uint8_t> dt_mem; DevBuf<unsigned long long> dq_mem;   // (freed on every way out; hipFree waits for the device)
    QS_HIP(c, dt_mem.reserve(nq, nullptr));
    if (dq_mem.reserve(nq * 24, nullptr) != hipSuccess) return fail(c, QS_ERR_OOM, "qs_raw_qic: hipMalloc");
    uint8_t *const dt = dt_mem.get(); unsigned long long *const dq = dq_mem.get();
    { int rc_t = ensure_score_tables(c); if (rc_t != QS_OK) return rc_t; }
    ScoreDevice sd;
    fill_score_device(c, R, c->ref_lca_dev.get(), sd);
    sd.frame = 1; // printRawQICScores uses the multifurcating loop's argument order
    hipError_t e = lex ? launch_raw_qic_lex(c->stream, sd, r0, nq, dt, dq) : launch_raw_qic(c->stream, sd, r0, nq, dt, dq);
    if (e == hipSuccess) e = hipMemcpyAsync(topo, dt, nq, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(q, dq, nq * 24, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, QS_ERR_HIP, std::string("qs_raw_qic: ") + hipGetErrorString(e));
    return QS_OK;
}

extern "C" int qs_raw_qic(qs_ctx *c, const qs_ref_tree *ref, uint64_t r0, uint64_t nq, uint8_t *topo, uint64_t *q) {
    return raw_qic_impl(c, ref, r0, nq, topo, q, false);
}
extern "C" int qs_raw_qic_lex(qs_ctx *c, const qs_ref_tree *ref, uint64_t i0, uint64_t nq, uint8_t *topo, uint64_t *q) {
    return raw_qic_impl(c, ref, i0, nq, topo, q, true);
}
