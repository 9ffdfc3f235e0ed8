// sanitizer driver for the host drivers' shared pieces (host_common.hpp; AddressSanitizer + UBSan, CPU only): BatchQueue, ScoreFold,
// edge_scores and the two views against stubs of the C-ABI and the HIP runtime whose allocators count -- a double free, a free
// of an unknown pointer and a leak at exit abort.   make -C tools asan && tools/bin/asan_host_driver
#include "host_common.hpp"

#include <cstdlib>
#include <cstring>
#include <iostream>
#include <new>
#include <set>
using namespace qsh;

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); std::abort(); } } while (0)

// ---- counting allocator behind every stub that hands out memory
static std::set<void *> live;
static void *take(size_t bytes) { void *p = std::malloc(bytes ? bytes : 1); live.insert(p); return p; }
static void give(void *p) { CHECK(live.erase(p) == 1); std::free(p); }   // unknown pointer or second free: abort

// ---- the scripted context: failures by call number, the partial results of its score passes
struct qs_device_batch { uint32_t n_trees; };
struct qs_ctx {
    int uploads = 0, counts = 0, syncs = 0, alive = 0, most_alive = 0;
    int fail_upload = 0, fail_count = 0, fail_sync = 0;   // fail the k-th call (0 = never)
    std::vector<int64_t> sums, mins, cand, overflow;      // what pass 1 / pass 2 / qs_score_overflow of this part hand out
};
static uint32_t finish_parts;
static uint64_t finish_extra;
static int finish_bif;

extern "C" {
const char *qs_last_error(const qs_ctx *ctx) { return ctx ? "scripted failure" : "scripted failure (no context)"; }
int qs_batch_upload(qs_ctx *c, const qs_tree_batch *b, qs_device_batch **out) {
    if (++c->uploads == c->fail_upload) return QS_ERR_OOM;
    *out = new (take(sizeof(qs_device_batch))) qs_device_batch{b->n_trees};
    c->most_alive = std::max(c->most_alive, ++c->alive);
    return QS_OK;
}
void qs_batch_free(qs_ctx *c, qs_device_batch *b) { --c->alive; give(b); }
int qs_count_batch(qs_ctx *c, const qs_device_batch *, uint32_t) { return ++c->counts == c->fail_count ? QS_ERR_OOM : QS_OK; }
int qs_sync(qs_ctx *c) { return ++c->syncs == c->fail_sync ? QS_ERR_OOM : QS_OK; }
int qs_score(qs_ctx *, const qs_ref_tree *r, uint32_t, double *lq, double *qp, double *eqp, int *bif) {
    for (uint32_t v = 0; v < r->n_nodes; ++v) { lq[v] = v; qp[v] = 10 + v; eqp[v] = 20 + v; }
    *bif = finish_bif;
    return QS_OK;
}
int qs_score_pass1(qs_ctx *c, const qs_ref_tree *, int64_t *sums_dev, int64_t *min_dev) {
    std::memcpy(sums_dev, c->sums.data(), c->sums.size() * 8);
    std::memcpy(min_dev, c->mins.data(), c->mins.size() * 8);
    return QS_OK;
}
int qs_score_pass2(qs_ctx *c, const qs_ref_tree *, const int64_t *, int64_t *cand_dev) { std::memcpy(cand_dev, c->cand.data(), c->cand.size() * 8); return QS_OK; }
int qs_score_overflow(qs_ctx *c, const qs_ref_tree *, const int64_t *, const int64_t *, int64_t **list_out, uint64_t *n_out) {
    *n_out = c->overflow.size() / 4;
    *list_out = *n_out ? (int64_t *)take(c->overflow.size() * 8) : nullptr;
    if (*n_out) std::memcpy(*list_out, c->overflow.data(), c->overflow.size() * 8);
    return QS_OK;
}
void qs_free_host(void *p) { give(p); }
int qs_score_finish(qs_ctx *c, const qs_ref_tree *r, uint32_t f, const int64_t *, const int64_t *, uint32_t n_parts, const int64_t *extra, uint64_t n_extra,
                    double *lq, double *qp, double *eqp, int *bif) {
    CHECK((extra == nullptr) == (n_extra == 0));
    finish_parts = n_parts; finish_extra = n_extra;
    return qs_score(c, r, f, lq, qp, eqp, bif);
}
hipError_t hipMalloc(void **p, size_t bytes) { *p = take(bytes); return hipSuccess; }
hipError_t hipFree(void *p) { give(p); return hipSuccess; }
hipError_t hipHostMalloc(void **p, size_t bytes, unsigned) { *p = take(bytes); return hipSuccess; }
hipError_t hipHostFree(void *p) { give(p); return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipMemcpy(void *dst, const void *src, size_t bytes, hipMemcpyKind) { std::memcpy(dst, src, bytes); return hipSuccess; }
const char *hipGetErrorString(hipError_t) { return "stub"; }
}

template <typename F> static bool throws(F f) { try { f(); } catch (const std::runtime_error &) { return true; } return false; }

static void batch_queue() {
    BatchFlat b;
    b.n_trees = 1;
    {   // five submits and finish: never more than two alive, one sync, nothing left
        qs_ctx c;
        BatchQueue q(&c);
        for (int i = 0; i < 5; ++i) { CHECK(q.submit(b, false, 0)->n_trees == 1); CHECK(c.alive <= 2); }
        q.finish();
        CHECK(c.uploads == 5 && c.counts == 5 && c.most_alive == 2 && c.alive == 0 && c.syncs == 1);
    }
    for (int what = 0; what < 3; ++what) {   // the third upload / the third count / the sync of finish() fails
        qs_ctx c;
        (what == 0 ? c.fail_upload : what == 1 ? c.fail_count : c.fail_sync) = what == 2 ? 1 : 3;
        CHECK(throws([&] { BatchQueue q(&c); for (int i = 0; i < 5; ++i) q.submit(b, true, 0); q.finish(); }));
        CHECK(c.alive == 0 && c.uploads == (what == 2 ? 5 : 3) && c.syncs == (what == 2 ? 2 : 1));   // the queue waited and freed
    }
    {   // destruction with batches alive
        qs_ctx c;
        { BatchQueue q(&c); q.submit(b, false, 0); q.submit(b, false, 0); CHECK(c.alive == 2); }
        CHECK(c.alive == 0 && c.syncs == 1);
    }
    {   // move: the batches go with the queue, the moved-from one neither waits nor frees
        qs_ctx c;
        {
            BatchQueue q(&c);
            q.submit(b, false, 0);
            { BatchQueue q2(std::move(q)); q2.submit(b, false, 0); q2.sync(); CHECK(c.alive == 2); q2.release(); }
            CHECK(c.alive == 0 && c.syncs == 1);
        }
        CHECK(c.syncs == 1);
    }
}

static void score_fold() {
    const size_t P = 3, S = QS_SCORE_CAND_SLOTS;
    RefFlat rf;
    rf.parent = {-1, 0, 0, 0}; rf.leaf_node = {1, 2, 3}; rf.names = {"a", "b", "c"};
    const qs_ref_tree rt = ref_view(rf);
    qs_ctx part[2];
    part[0].sums = {(int64_t)0xFFFFFFFFFFFFFFF0ull, 1, INT64_MAX, 0, 0, 0, 0, 0, 7};   // + part 1: wraps past 2^64 and past 2^63
    part[1].sums = {0x20, 2, 1, 0, 0, 0, 0, 0, -9};
    part[0].mins = {5, INT64_MAX, INT64_MAX};
    part[1].mins = {7, 2, INT64_MAX};
    for (int g = 0; g < 2; ++g) for (size_t i = 0; i < P * S; ++i) part[g].cand.push_back(100 * (g + 1) + (int64_t)i);
    part[1].overflow = {1, 2, 3, 4, 5, 6, 7, 8};   // k = 2; part 0: k = 0, no list
    ScoreFold direct(P, 2), per_gpu[2] = {ScoreFold(P), ScoreFold(P)}, merged(P, 2);
    {
        ScoreAcc acc(0, P);
        for (int g = 0; g < 2; ++g) {
            direct.pass1_launch(&part[g], rt, acc); direct.pass1_fold(acc);
            per_gpu[g].pass1_launch(&part[g], rt, acc); per_gpu[g].pass1_fold(acc);
            merged.merge(per_gpu[g]);
        }
        CHECK(direct.sums == (std::vector<int64_t>{0x10, 3, INT64_MIN, 0, 0, 0, 0, 0, -2}));
        CHECK(direct.mins == (std::vector<int64_t>{5, 2, INT64_MAX}));
        CHECK(merged.sums == direct.sums && merged.mins == direct.mins);
        direct.upload_mins(acc);
        CHECK(std::memcmp(acc.mins.get(), direct.mins.data(), P * 8) == 0);
        for (int g = 0; g < 2; ++g) {   // candidates into their own slot of the fold itself and of another one
            direct.pass2_launch(&part[g], rt, acc); direct.pass2_collect(&part[g], rt, acc, (size_t)g, direct);
            per_gpu[g].pass2_launch(&part[g], rt, acc); per_gpu[g].pass2_collect(&part[g], rt, acc, (size_t)(1 - g), merged);
        }
    }
    for (size_t i = 0; i < P * S; ++i) {
        CHECK(direct.cand[i] == 100 + (int64_t)i && direct.cand[P * S + i] == 200 + (int64_t)i);
        CHECK(merged.cand[i] == 200 + (int64_t)i && merged.cand[P * S + i] == 100 + (int64_t)i);
    }
    CHECK(direct.extra == part[1].overflow && per_gpu[0].extra.empty() && per_gpu[1].extra == part[1].overflow && merged.extra.empty());
    finish_bif = 1;
    const EdgeScores bif = direct.finish(nullptr, rt, 0);
    CHECK(finish_parts == 2 && finish_extra == 2 && bif.bifurcating);
    CHECK(bif.lq == (std::vector<double>{1, 2, 3}) && bif.qp == (std::vector<double>{11, 12, 13}) && bif.eqp == (std::vector<double>{21, 22, 23}));
    finish_bif = 0;
    const EdgeScores multi = merged.finish(&part[0], rt, 0);
    CHECK(finish_parts == 2 && finish_extra == 0 && !multi.bifurcating && multi.lq == bif.lq && multi.qp.empty() && multi.eqp.empty());
    CHECK(score_table(&part[0], rt, 0).lq == bif.lq);
}

static void views() {
    RefFlat rf;
    rf.parent = {-1, 0, 0}; rf.leaf_node = {1, 2}; rf.names = {"x", "y"};
    const qs_ref_tree rt = ref_view(rf);
    CHECK(rt.n_nodes == 3 && rt.n_taxa == 2 && rt.parent == rf.parent.data() && rt.leaf_node == rf.leaf_node.data());
    BatchFlat b;
    b.n_trees = 2; b.leaf_ids = {0, 1, 1, 0}; b.leaf_off = {0, 2, 4}; b.adj_depth = {0, 0, 0, 0}; b.ranges = {0, 1};
    const qs_tree_batch with = batch_view(b, true), without = batch_view(b, false);
    CHECK(with.n_trees == 2 && with.leaf_off == b.leaf_off.data() && with.leaf_ids == b.leaf_ids.data() && with.adj_depth == b.adj_depth.data());
    CHECK(with.node_off == b.node_off.data() && with.rng_off == b.rng_off.data() && with.ranges == b.ranges.data());
    CHECK(without.node_off == nullptr && without.rng_off == nullptr && without.ranges == b.ranges.data() && without.leaf_ids == with.leaf_ids);
    DeviceOptions o;
    CHECK(score_flags(o) == QS_SCORE_QP_WRAP32);
    o.qp_exact64 = o.root_as_edge = o.savemem_lookups = true;
    CHECK(score_flags(o) == (QS_SCORE_QP_EXACT64 | QS_SCORE_ROOT_AS_EDGE | QS_SCORE_SAVEMEM_LOOKUPS));
    CHECK(c4(3) == 0 && c4(4) == 1 && c4(24) == 10626 && c4(4096) == 11710951848960ull);
    CHECK(throws([&] { check_device_range(o, 2, 1); }) && !throws([&] { check_device_range(o, 2, 2); }));
    o.gpus_on_one_device = true;
    CHECK(!throws([&] { check_device_range(o, 3, 1); }));
}

int main() {
    batch_queue();
    score_fold();
    views();
    CHECK(live.empty());   // a leak
    std::cout << "host drivers: count queue, score fold, views and edge scores ran clean" << std::endl;
    return 0;
}
