// sanitizer driver for the host side of --tree-distances (tree_distances.hpp; AddressSanitizer + UBSan, CPU only): the chained
// after_count / after_sync callbacks, the kept batches, the row blocks and the lines, and TreeDistances::write against stubs of the
// C-ABI and the HIP runtime whose allocator counts -- a free of an unknown pointer and a leak at exit abort.
//   make -C tools asan && tools/bin/asan_tree_distances
#include "tree_distances.hpp"

#include <cstdlib>
#include <cstring>
#include <filesystem>
#include <set>
#include <sstream>
using namespace qsh;

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); std::abort(); } } while (0)

static std::set<void *> live;
static void *take(size_t bytes) { void *p = std::malloc(bytes ? bytes : 1); live.insert(p); return p; }
static void give(void *p) { CHECK(live.erase(p) == 1); std::free(p); }

struct qs_device_batch { uint32_t n_trees; };
struct qs_ctx { int uploads = 0, calls = 0, fail_call = 0; size_t most_words = 0; };

// the words the scripted device hands out for the pair (a, b)
static void pair_words(uint64_t a, uint64_t b, uint64_t *w) {
    const uint64_t n = 4 + (a + b) % 5, q = c4(n), c = (a * 7 + b) % (q + 1), d = (q - c) / 2;
    w[0] = c; w[1] = d; w[2] = c + d; w[3] = c + d + (q - c - d) / 3; w[4] = (a + b) % 7 == 0 ? 3 : n;
    if (w[4] < 4) w[0] = w[1] = w[2] = w[3] = 0;
}

extern "C" {
const char *qs_last_error(const qs_ctx *) { return "scripted failure"; }
int qs_batch_upload(qs_ctx *c, const qs_tree_batch *b, qs_device_batch **out) {
    CHECK(b->node_off && b->rng_off && b->ranges);
    ++c->uploads;
    *out = new (take(sizeof(qs_device_batch))) qs_device_batch{b->n_trees};
    return QS_OK;
}
void qs_batch_free(qs_ctx *, qs_device_batch *b) { give(b); }
int qs_sync(qs_ctx *) { return QS_OK; }
int qs_tree_pair_agreement(qs_ctx *c, const qs_device_batch *rows, uint32_t r0, uint32_t r1, const qs_device_batch *cols, uint32_t c0,
                           uint32_t c1, uint32_t flags, uint64_t *dst) {
    CHECK(rows == cols && flags == QS_PAIRS_UPPER && r0 < r1 && r1 <= rows->n_trees && c0 == 0 && c1 == cols->n_trees);
    if (++c->calls == c->fail_call) return QS_ERR_OOM;
    c->most_words = std::max<size_t>(c->most_words, (size_t)(r1 - r0) * c1 * 5);
    for (uint32_t a = r0; a < r1; ++a)
        for (uint32_t b = 0; b < c1; ++b) {
            uint64_t *w = dst + ((size_t)(a - r0) * c1 + b) * 5;   // (a write past the caller's buffer is the sanitizer's to find)
            if (b > a) pair_words(a, b, w); else std::memset(w, 0, 40);
        }
    return QS_OK;
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

static BatchFlat some_batch(uint32_t trees, uint32_t leaves) {   // `trees` stars of `leaves` leaves: one node of `leaves` links each
    BatchFlat b;
    for (uint32_t t = 0; t < trees; ++t) {
        for (uint32_t i = 0; i < leaves; ++i) { b.leaf_ids.push_back((uint16_t)i); b.adj_depth.push_back(0); b.ranges.push_back((uint16_t)i); b.ranges.push_back((uint16_t)((i + 1) % leaves)); }
        b.leaf_off.push_back((uint32_t)b.leaf_ids.size());
        b.rng_off.push_back((uint32_t)(b.ranges.size() / 2));
        b.node_off.push_back((uint32_t)(b.rng_off.size() - 1));
    }
    b.n_trees = trees;
    return b;
}

static void blocks_and_lines() {
    CHECK(pair_block_rows(0) == 1 && pair_block_rows(1) == 1);
    CHECK(pair_block_rows(1000) == 1000);                        // 40 MB: one call
    CHECK(pair_block_rows(10000) == (size_t(256) << 20) / 400000);
    CHECK(pair_block_rows(10000) * 400000 <= (size_t(256) << 20));
    CHECK(pair_block_rows(100, 40 * 100 * 7 + 39) == 7);
    CHECK(pair_block_rows(100, 10) == 1);                        // a row that does not fit goes alone
    CHECK(pair_block_rows(size_t(1) << 20) * (size_t(1) << 20) <= (size_t(1) << 28));
    std::string s;
    const uint64_t w[5] = {10, 3, 14, 13, 6};                    // C(6,4) = 15: a_only 1, b_only 0, unresolved 1
    append_pair_line(s, 2, 9, w);
    CHECK(s == "2\t9\t6\t15\t10\t3\t1\t0\t1\t0.769231\t0.266667\n");
    s.clear();
    const uint64_t z[5] = {0, 0, 0, 0, 3};
    append_pair_line(s, 0, 1, z);
    CHECK(s == "0\t1\t3\t0\t0\t0\t0\t0\t0\tnan\tnan\n");
    s.clear();
    const uint64_t big[5] = {~0ull / 8, 5, ~0ull / 8 + 5, ~0ull / 8 + 5, 65535};   // the widest numbers still fit a line
    append_pair_line(s, 4000000000u, 4000000001u, big);
    CHECK(s.back() == '\n' && std::count(s.begin(), s.end(), '\t') == 10);
}

static void hooks_and_write() {
    DeviceOptions opt;
    std::vector<int> order;
    add_after_count(opt, [&](qs_ctx *, const qs_device_batch *, size_t, const BatchFlat &) { order.push_back(1); });
    add_after_sync(opt, [&](qs_ctx *) { order.push_back(10); });
    TreeDistances td;
    td.hook(opt);
    add_after_count(opt, [&](qs_ctx *, const qs_device_batch *, size_t, const BatchFlat &) { order.push_back(2); });
    add_after_sync(opt, [&](qs_ctx *) { order.push_back(20); });
    size_t m = 0;
    for (uint32_t trees : {3u, 1u, 5u, 2u}) {
        const BatchFlat b = some_batch(trees, 4 + trees);
        opt.after_count(nullptr, nullptr, m, b);
        m += trees;
    }
    opt.after_sync(nullptr);
    CHECK((order == std::vector<int>{1, 2, 1, 2, 1, 2, 1, 2, 10, 20}));
    CHECK(td.all.n_trees == m && td.all.leaf_off.size() == m + 1 && td.all.node_off.size() == m + 1 && td.all.rng_off.size() == m + 1);
    CHECK(td.all.leaf_off.back() == td.all.leaf_ids.size() && td.all.rng_off.back() * 2 == td.all.ranges.size());
    for (size_t t = 0; t < m; ++t) CHECK(td.all.node_off[t + 1] == t + 1 && td.all.rng_off[t + 1] - td.all.rng_off[t] == td.all.leaf_off[t + 1] - td.all.leaf_off[t]);

    std::string want = pair_header();
    for (size_t a = 0; a < m; ++a)
        for (size_t b = a + 1; b < m; ++b) { uint64_t w[5]; pair_words(a, b, w); append_pair_line(want, a, b, w); }
    const std::string path = (std::filesystem::temp_directory_path() / "asan_tree_distances.tsv").string();
    for (size_t budget : {size_t(256) << 20, size_t(40 * 11 * 4), size_t(40 * 11 * 3 + 1), size_t(1)}) {   // one block, 4-row, 3-row and 1-row blocks
        qs_ctx c;
        td.write(&c, 0, path, budget);
        std::ifstream f(path);
        std::stringstream got;
        got << f.rdbuf();
        CHECK(got.str() == want);
        const size_t rows = pair_block_rows(m, budget);
        CHECK(c.uploads == 1 && c.calls == (int)((m - 1 + rows - 1) / rows) && c.most_words <= rows * m * 5 && live.empty());
    }
    {   // the second call fails: the batch and the buffer are released
        qs_ctx c;
        c.fail_call = 2;
        bool threw = false;
        try { td.write(&c, 0, path, 40 * 11 * 3); } catch (const std::runtime_error &) { threw = true; }
        CHECK(threw && live.empty());
    }
    {   // fewer than two trees: the header alone, nothing uploaded
        TreeDistances one;
        one.all = some_batch(1, 5);
        qs_ctx c;
        one.write(&c, 0, path);
        std::ifstream f(path);
        std::stringstream got;
        got << f.rdbuf();
        CHECK(got.str() == pair_header() && c.uploads == 0);
    }
    std::remove(path.c_str());
}

int main() {
    blocks_and_lines();
    hooks_and_write();
    CHECK(live.empty());
    std::puts("asan_tree_distances: ok");
    return 0;
}
