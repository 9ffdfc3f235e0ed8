// tree_distances.hpp -- the host side of `QuartetScores --tree-distances FILE`: the flattened batches are kept while they are counted,
// uploaded once more as ONE batch after the last count, compared pair by pair (qs_tree_pair_agreement, upper triangle) in blocks of rows
// and written as one TSV line per pair a < b. What needs no device (the kept batches, the row blocks, the lines) stands apart from the
// calls, so that a sanitizer build can drive it alone (tools/asan_tree_distances.cpp).
#pragma once

#include "host_common.hpp"
#include "ingest.hpp"

#include <algorithm>
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

namespace qsh {

constexpr size_t kPairWordsHost = 5;                       // concordant, discordant, resolved_row, resolved_col, shared
constexpr size_t kPairBlockBytes = size_t(256) << 20;      // the device buffer of one row block stays within this

// rows of one call for m trees: whole rows of m pairs, at least one, the buffer within `budget` bytes and the pairs within 2^28
inline size_t pair_block_rows(size_t m, size_t budget = kPairBlockBytes) {
    if (m == 0) return 1;
    const size_t by_bytes = budget / (m * kPairWordsHost * 8), by_pairs = (size_t(1) << 28) / m;
    return std::max<size_t>(1, std::min(std::min(by_bytes, by_pairs), m));
}

inline const char *pair_header() { return "a\tb\ttaxa\tquartets\tconcordant\tdiscordant\ta_only\tb_only\tunresolved\tconcordance\tdistance\n"; }

// one line of the file from the five words of the pair (a, b); the two ratios as %.6f, or nan where their denominator is 0
inline void append_pair_line(std::string &out, size_t a, size_t b, const uint64_t *w) {
    const uint64_t c = w[0], d = w[1], ao = w[2] - c - d, bo = w[3] - c - d, n = w[4], q = c4(n);
    char conc[32], dist[32], line[320];
    if (c + d) std::snprintf(conc, sizeof conc, "%.6f", (double)c / (double)(c + d));
    else std::snprintf(conc, sizeof conc, "nan");
    if (q) std::snprintf(dist, sizeof dist, "%.6f", (double)(d + ao + bo) / (double)q);
    else std::snprintf(dist, sizeof dist, "nan");
    std::snprintf(line, sizeof line, "%zu\t%zu\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%s\t%s\n", a, b, (unsigned long long)n,
                  (unsigned long long)q, (unsigned long long)c, (unsigned long long)d, (unsigned long long)ao, (unsigned long long)bo,
                  (unsigned long long)(q - c - d - ao - bo), conc, dist);
    out += line;
}

// the lines of row a of an m x m square from the words of that row ([m][5]): the pairs a < b
inline void append_row_lines(std::string &out, size_t a, size_t m, const uint64_t *row_words) {
    for (size_t b = a + 1; b < m; ++b) append_pair_line(out, a, b, row_words + b * kPairWordsHost);
}

struct TreeDistances {
    BatchFlat all;   // every counted batch, in file order
    void hook(DeviceOptions &opt) {
        add_after_count(opt, [this](qs_ctx *, const qs_device_batch *, size_t, const BatchFlat &b) { append_batch(all, b); });
    }
    // after the last count: one upload with ranges, the upper triangle in row blocks, the lines streamed out
    void write(qs_ctx *ctx, int device, const std::string &path, size_t budget = kPairBlockBytes) const {
        std::ofstream f(path);
        if (!f) throw std::runtime_error("cannot write " + path);
        f << pair_header();
        const size_t m = all.n_trees;
        if (m >= 2) {
            const qs_tree_batch hb = batch_view(all, true);
            qs_device_batch *db = nullptr;
            if (qs_batch_upload(ctx, &hb, &db) != QS_OK) throw std::runtime_error(std::string("--tree-distances: ") + qs_last_error(ctx));
            struct Free { qs_ctx *c; qs_device_batch *b; ~Free() { (void)qs_sync(c); qs_batch_free(c, b); } } guard{ctx, db};
            const size_t rows = pair_block_rows(m, budget);
            qs::DevBuf<uint64_t> dev;
            if (hipSetDevice(device) != hipSuccess || dev.reserve(rows * m * kPairWordsHost * 8, nullptr) != hipSuccess)
                throw std::runtime_error("--tree-distances: Insufficient memory!");
            std::vector<uint64_t> words(rows * m * kPairWordsHost);
            std::string lines;
            for (size_t r0 = 0; r0 + 1 < m; r0 += rows) {   // (the last tree's row holds no pair a < b)
                const size_t r1 = std::min(m, r0 + rows);
                if (qs_tree_pair_agreement(ctx, db, (uint32_t)r0, (uint32_t)r1, db, 0, (uint32_t)m, QS_PAIRS_UPPER, dev.get()) != QS_OK || qs_sync(ctx) != QS_OK)
                    throw std::runtime_error(std::string("--tree-distances: ") + qs_last_error(ctx));
                if (hipMemcpy(words.data(), dev.get(), (r1 - r0) * m * kPairWordsHost * 8, hipMemcpyDeviceToHost) != hipSuccess)
                    throw std::runtime_error("--tree-distances: download failed");
                for (size_t a = r0; a < r1; ++a) {
                    lines.clear();
                    append_row_lines(lines, a, m, words.data() + (a - r0) * m * kPairWordsHost);
                    f << lines;
                }
            }
        }
        if (!f) throw std::runtime_error("cannot write " + path);
    }
};

} // namespace qsh
