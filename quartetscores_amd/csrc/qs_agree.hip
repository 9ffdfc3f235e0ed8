// qs_agree.hip -- per-tree quartet agreement of the evaluation trees with the reference tree on gfx950 (qs_tree_agreement).
//
// For evaluation tree t with taxon set P_t (N = |P_t|) and the reference restricted to P_t, four exact counts over the
// C(N,4) quartets: concordant, discordant, resolved in t, resolved in the reference. No quartet is enumerated: a resolved
// quartet ab|cd is claimed by exactly two inner nodes of a tree (the two junctions of its a-b and c-d paths), so the
// counts are sums over node pairs (u of the reference, v of t) of closed forms in the matrix I[r][c] = |A_r & B_c & P_t|
// of their links (tests/agreement_model.py is the numpy model).
//
// A workgroup owns (tree t, a block of t's inner nodes). It builds in LDS the id bitmap of P_t and of every link of its
// nodes, each word paired with the popcount of the words before it, so that the number of a link's leaves in an id
// interval is two LDS reads. The reference's links are id intervals: the children of u split u's id interval, the parent
// link is the rest. Each lane takes reference nodes u and walks the block's nodes v. A binary pair (3 x 3) needs six
// interval counts and runs unrolled; other degrees go through the loops of pair_terms, O(min(k,l) k l) per pair. When the
// links of the block exceed the LDS budget of a round (agree_plan's cap: 256 links up to 991 taxa, fewer above: 232 at
// 1100, 112 at 2259), the nodes are taken in rounds; a single node with more than cap links -- 257 links are enough up to
// 991 taxa, so a 258-taxon tree with one big polytomy has one -- gets no bitmaps and has its interval counts taken from
// the tree's leaf list instead. Exact, and slow: its pair with a reference node is the same O(min(k,l) k l) accessor calls
// in one lane, but each call is two walks over one link's stretch of the leaf list in place of two LDS reads
// (tests/agree_rounds.py restates the plan and the rounds; tests/test_gpu_tree_rounds.py runs them).
//
// Every lane adds exact integers (4x concordant, 4x discordant, 2x resolved counts; int64 arithmetic, modulo 2^64 in the
// atomics) into dst; agree_finish_kernel divides. Integer sums do not depend on the order: the result is deterministic.
#include "qs_agree_terms.hpp"
#include "qs_common.hpp"
#include "qs_internal.hpp"

#include <algorithm>

namespace qs {

constexpr int kAgreeThreads = 256;
constexpr uint32_t kAgreeLdsBytes = 65536;

struct AgreeArgs {
    const uint32_t *leaf_off, *node_off, *rng_off;
    const uint16_t *leaf_ids, *ranges;
    const uint32_t *ref_off;   // n_u + 1: boundaries of reference node u are ref_bnd[ref_off[u] .. ref_off[u+1])
    const uint16_t *ref_bnd;   // b_0 < ... < b_m: child j holds the ids [b_j, b_{j+1})
    const uint8_t *ref_par;    // 1: u has a parent link (the ids outside [b_0, b_m))
    uint32_t n_u, n, W, cap, nb;
    unsigned long long *dst;   // 4 words per tree
};

__global__ __launch_bounds__(kAgreeThreads) void tree_agree_kernel(AgreeArgs a) {
    extern __shared__ uint2 lds[];   // [W] presence bitmap, then cap links x [W]
    const uint32_t t = blockIdx.x, tid = threadIdx.x;
    const uint32_t l0 = a.leaf_off[t], L = a.leaf_off[t + 1] - l0;
    if (L < 4) return;
    const uint32_t v_lo = a.node_off[t] + blockIdx.y * a.nb, v_all = a.node_off[t + 1];
    if (blockIdx.y > 0 && v_lo >= v_all) return;
    const uint32_t v_hi = min(v_lo + a.nb, v_all);
    const uint32_t W = a.W;
    const uint16_t *ids = a.leaf_ids + l0;
    const long long N = L;
    uint2 *pres = lds, *links = lds + W;

    bm_build_presence(pres, ids, L, W, tid, kAgreeThreads);

    unsigned long long *out = a.dst + 4ull * t;
    const auto range_len = [&](uint32_t k) { return (int)((a.ranges[2 * k + 1] + L - a.ranges[2 * k]) % L); };

    // 2 x resolved in t: the block's nodes
    long long res_e = 0;
    for (uint32_t v = v_lo + tid; v < v_hi; v += kAgreeThreads) {
        const uint32_t k0 = a.rng_off[v];
        res_e += node_resolved2((int)(a.rng_off[v + 1] - k0), [&](int r) { return (long long)range_len(k0 + r); }, N);
    }
    wave_add(out + 2, res_e);
    // 2 x resolved in the reference restricted to P_t: block 0
    if (blockIdx.y == 0) {
        long long res_r = 0;
        for (uint32_t u = tid; u < a.n_u; u += kAgreeThreads) {
            const uint16_t *b = a.ref_bnd + a.ref_off[u];
            const int m = (int)(a.ref_off[u + 1] - a.ref_off[u]) - 1;
            const int all = bm_count(pres, b[m]) - bm_count(pres, b[0]);
            res_r += node_resolved2(m + a.ref_par[u], [&](int r) {
                return (long long)(r < m ? bm_count(pres, b[r + 1]) - bm_count(pres, b[r]) : (int)N - all);
            }, N);
        }
        wave_add(out + 3, res_r);
    }

    ClaimSums acc;
    for (uint32_t v0 = v_lo; v0 < v_hi;) {
        // this round: the nodes [v0, v1) whose links fit; a node with more links than the budget alone and unstored
        const uint32_t k_base = a.rng_off[v0];
        uint32_t v1 = v0;
        while (v1 < v_hi && a.rng_off[v1 + 1] - k_base <= a.cap) ++v1;
        const bool stored = v1 > v0;
        if (!stored) v1 = v0 + 1;
        const uint32_t n_links = stored ? a.rng_off[v1] - k_base : 0;
        bm_build_links(links, a.ranges, ids, L, W, k_base, n_links, tid, kAgreeThreads);

        for (uint32_t u = tid; u < a.n_u; u += kAgreeThreads) {
            const uint32_t bo = a.ref_off[u];
            const uint16_t *b = a.ref_bnd + bo;
            const int m = (int)(a.ref_off[u + 1] - bo) - 1, K = m + a.ref_par[u];
            const int pall = bm_count(pres, b[m]) - bm_count(pres, b[0]);
            const auto R = [&](int r) { return (long long)(r < m ? bm_count(pres, b[r + 1]) - bm_count(pres, b[r]) : (int)N - pall); };
            const uint32_t b0 = b[0], b1 = b[1], b2 = b[2];
            long long R3[3] = {0, 0, 0};
            if (K == 3) { R3[0] = R(0); R3[1] = R(1); R3[2] = N - R3[0] - R3[1]; }
            for (uint32_t v = v0; v < v1; ++v) {
                const uint32_t k0 = a.rng_off[v];
                const int Lc = (int)(a.rng_off[v + 1] - k0);
                const auto C = [&](int c) { return (long long)range_len(k0 + c); };
                if (stored && K == 3 && Lc == 3) {
                    // binary pair: rows 0, 1 and columns 0, 1 from the bitmaps, the rest from the sizes
                    const uint2 *B0 = links + (k0 - k_base) * W, *B1 = B0 + W;
                    const int x0 = bm_count(B0, b0), y0 = bm_count(B1, b0);
                    const int x1 = bm_count(B0, b1), y1 = bm_count(B1, b1);
                    const int x2 = bm_count(B0, b2), y2 = bm_count(B1, b2);
                    const long long C3[3] = {C(0), C(1), C(2)};
                    long long I[3][3];
                    I[0][0] = x1 - x0; I[1][0] = x2 - x1; I[2][0] = C3[0] - I[0][0] - I[1][0];
                    I[0][1] = y1 - y0; I[1][1] = y2 - y1; I[2][1] = C3[1] - I[0][1] - I[1][1];
                    for (int r = 0; r < 3; ++r) I[r][2] = R3[r] - I[r][0] - I[r][1];
                    pair_terms(3, 3, [&](int r, int c) { return I[r][c]; }, [&](int r) { return R3[r]; }, [&](int c) { return C3[c]; }, N, acc);
                } else {
                    // count of link c's leaves with ids < x: its bitmap, or (unstored node) its stretch of the leaf list
                    const auto cnt = [&](int c, uint32_t x) -> int {
                        if (stored) return bm_count(links + (k0 - k_base + c) * W, x);
                        const uint32_t s = a.ranges[2 * (k0 + c)], len = range_len(k0 + c);
                        int z = 0;
                        for (uint32_t i = 0; i < len; ++i) z += ids[(s + i) % L] < x;
                        return z;
                    };
                    const auto I = [&](int r, int c) -> long long {
                        if (r < m) return cnt(c, b[r + 1]) - cnt(c, b[r]);
                        return C(c) - (cnt(c, b[m]) - cnt(c, b[0]));
                    };
                    // the terms are symmetric in the two trees: the longer side goes inside (O(min(k,l) k l) per pair)
                    if (K <= Lc) pair_terms(K, Lc, I, R, C, N, acc);
                    else pair_terms(Lc, K, [&](int r, int c) { return I(c, r); }, C, R, N, acc);
                }
            }
        }
        v0 = v1;
    }
    wave_add(out + 0, acc.sm);
    wave_add(out + 1, acc.dc);
}

__global__ void agree_finish_kernel(unsigned long long *dst, uint32_t n_trees) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_trees) return;
    unsigned long long *p = dst + 4ull * i;   // (8-byte alignment is all the caller promises)
    p[0] /= 4; p[1] /= 4; p[2] /= 2; p[3] /= 2;
}

// LDS plan of a launch for n taxa: W words per bitmap, the link budget of one round and the inner nodes of one workgroup
void agree_plan(uint32_t n, uint32_t &W, uint32_t &cap, uint32_t &nb) {
    W = n / 32 + 1;
    const uint32_t cap_max = (kAgreeLdsBytes / 8 - W) / W;
    nb = std::max(1u, std::min(64u, cap_max / 4));
    cap = std::min(cap_max, 4 * nb);
}

hipError_t launch_tree_agree(hipStream_t s, const DeviceBatch &b, uint32_t n, uint32_t max_tree_nodes, const uint32_t *ref_off,
                             const uint16_t *ref_bnd, const uint8_t *ref_par, uint32_t n_u, unsigned long long *dst) {
    if (b.n_trees == 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(dst, 0, (size_t)b.n_trees * 4 * sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    AgreeArgs a{b.leaf_off, b.node_off, b.rng_off, b.leaf_ids, b.ranges, ref_off, ref_bnd, ref_par, n_u, n, 0, 0, 0, dst};
    agree_plan(n, a.W, a.cap, a.nb);
    const uint32_t blocks_y = std::max(1u, (max_tree_nodes + a.nb - 1) / a.nb);
    const size_t lds = (size_t)(a.W + a.cap * a.W) * sizeof(uint2);
    hipLaunchKernelGGL(tree_agree_kernel, dim3(b.n_trees, blocks_y), dim3(kAgreeThreads), lds, s, a);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(agree_finish_kernel, dim3((b.n_trees + 255) / 256), dim3(256), 0, s, dst, b.n_trees);
    return hipGetLastError();
}

} // namespace qs
