// qs_tree_branch.hip -- per evaluation tree the quartet support of every internode of the reference tree on gfx950
// (qs_tree_branch_support), weighted sums of such rows over the trees (qs_branch_resample) and the sums of their per-tree normalised
// frequencies (qs_branch_frequencies).
//
// Replaces nothing in the reference: it sums over the trees before it looks at a branch.
//
// For tree t with taxon set P_t and internode e of the reference (lower end v, upper end w) four exact words over
// the 4-sets around e that lie inside P_t: their number, and how many of them t shows as the reference's topology (q1) and as the two
// others (q2, q3, in the order qs_score uses without flags). No 4-set is enumerated. The method is qs_agree.hip's: a workgroup owns
// (tree t, a block of t's inner nodes) and holds in LDS the id bitmaps of P_t and of every link of its nodes, each word beside the
// popcount of the words before it, so that a link's leaves in an id interval are two LDS reads. A lane owns internodes and walks the
// block's nodes. The groups at the two ends of e are id intervals: the children of v split [lo_v, hi_v); the other children of w are
// intervals on its left and right; w's parent link is the rest, a left piece [0, lo_w) and a right piece [hi_w, n).
//
// A 4-set x < y (different groups of v), z < w (different groups of w, by id) that t shows as pq|rs is claimed at ONE node of t: where
// p and q lie in different links and r, s together in a third. For a group i >= 1 of v and a piece j of the upper end, with per link c
//   xs_c = |groups of v in front of i & c|, ya_c = |group i & c|, zs_c = |upper-end taxa in front of piece j, outside its group, & c|,
//   wg_c = |piece j & c|,   S. = sums over c, P.. = sums of products of two, A = sum ya zs wg, B = sum xs zs wg, C = sum xs ya wg,
//   Q = sum xs ya zs wg:
//     xy|zw  P_zw (S_x S_y - P_xy) - S_x A - S_y B + 2 Q
//     xz|yw  P_yw (S_x S_z - P_xz) - S_x A - S_z C + 2 Q
//     xw|yz  P_xw (S_y S_z - P_yz) - S_y B - S_z C + 2 Q
// zs is taken in two intervals, the part on w's side of v's interval and the part on the other side: in the multifurcating frame
// q2 = xz|yw everywhere, in the node-pair frame of a bifurcating reference q2 is the pairing that crosses in the cyclic id order, which
// is xw|yz where z and w lie on opposite sides of v (tests/tree_branch_model.py is the numpy model, branch_taxon_model.plan's cols the
// statement it matches). O(k p q) interval counts per pair of a node with k links and ends with p and q groups; a tree node of degree
// 3 runs the loop over its links unrolled.
//
// A lane adds the words of its own internodes to dst: plainly where the tree has one block of nodes, with one 64-bit atomic per
// non-zero word where it has several. Integer sums: the result does not depend on grid, batching, rooting or repetition. The rounds
// of a block whose links exceed a round's LDS budget (agree_plan's cap) and the leaf-list counts of a single node beyond it are
// qs_agree.hip's: a node with more than cap links (257 are enough up to 991 taxa) has no bitmaps, and every cnt of it walks its link's
// stretch of the leaf list: branch_piece calls cnt seven times per link, seven passes over the tree's leaves per (group, piece).
#include "qs_agree_terms.hpp"
#include "qs_common.hpp"
#include "qs_internal.hpp"

#include <algorithm>

namespace qs {

constexpr int kTreeBranchThreads = 256;

struct TreeBranchArgs {
    const uint32_t *leaf_off, *node_off, *rng_off;
    const uint16_t *leaf_ids, *ranges;
    const uint32_t *edges;    // n_e x kTreeBranchEdgeWords
    const uint16_t *bnd;      // child boundaries of the reference's inner nodes
    uint32_t n_e, n, W, cap, nb, n_nodes;
    int frame;
    unsigned long long *dst;  // [tree][node][4]
};

// the sums over K links (K = 0: Lc links) of one (group i of the lower end, piece of the upper end); cnt(c, x) = ids < x in link c
template <int K, class CF>
__device__ __forceinline__ void branch_piece(int Lc, CF cnt, uint32_t x0, uint32_t x1, uint32_t x2, uint32_t z0, uint32_t z1, uint32_t w0, uint32_t w1,
                                             bool swap, long long &f1, long long &f2, long long &f3) {
    long long Sx = 0, Sy = 0, Sz = 0, Pxy = 0, Pxz = 0, Pyz = 0, Pxw = 0, Pyw = 0, Pzw = 0, A = 0, B = 0, C = 0, Q = 0;
    const auto link = [&](int c) {
        const int m1 = cnt(c, x1);
        const long long xs = m1 - cnt(c, x0), ya = cnt(c, x2) - m1, zs = cnt(c, z1) - cnt(c, z0), wg = cnt(c, w1) - cnt(c, w0);
        const long long xy = xs * ya, zw = zs * wg;
        Sx += xs; Sy += ya; Sz += zs;
        Pxy += xy; Pxz += xs * zs; Pyz += ya * zs; Pxw += xs * wg; Pyw += ya * wg; Pzw += zw;
        A += ya * zw; B += xs * zw; C += xy * wg; Q += xy * zw;
    };
    if constexpr (K > 0) {
#pragma unroll
        for (int c = 0; c < K; ++c) link(c);
    } else {
        for (int c = 0; c < Lc; ++c) link(c);
    }
    const long long t1 = Pzw * (Sx * Sy - Pxy) - Sx * A - Sy * B + 2 * Q;
    const long long tc = Pyw * (Sx * Sz - Pxz) - Sx * A - Sz * C + 2 * Q;
    const long long tn = Pxw * (Sy * Sz - Pyz) - Sy * B - Sz * C + 2 * Q;
    f1 += t1; f2 += swap ? tn : tc; f3 += swap ? tc : tn;
}

__global__ __launch_bounds__(kTreeBranchThreads) void tree_branch_kernel(TreeBranchArgs a) {
    extern __shared__ uint2 lds[];   // [W] presence bitmap, then cap links x [W]
    const uint32_t t = blockIdx.x, tid = threadIdx.x;
    const uint32_t l0 = a.leaf_off[t], L = a.leaf_off[t + 1] - l0;
    if (L < 4) return;
    const uint32_t v_first = a.node_off[t], v_lo = v_first + blockIdx.y * a.nb, v_all = a.node_off[t + 1];
    if (blockIdx.y > 0 && v_lo >= v_all) return;
    const uint32_t v_hi = min(v_lo + a.nb, v_all);
    const bool shared_rows = v_all - v_first > a.nb;   // several workgroups add to this tree's rows
    const uint32_t W = a.W, n = a.n;
    const uint16_t *ids = a.leaf_ids + l0;
    uint2 *pres = lds, *links = lds + W;

    bm_build_presence(pres, ids, L, W, tid, kTreeBranchThreads);

    unsigned long long *out = a.dst + (size_t)t * a.n_nodes * kBranchWords;
    const auto range_len = [&](uint32_t k) { return (int)((a.ranges[2 * k + 1] + L - a.ranges[2 * k]) % L); };
    const auto in_tree = [&](uint32_t s, uint32_t e) { return e > s ? (long long)(bm_count(pres, e) - bm_count(pres, s)) : 0ll; };
    const auto add = [&](const uint32_t *ed, int k, long long v) {
        if (!v) return;
        for (int i = 0; i < 2; ++i) {
            if (ed[i] == 0xFFFFFFFFu) continue;          // (the second node: under a degree-2 root only)
            unsigned long long *p = out + (size_t)ed[i] * kBranchWords + k;
            if (shared_rows) atomicAdd(p, (unsigned long long)v);
            else *p += (unsigned long long)v;            // this lane alone owns the internode
        }
    };

    // word 0, block 0: pairs of different groups at the lower end x pairs of different groups at the upper end, inside P_t
    if (blockIdx.y == 0)
        for (uint32_t e = tid; e < a.n_e; e += kTreeBranchThreads) {
            const uint32_t *ed = a.edges + (size_t)e * kTreeBranchEdgeWords;
            const uint16_t *b = a.bnd + ed[2], *ub = a.bnd + ed[4];
            const uint32_t p = ed[3], m = ed[5], iv = ed[6], par = ed[7];
            long long s = 0, s2 = 0;
            for (uint32_t i = 0; i < p; ++i) { const long long x = in_tree(b[i], b[i + 1]); s += x; s2 += x * x; }
            const long long low = (s * s - s2) / 2;
            s = 0; s2 = 0;
            for (uint32_t j = 0; j < m; ++j)
                if (j != iv) { const long long x = in_tree(ub[j], ub[j + 1]); s += x; s2 += x * x; }
            if (par) { const long long x = in_tree(0, ub[0]) + in_tree(ub[m], n); s += x; s2 += x * x; }
            add(ed, 0, low * ((s * s - s2) / 2));
        }

    for (uint32_t v0 = v_lo; v0 < v_hi;) {
        // this round: the nodes [v0, v1) whose links fit; a node with more links than the budget alone and unstored
        const uint32_t k_base = a.rng_off[v0];
        uint32_t v1 = v0;
        while (v1 < v_hi && a.rng_off[v1 + 1] - k_base <= a.cap) ++v1;
        const bool stored = v1 > v0;
        if (!stored) v1 = v0 + 1;
        const uint32_t n_links = stored ? a.rng_off[v1] - k_base : 0;
        bm_build_links(links, a.ranges, ids, L, W, k_base, n_links, tid, kTreeBranchThreads);

        for (uint32_t e = tid; e < a.n_e; e += kTreeBranchThreads) {
            const uint32_t *ed = a.edges + (size_t)e * kTreeBranchEdgeWords;
            const uint16_t *b = a.bnd + ed[2], *ub = a.bnd + ed[4];
            const uint32_t p = ed[3], m = ed[5], iv = ed[6], par = ed[7];
            const uint32_t lo_v = b[0], hi_v = b[p], lo_w = ub[0], hi_w = ub[m], zl = par ? 0u : lo_w;
            if (in_tree(lo_v, hi_v) < 2) continue;
            long long f1 = 0, f2 = 0, f3 = 0;
            for (uint32_t v = v0; v < v1; ++v) {
                const uint32_t k0 = a.rng_off[v];
                const int Lc = (int)(a.rng_off[v + 1] - k0);
                // count of link c's leaves with ids < x: its bitmap, or (unstored node) its stretch of the leaf list
                const auto cnt = [&](int c, uint32_t x) -> int {
                    if (stored) return bm_count(links + (k0 - k_base + c) * W, x);
                    const uint32_t s = a.ranges[2 * (k0 + c)], len = range_len(k0 + c);
                    int z = 0;
                    for (uint32_t i = 0; i < len; ++i) z += ids[(s + i) % L] < x;
                    return z;
                };
                for (uint32_t i = 1; i < p; ++i) {
                    const uint32_t x0 = lo_v, x1 = b[i], x2 = b[i + 1];
                    if (!in_tree(x0, x1) || !in_tree(x1, x2)) continue;
                    // a piece [w0, w1) of the upper end with the taxa [z0, z1) in front of it; `opposite`: on the other side of v
                    const auto piece = [&](uint32_t w0, uint32_t w1, uint32_t z0, uint32_t z1, bool opposite) {
                        if (!in_tree(w0, w1) || !in_tree(z0, z1)) return;
                        const bool swap = opposite && a.frame == 0;
                        if (stored && Lc == 3) branch_piece<3>(3, cnt, x0, x1, x2, z0, z1, w0, w1, swap, f1, f2, f3);
                        else branch_piece<0>(Lc, cnt, x0, x1, x2, z0, z1, w0, w1, swap, f1, f2, f3);
                    };
                    for (uint32_t j = 0; j < m; ++j) {
                        if (j == iv) continue;
                        const uint32_t s = ub[j], en = ub[j + 1];
                        if (en <= lo_v) piece(s, en, zl, s, false);
                        else { piece(s, en, hi_v, s, false); piece(s, en, zl, lo_v, true); }
                    }
                    if (par) { piece(hi_w, n, hi_v, hi_w, false); piece(hi_w, n, lo_w, lo_v, true); }
                }
            }
            add(ed, 1, f1); add(ed, 2, f2); add(ed, 3, f3);
        }
        v0 = v1;
    }
}

hipError_t launch_tree_branch(hipStream_t s, const DeviceBatch &b, uint32_t n, uint32_t max_tree_nodes, const uint32_t *edges, const uint16_t *bnd,
                              uint32_t n_e, uint32_t n_nodes, int frame, unsigned long long *dst) {
    if (b.n_trees == 0 || n_nodes == 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(dst, 0, (size_t)b.n_trees * n_nodes * kBranchWords * sizeof(unsigned long long), s);
    if (e != hipSuccess || n_e == 0) return e;
    TreeBranchArgs a{b.leaf_off, b.node_off, b.rng_off, b.leaf_ids, b.ranges, edges, bnd, n_e, n, 0, 0, 0, n_nodes, frame, dst};
    agree_plan(n, a.W, a.cap, a.nb);
    const uint32_t blocks_y = std::max(1u, (max_tree_nodes + a.nb - 1) / a.nb);
    const size_t lds = (size_t)(a.W + a.cap * a.W) * sizeof(uint2);
    hipLaunchKernelGGL(tree_branch_kernel, dim3(b.n_trees, blocks_y), dim3(kTreeBranchThreads), lds, s, a);
    return hipGetLastError();
}

// dst[rep][cell] += sum over t of weights[rep][t] x rows[t][cell]: a workgroup takes 256 cells x kResampleReps replicates x a chunk of
// trees, the chunk's weights in LDS, so the rows are read once per kResampleReps replicates; one 64-bit atomic per non-zero sum
constexpr int kResampleReps = 16, kResampleTrees = 256;

__global__ __launch_bounds__(256) void branch_resample_kernel(const long long *__restrict__ rows, uint32_t n_trees, uint32_t cells,
                                                              const uint32_t *__restrict__ weights, uint32_t n_rep, unsigned long long *__restrict__ dst) {
    __shared__ uint32_t w[kResampleReps][kResampleTrees];
    const uint32_t cell = blockIdx.x * 256 + threadIdx.x, r0 = blockIdx.y * kResampleReps, t0 = blockIdx.z * kResampleTrees;
    const uint32_t nt = min((uint32_t)kResampleTrees, n_trees - t0), nr = min((uint32_t)kResampleReps, n_rep - r0);
    for (uint32_t i = threadIdx.x; i < kResampleReps * kResampleTrees; i += 256) {
        const uint32_t r = i / kResampleTrees, t = i % kResampleTrees;
        w[r][t] = r < nr && t < nt ? weights[(size_t)(r0 + r) * n_trees + t0 + t] : 0u;
    }
    __syncthreads();
    if (cell >= cells) return;
    long long acc[kResampleReps];
#pragma unroll
    for (int r = 0; r < kResampleReps; ++r) acc[r] = 0;
    for (uint32_t t = 0; t < nt; ++t) {
        const long long x = rows[(size_t)(t0 + t) * cells + cell];
        if (x == 0) continue;
#pragma unroll
        for (int r = 0; r < kResampleReps; ++r) acc[r] += x * (long long)w[r][t];
    }
#pragma unroll
    for (int r = 0; r < kResampleReps; ++r)
        if ((uint32_t)r < nr && acc[r]) atomicAdd(&dst[(size_t)(r0 + r) * cells + cell], (unsigned long long)acc[r]);
}

hipError_t launch_branch_resample(hipStream_t s, const long long *rows, uint32_t n_trees, uint32_t cells, const uint32_t *weights, uint32_t n_rep,
                                  unsigned long long *dst) {
    if (n_trees == 0 || cells == 0 || n_rep == 0) return hipSuccess;
    const dim3 grid((cells + 255) / 256, (n_rep + kResampleReps - 1) / kResampleReps, (n_trees + kResampleTrees - 1) / kResampleTrees);
    hipLaunchKernelGGL(branch_resample_kernel, grid, dim3(256), 0, s, rows, n_trees, cells, weights, n_rep, dst);
    return hipGetLastError();
}

// floor(q x 2^40 / S) for 0 <= q <= S < 2^53, exact, without a 128-bit division: q / S in double is within 2^-53 of the ratio (q and S
// are exact doubles, the division is rounded once), so e = the integer part of it x 2^40 is the quotient or one beside it; q x 2^40 -
// e x S lies in (-S, 2S) and is therefore right in 64-bit wrap-around arithmetic, and its sign and size say which of the three e is
__device__ __forceinline__ unsigned long long frequency_fixed(unsigned long long q, unsigned long long S) {
    unsigned long long e = (unsigned long long)((double)q / (double)S * 1099511627776.0);
    const long long r = (long long)((q << 40) - e * S);
    if (r < 0) --e;
    else if ((unsigned long long)r >= S) ++e;
    return e;
}

// dst[node] += (trees with q1 + q2 + q3 > 0, sum over them of floor(q_i x 2^40 / (q1 + q2 + q3)), i = 1..3): a lane owns a node and
// reads its row of every tree of the chunk (lanes read consecutive rows; q1 q2 q3 come as one 16-byte and one 8-byte load), the four
// sums stay in registers; one 64-bit atomic per non-zero sum. One wave per workgroup: 64 nodes x kFreqTrees trees, so that 512 taxa x
// 10 000 trees are 157 x 16 workgroups, about ten waves for each of the chip's 256 CUs, all resident at once: that, not the loop (load,
// wait, divide), keeps the loads in flight. No LDS.
constexpr int kFreqNodes = 64, kFreqTrees = 64;

__global__ __launch_bounds__(kFreqNodes) void branch_frequencies_kernel(const long long *__restrict__ rows, uint32_t n_trees, uint32_t n_nodes,
                                                                        unsigned long long *__restrict__ dst) {
    const uint32_t v = blockIdx.y * kFreqNodes + threadIdx.x, t0 = blockIdx.x * kFreqTrees;   // (the trees in x: up to 2^17 chunks)
    if (v >= n_nodes) return;
    const uint32_t nt = min((uint32_t)kFreqTrees, n_trees - t0);
    struct Row { long long present, q1, q2, q3; };   // (8-byte aligned, as the ABI asks of the rows)
    const Row *p = reinterpret_cast<const Row *>(rows) + (size_t)t0 * n_nodes + v;
    unsigned long long acc[kBranchWords] = {0, 0, 0, 0};
    for (uint32_t t = 0; t < nt; ++t, p += n_nodes) {
        const Row r = *p;
        const long long S = r.q1 + r.q2 + r.q3;
        if (S <= 0) continue;
        acc[0] += 1;
        acc[1] += frequency_fixed((unsigned long long)r.q1, (unsigned long long)S);
        acc[2] += frequency_fixed((unsigned long long)r.q2, (unsigned long long)S);
        acc[3] += frequency_fixed((unsigned long long)r.q3, (unsigned long long)S);
    }
#pragma unroll
    for (int k = 0; k < kBranchWords; ++k)
        if (acc[k]) atomicAdd(&dst[(size_t)v * kBranchWords + k], acc[k]);
}

hipError_t launch_branch_frequencies(hipStream_t s, const long long *rows, uint32_t n_trees, uint32_t n_nodes, unsigned long long *dst) {
    if (n_trees == 0 || n_nodes == 0) return hipSuccess;
    const dim3 grid((n_trees + kFreqTrees - 1) / kFreqTrees, (n_nodes + kFreqNodes - 1) / kFreqNodes);
    hipLaunchKernelGGL(branch_frequencies_kernel, grid, dim3(kFreqNodes), 0, s, rows, n_trees, n_nodes, dst);
    return hipGetLastError();
}

} // namespace qs
