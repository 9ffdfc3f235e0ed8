// qs_tree_taxa.hip -- per evaluation tree and per taxon it holds the quartet agreement with the reference tree on gfx950
// (qs_tree_taxon_agreement).
//
// Replaces nothing in the reference: it has no output per tree, and none per taxon.
//
// For tree t with taxon set P_t (L = |P_t|), the reference restricted to P_t and a taxon x of P_t four exact words over the C(L-1,3)
// 4-sets of P_t that hold x: concordant, discordant, resolved in t, resolved in the reference (tests/tree_taxon_model.py is
// the numpy model). No 4-set is enumerated. The frame is qs_agree.hip's: a workgroup owns (tree t, a block of t's inner nodes) and holds
// in LDS the id bitmaps of P_t and of every link of its nodes with running popcounts; a lane takes reference nodes. A 4-set {x,b,c,d}
// that a tree shows as xb|cd is claimed at ONE node of that tree, the junction on x's side: x, b and {c,d} lie behind three different
// links. For a node of t with links i (sizes C_i) and a reference node with groups j (sizes R_j inside P_t), I[i][j] = |link i & group j|,
// a leaf of cell (i1, j1) receives
//   Wc[i1][j1] = sum over i3 != i1, j3 != j1 of c2(I[i3][j3]) (L - C_i1 - C_i3 - R_j1 - R_j3 + I[i1][j1] + I[i1][j3] + I[i3][j1] + I[i3][j3])
//   Wd[i1][j1] = sum over i3 != i1, j3 != j1 of I[i3][j3] (R_j3 - I[i1][j3] - I[i3][j3]) (C_i3 - I[i3][j1] - I[i3][j3])
// (the definition's sums over i2 and j2 in closed form from the sizes). A binary pair is 3 x 3 with four products per cell and runs
// unrolled from six interval counts; other degrees evaluate the two sums as they stand, over the non-empty cells (i1, j1) only, with
// links of fewer than two leaves skipped as i3 and empty cells as (i3, j3): O(k l) per non-empty cell.
//
// How W reaches the taxa: for a fixed node of t and link i1, the value a leaf with id y receives from ALL reference nodes is a sum of
// functions that are constant between the child boundaries of each reference node. So a lane adds the differences of its node's values
// at that node's boundaries into a difference array over the ids in LDS (64-bit atomics, modulo 2^64), one array per link in flight
// (kTaxaFlight of them) and per word; one prefix sum over the n + 1 entries follows, and each leaf of link i1 reads the entry of its
// own id. O(pairs + nodes of t x n) per tree where adding W to every leaf of a cell would be O(pairs x n). resolved_ref is one such
// array per tree (block 0), resolved_eval a constant per link from the link sizes. A node whose links all hold at most one leaf claims
// nothing and is skipped, as is a reference node whose groups do.
//
// A lane keeps the sums of the leaf positions it owns (position p = lane + 256 o, o < kTaxaOwn) in registers across the nodes of its
// block and adds them to dst once: a plain store where the tree has one block of nodes, a 64-bit atomic per non-zero word where it has
// several. Integer sums: the result does not depend on grid, batching, rooting or repetition. The rounds of a block whose links exceed
// the round's bitmap budget and the leaf-list counts of a single node beyond it are qs_agree.hip's.
#include "qs_agree_terms.hpp"
#include "qs_common.hpp"
#include "qs_internal.hpp"

#include <algorithm>

namespace qs {

constexpr int kTaxaThreads = 256;
constexpr int kTaxaFlight = 3;               // links of a node whose difference arrays are in LDS at once: a binary node in one go
constexpr int kTaxaOwn = 6;                 // leaf positions of one lane: 256 x 6 leaves per tree at the most
constexpr uint32_t kTaxaLdsBytes = 65536;
constexpr uint32_t kTaxaMinCap = 12;         // a launch is refused where a round could not hold the links of four binary nodes
constexpr uint32_t kTaxaNodes = 64;          // inner nodes of one workgroup
constexpr uint32_t kTaxaMaxCap = 3 * kTaxaNodes;   // the links of a block of binary nodes: more bitmaps would cost the third workgroup of a CU

struct TreeTaxaArgs {
    const uint32_t *leaf_off, *node_off, *rng_off;
    const uint16_t *leaf_ids, *ranges;
    const uint32_t *ref_off;
    const uint16_t *ref_bnd;
    const uint8_t *ref_par;
    uint32_t n_u, n, W, cap, nb;
    unsigned long long *dst;   // [tree][id][4]
};

// inclusive prefix sums of n_arr arrays of D entries each, in place; a half-wave per array, a lane sums a contiguous stretch
__device__ __forceinline__ void taxa_scan(unsigned long long *arr, uint32_t n_arr, uint32_t D, uint32_t tid) {
    const uint32_t g = tid / 32, lane = tid % 32, chunk = (D + 31) / 32;
    for (uint32_t k = g; k < n_arr; k += kTaxaThreads / 32) {
        unsigned long long *p = arr + (size_t)k * D;
        const uint32_t lo = min(lane * chunk, D), hi = min(lo + chunk, D);
        unsigned long long own = 0;
        for (uint32_t i = lo; i < hi; ++i) own += p[i];
        unsigned long long incl = own;
        for (int d = 1; d < 32; d <<= 1) {
            const unsigned long long y = __shfl_up(incl, d, 32);
            if ((int)lane >= d) incl += y;
        }
        unsigned long long run = incl - own;
        for (uint32_t i = lo; i < hi; ++i) { run += p[i]; p[i] = run; }
    }
}

__global__ __launch_bounds__(kTaxaThreads) void tree_taxa_kernel(TreeTaxaArgs a) {
    extern __shared__ unsigned long long lds64[];   // kTaxaFlight x 2 difference arrays of n + 1 words, the presence bitmap [W], cap links x [W]
    const uint32_t t = blockIdx.x, tid = threadIdx.x;
    const uint32_t l0 = a.leaf_off[t], L = a.leaf_off[t + 1] - l0;
    if (L < 4) return;
    const uint32_t v_first = a.node_off[t], v_lo = v_first + blockIdx.y * a.nb, v_all = a.node_off[t + 1];
    if (blockIdx.y > 0 && v_lo >= v_all) return;
    const uint32_t v_hi = min(v_lo + a.nb, v_all);
    const bool shared_rows = v_all - v_first > a.nb;   // several workgroups add to this tree's rows
    const uint32_t W = a.W, D = a.n + 1;
    const uint16_t *ids = a.leaf_ids + l0;
    const long long N = L;
    unsigned long long *diff = lds64;
    uint2 *pres = reinterpret_cast<uint2 *>(lds64 + (size_t)kTaxaFlight * 2 * D), *links = pres + W;

    bm_build_presence(pres, ids, L, W, tid, kTaxaThreads);

    const auto range_len = [&](uint32_t k) { return (int)((a.ranges[2 * k + 1] + L - a.ranges[2 * k]) % L); };
    const auto add = [&](uint32_t arr, uint32_t idx, long long v) {
        if (v) atomicAdd(&diff[(size_t)arr * D + idx], (unsigned long long)v);
    };

    uint32_t my_id[kTaxaOwn];
    long long acc_c[kTaxaOwn], acc_d[kTaxaOwn], acc_e[kTaxaOwn], acc_r[kTaxaOwn];
#pragma unroll
    for (int o = 0; o < kTaxaOwn; ++o) {
        const uint32_t p = tid + o * kTaxaThreads;
        my_id[o] = p < L ? ids[p] : 0u;
        acc_c[o] = acc_d[o] = acc_e[o] = acc_r[o] = 0;
    }

    // resolved in the reference restricted to P_t: block 0, one difference array
    if (blockIdx.y == 0) {
        for (uint32_t i = tid; i < D; i += kTaxaThreads) diff[i] = 0;
        __syncthreads();
        for (uint32_t u = tid; u < a.n_u; u += kTaxaThreads) {
            const uint16_t *b = a.ref_bnd + a.ref_off[u];
            const int m = (int)(a.ref_off[u + 1] - a.ref_off[u]) - 1, par = a.ref_par[u];
            const int all = bm_count(pres, b[m]) - bm_count(pres, b[0]);
            const auto S = [&](int r) { return (long long)(r < m ? bm_count(pres, b[r + 1]) - bm_count(pres, b[r]) : (int)N - all); };
            long long s2 = 0, s3 = 0;
            for (int r = 0; r < m + par; ++r) { const long long x = S(r); s2 += c2(x); s3 += x * c2(x); }
            if (s2 == 0) continue;
            const auto res = [&](int r) { const long long x = S(r); return (s2 - c2(x)) * (N - x) - (s3 - x * c2(x)); };
            const long long rest = par ? res(m) : 0;
            long long prev = rest;
            add(0, 0, rest);
            for (int r = 0; r < m; ++r) { const long long w = res(r); add(0, b[r], w - prev); prev = w; }
            add(0, b[m], rest - prev);
        }
        __syncthreads();
        taxa_scan(diff, 1, D, tid);
        __syncthreads();
#pragma unroll
        for (int o = 0; o < kTaxaOwn; ++o)
            if (tid + o * kTaxaThreads < L) acc_r[o] = (long long)diff[my_id[o]];
        __syncthreads();
    }

    for (uint32_t v0 = v_lo; v0 < v_hi;) {
        // this round: the nodes [v0, v1) whose links fit; a node with more links than the budget alone and unstored
        const uint32_t k_base = a.rng_off[v0];
        uint32_t v1 = v0;
        while (v1 < v_hi && a.rng_off[v1 + 1] - k_base <= a.cap) ++v1;
        const bool stored = v1 > v0;
        if (!stored) v1 = v0 + 1;
        const uint32_t n_links = stored ? a.rng_off[v1] - k_base : 0;
        bm_build_links(links, a.ranges, ids, L, W, k_base, n_links, tid, kTaxaThreads);

        for (uint32_t v = v0; v < v1; ++v) {
            const uint32_t k0 = a.rng_off[v];
            const int Lc = (int)(a.rng_off[v + 1] - k0);
            const auto C = [&](int c) { return (long long)range_len(k0 + c); };
            long long s2 = 0, s3 = 0;
            for (int c = 0; c < Lc; ++c) { const long long x = C(c); s2 += c2(x); s3 += x * c2(x); }
            if (Lc < 3 || s2 == 0) continue;   // no link with two leaves: the node claims nothing (the same for every lane)
            // count of link c's leaves with ids < x: its bitmap, or (unstored node) its stretch of the leaf list
            const auto cnt = [&](int c, uint32_t x) -> int {
                if (stored) return bm_count(links + (k0 - k_base + c) * W, x);
                const uint32_t s = a.ranges[2 * (k0 + c)], len = range_len(k0 + c);
                int z = 0;
                for (uint32_t i = 0; i < len; ++i) z += ids[(s + i) % L] < x;
                return z;
            };
            for (int c0 = 0; c0 < Lc; c0 += kTaxaFlight) {
                const int Fc = min(kTaxaFlight, Lc - c0);
                for (uint32_t i = tid; i < (uint32_t)Fc * 2 * D; i += kTaxaThreads) diff[i] = 0;
                __syncthreads();

                for (uint32_t u = tid; u < a.n_u; u += kTaxaThreads) {
                    const uint16_t *b = a.ref_bnd + a.ref_off[u];
                    const int m = (int)(a.ref_off[u + 1] - a.ref_off[u]) - 1, par = a.ref_par[u], K = m + par;
                    const int pall = bm_count(pres, b[m]) - bm_count(pres, b[0]);
                    const auto R = [&](int r) { return (long long)(r < m ? bm_count(pres, b[r + 1]) - bm_count(pres, b[r]) : (int)N - pall); };
                    if (stored && K == 3 && Lc == 3) {
                        // binary pair: groups 0, 1 and links 0, 1 from the bitmaps, the rest from the sizes; group 2 is the complement of
                        // [b0, b2), the parent link or the third child of a root
                        const uint32_t b0 = b[0], b1 = b[1], b2 = b[2];
                        const uint2 *B0 = links + (k0 - k_base) * W, *B1 = B0 + W;
                        const int x0 = bm_count(B0, b0), y0 = bm_count(B1, b0);
                        const int x1 = bm_count(B0, b1), y1 = bm_count(B1, b1);
                        const int x2 = bm_count(B0, b2), y2 = bm_count(B1, b2);
                        const long long C3[3] = {C(0), C(1), C(2)};
                        long long R3[3], I[3][3], Q[3][3];   // I[group][link], Q = c2(I)
                        R3[0] = R(0); R3[1] = R(1); R3[2] = N - R3[0] - R3[1];
                        I[0][0] = x1 - x0; I[1][0] = x2 - x1; I[2][0] = C3[0] - I[0][0] - I[1][0];
                        I[0][1] = y1 - y0; I[1][1] = y2 - y1; I[2][1] = C3[1] - I[0][1] - I[1][1];
#pragma unroll
                        for (int r = 0; r < 3; ++r) I[r][2] = R3[r] - I[r][0] - I[r][1];
#pragma unroll
                        for (int r = 0; r < 3; ++r)
#pragma unroll
                            for (int c = 0; c < 3; ++c) Q[r][c] = c2(I[r][c]);
#pragma unroll
                        for (int c = 0; c < 3; ++c) {
                            const int ca = (c + 1) % 3, cb = (c + 2) % 3;
                            long long wc[3], wd[3];
#pragma unroll
                            for (int r = 0; r < 3; ++r) {
                                const int ra = (r + 1) % 3, rb = (r + 2) % 3;
                                wc[r] = I[ra][ca] * Q[rb][cb] + I[rb][ca] * Q[ra][cb] + I[ra][cb] * Q[rb][ca] + I[rb][cb] * Q[ra][ca];
                                wd[r] = I[ra][ca] * I[ra][cb] * I[rb][cb] + I[ra][ca] * I[rb][ca] * I[rb][cb] +
                                        I[rb][ca] * I[ra][cb] * (I[rb][cb] + I[ra][ca]);
                            }
                            // along the ids: group 2 | group 0 | group 1 | group 2; an empty cell has no reader and repeats its neighbour
                            const long long c_2 = I[2][c] ? wc[2] : 0, c_0 = I[0][c] ? wc[0] : c_2, c_1 = I[1][c] ? wc[1] : c_0;
                            const long long d_2 = I[2][c] ? wd[2] : 0, d_0 = I[0][c] ? wd[0] : d_2, d_1 = I[1][c] ? wd[1] : d_0;
                            add(2 * c, 0, c_2); add(2 * c, b0, c_0 - c_2); add(2 * c, b1, c_1 - c_0); add(2 * c, b2, c_2 - c_1);
                            add(2 * c + 1, 0, d_2); add(2 * c + 1, b0, d_0 - d_2); add(2 * c + 1, b1, d_1 - d_0); add(2 * c + 1, b2, d_2 - d_1);
                        }
                        continue;
                    }
                    bool two = false;
                    for (int r = 0; r < K && !two; ++r) two = R(r) >= 2;
                    if (!two) continue;   // no group with two leaves inside P_t: the reference node claims nothing
                    const auto I = [&](int c, int r) -> long long {   // |link c & group r|
                        if (r < m) return cnt(c, b[r + 1]) - cnt(c, b[r]);
                        return C(c) - (cnt(c, b[m]) - cnt(c, b[0]));
                    };
                    // the two sums of the cell (link i1, group j1), which is not empty
                    const auto cell = [&](int i1, int j1, long long x11, long long &wc, long long &wd) {
                        const long long base = N - C(i1) - R(j1) + x11;
                        wc = 0; wd = 0;
                        for (int i3 = 0; i3 < Lc; ++i3) {
                            const long long C3 = C(i3);
                            if (i3 == i1 || C3 < 2) continue;
                            const long long y = I(i3, j1);
                            if (C3 - y < 2) continue;   // fewer than two leaves of the link outside group j1
                            for (int j3 = 0; j3 < K; ++j3) {
                                if (j3 == j1) continue;
                                const long long x = I(i3, j3);
                                if (!x) continue;
                                const long long z = I(i1, j3), Rj = R(j3);
                                wc += c2(x) * (base - C3 - Rj + z + y + x);
                                wd += x * (Rj - z - x) * (C3 - y - x);
                            }
                        }
                    };
                    for (int f = 0; f < Fc; ++f) {
                        const int i1 = c0 + f;
                        // along the ids: the rest | group 0 | ... | group m - 1 | the rest; an empty cell has no reader and repeats its neighbour
                        long long rest_c = 0, rest_d = 0;
                        if (par) {
                            const long long x11 = I(i1, m);
                            if (x11) cell(i1, m, x11, rest_c, rest_d);
                        }
                        long long prev_c = rest_c, prev_d = rest_d;
                        add(2 * f, 0, rest_c); add(2 * f + 1, 0, rest_d);
                        for (int j1 = 0; j1 < m; ++j1) {
                            const long long x11 = I(i1, j1);
                            if (!x11) continue;
                            long long wc, wd;
                            cell(i1, j1, x11, wc, wd);
                            add(2 * f, b[j1], wc - prev_c); add(2 * f + 1, b[j1], wd - prev_d);
                            prev_c = wc; prev_d = wd;
                        }
                        add(2 * f, b[m], rest_c - prev_c); add(2 * f + 1, b[m], rest_d - prev_d);
                    }
                }
                __syncthreads();
                taxa_scan(diff, 2 * Fc, D, tid);
                __syncthreads();

                for (int f = 0; f < Fc; ++f) {
                    const uint32_t s = a.ranges[2 * (k0 + c0 + f)];
                    const long long x = C(c0 + f);
                    const long long res_e = (s2 - c2(x)) * (N - x) - (s3 - x * c2(x));
                    const unsigned long long *dc = diff + (size_t)(2 * f) * D, *dd = dc + D;
#pragma unroll
                    for (int o = 0; o < kTaxaOwn; ++o) {
                        const uint32_t p = tid + o * kTaxaThreads;
                        if (p < L && (p + L - s) % L < (uint32_t)x) {
                            acc_c[o] += (long long)dc[my_id[o]]; acc_d[o] += (long long)dd[my_id[o]]; acc_e[o] += res_e;
                        }
                    }
                }
                __syncthreads();
            }
        }
        v0 = v1;
    }

#pragma unroll
    for (int o = 0; o < kTaxaOwn; ++o) {
        if (tid + o * kTaxaThreads >= L) continue;
        unsigned long long *out = a.dst + ((size_t)t * a.n + my_id[o]) * kTreeTaxaWords;
        const long long w[kTreeTaxaWords] = {acc_c[o], acc_d[o], acc_e[o], acc_r[o]};
#pragma unroll
        for (int k = 0; k < kTreeTaxaWords; ++k) {
            if (!shared_rows) out[k] = (unsigned long long)w[k];   // this lane alone owns the taxon's row
            else if (w[k]) atomicAdd(out + k, (unsigned long long)w[k]);
        }
    }
}

// LDS plan of a launch for n taxa: the difference arrays first, the bitmaps in what is left. False: n is beyond the limit (a round
// could not hold kTaxaMinCap link bitmaps, or a lane would own more than kTaxaOwn leaf positions).
bool tree_taxa_plan(uint32_t n, TreeTaxaPlan &p) {
    p.W = n / 32 + 1;
    p.flight = kTaxaFlight;
    p.nb = kTaxaNodes;
    p.diff_bytes = (uint32_t)std::min<uint64_t>((uint64_t)kTaxaFlight * 2 * ((uint64_t)n + 1) * 8, 0xFFFFFFFFu);
    p.cap = 0; p.lds_bytes = 0;
    if (n > (uint32_t)kTaxaThreads * kTaxaOwn || (uint64_t)p.diff_bytes + (uint64_t)(1 + kTaxaMinCap) * p.W * 8 > kTaxaLdsBytes) return false;
    p.cap = std::min(kTaxaMaxCap, (kTaxaLdsBytes - p.diff_bytes) / 8 / p.W - 1);
    p.lds_bytes = p.diff_bytes + (1 + p.cap) * p.W * 8;
    return true;
}

uint32_t tree_taxa_max_taxa() {
    static const uint32_t limit = [] {
        TreeTaxaPlan p;
        uint32_t n = 4;
        while (tree_taxa_plan(n + 1, p)) ++n;   // (the plan is monotone in n)
        return n;
    }();
    return limit;
}

hipError_t launch_tree_taxa(hipStream_t s, const DeviceBatch &b, uint32_t n, uint32_t max_tree_nodes, const uint32_t *ref_off,
                            const uint16_t *ref_bnd, const uint8_t *ref_par, uint32_t n_u, unsigned long long *dst) {
    if (b.n_trees == 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(dst, 0, (size_t)b.n_trees * n * kTreeTaxaWords * sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    TreeTaxaPlan p;
    if (!tree_taxa_plan(n, p)) return hipErrorInvalidValue;   // (the ABI refuses such a context before it comes here)
    TreeTaxaArgs a{b.leaf_off, b.node_off, b.rng_off, b.leaf_ids, b.ranges, ref_off, ref_bnd, ref_par, n_u, n, p.W, p.cap, p.nb, dst};
    const uint32_t blocks_y = std::max(1u, (max_tree_nodes + p.nb - 1) / p.nb);
    hipLaunchKernelGGL(tree_taxa_kernel, dim3(b.n_trees, blocks_y), dim3(kTaxaThreads), p.lds_bytes, s, a);
    return hipGetLastError();
}

} // namespace qs
