// qs_agree_pairs.hip -- quartet agreement of the evaluation trees with EACH OTHER on gfx950 (qs_tree_pair_agreement).
//
// For row tree s (taxa P_s) and column tree t (taxa P_t), S = P_s & P_t, N = |S|, both trees restricted to S, five exact words over
// the C(N,4) quartets of S: concordant, discordant, resolved in s, resolved in t, N. The method is qs_agree.hip's (a
// resolved quartet is claimed by exactly two inner nodes of a tree, so the counts are sums over node pairs of closed forms in
// I[r][c] = |A_r & B_c & S|), moved into another coordinate system: the reference's links are intervals of ids, any
// tree's links are circular arcs [st, en) of its OWN leaf-tour positions -- what qs_tree_batch::ranges stores.
//
// pair_pos_kernel writes pos_s[id] = the tour position of taxon id in s (0xFFFF: s lacks it) for the row trees of a call, and the
// inner nodes of s ordered by (binary first, then by degree): lanes take their nodes u in that order, so that the 64 lanes of a wave
// hold nodes of one degree wherever they can -- a wave runs the general loops of pair_terms as soon as ONE lane's pair is not binary,
// and for as long as its highest degree asks.
//
// A workgroup owns (pair (s,t), a block of t's inner nodes). Its LDS bitmaps are indexed by s-POSITION: the presence bitmap holds
// the leaves of t that have a position in s (its total is N), and every link of the block's nodes gets a bitmap of its leaves
// built the same way, each word paired with the popcount of the words before it. The number of a bitmap's leaves in an arc of s
// is then cnt(en) - cnt(st), or total - cnt(st) + cnt(en) for an arc that wraps (an end stored as 0 is L_s and wraps the same
// way). Rows R(r) are arc counts on the presence bitmap, columns C(c) the totals of the link bitmaps (NOT the range lengths:
// leaves outside S do not count), I[r][c] arc counts on the link bitmaps. Links without a shared leaf give zeros, which
// pair_terms and node_resolved2 take unchanged. Each lane takes inner nodes u of s and walks the block's nodes v; a binary pair
// runs unrolled (rows 0, 1 and columns 0, 1 from the bitmaps: eight counts; the rest from the sizes). Rounds and the unstored
// path are qs_agree.hip's: a node of t with more links than a round's budget (agree_plan's cap; 257 links are enough up to 991 taxa)
// gets no bitmaps, and each accessor call of its pairs is one walk over its link's stretch of t's leaf list through pos_s (list_count:
// leaves without a position in s do not count, the others by the arc test), the same O(min(k,l) k l) calls per pair, in one lane.
//
// Cost per node pair O(min(k,l) k l) in the two degrees: two stars of a thousand leaves meeting are 1e9 operations in ONE lane.
// Every lane adds exact integers (4x, 4x, 2x, 2x; modulo 2^64 in the atomics), one atomic per wave; pair_finish_kernel divides.
#include "qs_agree_terms.hpp"
#include "qs_common.hpp"
#include "qs_internal.hpp"

#include <algorithm>

namespace qs {

constexpr int kPairThreads = 256;
constexpr uint32_t kNoPos = 0xFFFFu;

struct PairTreeArrays {
    const uint32_t *leaf_off, *node_off, *rng_off;
    const uint16_t *leaf_ids, *ranges;
};

struct PairArgs {
    PairTreeArrays s, t;    // the row batch and the column batch
    const uint16_t *pos;    // [n_rows][n]: pos[(row - r0) * n + id]
    const uint16_t *ord;    // [n_rows][ord_stride]: the inner nodes of a row tree (numbered within the tree) by (binary first, degree)
    uint32_t ord_stride;
    uint32_t r0, c0, n_rows, n_cols;
    uint32_t upper;         // 1: pairs with column index <= row index are skipped
    uint32_t n, W, cap, nb;
    unsigned long long *dst;   // kPairWords words per pair
};

__global__ __launch_bounds__(kPairThreads) void pair_pos_kernel(PairTreeArrays s, uint32_t r0, uint32_t n, uint32_t ord_stride, uint16_t *pos,
                                                                uint16_t *ord) {
    extern __shared__ uint32_t key[];   // per inner node of the tree (at most ord_stride): (not binary) << 16 | links
    const uint32_t row = blockIdx.x, l0 = s.leaf_off[r0 + row], L = s.leaf_off[r0 + row + 1] - l0;
    uint16_t *p = pos + (size_t)row * n;   // (filled with 0xFFFF beforehand)
    for (uint32_t i = threadIdx.x; i < L; i += kPairThreads) {
        const uint32_t id = s.leaf_ids[l0 + i];
        if (id < n) p[id] = (uint16_t)i;
    }
    const uint32_t u_lo = s.node_off[r0 + row], n_u = min(s.node_off[r0 + row + 1] - u_lo, ord_stride);
    for (uint32_t i = threadIdx.x; i < n_u; i += kPairThreads) {
        const uint32_t d = s.rng_off[u_lo + i + 1] - s.rng_off[u_lo + i];
        key[i] = (d != 3 ? 0x10000u : 0u) | min(d, 0xFFFFu);
    }
    __syncthreads();
    uint16_t *o = ord + (size_t)row * ord_stride;
    for (uint32_t i = threadIdx.x; i < n_u; i += kPairThreads) {   // the rank of node i: a permutation of [0, n_u)
        const uint32_t k = key[i];
        uint32_t rank = 0;
        for (uint32_t j = 0; j < n_u; ++j) rank += (key[j] < k || (key[j] == k && j < i)) ? 1u : 0u;
        o[rank] = (uint16_t)i;
    }
}

// the entries of a bitmap (total of them: tot) at the positions of the circular arc [st, en)
__device__ __forceinline__ int arc_count(const uint2 *bm, int tot, uint32_t st, uint32_t en) {
    const int d = bm_count(bm, en) - bm_count(bm, st);
    return st <= en ? d : tot + d;
}

__global__ __launch_bounds__(kPairThreads) void tree_pair_kernel(PairArgs a) {
    extern __shared__ uint2 lds[];   // [W] presence bitmap, then cap links x [W]
    const uint32_t tid = threadIdx.x;
    const uint32_t row = blockIdx.x / a.n_cols, col = blockIdx.x % a.n_cols;
    const uint32_t si = a.r0 + row, ti = a.c0 + col;
    if (a.upper && ti <= si) return;
    const uint32_t ls0 = a.s.leaf_off[si], Ls = a.s.leaf_off[si + 1] - ls0;
    const uint32_t lt0 = a.t.leaf_off[ti], Lt = a.t.leaf_off[ti + 1] - lt0;
    const uint32_t v_lo = a.t.node_off[ti] + blockIdx.y * a.nb, v_all = a.t.node_off[ti + 1];
    if (blockIdx.y > 0 && v_lo >= v_all) return;
    const uint32_t v_hi = min(v_lo + a.nb, v_all);
    const uint32_t u_lo = a.s.node_off[si], u_hi = a.s.node_off[si + 1];
    const uint32_t W = a.W;
    const uint16_t *ids = a.t.leaf_ids + lt0;
    const uint16_t *pos = a.pos + (size_t)row * a.n;
    const uint16_t *ord = a.ord + (size_t)row * a.ord_stride;
    const uint16_t *rs = a.s.ranges, *rt = a.t.ranges;
    uint2 *pres = lds, *links = lds + W;

    for (uint32_t w = tid; w < W; w += kPairThreads) pres[w] = make_uint2(0, 0);
    __syncthreads();
    for (uint32_t p = tid; p < Lt; p += kPairThreads) {
        const uint32_t q = pos[ids[p]];
        if (q != kNoPos) atomicOr(&pres[q >> 5].x, 1u << (q & 31));
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t s = 0;
        for (uint32_t w = 0; w < W; ++w) { pres[w].y = s; s += __popc(pres[w].x); }
    }
    __syncthreads();
    const int Ni = bm_count(pres, Ls);   // every position is below L_s <= n < 32 W
    const long long N = Ni;
    unsigned long long *out = a.dst + (size_t)kPairWords * blockIdx.x;
    if (blockIdx.y == 0 && tid == 0) out[4] = (unsigned long long)N;
    if (N < 4) return;

    const auto range_len = [&](uint32_t k) { return (uint32_t)((rt[2 * k + 1] + Lt - rt[2 * k]) % Lt); };
    // leaves of link k of t that s holds (in the arc [st, en) of s: in_arc), from t's leaf list: the unstored path
    const auto list_count = [&](uint32_t k, bool in_arc, uint32_t st, uint32_t en) -> int {
        const uint32_t b = rt[2 * k], len = range_len(k);
        int z = 0;
        for (uint32_t i = 0; i < len; ++i) {
            const uint32_t q = pos[ids[(b + i) % Lt]];
            z += q != kNoPos && (!in_arc || (st <= en ? (q >= st && q < en) : (q >= st || q < en)));
        }
        return z;
    };

    // 2 x resolved in s restricted to S: block 0
    if (blockIdx.y == 0) {
        long long res_r = 0;
        for (uint32_t u = u_lo + tid; u < u_hi; u += kPairThreads) {
            const uint32_t k0 = a.s.rng_off[u];
            res_r += node_resolved2((int)(a.s.rng_off[u + 1] - k0), [&](int r) {
                return (long long)arc_count(pres, Ni, rs[2 * (k0 + r)], rs[2 * (k0 + r) + 1]);
            }, N);
        }
        wave_add(out + 2, res_r);
    }

    ClaimSums acc;
    long long res_c = 0;
    for (uint32_t v0 = v_lo; v0 < v_hi;) {
        // this round: the nodes [v0, v1) whose links fit; a node with more links than the budget alone and unstored
        const uint32_t k_base = a.t.rng_off[v0];
        uint32_t v1 = v0;
        while (v1 < v_hi && a.t.rng_off[v1 + 1] - k_base <= a.cap) ++v1;
        const bool stored = v1 > v0;
        if (!stored) v1 = v0 + 1;
        const uint32_t n_links = stored ? a.t.rng_off[v1] - k_base : 0;
        __syncthreads();   // the previous round's readers are done
        for (uint32_t i = tid; i < n_links * W; i += kPairThreads) links[i] = make_uint2(0, 0);
        __syncthreads();
        for (uint32_t li = tid / kWave; li < n_links; li += kPairThreads / kWave) {
            const uint32_t b = rt[2 * (k_base + li)], len = range_len(k_base + li);
            uint2 *bm = links + li * W;
            for (uint32_t i = tid % kWave; i < len; i += kWave) {
                const uint32_t q = pos[ids[(b + i) % Lt]];
                if (q != kNoPos) atomicOr(&bm[q >> 5].x, 1u << (q & 31));
            }
        }
        __syncthreads();
        for (uint32_t li = tid; li < n_links; li += kPairThreads) {
            uint2 *bm = links + li * W;
            uint32_t s = 0;
            for (uint32_t w = 0; w < W; ++w) { bm[w].y = s; s += __popc(bm[w].x); }
        }
        __syncthreads();

        // 2 x resolved in t restricted to S: the round's nodes, from the restricted sizes
        for (uint32_t v = v0 + tid; v < v1; v += kPairThreads) {
            const uint32_t k0 = a.t.rng_off[v];
            res_c += node_resolved2((int)(a.t.rng_off[v + 1] - k0), [&](int c) {
                return (long long)(stored ? bm_count(links + (k0 - k_base + c) * W, Ls) : list_count(k0 + c, false, 0, 0));
            }, N);
        }

        for (uint32_t i = tid; i < u_hi - u_lo; i += kPairThreads) {
            const uint32_t u = u_lo + ord[i];
            const uint32_t ks = a.s.rng_off[u];
            const int K = (int)(a.s.rng_off[u + 1] - ks);
            const uint16_t *arcs = rs + 2 * ks;   // link r of u: [arcs[2r], arcs[2r+1])
            const auto R = [&](int r) { return (long long)arc_count(pres, Ni, arcs[2 * r], arcs[2 * r + 1]); };
            uint32_t st0 = 0, en0 = 0, st1 = 0, en1 = 0;
            long long R3[3] = {0, 0, 0};
            if (K == 3) {
                st0 = arcs[0]; en0 = arcs[1]; st1 = arcs[2]; en1 = arcs[3];
                R3[0] = R(0); R3[1] = R(1); R3[2] = N - R3[0] - R3[1];
            }
            for (uint32_t v = v0; v < v1; ++v) {
                const uint32_t k0 = a.t.rng_off[v];
                const int Lc = (int)(a.t.rng_off[v + 1] - k0);
                if (stored && K == 3 && Lc == 3) {
                    // binary pair: rows 0, 1 and columns 0, 1 from the bitmaps, the rest from the sizes
                    const uint2 *B0 = links + (k0 - k_base) * W, *B1 = B0 + W;
                    const int c0 = bm_count(B0, Ls), c1 = bm_count(B1, Ls);
                    const long long C3[3] = {c0, c1, N - c0 - c1};
                    long long I[3][3];
                    I[0][0] = arc_count(B0, c0, st0, en0); I[1][0] = arc_count(B0, c0, st1, en1); I[2][0] = C3[0] - I[0][0] - I[1][0];
                    I[0][1] = arc_count(B1, c1, st0, en0); I[1][1] = arc_count(B1, c1, st1, en1); I[2][1] = C3[1] - I[0][1] - I[1][1];
                    for (int r = 0; r < 3; ++r) I[r][2] = R3[r] - I[r][0] - I[r][1];
                    pair_terms(3, 3, [&](int r, int c) { return I[r][c]; }, [&](int r) { return R3[r]; }, [&](int c) { return C3[c]; }, N, acc);
                } else {
                    const auto C = [&](int c) -> long long {
                        return stored ? bm_count(links + (k0 - k_base + c) * W, Ls) : list_count(k0 + c, false, 0, 0);
                    };
                    const auto I = [&](int r, int c) -> long long {
                        const uint32_t st = arcs[2 * r], en = arcs[2 * r + 1];
                        if (!stored) return list_count(k0 + c, true, st, en);
                        const uint2 *bm = links + (k0 - k_base + c) * W;
                        return arc_count(bm, bm_count(bm, Ls), st, en);
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
    wave_add(out + 3, res_c);
}

__global__ void pair_finish_kernel(unsigned long long *dst, uint32_t n_pairs) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pairs) return;
    unsigned long long *p = dst + (size_t)kPairWords * i;   // (8-byte alignment is all the caller promises)
    p[0] /= 4; p[1] /= 4; p[2] /= 2; p[3] /= 2;
}

hipError_t launch_tree_pairs(hipStream_t s, const DeviceBatch &rows, uint32_t r0, uint32_t r1, const DeviceBatch &cols, uint32_t c0,
                             uint32_t c1, bool upper, uint32_t n, uint16_t *work, unsigned long long *dst) {
    const uint32_t n_rows = r1 - r0, n_cols = c1 - c0;
    if (n_rows == 0 || n_cols == 0) return hipSuccess;
    const uint32_t n_pairs = n_rows * n_cols;   // (the caller keeps it within 2^28)
    hipError_t e = hipMemsetAsync(dst, 0, (size_t)n_pairs * kPairWords * sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    uint16_t *pos = work, *ord = work + (size_t)n_rows * n;
    const uint32_t ord_stride = rows.max_tree_nodes;
    e = hipMemsetAsync(pos, 0xFF, (size_t)n_rows * n * sizeof(uint16_t), s);
    if (e != hipSuccess) return e;
    PairArgs a{};
    a.s = PairTreeArrays{rows.leaf_off, rows.node_off, rows.rng_off, rows.leaf_ids, rows.ranges};
    a.t = PairTreeArrays{cols.leaf_off, cols.node_off, cols.rng_off, cols.leaf_ids, cols.ranges};
    a.pos = pos; a.ord = ord; a.ord_stride = ord_stride; a.r0 = r0; a.c0 = c0; a.n_rows = n_rows; a.n_cols = n_cols; a.upper = upper ? 1u : 0u; a.n = n; a.dst = dst;
    agree_plan(n, a.W, a.cap, a.nb);
    hipLaunchKernelGGL(pair_pos_kernel, dim3(n_rows), dim3(kPairThreads), (size_t)ord_stride * sizeof(uint32_t), s, a.s, r0, n, ord_stride, pos, ord);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    const uint32_t blocks_y = std::max(1u, (cols.max_tree_nodes + a.nb - 1) / a.nb);
    const size_t lds = (size_t)(a.W + a.cap * a.W) * sizeof(uint2);
    hipLaunchKernelGGL(tree_pair_kernel, dim3(n_pairs, blocks_y), dim3(kPairThreads), lds, s, a);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(pair_finish_kernel, dim3((n_pairs + 255) / 256), dim3(256), 0, s, dst, n_pairs);
    return hipGetLastError();
}

} // namespace qs
