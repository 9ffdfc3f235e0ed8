// qs_agree_terms.hpp -- the node-pair closed forms of the quartet agreement of two trees, shared by the kernels that
// compare the evaluation trees with the reference (qs_agree.hip) and with each other (qs_agree_pairs.hip). Device code only.
#pragma once
#include "qs_common.hpp"

namespace qs {

__device__ __forceinline__ long long c2(long long x) { return x * (x - 1) / 2; }

// ids < x among the entries of one LDS bitmap (W words of {bits, popcount of the words before})
__device__ __forceinline__ int bm_count(const uint2 *bm, uint32_t x) {
    const uint2 e = bm[x >> 5];
    return (int)e.y + __popc(e.x & ((1u << (x & 31)) - 1u));
}

// The LDS bitmaps of the kernels that walk (reference node, node of one evaluation tree) pairs (qs_agree.hip, qs_tree_branch.hip), built
// by the whole workgroup of `threads` lanes; both end with a barrier.
// pres <- the ids of the tree's L leaves
__device__ __forceinline__ void bm_build_presence(uint2 *pres, const uint16_t *ids, uint32_t L, uint32_t W, uint32_t tid, uint32_t threads) {
    for (uint32_t w = tid; w < W; w += threads) pres[w] = make_uint2(0, 0);
    __syncthreads();
    for (uint32_t p = tid; p < L; p += threads) atomicOr(&pres[ids[p] >> 5].x, 1u << (ids[p] & 31));
    __syncthreads();
    if (tid == 0) {
        uint32_t s = 0;
        for (uint32_t w = 0; w < W; ++w) { pres[w].y = s; s += __popc(pres[w].x); }
    }
    __syncthreads();
}
// links[li] <- the ids behind link k_base + li of the tree, li < n_links: the circular stretch ranges[2k] .. ranges[2k + 1] of its leaf
// list; a wave per link. Starts with a barrier: the previous round's readers are done.
__device__ __forceinline__ void bm_build_links(uint2 *links, const uint16_t *ranges, const uint16_t *ids, uint32_t L, uint32_t W, uint32_t k_base,
                                               uint32_t n_links, uint32_t tid, uint32_t threads) {
    __syncthreads();
    for (uint32_t i = tid; i < n_links * W; i += threads) links[i] = make_uint2(0, 0);
    __syncthreads();
    for (uint32_t li = tid / kWave; li < n_links; li += threads / kWave) {
        const uint32_t s = ranges[2 * (k_base + li)], len = (ranges[2 * (k_base + li) + 1] + L - s) % L;
        uint2 *bm = links + li * W;
        for (uint32_t i = tid % kWave; i < len; i += kWave) {
            const uint32_t id = ids[(s + i) % L];
            atomicOr(&bm[id >> 5].x, 1u << (id & 31));
        }
    }
    __syncthreads();
    for (uint32_t li = tid; li < n_links; li += threads) {
        uint2 *bm = links + li * W;
        uint32_t s = 0;
        for (uint32_t w = 0; w < W; ++w) { bm[w].y = s; s += __popc(bm[w].x); }
    }
    __syncthreads();
}

struct ClaimSums {
    long long sm = 0;   // sum over node pairs of same + mixed = 4 x concordant
    long long dc = 0;   // 4 x discordant
};

// One node pair: I(r,c), row sizes R(r), column sizes C(c) as accessors (r < K, c < Lc). Row and column aggregates are
// recomputed where they are needed, so nothing of size K or Lc is stored: O(K Lc (1 + K)) accessor calls, so K should be
// the shorter side.
template <class IF, class RF, class CF>
__device__ __forceinline__ void pair_terms(int K, int Lc, IF I, RF R, CF C, long long N, ClaimSums &acc) {
    long long T2 = 0;
    for (int r = 0; r < K; ++r)
        for (int c = 0; c < Lc; ++c) T2 += c2(I(r, c));
    long long sm = 0, dc = 0;
    for (int r = 0; r < K; ++r) {
        const long long Rr = R(r);
        long long rowC2 = 0, rowX = 0, rowIC = 0, rowSq = 0;
        for (int c = 0; c < Lc; ++c) {
            const long long x = I(r, c), Cc = C(c);
            rowC2 += c2(x); rowX += c2(Cc - x); rowIC += x * Cc; rowSq += x * x;
        }
        for (int c = 0; c < Lc; ++c) {
            const long long x = I(r, c), Cc = C(c);
            long long colC2 = 0, colX = 0, colIR = 0, colSq = 0;
            for (int i = 0; i < K; ++i) {
                const long long y = I(i, c), Ri = R(i);
                colC2 += c2(y); colX += c2(Ri - y); colIR += y * Ri; colSq += y * y;
            }
            const long long ci = c2(x), X = N - Rr - Cc + x, A = Rr - x, B = Cc - x;
            const long long D = c2(X) - (colX - c2(A)) - (rowX - c2(B)) + (T2 - rowC2 - colC2 + ci);
            sm += ci * D + (c2(A) - (rowC2 - ci)) * (c2(B) - (colC2 - ci));
            if (x) dc += x * (X * A * B - A * (colIR - x * Rr) - (rowIC - x * Cc) * B + (rowSq - x * x) * B + A * (colSq - x * x));
        }
    }
    // sum over r != i, c != j of I_rc I_rj I_ic I_ij, along the shorter side
    if (K <= Lc) {
        for (int r = 0; r < K; ++r)
            for (int i = r + 1; i < K; ++i) {
                long long G = 0, H = 0;
                for (int c = 0; c < Lc; ++c) { const long long a = I(r, c), b = I(i, c); G += a * b; H += a * a * b * b; }
                dc += 2 * (G * G - H);
            }
    } else {
        for (int c = 0; c < Lc; ++c)
            for (int j = c + 1; j < Lc; ++j) {
                long long G = 0, H = 0;
                for (int r = 0; r < K; ++r) { const long long a = I(r, c), b = I(r, j); G += a * b; H += a * a * b * b; }
                dc += 2 * (G * G - H);
            }
    }
    acc.sm += sm;
    acc.dc += dc;
}

// 2 x the quartets one node resolves, from its link sizes
template <class SF>
__device__ __forceinline__ long long node_resolved2(int K, SF S, long long N) {
    long long s2 = 0, out = 0;
    for (int r = 0; r < K; ++r) s2 += c2(S(r));
    for (int r = 0; r < K; ++r) { const long long x = S(r); out += c2(x) * (c2(N - x) - (s2 - c2(x))); }
    return out;
}

__device__ __forceinline__ void wave_add(unsigned long long *dst, long long v) {
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    if ((threadIdx.x % kWave) == 0 && v) atomicAdd(dst, (unsigned long long)v);
}

}  // namespace qs
