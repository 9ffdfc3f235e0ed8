// qs_taxon_walk.hpp -- the gather of the table tuples that hold one taxon x, shared by qs_place.hip, qs_taxon_pairs.hip,
// qs_branch_taxa.hip and (chunk loads, placement accounting) qs_place_clade.hip.
//
// A wave owns the middle id q, its lanes own 64 consecutive largest ids r > q and walk p = 0 .. q-1 in lockstep, skipping p = x: one
// tuple per step and lane, the one of the 4-set {x,p,q,r}. Where x stands among the sorted ids decides the tuple's address and which
// of its three cells belongs to p, q and r:
//   x > r      (p,q,r,x)  rank C(x,4) + C(r,3) + C(q,2) + p   cells (r, q, p)   consecutive in p
//   q < x < r  (p,q,x,r)  rank C(r,4) + C(x,3) + C(q,2) + p   cells (r, p, q)   consecutive in p
//   p < x < q  (p,x,q,r)  rank C(r,4) + C(q,3) + C(x,2) + p   cells (p, r, q)   consecutive in p
//   x < p      (x,p,q,r)  rank C(r,4) + C(q,3) + C(p,2) + x   cells (p, q, r)   one tuple per table row: scattered
// The consecutive stretch [0, min(q,x)) is streamed in 96-byte chunks of 16-byte loads like the bundle kernels' rows (qs_score.hip,
// qs_taxon.hip); its last steps and the scattered tuples behind it are read tuple by tuple. What a kernel does with a step's tuple is
// its own; its sums live in 64-bit LDS words, flushed with one 64-bit atomic per non-zero word: integer sums, independent of order,
// grid and repetition.
#pragma once
#include <algorithm>

#include "qs_common.hpp"
#include "qs_internal.hpp"
#include "qs_wave_sum.hpp"

namespace qs {

typedef uint32_t walk_u32x4 __attribute__((ext_vector_type(4)));
typedef walk_u32x4 walk_u32x4_a2 __attribute__((aligned(2)));   // rows and pieces start at any tuple

template <typename CT> struct WalkChunk {
    static constexpr int CH = sizeof(CT) == 2 ? 16 : 8;         // tuples a lane requests at once: 96 bytes of its row
    static constexpr int NV = CH * 3 * (int)sizeof(CT) / 16;    // as 16-byte loads
};

// t[u][k] (ADD: +=) the cell k of the CH tuples that start at src (96 bytes); a lane that is not live reads nothing and sees zeros
template <bool ADD, typename CT, typename T>
__device__ __forceinline__ void walk_chunk(const CT *src, bool live, T (&t)[WalkChunk<CT>::CH][3]) {
    constexpr int CH = WalkChunk<CT>::CH, NV = WalkChunk<CT>::NV;
    uint32_t w[NV * 4];
#pragma unroll
    for (int j = 0; j < NV * 4; ++j) w[j] = 0;
    if (live) {
        const walk_u32x4_a2 *v = reinterpret_cast<const walk_u32x4_a2 *>(src);
#pragma unroll
        for (int j = 0; j < NV; ++j) { const walk_u32x4 x = v[j]; w[4 * j] = x.x; w[4 * j + 1] = x.y; w[4 * j + 2] = x.z; w[4 * j + 3] = x.w; }
    }
#pragma unroll
    for (int u = 0; u < CH; ++u)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int e = 3 * u + k;
            const uint32_t cell = sizeof(CT) == 4 ? w[e] : ((w[e >> 1] >> (16 * (e & 1))) & 0xFFFFu);
            if (ADD) t[u][k] += (T)cell; else t[u][k] = (T)cell;
        }
}

// the walk of one task word (q | group of 64 largest ids << 16) for the taxon x
template <typename CT> struct TaxonWalk {
    static constexpr int CH = WalkChunk<CT>::CH;
    uint32_t x, q, r, seg;      // seg: the consecutive stretch is [0, seg); beyond it (x < p < q) scattered tuples
    bool live;                  // idle lanes (no such r, or r = x) read nothing of the table
    const CT *row, *scat;       // the tuple of step p: row + 3 p inside the stretch, scat + 3 C(p,2) behind it
    uint32_t t[CH][3];          // the chunk load() read last: the tuple of step p0 + u (a member: as an argument by reference it costs the
                                // wide branch instance ten registers and a wave)
    uint32_t pp, pq, pr;        // inside the stretch: the index of the cell of p, of q, of r (behind it: 0, 1, 2)

    // false: q is x itself, the task has no walk (uniform)
    __device__ __forceinline__ bool begin(uint32_t task_word, uint32_t x_, uint32_t n, uint32_t lane, const CT *table) {
        x = x_;
        q = task_word & 0xFFFFu;
        if (q == x) return false;
        const uint32_t r_raw = q + 1 + (task_word >> 16) * kWave + lane;
        live = r_raw < n && r_raw != x;
        r = live ? r_raw : q + 1;   // (q + 1 < n keeps the idle lanes' tree lookups in range)
        seg = min(q, x);
        uint64_t rank0;
        if (x < q) { rank0 = binom4(r) + binom3(q) + binom2(x); pp = 0; pq = 2; pr = 1; }
        else if (x < r) { rank0 = binom4(r) + binom3(x) + binom2(q); pp = 1; pq = 2; pr = 0; }
        else { rank0 = binom4(x) + binom3(r) + binom2(q); pp = 2; pq = 1; pr = 0; }
        row = table + rank0 * 3;
        scat = table + (binom4(r) + binom3(q) + x) * 3;
        return true;
    }
    // t[u] = the tuple of step p0 + u (zeros where there is none: p >= q, p = x, idle lane); p0 uniform
    __device__ __forceinline__ void load(uint32_t p0) {
        if (p0 + CH <= seg) walk_chunk<false>(row + 3 * (size_t)p0, live, t);   // the whole chunk lies in the consecutive stretch
        else {
#pragma unroll
            for (int u = 0; u < CH; ++u) {
                const uint32_t p = p0 + u;
                t[u][0] = t[u][1] = t[u][2] = 0;
                if (live && p < q && p != x) {
                    const CT *src = p < seg ? row + 3 * (size_t)p : scat + 3 * binom2(p);
                    t[u][0] = src[0]; t[u][1] = src[1]; t[u][2] = src[2];
                }
            }
        }
    }
    // the counts of the tuple of step p = p0 + u that belong to p, q and r: n(xp|qr), n(xq|pr), n(xr|pq)
    __device__ __forceinline__ void cells(uint32_t p, int u, uint32_t &vp, uint32_t &vq, uint32_t &vr) const {
        const uint32_t (&tu)[3] = t[u];
        const bool lo = p < seg;    // uniform: the row's cell order, else (p, q, r)
        const uint32_t ip = lo ? pp : 0u, iq = lo ? pq : 1u, ir = lo ? pr : 2u;
        vp = ip == 0 ? tu[0] : ip == 1 ? tu[1] : tu[2];
        vq = iq == 0 ? tu[0] : iq == 1 ? tu[1] : tu[2];
        vr = ir == 0 ? tu[0] : ir == 1 ? tu[1] : tu[2];
    }
};

// The placement accounting of one walk: the three counts of a triple p < q < r go to the links of its median node
// that lead towards p, q and r. With P = lca(p,q) (wave-uniform, constant over a run of p) and Q = lca(q,r) (a lane constant), both
// ancestors of q:
//   P deeper   m = P: p -> child of P holding p, q -> child of P holding q, r -> P's parent link: targets are wave-uniform,
//              the lanes' run sums are added over the wave and lane 0 hands them in at the run's end;
//   Q deeper   m = Q: p -> Q's parent link, q, r -> the children of Q holding them: lane constants, summed over the whole walk;
//   P = Q      p -> child of P holding p (uniform), q, r -> as for "Q deeper".
// A run ends where lca(p,q) OR the child of it that holds p changes (next[q][p], see PlaceDevice).
template <typename ACC> struct PlaceAccount {
    typedef unsigned long long u64;
    const uint32_t *inner_node, *lrow;
    const uint16_t *child, *nrow, *crow;
    uint32_t n, N, q;
    bool live;
    uint32_t dQ, upQ, lq, lr;                       // the lane's constants: Q's depth, its parent link, its children towards q and r
    uint32_t end = 0, cp = 0, cq = 0, upP = 0;      // uniform: the run's end and its three targets
    bool c1 = false, c13 = false, c2 = false, c23 = false, any1 = false, any13 = false;
    ACC Ucp = 0, Ucq = 0, Uup = 0;                  // the lane's share of the run's wave-uniform targets
    ACC Aup = 0, Alq = 0, Alr = 0;                  // the lane's own targets, over the whole walk

    __device__ __forceinline__ void begin(const uint32_t *ref_lca, const uint32_t *inner_node_, const uint16_t *child_, const uint16_t *next,
                                          uint32_t n_, uint32_t n_nodes, uint32_t q_, uint32_t r, bool live_) {
        inner_node = inner_node_; child = child_; n = n_; N = n_nodes; q = q_; live = live_;
        const uint32_t eQ = ref_lca[(size_t)q * n + r];
        dQ = eQ >> 16;
        upQ = N + inner_node[eQ & 0xFFFFu];
        lq = child[(size_t)r * n + q]; lr = child[(size_t)q * n + r];
        lrow = ref_lca + (size_t)q * n; nrow = next + (size_t)q * n; crow = child + (size_t)q * n;
    }
    __device__ __forceinline__ void close_run(u64 *acc, uint32_t lane) {
        if (any13) { const u64 s = wave_sum((u64)Ucp); if (lane == 0 && s) atomicAdd(&acc[cp], s); }
        if (any1) {
            const u64 s = wave_sum((u64)Ucq), s2 = wave_sum((u64)Uup);
            if (lane == 0 && s) atomicAdd(&acc[cq], s);
            if (lane == 0 && s2) atomicAdd(&acc[upP], s2);
        }
        Ucp = 0; Ucq = 0; Uup = 0;
    }
    // before step p (uniform): where a run ends -- or `also` says so -- it is closed and the next one's state read
    __device__ __forceinline__ void run_break(uint32_t p, bool also, u64 *acc, uint32_t lane) {
        if (p == end || also) {
            close_run(acc, lane);
            const uint32_t eP = __builtin_amdgcn_readfirstlane(lrow[p]);
            const uint32_t dP = eP >> 16;
            upP = N + __builtin_amdgcn_readfirstlane(inner_node[eP & 0xFFFFu]);
            cp = __builtin_amdgcn_readfirstlane((uint32_t)crow[p]);
            cq = __builtin_amdgcn_readfirstlane((uint32_t)child[(size_t)p * n + q]);
            end = __builtin_amdgcn_readfirstlane((uint32_t)nrow[p]);
            c1 = live && dP > dQ; c2 = live && dP < dQ;
            c13 = live && dP >= dQ; c23 = live && dP <= dQ;
            any1 = __any(c1) != 0; any13 = __any(c13) != 0;
        }
    }
    __device__ __forceinline__ void step(ACC vp, ACC vq, ACC vr) {
        Ucp += c13 ? vp : (ACC)0; Ucq += c1 ? vq : (ACC)0; Uup += c1 ? vr : (ACC)0;
        Aup += c2 ? vp : (ACC)0; Alq += c23 ? vq : (ACC)0; Alr += c23 ? vr : (ACC)0;
    }
    __device__ __forceinline__ void finish(u64 *acc, uint32_t lane) {
        close_run(acc, lane);
        if (live) {
            if (Aup) atomicAdd(&acc[upQ], (u64)Aup);
            if (Alq) atomicAdd(&acc[lq], (u64)Alq);
            if (Alr) atomicAdd(&acc[lr], (u64)Alr);
        }
    }
};

// the 64-bit LDS words of a workgroup of kPlaceWaves waves: zeroed before its walks (the caller synchronises) ...
__device__ __forceinline__ void walk_zero(unsigned long long *acc, uint32_t cells) {
    for (uint32_t i = threadIdx.x; i < cells; i += kPlaceWaves * kWave) acc[i] = 0;
}
// ... and added to `out` after them, one atomic per non-zero word
__device__ __forceinline__ void walk_flush(const unsigned long long *acc, uint32_t cells, unsigned long long *out) {
    for (uint32_t i = threadIdx.x; i < cells; i += kPlaceWaves * kWave) {
        const unsigned long long v = acc[i];
        if (v) atomicAdd(&out[i], v);
    }
}

// Host: one launch over the list g.taxa[0 .. n_list), workgroup row y = list entry y. About eight workgroups per CU over the whole
// list; one taxon alone spreads its walks over as many workgroups as it has.
template <typename K, typename D>
hipError_t launch_list_gather(K kernel, hipStream_t s, const D &d, const GatherDevice &g, size_t lds, uint32_t n_list, int n_cu,
                              unsigned long long *dst) {
    if (g.n_tasks == 0 || n_list == 0) return hipSuccess;
    if (lds > 160u * 1024u || n_list > 65535u) return hipErrorInvalidValue;
    hipError_t e = hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    const uint32_t most = (g.n_tasks + kPlaceWaves - 1) / kPlaceWaves;
    const uint32_t want = ((uint32_t)std::max(1, n_cu) * 8u + n_list - 1) / n_list;
    dim3 block(kPlaceWaves * kWave), grid(std::max(1u, std::min(most, want)), n_list);
    hipLaunchKernelGGL(kernel, grid, block, lds, s, d, dst);
    return hipGetLastError();
}
// f(cell type, sum type) of the instance for a table's cell width: 16-bit cells keep 32-bit sums (4096 x 3 x 65535 < 2^32)
template <typename F> hipError_t gather_dispatch(int count_bits, bool wide, F f) {
    if (count_bits == 16) return f(uint16_t(), uint32_t());
    return wide ? f(uint32_t(), 0ull) : f(uint32_t(), uint32_t());
}

} // namespace qs
