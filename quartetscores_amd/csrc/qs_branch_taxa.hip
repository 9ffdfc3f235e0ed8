// qs_branch_taxa.hip -- quartet sums of every reference internode through every listed taxon on gfx950 (qs_branch_taxon_support).
//
// Replaces nothing in the reference: it never asks what a branch's support would be without one taxon.
//
// QP-IC of an internode e is log_score of three sums over the 4-sets "around" e: those the reference resolves with its two junction
// nodes at the two ends of e (what processNodePair sums for an adjacent node pair). For a listed taxon x this
// kernel sums, per internode, the same three counts and the number of 4-sets over the 4-sets around e that HOLD x: row x of
// qs_branch_taxon_support. They are the tuples of x's gather (qs_taxon_walk.hpp: a wave owns the middle id q, its lanes 64 largest ids
// r, the steps are p). In every address case the tuple's three cells are n(ab|cd), n(ac|bd), n(ad|bc) of the SORTED ids a<b<c<d,
// which is all classify() (qs_score.hip) needs:
//   x > r      (p,q,r,x)  e01 = lca(p,q)  e12 = lca(q,r)  e23 = lca(r,x)
//   q < x < r  (p,q,x,r)  e01 = lca(p,q)  e12 = lca(q,x)  e23 = lca(x,r)
//   p < x < q  (p,x,q,r)  e01 = lca(p,x)  e12 = lca(x,q)  e23 = lca(q,r)
//   x < p      (x,p,q,r)  e01 = lca(x,p)  e12 = lca(p,q)  e23 = lca(q,r)
// lca(p,q) and lca(p,x) are wave-uniform per step, lca(q,x) per walk; lca(q,r) and lca(x,r) are lane constants. Topology, the two
// junctions and the order of (q1,q2,q3) are classify()'s in the frame qs_score uses without flags. A 4-set counts if it is resolved
// and one junction is the other's parent (par[], compact inner ids; under a degree-2 root par[second child] = first child: the two
// are the ends of ONE internode, whose words go to both children's entries at the flush).
// A lane's topology and target edge are constant over a run of p: until lca(p,q) or lca(p,x) changes or p passes x (next[][], the
// breakpoints of every row of the LCA matrix on both sides of its diagonal, merged on the fly: the smaller of the rows q and x). Over
// a run a lane adds the three raw cells; at its end it hands in (steps, F1, F2, F3) to the workgroup's accumulators in LDS, indexed
// by the compact id of the edge's child node -- summed over the wave first where every counting lane has the same target and
// topology, else one LDS atomic per word and lane. The workgroup flushes its non-zero cells with one 64-bit atomic each into row
// blockIdx.y: integer sums, independent of order, grid and repetition.
// 32-bit run sums need 4096 x (largest count) < 2^32 and at most 4096 taxa (a run has fewer than q steps); the host picks the WIDE
// instance otherwise (the rule of qs_taxon_placement).
#include "qs_taxon_walk.hpp"

namespace qs {

constexpr uint32_t kBranchNone = 0xFFFFFFFFu;

template <typename CT, typename ACC>
__global__ __launch_bounds__(kPlaceWaves * kWave) void branch_taxa_kernel(BranchDevice bd, unsigned long long *__restrict__ dst) {
    extern __shared__ __align__(16) unsigned char branch_smem[];
    typedef unsigned long long u64;
    u64 *acc = reinterpret_cast<u64 *>(branch_smem);                                // [inner id of the edge's child][word]
    uint32_t *par = reinterpret_cast<uint32_t *>(acc + (size_t)bd.n_inner * kBranchWords);   // [inner id]
    constexpr int kThreads = kPlaceWaves * kWave, CH = WalkChunk<CT>::CH;
    const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const uint32_t n = bd.g.n, cells = bd.n_inner * kBranchWords;
    const uint32_t x = bd.g.taxa[blockIdx.y];
    walk_zero(acc, cells);
    for (uint32_t i = tid; i < bd.n_inner; i += kThreads) par[i] = bd.par[i];
    __syncthreads();
    const uint32_t *__restrict__ L = bd.g.ref_lca;
    const uint32_t *__restrict__ xrow = L + (size_t)x * n;
    const uint16_t *__restrict__ nx = bd.next + (size_t)x * n;
    const uint32_t code_ad = bd.frame == 0 ? 1u : 2u;      // ad|bc: (q1,q2,q3) = (n2,n1,n0) in the node-pair frame, (n2,n0,n1) in the other
    for (uint32_t task = blockIdx.x * kPlaceWaves + wave; task < bd.g.n_tasks; task += gridDim.x * kPlaceWaves) {   // uniform over the wave
        TaxonWalk<CT> w;
        if (!w.begin(__builtin_amdgcn_readfirstlane(bd.g.tasks[task]), x, n, lane, reinterpret_cast<const CT *>(bd.g.table))) continue;
        const uint32_t q = w.q, r = w.r;
        const bool live = w.live;
        const uint32_t *__restrict__ lrow = L + (size_t)q * n;
        const uint16_t *__restrict__ nq = bd.next + (size_t)q * n;
        const uint32_t eXQ = __builtin_amdgcn_readfirstlane(xrow[q]);   // uniform
        const uint32_t eQR = lrow[r], eXR = xrow[r];                    // lane constants
        const bool xlow = x < q;                                        // uniform
        const uint32_t e12_hi = x > r ? eQR : eXQ;                      // x behind q: everything but lca(p,q) is a lane constant
        uint32_t end = 0, len = 0;                          // uniform: the run's end, its steps so far
        bool has = false, uni = false;                      // this lane counts in the run; every counting lane has the target and code below
        uint32_t tgt = 0, code = 0, n_has = 0, ukey = 0;     // ukey (uniform): target << 2 | code of the first counting lane
        ACC S0 = 0, S1 = 0, S2 = 0;                         // the lane's raw cell sums of the run
        auto hand_in = [&]() {
            if (len == 0 || n_has == 0) return;             // uniform
            if (uni) {
                const u64 s0 = wave_sum_exact(has ? S0 : (ACC)0), s1 = wave_sum_exact(has ? S1 : (ACC)0), s2 = wave_sum_exact(has ? S2 : (ACC)0);
                const uint32_t t = ukey >> 2, c = ukey & 3u;
                if (lane < (uint32_t)kBranchWords) {
                    const u64 v = lane == 0 ? (u64)len * n_has : lane == 1 ? (c == 0 ? s0 : s2) : lane == 2 ? (c == 2 ? s0 : s1) : (c == 0 ? s2 : c == 1 ? s0 : s1);
                    if (v) atomicAdd(&acc[t * kBranchWords + lane], v);
                }
            } else if (has) {
                const u64 f1 = code == 0 ? S0 : S2, f2 = code == 2 ? S0 : S1, f3 = code == 0 ? S2 : code == 1 ? S0 : S1;
                u64 *cell = acc + tgt * kBranchWords;
                atomicAdd(&cell[0], (u64)len);
                if (f1) atomicAdd(&cell[1], f1);
                if (f2) atomicAdd(&cell[2], f2);
                if (f3) atomicAdd(&cell[3], f3);
            }
        };
        for (uint32_t p0 = 0; p0 < q; p0 += CH) {           // uniform
            w.load(p0);
#pragma unroll
            for (int u = 0; u < CH; ++u) {
                const uint32_t p = p0 + u;
                if (p < q) {                                // uniform
                    if (p == end) {                         // uniform: lca(p,q) or lca(p,x) changes here, or p has passed x
                        hand_in();
                        S0 = 0; S1 = 0; S2 = 0; len = 0;
                        const uint32_t ePQ = __builtin_amdgcn_readfirstlane(lrow[p]);
                        end = __builtin_amdgcn_readfirstlane((uint32_t)nq[p]);
                        uint32_t e01 = ePQ, e12 = e12_hi, e23 = eXR;
                        if (xlow) {                         // uniform
                            e01 = __builtin_amdgcn_readfirstlane(xrow[p]);
                            end = min(end, __builtin_amdgcn_readfirstlane((uint32_t)nx[p]));
                            e12 = p < x ? eXQ : ePQ;
                            e23 = eQR;
                        }
                        // classify() on the sorted ids: topology, junctions, and the edge between them if they are adjacent
                        const uint32_t d01 = e01 >> 16, d12 = e12 >> 16, d23 = e23 >> 16;
                        const uint32_t i01 = e01 & 0xFFFFu, i12 = e12 & 0xFFFFu, i23 = e23 & 0xFFFFu;
                        const uint32_t mx = max(d01, d23);
                        const bool ab = d12 < mx;
                        const uint32_t j1 = ab ? (d01 > d12 ? i01 : i12) : i12;
                        const uint32_t j2 = ab ? (d23 > d12 ? i23 : i12) : (d01 >= d23 ? i01 : i23);
                        const uint32_t p1 = par[j1], p2 = par[j2];
                        code = ab ? 0u : code_ad;
                        tgt = p1 == j2 ? j1 : j2;
                        has = live && d12 != mx && (p1 == j2 || p2 == j1);
                        const unsigned long long m = __ballot(has);
                        n_has = (uint32_t)__popcll(m);
                        uni = false;
                        if (n_has) {                        // uniform
                            const uint32_t key = tgt << 2 | code;
                            ukey = __builtin_amdgcn_readfirstlane((uint32_t)__shfl((int)key, __ffsll((long long)m) - 1, kWave));
                            uni = __all(!has || key == ukey) != 0;
                        }
                    }
                    if (p != x) {                           // uniform
                        S0 += w.t[u][0]; S1 += w.t[u][1]; S2 += w.t[u][2]; ++len;
                    }
                }
            }
        }
        hand_in();
    }
    __syncthreads();
    // (not walk_flush: cell j of LDS is node inner_node[j] of the row, and the merged root internode goes to both its ends)
    unsigned long long *out = dst + (size_t)blockIdx.y * bd.n_nodes * kBranchWords;
    for (uint32_t i = tid; i < cells; i += kThreads) {
        const unsigned long long v = acc[i];
        if (v) {
            const uint32_t j = i / kBranchWords, k = i % kBranchWords;
            atomicAdd(&out[(size_t)bd.inner_node[j] * kBranchWords + k], v);
            if (j == bd.dup_from) atomicAdd(&out[(size_t)bd.dup_to * kBranchWords + k], v);
        }
    }
}

size_t branch_taxa_lds_bytes(uint32_t n_inner) { return (size_t)n_inner * (kBranchWords * 8 + 4); }

// dst (n_list rows of n_nodes x 4 words, zeroed by the caller) += the sums of the taxa bd.g.taxa[0 .. n_list)
hipError_t launch_branch_taxa(hipStream_t s, const BranchDevice &bd, uint32_t n_list, bool wide, int n_cu, unsigned long long *dst) {
    return gather_dispatch(bd.g.count_bits, wide, [&](auto ct, auto sum) {
        return launch_list_gather(branch_taxa_kernel<decltype(ct), decltype(sum)>, s, bd, bd.g, branch_taxa_lds_bytes(bd.n_inner), n_list, n_cu, dst);
    });
}

// totals of the internodes from the node-pair sums of a score pass 1 (sums = n_inner x n_inner x 3 words, key = lo * n_inner + hi):
// dst[v] = (quartets[v], sums[edge_key[v]]) for the nodes v with an internode (edge_key != none), 0 elsewhere
__global__ void branch_totals_kernel(const unsigned long long *__restrict__ sums, const uint32_t *__restrict__ edge_key,
                                     const unsigned long long *__restrict__ quartets, uint32_t n_nodes, unsigned long long *__restrict__ dst) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n_nodes) return;
    const uint32_t key = edge_key[v];
    const bool on = key != kBranchNone;
    dst[(size_t)v * kBranchWords + 0] = on ? quartets[v] : 0ull;
#pragma unroll
    for (int k = 0; k < 3; ++k) dst[(size_t)v * kBranchWords + 1 + k] = on ? sums[(size_t)key * 3 + k] : 0ull;
}

hipError_t launch_branch_totals(hipStream_t s, const unsigned long long *sums, const uint32_t *edge_key, const unsigned long long *quartets,
                                uint32_t n_nodes, unsigned long long *dst) {
    if (n_nodes == 0) return hipSuccess;
    hipLaunchKernelGGL(branch_totals_kernel, dim3((n_nodes + 255) / 256), dim3(256), 0, s, sums, edge_key, quartets, n_nodes, dst);
    return hipGetLastError();
}

} // namespace qs
