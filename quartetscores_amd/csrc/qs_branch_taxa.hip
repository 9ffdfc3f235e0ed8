// qs_branch_taxa.hip -- quartet sums of every reference internode through every listed taxon on gfx950 (qs_branch_taxon_support).
//
// Replaces nothing in the reference: it never asks what a branch's support would be without one taxon.
//
// QP-IC of an internode e is log_score of three sums over the 4-sets "around" e: those the reference resolves with its two junction
// nodes at the two ends of e (what processNodePair sums for an adjacent node pair). For a listed taxon x this
// kernel sums, per internode, the same three counts and the number of 4-sets over the 4-sets around e that HOLD x: row x of
// qs_branch_taxon_support. They are the tuples of x's gather (qs_place.hip): a wave owns the middle id q, its lanes own 64
// consecutive largest ids r > q and walk p = 0 .. q-1 in lockstep, skipping p = x; the four address cases, the 96-byte chunks of the
// consecutive stretch [0, min(q,x)) and the scattered tuples behind it are that kernel's. In every case the tuple's three cells are
// n(ab|cd), n(ac|bd), n(ad|bc) of the SORTED ids a<b<c<d, which is all classify() (qs_score.hip) needs:
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
#include "qs_common.hpp"
#include "qs_internal.hpp"

#include <algorithm>

namespace qs {

typedef uint32_t qb_u32x4 __attribute__((ext_vector_type(4)));
typedef qb_u32x4 qb_u32x4_a2 __attribute__((aligned(2)));   // rows start at any tuple

// sum over the wave, the same value in every lane's copy. 32-bit lane sums: two halves of 16 bits (64 x 65535 stays in a word) by DPP
// inside the rows of 16, the row totals read out (qs_taxon_pairs.hip); 64-bit ones by shuffles
__device__ __forceinline__ uint32_t branch_row_sum(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, true);    // quad_perm [1,0,3,2]
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, true);    // quad_perm [2,3,0,1]
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, true);   // row_half_mirror
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, true);   // row_mirror
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 0) + (uint32_t)__builtin_amdgcn_readlane((int)v, 16) +
           (uint32_t)__builtin_amdgcn_readlane((int)v, 32) + (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
}
__device__ __forceinline__ unsigned long long branch_wave_sum(uint32_t v) {
    return (unsigned long long)branch_row_sum(v & 0xFFFFu) + ((unsigned long long)branch_row_sum(v >> 16) << 16);
}
__device__ __forceinline__ unsigned long long branch_wave_sum(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
    return v;
}

constexpr uint32_t kBranchNone = 0xFFFFFFFFu;

template <typename CT, typename ACC>
__global__ __launch_bounds__(kPlaceWaves * kWave) void branch_taxa_kernel(BranchDevice bd, unsigned long long *__restrict__ dst) {
    extern __shared__ __align__(16) unsigned char branch_smem[];
    typedef unsigned long long u64;
    u64 *acc = reinterpret_cast<u64 *>(branch_smem);                                // [inner id of the edge's child][word]
    uint32_t *par = reinterpret_cast<uint32_t *>(acc + (size_t)bd.n_inner * kBranchWords);   // [inner id]
    constexpr int kThreads = kPlaceWaves * kWave;
    const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const uint32_t n = bd.n, cells = bd.n_inner * kBranchWords;
    const uint32_t x = bd.taxa[blockIdx.y];
    for (uint32_t i = tid; i < cells; i += kThreads) acc[i] = 0;
    for (uint32_t i = tid; i < bd.n_inner; i += kThreads) par[i] = bd.par[i];
    __syncthreads();
    const CT *table = reinterpret_cast<const CT *>(bd.table);
    const uint32_t *__restrict__ L = bd.ref_lca;
    const uint32_t *__restrict__ xrow = L + (size_t)x * n;
    const uint16_t *__restrict__ nx = bd.next + (size_t)x * n;
    const uint32_t code_ad = bd.frame == 0 ? 1u : 2u;      // ad|bc: (q1,q2,q3) = (n2,n1,n0) in the node-pair frame, (n2,n0,n1) in the other
    constexpr int CH = sizeof(CT) == 2 ? 16 : 8;            // tuples a lane requests at once: 96 bytes of its row
    constexpr int NV = CH * 3 * (int)sizeof(CT) / 16;       // as 16-byte loads
    for (uint32_t task = blockIdx.x * kPlaceWaves + wave; task < bd.n_tasks; task += gridDim.x * kPlaceWaves) {   // uniform over the wave
        const uint32_t tk = __builtin_amdgcn_readfirstlane(bd.tasks[task]);
        const uint32_t q = tk & 0xFFFFu, rg = tk >> 16;
        if (q == x) continue;
        const uint32_t r_raw = q + 1 + rg * kWave + lane;
        const bool live = r_raw < n && r_raw != x;
        const uint32_t r = live ? r_raw : q + 1;   // (idle lanes read nothing of the table; q + 1 < n keeps their tree lookups in range)
        const uint32_t *__restrict__ lrow = L + (size_t)q * n;
        const uint16_t *__restrict__ nq = bd.next + (size_t)q * n;
        const uint32_t eXQ = __builtin_amdgcn_readfirstlane(xrow[q]);   // uniform
        const uint32_t eQR = lrow[r], eXR = xrow[r];                    // lane constants
        const bool xlow = x < q;                                        // uniform
        const uint32_t e12_hi = x > r ? eQR : eXQ;                      // x behind q: everything but lca(p,q) is a lane constant
        // consecutive stretch [0, seg): where x stands behind q decides the row; beyond it (x < p < q) scattered tuples
        const uint32_t seg = min(q, x);
        uint64_t rank0;
        if (x < q) rank0 = binom4(r) + binom3(q) + binom2(x);
        else if (x < r) rank0 = binom4(r) + binom3(x) + binom2(q);
        else rank0 = binom4(x) + binom3(r) + binom2(q);
        const CT *row = table + rank0 * 3;
        const CT *scat = table + (binom4(r) + binom3(q) + x) * 3;   // + 3 C(p,2): the tuple of (x,p,q,r)
        uint32_t end = 0, len = 0;                          // uniform: the run's end, its steps so far
        bool has = false, uni = false;                      // this lane counts in the run; every counting lane has the target and code below
        uint32_t tgt = 0, code = 0, n_has = 0, ukey = 0;     // ukey (uniform): target << 2 | code of the first counting lane
        ACC S0 = 0, S1 = 0, S2 = 0;                         // the lane's raw cell sums of the run
        auto hand_in = [&]() {
            if (len == 0 || n_has == 0) return;             // uniform
            if (uni) {
                const u64 s0 = branch_wave_sum(has ? S0 : (ACC)0), s1 = branch_wave_sum(has ? S1 : (ACC)0), s2 = branch_wave_sum(has ? S2 : (ACC)0);
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
            uint32_t t[CH][3];
            if (p0 + CH <= seg) {                           // the whole chunk lies in the consecutive stretch
                uint32_t w[NV * 4];
#pragma unroll
                for (int j = 0; j < NV * 4; ++j) w[j] = 0;
                if (live) {
                    const qb_u32x4_a2 *src = reinterpret_cast<const qb_u32x4_a2 *>(row + 3 * (size_t)p0);
#pragma unroll
                    for (int j = 0; j < NV; ++j) { const qb_u32x4 v = src[j]; w[4 * j] = v.x; w[4 * j + 1] = v.y; w[4 * j + 2] = v.z; w[4 * j + 3] = v.w; }
                }
#pragma unroll
                for (int u = 0; u < CH; ++u)
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        const int e = 3 * u + k;
                        t[u][k] = sizeof(CT) == 4 ? w[e] : ((w[e >> 1] >> (16 * (e & 1))) & 0xFFFFu);
                    }
            } else {
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
                        S0 += t[u][0]; S1 += t[u][1]; S2 += t[u][2]; ++len;
                    }
                }
            }
        }
        hand_in();
    }
    __syncthreads();
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

template <typename CT, typename ACC>
static hipError_t launch_branch_t(hipStream_t s, const BranchDevice &bd, uint32_t n_list, int n_cu, unsigned long long *dst) {
    if (bd.n_tasks == 0 || n_list == 0) return hipSuccess;
    const size_t lds = branch_taxa_lds_bytes(bd.n_inner);
    if (lds > 160u * 1024u || n_list > 65535u) return hipErrorInvalidValue;
    auto k = branch_taxa_kernel<CT, ACC>;
    hipError_t e = hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    // the placement gather's grid: about eight workgroups per CU over the whole list; one taxon alone spreads its walks over as many
    // workgroups as it has
    const uint32_t most = (bd.n_tasks + kPlaceWaves - 1) / kPlaceWaves;
    const uint32_t want = ((uint32_t)std::max(1, n_cu) * 8u + n_list - 1) / n_list;
    dim3 block(kPlaceWaves * kWave), grid(std::max(1u, std::min(most, want)), n_list);
    hipLaunchKernelGGL(k, grid, block, lds, s, bd, dst);
    return hipGetLastError();
}

// dst (n_list rows of n_nodes x 4 words, zeroed by the caller) += the sums of the taxa bd.taxa[0 .. n_list)
hipError_t launch_branch_taxa(hipStream_t s, const BranchDevice &bd, uint32_t n_list, bool wide, int n_cu, unsigned long long *dst) {
    if (bd.count_bits == 16) return launch_branch_t<uint16_t, uint32_t>(s, bd, n_list, n_cu, dst);   // 4096 x 65535 < 2^32
    return wide ? launch_branch_t<uint32_t, unsigned long long>(s, bd, n_list, n_cu, dst) : launch_branch_t<uint32_t, uint32_t>(s, bd, n_list, n_cu, dst);
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
