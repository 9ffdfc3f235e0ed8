// qs_place.hip -- quartet placement of taxa on the reference tree from the count table on gfx950 (qs_taxon_placement).
//
// Replaces nothing in the reference: it never asks where the evaluation trees would put a taxon.
//
// For a listed taxon x and every three other taxa p < q < r the 4-set {x,p,q,r} has one table tuple; its three counts
// n(xp|qr), n(xq|pr), n(xr|pq) go to the links of the median node m of p, q, r that lead towards p, q and r (DESIGN.md 12;
// link v = the edge into node v, link N + m = the edge from m to its parent). The host turns the 2N link sums of x into the
// score of every edge (qs_placement_scores).
//
// Shape: the bundle kernels' (qs_score.hip, qs_taxon.hip). A wave owns the middle id q, its lanes own 64 consecutive
// largest ids r > q and walk p = 0 .. q-1 in lockstep, skipping p = x. Where x stands among the sorted ids decides the
// tuple's address and which of its three cells belongs to p, q and r:
//   x > r      (p,q,r,x)  rank C(x,4) + C(r,3) + C(q,2) + p   cells (r, q, p)   consecutive in p
//   q < x < r  (p,q,x,r)  rank C(r,4) + C(x,3) + C(q,2) + p   cells (r, p, q)   consecutive in p
//   p < x < q  (p,x,q,r)  rank C(r,4) + C(q,3) + C(x,2) + p   cells (p, r, q)   consecutive in p
//   x < p      (x,p,q,r)  rank C(r,4) + C(q,3) + C(p,2) + x   cells (p, q, r)   one tuple per table row: scattered
// The consecutive stretch [0, min(q,x)) is streamed in 96-byte chunks of 16-byte loads like the bundle kernels' rows.
// With P = lca(p,q) (wave-uniform, constant over a run of p) and Q = lca(q,r) (a lane constant), both ancestors of q:
//   P deeper   m = P: p -> child of P holding p, q -> child of P holding q, r -> P's parent link: targets are wave-uniform,
//              the lanes' run sums are added over the wave and lane 0 hands them in at the run's end;
//   Q deeper   m = Q: p -> Q's parent link, q, r -> the children of Q holding them: lane constants, summed over the whole walk;
//   P = Q      p -> child of P holding p (uniform), q, r -> as for "Q deeper".
// A run ends where lca(p,q) OR the child of it that holds p changes (place_next, refined from ref_next on the host: under a
// multifurcation the child changes inside a run of ref_next). The accumulators of a workgroup are 2N 64-bit words in LDS,
// flushed with one 64-bit atomic per non-zero cell: integer sums, independent of order and grid.
// 32-bit partial sums need 4096 x (largest count) < 2^32 AND at most 4096 taxa (a walk has q < n_taxa steps); the host
// (qs_taxon_placement) checks both and picks the WIDE instance otherwise.
#include "qs_common.hpp"
#include "qs_internal.hpp"

#include <algorithm>

namespace qs {

typedef uint32_t qp_u32x4 __attribute__((ext_vector_type(4)));
typedef qp_u32x4 qp_u32x4_a2 __attribute__((aligned(2)));   // rows start at any tuple

__device__ __forceinline__ unsigned long long place_wave_sum(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
    return v;
}

template <typename CT, typename ACC>
__global__ __launch_bounds__(kPlaceWaves * kWave) void place_gather_kernel(PlaceDevice pd, unsigned long long *__restrict__ dst) {
    extern __shared__ __align__(16) unsigned char place_smem[];
    unsigned long long *acc = reinterpret_cast<unsigned long long *>(place_smem);   // [link]
    constexpr int kThreads = kPlaceWaves * kWave;
    const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const uint32_t n = pd.n, N = pd.n_nodes, cells = 2 * N;
    const uint32_t x = pd.taxa[blockIdx.y];
    for (uint32_t i = tid; i < cells; i += kThreads) acc[i] = 0;
    __syncthreads();
    const CT *table = reinterpret_cast<const CT *>(pd.table);
    const uint32_t *__restrict__ L = pd.ref_lca;
    constexpr int CH = sizeof(CT) == 2 ? 16 : 8;            // tuples a lane requests at once: 96 bytes of its row
    constexpr int NV = CH * 3 * (int)sizeof(CT) / 16;       // as 16-byte loads
    for (uint32_t task = blockIdx.x * kPlaceWaves + wave; task < pd.n_tasks; task += gridDim.x * kPlaceWaves) {   // uniform over the wave
        const uint32_t tk = __builtin_amdgcn_readfirstlane(pd.tasks[task]);
        const uint32_t q = tk & 0xFFFFu, rg = tk >> 16;
        if (q == x) continue;
        const uint32_t r_raw = q + 1 + rg * kWave + lane;
        const bool live = r_raw < n && r_raw != x;
        const uint32_t r = live ? r_raw : q + 1;   // (idle lanes read nothing of the table; q + 1 < n keeps their tree lookups in range)
        // the lane's constants: Q = lca(q,r), its parent link and its children towards q and r
        const uint32_t eQ = L[(size_t)q * n + r];
        const uint32_t dQ = eQ >> 16;
        const uint32_t upQ = N + pd.inner_node[eQ & 0xFFFFu];
        const uint32_t lq = pd.child[(size_t)r * n + q], lr = pd.child[(size_t)q * n + r];
        // consecutive stretch [0, seg): where x stands behind q decides the row and the cells; beyond it (x < p < q) scattered tuples
        const uint32_t seg = min(q, x);
        uint64_t rank0;
        uint32_t perm;    // index of the cell of p | q << 2 | r << 4
        if (x < q) { rank0 = binom4(r) + binom3(q) + binom2(x); perm = 0u | 2u << 2 | 1u << 4; }
        else if (x < r) { rank0 = binom4(r) + binom3(x) + binom2(q); perm = 1u | 2u << 2 | 0u << 4; }
        else { rank0 = binom4(x) + binom3(r) + binom2(q); perm = 2u | 1u << 2 | 0u << 4; }
        const CT *row = table + rank0 * 3;
        const CT *scat = table + (binom4(r) + binom3(q) + x) * 3;   // + 3 C(p,2): the tuple of (x,p,q,r)
        const uint32_t pp = perm & 3u, pq = (perm >> 2) & 3u, pr = perm >> 4;
        const uint32_t *__restrict__ lrow = L + (size_t)q * n;
        const uint16_t *__restrict__ nrow = pd.next + (size_t)q * n;
        const uint16_t *__restrict__ crow = pd.child + (size_t)q * n;
        uint32_t end = 0, cp = 0, cq = 0, upP = 0;          // uniform: the run's end and its three targets
        bool c1 = false, c13 = false, c2 = false, c23 = false, any1 = false, any13 = false;
        ACC Ucp = 0, Ucq = 0, Uup = 0;                      // the lane's share of the run's wave-uniform targets
        ACC Aup = 0, Alq = 0, Alr = 0;                      // the lane's own targets, over the whole walk
        for (uint32_t p0 = 0; p0 < q; p0 += CH) {           // uniform
            uint32_t t[CH][3];
            if (p0 + CH <= seg) {                           // the whole chunk lies in the consecutive stretch
                uint32_t w[NV * 4];
#pragma unroll
                for (int j = 0; j < NV * 4; ++j) w[j] = 0;
                if (live) {
                    const qp_u32x4_a2 *src = reinterpret_cast<const qp_u32x4_a2 *>(row + 3 * (size_t)p0);
#pragma unroll
                    for (int j = 0; j < NV; ++j) { const qp_u32x4 v = src[j]; w[4 * j] = v.x; w[4 * j + 1] = v.y; w[4 * j + 2] = v.z; w[4 * j + 3] = v.w; }
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
                    if (p == end) {                         // uniform: lca(p,q) or its child towards p changes here
                        if (any13) { const unsigned long long s = place_wave_sum((unsigned long long)Ucp); if (lane == 0 && s) atomicAdd(&acc[cp], s); }
                        if (any1) {
                            const unsigned long long s = place_wave_sum((unsigned long long)Ucq), s2 = place_wave_sum((unsigned long long)Uup);
                            if (lane == 0 && s) atomicAdd(&acc[cq], s);
                            if (lane == 0 && s2) atomicAdd(&acc[upP], s2);
                        }
                        Ucp = 0; Ucq = 0; Uup = 0;
                        const uint32_t eP = __builtin_amdgcn_readfirstlane(lrow[p]);
                        const uint32_t dP = eP >> 16;
                        upP = N + __builtin_amdgcn_readfirstlane(pd.inner_node[eP & 0xFFFFu]);
                        cp = __builtin_amdgcn_readfirstlane((uint32_t)crow[p]);
                        cq = __builtin_amdgcn_readfirstlane((uint32_t)pd.child[(size_t)p * n + q]);
                        end = __builtin_amdgcn_readfirstlane((uint32_t)nrow[p]);
                        c1 = live && dP > dQ; c2 = live && dP < dQ;
                        c13 = live && dP >= dQ; c23 = live && dP <= dQ;
                        any1 = __any(c1) != 0; any13 = __any(c13) != 0;
                    }
                    if (p != x) {                           // uniform
                        const bool lo = p < seg;            // uniform: the row's cell order, else (p, q, r)
                        const uint32_t ip = lo ? pp : 0u, iq = lo ? pq : 1u, ir = lo ? pr : 2u;
                        const uint32_t vp = ip == 0 ? t[u][0] : ip == 1 ? t[u][1] : t[u][2];
                        const uint32_t vq = iq == 0 ? t[u][0] : iq == 1 ? t[u][1] : t[u][2];
                        const uint32_t vr = ir == 0 ? t[u][0] : ir == 1 ? t[u][1] : t[u][2];
                        Ucp += c13 ? (ACC)vp : (ACC)0; Ucq += c1 ? (ACC)vq : (ACC)0; Uup += c1 ? (ACC)vr : (ACC)0;
                        Aup += c2 ? (ACC)vp : (ACC)0; Alq += c23 ? (ACC)vq : (ACC)0; Alr += c23 ? (ACC)vr : (ACC)0;
                    }
                }
            }
        }
        if (any13) { const unsigned long long s = place_wave_sum((unsigned long long)Ucp); if (lane == 0 && s) atomicAdd(&acc[cp], s); }
        if (any1) {
            const unsigned long long s = place_wave_sum((unsigned long long)Ucq), s2 = place_wave_sum((unsigned long long)Uup);
            if (lane == 0 && s) atomicAdd(&acc[cq], s);
            if (lane == 0 && s2) atomicAdd(&acc[upP], s2);
        }
        if (live) {
            if (Aup) atomicAdd(&acc[upQ], (unsigned long long)Aup);
            if (Alq) atomicAdd(&acc[lq], (unsigned long long)Alq);
            if (Alr) atomicAdd(&acc[lr], (unsigned long long)Alr);
        }
    }
    __syncthreads();
    unsigned long long *out = dst + (size_t)blockIdx.y * cells;
    for (uint32_t i = tid; i < cells; i += kThreads) {
        const unsigned long long v = acc[i];
        if (v) atomicAdd(&out[i], v);
    }
}

size_t place_lds_bytes(uint32_t n_nodes) { return (size_t)n_nodes * 2 * 8; }

template <typename CT, typename ACC>
static hipError_t launch_place_t(hipStream_t s, const PlaceDevice &pd, uint32_t n_list, int n_cu, unsigned long long *dst) {
    if (pd.n_tasks == 0 || n_list == 0) return hipSuccess;
    const size_t lds = place_lds_bytes(pd.n_nodes);
    if (lds > 160u * 1024u || n_list > 65535u) return hipErrorInvalidValue;
    auto k = place_gather_kernel<CT, ACC>;
    hipError_t e = hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    // about eight workgroups per CU over the whole list; one taxon alone spreads its tasks over as many workgroups as it has
    const uint32_t most = (pd.n_tasks + kPlaceWaves - 1) / kPlaceWaves;
    const uint32_t want = ((uint32_t)std::max(1, n_cu) * 8u + n_list - 1) / n_list;
    dim3 block(kPlaceWaves * kWave), grid(std::max(1u, std::min(most, want)), n_list);
    hipLaunchKernelGGL(k, grid, block, lds, s, pd, dst);
    return hipGetLastError();
}

// dst (n_list rows of 2 x n_nodes words, zeroed by the caller) += the link sums of the taxa pd.taxa[0 .. n_list)
hipError_t launch_taxon_placement(hipStream_t s, const PlaceDevice &pd, uint32_t n_list, bool wide, int n_cu, unsigned long long *dst) {
    if (pd.count_bits == 16) return launch_place_t<uint16_t, uint32_t>(s, pd, n_list, n_cu, dst);   // 4096 x 65535 < 2^32
    return wide ? launch_place_t<uint32_t, unsigned long long>(s, pd, n_list, n_cu, dst) : launch_place_t<uint32_t, uint32_t>(s, pd, n_list, n_cu, dst);
}

} // namespace qs
