// qs_place.hip -- quartet placement of taxa on the reference tree from the count table on gfx950 (qs_taxon_placement).
//
// Replaces nothing in the reference: it never asks where the evaluation trees would put a taxon.
//
// For a listed taxon x and every three other taxa p < q < r the 4-set {x,p,q,r} has one table tuple; its three counts
// n(xp|qr), n(xq|pr), n(xr|pq) go to the links of the median node m of p, q, r that lead towards p, q and r (DESIGN.md 12;
// link v = the edge into node v, link N + m = the edge from m to its parent). The host turns the 2N link sums of x into the
// score of every edge (qs_placement_scores).
//
// The tuples of x come from the gather of qs_taxon_walk.hpp, which also describes the accounting (PlaceAccount: where the median
// node lies decides whether a count's target link is wave-uniform over a run of p or a lane constant). The accumulators of a
// workgroup are 2N 64-bit words in LDS.
// 32-bit partial sums need 4096 x (largest count) < 2^32 AND at most 4096 taxa (a walk has q < n_taxa steps); the host
// (qs_taxon_placement) checks both and picks the WIDE instance otherwise.
#include "qs_taxon_walk.hpp"

namespace qs {

template <typename CT, typename ACC>
__global__ __launch_bounds__(kPlaceWaves * kWave) void place_gather_kernel(PlaceDevice pd, unsigned long long *__restrict__ dst) {
    extern __shared__ __align__(16) unsigned char place_smem[];
    unsigned long long *acc = reinterpret_cast<unsigned long long *>(place_smem);   // [link]
    constexpr int CH = WalkChunk<CT>::CH;
    const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const uint32_t n = pd.g.n, cells = 2 * pd.n_nodes;
    const uint32_t x = pd.g.taxa[blockIdx.y];
    walk_zero(acc, cells);
    __syncthreads();
    for (uint32_t task = blockIdx.x * kPlaceWaves + wave; task < pd.g.n_tasks; task += gridDim.x * kPlaceWaves) {   // uniform over the wave
        TaxonWalk<CT> w;
        if (!w.begin(__builtin_amdgcn_readfirstlane(pd.g.tasks[task]), x, n, lane, reinterpret_cast<const CT *>(pd.g.table))) continue;
        PlaceAccount<ACC> a;
        a.begin(pd.g.ref_lca, pd.inner_node, pd.child, pd.next, n, pd.n_nodes, w.q, w.r, w.live);
        for (uint32_t p0 = 0; p0 < w.q; p0 += CH) {         // uniform
            w.load(p0);
#pragma unroll
            for (int u = 0; u < CH; ++u) {
                const uint32_t p = p0 + u;
                if (p < w.q) {                              // uniform
                    a.run_break(p, false, acc, lane);
                    if (p != x) {                           // uniform
                        uint32_t vp, vq, vr;
                        w.cells(p, u, vp, vq, vr);
                        a.step((ACC)vp, (ACC)vq, (ACC)vr);
                    }
                }
            }
        }
        a.finish(acc, lane);
    }
    __syncthreads();
    walk_flush(acc, cells, dst + (size_t)blockIdx.y * cells);
}

size_t place_lds_bytes(uint32_t n_nodes) { return (size_t)n_nodes * 2 * 8; }

// dst (n_list rows of 2 x n_nodes words, zeroed by the caller) += the link sums of the taxa pd.g.taxa[0 .. n_list)
hipError_t launch_taxon_placement(hipStream_t s, const PlaceDevice &pd, uint32_t n_list, bool wide, int n_cu, unsigned long long *dst) {
    return gather_dispatch(pd.g.count_bits, wide, [&](auto ct, auto sum) {
        return launch_list_gather(place_gather_kernel<decltype(ct), decltype(sum)>, s, pd, pd.g, place_lds_bytes(pd.n_nodes), n_list, n_cu, dst);
    });
}

} // namespace qs
