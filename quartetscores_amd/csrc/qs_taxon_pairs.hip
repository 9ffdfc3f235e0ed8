// qs_taxon_pairs.hip -- quartet support of taxon pairs from the count table on gfx950 (qs_taxon_pair_support).
//
// Replaces nothing in the reference: it has no output per pair of taxa.
//
// For a listed taxon x and every other taxon j, over the C(n-2,2) 4-sets {x,j,k,l}: t = n(xj|kl), s = the tuple sum, split by what
// the reference tree shows for the 4-set (rt: xj|kl, ra: another resolution, neither: unresolved) into eight exact 64-bit words
// (kPairFields). Row x of the matrix comes from the tuples that hold x: the gather of qs_taxon_walk.hpp (a wave owns the
// middle id q, its lanes 64 largest ids r, the steps are p). Of a tuple's three cells one each is the "together" count of the pairs
// (x,p), (x,q) and (x,r).
//
// The reference's topology of {x,p,q,r} is the decision of classify() (qs_score.hip) on the four ids in sorted order a<b<c<d:
// d12 = depth(lca(b,c)) against mx = max(depth(lca(a,b)), depth(lca(c,d))); d12 < mx: ab|cd, d12 > mx: ad|bc, else unresolved.
//   x > r      (p,q,r,x)  d01 = lca(p,q)  d12 = lca(q,r)  d23 = lca(r,x)   ab|cd: x with r   ad|bc: x with p
//   q < x < r  (p,q,x,r)  d01 = lca(p,q)  d12 = lca(q,x)  d23 = lca(x,r)   ab|cd: x with r   ad|bc: x with q
//   p < x < q  (p,x,q,r)  d01 = lca(p,x)  d12 = lca(x,q)  d23 = lca(q,r)   ab|cd: x with p   ad|bc: x with q
//   x < p      (x,p,q,r)  d01 = lca(x,p)  d12 = lca(p,q)  d23 = lca(q,r)   ab|cd: x with p   ad|bc: x with r
// lca(x,q) is uniform per walk, lca(x,r) and lca(q,r) are lane constants, lca(p,q) and lca(x,p) are uniform per step: the rows q and
// x of the LCA matrix, read a chunk ahead through the scalar cache.
//   * pair (x,r): a lane constant; register sums over the whole walk, handed in once;
//   * pair (x,q): wave-uniform over the walk; the same register sums, one wave reduction at the walk's end, lanes 0..7 hand them in;
//   * pair (x,p): wave-uniform, another p every step. The step's values (T_rt, S_rt, T_ra, the tuple sum of the resolved lanes, T_all,
//     S_all) are summed over the wave -- qs_wave_sum.hpp, as qs_taxon.hip does for its taxon a -- the two counts are ballots, and lanes 0..7 add the eight words to p's cells. T_rt and S_rt are skipped
//     while no lane of the step shows x with p, T_all and S_all while every live lane is resolved (always, under a binary reference:
//     they are the sums of the two classes then).
// The accumulators of a workgroup are n x 8 words in LDS (145 KB at 2259 taxa), flushed with one 64-bit atomic per non-zero cell into
// row blockIdx.y: integer sums, independent of order, grid and repetition.
// 32-bit partial sums need 4096 x 3 x (largest count) < 2^32 (a walk has q < 4096 steps, s is up to three counts); the host
// (qs_taxon_pair_support) picks the WIDE instance (64-bit, shuffles) otherwise.
#include "qs_taxon_walk.hpp"

namespace qs {

template <typename CT, typename ACC>
__global__ __launch_bounds__(kPlaceWaves * kWave) void taxon_pairs_kernel(GatherDevice pd, unsigned long long *__restrict__ dst) {
    extern __shared__ __align__(16) unsigned char pairs_smem[];
    unsigned long long *acc = reinterpret_cast<unsigned long long *>(pairs_smem);   // [taxon][field]
    constexpr int CH = WalkChunk<CT>::CH;
    typedef unsigned long long u64;
    const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const uint32_t n = pd.n, cells = n * kPairFields;
    const uint32_t x = pd.taxa[blockIdx.y];
    walk_zero(acc, cells);
    __syncthreads();
    const uint32_t *__restrict__ L = pd.ref_lca;
    const uint32_t *__restrict__ xrow = L + (size_t)x * n;
    for (uint32_t task = blockIdx.x * kPlaceWaves + wave; task < pd.n_tasks; task += gridDim.x * kPlaceWaves) {   // uniform over the wave
        TaxonWalk<CT> w;
        if (!w.begin(__builtin_amdgcn_readfirstlane(pd.tasks[task]), x, n, lane, reinterpret_cast<const CT *>(pd.table))) continue;
        const uint32_t q = w.q, r = w.r;
        const bool live = w.live;
        const uint32_t n_live = (uint32_t)__popcll(__ballot(live));
        const uint32_t *__restrict__ lrow = L + (size_t)q * n;
        const uint32_t dxq = __builtin_amdgcn_readfirstlane(xrow[q]) >> 16;   // uniform
        const uint32_t dqr = lrow[r] >> 16, dxr = xrow[r] >> 16;             // lane constants
        const bool xlow = x < q;                                              // uniform
        // x behind q: everything but lca(p,q) is a lane constant
        const uint32_t hi12 = x > r ? dqr : dxq;
        const uint32_t hi_second = x > r ? 0u : 1u;         // ad|bc puts x with p (0) or with q (1); ab|cd with r (2)
        // the lane's sums over the walk: S_all and the tuple sum of its resolved 4-sets serve q and r alike
        ACC Sall = 0, Sres = 0;
        ACC QTrt = 0, QSrt = 0, QTra = 0, QTall = 0;
        ACC RTrt = 0, RSrt = 0, RTra = 0, RTall = 0;
        uint32_t Nres = 0, Nqr = 0;                         // resolved 4-sets; those with x beside q | beside r << 16 (q < 4096 steps)
        for (uint32_t p0 = 0; p0 < q; p0 += CH) {           // uniform
            w.load(p0);
            // lca(p,q) and lca(x,p) of the chunk's steps: uniform loads (p < q < n: inside the rows)
            uint32_t dpq[CH], dxp[CH];
#pragma unroll
            for (int u = 0; u < CH; ++u) {
                const uint32_t p = min(p0 + u, q - 1);
                dpq[u] = __builtin_amdgcn_readfirstlane(lrow[p]) >> 16;
                dxp[u] = __builtin_amdgcn_readfirstlane(xrow[p]) >> 16;
            }
#pragma unroll
            for (int u = 0; u < CH; ++u) {
                const uint32_t p = p0 + u;
                if (p < q && p != x) {                      // uniform
                    const bool lo = p < w.seg;              // uniform: inside the consecutive stretch
                    uint32_t vp, vq, vr;
                    w.cells(p, u, vp, vq, vr);
                    const ACC s = (ACC)w.t[u][0] + w.t[u][1] + w.t[u][2];
                    // classify() on the sorted ids; with: x's neighbour, 0 = p, 1 = q, 2 = r
                    const uint32_t d01 = xlow ? dxp[u] : dpq[u];
                    const uint32_t d12 = xlow ? (lo ? dxq : dpq[u]) : hi12;
                    const uint32_t d23 = xlow ? dqr : dxr;
                    const uint32_t mx = max(d01, d23);
                    const bool res = live && d12 != mx;
                    const uint32_t with = d12 < mx ? (xlow ? 0u : 2u) : (xlow ? (lo ? 1u : 2u) : hi_second);
                    const bool isP = res && with == 0, isQ = res && with == 1, isR = res && with == 2;
                    const ACC sres = res ? s : (ACC)0;
                    Sall += s; Sres += sres; Nres += res ? 1u : 0u;
                    Nqr += (isQ ? 1u : 0u) | (isR ? 0x10000u : 0u);
                    QTall += vq; QTrt += isQ ? (ACC)vq : (ACC)0; QSrt += isQ ? s : (ACC)0; QTra += (res && !isQ) ? (ACC)vq : (ACC)0;
                    RTall += vr; RTrt += isR ? (ACC)vr : (ACC)0; RSrt += isR ? s : (ACC)0; RTra += (res && !isR) ? (ACC)vr : (ACC)0;
                    // pair (x,p): the step's sums over the wave, then eight words to p's cells
                    const uint32_t nP = (uint32_t)__popcll(__ballot(isP)), nRes = (uint32_t)__popcll(__ballot(res));
                    u64 tTrt = 0, tSrt = 0;
                    if (nP) { tTrt = wave_sum(isP ? (ACC)vp : (ACC)0); tSrt = wave_sum(isP ? s : (ACC)0); }
                    const u64 tTra = nRes ? (u64)wave_sum((res && !isP) ? (ACC)vp : (ACC)0) : 0ull;
                    const u64 tSres = nRes ? (u64)wave_sum(sres) : 0ull;
                    u64 tTall = tTrt + tTra, tSall = tSres;
                    if (nRes != n_live) { tTall = wave_sum((ACC)vp); tSall = wave_sum(s); }
                    if (lane < (uint32_t)kPairFields) {
                        const u64 v = lane == 0 ? nP : lane == 1 ? nRes - nP : lane == 2 ? tTrt : lane == 3 ? tSrt
                                      : lane == 4 ? tTra : lane == 5 ? tSres - tSrt : lane == 6 ? tTall : tSall;
                        if (v) atomicAdd(&acc[p * kPairFields + lane], v);
                    }
                }
            }
        }
        // pair (x,r): the lane's own; pair (x,q): the lanes' sums over the wave
        const uint32_t nQ = Nqr & 0xFFFFu, nR = Nqr >> 16;
        const u64 vr8[kPairFields] = {nR, Nres - nR, (u64)RTrt, (u64)RSrt, (u64)RTra, (u64)Sres - (u64)RSrt, (u64)RTall, (u64)Sall};
        const u64 vq8[kPairFields] = {nQ, Nres - nQ, (u64)QTrt, (u64)QSrt, (u64)QTra, (u64)Sres - (u64)QSrt, (u64)QTall, (u64)Sall};
        u64 mine = 0;
#pragma unroll
        for (int k = 0; k < kPairFields; ++k) {
            if (live && vr8[k]) atomicAdd(&acc[r * kPairFields + k], vr8[k]);
            const u64 tq = wave_sum(live ? vq8[k] : 0ull);
            if (lane == (uint32_t)k) mine = tq;
        }
        if (lane < (uint32_t)kPairFields && mine) atomicAdd(&acc[q * kPairFields + lane], mine);
    }
    __syncthreads();
    walk_flush(acc, cells, dst + (size_t)blockIdx.y * cells);
}

size_t taxon_pairs_lds_bytes(uint32_t n) { return (size_t)n * kPairFields * 8; }

// dst (n_list rows of n x 8 words, zeroed by the caller) += the pair sums of the taxa pd.taxa[0 .. n_list)
hipError_t launch_taxon_pairs(hipStream_t s, const GatherDevice &pd, uint32_t n_list, bool wide, int n_cu, unsigned long long *dst) {
    return gather_dispatch(pd.count_bits, wide, [&](auto ct, auto sum) {
        return launch_list_gather(taxon_pairs_kernel<decltype(ct), decltype(sum)>, s, pd, pd, taxon_pairs_lds_bytes(pd.n), n_list, n_cu, dst);
    });
}

} // namespace qs
