// qs_taxon_pairs.hip -- quartet support of taxon pairs from the count table on gfx950 (qs_taxon_pair_support).
//
// Replaces nothing in the reference: it has no output per pair of taxa.
//
// For a listed taxon x and every other taxon j, over the C(n-2,2) 4-sets {x,j,k,l}: t = n(xj|kl), s = the tuple sum, split by what
// the reference tree shows for the 4-set (rt: xj|kl, ra: another resolution, neither: unresolved) into eight exact 64-bit words
// (kPairFields). Row x of the matrix comes from the tuples that hold x: the gather of qs_place.hip. A wave owns the
// middle id q, its lanes own 64 consecutive largest ids r > q and walk p = 0 .. q-1 in lockstep, skipping p = x; the four address
// cases by where x stands among the sorted ids, the 96-byte chunks of the consecutive stretch [0, min(q,x)) and the scattered tuples
// behind it are that kernel's. Of a tuple's three cells one each is the "together" count of the pairs (x,p), (x,q) and (x,r).
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
//     S_all) are summed over the wave -- DPP adds inside the rows of 16, the row totals read into scalar registers, as qs_taxon.hip
//     does for its taxon a -- the two counts are ballots, and lanes 0..7 add the eight words to p's cells. T_rt and S_rt are skipped
//     while no lane of the step shows x with p, T_all and S_all while every live lane is resolved (always, under a binary reference:
//     they are the sums of the two classes then).
// The accumulators of a workgroup are n x 8 words in LDS (145 KB at 2259 taxa), flushed with one 64-bit atomic per non-zero cell into
// row blockIdx.y: integer sums, independent of order, grid and repetition.
// 32-bit partial sums need 4096 x 3 x (largest count) < 2^32 (a walk has q < 4096 steps, s is up to three counts); the host
// (qs_taxon_pair_support) picks the WIDE instance (64-bit, shuffles) otherwise.
#include "qs_common.hpp"
#include "qs_internal.hpp"

#include <algorithm>

namespace qs {

typedef uint32_t qx_u32x4 __attribute__((ext_vector_type(4)));
typedef qx_u32x4 qx_u32x4_a2 __attribute__((aligned(2)));   // rows start at any tuple

// sum over the wave, the same value in every lane's copy: DPP inside the rows of 16, row totals by readlane (qs_taxon.hip)
__device__ __forceinline__ uint32_t pair_wave_sum(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, true);    // quad_perm [1,0,3,2]
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, true);    // quad_perm [2,3,0,1]
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, true);   // row_half_mirror
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, true);   // row_mirror
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 0) + (uint32_t)__builtin_amdgcn_readlane((int)v, 16) +
           (uint32_t)__builtin_amdgcn_readlane((int)v, 32) + (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
}
__device__ __forceinline__ unsigned long long pair_wave_sum(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
    return v;
}

template <typename CT, typename ACC>
__global__ __launch_bounds__(kPlaceWaves * kWave) void taxon_pairs_kernel(PairDevice pd, unsigned long long *__restrict__ dst) {
    extern __shared__ __align__(16) unsigned char pairs_smem[];
    unsigned long long *acc = reinterpret_cast<unsigned long long *>(pairs_smem);   // [taxon][field]
    constexpr int kThreads = kPlaceWaves * kWave;
    typedef unsigned long long u64;
    const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const uint32_t n = pd.n, cells = n * kPairFields;
    const uint32_t x = pd.taxa[blockIdx.y];
    for (uint32_t i = tid; i < cells; i += kThreads) acc[i] = 0;
    __syncthreads();
    const CT *table = reinterpret_cast<const CT *>(pd.table);
    const uint32_t *__restrict__ L = pd.ref_lca;
    const uint32_t *__restrict__ xrow = L + (size_t)x * n;
    constexpr int CH = sizeof(CT) == 2 ? 16 : 8;            // tuples a lane requests at once: 96 bytes of its row
    constexpr int NV = CH * 3 * (int)sizeof(CT) / 16;       // as 16-byte loads
    for (uint32_t task = blockIdx.x * kPlaceWaves + wave; task < pd.n_tasks; task += gridDim.x * kPlaceWaves) {   // uniform over the wave
        const uint32_t tk = __builtin_amdgcn_readfirstlane(pd.tasks[task]);
        const uint32_t q = tk & 0xFFFFu, rg = tk >> 16;
        if (q == x) continue;
        const uint32_t r_raw = q + 1 + rg * kWave + lane;
        const bool live = r_raw < n && r_raw != x;
        const uint32_t r = live ? r_raw : q + 1;   // (idle lanes read nothing of the table; q + 1 < n keeps their tree lookups in range)
        const uint32_t n_live = (uint32_t)__popcll(__ballot(live));
        const uint32_t *__restrict__ lrow = L + (size_t)q * n;
        const uint32_t dxq = __builtin_amdgcn_readfirstlane(xrow[q]) >> 16;   // uniform
        const uint32_t dqr = lrow[r] >> 16, dxr = xrow[r] >> 16;             // lane constants
        const bool xlow = x < q;                                              // uniform
        // x behind q: everything but lca(p,q) is a lane constant
        const uint32_t hi12 = x > r ? dqr : dxq;
        const uint32_t hi_second = x > r ? 0u : 1u;         // ad|bc puts x with p (0) or with q (1); ab|cd with r (2)
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
        // the lane's sums over the walk: S_all and the tuple sum of its resolved 4-sets serve q and r alike
        ACC Sall = 0, Sres = 0;
        ACC QTrt = 0, QSrt = 0, QTra = 0, QTall = 0;
        ACC RTrt = 0, RSrt = 0, RTra = 0, RTall = 0;
        uint32_t Nres = 0, Nqr = 0;                         // resolved 4-sets; those with x beside q | beside r << 16 (q < 4096 steps)
        for (uint32_t p0 = 0; p0 < q; p0 += CH) {           // uniform
            uint32_t t[CH][3];
            if (p0 + CH <= seg) {                           // the whole chunk lies in the consecutive stretch
                uint32_t w[NV * 4];
#pragma unroll
                for (int j = 0; j < NV * 4; ++j) w[j] = 0;
                if (live) {
                    const qx_u32x4_a2 *src = reinterpret_cast<const qx_u32x4_a2 *>(row + 3 * (size_t)p0);
#pragma unroll
                    for (int j = 0; j < NV; ++j) { const qx_u32x4 v = src[j]; w[4 * j] = v.x; w[4 * j + 1] = v.y; w[4 * j + 2] = v.z; w[4 * j + 3] = v.w; }
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
                    const bool lo = p < seg;                // uniform: the row's cell order, else (p, q, r)
                    const uint32_t ip = lo ? pp : 0u, iq = lo ? pq : 1u, ir = lo ? pr : 2u;
                    const uint32_t vp = ip == 0 ? t[u][0] : ip == 1 ? t[u][1] : t[u][2];
                    const uint32_t vq = iq == 0 ? t[u][0] : iq == 1 ? t[u][1] : t[u][2];
                    const uint32_t vr = ir == 0 ? t[u][0] : ir == 1 ? t[u][1] : t[u][2];
                    const ACC s = (ACC)t[u][0] + t[u][1] + t[u][2];
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
                    if (nP) { tTrt = pair_wave_sum(isP ? (ACC)vp : (ACC)0); tSrt = pair_wave_sum(isP ? s : (ACC)0); }
                    const u64 tTra = nRes ? (u64)pair_wave_sum((res && !isP) ? (ACC)vp : (ACC)0) : 0ull;
                    const u64 tSres = nRes ? (u64)pair_wave_sum(sres) : 0ull;
                    u64 tTall = tTrt + tTra, tSall = tSres;
                    if (nRes != n_live) { tTall = pair_wave_sum((ACC)vp); tSall = pair_wave_sum(s); }
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
            const u64 tq = pair_wave_sum(live ? vq8[k] : 0ull);
            if (lane == (uint32_t)k) mine = tq;
        }
        if (lane < (uint32_t)kPairFields && mine) atomicAdd(&acc[q * kPairFields + lane], mine);
    }
    __syncthreads();
    unsigned long long *out = dst + (size_t)blockIdx.y * cells;
    for (uint32_t i = tid; i < cells; i += kThreads) {
        const unsigned long long v = acc[i];
        if (v) atomicAdd(&out[i], v);
    }
}

size_t taxon_pairs_lds_bytes(uint32_t n) { return (size_t)n * kPairFields * 8; }

template <typename CT, typename ACC>
static hipError_t launch_pairs_t(hipStream_t s, const PairDevice &pd, uint32_t n_list, int n_cu, unsigned long long *dst) {
    if (pd.n_tasks == 0 || n_list == 0) return hipSuccess;
    const size_t lds = taxon_pairs_lds_bytes(pd.n);
    if (lds > 160u * 1024u || n_list > 65535u) return hipErrorInvalidValue;
    auto k = taxon_pairs_kernel<CT, ACC>;
    hipError_t e = hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    // the placement gather's grid: about eight workgroups per CU over the whole list; one taxon alone spreads its walks over as many
    // workgroups as it has
    const uint32_t most = (pd.n_tasks + kPlaceWaves - 1) / kPlaceWaves;
    const uint32_t want = ((uint32_t)std::max(1, n_cu) * 8u + n_list - 1) / n_list;
    dim3 block(kPlaceWaves * kWave), grid(std::max(1u, std::min(most, want)), n_list);
    hipLaunchKernelGGL(k, grid, block, lds, s, pd, dst);
    return hipGetLastError();
}

// dst (n_list rows of n x 8 words, zeroed by the caller) += the pair sums of the taxa pd.taxa[0 .. n_list)
hipError_t launch_taxon_pairs(hipStream_t s, const PairDevice &pd, uint32_t n_list, bool wide, int n_cu, unsigned long long *dst) {
    if (pd.count_bits == 16) return launch_pairs_t<uint16_t, uint32_t>(s, pd, n_list, n_cu, dst);   // 4096 x 3 x 65535 < 2^32
    return wide ? launch_pairs_t<uint32_t, unsigned long long>(s, pd, n_list, n_cu, dst) : launch_pairs_t<uint32_t, uint32_t>(s, pd, n_list, n_cu, dst);
}

} // namespace qs
