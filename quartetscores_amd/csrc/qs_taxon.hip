// qs_taxon.hip -- per-taxon quartet support from the count table on gfx950 (qs_taxon_support).
//
// Replaces nothing in the reference; the nearest is printRawQICScores (QuartetScoreComputer.hpp:612-680), whose text
// file (one line per quartet) a user would have to reduce on the host to get the same sums.
//
// For every taxon x, over the 4-sets that contain x: six exact 64-bit sums (kTaxonFields). The reference's
// topology of a 4-set a<b<c<d is the decision of classify() (qs_score.hip): depth(lca(b,c)) against
// max(depth(lca(a,b)), depth(lca(c,d))). Only q1 (the reference topology's count), the tuple sum and max(q2,q3) enter,
// so the node-pair frame and a degree-2 root play no part.
//
// Shape: the score bundle kernel's. A wave takes 64 table rows with the same b -- 64 consecutive pairs (c,d) -- and
// walks them in lockstep along a; a lane streams its own row in 96-byte chunks requested as 16-byte loads back to back
// (the load shape that reads this table fastest). b, a and lca(a,b) are wave-uniform, lca(b,c) and
// lca(c,d) are lane constants, and the topology changes only at the breakpoints ref_next[b][a].
//   * taxa b, c, d: plain per-lane sums over the whole row (32-bit per chunk, widened once per chunk), handed in once
//     per row: c and d by LDS atomics, b after a wave reduction;
//   * taxon a: the 64 lanes of a step all hold the SAME a, so an indexed LDS add per lane would be 64 updates of one
//     address. Instead the step's four 32-bit partial values (q1 of the resolved lanes, tuple sum of the resolved
//     lanes, tuple sum of all lanes, three packed counts) are summed over the wave -- four DPP adds inside each row of
//     16 lanes, the four row totals read into scalar registers -- and lanes 0..5 add the six words to a's cells. The
//     third value is skipped while every lane of the run is resolved (always, under a binary reference).
// The accumulators of a workgroup are n x 6 words in LDS (108 KB at 2259 taxa) and go to memory with one 64-bit atomic
// per non-zero cell when the workgroup ends: integer sums, independent of order and grid.
// 32-bit partial sums need 64 x 3 x (largest count) < 2^32; the host picks the WIDE instance (64-bit, shuffles) otherwise.
#include "qs_common.hpp"
#include "qs_internal.hpp"
#include "qs_wave_sum.hpp"

#include <algorithm>

namespace qs {

constexpr int kTaxonFields = 6;   // ref_resolved, concordant, discordant, eval_only, outvoted, uninformed

typedef uint32_t qt_u32x4 __attribute__((ext_vector_type(4)));
typedef qt_u32x4 qt_u32x4_a2 __attribute__((aligned(2)));   // rows start at any tuple

template <typename CT> __device__ __forceinline__ void taxon_load_tuple(const CT *p, uint32_t &n0, uint32_t &n1, uint32_t &n2) {
    n0 = p[0]; n1 = p[1]; n2 = p[2];
}

// ACC = uint32_t: 32-bit partial sums per step and chunk (64 x 3 x largest count < 2^32); unsigned long long: any counts
template <typename CT, typename ACC, int WAVES>
__global__ __launch_bounds__(WAVES * kWave) void taxon_bundle_kernel(ScoreDevice sd, unsigned long long *__restrict__ dst) {
    extern __shared__ __align__(16) unsigned char taxon_smem[];
    unsigned long long *acc = reinterpret_cast<unsigned long long *>(taxon_smem);   // [taxon][field]
    constexpr int kThreads = WAVES * kWave;
    const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const uint32_t n = sd.n, cells = n * kTaxonFields;
    for (uint32_t i = tid; i < cells; i += kThreads) acc[i] = 0;
    __syncthreads();
    const CT *table = reinterpret_cast<const CT *>(sd.table);
    const uint32_t *__restrict__ L = sd.ref_lca;
    constexpr int CH = sizeof(CT) == 2 ? 16 : 8;            // tuples a lane requests at once: 96 bytes of its row
    constexpr int NV = CH * 3 * (int)sizeof(CT) / 16;       // as 16-byte loads
    for (uint32_t round = blockIdx.x; round < sd.n_rounds; round += gridDim.x) {
        const uint32_t rk = sd.bundle_rounds[2 * round], rg = sd.bundle_rounds[2 * round + 1];
        const uint32_t b = __builtin_amdgcn_readfirstlane(rk * WAVES + wave);
        const uint32_t pcnt = b < n ? sd.bundle_pcnt[b] : 0u;
        if (pcnt <= rg * kWave) continue;                                         // uniform over the wave
        const bool live = rg * kWave + lane < pcnt;
        const uint32_t p = sd.bundle_plo[b] + min(rg * kWave + lane, pcnt - 1);   // (idle lanes repeat the last row and add nothing)
        uint32_t c, d;
        unrank2(p, c, d);
        c += b + 1; d += b + 1;
        const CT *row = table + (rank4(0, b, c, d) - sd.rank_lo) * 3;
        const uint32_t d12 = L[(size_t)c * n + b] >> 16, d23 = L[(size_t)d * n + c] >> 16;
        const uint32_t *__restrict__ lrow = L + (size_t)b * n;
        const uint16_t *__restrict__ nrow = sd.ref_next + (size_t)b * n;
        bool res = false, first = false, any_open = true;   // any_open (uniform): some live lane of the run is unresolved
        uint32_t end = 0;
        unsigned long long LX = 0, LW = 0, LZ = 0;          // the lane's row: q1 | tuple sum of its resolved quartets, tuple sum of all
        uint32_t LR = 0, LO = 0, LU = 0;                    // ... resolved, outvoted, uninformed
        for (uint32_t a0 = 0; a0 < b; a0 += CH) {           // uniform
            uint32_t q[CH][3];
            if (a0 + CH <= b) {                             // the whole chunk lies in the row
                uint32_t w[NV * 4];
                const qt_u32x4_a2 *src = reinterpret_cast<const qt_u32x4_a2 *>(row + 3 * (size_t)a0);
#pragma unroll
                for (int j = 0; j < NV; ++j) { const qt_u32x4 v = src[j]; w[4 * j] = v.x; w[4 * j + 1] = v.y; w[4 * j + 2] = v.z; w[4 * j + 3] = v.w; }
#pragma unroll
                for (int u = 0; u < CH; ++u)
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        const int e = 3 * u + k;
                        q[u][k] = sizeof(CT) == 4 ? w[e] : ((w[e >> 1] >> (16 * (e & 1))) & 0xFFFFu);
                    }
            } else {
#pragma unroll
                for (int u = 0; u < CH; ++u) {
                    q[u][0] = q[u][1] = q[u][2] = 0;
                    if (a0 + u < b) taxon_load_tuple<CT>(row + 3 * (size_t)(a0 + u), q[u][0], q[u][1], q[u][2]);
                }
            }
            ACC cX = 0, cW = 0, cZ = 0;                     // the lane's chunk
            uint32_t cF = 0;                                // resolved | outvoted << 8 | uninformed << 16 (<= 16 each)
#pragma unroll
            for (int u = 0; u < CH; ++u) {
                const uint32_t a = a0 + u;
                if (a < b) {                                // uniform
                    if (a == end) {                         // uniform: lca(a,b) changes here
                        const uint32_t d01 = __builtin_amdgcn_readfirstlane(lrow[a]) >> 16;
                        end = __builtin_amdgcn_readfirstlane((uint32_t)nrow[a]);
                        const uint32_t mx = max(d01, d23);
                        first = d12 < mx;                   // ab|cd
                        res = live && d12 != mx;            // else ad|bc
                        any_open = __any(live && !res) != 0;
                    }
                    const uint32_t n0 = q[u][0], n1 = q[u][1], n2 = q[u][2];
                    const ACC s = (ACC)n0 + n1 + n2;
                    const uint32_t q1 = first ? n0 : n2, alt = max(n1, first ? n2 : n0);
                    const ACC X = res ? (ACC)q1 : (ACC)0, W = res ? s : (ACC)0, Z = live ? s : (ACC)0;
                    const uint32_t F = res ? (1u | (alt > q1 ? 0x100u : 0u) | (s == 0 ? 0x10000u : 0u)) : 0u;
                    cX += X; cW += W; cZ += Z; cF += F;
                    // taxon a: the step's sums over the wave, then six words to a's cells
                    const unsigned long long tX = wave_sum(X), tW = wave_sum(W), tZ = any_open ? (unsigned long long)wave_sum(Z) : tW;
                    const uint32_t tF = wave_sum(F);
                    if (lane < (uint32_t)kTaxonFields) {
                        const unsigned long long v = lane == 0 ? (tF & 0xFFu) : lane == 1 ? tX : lane == 2 ? tW - tX
                                                     : lane == 3 ? tZ - tW : lane == 4 ? ((tF >> 8) & 0xFFu) : (tF >> 16);
                        if (v) atomicAdd(&acc[a * kTaxonFields + lane], v);
                    }
                }
            }
            LX += cX; LW += cW; LZ += cZ;
            LR += cF & 0xFFu; LO += (cF >> 8) & 0xFFu; LU += cF >> 16;
        }
        // the row's sums belong to b, c and d alike
        const unsigned long long v[kTaxonFields] = {LR, LX, LW - LX, LZ - LW, LO, LU};
#pragma unroll
        for (int k = 0; k < kTaxonFields; ++k) {
            if (live && v[k]) { atomicAdd(&acc[c * kTaxonFields + k], v[k]); atomicAdd(&acc[d * kTaxonFields + k], v[k]); }
            const unsigned long long t = wave_sum(live ? v[k] : 0ull);
            if (lane == 0 && t) atomicAdd(&acc[b * kTaxonFields + k], t);
        }
    }
    __syncthreads();
    for (uint32_t i = tid; i < cells; i += kThreads) {
        const unsigned long long v = acc[i];
        if (v) atomicAdd(&dst[i], v);
    }
}

size_t taxon_lds_bytes(uint32_t n) { return (size_t)n * kTaxonFields * 8; }

template <typename CT, typename ACC>
static hipError_t launch_taxon_t(hipStream_t s, const ScoreDevice &sd, int n_cu, unsigned long long *dst) {
    if (sd.n_rounds == 0) return hipSuccess;
    // one workgroup per CU, as in the score passes (more row streams per CU lose their cache lines in the L1 between two
    // accesses, qs_score.hip): the LDS request is raised to more than half a CU's LDS where the accumulators need less
    const size_t lds = std::max<size_t>(taxon_lds_bytes(sd.n), 81u * 1024u);
    if (lds > 160u * 1024u) return hipErrorInvalidValue;
    auto k = taxon_bundle_kernel<CT, ACC, kTaxonWaves>;
    hipError_t e = hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    dim3 block(kTaxonWaves * kWave), grid(std::min<uint32_t>(sd.n_rounds, (uint32_t)std::max(1, n_cu)));
    hipLaunchKernelGGL(k, grid, block, lds, s, sd, dst);
    return hipGetLastError();
}

// dst (6 x n words, zeroed by the caller) += the sums of the whole rows of sd's rank range (sd.bundle_* = plan_bundles with
// kTaxonWaves waves). A context's table starts and ends at a row start (shards are cut by the largest id), so there are no
// partial rows to add; the caller refuses a range that has some.
hipError_t launch_taxon_support(hipStream_t s, const ScoreDevice &sd, bool wide, int n_cu, unsigned long long *dst) {
    if (sd.count_bits == 16) return launch_taxon_t<uint16_t, uint32_t>(s, sd, n_cu, dst);   // 64 x 3 x 65535 < 2^32
    return wide ? launch_taxon_t<uint32_t, unsigned long long>(s, sd, n_cu, dst) : launch_taxon_t<uint32_t, uint32_t>(s, sd, n_cu, dst);
}

} // namespace qs
