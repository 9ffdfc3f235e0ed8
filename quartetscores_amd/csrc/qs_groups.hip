// qs_groups.hip -- quartet support of user-defined taxon groups from the count table on gfx950 (qs_group_support).
//
// Replaces nothing in the reference; the nearest is the metaquartet sum of processNodePair (QuartetScoreComputer.hpp:379-472), which
// sums (q1, q2, q3) over S1 x S2 x S3 x S4 for the four subtrees beside a node pair of the reference tree. Here the four sets are any
// disjoint taxon sets (a quad hypothesis), or two sets with two taxa taken from each (a split hypothesis); DESIGN.md 14.
//
// Shape: qs_taxon.hip's. A wave takes 64 table rows with the same b -- 64 consecutive pairs (c,d) -- and walks them in lockstep along
// a; a lane streams its own row in 96-byte chunks requested as 16-byte loads back to back. For one hypothesis the labels of b (wave-
// uniform) and of c, d (lane constants) leave ONE label a may carry for the 4-set to count, or none:
//   quad:  b, c, d carry three different labels of 1..4, a needs the fourth;
//   split: b, c, d carry labels 1 and 2, a needs the one that occurs once among them (two taxa of either label).
// They also fix which of the tuple's cells (n0, n1, n2) = (ab|cd, ac|bd, ad|bc) is q1, q2 and q3: a's partner in q1 is the taxon of
// the other label of its side (quad) or the other taxon of its own label (split); a is the smallest id, so in a split it is g1 or h1
// and its partner in q2 is the smaller, in q3 the larger id of the other label. Per step only a compare of the wave-uniform label of a
// against the lane's needed label is left; the three sums and the three "this cell is below the tuple's maximum" counts stay
// unpermuted in the lane and are permuted once at the row's end.
// One read of the table serves kGroupHyp hypotheses: their labels of a taxon are the nibbles of one word. A wave skips a row in which
// no lane needs anything, and a chunk whose a all carry label 0 in every hypothesis of the pass.
// The sums of a workgroup are [hypothesis][word][lane] in LDS and go to memory with one 64-bit atomic per non-zero word when the
// workgroup ends: integer sums, independent of order and grid.
// Three instances. 32-bit cells, CHUNKED: 32-bit sums per chunk, widened once per chunk (the host asks 64 x 3 x largest count < 2^32,
// the taxon kernel's rule; 8 x largest count < 2^32 is what is needed here); 32-bit cells, any counts: 64-bit sums throughout;
// 16-bit cells: a row has fewer than 65535 steps of at most 65535 each, so its sums are 32-bit words and need no chunk sums.
#include "qs_common.hpp"
#include "qs_internal.hpp"

#include <algorithm>
#include <type_traits>

namespace qs {

typedef uint32_t qg_u32x4 __attribute__((ext_vector_type(4)));
typedef qg_u32x4 qg_u32x4_a2 __attribute__((aligned(2)));   // rows start at any tuple

constexpr uint32_t kNoNeed = 0xFu;   // a label no taxon carries

// The label a must carry (kNoNeed: the row counts for nothing) and the cells of q1, q2 in bits 4..5 and 6..7, from the labels of b, c, d
__device__ __forceinline__ uint32_t group_need(uint32_t lb, uint32_t lc, uint32_t ld, bool split) {
    if (lb == 0 || lc == 0 || ld == 0) return kNoNeed;
    auto pos = [&](uint32_t label) { return lb == label ? 0u : lc == label ? 1u : 2u; };
    if (split) {
        if (lb == lc && lc == ld) return kNoNeed;
        const uint32_t ones = (lb == 1) + (lc == 1) + (ld == 1);
        const uint32_t need = ones == 1 ? 1u : 2u;
        const uint32_t i1 = pos(need);
        const uint32_t i2 = i1 == 0 ? 1u : 0u;   // the smaller id of the other label; q3 gets the remaining cell
        return need | i1 << 4 | i2 << 6;
    }
    if (lb == lc || lb == ld || lc == ld) return kNoNeed;
    const uint32_t need = 10u - lb - lc - ld;
    return need | pos(((need - 1) ^ 1u) + 1) << 4 | pos(((need - 1) ^ 2u) + 1) << 6;
}

template <typename CT, typename LT, bool CHUNKED, int WAVES>
__global__ __launch_bounds__(WAVES * kWave) void group_bundle_kernel(ScoreDevice sd, const uint32_t *__restrict__ labw, uint32_t split_mask,
                                                                     uint32_t n_hyp, unsigned long long *__restrict__ dst) {
    extern __shared__ __align__(16) unsigned char group_smem[];
    unsigned long long *acc = reinterpret_cast<unsigned long long *>(group_smem);   // [hypothesis][word][lane]
    constexpr int kThreads = WAVES * kWave, HG = kGroupHyp;
    constexpr uint32_t kCells = HG * kGroupWords * kWave;
    const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const uint32_t n = sd.n;
    for (uint32_t i = tid; i < kCells; i += kThreads) acc[i] = 0;
    __syncthreads();
    const CT *table = reinterpret_cast<const CT *>(sd.table);
    constexpr int CH = sizeof(CT) == 2 ? 16 : 8;            // tuples a lane requests at once: 96 bytes of its row
    constexpr int NV = CH * 3 * (int)sizeof(CT) / 16;       // as 16-byte loads
    for (uint32_t round = blockIdx.x; round < sd.n_rounds; round += gridDim.x) {
        const uint32_t rk = sd.bundle_rounds[2 * round], rg = sd.bundle_rounds[2 * round + 1];
        const uint32_t b = __builtin_amdgcn_readfirstlane(rk * WAVES + wave);
        const uint32_t pcnt = b < n ? sd.bundle_pcnt[b] : 0u;
        if (pcnt <= rg * kWave) continue;                                         // uniform over the wave
        const bool live = rg * kWave + lane < pcnt;
        const uint32_t p = sd.bundle_plo[b] + min(rg * kWave + lane, pcnt - 1);   // (idle lanes repeat the last row and need nothing)
        uint32_t c, d;
        unrank2(p, c, d);
        c += b + 1; d += b + 1;
        const CT *row = table + (rank4(0, b, c, d) - sd.rank_lo) * 3;
        const uint32_t wb = __builtin_amdgcn_readfirstlane(labw[b]), wc = labw[c], wd = labw[d];
        auto info_of = [&](int h) { return group_need((wb >> (4 * h)) & 0xFu, (wc >> (4 * h)) & 0xFu, (wd >> (4 * h)) & 0xFu, (split_mask >> h) & 1u); };
        uint32_t need[HG];
        bool any = false;
#pragma unroll
        for (int h = 0; h < HG; ++h) {
            need[h] = live ? info_of(h) & 0xFu : kNoNeed;
            any |= need[h] != kNoNeed;
        }
        if (!__any(any)) continue;                          // uniform: no lane of the wave needs anything of this row
        LT L[HG][3];                                        // the lane's row: sums of n0, n1, n2 over the 4-sets that count
        uint32_t FA[HG], FB[HG], FU[HG];                    // ... their number | those with n0 below the maximum << 16; the same for n1 | n2; all zero
#pragma unroll
        for (int h = 0; h < HG; ++h) { L[h][0] = L[h][1] = L[h][2] = 0; FA[h] = FB[h] = FU[h] = 0; }
        for (uint32_t a0 = 0; a0 < b; a0 += CH) {           // uniform
            uint32_t wa[CH], wany = 0;                      // uniform: the labels of the chunk's a (0 past the row's end: no lane needs label 0)
#pragma unroll
            for (int u = 0; u < CH; ++u) { wa[u] = a0 + u < b ? __builtin_amdgcn_readfirstlane(labw[a0 + u]) : 0u; wany |= wa[u]; }
            if (wany == 0) continue;                        // no a of the chunk takes part in a hypothesis of the pass: its tuples are not read
            uint32_t q[CH][3];
            if (a0 + CH <= b) {                             // the whole chunk lies in the row
                uint32_t w[NV * 4];
                const qg_u32x4_a2 *src = reinterpret_cast<const qg_u32x4_a2 *>(row + 3 * (size_t)a0);
#pragma unroll
                for (int j = 0; j < NV; ++j) { const qg_u32x4 v = src[j]; w[4 * j] = v.x; w[4 * j + 1] = v.y; w[4 * j + 2] = v.z; w[4 * j + 3] = v.w; }
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
                    if (a0 + u < b) { const CT *t = row + 3 * (size_t)(a0 + u); q[u][0] = t[0]; q[u][1] = t[1]; q[u][2] = t[2]; }
                }
            }
            uint32_t cs[CHUNKED ? HG : 1][3];               // the lane's chunk (not CHUNKED: the row's sums take every tuple)
            uint32_t cF[HG];                                // five 6-bit counts (<= 16 each): counted, n0 / n1 / n2 below the maximum, all zero
#pragma unroll
            for (int h = 0; h < HG; ++h) { cF[h] = 0; if (CHUNKED) cs[h][0] = cs[h][1] = cs[h][2] = 0; }
#pragma unroll
            for (int u = 0; u < CH; ++u) {
                const uint32_t n0 = q[u][0], n1 = q[u][1], n2 = q[u][2];
                const uint32_t mx = max(n0, max(n1, n2));
                const uint32_t G = 1u | (mx > n0 ? 1u << 6 : 0u) | (mx > n1 ? 1u << 12 : 0u) | (mx > n2 ? 1u << 18 : 0u) | ((n0 | n1 | n2) == 0 ? 1u << 24 : 0u);
#pragma unroll
                for (int h = 0; h < HG; ++h)
                    if (need[h] == ((wa[u] >> (4 * h)) & 0xFu)) {
                        if (CHUNKED) { cs[h][0] += n0; cs[h][1] += n1; cs[h][2] += n2; } else { L[h][0] += n0; L[h][1] += n1; L[h][2] += n2; }
                        cF[h] += G;
                    }
            }
#pragma unroll
            for (int h = 0; h < HG; ++h) {
                if (CHUNKED) { L[h][0] += cs[h][0]; L[h][1] += cs[h][1]; L[h][2] += cs[h][2]; }
                FA[h] += (cF[h] & 0x3Fu) | ((cF[h] >> 6) & 0x3Fu) << 16;      // (a row has fewer than 65535 steps)
                FB[h] += ((cF[h] >> 12) & 0x3Fu) | ((cF[h] >> 18) & 0x3Fu) << 16;
                FU[h] += cF[h] >> 24;
            }
        }
        // the row's sums in the hypothesis' order of the cells
#pragma unroll
        for (int h = 0; h < HG; ++h) {
            const uint32_t cnt = FA[h] & 0xFFFFu;
            if (cnt == 0) continue;
            const uint32_t info = info_of(h), i1 = (info >> 4) & 3u, i2 = (info >> 6) & 3u, i3 = 3u - i1 - i2;
            auto cell = [&](uint32_t i) -> unsigned long long { return i == 0 ? L[h][0] : i == 1 ? L[h][1] : L[h][2]; };
            const uint32_t below = i1 == 0 ? FA[h] >> 16 : i1 == 1 ? FB[h] & 0xFFFFu : FB[h] >> 16;   // max(q2,q3) > q1
            const unsigned long long v[kGroupWords] = {cnt, cell(i1), cell(i2), cell(i3), below, FU[h]};
#pragma unroll
            for (int k = 0; k < kGroupWords; ++k)
                if (v[k]) atomicAdd(&acc[(h * kGroupWords + k) * kWave + lane], v[k]);
        }
    }
    __syncthreads();
    if (tid < n_hyp * kGroupWords) {
        unsigned long long t = 0;
        for (int l = 0; l < kWave; ++l) t += acc[tid * kWave + ((l + tid) & (kWave - 1))];
        if (t) atomicAdd(&dst[tid], t);
    }
}

template <typename CT, typename LT, bool CHUNKED>
static hipError_t launch_group_t(hipStream_t s, const ScoreDevice &sd, const uint32_t *labw, uint32_t split_mask, uint32_t n_hyp, int n_cu,
                                 unsigned long long *dst) {
    if (sd.n_rounds == 0) return hipSuccess;
    // one workgroup per CU, as in the taxon pass: the LDS request is raised to more than half a CU's LDS
    const size_t lds = std::max<size_t>((size_t)kGroupHyp * kGroupWords * kWave * 8, 81u * 1024u);
    auto k = group_bundle_kernel<CT, LT, CHUNKED, kTaxonWaves>;
    hipError_t e = hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    dim3 block(kTaxonWaves * kWave), grid(std::min<uint32_t>(sd.n_rounds, (uint32_t)std::max(1, n_cu)));
    hipLaunchKernelGGL(k, grid, block, lds, s, sd, labw, split_mask, n_hyp, dst);
    return hipGetLastError();
}

// dst (6 x n_hyp words, zeroed by the caller) += the sums of up to kGroupHyp hypotheses over the whole rows of sd's rank range
// (sd.bundle_* = plan_bundles with kTaxonWaves waves; of sd only n, rank_lo, table, count_bits and the bundle plan are read).
// labw[t] = the labels of taxon t, hypothesis h in bits 4h .. 4h+3; split_mask bit h = hypothesis h is a split.
hipError_t launch_group_support(hipStream_t s, const ScoreDevice &sd, const uint32_t *labw, uint32_t split_mask, uint32_t n_hyp, bool wide,
                                int n_cu, unsigned long long *dst) {
    if (n_hyp == 0 || n_hyp > (uint32_t)kGroupHyp) return hipErrorInvalidValue;
    if (sd.count_bits == 16) return launch_group_t<uint16_t, uint32_t, false>(s, sd, labw, split_mask, n_hyp, n_cu, dst);
    return wide ? launch_group_t<uint32_t, unsigned long long, false>(s, sd, labw, split_mask, n_hyp, n_cu, dst)
                : launch_group_t<uint32_t, unsigned long long, true>(s, sd, labw, split_mask, n_hyp, n_cu, dst);
}

} // namespace qs
