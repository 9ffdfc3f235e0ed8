// qs_collapse.hip -- the count table of SPECIES summed out of a table counted over their individuals, on gfx950.
//
// The topology a tree displays for four individuals does not depend on its other leaves, so the species-level count of a 4-set of
// species S0 < S1 < S2 < S3 is the sum of the individual-level tuples over every choice of one individual per species (the
// multi-individual quartet score of Rabiee, Sayyari & Mirarab 2019). Species i owns the consecutive source ids
// [first[i], first[i + 1]), so a < b < c < d holds for every choice and the slots carry over unchanged: no min/max network, no
// slot_of_pairing. Source tuples with two individuals of one species belong to no destination and are never read. The reference has
// no such step (its TaxonMapper is dead code).
//
// Work unit = one destination row (S1, S2, S3), S1 >= 1, owned by ONE wave: its tuples S0 = 0 .. S1 - 1 are consecutive ranks, and
// in every source row (b, c, d) of S1 x S2 x S3 the tuples a = 0 .. first[S1] - 1 are consecutive too -- exactly the groups S0 < S1,
// one after another. A lane owns a source id a (chunks of 64 when the prefix is longer), adds up three 64-bit sums over the source
// rows (coalesced loads, every contributing tuple read once through load_tuple), then the sums are added up per species by a
// segmented scan over the lanes (shuffles; a species that crosses a chunk end is carried in a wave-uniform register) and the last
// lane of a species stores its tuple. No atomics, no LDS traffic besides the two id lists.
//   Short prefixes (first[S1] <= 32: the rows with small S1): the wave is cut into 64 / p2 lane groups (p2 = the power of two that
//   holds the prefix), group g takes the source rows g, g + G, ..; the groups' sums are added with xor-shuffles before the scan.
// A row's cost is first[S1] x |S1| x |S2| x |S3| loads by one wave: a few species of very many individuals each leave most of the
// device idle.
#include "qs_common.hpp"
#include "qs_internal.hpp"
#include "qs_tuple_io.hpp"

namespace qs {

constexpr int kCollapseWaves = 4;         // waves per workgroup
constexpr uint32_t kCollapseRows = 4;     // destination rows per wave (kCollapseWaves apart)
constexpr uint32_t kCollapseIdsMax = 4096;

__device__ __forceinline__ unsigned long long sat_add(unsigned long long x, unsigned long long y) {
    const unsigned long long s = x + y;
    return s < x ? ~0ull : s;   // (beyond 64 bits: beyond every cell width, the overflow flag goes up)
}

// row index -> x < y < z with binom3(z) + binom2(y) + x = r
__device__ __forceinline__ void unrank3(uint64_t r, uint32_t &x, uint32_t &y, uint32_t &z) {
    uint32_t c = (uint32_t)(cbrt(6.0 * (double)r + 1.0) + 1.0);
    while (binom3(c) > r) --c;
    while (binom3((uint64_t)c + 1) <= r) ++c;
    r -= binom3(c);
    unrank2((uint32_t)r, x, y);
    z = c;
}

// ids: first[0 .. n_dst] | species_of[0 .. n_src) from entry kCollapseIdsMax + 1 on
template <typename ST, typename DT>
__global__ __launch_bounds__(kCollapseWaves * kWave) void table_collapse_kernel(const ST *__restrict__ src, DT *__restrict__ dst,
                                                                                const uint16_t *__restrict__ ids, uint32_t n_dst, uint32_t n_src,
                                                                                uint64_t n_rows, uint32_t *__restrict__ overflow_flag) {
    __shared__ uint16_t first[kCollapseIdsMax + 1];
    __shared__ uint16_t sp_of[kCollapseIdsMax];
    for (uint32_t i = threadIdx.x; i <= n_dst; i += kCollapseWaves * kWave) first[i] = ids[i];
    for (uint32_t i = threadIdx.x; i < n_src; i += kCollapseWaves * kWave) sp_of[i] = ids[kCollapseIdsMax + 1 + i];
    __syncthreads();   // (the only one: from here on every wave is on its own)
    constexpr unsigned long long cell_max = sizeof(DT) == 2 ? 0xFFFFull : 0xFFFFFFFFull;
    const uint32_t lane = threadIdx.x % kWave;
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    const uint64_t row0 = (uint64_t)blockIdx.x * (kCollapseWaves * kCollapseRows) + w;
    for (uint32_t k = 0; k < kCollapseRows; ++k) {
        const uint64_t row = row0 + (uint64_t)k * kCollapseWaves;
        if (row >= n_rows) return;
        uint32_t S1, S2, S3;
        unrank3(row, S1, S2, S3);
        ++S1; ++S2; ++S3;   // (rows with S1 = 0 hold no tuple)
        const uint32_t pre = first[S1];
        const uint32_t b0 = pre, nb = first[S1 + 1] - b0, c0 = first[S2], nc = first[S2 + 1] - c0, d0 = first[S3], nd = first[S3 + 1] - d0;
        const uint64_t dbase = binom4(S3) + binom3(S2) + binom2(S1);
        uint32_t sh = 6;   // log2 of the lanes one source row takes
        if (pre <= 32) { sh = 0; while ((1u << sh) < pre) ++sh; }
        const uint32_t p2 = 1u << sh, G = kWave >> sh, g = lane >> sh, al = lane & (p2 - 1);
        unsigned long long carry0 = 0, carry1 = 0, carry2 = 0;   // the sums of a species that began in an earlier chunk
        for (uint32_t a0 = 0; a0 < pre; a0 += kWave) {           // (G > 1: one chunk)
            const uint32_t a = a0 + al;
            unsigned long long s0 = 0, s1 = 0, s2 = 0;
            if (a < pre) {
                uint32_t ib = g, ic = 0, id = 0;
                if (ib >= nb) { const uint32_t q = ib / nb; ib -= q * nb; ic = q; if (ic >= nc) { id = ic / nc; ic -= id * nc; } }
                uint64_t base = binom4(d0 + id) + binom3(c0 + ic) + a;   // (c, d) change only where b wraps
                while (id < nd) {
                    uint32_t v[3];
                    load_tuple(src, base + binom2(b0 + ib), v);
                    s0 += v[0]; s1 += v[1]; s2 += v[2];   // (fewer than 2^32 terms below 2^32 each)
                    ib += G;
                    if (ib >= nb) {
                        const uint32_t q = ib / nb;
                        ib -= q * nb; ic += q;
                        if (ic >= nc) { const uint32_t q2 = ic / nc; ic -= q2 * nc; id += q2; }
                        base = binom4(d0 + id) + binom3(c0 + ic) + a;   // (id = nd: past the table, and not loaded)
                    }
                }
            }
            for (uint32_t off = p2; off < (uint32_t)kWave; off <<= 1) {   // the lane groups' shares of one source id
                s0 += __shfl_xor(s0, (int)off, kWave); s1 += __shfl_xor(s1, (int)off, kWave); s2 += __shfl_xor(s2, (int)off, kWave);
            }
            // per species: an inclusive scan that does not reach below the species' first lane of this chunk
            const bool valid = g == 0 && a < pre;
            const uint32_t sp = valid ? sp_of[a] : 0;
            const uint32_t sp_lo = first[sp], sp_hi = first[sp + 1];
            const uint32_t lo = valid ? (sp_lo > a0 ? sp_lo - a0 : 0) : lane;
#pragma unroll
            for (uint32_t off = 1; off < (uint32_t)kWave; off <<= 1) {
                const unsigned long long t0 = __shfl_up(s0, off, kWave), t1 = __shfl_up(s1, off, kWave), t2 = __shfl_up(s2, off, kWave);
                if (lane >= lo + off) { s0 = sat_add(s0, t0); s1 = sat_add(s1, t1); s2 = sat_add(s2, t2); }
            }
            if (valid && sp_lo < a0) { s0 = sat_add(s0, carry0); s1 = sat_add(s1, carry1); s2 = sat_add(s2, carry2); }
            if (valid && a + 1 == sp_hi) {   // the species ends here (first[S1] is a species' end: the last chunk leaves nothing over)
                if (s0 > cell_max || s1 > cell_max || s2 > cell_max) *overflow_flag = 1;
                store_tuple(dst, dbase + sp, (uint32_t)s0, (uint32_t)s1, (uint32_t)s2);
            }
            // lane 63's species goes on in the next chunk: its sum so far (with what it brought along) is the carry
            const bool more = valid && lane == kWave - 1 && a + 1 < sp_hi;
            const bool any_more = __shfl((int)more, kWave - 1, kWave) != 0;
            carry0 = any_more ? __shfl(s0, kWave - 1, kWave) : 0;
            carry1 = any_more ? __shfl(s1, kWave - 1, kWave) : 0;
            carry2 = any_more ? __shfl(s2, kWave - 1, kWave) : 0;
        }
    }
}

hipError_t launch_table_collapse(hipStream_t s, const void *src, int src_bits, void *dst, int dst_bits, const uint16_t *ids_dev,
                                 uint32_t n_dst, uint32_t n_src, uint32_t *overflow_flag) {
    if (n_dst < 4) return hipSuccess;
    if (n_src > kCollapseIdsMax || n_dst > n_src) return hipErrorInvalidValue;
    const uint64_t n_rows = binom3(n_dst - 1);   // (S1, S2, S3) with 1 <= S1
    const uint64_t per_block = (uint64_t)kCollapseWaves * kCollapseRows;
    const uint64_t blocks = (n_rows + per_block - 1) / per_block;
    if (blocks >= (1ull << 31)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks), block(kCollapseWaves * kWave);
    if (src_bits == 32 && dst_bits == 32)
        hipLaunchKernelGGL((table_collapse_kernel<uint32_t, uint32_t>), grid, block, 0, s, (const uint32_t *)src, (uint32_t *)dst, ids_dev, n_dst, n_src, n_rows, overflow_flag);
    else if (src_bits == 16 && dst_bits == 16)
        hipLaunchKernelGGL((table_collapse_kernel<uint16_t, uint16_t>), grid, block, 0, s, (const uint16_t *)src, (uint16_t *)dst, ids_dev, n_dst, n_src, n_rows, overflow_flag);
    else if (src_bits == 16 && dst_bits == 32)
        hipLaunchKernelGGL((table_collapse_kernel<uint16_t, uint32_t>), grid, block, 0, s, (const uint16_t *)src, (uint32_t *)dst, ids_dev, n_dst, n_src, n_rows, overflow_flag);
    else
        return hipErrorInvalidValue;   // narrowing: refused by qs_table_collapse before it gets here
    return hipGetLastError();
}

} // namespace qs
