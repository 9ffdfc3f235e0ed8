// qs_restrict.hip -- the count table of a SUBSET of the taxa, cut out of a counted table on gfx950.
//
// The topology a tree displays for a 4-set does not depend on the tree's other taxa, so the count table of the problem
// without some taxa is the sub-table of the counted one over the kept taxa: destination ids t0 < t1 < t2 < t3 (the kept
// taxa, renumbered in the pruned reference tree's depth-first leaf order) take the source tuple at
// rank4(sorted src_id_of[t_k]). The reference has no such step: it rejects a leaf it does not know and recounts per run.
//
// Destination-major like qs_remap.hip: lane l of a wave owns the destination ranks r0 + l + 64 k, k < kRemapSteps, every
// step of the wave stores 64 consecutive tuples; the lane un-ranks its first rank once and steps with decode_near;
// src_id_of (n_dst entries) lives in LDS; the source tuple is ONE load per lane (qs_tuple_io.hpp); no atomics.
//   Monotone = true   src_id_of is strictly increasing (pruning keeps the leaf order): the source ids are sorted as they
//                     come and the slots are the identity -- no min/max network, no slot_of_pairing. Along a destination
//                     row (t1, t2, t3) the lanes read src a = K[t0] inside ONE source row (K[t1], K[t2], K[t3]): ascending
//                     addresses with gaps where a dropped id lies.
//   Monotone = false  any injective map (restrict and re-order in one pass); with n_dst = n_src it is qs_remap.hip's kernel.
#include "qs_common.hpp"
#include "qs_internal.hpp"
#include "qs_tuple_io.hpp"

namespace qs {

template <bool Monotone, typename ST, typename DT>
__global__ __launch_bounds__(kRemapThreads) void table_restrict_kernel(const ST *__restrict__ src, DT *__restrict__ dst,
                                                                       const uint16_t *__restrict__ src_id_of, uint32_t n_dst,
                                                                       uint64_t n_tuples) {
    __shared__ uint16_t sid[4096];
    for (uint32_t i = threadIdx.x; i < n_dst; i += kRemapThreads) sid[i] = src_id_of[i];
    __syncthreads();
    const uint32_t lane = threadIdx.x % kWave;
    const uint64_t wave = (uint64_t)blockIdx.x * (kRemapThreads / kWave) + threadIdx.x / kWave;
    uint64_t r = wave * (kWave * kRemapSteps) + lane;
    if (r >= n_tuples) return;
    Ids4 t;
    unrank4(r, t.a, t.b, t.c, t.d);
    for (uint32_t k = 0;;) {
        const uint32_t u0 = sid[t.a], u1 = sid[t.b], u2 = sid[t.c], u3 = sid[t.d];
        uint32_t v[3];
        if constexpr (Monotone) {
            load_tuple(src, rank4(u0, u1, u2, u3), v);
            store_tuple(dst, r, v[0], v[1], v[2]);
        } else {
            const uint32_t lo01 = min(u0, u1), hi01 = max(u0, u1), lo23 = min(u2, u3), hi23 = max(u2, u3);
            const uint32_t m1 = max(lo01, lo23), m2 = min(hi01, hi23);
            load_tuple(src, rank4(min(lo01, lo23), min(m1, m2), max(m1, m2), max(hi01, hi23)), v);
            store_tuple(dst, r, pick3(v, slot_of_pairing(u0, u1, u2, u3)), pick3(v, slot_of_pairing(u0, u2, u1, u3)),
                        pick3(v, slot_of_pairing(u0, u3, u1, u2)));
        }
        if (++k == kRemapSteps) break;
        r += kWave;
        if (r >= n_tuples) break;
        t = decode_near(t, kWave);
    }
}

template <bool Monotone>
static hipError_t launch_restrict(hipStream_t s, const void *src, int src_bits, void *dst, int dst_bits, const uint16_t *ids,
                                  uint32_t n_dst, uint64_t n_tuples) {
    dim3 grid, block;
    if (!reindex_grid(n_tuples, grid, block)) return hipErrorInvalidValue;
    if (src_bits == 32 && dst_bits == 32)
        hipLaunchKernelGGL((table_restrict_kernel<Monotone, uint32_t, uint32_t>), grid, block, 0, s, (const uint32_t *)src, (uint32_t *)dst, ids, n_dst, n_tuples);
    else if (src_bits == 16 && dst_bits == 16)
        hipLaunchKernelGGL((table_restrict_kernel<Monotone, uint16_t, uint16_t>), grid, block, 0, s, (const uint16_t *)src, (uint16_t *)dst, ids, n_dst, n_tuples);
    else if (src_bits == 16 && dst_bits == 32)
        hipLaunchKernelGGL((table_restrict_kernel<Monotone, uint16_t, uint32_t>), grid, block, 0, s, (const uint16_t *)src, (uint32_t *)dst, ids, n_dst, n_tuples);
    else
        return hipErrorInvalidValue;   // narrowing: refused by qs_table_restrict before it gets here
    return hipGetLastError();
}

hipError_t launch_table_restrict(hipStream_t s, const void *src, int src_bits, void *dst, int dst_bits, const uint16_t *src_id_of_dev,
                                 uint32_t n_dst, uint64_t n_tuples, bool monotone) {
    if (n_tuples == 0) return hipSuccess;
    if (n_dst > 4096) return hipErrorInvalidValue;
    return monotone ? launch_restrict<true>(s, src, src_bits, dst, dst_bits, src_id_of_dev, n_dst, n_tuples)
                    : launch_restrict<false>(s, src, src_bits, dst, dst_bits, src_id_of_dev, n_dst, n_tuples);
}

} // namespace qs
