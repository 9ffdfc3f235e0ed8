// qs_remap.hip -- re-index a count table into the lookup-id order of another reference tree on gfx950.
//
// The count table is a function of the taxon set; only its id order (the reference tree's depth-first leaf order,
// QuartetCounterLookup.hpp:252-258) depends on the reference tree. A second reference tree over the same taxa needs
// the table in ITS id order, because the score kernels rely on that order (qs_score.hip: for sorted ids only ab|cd and
// ad|bc can be the reference topology). The reference has no such step: it recounts per run.
//
// Destination-major: lane l of a wave owns the destination ranks r0 + l + 64 k, k < kRemapSteps, so that every step
// of the wave writes 64 consecutive tuples. The lane un-ranks its first rank once and steps 64 ranks at a time with
// decode_near. For destination ids t0 < t1 < t2 < t3 with source ids u_i = src_id_of[t_i]: the source tuple sits at
// rank4(sorted u), and destination slot k (t0 paired with t_{k+1}) is the source slot of the pairing
// {u0, u_{k+1}} | {the other two} (slot_of_pairing). src_id_of lives in LDS. The source tuple is read with ONE load
// (qs_tuple_io.hpp).
#include "qs_common.hpp"
#include "qs_internal.hpp"
#include "qs_tuple_io.hpp"

namespace qs {

template <typename ST, typename DT>
__global__ __launch_bounds__(kRemapThreads) void table_remap_kernel(const ST *__restrict__ src, DT *__restrict__ dst,
                                                                    const uint16_t *__restrict__ src_id_of, uint32_t n,
                                                                    uint64_t n_tuples) {
    __shared__ uint16_t sid[4096];
    for (uint32_t i = threadIdx.x; i < n; i += kRemapThreads) sid[i] = src_id_of[i];
    __syncthreads();
    const uint32_t lane = threadIdx.x % kWave;
    const uint64_t wave = (uint64_t)blockIdx.x * (kRemapThreads / kWave) + threadIdx.x / kWave;
    uint64_t r = wave * (kWave * kRemapSteps) + lane;
    if (r >= n_tuples) return;
    Ids4 t;
    unrank4(r, t.a, t.b, t.c, t.d);
    for (uint32_t k = 0;;) {
        const uint32_t u0 = sid[t.a], u1 = sid[t.b], u2 = sid[t.c], u3 = sid[t.d];
        const uint32_t lo01 = min(u0, u1), hi01 = max(u0, u1), lo23 = min(u2, u3), hi23 = max(u2, u3);
        const uint32_t m1 = max(lo01, lo23), m2 = min(hi01, hi23);
        uint32_t v[3];
        load_tuple(src, rank4(min(lo01, lo23), min(m1, m2), max(m1, m2), max(hi01, hi23)), v);
        store_tuple(dst, r, pick3(v, slot_of_pairing(u0, u1, u2, u3)), pick3(v, slot_of_pairing(u0, u2, u1, u3)),
                    pick3(v, slot_of_pairing(u0, u3, u1, u2)));
        if (++k == kRemapSteps) break;
        r += kWave;
        if (r >= n_tuples) break;
        t = decode_near(t, kWave);
    }
}

hipError_t launch_table_remap(hipStream_t s, const void *src, int src_bits, void *dst, int dst_bits, const uint16_t *src_id_of_dev,
                              uint32_t n, uint64_t n_tuples) {
    if (n_tuples == 0) return hipSuccess;
    if (n > 4096) return hipErrorInvalidValue;
    dim3 grid, block;
    if (!reindex_grid(n_tuples, grid, block)) return hipErrorInvalidValue;
    if (src_bits == 32 && dst_bits == 32)
        hipLaunchKernelGGL((table_remap_kernel<uint32_t, uint32_t>), grid, block, 0, s, (const uint32_t *)src, (uint32_t *)dst, src_id_of_dev, n, n_tuples);
    else if (src_bits == 16 && dst_bits == 16)
        hipLaunchKernelGGL((table_remap_kernel<uint16_t, uint16_t>), grid, block, 0, s, (const uint16_t *)src, (uint16_t *)dst, src_id_of_dev, n, n_tuples);
    else if (src_bits == 16 && dst_bits == 32)
        hipLaunchKernelGGL((table_remap_kernel<uint16_t, uint32_t>), grid, block, 0, s, (const uint16_t *)src, (uint32_t *)dst, src_id_of_dev, n, n_tuples);
    else
        return hipErrorInvalidValue;   // narrowing: refused by qs_table_remap before it gets here
    return hipGetLastError();
}

} // namespace qs
