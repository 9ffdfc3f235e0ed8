// qs_tuple_io.hpp -- one count-table tuple (three cells) per lane: what the re-indexing kernels (qs_remap.hip,
// qs_restrict.hip) share. The source tuple is read with ONE load (dwordx3 for 32-bit cells, the two dwords around the
// 6 bytes for 16-bit cells): a read that leaves the source row is one scattered cache line per lane.
#pragma once
#include "qs_common.hpp"

namespace qs {

constexpr int kRemapThreads = 256;
constexpr uint32_t kRemapSteps = 32;   // destination ranks per lane (64 apart)

struct alignas(4) Cells3 { uint32_t x, y, z; };
struct alignas(4) Words2 { uint32_t x, y; };

__device__ __forceinline__ void load_tuple(const uint32_t *__restrict__ t, uint64_t r, uint32_t v[3]) {
    const Cells3 q = *reinterpret_cast<const Cells3 *>(t + 3 * r);
    v[0] = q.x; v[1] = q.y; v[2] = q.z;
}
// 6 bytes at 2-byte alignment: the two dwords that hold them. They end at most 2 bytes behind the tuple, which the
// table's allocation (16 bytes of padding) and an attached table (bytes rounded up to a multiple of 4) both cover.
__device__ __forceinline__ void load_tuple(const uint16_t *__restrict__ t, uint64_t r, uint32_t v[3]) {
    const uint64_t byte = 6 * r;
    const Words2 q = *reinterpret_cast<const Words2 *>(reinterpret_cast<const char *>(t) + (byte & ~3ull));
    const uint64_t w = ((uint64_t)q.y << 32 | q.x) >> ((byte & 2) * 8);
    v[0] = (uint32_t)w & 0xFFFFu; v[1] = (uint32_t)(w >> 16) & 0xFFFFu; v[2] = (uint32_t)(w >> 32) & 0xFFFFu;
}

__device__ __forceinline__ void store_tuple(uint32_t *__restrict__ t, uint64_t r, uint32_t a, uint32_t b, uint32_t c) {
    *reinterpret_cast<Cells3 *>(t + 3 * r) = Cells3{a, b, c};
}
__device__ __forceinline__ void store_tuple(uint16_t *__restrict__ t, uint64_t r, uint32_t a, uint32_t b, uint32_t c) {
    t[3 * r] = (uint16_t)a; t[3 * r + 1] = (uint16_t)b; t[3 * r + 2] = (uint16_t)c;
}

__device__ __forceinline__ uint32_t pick3(const uint32_t v[3], int k) { return k == 0 ? v[0] : k == 1 ? v[1] : v[2]; }

// the launch shape of both kernels: one workgroup per kRemapThreads * kRemapSteps destination ranks; false = more than 2^31 - 1 workgroups
inline bool reindex_grid(uint64_t n_tuples, dim3 &grid, dim3 &block) {
    const uint64_t per_block = (uint64_t)kRemapThreads * kRemapSteps;
    const uint64_t blocks = (n_tuples + per_block - 1) / per_block;
    if (blocks >= (1ull << 31)) return false;
    grid = dim3((unsigned)blocks); block = dim3(kRemapThreads);
    return true;
}

} // namespace qs
