// qs_wave_sum.hpp -- sums over the 64 lanes of a wave, the same value in every lane's copy (wave-uniform).
#pragma once
#include "qs_common.hpp"

namespace qs {

// 32-bit (wraps like any 32-bit sum): DPP adds inside the rows of 16, the four row totals read into scalar registers
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, true);    // quad_perm [1,0,3,2]
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, true);    // quad_perm [2,3,0,1]
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, true);   // row_half_mirror
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, true);   // row_mirror
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 0) + (uint32_t)__builtin_amdgcn_readlane((int)v, 16) +
           (uint32_t)__builtin_amdgcn_readlane((int)v, 32) + (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
}
// 64-bit: shuffles
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
    return v;
}
// the exact 64-bit sum of 32-bit lane values: two halves of 16 bits (64 x 65535 stays in a word), each by the 32-bit form
__device__ __forceinline__ unsigned long long wave_sum_exact(uint32_t v) {
    return (unsigned long long)wave_sum(v & 0xFFFFu) + ((unsigned long long)wave_sum(v >> 16) << 16);
}
__device__ __forceinline__ unsigned long long wave_sum_exact(unsigned long long v) { return wave_sum(v); }

} // namespace qs
