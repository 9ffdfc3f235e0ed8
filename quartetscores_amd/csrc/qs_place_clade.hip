// qs_place_clade.hip -- quartet placement of clades on the reference tree from the count table on gfx950 (qs_clade_placement).
//
// Replaces nothing in the reference: it never asks where the evaluation trees would put a subtree.
//
// The clade below a listed node holds the lookup ids [lo, hi). Of the 4-sets only those with exactly one taxon x of the clade
// depend on where the clade is regrafted; with p < q < r outside the clade their three counts n(xp|qr), n(xq|pr),
// n(xr|pq) go to the links of the median node of p, q, r that lead towards p, q and r, exactly as for one taxon (qs_place.hip).
// The median, its links and the cell order depend on (p, q, r) and on where the INTERVAL stands among them, not on x: the
// kernel sums the tuples of a triple over x first and accounts for the triple once.
//
// Shape: qs_place.hip's. A wave owns the middle id q, its lanes 64 consecutive largest ids r > q (both outside the clade: the
// walks are numbered in the n - |C| outside ids and mapped over the interval), and walks p over [0, min(q, lo)) and then over
// [hi, q): the walk jumps the interval.
//   first stretch (p < lo)   per x one table row, consecutive in p, as in qs_place.hip:
//       r < lo        (p,q,r,x)  rank C(x,4) + C(r,3) + C(q,2) + p   cells (r, q, p)
//       q < lo, hi<=r (p,q,x,r)  rank C(r,4) + C(x,3) + C(q,2) + p   cells (r, p, q)
//       hi <= q       (p,x,q,r)  rank C(r,4) + C(q,3) + C(x,2) + p   cells (p, r, q)
//     a chunk of 8 / 16 steps is requested as 96 bytes of 16-byte loads from the row of every x and summed over x in registers;
//   second stretch (hi <= p) (x,p,q,r)  rank C(r,4) + C(q,3) + C(p,2) + x   cells (p, q, r): consecutive in x, the clade's tuples
//     are one contiguous piece of a table row, streamed in the same 96-byte chunks (what is left over: tuple by tuple), four
//     steps of p requested together.
// Then one accounting per step, qs_place.hip's: run sums with wave-uniform targets (reduced over the wave at the run's end),
// lane-constant targets summed over the whole walk. A run of place_next may span the interval (a child of lca(p,q) can hold
// p, the clade and p' together): at p = hi the run is always closed and its state read again.
// A large clade is cut into x-slices [xa, xb) so that one clade alone still fills the device; an item = (walk, x-slice). The
// workgroups are listed by the host (clade, first item, stride): a workgroup stays with one clade, its 2N 64-bit LDS words
// are flushed once with one 64-bit atomic per non-zero cell. Integer sums: independent of order, grid and slicing.
// 32-bit register sums hold at most (n - |C| - 2 steps) x (slice length) tuples: the host (qs_clade_placement) keeps
// (n - |C|) x slice x (largest count) < 2^32 by shortening the slices, and picks the instance with 64-bit sums otherwise.
#include "qs_common.hpp"
#include "qs_internal.hpp"

#include <algorithm>

namespace qs {

typedef uint32_t qc_u32x4 __attribute__((ext_vector_type(4)));
typedef qc_u32x4 qc_u32x4_a2 __attribute__((aligned(2)));   // rows and pieces start at any tuple

__device__ __forceinline__ unsigned long long clade_wave_sum(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
    return v;
}

// sums[k] += the cells k of the CH tuples that start at src (96 bytes)
template <typename CT, typename ACC, int CH>
__device__ __forceinline__ void clade_add_chunk(const CT *src, ACC (&sums)[CH][3]) {
    constexpr int NV = CH * 3 * (int)sizeof(CT) / 16;
    const qc_u32x4_a2 *v = reinterpret_cast<const qc_u32x4_a2 *>(src);
    uint32_t w[NV * 4];
#pragma unroll
    for (int j = 0; j < NV; ++j) { const qc_u32x4 x = v[j]; w[4 * j] = x.x; w[4 * j + 1] = x.y; w[4 * j + 2] = x.z; w[4 * j + 3] = x.w; }
#pragma unroll
    for (int u = 0; u < CH; ++u)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int e = 3 * u + k;
            sums[u][k] += (ACC)(sizeof(CT) == 4 ? w[e] : ((w[e >> 1] >> (16 * (e & 1))) & 0xFFFFu));
        }
}

template <typename CT, typename ACC>
__global__ __launch_bounds__(kPlaceWaves * kWave) void place_clade_kernel(CladeDevice cd, unsigned long long *__restrict__ dst) {
    extern __shared__ __align__(16) unsigned char clade_smem[];
    unsigned long long *acc = reinterpret_cast<unsigned long long *>(clade_smem);   // [link]
    constexpr int kThreads = kPlaceWaves * kWave;
    constexpr int CH = sizeof(CT) == 2 ? 16 : 8;            // tuples a lane requests at once: 96 bytes
    constexpr int PU = 4;                                   // steps of the second stretch requested together
    const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const uint32_t n = cd.n, N = cd.n_nodes, cells = 2 * N;
    const uint32_t ci = cd.groups[2 * blockIdx.x], ks = cd.groups[2 * blockIdx.x + 1];
    const uint32_t first = ks & 0xFFFFu, share = ks >> 16;
    const uint32_t lo = cd.clades[4 * ci], hi = cd.clades[4 * ci + 1], xs = cd.clades[4 * ci + 2], n_tasks = cd.clades[4 * ci + 3];
    const uint32_t s = hi - lo, no = n - s, nsl = (s + xs - 1) / xs, n_items = n_tasks * nsl;
    for (uint32_t i = tid; i < cells; i += kThreads) acc[i] = 0;
    __syncthreads();
    const CT *table = reinterpret_cast<const CT *>(cd.table);
    const uint32_t *__restrict__ L = cd.ref_lca;
    for (uint32_t item = first * kPlaceWaves + wave; item < n_items; item += share * kPlaceWaves) {   // uniform over the wave
        const uint32_t task = item / nsl, sl = item - task * nsl;
        const uint32_t xa = lo + sl * xs, xb = min(hi, xa + xs), cnt = xb - xa;
        const uint32_t tk = __builtin_amdgcn_readfirstlane(cd.tasks[task]);
        const uint32_t qo = no - 1 - (tk & 0xFFFFu), rg = tk >> 16;          // in the numbering of the outside ids
        const uint32_t q = qo < lo ? qo : qo + s;
        const uint32_t ro_raw = qo + 1 + rg * kWave + lane;
        const bool live = ro_raw < no;
        const uint32_t ro = live ? ro_raw : qo + 1;   // (idle lanes read nothing of the table; qo + 1 < no keeps their tree lookups in range)
        const uint32_t r = ro < lo ? ro : ro + s;
        // the lane's constants: Q = lca(q,r), its parent link and its children towards q and r
        const uint32_t eQ = L[(size_t)q * n + r];
        const uint32_t dQ = eQ >> 16;
        const uint32_t upQ = N + cd.inner_node[eQ & 0xFFFFu];
        const uint32_t lq = cd.child[(size_t)r * n + q], lr = cd.child[(size_t)q * n + r];
        const uint32_t *__restrict__ lrow = L + (size_t)q * n;
        const uint16_t *__restrict__ nrow = cd.next + (size_t)q * n;
        const uint16_t *__restrict__ crow = cd.child + (size_t)q * n;
        uint32_t end = 0, cp = 0, cq = 0, upP = 0;          // uniform: the run's end and its three targets
        bool c1 = false, c13 = false, c2 = false, c23 = false, any1 = false, any13 = false;
        ACC Ucp = 0, Ucq = 0, Uup = 0;                      // the lane's share of the run's wave-uniform targets
        ACC Aup = 0, Alq = 0, Alr = 0;                      // the lane's own targets, over the whole walk
        auto close_run = [&]() {
            if (any13) { const unsigned long long t = clade_wave_sum((unsigned long long)Ucp); if (lane == 0 && t) atomicAdd(&acc[cp], t); }
            if (any1) {
                const unsigned long long t = clade_wave_sum((unsigned long long)Ucq), t2 = clade_wave_sum((unsigned long long)Uup);
                if (lane == 0 && t) atomicAdd(&acc[cq], t);
                if (lane == 0 && t2) atomicAdd(&acc[upP], t2);
            }
            Ucp = 0; Ucq = 0; Uup = 0;
        };
        // one step of the walk: the triple (p,q,r) with its three counts summed over the slice's x
        auto step = [&](uint32_t p, ACC vp, ACC vq, ACC vr) {
            if (p == end || p == hi) {                      // uniform: lca(p,q) or its child towards p changes here, or the walk has jumped
                close_run();
                const uint32_t eP = __builtin_amdgcn_readfirstlane(lrow[p]);
                const uint32_t dP = eP >> 16;
                upP = N + __builtin_amdgcn_readfirstlane(cd.inner_node[eP & 0xFFFFu]);
                cp = __builtin_amdgcn_readfirstlane((uint32_t)crow[p]);
                cq = __builtin_amdgcn_readfirstlane((uint32_t)cd.child[(size_t)p * n + q]);
                end = __builtin_amdgcn_readfirstlane((uint32_t)nrow[p]);
                c1 = live && dP > dQ; c2 = live && dP < dQ;
                c13 = live && dP >= dQ; c23 = live && dP <= dQ;
                any1 = __any(c1) != 0; any13 = __any(c13) != 0;
            }
            Ucp += c13 ? vp : (ACC)0; Ucq += c1 ? vq : (ACC)0; Uup += c1 ? vr : (ACC)0;
            Aup += c2 ? vp : (ACC)0; Alq += c23 ? vq : (ACC)0; Alr += c23 ? vr : (ACC)0;
        };
        // first stretch [0, seg): where the interval stands behind q decides the rows and the cells (per lane: r < lo or hi <= r)
        const uint32_t seg = min(q, lo);
        if (seg) {
            const uint32_t kind = q >= hi ? 2u : r >= hi ? 1u : 0u;
            const uint64_t rank0 = kind == 2 ? binom4(r) + binom3(q) + binom2(xa) : kind == 1 ? binom4(r) + binom3(xa) + binom2(q) : binom4(xa) + binom3(r) + binom2(q);
            const uint32_t pp = kind == 2 ? 0u : kind == 1 ? 1u : 2u, pq = kind == 0 ? 1u : 2u, pr = kind == 2 ? 1u : 0u;   // the cell of p, of q, of r
            for (uint32_t p0 = 0; p0 < seg; p0 += CH) {     // uniform
                ACC t[CH][3];
#pragma unroll
                for (int u = 0; u < CH; ++u) t[u][0] = t[u][1] = t[u][2] = 0;
                if (live) {
                    uint64_t row = (rank0 + p0) * 3;        // of x = xa; the next x: + 3 x, + 3 C(x,2), + 3 C(x,3) tuples further
                    uint64_t b2 = binom2(xa), b3 = binom3(xa);
                    const bool whole = p0 + CH <= seg;      // uniform: else the stretch's last steps, tuple by tuple
                    for (uint32_t x = xa; x < xb; ++x) {    // uniform
                        if (whole) clade_add_chunk<CT, ACC, CH>(table + row, t);
                        else {
#pragma unroll
                            for (int u = 0; u < CH; ++u)
                                if (p0 + u < seg) {
                                    const CT *src = table + row + 3 * u;
                                    t[u][0] += (ACC)src[0]; t[u][1] += (ACC)src[1]; t[u][2] += (ACC)src[2];
                                }
                        }
                        row += 3 * (kind == 2 ? (uint64_t)x : kind == 1 ? b2 : b3);
                        b3 += b2; b2 += x;
                    }
                }
#pragma unroll
                for (int u = 0; u < CH; ++u) {
                    const uint32_t p = p0 + u;
                    if (p < seg) {                          // uniform
                        const ACC vp = pp == 0 ? t[u][0] : pp == 1 ? t[u][1] : t[u][2];
                        const ACC vq = pq == 1 ? t[u][1] : t[u][2];
                        const ACC vr = pr == 0 ? t[u][0] : t[u][1];
                        step(p, vp, vq, vr);
                    }
                }
            }
        }
        // second stretch [hi, q): the tuples of (x,p,q,r) over x are consecutive
        if (q > hi) {
            const uint64_t base = (binom4(r) + binom3(q) + xa) * 3;
            for (uint32_t p0 = hi; p0 < q; p0 += PU) {      // uniform
                ACC t[PU][3];
#pragma unroll
                for (int u = 0; u < PU; ++u) t[u][0] = t[u][1] = t[u][2] = 0;
                if (live) {
                    const CT *src[PU];
#pragma unroll
                    for (int u = 0; u < PU; ++u) src[u] = table + base + 3 * binom2(min(p0 + u, q - 1));
                    uint32_t j = 0;
                    for (; j + CH <= cnt; j += CH) {        // uniform
#pragma unroll
                        for (int u = 0; u < PU; ++u)
                            if (p0 + u < q) {               // uniform
                                ACC c[CH][3];
#pragma unroll
                                for (int e = 0; e < CH; ++e) c[e][0] = c[e][1] = c[e][2] = 0;
                                clade_add_chunk<CT, ACC, CH>(src[u] + 3 * (size_t)j, c);
#pragma unroll
                                for (int e = 0; e < CH; ++e) { t[u][0] += c[e][0]; t[u][1] += c[e][1]; t[u][2] += c[e][2]; }
                            }
                    }
                    for (; j < cnt; ++j) {                  // uniform
#pragma unroll
                        for (int u = 0; u < PU; ++u)
                            if (p0 + u < q) {
                                const CT *one = src[u] + 3 * (size_t)j;
                                t[u][0] += (ACC)one[0]; t[u][1] += (ACC)one[1]; t[u][2] += (ACC)one[2];
                            }
                    }
                }
#pragma unroll
                for (int u = 0; u < PU; ++u)
                    if (p0 + u < q) step(p0 + u, t[u][0], t[u][1], t[u][2]);
            }
        }
        close_run();
        if (live) {
            if (Aup) atomicAdd(&acc[upQ], (unsigned long long)Aup);
            if (Alq) atomicAdd(&acc[lq], (unsigned long long)Alq);
            if (Alr) atomicAdd(&acc[lr], (unsigned long long)Alr);
        }
    }
    __syncthreads();
    unsigned long long *out = dst + (size_t)ci * cells;
    for (uint32_t i = tid; i < cells; i += kThreads) {
        const unsigned long long v = acc[i];
        if (v) atomicAdd(&out[i], v);
    }
}

template <typename CT, typename ACC>
static hipError_t launch_clade_t(hipStream_t s, const CladeDevice &cd, uint32_t n_groups, unsigned long long *dst) {
    if (n_groups == 0) return hipSuccess;
    const size_t lds = place_lds_bytes(cd.n_nodes);
    if (lds > 160u * 1024u) return hipErrorInvalidValue;
    auto k = place_clade_kernel<CT, ACC>;
    hipError_t e = hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    dim3 block(kPlaceWaves * kWave), grid(n_groups);
    hipLaunchKernelGGL(k, grid, block, lds, s, cd, dst);
    return hipGetLastError();
}

// dst (one row of 2 x n_nodes words per listed clade, zeroed by the caller) += the link sums of the clades cd.clades[0 ..)
hipError_t launch_clade_placement(hipStream_t s, const CladeDevice &cd, uint32_t n_groups, bool wide, unsigned long long *dst) {
    if (cd.count_bits == 16) return wide ? launch_clade_t<uint16_t, unsigned long long>(s, cd, n_groups, dst) : launch_clade_t<uint16_t, uint32_t>(s, cd, n_groups, dst);
    return wide ? launch_clade_t<uint32_t, unsigned long long>(s, cd, n_groups, dst) : launch_clade_t<uint32_t, uint32_t>(s, cd, n_groups, dst);
}

} // namespace qs
