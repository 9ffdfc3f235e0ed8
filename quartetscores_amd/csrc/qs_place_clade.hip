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
// Shape: the taxon gather's (qs_taxon_walk.hpp). A wave owns the middle id q, its lanes 64 consecutive largest ids r > q (both outside the clade: the
// walks are numbered in the n - |C| outside ids and mapped over the interval), and walks p over [0, min(q, lo)) and then over
// [hi, q): the walk jumps the interval.
//   first stretch (p < lo)   per x one table row, consecutive in p, the taxon gather's first three address cases:
//       r < lo        (p,q,r,x)  rank C(x,4) + C(r,3) + C(q,2) + p   cells (r, q, p)
//       q < lo, hi<=r (p,q,x,r)  rank C(r,4) + C(x,3) + C(q,2) + p   cells (r, p, q)
//       hi <= q       (p,x,q,r)  rank C(r,4) + C(q,3) + C(x,2) + p   cells (p, r, q)
//     a chunk of 8 / 16 steps is requested as 96 bytes of 16-byte loads from the row of every x and summed over x in registers;
//   second stretch (hi <= p) (x,p,q,r)  rank C(r,4) + C(q,3) + C(p,2) + x   cells (p, q, r): consecutive in x, the clade's tuples
//     are one contiguous piece of a table row, streamed in the same 96-byte chunks (what is left over: tuple by tuple), four
//     steps of p requested together.
// Then one accounting per step, PlaceAccount of qs_taxon_walk.hpp. A run of place_next may span the interval (a child of lca(p,q) can hold
// p, the clade and p' together): at p = hi the run is always closed and its state read again.
// A large clade is cut into x-slices [xa, xb) so that one clade alone still fills the device; an item = (walk, x-slice). The
// workgroups are listed by the host (clade, first item, stride): a workgroup stays with one clade, its 2N 64-bit LDS words
// are flushed once with one 64-bit atomic per non-zero cell. Integer sums: independent of order, grid and slicing.
// 32-bit register sums hold at most (n - |C| - 2 steps) x (slice length) tuples: the host (qs_clade_placement) keeps
// (n - |C|) x slice x (largest count) < 2^32 by shortening the slices, and picks the instance with 64-bit sums otherwise.
#include "qs_taxon_walk.hpp"

namespace qs {

template <typename CT, typename ACC>
__global__ __launch_bounds__(kPlaceWaves * kWave) void place_clade_kernel(CladeDevice cd, unsigned long long *__restrict__ dst) {
    extern __shared__ __align__(16) unsigned char clade_smem[];
    unsigned long long *acc = reinterpret_cast<unsigned long long *>(clade_smem);   // [link]
    constexpr int CH = WalkChunk<CT>::CH;                   // tuples a lane requests at once: 96 bytes
    constexpr int PU = 4;                                   // steps of the second stretch requested together
    const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const uint32_t n = cd.n, cells = 2 * cd.n_nodes;
    const uint32_t ci = cd.groups[2 * blockIdx.x], ks = cd.groups[2 * blockIdx.x + 1];
    const uint32_t first = ks & 0xFFFFu, share = ks >> 16;
    const uint32_t lo = cd.clades[4 * ci], hi = cd.clades[4 * ci + 1], xs = cd.clades[4 * ci + 2], n_tasks = cd.clades[4 * ci + 3];
    const uint32_t s = hi - lo, no = n - s, nsl = (s + xs - 1) / xs, n_items = n_tasks * nsl;
    walk_zero(acc, cells);
    __syncthreads();
    const CT *table = reinterpret_cast<const CT *>(cd.table);
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
        // one step of the walk: the triple (p,q,r) with its three counts summed over the slice's x; at p = hi the walk has jumped
        PlaceAccount<ACC> a;
        a.begin(cd.ref_lca, cd.inner_node, cd.child, cd.next, n, cd.n_nodes, q, r, live);
        auto step = [&](uint32_t p, ACC vp, ACC vq, ACC vr) { a.run_break(p, p == hi, acc, lane); a.step(vp, vq, vr); };
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
                        if (whole) walk_chunk<true>(table + row, true, t);
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
                                walk_chunk<true>(src[u] + 3 * (size_t)j, true, c);
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
        a.finish(acc, lane);
    }
    __syncthreads();
    walk_flush(acc, cells, dst + (size_t)ci * cells);
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
