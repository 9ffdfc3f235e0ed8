// qs_abi_count.hip -- the count step of the C-ABI: batch staging and upload, the launch order, slices, and the dispatch of the count
// kernels with their depth-clamp corrections (run_launch, qs_count_batch). Host code only.
#include "qs_ctx.hpp"
#include "qs_plan.hpp"

#include <algorithm>
#include <cstring>
#include <string>
#include <thread>
#include <utility>
#include <vector>

using namespace qs;

// Tree groups (panel elements along the tree axis) per sub-batch of a batch of n_total groups.
// A batch is counted slice by slice: panel build + count kernel per slice, the first slice stores into the table, the
// others read-modify-write it. qs_set_tuning(QS_TUNE_PANEL_SLICE_BYTES) fixes the slice size in bytes (tests, sweeps).
//  * bit-sliced kernel in (a,b)-major tile order (the default): what must stay in an XCD's 4 MB L2 is the working set of
//    its concurrent tiles, which grows with the number of groups G of the slice (about 40 KB x G at 20-byte elements), not
//    with the panel's size; against that every extra slice costs one read + one write of the table. Measured optimum
//    (profiles/r02_experiments.md): 128-150 groups at 256 taxa (2 GB table), ~105 at 512 taxa (34 GB table; 3 slices
//    for 10000 trees: 401 ms, 2: 415, 5: 432, unsliced 440), >= 80 at 1024 taxa (34 GB table shard). Rule: 128 groups,
//    slices balanced (313 groups -> 3 x 105, not 128 + 128 + 57), at most 2 GiB of panel.
//  * (d,c)-major order and the byte-SWAR kernel: the whole slice has to stay in the 256 MiB Infinity Cache while every
//    wave streams through it: 96 MiB, but at least 32 groups (a tile's fixed cost needs that many steps to amortise),
//    capped at 384 MiB (round-1 measurements: 512 taxa 0.60 s at 100 MB, 0.72 s at 50 MB, 0.80 s unsliced).
uint32_t qs::slice_groups(const qs_ctx *c, size_t group_bytes, uint32_t n_total, bool ab_major) {
    size_t g;
    bool balance = false;
    if (c->tune_slice_bytes) g = (size_t)c->tune_slice_bytes / group_bytes;
    else if (ab_major) {
        // Every slice costs a pass over the table (read + write of every tuple), a larger slice a larger L2 working set. Measured
        // on the round-3 kernel (profiles/r03_experiments.md 14): 512 taxa x 30000 trees best at 256 groups per slice (670 MB;
        // 128: +3.5 %, 512: +0.7 %), 256 taxa x 100000 best at 512 groups (334 MB; 128: +3 %, 1024: +1.5 %), a 34 GB shard of 1024
        // taxa x 5000 trees best in ONE slice of 157 groups (1.65 GB; two slices: +5 %): 256 groups, but at least 350 MB worth.
        g = std::max<size_t>(256, (350ull << 20) / group_bytes);
        g = std::min<size_t>(g, std::max<size_t>(1, (4096ull << 20) / group_bytes));
        balance = true;
    }
    else g = std::min<size_t>(std::max<size_t>(96ull << 20, 32 * group_bytes), 384ull << 20) / group_bytes;
    g = std::min<size_t>(std::max<size_t>(g, 1), std::max<uint32_t>(n_total, 1));
    // (round 5: up to 1.5 slices' worth stays ONE slice -- 313 groups at configs[2] since the depth clamp put all 10000 trees in one
    // class: 301.5 ms in one slice against 308.1 ms in two of 157, the second pass over the table costs more than the larger L2 set)
    if (balance && !c->tune_slice_bytes && n_total <= g + g / 2) g = std::max<uint32_t>(n_total, 1);
    if (balance) { const size_t slices = (n_total + g - 1) / g; g = (n_total + slices - 1) / std::max<size_t>(slices, 1); }
    return (uint32_t)std::max<size_t>(g, 1);
}

// QS_COUNT_TIMED: an event after every kernel launch of the call (created on demand, re-used by later calls)
// The event goes onto the stream its kernel ran on (`on`; NULL pointer = the context's stream). Its interval starts at event
// `from` (index into evs), by default the event recorded before it.
hipError_t qs::mark(qs_ctx *c, int kind, const hipStream_t *on, uint32_t from) {
    if (c->ev_used == c->evs.size()) {
        hipEvent_t e;
        hipError_t rc = hipEventCreate(&e);
        if (rc != hipSuccess) return rc;
        c->evs.push_back(e); c->ev_kind.push_back(0); c->ev_from.push_back(0);
    }
    c->ev_kind[c->ev_used] = (uint8_t)kind;
    c->ev_from[c->ev_used] = from != kEvPrev ? from : (c->ev_used ? c->ev_used - 1 : 0);
    return hipEventRecord(c->evs[c->ev_used++], on ? *on : c->stream);
}

// (a,b)-major launch order of the tiles of count_bitslice3_kernel. The kernel decodes a tile id as (d-block k, c, tile
// inside c) -- the order in which the TABLE is contiguous. Walked in that order, the waves that run at the same time
// cover every (a,b) pair, so the private M[ab] loads (60 % of a wave's panel bytes) never hit in L2 and the launch is
// bound by the Infinity Cache (knock-out at 512 taxa: no panel loads = 45 % less time; profiles/r02_experiments.md).
// Here the launch slots are permuted: outermost the b-block Bk and a chunk of `chunk` a-blocks (pairs of a-blocks in
// the binary tiling) under it, then blocks of `cblock` values of c, then the d-blocks, then c inside the block,
// innermost the a-blocks of the chunk. Concurrent waves of an XCD (with xcd_remap each XCD walks a contiguous eighth of
// the slots) then share one chunk's M[ab] elements (8 b-rows x 16*chunk a's x the tree groups of the slice), the
// M[bd] elements of (Bk, d-block) and the M[xc] rows of the c-block, which stay in its 4 MB L2; per (c,d) a chunk still
// writes 8 contiguous runs of the table. Diagonal tiles follow at the end. 512 taxa x 10000 trees: 568 -> 401 ms,
// 256 taxa: -35 %. Shards with more than 2^26 tiles keep the (d,c)-major order (the slot array would be > 256 MB).
int qs::tile_order(qs_ctx *c, const uint32_t **out) {
    *out = nullptr;
    if (c->perm_built) { *out = c->perm.get(); return QS_OK; }
    c->perm_built = true;
    const uint32_t total = c->total_tiles3;
    const uint32_t chunk = c->tile_chunk;
    if (chunk == 0 || total == 0 || total > (1u << 26)) {
        if (c->perm_early.valid()) c->perm_early.wait();
        return QS_OK;
    }
    const uint32_t d_hi = c->d_hi, n_dblk = c->n_dblk;
    const std::vector<uint32_t> &cp = c->h_cp3, &dp = c->h_dp3;
    const TilePermParams P{chunk, c->tile_cblock, c->tile_cgroup, d_hi, n_dblk, total};
    std::vector<uint32_t> perm;
    std::string perr;
    bool have = false;
    if (c->perm_early.valid()) {       // started by qs_create beside the HIP start-up
        EarlyPerm ep = c->perm_early.get();
        if (ep.ok && ep.chunk == P.chunk && ep.cblock_in == P.cblock_in && ep.cgroup == P.cgroup) { perm.swap(ep.perm); have = true; }
    }
    if (!have && !build_tile_perm(P, cp, dp, perm, perr)) return fail(c, QS_ERR_STATE, perr);
    auto T_of = [](uint32_t cc) { return (cc + 7) / 8; };
    const uint32_t cmax = d_hi >= 2 ? d_hi - 2 : 0;
    const uint32_t Tmax = T_of(cmax);
    const uint32_t cblock = c->tile_cblock ? c->tile_cblock : cmax + 1;
    // Off unless asked for (QS_TUNE_COOP = 1): measured on MI355X the real barrier per 32-tree step costs more than the
    // shared loads save (512 taxa x 10000 trees: 368 ms against 354 ms; profiles/r03_experiments.md)
    if (c->tune_coop == 1) {
        // Cooperative launch order: same nesting ((a,b)-major: b-block, chunk of a-block pairs, c-block, d-block), but
        // innermost FOUR consecutive c of one a-block pair -- one workgroup of count_bitslice4_kernel. A group short of
        // four valid c is filled with shadow copies of its first tile.
        std::vector<uint32_t> coop, rest;
        coop.reserve(total + total / 8);
        for (uint32_t Bk = 1; Bk < Tmax; ++Bk) {
            const uint32_t base = (Bk * Bk) / 4;
            const uint32_t nj = ((Bk + 1) * (Bk + 1)) / 4 - base;     // tiles under this b-block; the last one lacks a2 when Bk is odd
            const uint32_t nj2 = Bk / 2;                              // pairs (2j, 2j+1) with 2j+1 < Bk
            const uint32_t c_lo = std::max(2u, 8 * Bk + 1);
            for (uint32_t j0 = 0; j0 < nj2; j0 += chunk) {
                const uint32_t j1 = std::min(nj2, j0 + chunk);
                for (uint32_t cb = c_lo; cb <= cmax; cb += cblock)
                    for (uint32_t k = 0; k < n_dblk; ++k) {
                        const uint32_t d1 = d_hi - k * kDB;
                        for (uint32_t j = j0; j < j1; ++j)
                            for (uint32_t c4 = cb; c4 < cb + cblock && c4 + 1 < d1; c4 += 4) {
                                const uint32_t first = dp[k] + cp[c4] + base + j;
                                for (uint32_t cc = c4; cc < c4 + 4; ++cc)
                                    coop.push_back((cc < cb + cblock && cc + 1 < d1) ? dp[k] + cp[cc] + base + j : (first | 0x80000000u));
                            }
                    }
            }
            if (nj > nj2)                                            // the tile with a single a-block
                for (uint32_t k = 0; k < n_dblk; ++k) {
                    const uint32_t d1 = d_hi - k * kDB;
                    for (uint32_t cc = c_lo; cc + 1 < d1; ++cc) rest.push_back(dp[k] + cp[cc] + base + nj2);
                }
        }
        for (uint32_t kd = 0; kd < (Tmax + 1) / 2; ++kd)
            for (uint32_t k = 0; k < n_dblk; ++k) {
                const uint32_t d1 = d_hi - k * kDB;
                for (uint32_t cc = 2; cc + 1 < d1; ++cc) {
                    const uint32_t T = T_of(cc);
                    if (kd < (T + 1) / 2) rest.push_back(dp[k] + cp[cc] + (T * T) / 4 + kd);
                }
            }
        {   // coop (without shadows) and rest together: every tile exactly once
            std::vector<uint8_t> seen(total, 0);
            size_t real = 0;
            auto take = [&](uint32_t id) { if (id >= total || seen[id]) return false; seen[id] = 1; ++real; return true; };
            for (uint32_t id : coop) if (!(id & 0x80000000u) && !take(id)) return fail(c, QS_ERR_STATE, "tile order: cooperative list is not a partition");
            for (uint32_t id : rest) if (!take(id)) return fail(c, QS_ERR_STATE, "tile order: rest list is not a partition");
            if (real != total || coop.size() % 4) return fail(c, QS_ERR_STATE, "tile order: cooperative + rest lists do not cover the tiling");
        }
        if (!coop.empty()) {
            if (c->perm_coop.reserve(coop.size() * 4, nullptr) != hipSuccess || c->perm_rest.reserve(std::max<size_t>(rest.size(), 1) * 4, nullptr) != hipSuccess)
                return fail(c, QS_ERR_OOM, "hipMalloc tile order (cooperative lists)");
            if (hipMemcpyAsync(c->perm_coop.get(), coop.data(), coop.size() * 4, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
                (!rest.empty() && hipMemcpyAsync(c->perm_rest.get(), rest.data(), rest.size() * 4, hipMemcpyHostToDevice, c->stream) != hipSuccess) ||
                hipStreamSynchronize(c->stream) != hipSuccess) return fail(c, QS_ERR_HIP, "memcpy tile order (cooperative lists)");
            c->n_coop = (uint32_t)coop.size(); c->n_rest = (uint32_t)rest.size();
        }
    }
    if (c->perm.reserve(perm.size() * 4, nullptr) != hipSuccess) return fail(c, QS_ERR_OOM, "hipMalloc tile order");
    if (hipMemcpyAsync(c->perm.get(), perm.data(), perm.size() * 4, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess) return fail(c, QS_ERR_HIP, "memcpy tile order");
    *out = c->perm.get();
    return QS_OK;
}

// The launch-order lists depend on the tile-order tuning and on QS_TUNE_COOP: dropped here, tile_order rebuilds them on next use.
int qs::drop_tile_order(qs_ctx *c) {
    QS_HIP(c, hipSetDevice(c->device));
    QS_HIP(c, hipStreamSynchronize(c->stream));
    c->perm.reset(); c->perm_coop.reset(); c->perm_rest.reset();
    c->perm_built = false; c->n_coop = c->n_rest = 0;
    c->split.d_mid = 0;   // (cut from the order just dropped)
    return QS_OK;
}

// ---- batches -----------------------------------------------------------------------------

extern "C" void qs_batch_free(qs_ctx *c, qs_device_batch *b) {
    if (!b) return;
    if (c) (void)hipSetDevice(c->device);
    DeviceBatch &d = b->d;
    if (d.ready) { (void)hipEventSynchronize(d.ready); (void)hipEventDestroy(d.ready); }
    if (d.slab.p) {
        // kernels that read the batch may still be queued: remember where the compute stream stands and keep the slab
        bool kept = false;
        if (c && c->slabs.size() < 4) {
            if (!d.slab.last_use && hipEventCreateWithFlags(&d.slab.last_use, hipEventDisableTiming) != hipSuccess) d.slab.last_use = nullptr;
            if (d.slab.last_use && hipEventRecord(d.slab.last_use, c->stream) == hipSuccess) { c->slabs.push_back(d.slab); kept = true; }
        }
        if (!kept) { (void)hipFree(d.slab.p); if (d.slab.last_use) (void)hipEventDestroy(d.slab.last_use); }   // (hipFree waits for the device)
    }
    delete b;
}

// One batch's arrays are packed (256-byte aligned pieces) into a pinned staging buffer of the context and go to a device
// slab of the same layout with ONE copy on the copy stream. Slabs come from a small cache of the context: qs_batch_free
// records where the compute stream stands and hands the slab back, the next upload makes the copy stream wait for that
// point -- no hipMalloc / hipFree (a device-wide synchronisation) per batch, and no host thread ever waits for a kernel.
struct Stager {
    qs_ctx *c = nullptr; int slot = 0; size_t off = 0, need = 0; hipError_t err = hipSuccess;
    BatchSlab slab;
    hipError_t begin(qs_ctx *ctx, size_t bytes) {
        c = ctx; need = std::max<size_t>(bytes, 256); slot = (int)(c->pin_next++ & 1u);
        hipError_t e = hipSuccess;
        if (!c->copy_stream) e = hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking);
        if (e == hipSuccess && !c->pin_ev[slot]) e = hipEventCreateWithFlags(&c->pin_ev[slot], hipEventDisableTiming);
        else if (e == hipSuccess) e = hipEventSynchronize(c->pin_ev[slot]);      // its previous contents are on the device
        if (e == hipSuccess) e = ensure_pinned(c, slot, need);
        if (e != hipSuccess) return err = e;
        // device slab: the smallest cached one that is large enough, else a new one
        int best = -1;
        for (size_t i = 0; i < c->slabs.size(); ++i)
            if (c->slabs[i].cap >= need && (best < 0 || c->slabs[i].cap < c->slabs[(size_t)best].cap)) best = (int)i;
        if (best >= 0) { slab = c->slabs[(size_t)best]; c->slabs.erase(c->slabs.begin() + best); }
        else {
            slab = BatchSlab();
            slab.cap = need + need / 4;
            e = hipMalloc(&slab.p, slab.cap);
            if (e != hipSuccess) { slab = BatchSlab(); return err = e; }
        }
        if (slab.last_use) e = hipStreamWaitEvent(c->copy_stream, slab.last_use, 0);   // kernels of its previous batch
        return err = e;
    }
    template <typename T> T *put(const T *src, size_t count) {
        if (err != hipSuccess) return nullptr;
        const size_t bytes = count * sizeof(T);
        if (count) std::memcpy(static_cast<unsigned char *>(c->pin[slot].get()) + off, src, bytes);
        T *dev = reinterpret_cast<T *>(static_cast<unsigned char *>(slab.p) + off);
        off += padded(bytes);
        return dev;
    }
    // `ready` fires when the batch is on the device; the staging buffer is free again at the same moment
    hipError_t finish(hipEvent_t *ready) {
        if (err != hipSuccess) return err;
        err = hipMemcpyAsync(slab.p, c->pin[slot].get(), std::max<size_t>(off, 1), hipMemcpyHostToDevice, c->copy_stream);
        if (err == hipSuccess) err = hipEventCreateWithFlags(ready, hipEventDisableTiming);
        if (err == hipSuccess) err = hipEventRecord(*ready, c->copy_stream);
        if (err == hipSuccess) err = hipEventRecord(c->pin_ev[slot], c->copy_stream);
        return err;
    }
};

extern "C" int qs_batch_upload(qs_ctx *c, const qs_tree_batch *hb, qs_device_batch **out) {
    if (!c || !hb || !out) return fail(c, QS_ERR_ARG, "qs_batch_upload: NULL argument");
    *out = nullptr;
    if (!hb->leaf_off || (hb->n_trees && (!hb->leaf_ids || !hb->adj_depth)))
        return fail(c, QS_ERR_ARG, "qs_batch_upload: leaf arrays missing");
    const uint32_t nt = hb->n_trees, n = c->n;
    // ---- validate (the reference dies on malformed input; we return a status) ----
    // Trees are independent: large batches are checked by a few host threads, the first error in tree order wins.
    struct Part { uint32_t max_depth = 0; bool all_full = true, all_binary = true; uint32_t err_tree = 0xFFFFFFFFu; std::string err; };
    std::vector<uint16_t> tree_depth(nt, 0); // deepest LCA of every tree
    std::vector<uint8_t> tree_mode(nt, 0);   // CountMode of every tree: the cheapest kernel instance that is exact for it
    std::vector<uint8_t> eff_soft(nt, 0), eff_hard(nt, 0);   // depth clamp: the lowest class (depth bits) the budget allows the tree (clamp_choice)
    const uint64_t clamp_budget = (uint64_t)((double)binom4(n) * (double)c->tune_clamp_ppm * 1e-6);
    auto check = [&](uint32_t t0, uint32_t t1, Part &P) {
        std::vector<uint32_t> stamp(n, 0xFFFFFFFFu);
        std::vector<uint32_t> stack;
        auto bad = [&](uint32_t t, const std::string &m) { P.err_tree = t; P.err = m; };
        for (uint32_t t = t0; t < t1; ++t) {
            if (hb->leaf_off[t + 1] < hb->leaf_off[t]) return bad(t, "qs_batch_upload: leaf_off not monotone");
            const uint32_t base = hb->leaf_off[t], L = hb->leaf_off[t + 1] - base;
            if (L > n) return bad(t, "qs_batch_upload: tree " + std::to_string(t) + " has more leaves than taxa");
            if (L != n) P.all_full = false;
            for (uint32_t i = 0; i < L; ++i) {
                const uint32_t id = hb->leaf_ids[base + i];
                if (id >= n) return bad(t, "qs_batch_upload: tree " + std::to_string(t) + ": taxon id out of range (unknown taxon)");
                if (stamp[id] == t) return bad(t, "qs_batch_upload: tree " + std::to_string(t) + ": duplicate taxon");
                stamp[id] = t;
            }
            // internal nodes from the adjacent-LCA depth sequence
            uint32_t depth = 0;
            bool binary = false;
            tree_shape(hb->adj_depth + base, L, stack, depth, binary);
            P.max_depth = std::max(P.max_depth, depth);
            tree_depth[t] = (uint16_t)depth;
            if (!binary) P.all_binary = false;
            tree_mode[t] = (uint8_t)(L == n ? (binary ? MODE_BINARY_FULL : MODE_GENERAL_FULL) : (binary ? MODE_BINARY_PARTIAL : MODE_PARTIAL));
            clamp_choice(hb->adj_depth + base, L, depth_class_of(tree_depth[t]), clamp_budget, eff_soft[t], eff_hard[t]);
        }
    };
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    const unsigned workers = nt >= 2048 ? std::min(8u, std::min(hw, nt / 1024)) : 1u;
    std::vector<Part> parts(workers);
    if (workers == 1) check(0, nt, parts[0]);
    else {
        std::vector<std::thread> pool;
        for (unsigned w = 0; w < workers; ++w)
            pool.emplace_back([&, w] { check((uint32_t)((uint64_t)nt * w / workers), (uint32_t)((uint64_t)nt * (w + 1) / workers), parts[w]); });
        for (auto &th : pool) th.join();
    }
    uint32_t max_depth = 0;
    bool all_full = true, all_binary = true;
    for (const Part &P : parts) { // parts are in tree order: the first one with an error holds the earliest bad tree
        if (P.err_tree != 0xFFFFFFFFu) return fail(c, QS_ERR_ARG, P.err);
        max_depth = std::max(max_depth, P.max_depth);
        all_full = all_full && P.all_full; all_binary = all_binary && P.all_binary;
    }
    qs_device_batch *b = new qs_device_batch();
    DeviceBatch &d = b->d;
    d.n_trees = nt;
    d.total_leaves = nt ? hb->leaf_off[nt] : 0;
    d.max_depth = max_depth; d.all_full = all_full && nt > 0; d.all_binary = all_binary && nt > 0;
    // classes = (kernel mode, depth bits) per tree: plan_classes (qs_plan.hip)
    std::vector<uint32_t> order_host;
    std::vector<FixUnit> fix_units;
    ClassPlan plan;
    {
        TreeFacts F;
        F.depth.swap(tree_depth); F.mode.swap(tree_mode); F.soft.swap(eff_soft); F.hard.swap(eff_hard);
        plan_classes(n, nt, hb->leaf_off, hb->adj_depth, F, c->tune_class_min, c->tune_class_pct, c->tune_clamp_ppm, plan,
                     c->tune_fuse && c->tune_gather_impl != QS_IMPL_SWAR);
        tree_depth.swap(F.depth); tree_mode.swap(F.mode);
        d.n_classes = plan.n_classes;
        for (uint32_t k = 0; k < plan.n_classes; ++k) { d.class_mode[k] = plan.class_mode[k]; d.class_bits[k] = plan.class_bits[k]; d.class_end[k] = plan.class_end[k]; d.class_max_depth[k] = plan.class_max_depth[k]; }
        order_host = plan.order;
        constexpr uint32_t top_bits = 10;
        // correction units of the trees whose class holds fewer depth bits than they need, by slot (a slice of a class = a range of
        // slots = a range of units). One unit = one workgroup = a stretch of a run's triples worth ~32 K fourth leaves.
        if (c->tune_clamp_ppm) {
            std::vector<std::pair<uint32_t, uint32_t>> runs;
            auto emit = [&](uint32_t slot, uint32_t t) {
                const uint32_t fb = plan.bits[t];
                if (fb > top_bits || depth_class_of(tree_depth[t]) <= fb) return;
                const uint32_t base = hb->leaf_off[t], L = hb->leaf_off[t + 1] - base;
                runs.clear();
                const uint64_t cost = clamp_cost(hb->adj_depth + base, L, (1u << fb) - 1u, &runs);
                if (cost == ~0ull) return;   // cannot happen: the cut of a lower class was accepted, and runs only shrink with the cut
                d.fix_quartets += cost; d.clamped_trees++;
                const uint32_t per_unit = std::max<uint32_t>(1u, 32768u / std::max<uint32_t>(L, 1u));
                for (const auto &r : runs) {
                    const uint32_t triples = (uint32_t)binom3(r.second);
                    for (uint32_t t0 = 0; t0 < triples; t0 += per_unit) {
                        fix_units.push_back(FixUnit{t, r.first | (r.second << 16), t0, std::min(triples, t0 + per_unit)});
                        b->fix_slot.push_back(slot);
                        if (b->fix_work.empty()) b->fix_work.push_back(0);
                        b->fix_work.push_back(b->fix_work.back() + (uint64_t)(std::min(triples, t0 + per_unit) - t0) * (L > 3 ? L - 3 : 0));
                    }
                }
            };
            if (order_host.empty()) for (uint32_t t = 0; t < nt; ++t) emit(t, t);
            else for (uint32_t sl = 0; sl < nt; ++sl) emit(sl, order_host[sl]);
            d.n_fix = (uint32_t)fix_units.size();
        }
    }
    // scatter batches: the tree of every inner node, and a bounds check of the leaf ranges (host side, before any copy)
    const bool with_nodes = hb->node_off && hb->rng_off && hb->ranges;
    std::vector<uint32_t> node_tree;
    if (with_nodes) {
        d.n_nodes = hb->node_off[nt];
        d.n_links = hb->rng_off[d.n_nodes];
        node_tree.resize(d.n_nodes);
        for (uint32_t t = 0; t < nt; ++t) {
            const uint32_t L = hb->leaf_off[t + 1] - hb->leaf_off[t];
            d.max_tree_nodes = std::max(d.max_tree_nodes, hb->node_off[t + 1] - hb->node_off[t]);
            for (uint32_t v = hb->node_off[t]; v < hb->node_off[t + 1]; ++v) {
                node_tree[v] = t;
                for (uint32_t k = hb->rng_off[v]; k < hb->rng_off[v + 1]; ++k)
                    if (hb->ranges[2 * k] >= std::max(L, 1u) || hb->ranges[2 * k + 1] >= std::max(L, 1u)) {
                        qs_batch_free(c, b);
                        return fail(c, QS_ERR_ARG, "qs_batch_upload: range position out of bounds");
                    }
            }
        }
    }
    hipError_t e = hipSetDevice(c->device);
    Stager st;
    if (e == hipSuccess) {
        size_t need = padded(((size_t)nt + 1) * 4) + 2 * padded((size_t)d.total_leaves * 2) + padded(order_host.size() * 4) +
                      padded(fix_units.size() * sizeof(FixUnit));
        if (with_nodes) need += padded(((size_t)nt + 1) * 4) + padded(((size_t)d.n_nodes + 1) * 4) + padded((size_t)d.n_nodes * 4) + padded((size_t)2 * d.n_links * 2);
        e = st.begin(c, need);
    }
    if (e == hipSuccess) {
        d.leaf_off = st.put(hb->leaf_off, (size_t)nt + 1);
        d.leaf_ids = st.put(hb->leaf_ids, d.total_leaves);
        d.adj_depth = st.put(hb->adj_depth, d.total_leaves);
        if (!order_host.empty()) d.tree_order = st.put(order_host.data(), order_host.size());
        if (!fix_units.empty()) d.fix_units = st.put(fix_units.data(), fix_units.size());
        if (with_nodes) {
            d.node_off = st.put(hb->node_off, (size_t)nt + 1);
            d.rng_off = st.put(hb->rng_off, (size_t)d.n_nodes + 1);
            d.node_tree = st.put(node_tree.data(), d.n_nodes);
            d.ranges = st.put(hb->ranges, (size_t)2 * d.n_links);
        }
        e = st.finish(&d.ready);
    }
    d.slab = st.slab;
    if (e != hipSuccess) {
        qs_batch_free(c, b);
        return fail(c, e == hipErrorOutOfMemory ? QS_ERR_OOM : QS_ERR_HIP, std::string("qs_batch_upload: ") + hipGetErrorString(e));
    }
    *out = b;
    return QS_OK;
}

extern "C" uint32_t qs_batch_flags(const qs_device_batch *b) {
    if (!b) return 0;
    return (b->d.all_full ? QS_BATCH_ALL_TAXA : 0u) | (b->d.all_binary ? QS_BATCH_BINARY : 0u);
}

// corrections of the depth clamp for the trees in slots [slot_lo, slot_hi) of the batch whose largest id lies in [d_a, d_b), on
// stream s: after the count kernel that stored that range
static hipError_t clamp_fix_slots(qs_ctx *c, hipStream_t s, const qs_device_batch *b, uint32_t slot_lo, uint32_t slot_hi, uint32_t d_a, uint32_t d_b,
                                  int mode, uint32_t *wire) {
    const auto lo = std::lower_bound(b->fix_slot.begin(), b->fix_slot.end(), slot_lo), hi = std::lower_bound(lo, b->fix_slot.end(), slot_hi);
    if (lo == hi || d_a >= d_b) return hipSuccess;
    return launch_clamp_fix(s, b->d, b->d.fix_units + (lo - b->fix_slot.begin()), (uint32_t)(hi - lo), d_a, d_b,
                            c->rank_lo, c->table, (int)c->count_bits, mode, wire, c->dev_flags.get());
}
// ... and what they are modelled to cost: (tree, quartet) corrections over the whole table (an upper bound, see qs_batch_upload)
static uint64_t clamp_fix_work(const qs_device_batch *b, uint32_t slot_lo, uint32_t slot_hi) {
    const auto lo = std::lower_bound(b->fix_slot.begin(), b->fix_slot.end(), slot_lo), hi = std::lower_bound(lo, b->fix_slot.end(), slot_hi);
    return b->fix_work.empty() ? 0 : b->fix_work[hi - b->fix_slot.begin()] - b->fix_work[lo - b->fix_slot.begin()];
}

// the pair-depth panel holds `need` bytes (growing it waits for the launches that read the old one)
static int ensure_panel(qs_ctx *c, size_t need) {
    const hipError_t e = c->panel.reserve(need, &c->stream);   // exactly `need`: see run_launch
    if (e == hipErrorOutOfMemory) return fail(c, QS_ERR_OOM, "Insufficient memory! (pair-depth panel)");
    QS_HIP(c, e);   // (the wait for the stream)
    return QS_OK;
}

// The shard as a count kernel sees it: the 8x8 tiling of the byte-SWAR gather kernel, or (tiles16x8) the 16x8 tiling of the bit-sliced
// kernels with its launch order -- asked for here, so that a batch without a bit-sliced launch never builds it -- and, for a
// binary_full launch that is not fused (coop), the cooperative lists.
static int count_geometry(qs_ctx *c, bool tiles16x8, bool coop, CountGeometry &g) {
    g.n = c->n; g.d_lo = std::max(c->d_lo, 3u); g.d_hi = c->d_hi; g.rank_lo = c->rank_lo; g.n_dblk = c->n_dblk;
    if (!tiles16x8) { g.total_tiles = c->total_tiles; g.dprefix = c->dprefix.get(); g.cprefix = c->cprefix.get(); return QS_OK; }
    g.total_tiles = c->total_tiles3; g.dprefix = c->dprefix3.get(); g.cprefix = c->cprefix3.get();
    const int rc = tile_order(c, &g.perm);
    if (rc == QS_OK && coop) { g.perm_coop = c->perm_coop.get(); g.n_coop = c->n_coop; g.perm_rest = c->perm_rest.get(); g.n_rest = c->n_rest; }
    return rc;
}

// The 16x8 tiling `g` of the shard cut at d_mid into the tilings of [d_mid, d_hi) (hi: the leading d-blocks of g, so g's prefix
// array serves) and [d_lo, d_mid) (lo: d-blocks counted down from d_mid, a prefix array of its own), each with its launch order in
// the nesting of g's. Kept in the context for the d_mid they were built for.
static int split_geometry(qs_ctx *c, uint32_t d_mid, const CountGeometry &g, CountGeometry &hi, CountGeometry &lo, bool *rebuilt) {
    *rebuilt = false;
    qs_ctx::Split &S = c->split;
    const uint32_t d_start = g.d_lo;
    if (S.d_mid != d_mid || S.perm_of != g.perm) {
        // Everything goes onto the context's stream, behind the launches that may still read the old lists. The host waits only
        // where it rewrites what the device may still use: for the copies out of the host lists of an earlier split (the runtime may
        // read pageable memory after the call returns), and for the stream where a buffer has to grow. The first split of a context
        // finds neither.
        S.d_mid = 0;
        if (S.copied_valid) QS_HIP(c, hipEventSynchronize(S.copied.get()));
        S.copied_valid = false;
        S.n_dblk_hi = (g.d_hi - std::max(d_mid, d_start) + kDB - 1) / kDB;
        S.tiles_hi = c->h_dp3[S.n_dblk_hi];
        S.n_dblk_lo = d_mid > d_start ? (d_mid - d_start + kDB - 1) / kDB : 0;
        S.h_dp_lo.assign(S.n_dblk_lo + 1, 0);   // (host copies stay in the context: the asynchronous copies read them)
        for (uint32_t k = 0; k < S.n_dblk_lo; ++k) S.h_dp_lo[k + 1] = S.h_dp_lo[k] + c->h_cp3[d_mid - k * kDB - 1];
        S.tiles_lo = S.h_dp_lo[S.n_dblk_lo];
        if (S.dprefix_lo.reserve(S.h_dp_lo.size() * 4, &c->stream) != hipSuccess) return fail(c, QS_ERR_OOM, "hipMalloc split tiling");
        QS_HIP(c, hipMemcpyAsync(S.dprefix_lo.get(), S.h_dp_lo.data(), S.h_dp_lo.size() * 4, hipMemcpyHostToDevice, c->stream));
        if (g.perm) {
            // upper range: the shard's launch order without the tiles of the lower d-blocks -- its tiles are the ids below tiles_hi and
            // the nesting stays --, filtered on the device (12 M entries at 512 taxa: two short kernels instead of 25 ms of host work)
            if (S.perm_hi.reserve(std::max<size_t>(S.tiles_hi, 1) * 4, &c->stream) != hipSuccess ||
                S.filter_scratch.reserve(perm_filter_scratch_bytes(g.total_tiles), &c->stream) != hipSuccess)
                return fail(c, QS_ERR_OOM, "hipMalloc split tile order");
            QS_HIP(c, launch_perm_filter(c->stream, g.perm, g.total_tiles, S.tiles_hi, S.perm_hi.get(), S.tiles_hi, S.filter_scratch.get()));
            // lower range: a tiling of its own (d-blocks counted down from d_mid), a few per cent of the tiles: enumerated on the host
            std::string perr;
            const TilePermParams P_lo{c->tile_chunk, c->tile_cblock, c->tile_cgroup, d_mid, S.n_dblk_lo, S.tiles_lo};
            if (!build_tile_perm(P_lo, c->h_cp3, S.h_dp_lo, S.h_perm_lo, perr)) return fail(c, QS_ERR_STATE, perr);
            if (S.perm_lo.reserve(std::max<size_t>(S.h_perm_lo.size(), 1) * 4, &c->stream) != hipSuccess) return fail(c, QS_ERR_OOM, "hipMalloc split tile order");
            if (!S.h_perm_lo.empty()) QS_HIP(c, hipMemcpyAsync(S.perm_lo.get(), S.h_perm_lo.data(), S.h_perm_lo.size() * 4, hipMemcpyHostToDevice, c->stream));
        }
        QS_HIP(c, S.copied.ensure());
        QS_HIP(c, hipEventRecord(S.copied.get(), c->stream));
        S.copied_valid = true;
        S.perm_of = g.perm; S.d_mid = d_mid;
        *rebuilt = true;
    }
    hi = g; lo = g;
    hi.d_lo = std::max(d_mid, d_start); hi.n_dblk = S.n_dblk_hi; hi.total_tiles = S.tiles_hi; hi.perm = g.perm ? S.perm_hi.get() : nullptr;
    lo.d_hi = std::max(d_mid, d_start); lo.n_dblk = S.n_dblk_lo; lo.total_tiles = S.tiles_lo; lo.dprefix = S.dprefix_lo.get(); lo.perm = g.perm ? S.perm_lo.get() : nullptr;
    return QS_OK;
}

// One launch of a count kernel = 1..4 segments; a segment = one class's share of it: the slots [slot0, slot0 + trees) of the
// class-ordered batch in a panel of their own. (Classes = kernel mode x depth bits per TREE: qs_batch_upload.)
struct Seg {
    uint32_t slot0, trees;
    int mode;             // CountMode of the kernel instance
    bool part;            // panel elements carry a presence word
    uint32_t nw;          // bit-sliced: words per compact panel element
    uint32_t tpg;         // trees per group (= panel element along the tree axis): 32, byte-SWAR 16 / 8
    size_t group_bytes;   // bytes of one group: an element per pair
    uint32_t groups() const { return (trees + tpg - 1) / tpg; }
};
enum CountKernel { KERNEL_BITSLICE3, KERNEL_FUSED, KERNEL_SWAR };
struct Launch {
    CountKernel kernel;
    int bits;             // depth bits of the bit-sliced instance, panel bits (8 / 16) of the byte-SWAR kernel
    std::vector<Seg> segs;
};

static Seg bitslice_seg(const qs_ctx *c, uint32_t slot0, uint32_t trees, int mode, uint32_t depth_bits) {
    const bool part = mode == MODE_PARTIAL || mode == MODE_BINARY_PARTIAL;
    const uint32_t nw = std::max(depth_bits, 4u) + (part ? 1u : 0u);
    return Seg{slot0, trees, mode, part, nw, 32u, (size_t)binom2(c->n) * nw * 4};
}

// a class in the variant string: [mode.]bitslice_b<planes>x2[:trees] or [mode.]depth_u<panel bits>[:trees]; the wire format names the
// kernel family once, in front of its classes (family = false)
static std::string class_name(const Launch &L, const Seg &sg, bool family, const char *mode, bool with_trees) {
    std::string nm = L.kernel == KERNEL_SWAR ? "depth_u" + std::to_string(L.bits)
                                             : (family ? "bitslice_b" : "b") + std::to_string(std::max(L.bits, 4)) + "x2";
    if (mode) nm = std::string(mode) + "." + nm;
    if (with_trees) nm += ":" + std::to_string(sg.trees);
    return nm;
}

// QS_TUNE_STEP_ORDER: which order of the 32-tree step a class of count_bitslice3_kernel runs. 1 = prefetch everywhere, 2 = late loads
// wherever the instance exists (bitslice3_late_waves), 0 = automatic: late loads for exactly the instances listed here, prefetch for all
// others. A row = (mode, depth bits, cell bits) MEASURED faster late than prefetch on an MI355X, with the workload and its ms per step,
// prefetch -> late (profiles/r13_step_order.md; the bar: every late run below every prefetch run and the mean difference at least three
// times the spread of the prefetch runs). The wire format counts into 32-bit words: it follows the u32 rows.
struct LateAuto { int mode, bits, cell_bits; const char *measured; };
static constexpr LateAuto kLateAuto[] = {
    {MODE_BINARY_FULL, 4, 32, "512 taxa x 10000 trees: 296.43 / 297.51 / 297.01 -> 288.29 / 288.91 / 289.77 (-2.7 %, 7.4 spreads); "
                              "128 x 1000: 0.1675 / 0.1678 / 0.1680 -> 0.1592 / 0.1600 / 0.1601 (-4.8 %); "
                              "256 x 12500: 25.46 / 25.54 / 25.41 -> 24.59 / 24.72 / 24.62 (-3.2 %, 6.5 spreads)"},
    {MODE_BINARY_FULL, 4, 16, "1024 taxa x 5000 trees, shard 0 of 8: 313.85 / 314.56 / 314.14 -> 309.75 / 309.56 / 310.00 (-1.4 %, 6.1 spreads)"},
    // not listed: 5 bits (u32, u16) -- compiled and tested, measured only as the smaller class of the --nni batch (with the 4-bit class:
    // 297.37 / 296.90 / 294.74 -> 286.79 / 286.99 / 284.12), not on a batch of its own
};
// waves per SIMD of the late instance the class takes under `knob`; 0 = it takes the prefetch instance
static int step_order_late_waves(uint32_t knob, int mode, int depth_bits, int cell_bits) {
    const int w = knob == 1 ? 0 : bitslice3_late_waves(mode, depth_bits);
    if (!w || knob == 2) return w;
    for (const LateAuto &e : kLateAuto)
        if (e.mode == mode && e.bits == std::max(depth_bits, 4) && e.cell_bits == cell_bits) return w;
    return 0;
}

// QS_TUNE_STAGE_SIX: the six-wave instance (bitslice3_six_waves; the dma order). 2 = wherever it exists, 1 = never, 0 = automatic: where
// QS_TUNE_STEP_ORDER is automatic too, exactly the instances listed here; an explicit step order is obeyed. A row as in kLateAuto, measured
// against the five-wave late instance the class took before (profiles/r15_stage_dma.md; the same bar).
static constexpr LateAuto kSixAuto[] = {
    {MODE_BINARY_FULL, 4, 32, "512 taxa x 10000 trees, late at five waves -> dma at six: 282.58 / 283.13 / 283.32 -> 278.36 / 279.18 / 278.92 (-1.5 %, 5.6 spreads); "
                              "on a second box 292.68 / 292.91 / 293.96 -> 290.04 / 290.05 / 290.38 (-1.0 %, 2.4 spreads: every run below, the bar missed there); "
                              "128 x 1000: 0.1596 / 0.1603 / 0.1586 -> 0.1577 / 0.1584 / 0.1579 (-0.9 %); 256 x 12500: 24.35 / 24.39 / 24.55 -> 24.03 / 24.02 / 24.05 (-1.6 %)"},
    {MODE_BINARY_FULL, 4, 16, "1024 taxa x 5000 trees, shard 0 of 8: 313.49 / 312.71 -> 306.49 / 306.90 (-2.0 %)"},
};
// waves per SIMD of the six-wave instance the class takes; 0 = it takes what step_order_late_waves says
static int stage_six_waves(uint32_t six_knob, uint32_t order_knob, int mode, int depth_bits, int cell_bits) {
    const int w = six_knob == 1 ? 0 : bitslice3_six_waves(mode, depth_bits);
    if (!w || six_knob == 2) return w;
    if (order_knob != 0) return 0;
    for (const LateAuto &e : kSixAuto)
        if (e.mode == mode && e.bits == std::max(depth_bits, 4) && e.cell_bits == cell_bits) return w;
    return 0;
}

// Enqueue one launch, slice by slice (slice_groups over the concatenated group list [0, g_total) of its segments; slice [g0, g1)
// takes from every segment the groups that fall into it): panel build(s), count kernel, depth-clamp corrections, and with
// `timed` an event after each of the three. Into the table, or (wire != NULL) the two-cell wire words.
static int run_launch(qs_ctx *c, const qs_device_batch *b, const Launch &L, uint32_t *wire, bool timed, bool overwrite, bool &first) {
    const DeviceBatch &d = b->d;
    const bool bitsliced = L.kernel != KERNEL_SWAR;
    const int mode0 = L.segs[0].mode;
    CountGeometry g;
    int rc = count_geometry(c, bitsliced, L.kernel == KERNEL_BITSLICE3 && mode0 == MODE_BINARY_FULL, g);
    if (rc != QS_OK) return rc;
    uint32_t g_total = 0;
    size_t group_bytes = 0;
    for (const Seg &sg : L.segs) { g_total += sg.groups(); group_bytes = std::max(group_bytes, sg.group_bytes); }
    const uint32_t per_slice = slice_groups(c, group_bytes, g_total, g.perm != nullptr);
    // The segments of a slice lie one behind the other, each at a 256-byte boundary: only the gaps BETWEEN them need room. A launch
    // of one segment so asks for per_slice groups exactly -- what qs_prepare has allocated ahead for the common 5-plane class; a
    // byte more would make the CLI's first count wait for the stream, free that panel and allocate another.
    rc = ensure_panel(c, (size_t)per_slice * group_bytes + 256 * (L.segs.size() - 1));
    if (rc != QS_OK) return rc;
    // Split slices (QS_TUNE_FIX_OVERLAP): one d_mid for the launch, planned for a slice's groups and its share of the launch's
    // corrections. Not with the byte-SWAR kernel (no corrections), the cooperative lists, or where the plan says a split does not pay.
    uint32_t d_mid = 0;
    CountGeometry g_hi = g, g_lo = g;
    if (bitsliced && d.n_fix && c->tune_fix_overlap && !g.perm_coop) {
        uint64_t work = 0;
        for (const Seg &sg : L.segs) work += clamp_fix_work(b, sg.slot0, sg.slot0 + sg.trees);
        const uint32_t grp = std::min(per_slice, g_total), n_slices = (g_total + per_slice - 1) / per_slice;
        work = (work + n_slices - 1) / std::max(n_slices, 1u);
        if (c->tune_fix_split_at) d_mid = (work && c->tune_fix_split_at > c->d_lo && c->tune_fix_split_at < c->d_hi) ? c->tune_fix_split_at : 0;
        else {
            int gen = 0;
            for (const Seg &sg : L.segs) gen = gen || sg.mode == MODE_GENERAL_FULL || sg.mode == MODE_PARTIAL;
            const int pick = qs_fix_overlap_plan(c->n, c->d_lo, c->d_hi, c->count_bits, gen ? MODE_GENERAL_FULL : MODE_BINARY_FULL, (uint32_t)L.bits, grp, work, c->split.d_mid, nullptr);
            d_mid = pick > 0 ? (uint32_t)pick : 0;
        }
        if (d_mid) {
            QS_HIP(c, c->fix_stream.ensure());
            QS_HIP(c, c->fix_go.ensure());
            QS_HIP(c, c->fix_done.ensure());
            bool rebuilt = false;
            rc = split_geometry(c, d_mid, g, g_hi, g_lo, &rebuilt);
            if (rc != QS_OK) return rc;
            if (timed && rebuilt) QS_HIP(c, mark(c, 3));   // (the filter kernels and copies of a new split: not the next panel build's time)
        }
    }
    for (uint32_t g0 = 0; g0 < g_total; g0 += per_slice) {
        const uint32_t g1 = std::min(g_total, g0 + per_slice);
        // per CountMode, as the fused kernel takes them (a mode without trees in this slice: 0 groups)
        const void *seg_panel[4] = {nullptr, nullptr, nullptr, nullptr};
        uint32_t seg_groups[4] = {0, 0, 0, 0}, seg_trees[4] = {0, 0, 0, 0}, seg_slot[4] = {0, 0, 0, 0};
        size_t off = 0;
        uint32_t base = 0;
        for (const Seg &sg : L.segs) {
            const uint32_t a = std::max(g0, base), e_ = std::min(g1, base + sg.groups());
            base += sg.groups();
            if (a >= e_) continue;
            const uint32_t ga = a - (base - sg.groups()), nch = e_ - a;
            const uint32_t t0 = ga * sg.tpg, nt = std::min(nch * sg.tpg, sg.trees - t0);
            DeviceBatch sub = d;
            sub.slot0 = sg.slot0 + t0;        // slots [slot0, slot0 + nt) of the class-ordered batch
            sub.n_trees = nt;
            void *pp = (char *)c->panel.get() + off;
            if (bitsliced) QS_HIP(c, launch_build_bitpanel(c->stream, sub, c->n, sg.part, pp, nch, sg.nw, c->tune_panel_kernel == 1));
            else QS_HIP(c, launch_build_panel(c->stream, sub, c->n, L.bits, sg.part, pp, nch));
            seg_panel[sg.mode] = pp; seg_groups[sg.mode] = nch; seg_trees[sg.mode] = nt; seg_slot[sg.mode] = sub.slot0;
            off += ((size_t)nch * sg.group_bytes + 255) & ~(size_t)255;
        }
        if (timed) QS_HIP(c, mark(c, 0));
        const bool ow = overwrite && first;
        // a count launch over the tiling gg (the whole shard, or one d-range of a split slice)
        auto count_range = [&](const CountGeometry &gg) -> hipError_t {
            if (L.kernel == KERNEL_FUSED)
                return launch_count_bitslice3_fused(c->stream, gg, seg_panel, seg_groups, seg_trees, L.bits, c->table, (int)c->count_bits, c->dev_flags.get(), ow);
            if (L.kernel == KERNEL_BITSLICE3) {
                // (the cooperative lists send only the rest tiles through this kernel: they keep the prefetch order)
                const int cell_bits = wire ? 32 : (int)c->count_bits;
                const int sw = gg.perm_coop ? 0 : stage_six_waves(c->tune_stage_six, c->tune_step_order, mode0, L.bits, cell_bits);
                const int lw = (gg.perm_coop || sw) ? 0 : step_order_late_waves(c->tune_step_order, mode0, L.bits, cell_bits);
                if (sw) c->last_six_waves = (uint32_t)sw;
                if (lw) c->last_late_waves = (uint32_t)lw;
                return launch_count_bitslice3(c->stream, gg, seg_panel[mode0], L.bits, mode0, seg_groups[mode0], seg_trees[mode0], wire ? nullptr : c->table,
                                              cell_bits, c->dev_flags.get(), ow, wire, sw ? 2 : lw ? 1 : 0);
            }
            return launch_count_gather(c->stream, gg, seg_panel[mode0], L.bits, mode0, seg_groups[mode0], seg_trees[mode0], c->table, (int)c->count_bits, c->dev_flags.get(), ow);
        };
        // the corrections of the slice's trees in the d-range [d_a, d_b), on stream s
        auto fix_range = [&](hipStream_t s, uint32_t d_a, uint32_t d_b) -> hipError_t {
            for (int mo = 0; mo < 4; ++mo) {   // (the rule of the correction depends on the mode: a tied quartet sits in the third cell of a binary tree)
                const hipError_t e = seg_groups[mo] ? clamp_fix_slots(c, s, b, seg_slot[mo], seg_slot[mo] + seg_trees[mo], d_a, d_b, mo, wire) : hipSuccess;
                if (e != hipSuccess) return e;
            }
            return hipSuccess;
        };
        bool has_fix = false;   // (never the byte-SWAR kernel: its panel holds the trees' own depths)
        for (int mo = 0; mo < 4 && bitsliced && d.n_fix; ++mo) has_fix = has_fix || (seg_groups[mo] && clamp_fix_work(b, seg_slot[mo], seg_slot[mo] + seg_trees[mo]) > 0);
        // (with the first overwriting launch enqueued the old contents are gone: a later refusal must not leave their count behind)
        auto overwritten = [&] { if (ow) { if (wire) c->wire_trees = 0; else { c->trees_counted = 0; c->collapse_max_count = 0; } } };
        first = false;
        if (has_fix && d_mid) {
            // THE ORDERING RULE of a split slice. A correction must land after the store of the cell it corrects, and a cell belongs to
            // exactly one of the two d-ranges (a d-range is one contiguous piece of the table), so:
            //   main stream:        count [d_mid, d_hi) -> fix_go -> count [d_lo, d_mid) -> corrections of [d_lo, d_mid) -> wait for fix_done
            //   correction stream:  wait for fix_go -> corrections of [d_mid, d_hi) -> fix_done
            // Kernels in flight together (the lower count launch and the upper corrections) work on disjoint ranges; everything later on
            // the main stream -- the next slice, the next class, whoever reads the table -- comes after both. Whatever fails once the
            // correction stream has work, the main stream still waits for it before the error is returned.
            const hipStream_t fs = c->fix_stream.get();
            QS_HIP(c, count_range(g_hi));
            overwritten();
            const uint32_t ev_hi = c->ev_used;
            if (timed) QS_HIP(c, mark(c, 1));
            QS_HIP(c, hipEventRecord(c->fix_go.get(), c->stream));
            QS_HIP(c, hipStreamWaitEvent(fs, c->fix_go.get(), 0));
            hipError_t e = fix_range(fs, g_hi.d_lo, g_hi.d_hi);
            if (e == hipSuccess && timed) e = mark(c, 2, &fs, ev_hi);
            const hipError_t e_done = hipEventRecord(c->fix_done.get(), fs);
            uint32_t ev_lo = 0;
            if (e == hipSuccess) e = count_range(g_lo);
            if (e == hipSuccess) { ev_lo = c->ev_used; if (timed) e = mark(c, 4, nullptr, ev_hi); }
            if (e == hipSuccess) e = fix_range(c->stream, g_lo.d_lo, g_lo.d_hi);
            if (e == hipSuccess && timed) e = mark(c, 2, nullptr, ev_lo);
            // the join: behind fix_done, or -- if that event could not be recorded -- once the correction stream has drained
            const hipError_t e_join = e_done == hipSuccess ? hipStreamWaitEvent(c->stream, c->fix_done.get(), 0) : hipStreamSynchronize(fs);
            QS_HIP(c, e);
            QS_HIP(c, e_done);
            QS_HIP(c, e_join);
            if (timed) QS_HIP(c, mark(c, 3));
            c->last_split = d_mid; ++c->last_splits;
        } else {
            QS_HIP(c, count_range(g));
            overwritten();
            if (timed) QS_HIP(c, mark(c, 1));
            if (has_fix) {
                QS_HIP(c, fix_range(c->stream, g.d_lo, g.d_hi));
                if (timed) QS_HIP(c, mark(c, 2));
            }
        }
    }
    return QS_OK;
}

// QS_COUNT_WIRE16X2: count a binary_full batch straight into the attached wire buffer (one word per tuple), class by class
static int count_batch_wire(qs_ctx *c, const qs_device_batch *b, uint32_t algo) {
    const DeviceBatch &d = b->d;
    if (!c->wire_out) return fail(c, QS_ERR_STATE, "QS_COUNT_WIRE16X2: no wire buffer (qs_wire_attach first)");
    const bool overwrite = (algo & QS_COUNT_OVERWRITE) != 0;
    const uint32_t base_algo = algo & 0xFFu;
    if (base_algo != QS_ALGO_AUTO && base_algo != QS_ALGO_GATHER) return fail(c, QS_ERR_ARG, "QS_COUNT_WIRE16X2 needs the gather algorithm");
    const bool timed = (algo & QS_COUNT_TIMED) != 0;
    QS_HIP(c, hipSetDevice(c->device));
    if (d.n_trees == 0) {
        if (overwrite) { QS_HIP(c, hipMemsetAsync(c->wire_out, 0, c->n_tuples * 4, c->stream)); c->wire_trees = 0; }
        return QS_OK;
    }
    if (!(d.all_full && d.all_binary))
        return fail(c, QS_ERR_STATE, "QS_COUNT_WIRE16X2: the batch is not made of binary trees that hold all taxa (count into the table and use qs_table_pack16)");
    if (d.ready) QS_HIP(c, hipStreamWaitEvent(c->stream, d.ready, 0));
    if ((overwrite ? 0 : c->wire_trees) + d.n_trees > 0xFFFFull)
        return fail(c, QS_ERR_OVERFLOW, "QS_COUNT_WIRE16X2: more than 65535 trees do not fit 16-bit cells");
    if (d.class_bits[d.n_classes - 1] > 10) return fail(c, QS_ERR_UNSUPPORTED, "QS_COUNT_WIRE16X2: tree depth needs more than 10 bits; count into the table instead");
    { const uint32_t *order; int rc_o = tile_order(c, &order); if (rc_o != QS_OK) return rc_o; }   // (a failure here leaves the last call's events as they were)
    c->ev_used = 0; c->last_split = c->last_splits = 0; c->last_late_waves = c->last_six_waves = 0;
    if (timed) QS_HIP(c, mark(c, 0));
    bool first = true;
    c->variant = "gather/binary_full/bitslice_";
    for (uint32_t k = 0; k < d.n_classes; ++k) {
        const uint32_t s_lo = k ? d.class_end[k - 1] : 0;
        const Launch L{KERNEL_BITSLICE3, (int)d.class_bits[k], {bitslice_seg(c, s_lo, d.class_end[k] - s_lo, MODE_BINARY_FULL, d.class_bits[k])}};
        int rc = run_launch(c, b, L, c->wire_out, timed, overwrite, first);
        if (rc != QS_OK) return rc;
        c->variant += (k ? "+" : "") + class_name(L, L.segs[0], false, nullptr, d.n_classes > 1);
    }
    c->variant += "/wire_u16x2";
    if (c->last_six_waves) c->variant += std::string("/") + bitslice3_six_name() + std::to_string(c->last_six_waves);
    if (c->last_late_waves) c->variant += "/late" + std::to_string(c->last_late_waves);
    if (d.n_fix) c->variant += "/clamp:" + std::to_string(d.clamped_trees);
    if (c->last_splits) c->variant += "/overlap:" + std::to_string(c->last_split);
    if (c->n_coop) c->variant += "/coop4";
    c->wire_trees = (overwrite ? 0 : c->wire_trees) + d.n_trees;
    c->last_timed = timed;
    return QS_OK;
}

extern "C" int qs_count_batch(qs_ctx *c, const qs_device_batch *b, uint32_t algo) {
    if (c) c->log_valid = false;   // (the table / view / tuning may change: a logged pass 1 no longer describes it)
    if (!c || !b) return fail(c, QS_ERR_ARG, "qs_count_batch: NULL argument");
    if (algo & QS_COUNT_WIRE16X2) return count_batch_wire(c, b, algo);
    if (!c->table) return fail(c, QS_ERR_STATE, "qs_count_batch: no table (qs_table_alloc / qs_table_attach first)");
    const DeviceBatch &d = b->d;
    QS_HIP(c, hipSetDevice(c->device));
    if (d.n_trees == 0) {
        if (algo & QS_COUNT_OVERWRITE) { // "discard the previous contents" holds for an empty batch too
            QS_HIP(c, hipMemsetAsync(c->table, 0, c->n_tuples * 3 * (c->count_bits / 8), c->stream));
            c->trees_counted = 0;
            c->collapse_max_count = 0;
        }
        c->last_timed = false;
        return QS_OK;
    }
    if (c->count_bits == 16 && ((algo & QS_COUNT_OVERWRITE) ? 0 : c->trees_counted) + d.n_trees > 0xFFFFull)
        return fail(c, QS_ERR_OVERFLOW, "qs_count_batch: more than 65535 trees need count_bits = 32");
    if (d.ready) QS_HIP(c, hipStreamWaitEvent(c->stream, d.ready, 0));   // the batch's copies run on the copy stream
    const bool overwrite = (algo & QS_COUNT_OVERWRITE) != 0;
    const bool timed = (algo & QS_COUNT_TIMED) != 0;
    algo &= ~(QS_COUNT_OVERWRITE | QS_COUNT_TIMED);
    if (algo == QS_ALGO_AUTO) algo = QS_ALGO_GATHER;
    if (overwrite && algo != QS_ALGO_GATHER) return fail(c, QS_ERR_ARG, "qs_count_batch: QS_COUNT_OVERWRITE needs the gather algorithm");
    // (a call refused before its first launch leaves table and count as they were; run_launch resets trees_counted with the first
    // overwriting launch it enqueues, so that a refusal after it -- a later class too deep, a panel that cannot grow -- leaves no stale count)
    c->ev_used = 0; c->last_split = c->last_splits = 0; c->last_late_waves = c->last_six_waves = 0;
    if (timed) QS_HIP(c, mark(c, 0));
    if (algo == QS_ALGO_GATHER) {
        static const char *mode_names[4] = {"binary_full", "general_full", "partial", "binary_partial"};
        // This function only chooses the launches (run_launch enqueues them). With QS_IMPL_SWAR the whole batch is one class of the
        // byte-SWAR kernel, in the mode the batch as a whole needs.
        const uint32_t top_bits = 10u;
        const bool all_swar = c->tune_gather_impl == QS_IMPL_SWAR;
        if (c->tune_gather_impl == QS_IMPL_BITSLICE)
            for (uint32_t k = 0; k < d.n_classes; ++k)
                if (d.class_bits[k] > top_bits) return fail(c, QS_ERR_UNSUPPORTED, "QS_IMPL_BITSLICE: tree depth needs more than 10 bits");
        const uint32_t n_cls = all_swar ? 1u : d.n_classes;
        bool first = true, mixed = false;
        for (uint32_t k = 1; k < n_cls; ++k) mixed = mixed || d.class_mode[k] != d.class_mode[0];
        const int batch_mode = !d.all_full ? MODE_PARTIAL : (d.all_binary ? MODE_BINARY_FULL : MODE_GENERAL_FULL);
        std::string names;
        bool any_coop = false;
        // several classes: "a:trees+b:trees", classes of several modes: "mode.a:trees+..."
        auto run_and_name = [&](const Launch &L) {
            const int rc = run_launch(c, b, L, nullptr, timed, overwrite, first);
            for (const Seg &sg : L.segs)
                if (rc == QS_OK) names += (names.empty() ? "" : "+") + class_name(L, sg, true, mixed ? mode_names[sg.mode] : nullptr, n_cls > 1);
            return rc;
        };
        auto slot_lo = [&](uint32_t k) { return k ? d.class_end[k - 1] : 0u; };
        // ---- fused launches (QS_TUNE_FUSE_CLASSES): the bit-sliced classes that share their depth bits run as segments of ONE launch
        // of count_bitslice3_fused_kernel -- one pass over the table, one wave prologue / epilogue, whatever the mix of modes ----
        std::vector<bool> done(n_cls, false);
        uint32_t fused_launch_groups = 0;
        for (uint32_t bb = 4; c->tune_fuse && !all_swar && bb <= (uint32_t)kFusedMaxBits; ++bb) {
            std::vector<uint32_t> ks;
            for (uint32_t k = 0; k < n_cls; ++k) if (std::max(d.class_bits[k], 4u) == bb) ks.push_back(k);
            // a lone binary_partial class at 4 or 5 bits takes the fused binary kernel too (with an empty binary_full segment): under the one
            // dispatch it needs 123 VGPRs and spills nothing at 4 waves per SIMD, where the one-class instance is held to 128 with 6-24
            // spilled: 512 taxa x 1500 trees with 10 % of the taxa dropped 64.95 -> 63.7 ms (profiles/r06_experiments.md 3)
            const bool lone_bp4 = ks.size() == 1 && bb <= 5 && d.class_mode[ks[0]] == MODE_BINARY_PARTIAL;   // (5 bits: 4 waves instead of the one-class instance's 3)
            if (ks.size() < 2 && !lone_bp4) continue;
            Launch L{KERNEL_FUSED, (int)bb, {}};
            for (uint32_t k : ks) { L.segs.push_back(bitslice_seg(c, slot_lo(k), d.class_end[k] - slot_lo(k), (int)d.class_mode[k], bb)); done[k] = true; }
            const int rc = run_and_name(L);
            if (rc != QS_OK) return rc;
            ++fused_launch_groups;
        }
        // ---- the other classes one by one: count_bitslice3_kernel on the compact panel, beyond its 10 depth bits the byte-SWAR kernel ----
        for (uint32_t k = 0; k < n_cls; ++k) {
            if (done[k]) continue;
            const uint32_t s_lo = all_swar ? 0u : slot_lo(k), trees = (all_swar ? d.n_trees : d.class_end[k]) - s_lo;
            const uint32_t depth_bits = all_swar ? 11u : d.class_bits[k];   // 11 = beyond the bit-sliced instances
            int mode = all_swar ? batch_mode : (int)d.class_mode[k];
            Launch L{KERNEL_BITSLICE3, (int)depth_bits, {}};
            if (depth_bits <= top_bits) L.segs.push_back(bitslice_seg(c, s_lo, trees, mode, depth_bits));
            else {
                // the byte-SWAR kernel has no binary_partial instance: such trees are exact under its partial mode
                if (mode == MODE_BINARY_PARTIAL) mode = MODE_PARTIAL;
                const bool part = mode == MODE_PARTIAL;
                const uint32_t cls_max_depth = all_swar ? d.max_depth : d.class_max_depth[k];
                if (cls_max_depth <= (part ? kMaxDepthU8Partial : kMaxDepthU8Full)) L.bits = 8;
                else if (cls_max_depth <= (part ? kMaxDepthU16Partial : kMaxDepthU16Full)) L.bits = 16;
                else return fail(c, QS_ERR_UNSUPPORTED, "qs_count_batch: tree depth " + std::to_string(cls_max_depth) + " exceeds the panel range; re-root the tree at its centre");
                L.kernel = KERNEL_SWAR;
                L.segs.push_back(Seg{s_lo, trees, mode, part, 0u, 16u / (uint32_t)(L.bits / 8), (size_t)binom2(c->n) * 16});   // 16 bytes per (pair, group)
            }
            const int rc = run_and_name(L);
            if (rc != QS_OK) return rc;
            // tiles with two a-blocks of binary_full classes: count_bitslice4_kernel (it carries at most 7 planes)
            any_coop = any_coop || (L.kernel == KERNEL_BITSLICE3 && mode == MODE_BINARY_FULL && c->n_coop && depth_bits <= 7);
        }
        const int one_mode = all_swar ? batch_mode : (int)d.class_mode[0];
        c->variant = std::string("gather/") + (mixed ? "mixed" : mode_names[(!all_swar && d.class_bits[0] > top_bits && one_mode == MODE_BINARY_PARTIAL) ? (int)MODE_PARTIAL : one_mode]) + "/" + names + "/count_u" + std::to_string(c->count_bits);
        if (fused_launch_groups) c->variant += "/fused:" + std::to_string(fused_launch_groups);   // depth-bits groups whose classes shared a launch (count_bitslice3_fused_kernel)
        if (any_coop) c->variant += "/coop4";
        if (c->last_six_waves) c->variant += std::string("/") + bitslice3_six_name() + std::to_string(c->last_six_waves);   // ... the six-wave instance (QS_TUNE_STAGE_SIX)
        if (c->last_late_waves) c->variant += "/late" + std::to_string(c->last_late_waves);   // a binary_full class ran the late-load instance (QS_TUNE_STEP_ORDER) at that many waves per SIMD
        if (!all_swar && d.n_fix) c->variant += "/clamp:" + std::to_string(d.clamped_trees);   // trees counted below their own depth bits + clamp_fix_kernel
        if (c->last_splits) c->variant += "/overlap:" + std::to_string(c->last_split);           // slices split at that largest id: corrections beside the lower count launch
    } else if (algo == QS_ALGO_SCATTER) {
        if (!d.node_off) return fail(c, QS_ERR_ARG, "qs_count_batch: QS_ALGO_SCATTER needs node_off/rng_off/ranges in the batch");
        if (c->n > 4096) return fail(c, QS_ERR_UNSUPPORTED, "scatter: n too large");
        QS_HIP(c, launch_count_scatter(c->stream, d, c->n, c->d_lo, c->d_hi, c->rank_lo, c->table, (int)c->count_bits, c->dev_flags.get()));
        if (timed) QS_HIP(c, mark(c, 1));
        c->variant = std::string("scatter/atomic/count_u") + std::to_string(c->count_bits);
    } else {
        return fail(c, QS_ERR_ARG, "qs_count_batch: unknown algo");
    }
    c->last_timed = timed;
    c->trees_counted = (overwrite ? 0 : c->trees_counted) + d.n_trees;
    // (a collapsed table's bound: gone with the contents, else every cell may grow by the trees counted on top)
    c->collapse_max_count = overwrite || !c->collapse_max_count ? 0 : (c->collapse_max_count > UINT64_MAX - d.n_trees ? UINT64_MAX : c->collapse_max_count + d.n_trees);
    return QS_OK;
}

extern "C" int qs_count_trees(qs_ctx *c, const qs_tree_batch *batch, uint32_t algo) {
    qs_device_batch *b = nullptr;
    int rc = qs_batch_upload(c, batch, &b);
    if (rc != QS_OK) return rc;
    rc = qs_count_batch(c, b, algo);
    int rc2 = qs_sync(c);
    qs_batch_free(c, b);
    return rc != QS_OK ? rc : rc2;
}

extern "C" int qs_last_count_ms(qs_ctx *c, float out_ms[3]) {
    if (!c || !c->last_timed || c->ev_used < 2) return fail(c, QS_ERR_STATE, "qs_last_count_ms: the last qs_count_batch did not carry QS_COUNT_TIMED");
    QS_HIP(c, hipEventSynchronize(c->evs[c->ev_used - 1]));
    out_ms[0] = out_ms[1] = 0.f;
    for (uint32_t i = 1; i < c->ev_used; ++i) {
        float ms = 0.f;
        if (c->ev_kind[i] == 3) continue;      // (a wait for the correction stream or the set-up of a new split, not a kernel of the step)
        QS_HIP(c, hipEventElapsedTime(&ms, c->evs[c->ev_from[i]], c->evs[i]));
        out_ms[c->ev_kind[i] ? 1 : 0] += ms;   // (the depth-clamp corrections count as count-kernel time: qs_last_count_fix_ms has their share; those of a
                                               // split slice's upper range run beside its lower count launch, so the kernels may sum to more than [2])
    }
    QS_HIP(c, hipEventElapsedTime(&out_ms[2], c->evs[0], c->evs[c->ev_used - 1]));
    return QS_OK;
}

extern "C" int qs_last_count_launches(const qs_ctx *c) {
    if (!c || !c->last_timed) return 0;
    int k = 0;
    for (uint32_t i = 1; i < c->ev_used; ++i) k += c->ev_kind[i] == 1 ? 1 : 0;
    return k;
}

extern "C" float qs_last_count_fix_ms(qs_ctx *c) {
    if (!c || !c->last_timed || c->ev_used < 2) return 0.f;
    if (hipEventSynchronize(c->evs[c->ev_used - 1]) != hipSuccess) return 0.f;
    float sum = 0.f;
    for (uint32_t i = 1; i < c->ev_used; ++i) {
        float ms = 0.f;
        if (c->ev_kind[i] == 2 && hipEventElapsedTime(&ms, c->evs[c->ev_from[i]], c->evs[i]) == hipSuccess) sum += ms;
    }
    return sum;
}

extern "C" int qs_last_count_events(qs_ctx *c, float *ms, uint8_t *kind, int cap) {
    if (!c || !c->last_timed || c->ev_used < 2) return 0;
    if (hipEventSynchronize(c->evs[c->ev_used - 1]) != hipSuccess) return 0;
    int k = 0;
    for (uint32_t i = 1; i < c->ev_used && k < cap; ++i) {
        if (c->ev_kind[i] == 3) continue;   // (a wait for the correction stream or the set-up of a new split, not a kernel of the step)
        float t = 0.f;
        (void)hipEventElapsedTime(&t, c->evs[c->ev_from[i]], c->evs[i]);
        if (ms) ms[k] = t;
        if (kind) kind[k] = c->ev_kind[i] == 4 ? 1 : c->ev_kind[i];   // (the second count launch of a split slice is a count kernel)
        ++k;
    }
    return k;
}

extern "C" int qs_batch_clamp_info(const qs_device_batch *b, uint64_t out[3]) {
    if (!b || !out) return QS_ERR_ARG;
    out[0] = b->d.clamped_trees; out[1] = b->d.fix_quartets; out[2] = b->d.n_fix;
    return QS_OK;
}

extern "C" const char *qs_last_count_variant(const qs_ctx *c) { return c ? c->variant.c_str() : ""; }

extern "C" int qs_last_count_split(const qs_ctx *c, uint32_t *n_slices) {
    if (n_slices) *n_slices = c ? c->last_splits : 0;
    return c ? (int)c->last_split : 0;
}
