// qs_abi.hip -- the C-ABI declared in include/quartetscores_hip.h: context, tuning, table and wire calls, lookups. The count step is
// in qs_abi_count.hip, scoring in qs_abi_score.hip, the other table queries in qs_abi_query.hip, host-only planning in qs_plan.hip, the
// issue probe in qs_probe.hip; qs_ctx.hpp holds what they share.
//
// All of these are host-side orchestration only: validation of the flattened trees, device memory, kernel
// dispatch, and the O(#node pairs) finalisation of the scores. All O(m*C(n,4)) and O(C(n,4))
// work runs in the HIP kernels of qs_count.hip / qs_score.hip. There is no CPU fallback.
#include "qs_ctx.hpp"
#include "qs_plan.hpp"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <future>
#include <string>
#include <thread>
#include <vector>

using namespace qs;

thread_local std::string qs::g_create_err;   // per thread: qs_create of several contexts may run concurrently (multi_gpu.hpp)

int qs::fail(qs_ctx *c, int code, const std::string &msg) {
    if (c) c->err = msg; else g_create_err = msg;
    return code;
}

extern "C" const char *qs_version(void) { return "quartetscores_amd 0.1.0 (gfx950)"; }

extern "C" const char *qs_last_error(const qs_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }

extern "C" int qs_set_tuning(qs_ctx *c, uint32_t key, uint64_t value) {
    if (c) c->log_valid = false;   // (the table / view / tuning may change: a logged pass 1 no longer describes it)
    if (!c) return QS_ERR_ARG;
    switch (key) {
        case QS_TUNE_SCORE_CAND_SLOTS:
            if (value < 1 || value > (uint64_t)kCand) return fail(c, QS_ERR_ARG, "qs_set_tuning: QS_TUNE_SCORE_CAND_SLOTS takes 1..8");
            c->tune_cand_slots = (uint32_t)value; return QS_OK;
        case QS_TUNE_SCORE_KERNEL:
            if (value > 1) return fail(c, QS_ERR_ARG, "qs_set_tuning: QS_TUNE_SCORE_KERNEL takes 0 (bundle kernel) or 1 (scan kernel)");
            c->tune_score_kernel = (int)value; return QS_OK;
        case QS_TUNE_SCORE_TOL_EXP:
            if (value < 1 || value > 15) return fail(c, QS_ERR_ARG, "qs_set_tuning: QS_TUNE_SCORE_TOL_EXP takes 1..15 (tolerance 10^-value)");
            c->tune_score_tol = std::pow(10.0, -(double)value); return QS_OK;
        case QS_TUNE_TILE_ORDER:
            if (int rc = drop_tile_order(c)) return rc;
            c->tile_chunk = (uint32_t)(value & 0xFFFF); c->tile_cblock = (uint32_t)((value >> 16) & 0xFFFF); c->tile_cgroup = (uint32_t)((value >> 32) & 0xFF);
            return QS_OK;
        case QS_TUNE_PANEL_SLICE_BYTES: c->tune_slice_bytes = value; return QS_OK;
        case QS_TUNE_TABLE_TREES: c->table_trees_hint = value; return QS_OK;
        case QS_TUNE_SCORE_SAMPLE: {
            const uint64_t S = value & 0xFFFFu;
            if (value >> 17 || (value && (S < 2 || (S & (S - 1))))) return fail(c, QS_ERR_ARG, "qs_set_tuning: QS_TUNE_SCORE_SAMPLE takes 0 or a power of two in [2, 32768], optionally | 65536 (whole rounds)");
            c->tune_score_sample = (uint32_t)value; return QS_OK;
        }
        case QS_TUNE_CLASS_MIN_TREES: c->tune_class_min = (uint32_t)std::min<uint64_t>(value, 0xFFFFFFFFull); return QS_OK;
        case QS_TUNE_DEPTH_CLAMP: c->tune_clamp_ppm = (uint32_t)std::min<uint64_t>(value, 1000000ull); return QS_OK;
        case QS_TUNE_FUSE_CLASSES: c->tune_fuse = value ? 1u : 0u; return QS_OK;
        case QS_TUNE_FIX_OVERLAP: c->tune_fix_overlap = value ? 1u : 0u; return QS_OK;
        case QS_TUNE_FIX_SPLIT_AT:
            if (value > c->n) return fail(c, QS_ERR_ARG, "qs_set_tuning: QS_TUNE_FIX_SPLIT_AT takes 0 (planned) or a largest id up to n_taxa");
            c->tune_fix_split_at = (uint32_t)value; return QS_OK;
        case QS_TUNE_STEP_ORDER:
            if (value > 2) return fail(c, QS_ERR_ARG, "qs_set_tuning: QS_TUNE_STEP_ORDER takes 0 (automatic), 1 (prefetch) or 2 (late loads)");
            c->tune_step_order = (uint32_t)value; return QS_OK;
        case QS_TUNE_STAGE_SIX:
            if (value > 2) return fail(c, QS_ERR_ARG, "qs_set_tuning: QS_TUNE_STAGE_SIX takes 0 (automatic), 1 (the instances QS_TUNE_STEP_ORDER selects) or 2 (the six-wave instance)");
            c->tune_stage_six = (uint32_t)value; return QS_OK;
        case QS_TUNE_CLASS_PCT: if (value > 100) return fail(c, QS_ERR_ARG, "qs_set_tuning: QS_TUNE_CLASS_PCT takes 0 .. 100"); c->tune_class_pct = (uint32_t)value; return QS_OK;
        case QS_TUNE_SCORE_LOAD:
            if (value > 3) return fail(c, QS_ERR_ARG, "qs_set_tuning: QS_TUNE_SCORE_LOAD takes 0 .. 3");
            c->tune_score_load = (uint32_t)value;
            c->bundle_r0[0] = c->bundle_r0[1] = c->bundle_r1[0] = c->bundle_r1[1] = ~0ull;   // the rounds are planned per wave count, which the load mode sets
            return QS_OK;
        case QS_TUNE_SCORE_DEDUPE: c->tune_score_dedupe = value ? 1u : 0u; return QS_OK;
        case QS_TUNE_SCORE_LOG_CAP:
            if (value > (1ull << 26)) return fail(c, QS_ERR_ARG, "qs_set_tuning: QS_TUNE_SCORE_LOG_CAP takes at most 2^26 records");
            c->tune_score_log_cap = value; return QS_OK;
        case QS_TUNE_SCORE_PASSES:
            if (value > 2) return fail(c, QS_ERR_ARG, "qs_set_tuning: QS_TUNE_SCORE_PASSES takes 0 (automatic), 1 (two passes) or 2 (single read)");
            c->tune_score_passes = (uint32_t)value; return QS_OK;
        case QS_TUNE_COOP:
            if (value > 2) return fail(c, QS_ERR_ARG, "qs_set_tuning: QS_TUNE_COOP takes 0 (default: off), 1 (on) or 2 (off)");
            if (c->tune_coop != (uint32_t)value)
                if (int rc = drop_tile_order(c)) return rc;
            c->tune_coop = (uint32_t)value; return QS_OK;
        case QS_TUNE_GATHER_IMPL:
            if (value > QS_IMPL_BITSLICE) return fail(c, QS_ERR_ARG, "qs_set_tuning: QS_TUNE_GATHER_IMPL takes QS_IMPL_AUTO / _SWAR / _BITSLICE");
            c->tune_gather_impl = (uint32_t)value; return QS_OK;
        case QS_TUNE_PANEL_KERNEL:
            if (value > 1) return fail(c, QS_ERR_ARG, "qs_set_tuning: QS_TUNE_PANEL_KERNEL takes 0 (automatic) or 1 (general builder)");
            c->tune_panel_kernel = (uint32_t)value; return QS_OK;
        default: return fail(c, QS_ERR_ARG, "qs_set_tuning: unknown key");
    }
}

extern "C" int qs_create(qs_ctx **out, uint32_t n_taxa, uint32_t count_bits, uint32_t flags, int device, void *stream,
                         uint32_t d_lo, uint32_t d_hi) {
    if (!out) return fail(nullptr, QS_ERR_ARG, "qs_create: out is NULL");
    *out = nullptr;
    if (n_taxa < 4 || n_taxa > 4096) return fail(nullptr, QS_ERR_ARG, "qs_create: n_taxa must be in [4, 4096]");
    if (count_bits != 16 && count_bits != 32) return fail(nullptr, QS_ERR_ARG, "qs_create: count_bits must be 16 or 32");
    if (d_lo == 0 && d_hi == 0) d_hi = n_taxa;
    if (d_hi > n_taxa || d_lo >= d_hi) return fail(nullptr, QS_ERR_ARG, "qs_create: bad shard [d_lo, d_hi)");
    // Everything that needs no device first: the tile geometry and -- for large tilings, on a helper thread -- the launch order of the
    // binary tiling (build_tile_perm: ~25 ms at 512 taxa), so that in a fresh process it is computed while the first HIP call below
    // waits for the runtime to come up.
    qs_ctx *c = new qs_ctx();
    c->n = n_taxa; c->count_bits = count_bits; c->flags = flags; c->device = device;
    c->stream = (hipStream_t)stream;
    c->d_lo = d_lo; c->d_hi = d_hi;
    c->rank_lo = binom4(d_lo);
    c->n_tuples = binom4(d_hi) - binom4(d_lo);
    // tile geometry of the gather kernel
    std::vector<uint32_t> cp(n_taxa + 2, 0);
    for (uint32_t cc = 2; cc <= n_taxa; ++cc)
        cp[cc + 1] = cp[cc] + gather_tiles_for_c(cc);
    // note: cp[c] = tiles of all c' < c (c' >= 2)
    const uint32_t d_start = std::max(d_lo, 3u);
    c->n_dblk = d_hi > d_start ? (d_hi - d_start + kDB - 1) / kDB : 0;
    std::vector<uint32_t> dp(c->n_dblk + 1, 0);
    uint64_t tiles64 = 0;
    for (uint32_t k = 0; k < c->n_dblk; ++k) {
        uint32_t d0 = d_start + k * kDB, d1 = std::min(d0 + (uint32_t)kDB, d_hi);
        tiles64 += cp[d1 - 1]; // c in [2, d1-1)
        dp[k + 1] = (uint32_t)tiles64;
    }
    if (tiles64 >= (1ull << 31)) { delete c; return fail(nullptr, QS_ERR_UNSUPPORTED, "qs_create: shard too large for one launch; use a narrower [d_lo, d_hi)"); }
    c->total_tiles = dp[c->n_dblk];
    // the 16x8 tiles of count_bitslice3_kernel; block k = [max(d_start, d1 - 8), d1) with d1 = d_hi - 8k
    std::vector<uint32_t> cp3(n_taxa + 2, 0), dp3(c->n_dblk + 1, 0);
    {
        for (uint32_t cc = 2; cc <= n_taxa; ++cc) cp3[cc + 1] = cp3[cc] + bitslice3_tiles_for_c(cc);
        uint64_t t3 = 0;
        for (uint32_t k = 0; k < c->n_dblk; ++k) { t3 += cp3[d_hi - k * kDB - 1]; dp3[k + 1] = (uint32_t)t3; }
        if (t3 >= (1ull << 31)) { delete c; return fail(nullptr, QS_ERR_UNSUPPORTED, "qs_create: shard too large for one launch; use a narrower [d_lo, d_hi)"); }
        c->total_tiles3 = dp3[c->n_dblk];
        c->h_cp3 = cp3; c->h_dp3 = dp3;
    }
    if (c->total_tiles3 >= (1u << 20) && c->total_tiles3 <= (1u << 26) && c->tile_chunk) {
        const TilePermParams P{c->tile_chunk, c->tile_cblock, c->tile_cgroup, c->d_hi, c->n_dblk, c->total_tiles3};
        try {
            c->perm_early = std::async(std::launch::async, [P, cp3, dp3] {
                EarlyPerm ep; ep.chunk = P.chunk; ep.cblock_in = P.cblock_in; ep.cgroup = P.cgroup;
                std::string err;
                ep.ok = build_tile_perm(P, cp3, dp3, ep.perm, err);
                return ep;
            });
        } catch (...) { c->perm_early = std::future<EarlyPerm>(); }   // no thread to be had: tile_order builds it when asked
    }
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0) {
        delete c;   // (waits for the helper thread: a std::async future blocks in its destructor)
        return fail(nullptr, QS_ERR_NO_DEVICE,
                    "qs_create: no HIP device (this library has no CPU fallback; it needs a gfx950 GPU)");
    }
    if (device < 0 || device >= ndev) { delete c; return fail(nullptr, QS_ERR_ARG, "qs_create: bad device ordinal"); }
    if (hipSetDevice(device) != hipSuccess) { delete c; return fail(nullptr, QS_ERR_HIP, "qs_create: hipSetDevice"); }
    auto cleanup = [&](int code, const std::string &m) { qs_destroy(c); return fail(nullptr, code, m); };
    if (c->cprefix.reserve(cp.size() * 4, nullptr) != hipSuccess) return cleanup(QS_ERR_OOM, "hipMalloc cprefix");
    if (c->dprefix.reserve(dp.size() * 4, nullptr) != hipSuccess) return cleanup(QS_ERR_OOM, "hipMalloc dprefix");
    if (hipMemcpy(c->cprefix.get(), cp.data(), cp.size() * 4, hipMemcpyHostToDevice) != hipSuccess) return cleanup(QS_ERR_HIP, "memcpy cprefix");
    if (hipMemcpy(c->dprefix.get(), dp.data(), dp.size() * 4, hipMemcpyHostToDevice) != hipSuccess) return cleanup(QS_ERR_HIP, "memcpy dprefix");
    if (c->cprefix3.reserve(cp3.size() * 4, nullptr) != hipSuccess) return cleanup(QS_ERR_OOM, "hipMalloc cprefix3");
    if (c->dprefix3.reserve(dp3.size() * 4, nullptr) != hipSuccess) return cleanup(QS_ERR_OOM, "hipMalloc dprefix3");
    if (hipMemcpy(c->cprefix3.get(), cp3.data(), cp3.size() * 4, hipMemcpyHostToDevice) != hipSuccess) return cleanup(QS_ERR_HIP, "memcpy cprefix3");
    if (hipMemcpy(c->dprefix3.get(), dp3.data(), dp3.size() * 4, hipMemcpyHostToDevice) != hipSuccess) return cleanup(QS_ERR_HIP, "memcpy dprefix3");
    if (c->dev_flags.reserve(16, nullptr) != hipSuccess) return cleanup(QS_ERR_OOM, "hipMalloc flags");
    if (hipMemset(c->dev_flags.get(), 0, 16) != hipSuccess) return cleanup(QS_ERR_HIP, "memset flags");
    *out = c;
    return QS_OK;
}

// Every device and pinned buffer of the context is a DevBuf member and goes with `delete c`; what is left to do by hand is what
// has to happen before: wait for the copies out of the staging buffers, and release what the slab cache holds (BatchSlab is a
// plain struct shared with the launch code).
extern "C" void qs_destroy(qs_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    for (hipEvent_t e : c->evs) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->pin_ev) if (e) { (void)hipEventSynchronize(e); (void)hipEventDestroy(e); }
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    for (hipEvent_t e : c->score_ev) if (e) (void)hipEventDestroy(e);
    for (BatchSlab &sl : c->slabs) { (void)hipFree(sl.p); if (sl.last_use) (void)hipEventDestroy(sl.last_use); }
    delete c;
}

// Work the first qs_count_batch would otherwise do before its first launch, done ahead of time (the host calls this on its
// GPU-initialisation thread while the evaluation trees are still being parsed): the launch order of the bit-sliced count
// kernel for binary batches (12 M slots at 512 taxa: ~60 ms of host work + a 47 MB copy) and the pair-depth panel for a
// batch of n_trees_hint trees. Purely an optimisation: qs_count_batch builds whatever is missing. The reference does the
// equivalent set-up in the table's constructor (QuartetCounterLookup.hpp:245-273).
size_t qs::padded(size_t bytes) { return (bytes + 255) & ~(size_t)255; }   // the pieces of a staged batch start at 256-byte boundaries (Stager, qs_abi_count.hip)
// pinned staging buffer `slot` holds `need` bytes, with a quarter to spare when it has to grow (nothing reads it then: the
// caller has waited for pin_ev[slot], or it has never been used)
hipError_t qs::ensure_pinned(qs_ctx *c, int slot, size_t need) {
    return c->pin[slot].bytes() >= need ? hipSuccess : c->pin[slot].reserve(need + need / 4 + 4096, nullptr);
}
static int prepare_staging(qs_ctx *c, uint64_t n_trees_hint);
extern "C" int qs_prepare(qs_ctx *c, uint64_t n_trees_hint) {
    if (!c) return QS_ERR_ARG;
    QS_HIP(c, hipSetDevice(c->device));
    // the staging allocations (two pinned buffers + a device slab: ~10 ms) on a helper thread beside the launch order (~15 ms of
    // host work): they touch different members of the context
    std::thread staging;
    if (n_trees_hint) {
        try { staging = std::thread([c, n_trees_hint] { (void)prepare_staging(c, n_trees_hint); }); }
        catch (...) { (void)prepare_staging(c, n_trees_hint); }   // (no thread to be had: do it here; nothing throws across the C boundary)
    }
    struct Join { std::thread &t; ~Join() { if (t.joinable()) t.join(); } } join_staging{staging};
    const uint32_t *order = nullptr;
    int rc = tile_order(c, &order);
    if (rc != QS_OK) return rc;
    if (n_trees_hint && !c->panel) {   // (no stream to wait for: there is no panel yet)
        const size_t group_bytes = (size_t)binom2(c->n) * 5 * 4;   // 5 planes: the common depth class
        const uint32_t groups = slice_groups(c, group_bytes, (uint32_t)std::min<uint64_t>((n_trees_hint + 31) / 32, 1u << 20), order != nullptr);
        if (c->panel.reserve((size_t)groups * group_bytes, nullptr) != hipSuccess) (void)hipGetLastError();   // not fatal here: the count reports it if it persists
    }
    return QS_OK;
}
static int prepare_staging(qs_ctx *c, uint64_t n_trees_hint) {
    if (hipSetDevice(c->device) != hipSuccess) { (void)hipGetLastError(); return QS_ERR_HIP; }
    {
        // both pinned staging buffers and one device slab for batches of that many full trees (qs_batch_upload's Stager
        // would allocate them on first use: hipHostMalloc + hipMalloc, tens of ms in front of the first count)
        const uint64_t nt = std::min<uint64_t>(n_trees_hint, 1u << 22);
        const size_t need = padded(((size_t)nt + 1) * 4) + 2 * padded((size_t)nt * c->n * 2) + padded((size_t)nt * 4);
        if (!c->copy_stream && hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking) != hipSuccess) { c->copy_stream = nullptr; (void)hipGetLastError(); return QS_ERR_HIP; }
        for (int slot = 0; slot < 2; ++slot)
            if (ensure_pinned(c, slot, need) != hipSuccess) (void)hipGetLastError();   // (the first upload asks again and reports it)
        bool have = false;
        for (const BatchSlab &sl : c->slabs) have = have || sl.cap >= need;
        if (!have && c->slabs.size() < 4) {
            BatchSlab sl;
            sl.cap = need + need / 4;
            if (hipMalloc(&sl.p, sl.cap) == hipSuccess) c->slabs.push_back(sl); else (void)hipGetLastError();
        }
    }
    // first use of the count kernels' code object (~5 ms of loading on MI355X: tools/modload_probe.py) here, beside the launch
    // order, instead of in front of the first count: one lookup of the quartet {0,1,2,3} on the copy stream
    if (c->table && c->n >= 4 && c->d_lo == 0) {
        DevBuf<char> scratch;
        if (scratch.reserve(64, nullptr) == hipSuccess) {
            const uint16_t ids[4] = {0, 1, 2, 3};
            if (hipMemcpyAsync(scratch.get(), ids, sizeof ids, hipMemcpyHostToDevice, c->copy_stream) == hipSuccess)
                (void)launch_lookup(c->copy_stream, c->n, c->d_lo, c->d_hi, c->rank_lo, c->table, (int)c->count_bits, 1, (const uint16_t *)scratch.get(),
                                    (uint64_t *)(scratch.get() + 16));
            (void)hipStreamSynchronize(c->copy_stream);
        }
        (void)hipGetLastError();
    }
    // the correction stream of split slices (QS_TUNE_FIX_OVERLAP) with its hardware queue, which the runtime opens with the stream's
    // first work: here instead of inside the first count
    if (c->tune_fix_overlap && c->fix_stream.ensure() == hipSuccess) {
        DevBuf<char> word;
        if (word.reserve(64, nullptr) == hipSuccess && hipMemsetAsync(word.get(), 0, 64, c->fix_stream.get()) == hipSuccess)
            (void)hipStreamSynchronize(c->fix_stream.get());
    }
    (void)hipGetLastError();
    return QS_OK;
}

// ---- table -------------------------------------------------------------------------------

extern "C" uint64_t qs_table_tuples(const qs_ctx *c) { return c ? c->n_tuples : 0; }
extern "C" uint64_t qs_table_bytes(const qs_ctx *c) { return c ? c->n_tuples * 3 * (c->count_bits / 8) : 0; }
extern "C" void *qs_table_device_ptr(const qs_ctx *c) { return c ? c->table : nullptr; }
extern "C" uint64_t qs_trees_counted(const qs_ctx *c) { return c ? c->trees_counted : 0; }

// the largest count a cell of the context's table may hold: the trees behind the table if known, else what a cell can hold
uint64_t qs::table_max_count(const qs_ctx *c) {
    const uint64_t cell_max = c->count_bits == 16 ? 0xFFFFull : 0xFFFFFFFFull;
    const uint64_t trees = std::max(std::max(c->trees_counted, c->table_trees_hint), c->collapse_max_count);   // (a collapsed table's cells exceed its trees)
    return trees ? std::min(trees, cell_max) : cell_max;
}

extern "C" int qs_table_alloc(qs_ctx *c) {
    if (c) c->log_valid = false;   // (the table / view / tuning may change: a logged pass 1 no longer describes it)
    if (!c) return QS_ERR_ARG;
    QS_HIP(c, hipSetDevice(c->device));
    if (c->table_mem) { c->table_mem.reset(); c->table = nullptr; }
    size_t bytes = (size_t)qs_table_bytes(c);
    size_t freeb = 0, total = 0;
    QS_HIP(c, hipMemGetInfo(&freeb, &total));
    if (bytes + (64u << 20) > freeb) return fail(c, QS_ERR_OOM, "Insufficient memory!");
    if (c->table_mem.reserve(bytes + 16, nullptr) != hipSuccess) { c->table = nullptr; return fail(c, QS_ERR_OOM, "Insufficient memory!"); }
    c->table = c->table_mem.get();
    c->trees_counted = 0;
    c->collapse_max_count = 0;   // (describes contents that are gone)
    QS_HIP(c, hipMemsetAsync(c->table, 0, bytes + 16, c->stream));
    return QS_OK;
}

extern "C" int qs_table_attach(qs_ctx *c, void *device_ptr, uint64_t bytes) {
    if (c) c->log_valid = false;   // (the table / view / tuning may change: a logged pass 1 no longer describes it)
    if (!c) return QS_ERR_ARG;
    if (!device_ptr) {
        // detach: the caller takes its buffer back (e.g. to free a full table once its reduce-scattered shard is the scoring view)
        if (bytes != 0) return fail(c, QS_ERR_ARG, "qs_table_attach: NULL pointer with a size (detach = NULL, 0)");
        if (c->table_mem) return fail(c, QS_ERR_STATE, "qs_table_attach: detach of a table the context owns (qs_table_alloc)");
        QS_HIP(c, hipSetDevice(c->device));
        QS_HIP(c, hipStreamSynchronize(c->stream));   // nothing of this context may still be writing the buffer
        c->table = nullptr;
        return QS_OK;
    }
    // 16-bit cells are updated through their 32-bit word (packed half-word atomics of the scatter kernel, word-wise
    // collectives): the buffer must cover whole words
    const uint64_t need = (qs_table_bytes(c) + 3) & ~3ull;
    if (bytes < need) return fail(c, QS_ERR_ARG, "qs_table_attach: buffer smaller than qs_table_bytes() rounded up to a multiple of 4");
    if ((uintptr_t)device_ptr & 3) return fail(c, QS_ERR_ARG, "qs_table_attach: pointer must be 4-byte aligned");
    c->table_mem.reset();   // (the context's own table, if it had one)
    c->table = device_ptr;
    return QS_OK;
}

extern "C" int qs_table_clear(qs_ctx *c) {
    if (c) c->log_valid = false;   // (the table / view / tuning may change: a logged pass 1 no longer describes it)
    if (!c || !c->table) return fail(c, QS_ERR_STATE, "qs_table_clear: no table");
    QS_HIP(c, hipSetDevice(c->device));
    QS_HIP(c, hipMemsetAsync(c->table, 0, (size_t)qs_table_bytes(c), c->stream));
    c->trees_counted = 0;
    c->collapse_max_count = 0;   // (describes contents that are gone)
    return QS_OK;
}

extern "C" int qs_table_download(qs_ctx *c, void *host_dst, uint64_t bytes) {
    if (!c || !c->table) return fail(c, QS_ERR_STATE, "qs_table_download: no table");
    if (bytes > qs_table_bytes(c)) return fail(c, QS_ERR_ARG, "qs_table_download: too many bytes");
    QS_HIP(c, hipSetDevice(c->device));
    QS_HIP(c, hipMemcpyAsync(host_dst, c->table, (size_t)bytes, hipMemcpyDeviceToHost, c->stream));
    QS_HIP(c, hipStreamSynchronize(c->stream));
    return QS_OK;
}

extern "C" int qs_table_upload(qs_ctx *c, const void *host_src, uint64_t bytes) {
    if (c) c->log_valid = false;   // (the table / view / tuning may change: a logged pass 1 no longer describes it)
    if (!c || !c->table) return fail(c, QS_ERR_STATE, "qs_table_upload: no table");
    if (bytes > qs_table_bytes(c)) return fail(c, QS_ERR_ARG, "qs_table_upload: too many bytes");
    QS_HIP(c, hipSetDevice(c->device));
    QS_HIP(c, hipMemcpyAsync(c->table, host_src, (size_t)bytes, hipMemcpyHostToDevice, c->stream));
    QS_HIP(c, hipStreamSynchronize(c->stream));
    return QS_OK;
}

extern "C" int qs_table_pack16(qs_ctx *c, void *dst_device, uint64_t dst_bytes) {
    if (!c || !c->table || !dst_device) return fail(c, QS_ERR_STATE, "qs_table_pack16: no table / NULL destination");
    if (c->count_bits != 32) return fail(c, QS_ERR_ARG, "qs_table_pack16: the table already has 16-bit cells");
    const uint64_t cells = c->n_tuples * 3, need = ((cells + 1) / 2) * 4;
    if (dst_bytes < need) return fail(c, QS_ERR_ARG, "qs_table_pack16: destination smaller than " + std::to_string(need) + " bytes");
    QS_HIP(c, hipSetDevice(c->device));
    QS_HIP(c, launch_pack16(c->stream, c->table, dst_device, cells, c->dev_flags.get()));
    return QS_OK;
}

extern "C" int qs_wire_attach(qs_ctx *c, void *dst_device, uint64_t dst_bytes) {
    if (c) c->log_valid = false;   // (the table / view / tuning may change: a logged pass 1 no longer describes it)
    if (!c) return QS_ERR_ARG;
    if (!dst_device) { c->wire_out = nullptr; c->wire_trees = 0; return QS_OK; }
    if (dst_bytes < c->n_tuples * 4) return fail(c, QS_ERR_ARG, "qs_wire_attach: destination smaller than " + std::to_string(c->n_tuples * 4) + " bytes");
    c->wire_out = (uint32_t *)dst_device;
    c->wire_trees = 0;
    return QS_OK;
}

extern "C" int qs_table_pack16x2(qs_ctx *c, void *dst_device, uint64_t dst_bytes) {
    if (!c || !c->table || !dst_device) return fail(c, QS_ERR_STATE, "qs_table_pack16x2: no table / NULL destination");
    if (c->count_bits != 32) return fail(c, QS_ERR_ARG, "qs_table_pack16x2: needs a 32-bit table");
    if (c->trees_counted > 0xFFFFull) return fail(c, QS_ERR_OVERFLOW, "qs_table_pack16x2: more than 65535 trees counted");
    if (dst_bytes < c->n_tuples * 4) return fail(c, QS_ERR_ARG, "qs_table_pack16x2: destination smaller than " + std::to_string(c->n_tuples * 4) + " bytes");
    QS_HIP(c, hipSetDevice(c->device));
    QS_HIP(c, launch_pack16x2(c->stream, c->table, dst_device, c->n_tuples, (uint32_t)c->trees_counted, c->dev_flags.get(), c->dev_flags.get() + 3));
    return QS_OK;
}

extern "C" int qs_unpack16x2(qs_ctx *c, const void *src_device, uint64_t n_tuples, uint32_t total_trees, void *dst_device) {
    if (c) c->log_valid = false;   // (the table / view / tuning may change: a logged pass 1 no longer describes it)
    if (!c || !src_device || !dst_device) return fail(c, QS_ERR_ARG, "qs_unpack16x2: NULL argument");
    if (total_trees > 0xFFFFu) return fail(c, QS_ERR_OVERFLOW, "qs_unpack16x2: more than 65535 trees");
    QS_HIP(c, hipSetDevice(c->device));
    QS_HIP(c, launch_unpack16x2(c->stream, src_device, dst_device, n_tuples, total_trees, c->dev_flags.get() + 3));
    return QS_OK;
}

// Two-cell wire format with 32-bit cells: (n0, n1) per tuple, for batches of binary trees holding all taxa whose total
// over the ranks reaches 65536 trees (8 bytes per quartet on the wire instead of 12).
extern "C" int qs_table_pack32x2(qs_ctx *c, void *dst_device, uint64_t dst_bytes) {
    if (!c || !c->table || !dst_device) return fail(c, QS_ERR_STATE, "qs_table_pack32x2: no table / NULL destination");
    if (c->count_bits != 32) return fail(c, QS_ERR_ARG, "qs_table_pack32x2: needs a 32-bit table");
    if (c->trees_counted > 0xFFFFFFFFull) return fail(c, QS_ERR_OVERFLOW, "qs_table_pack32x2: more than 2^32 - 1 trees counted");
    if (dst_bytes < c->n_tuples * 8) return fail(c, QS_ERR_ARG, "qs_table_pack32x2: destination smaller than " + std::to_string(c->n_tuples * 8) + " bytes");
    QS_HIP(c, hipSetDevice(c->device));
    QS_HIP(c, launch_pack32x2(c->stream, c->table, dst_device, c->n_tuples, (uint32_t)c->trees_counted, c->dev_flags.get() + 3));
    return QS_OK;
}

extern "C" int qs_unpack32x2(qs_ctx *c, const void *src_device, uint64_t n_tuples, uint64_t total_trees, void *dst_device) {
    if (c) c->log_valid = false;   // (the table / view / tuning may change: a logged pass 1 no longer describes it)
    if (!c || !src_device || !dst_device) return fail(c, QS_ERR_ARG, "qs_unpack32x2: NULL argument");
    if (total_trees > 0xFFFFFFFFull) return fail(c, QS_ERR_OVERFLOW, "qs_unpack32x2: more than 2^32 - 1 trees");
    QS_HIP(c, hipSetDevice(c->device));
    QS_HIP(c, launch_unpack32x2(c->stream, src_device, dst_device, n_tuples, (uint32_t)total_trees, c->dev_flags.get() + 3));
    return QS_OK;
}

// the device's compute units, asked once per context
int qs::ensure_n_cu(qs_ctx *c) {
    if (c->n_cu == 0) { int v = 0; QS_HIP(c, hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, c->device)); c->n_cu = std::max(1, v); }
    return QS_OK;
}

extern "C" int qs_sum_words(qs_ctx *c, void *dst_device, const void *const *src_device, uint32_t n_src, uint64_t n_words) {
    if (c) c->log_valid = false;   // (a table may change under a logged pass 1)
    if (!c || (n_words && n_src && (!dst_device || !src_device))) return fail(c, QS_ERR_ARG, "qs_sum_words: NULL argument");
    if (n_src > 15) return fail(c, QS_ERR_ARG, "qs_sum_words: at most 15 sources");
    if ((uintptr_t)dst_device & 15) return fail(c, QS_ERR_ARG, "qs_sum_words: the destination must be 16-byte aligned");
    for (uint32_t k = 0; k < n_src; ++k)
        if (!src_device[k] || ((uintptr_t)src_device[k] & 15)) return fail(c, QS_ERR_ARG, "qs_sum_words: sources must be non-NULL and 16-byte aligned");
    QS_HIP(c, hipSetDevice(c->device));
    if (int rc = ensure_n_cu(c)) return rc;
    QS_HIP(c, launch_sum_words(c->stream, dst_device, src_device, n_src, n_words, c->n_cu));
    return QS_OK;   // asynchronous on the context's stream
}

// qs_table_remap (subset = false: a permutation of the same taxa, qs_remap.hip) and qs_table_restrict (subset = true: an injective
// map of dst's taxa into src's, qs_restrict.hip) differ in what they ask of the taxon counts and the id map and in the kernel they launch.
static int table_reindex(qs_ctx *dst, const qs_ctx *src, const uint16_t *src_id_of, bool subset) {
    const std::string fn = subset ? "qs_table_restrict: " : "qs_table_remap: ";
    if (dst) dst->log_valid = false;   // (the table changes: a logged pass 1 no longer describes it)
    if (!dst) return QS_ERR_ARG;
    if (!src || !src_id_of) return fail(dst, QS_ERR_ARG, fn + "NULL argument");
    if (dst == src) return fail(dst, QS_ERR_ARG, fn + "source and destination are the same context");
    if (dst->d_lo != 0 || dst->d_hi != dst->n || src->d_lo != 0 || src->d_hi != src->n)
        return fail(dst, QS_ERR_UNSUPPORTED, fn + "whole-table contexts only (no table shards)");
    if (subset ? dst->n > src->n : dst->n != src->n)
        return fail(dst, QS_ERR_ARG, fn + (subset ? "the destination has more taxa than the source" : "the contexts have different numbers of taxa"));
    if (dst->device != src->device) return fail(dst, QS_ERR_ARG, fn + "the contexts are on different devices");
    if (!dst->table || !src->table) return fail(dst, QS_ERR_STATE, fn + "the " + (src->table ? "destination" : "source") + " has no table");
    if (dst->table == src->table) return fail(dst, QS_ERR_ARG, fn + "source and destination share their table");
    if (dst->count_bits < src->count_bits) return fail(dst, QS_ERR_ARG, fn + "32-bit cells cannot be narrowed to 16 bits");
    std::vector<uint8_t> seen(src->n, 0);
    bool monotone = true;   // strictly increasing: the source ids of a destination 4-set are sorted as they come
    for (uint32_t i = 0; i < dst->n; ++i) {
        if (src_id_of[i] >= src->n || seen[src_id_of[i]])
            return fail(dst, QS_ERR_ARG, fn + (subset ? "src_id_of is not injective into [0, n_taxa of the source)" : "src_id_of is not a permutation of [0, n_taxa)"));
        seen[src_id_of[i]] = 1;
        if (i && src_id_of[i] < src_id_of[i - 1]) monotone = false;
    }
    QS_HIP(dst, hipSetDevice(dst->device));
    QS_HIP(dst, dst->remap_ids.reserve(4096 * sizeof(uint16_t), nullptr));
    if (src->stream != dst->stream) {   // the source's counting (or upload) first
        hipEvent_t ev = nullptr;
        QS_HIP(dst, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        hipError_t e = hipEventRecord(ev, src->stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(dst->stream, ev, 0);
        (void)hipEventDestroy(ev);
        QS_HIP(dst, e);
    }
    QS_HIP(dst, hipMemcpyAsync(dst->remap_ids.get(), src_id_of, dst->n * sizeof(uint16_t), hipMemcpyHostToDevice, dst->stream));
    if (subset)
        QS_HIP(dst, launch_table_restrict(dst->stream, src->table, (int)src->count_bits, dst->table, (int)dst->count_bits, dst->remap_ids.get(), dst->n, dst->n_tuples, monotone));
    else
        QS_HIP(dst, launch_table_remap(dst->stream, src->table, (int)src->count_bits, dst->table, (int)dst->count_bits, dst->remap_ids.get(), dst->n, dst->n_tuples));
    dst->trees_counted = src->trees_counted;   // sizes the log table and the 16-bit overflow guard of later counts
    dst->collapse_max_count = src->collapse_max_count;   // (the cells of a collapsed source stay as large as they were)
    return QS_OK;   // asynchronous on dst's stream
}

// The table of `src` in the lookup-id order of another reference tree over the same taxa (qs_remap.hip), so that one count
// serves several reference trees. The reference recounts per run: this replaces nothing there.
extern "C" int qs_table_remap(qs_ctx *dst, const qs_ctx *src, const uint16_t *src_id_of) { return table_reindex(dst, src, src_id_of, false); }

// The table of `src` over a subset of its taxa, in any id order (qs_restrict.hip): the table of the problem without the other taxa,
// because what a tree displays for a 4-set does not depend on its other taxa (a tree pruned below four taxa still counts towards
// trees-counted; scores never depend on it). The reference rejects a leaf it does not know and recounts per run: this replaces
// nothing there.
extern "C" int qs_table_restrict(qs_ctx *dst, const qs_ctx *src, const uint16_t *src_id_of) { return table_reindex(dst, src, src_id_of, true); }

// The table of `src` (individuals) summed into the table of the species that own them (qs_collapse.hip): species i owns the source ids
// [first_id[i], first_id[i + 1]), and a destination tuple is the sum of the source tuples over one individual per species. A cell of
// dst can exceed trees-counted afterwards: collapse_max_count tells the score's log table and the whole-table queries so. The
// reference has no species map (its TaxonMapper is dead code): this replaces nothing there.
extern "C" int qs_table_collapse(qs_ctx *dst, const qs_ctx *src, const uint16_t *first_id) {
    const std::string fn = "qs_table_collapse: ";
    if (dst) dst->log_valid = false;   // (the table changes: a logged pass 1 no longer describes it)
    if (!dst) return QS_ERR_ARG;
    if (!src || !first_id) return fail(dst, QS_ERR_ARG, fn + "NULL argument");
    if (dst == src) return fail(dst, QS_ERR_ARG, fn + "source and destination are the same context");
    if (dst->d_lo != 0 || dst->d_hi != dst->n || src->d_lo != 0 || src->d_hi != src->n)
        return fail(dst, QS_ERR_UNSUPPORTED, fn + "whole-table contexts only (no table shards)");
    if (dst->n > src->n) return fail(dst, QS_ERR_ARG, fn + "the destination has more taxa than the source");
    if (dst->device != src->device) return fail(dst, QS_ERR_ARG, fn + "the contexts are on different devices");
    if (!dst->table || !src->table) return fail(dst, QS_ERR_STATE, fn + "the " + (src->table ? "destination" : "source") + " has no table");
    if (dst->table == src->table) return fail(dst, QS_ERR_ARG, fn + "source and destination share their table");
    if (dst->count_bits < src->count_bits) return fail(dst, QS_ERR_ARG, fn + "32-bit cells cannot be narrowed to 16 bits");
    if (src->n > 4096) return fail(dst, QS_ERR_UNSUPPORTED, fn + "more than 4096 source taxa");
    if (first_id[0] != 0 || first_id[dst->n] != src->n) return fail(dst, QS_ERR_ARG, fn + "first_id does not run from 0 to the source's n_taxa");
    for (uint32_t i = 0; i < dst->n; ++i)
        if (first_id[i + 1] <= first_id[i]) return fail(dst, QS_ERR_ARG, fn + "first_id is not strictly increasing (group " + std::to_string(i) + " is empty)");
    // the largest sum: (largest source count) x the four largest groups
    uint64_t top[4] = {1, 1, 1, 1};
    for (uint32_t i = 0; i < dst->n; ++i) {
        uint64_t g = first_id[i + 1] - first_id[i];
        for (uint64_t &t : top) if (g > t) std::swap(g, t);
    }
    const uint64_t src_max = table_max_count(src), prod = top[0] * top[1] * top[2] * top[3];   // (groups sum to <= 4096: below 2^40)
    const uint64_t bound = src_max > UINT64_MAX / prod ? UINT64_MAX : src_max * prod;
    const size_t id_words = 4097 + (size_t)src->n;   // first_id | the species of every source id
    QS_HIP(dst, hipSetDevice(dst->device));
    QS_HIP(dst, dst->collapse_ids_dev.reserve((4097 + 4096) * sizeof(uint16_t), &dst->stream));
    QS_HIP(dst, hipStreamSynchronize(dst->stream));   // (an earlier call's upload may still read the host copy)
    dst->collapse_ids.assign(id_words, 0);
    for (uint32_t i = 0; i <= dst->n; ++i) dst->collapse_ids[i] = first_id[i];
    for (uint32_t i = 0; i < dst->n; ++i)
        for (uint32_t a = first_id[i]; a < first_id[i + 1]; ++a) dst->collapse_ids[4097 + a] = (uint16_t)i;
    if (src->stream != dst->stream) {   // the source's counting (or upload) first
        hipEvent_t ev = nullptr;
        QS_HIP(dst, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        hipError_t e = hipEventRecord(ev, src->stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(dst->stream, ev, 0);
        (void)hipEventDestroy(ev);
        QS_HIP(dst, e);
    }
    QS_HIP(dst, hipMemcpyAsync(dst->collapse_ids_dev.get(), dst->collapse_ids.data(), id_words * sizeof(uint16_t), hipMemcpyHostToDevice, dst->stream));
    QS_HIP(dst, launch_table_collapse(dst->stream, src->table, (int)src->count_bits, dst->table, (int)dst->count_bits, dst->collapse_ids_dev.get(),
                                      dst->n, src->n, dst->dev_flags.get()));
    dst->trees_counted = src->trees_counted;
    dst->collapse_max_count = bound;   // (sizes the log table of the device QIC: ensure_score_tables)
    return QS_OK;   // asynchronous on dst's stream
}

extern "C" int qs_sync(qs_ctx *c) {
    if (!c) return QS_ERR_ARG;
    QS_HIP(c, hipSetDevice(c->device));
    QS_HIP(c, hipStreamSynchronize(c->stream));
    uint32_t fl[4] = {0, 0, 0, 0};
    QS_HIP(c, hipMemcpy(fl, c->dev_flags.get(), 16, hipMemcpyDeviceToHost));
    if (fl[0]) {
        (void)hipMemset(c->dev_flags.get(), 0, 4);
        return fail(c, QS_ERR_OVERFLOW, "count table overflow: a counter exceeded count_bits");
    }
    if (fl[3]) {
        (void)hipMemset(c->dev_flags.get() + 3, 0, 4);
        return fail(c, QS_ERR_STATE, "two-cell wire format: a tuple does not sum to the number of trees (the batch was not binary with all taxa)");
    }
    return QS_OK;
}

extern "C" int qs_lookup(qs_ctx *c, uint64_t nq, const uint16_t *abcd, uint64_t *out3) {
    if (!c || !c->table) return fail(c, QS_ERR_STATE, "qs_lookup: no table");
    if (nq == 0) return QS_OK;
    if (!abcd || !out3) return fail(c, QS_ERR_ARG, "qs_lookup: NULL");
    for (uint64_t i = 0; i < nq * 4; ++i)
        if (abcd[i] >= c->n) return fail(c, QS_ERR_ARG, "qs_lookup: id out of range");
    QS_HIP(c, hipSetDevice(c->device));
    DevBuf<uint16_t> dq; DevBuf<uint64_t> dout;   // (freed on every way out; hipFree waits for the device)
    QS_HIP(c, dq.reserve(nq * 8, nullptr));
    if (dout.reserve(nq * 24, nullptr) != hipSuccess) return fail(c, QS_ERR_OOM, "qs_lookup: hipMalloc");
    hipError_t e = hipMemcpyAsync(dq.get(), abcd, nq * 8, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = launch_lookup(c->stream, c->n, c->d_lo, c->d_hi, c->rank_lo, c->table, (int)c->count_bits, nq, dq.get(), dout.get());
    if (e == hipSuccess) e = hipMemcpyAsync(out3, dout.get(), nq * 24, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, QS_ERR_HIP, std::string("qs_lookup: ") + hipGetErrorString(e));
    return QS_OK;
}
