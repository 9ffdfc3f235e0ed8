"""16-bit count cells at their limit, on every path that writes them.

count_bits = 16 is chosen whenever at most 65 535 trees are counted: three cells in six bytes, two cells per 32-bit word. Every
writer of that layout either checks what it stores ((w0 | w1 | w2) > 0xFFFF raises the overflow flag qs_sync reports) or relies
on the host keeping the totals below 2^16 so that a packed half-word add cannot carry. The parity tests say which cell a tree
increments; this module says how large a cell may get:

  1. 65 535 trees (a handful of distinct trees with multiplicities) counted into 16-bit cells equal the oracle's uint64 table,
     path by path; cells reach exactly 65 535, next to empty neighbours in the same word;
  2. the 65 536th tree is refused by every host guard and nothing changes;
  3. a preset table: filling every cell to exactly 65 535 passes, one more in a single cell is QS_ERR_OVERFLOW, on every writer.

The reference of every comparison is the CPU oracle's table for the same trees and multiplicities, never reduced modulo 2^16:
its cells are asserted to be at most 65 535 first.
Run on the GPU box: python -m pytest tests/test_gpu_cell_limits.py
"""
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import taxon_model
from helpers import concat_batches, repeat_trees, ulp_diff
from oracle_api import Oracle
from quartetscores_amd import _lib, flatten, ranks, synth

pytestmark = pytest.mark.gpu

FULL = 65535
MODES = ("binary_full", "general_full", "partial", "binary_partial")     # order of the library's kernel modes
ONE_CLASS = {_lib.QS_TUNE_CLASS_MIN_TREES: 1, _lib.QS_TUNE_CLASS_PCT: 0, _lib.QS_TUNE_DEPTH_CLAMP: 0}   # every tree in the class of its own mode and depth
CLAMP_ALL = {_lib.QS_TUNE_CLASS_MIN_TREES: 1, _lib.QS_TUNE_CLASS_PCT: 0, _lib.QS_TUNE_DEPTH_CLAMP: 1000000}


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    from quartetscores_amd import engine
    return engine


# ---- inputs (all of this runs without a device) ------------------------------------------------------------------------------

def _ladder(n, order):
    cat = f"(t{order[0]},t{order[1]})"
    for i in order[2:]:
        cat = "(" + cat + f",t{i})"
    return cat + ";"


def _shape(nw, mode, rng, n):
    """The tree `nw` turned into one the library counts in kernel mode `mode`: taxa dropped (only ids that are multiples of 3
    are ever dropped, so quartets of the other taxa stay unanimous) and / or at least one edge collapsed."""
    t = synth._parse_simple(nw)
    if mode in ("partial", "binary_partial"):
        gone = {f"t{i}" for i in rng.choice(np.arange(0, n, 3), size=int(rng.integers(1, 3)), replace=False)}
        t = synth._drop(t, {f"t{i}" for i in range(n)} - gone)
        if len(t) == 2:                                   # keep the top level unrooted, like synth.random_tree
            a, b = t
            t = tuple(a) + (b,) if isinstance(a, tuple) else (a,) + tuple(b)
    if mode in ("general_full", "partial"):
        while True:
            t2 = synth._collapse(t, rng, 0.06)
            if t2 != t:
                break
        t = t2
    return synth._to_newick(t) + ";"


def _multiplicities(k, total, rng):
    """k multiplicities that sum to `total`, each at least three 32-tree groups and none a multiple of 32 (ragged last group)"""
    m = 97 + np.floor(rng.dirichlet(np.full(k, 4.0)) * (total - 97 * k)).astype(np.int64)
    m[0] += total - m.sum()
    while (m % 32 == 0).any():
        i = int(np.nonzero(m % 32 == 0)[0][0])
        m[i] += 1
        m[(i + 1) % k] -= 1
    assert m.sum() == total and (m >= 97).all() and (m % 32 != 0).all()
    return m


def _build(n, kind, seed, k_nni, k_random, total):
    ref_nw = synth.reference_tree(n, seed)
    ref = flatten.flatten_reference(ref_nw)
    rng = np.random.default_rng(seed + 1)
    deep = kind in ("deep", "clamp_general")              # a ladder that is not re-rooted and its NNI neighbours: up to n - 2 LCA levels
    order = [int(x) for x in rng.permutation(n)]
    base = _ladder(n, order) if deep else synth.tree_set(n, 1, seed + 2)[0]
    distinct = [base] + synth.nni_tree_set(base, k_nni - 1, seed + 3, mean_nni=3) + synth.tree_set(n, k_random, seed + 4)
    k = len(distinct)
    if kind == "mixed":
        modes = [MODES[i % 4] for i in range(k)]          # the four kernel modes interleaved
    else:
        modes = [{"deep": "binary_full", "clamp_general": "general_full"}.get(kind, kind)] * k
    distinct = [_shape(t, mo, rng, n) for t, mo in zip(distinct, modes)]
    small = flatten.flatten_eval_trees(distinct, ref.name_to_id, recentre=not deep)
    if total == k:
        mult = np.ones(k, dtype=np.int64)
    else:
        mult = _multiplicities(k, total, rng)
    o = Oracle(ref_nw)
    o.count("\n".join(distinct), mult=mult.astype(np.uint64))
    assert o.names == ref.names
    return SimpleNamespace(n=n, kind=kind, ref_nw=ref_nw, ref=ref, distinct=distinct, modes=modes, small=small, mult=mult, total=int(total),
                           want=o.counts().copy(), oracle=o, ladder_order=order if deep else None, _big={})


@functools.lru_cache(maxsize=None)
def limit_case(n, kind):
    """65 535 trees: a few NNI neighbours of one tree and two random trees, with multiplicities. The preconditions every test of
    part 1 relies on are asserted here, on the oracle's table alone."""
    c = _build(n, kind, 6500 + 10 * n + len(kind), 12 if kind == "mixed" else 7, 2, FULL)
    W = c.want
    assert W.dtype == np.uint64 and int(W.max()) == FULL, (n, kind, int(W.max()))
    flat = W.reshape(-1)
    pairs = flat[: 2 * (len(flat) // 2)].reshape(-1, 2)   # the two cells of every 32-bit word of the 16-bit layout
    assert ((pairs[:, 0] == FULL) & (pairs[:, 1] == 0)).any(), "no word with a full low half next to an empty high half"
    assert ((pairs[:, 0] == 0) & (pairs[:, 1] == FULL)).any(), "no word with a full high half next to an empty low half"
    if kind in ("binary_full", "deep"):
        assert (W.sum(axis=1) == FULL).all()
    return c


def big_batch(c, with_nodes=False):
    """the trees of the case with their multiplicities: tree by tree, each spanning many 32-tree groups and a ragged last one (a
    mixed case in two rounds, so that the modes are interleaved in the batch too)"""
    if with_nodes not in c._big:
        if c.kind == "mixed":
            reps = [(t, int(m) // 2) for t, m in enumerate(c.mult)] + [(t, int(m) - int(m) // 2) for t, m in enumerate(c.mult)]
        else:
            reps = [(t, int(m)) for t, m in enumerate(c.mult)]
        c._big[with_nodes] = repeat_trees(c.small, reps, with_nodes=with_nodes)
        assert c._big[with_nodes].n_trees == c.total
    return c._big[with_nodes]


@functools.lru_cache(maxsize=None)
def small_case(n, kind):
    """a batch of a few dozen trees whose cells stay far below the limit (part 3)"""
    c = _build(n, kind, 7700 + 10 * n + len(kind), 30, 6, 36)
    assert 0 < int(c.want.max()) <= 36
    return c


def tune(monkeypatch, eng, settings):
    for key, value in settings.items():
        monkeypatch.setitem(eng.DEFAULT_TUNING, key, value)


def count_into(eng, c, batch, bits=16, pieces=None, algo=None, with_nodes=False, shard=None, preset=None):
    """a fresh context, optionally a preset table, `batch` counted in the given pieces; returns the context BEFORE qs_sync"""
    ctx = eng.Context(c.n, bits, d_lo=shard[0], d_hi=shard[1]) if shard else eng.Context(c.n, bits)
    ctx.table_alloc()
    if preset is not None:
        ctx.table_upload(preset)
    for lo, hi in pieces or [(0, batch.n_trees)]:
        hb = ctx.batch_upload(batch if (lo, hi) == (0, batch.n_trees) else batch.slice(lo, hi), with_nodes=with_nodes)
        ctx.count_batch(hb, eng.QS_ALGO_GATHER if algo is None else algo)
        ctx.batch_free(hb)
    return ctx


def assert_full_count(eng, c, expect, **kw):
    """part 1, one path: the variant names what was meant to run, the table equals the oracle's bit for bit, 65 535 trees counted,
    qs_sync raises nothing"""
    nodes = kw.get("with_nodes", False)
    ctx = count_into(eng, c, big_batch(c, nodes), **kw)
    ctx.sync()
    v = ctx.last_count_variant()
    for piece in expect:
        assert (piece[1:] not in v) if piece.startswith("!") else (piece in v), (piece, v)
    assert "count_u16" in v, v
    T = ctx.table_download()
    assert T.dtype == np.uint16
    want = c.want
    if kw.get("shard"):
        want = want[ranks.n_quartets(kw["shard"][0]):ranks.n_quartets(kw["shard"][1])]
    bad = np.nonzero((T.astype(np.uint64) != want).any(axis=1))[0]
    assert len(bad) == 0, (v, len(bad), int(bad[0]), T[bad[0]].tolist(), want[bad[0]].tolist())
    assert ctx.trees_counted == FULL
    ctx.sync()
    return ctx, T


# ---- 1. 65 535 trees counted into 16-bit cells equal the oracle, path by path ---------------------------------------------

@pytest.mark.parametrize("n", [24, 70])
@pytest.mark.parametrize("kind", ["binary_full", "binary_partial", "general_full", "partial"])
def test_full_count_one_class_of_the_bitsliced_kernel(eng, monkeypatch, kind, n):
    """count_bitslice3_kernel, one mode per launch: the four THIRD rules of bs3_store (third cell = trees - n0 - n1,
    z - n0 - n1, z) with cells that end at exactly 65 535."""
    tune(monkeypatch, eng, {**ONE_CLASS, _lib.QS_TUNE_FUSE_CLASSES: 0})
    assert_full_count(eng, limit_case(n, kind), [f"gather/{kind}/", "bitslice_b", "!/fused", "!/clamp", "!depth_u", "!coop"])


@pytest.mark.parametrize("fuse", [1, 0])
def test_full_count_fused_launch_and_class_by_class(eng, monkeypatch, fuse):
    """all four modes interleaved in one batch: one launch of count_bitslice3_fused_kernel per depth-bits group, and the same
    batch class by class"""
    tune(monkeypatch, eng, {**ONE_CLASS, _lib.QS_TUNE_FUSE_CLASSES: fuse})
    c = limit_case(70, "mixed")
    ctx, _ = assert_full_count(eng, c, ["gather/mixed/"] + [f"{mo}.bitslice_b" for mo in MODES] + (["/fused:1"] if fuse else ["!/fused"]))


def test_full_count_cooperative_kernel(eng, monkeypatch):
    """count_bitslice4_kernel (QS_TUNE_COOP = 1) takes the tiles with two a-blocks of a binary full batch"""
    tune(monkeypatch, eng, {**ONE_CLASS, _lib.QS_TUNE_COOP: 1})
    assert_full_count(eng, limit_case(70, "binary_full"), ["gather/binary_full/", "bitslice_b", "/coop4"])


@pytest.mark.parametrize("n,kind,panel", [(24, "binary_full", "depth_u8"), (70, "partial", "depth_u8"), (70, "deep", "depth_u16")])
def test_full_count_byte_swar_kernel(eng, monkeypatch, n, kind, panel):
    """the byte-SWAR kernel (QS_IMPL_SWAR) with 8-bit and with 16-bit depth panels (a ladder of 70 taxa: 68 > 63 LCA levels)"""
    tune(monkeypatch, eng, {_lib.QS_TUNE_GATHER_IMPL: _lib.QS_IMPL_SWAR})
    c = limit_case(n, kind)
    if panel == "depth_u16":
        assert int(c.small.adj_depth.max()) > 63
    assert_full_count(eng, c, [panel, "!bitslice"])


@pytest.mark.parametrize("n,kind", [(70, "deep"), (44, "clamp_general")])
def test_full_count_with_clamped_trees(eng, monkeypatch, n, kind):
    """Depth clamp: ladders counted in the 4-bit class. clamp_fix_kernel increments the true cell of every quartet the cut tied
    and, in the binary mode, decrements the third cell where the count kernel parked it -- on cells that end at 65 535 and at 0:
    some unanimous quartet has three leaves below the cut of the first ladder (asserted)."""
    tune(monkeypatch, eng, CLAMP_ALL)
    c = limit_case(n, kind)
    below_cut = np.zeros(n, dtype=bool)                    # leaf i of the ladder's order hangs at depth n - 1 - i: below 15 for i <= n - 16
    below_cut[[c.ref.name_to_id[f"t{x}"] for x in c.ladder_order[: n - 15]]] = True
    quads = taxon_model.quads_in_rank_order(n)
    tied = below_cut[quads].sum(axis=1) >= 3
    full_rows = (c.want == FULL).any(axis=1)
    assert (tied & full_rows).any()
    if kind == "deep":
        assert (tied & full_rows & (c.want[:, 2] == 0)).any()     # ... and its parked third cell is decremented back to 0
    ctx, _ = assert_full_count(eng, c, ["bitslice_b4", "!bitslice_b5", "!bitslice_b6", "!bitslice_b7", "/clamp:",
                                        "gather/binary_full/" if kind == "deep" else "gather/general_full/"])
    assert int(ctx.last_count_variant().split("/clamp:")[1].split("/")[0]) >= 97


@pytest.mark.parametrize("kind", ["binary_full", "partial"])
def test_full_count_scatter(eng, kind):
    """QS_ALGO_SCATTER: packed half-word atomics, at the smallest n only (it is slow by design)"""
    assert_full_count(eng, limit_case(24, kind), ["scatter"], algo=eng.QS_ALGO_SCATTER, with_nodes=True)


@pytest.mark.parametrize("how", ["two_uploads", "five_uploads", "panel_slices"])
def test_full_count_accumulates(eng, monkeypatch, how):
    """the read-modify-write of bs3_store: the same 65 535 trees as two and as five uploads cut at places that are not multiples
    of 32, and as several panel slices per launch"""
    tune(monkeypatch, eng, ONE_CLASS)
    c = limit_case(70, "mixed")
    if how == "panel_slices":
        tune(monkeypatch, eng, {_lib.QS_TUNE_PANEL_SLICE_BYTES: 12 << 20})   # a 32-tree group of 70 taxa is 48 300 or 57 960 bytes: ~10 slices
        pieces = None
    else:
        cuts = [0, 30001, FULL] if how == "two_uploads" else [0, 77, 12345, 12346 + 4097, 50001, FULL]
        assert all(x % 32 for x in cuts[1:-1])
        pieces = list(zip(cuts[:-1], cuts[1:]))
    assert_full_count(eng, c, ["bitslice_b"], pieces=pieces)


def test_full_count_on_a_table_shard(eng, monkeypatch):
    tune(monkeypatch, eng, ONE_CLASS)
    assert_full_count(eng, limit_case(70, "mixed"), ["bitslice_b"], shard=(21, 59))


def test_full_count_straight_into_the_wire_words(eng, monkeypatch):
    """QS_COUNT_WIRE16X2 in two accumulating uploads with clamped trees among them: n0 | n1 << 16 per tuple with halves of 65 535
    next to 0; qs_unpack16x2 gives the oracle's table, qs_table_pack16x2 of the three-cell table the same words."""
    import torch
    tune(monkeypatch, eng, CLAMP_ALL)
    c = limit_case(70, "deep")
    big = big_batch(c)
    nq = ranks.n_quartets(c.n)
    ctx = eng.Context(c.n, 32)                             # no table at all
    words = torch.zeros(nq, dtype=torch.int32, device="cuda")
    ctx.wire_attach(words)
    for lo, hi in ((0, 30001), (30001, FULL)):
        hb = ctx.batch_upload(big.slice(lo, hi), with_nodes=False)
        ctx.count_batch(hb, eng.QS_ALGO_GATHER | eng.QS_COUNT_WIRE16X2)
        ctx.batch_free(hb)
    ctx.sync()
    v = ctx.last_count_variant()
    assert "wire_u16x2" in v and "/clamp:" in v, v
    w = words.cpu().numpy().view(np.uint32)
    assert np.array_equal((w & 0xFFFF).astype(np.uint64), c.want[:, 0]) and np.array_equal((w >> 16).astype(np.uint64), c.want[:, 1])
    out = torch.zeros((nq * 3 + 1) // 2, dtype=torch.int32, device="cuda")
    ctx.unpack16x2(words, nq, FULL, out)
    ctx.sync()
    got = out.cpu().numpy().view(np.uint16)[: nq * 3].reshape(nq, 3)
    assert np.array_equal(got.astype(np.uint64), c.want)
    c32 = count_into(eng, c, big, bits=32)
    c32.sync()
    assert np.array_equal(c32.table_download().astype(np.uint64), c.want)
    packed = torch.full((nq,), -1, dtype=torch.int32, device="cuda")
    c32.table_pack16x2(packed)
    c32.sync()
    assert torch.equal(packed, words)


def test_scores_and_taxon_support_of_full_cells(eng):
    """On a table whose cells and tuple sums reach 65 535 (the last index of the device's log table): the scores equal the
    oracle's to 0 ulp, and qs_taxon_support (32-bit partial sums in the 16-bit instance: 64 x 3 x 65535 < 2^32) equals the
    numpy model."""
    c = limit_case(70, "binary_full")
    ctx = count_into(eng, c, big_batch(c))
    ctx.sync()
    assert np.array_equal(ctx.table_download().astype(np.uint64), c.want)
    lq, qp, eqp, bif = ctx.score(c.ref)
    assert bif
    view = object.__new__(eng.QuartetScoreComputer)       # only to key the three vectors by bipartition like the oracle does
    view.ref, view._lq, view._qp, view._eqp = c.ref, lq[1:], qp[1:], eqp[1:]
    got = view.scores_by_bipartition()
    c.oracle.score()
    want = c.oracle.scores_by_bipartition()
    assert set(got) == set(want) and len(want) == c.n - 3
    for key, ov in want.items():
        for g, o_ in zip(got[key], ov):
            assert int(ulp_diff(g, o_)) == 0, (sorted(key), g, o_)
    assert np.array_equal(ctx.taxon_support(c.ref), taxon_model.model_counts(c.want, c.ref))


# ---- 2. the 65 536th tree is refused and nothing changes --------------------------------------------------------------------

def _refused(eng, fn):
    with pytest.raises(eng.QSError) as ei:
        fn()
    assert ei.value.code == _lib.QS_ERR_OVERFLOW, ei.value
    return ei.value


def test_the_65536th_tree_is_refused(eng):
    import torch
    c = limit_case(24, "binary_full")
    big = big_batch(c, True)
    one = c.small.slice(0, 1)
    nq = ranks.n_quartets(c.n)
    ctx = count_into(eng, c, big, with_nodes=True)
    ctx.sync()
    T = ctx.table_download()
    assert np.array_equal(T.astype(np.uint64), c.want)
    hb = ctx.batch_upload(one)
    for algo in (eng.QS_ALGO_GATHER, eng.QS_ALGO_SCATTER, eng.QS_ALGO_AUTO):
        assert "65535" in str(_refused(eng, lambda: ctx.count_batch(hb, algo)))
        ctx.sync()
        assert ctx.trees_counted == FULL and np.array_equal(ctx.table_download(), T)
    # QS_COUNT_OVERWRITE: the guard ignores what is overwritten
    hbig = ctx.batch_upload(big)
    ctx.count_batch(hbig, eng.QS_ALGO_GATHER | eng.QS_COUNT_OVERWRITE)
    ctx.sync()
    assert ctx.trees_counted == FULL and np.array_equal(ctx.table_download(), T)
    ctx.batch_free(hbig)
    ctx.batch_free(hb)
    # 65 536 trees at once into an empty 16-bit context
    c0 = eng.Context(c.n, 16)
    c0.table_alloc()
    too_many = repeat_trees(c.small, [(0, FULL + 1)], with_nodes=False)
    hb0 = c0.batch_upload(too_many, with_nodes=False)
    _refused(eng, lambda: c0.count_batch(hb0, eng.QS_ALGO_GATHER))
    _refused(eng, lambda: c0.count_batch(hb0, eng.QS_ALGO_GATHER | eng.QS_COUNT_OVERWRITE))
    c0.sync()
    assert c0.trees_counted == 0 and not c0.table_download().any()
    # the wire words
    cw = eng.Context(c.n, 32)
    words = torch.zeros(nq, dtype=torch.int32, device="cuda")
    cw.wire_attach(words)
    W16 = eng.QS_ALGO_GATHER | eng.QS_COUNT_WIRE16X2
    hbw = cw.batch_upload(too_many, with_nodes=False)
    _refused(eng, lambda: cw.count_batch(hbw, W16))
    cw.sync()
    assert not words.any()
    cw.batch_free(hbw)
    hbw = cw.batch_upload(big, with_nodes=False)
    cw.count_batch(hbw, W16)
    cw.sync()
    w = words.cpu().numpy().view(np.uint32).copy()
    assert np.array_equal((w & 0xFFFF).astype(np.uint64), c.want[:, 0]) and np.array_equal((w >> 16).astype(np.uint64), c.want[:, 1])
    hb1 = cw.batch_upload(one, with_nodes=False)
    _refused(eng, lambda: cw.count_batch(hb1, W16))
    cw.sync()
    assert np.array_equal(words.cpu().numpy().view(np.uint32), w)
    cw.count_batch(hbw, W16 | eng.QS_COUNT_OVERWRITE)      # overwriting 65 535 trees with 65 535 trees is fine
    cw.sync()
    assert np.array_equal(words.cpu().numpy().view(np.uint32), w)
    # qs_table_pack16x2 / qs_unpack16x2: 65 535 trees pass, 65 536 do not
    c32 = count_into(eng, c, big, bits=32)
    c32.sync()
    packed = torch.full((nq,), -1, dtype=torch.int32, device="cuda")
    c32.table_pack16x2(packed)
    c32.sync()
    assert np.array_equal(packed.cpu().numpy().view(np.uint32), w)
    out = torch.zeros((nq * 3 + 1) // 2, dtype=torch.int32, device="cuda")
    c32.unpack16x2(packed, nq, FULL, out)
    c32.sync()
    assert np.array_equal(out.cpu().numpy().view(np.uint16)[: nq * 3].reshape(nq, 3).astype(np.uint64), c.want)
    before = out.clone()
    _refused(eng, lambda: c32.unpack16x2(packed, nq, FULL + 1, out))
    c32.count_trees(one)
    assert c32.trees_counted == FULL + 1
    keep = packed.clone()
    _refused(eng, lambda: c32.table_pack16x2(packed))
    c32.sync()
    assert torch.equal(packed, keep) and torch.equal(out, before)


@pytest.mark.parametrize("half", ["low", "high"])
def test_pack16_at_the_limit(eng, half):
    """qs_table_pack16: a cell of 65 535 passes (and arrives), a cell of 65 536 is QS_ERR_OVERFLOW at qs_sync, in the low and in
    the high half of a destination word"""
    import torch
    n = 9
    nq = ranks.n_quartets(n)
    rng = np.random.default_rng(99)
    T = rng.integers(0, 1000, size=(nq, 3)).astype(np.uint32)
    cell = 100 + (half == "high")                          # flat cell index: even = low half of word 50, odd = its high half
    T.reshape(-1)[cell] = FULL
    T.reshape(-1)[cell ^ 1] = 0
    ctx = eng.Context(n, 32)
    ctx.table_alloc()
    ctx.table_upload(T)
    packed = torch.full(((nq * 3 + 1) // 2,), -1, dtype=torch.int32, device="cuda")
    ctx.table_pack16(packed)
    ctx.sync()
    got = packed.cpu().numpy().view(np.uint16)[: nq * 3].reshape(nq, 3)
    assert np.array_equal(got.astype(np.uint32), T)
    T.reshape(-1)[cell] = FULL + 1
    ctx.table_upload(T)
    ctx.table_pack16(packed)
    _refused(eng, ctx.sync)
    ctx.sync()                                             # the flag is cleared once


# ---- 3. a preset table: exact fill passes, one more overflows, on every writer -----------------------------------------------

#           kind of the batch, tuning, algorithm, pieces of the variant
WRITERS = {
    "binary_full": ("binary_full", {**ONE_CLASS, _lib.QS_TUNE_FUSE_CLASSES: 0}, "gather", ["gather/binary_full/", "bitslice_b", "!/fused"]),
    "binary_partial": ("binary_partial", {**ONE_CLASS, _lib.QS_TUNE_FUSE_CLASSES: 0}, "gather", ["gather/binary_partial/", "bitslice_b", "!/fused"]),
    "general_full": ("general_full", {**ONE_CLASS, _lib.QS_TUNE_FUSE_CLASSES: 0}, "gather", ["gather/general_full/", "bitslice_b", "!/fused"]),
    "partial": ("partial", {**ONE_CLASS, _lib.QS_TUNE_FUSE_CLASSES: 0}, "gather", ["gather/partial/", "bitslice_b", "!/fused"]),
    "fused": ("mixed", {**ONE_CLASS, _lib.QS_TUNE_FUSE_CLASSES: 1}, "gather", ["gather/mixed/", "/fused:1"]),
    "coop": ("binary_full", {**ONE_CLASS, _lib.QS_TUNE_COOP: 1}, "gather", ["/coop4"]),
    "swar": ("mixed", {_lib.QS_TUNE_GATHER_IMPL: _lib.QS_IMPL_SWAR, _lib.QS_TUNE_DEPTH_CLAMP: 0}, "gather", ["depth_u8", "!bitslice"]),
    "scatter": ("mixed", {_lib.QS_TUNE_DEPTH_CLAMP: 0}, "scatter", ["scatter"]),
}
N_PRESET = 40
TARGETS = ["first_tuple", "last_tuple", "slot0_low", "slot0_high", "slot1_low", "slot1_high", "slot2_low", "slot2_high"]


def _writer(eng, monkeypatch, name):
    kind, settings, algo, expect = WRITERS[name]
    tune(monkeypatch, eng, settings)
    c = small_case(N_PRESET, kind)
    scatter = algo == "scatter"
    return c, dict(algo=eng.QS_ALGO_SCATTER if scatter else eng.QS_ALGO_GATHER, with_nodes=scatter), expect


def _check_variant(ctx, expect):
    v = ctx.last_count_variant()
    for piece in expect + ["!/clamp"]:
        assert (piece[1:] not in v) if piece.startswith("!") else (piece in v), (piece, v)


def _target_cell(W, target):
    """flat index of a cell the batch increments (W > 0): in the first / last tuple, or the first one in the given slot that
    sits in the low (even flat index) / high half of its 32-bit word"""
    if target in ("first_tuple", "last_tuple"):
        r = 0 if target == "first_tuple" else len(W) - 1
        slots = np.nonzero(W[r] > 0)[0]
        assert len(slots), (target, W[r])
        return 3 * r + int(slots[0])
    slot, half = int(target[4]), target.endswith("high")
    rows = np.nonzero((W[:, slot] > 0) & (((3 * np.arange(len(W)) + slot) & 1) == int(half)))[0]
    assert len(rows), target
    r = int(rows[len(rows) // 2])
    return 3 * r + slot


@pytest.mark.parametrize("writer", list(WRITERS))
def test_exact_fill_passes(eng, monkeypatch, writer):
    """Every cell preset to 65 535 minus what the batch adds: qs_sync raises nothing and every cell ends at 65 535 -- a check
    that says >= where it means > fails here. Only paths without clamped trees (QS_TUNE_DEPTH_CLAMP = 0, no /clamp in the
    variant): with clamped binary trees the count kernel parks tied quartets in the third cell before clamp_fix_kernel moves
    them, so that cell is legitimately above its final value for a moment; those paths are covered by
    test_full_count_with_clamped_trees and test_full_count_straight_into_the_wire_words instead."""
    c, kw, expect = _writer(eng, monkeypatch, writer)
    preset = (FULL - c.want).astype(np.uint16)
    ctx = count_into(eng, c, c.small, preset=preset, **kw)
    ctx.sync()
    _check_variant(ctx, expect)
    T = ctx.table_download()
    assert (T == FULL).all(), (int((T != FULL).sum()), ctx.last_count_variant())
    assert ctx.trees_counted == c.total


@pytest.mark.parametrize("writer", [w for w in WRITERS if w != "scatter"])
def test_exact_fill_of_32_bit_cells_passes(eng, monkeypatch, writer):
    c, kw, expect = _writer(eng, monkeypatch, writer)
    top = np.uint64(2 ** 32 - 1)
    ctx = count_into(eng, c, c.small, bits=32, preset=(top - c.want).astype(np.uint32), **kw)
    ctx.sync()
    assert (ctx.table_download() == np.uint32(top)).all()


def _assert_one_over(eng, c, flat, expect, clamp=False, **kw):
    preset = (FULL - c.want).astype(np.uint16)
    assert c.want.reshape(-1)[flat] > 0
    preset.reshape(-1)[flat] += 1                          # at most 65 535: the batch adds at least one here
    ctx = count_into(eng, c, c.small, preset=preset, **kw)
    v = ctx.last_count_variant()
    with pytest.raises(eng.QSError) as ei:
        ctx.sync()
    assert ei.value.code == _lib.QS_ERR_OVERFLOW, (v, ei.value)
    if clamp:
        assert "/clamp:1" in v, v
    else:
        _check_variant(ctx, expect)
    ctx.sync()                                             # the flag is cleared once
    ctx.table_upload(np.zeros_like(preset))                # ... and the context still counts correctly
    ctx2 = ctx
    hb = ctx2.batch_upload(c.small, with_nodes=kw.get("with_nodes", False))
    ctx2.count_batch(hb, kw.get("algo", eng.QS_ALGO_GATHER))
    ctx2.sync()
    ctx2.batch_free(hb)
    assert np.array_equal(ctx2.table_download().astype(np.uint64), c.want)


@pytest.mark.parametrize("target", TARGETS)
@pytest.mark.parametrize("writer", list(WRITERS))
def test_one_over_is_an_overflow(eng, monkeypatch, writer, target):
    """The exact fill plus one in a single cell the batch increments: QS_ERR_OVERFLOW at qs_sync (once), whichever half of its
    word, slot or end of the table the cell sits in."""
    c, kw, expect = _writer(eng, monkeypatch, writer)
    _assert_one_over(eng, c, _target_cell(c.want, target), expect, **kw)


@functools.lru_cache(maxsize=None)
def clamp_case():
    """One ladder of 44 taxa with a trifurcation at its tip (general_full, 42 LCA levels, not re-rooted) among 12 random
    multifurcating trees that fit 4 depth bits: the ladder is counted in their class with its depths cut at 15, and the
    quartets with three leaves below the cut are added by clamp_fix_kernel alone. Returns the case and the flat cells that
    only the correction increments: such a quartet of the ladder, in a cell no other tree of the batch touches."""
    n, seed = 44, 4470
    ref_nw = synth.reference_tree(n, seed)
    ref = flatten.flatten_reference(ref_nw)
    rng = np.random.default_rng(seed + 1)
    order = [int(x) for x in rng.permutation(n)]
    ladder = _ladder(n, order).replace("(((t", "((t", 1).replace("),", ",", 1)
    rest = synth.tree_set(n, 12, seed + 2, collapse=0.15)
    a = flatten.flatten_eval_trees([ladder], ref.name_to_id, recentre=False)
    b = flatten.flatten_eval_trees(rest, ref.name_to_id)
    assert int(a.adj_depth.max()) == n - 3 and int(b.adj_depth.max()) <= 15
    small = concat_batches(a, b)
    # the class plan the upload applies (host arithmetic): the ladder joins the 4-bit general_full class
    L = _lib.load()
    mode, bits = np.zeros(small.n_trees, np.uint8), np.zeros(small.n_trees, np.uint8)
    s = _lib.TreeBatchC(small.n_trees, small.leaf_off.ctypes.data, small.leaf_ids.ctypes.data, small.adj_depth.ctypes.data, None, None, None)
    assert L.qs_class_plan(n, C.byref(s), 1, 0 | _lib.QS_CLASS_PLAN_FUSED, 1000000, mode.ctypes.data, bits.ctypes.data, None) == 0
    assert (mode == 1).all() and (bits == 4).all(), (mode, bits)
    o_l, o_r, o = Oracle(ref_nw), Oracle(ref_nw), Oracle(ref_nw)
    o_l.count(ladder)
    o_r.count("\n".join(rest))
    o.count("\n".join([ladder] + rest))
    W_l, W_r = o_l.counts(), o_r.counts()
    # the run of the cut: tour positions joined by adjacent LCA depths >= 15
    deep = a.adj_depth[: n - 1] >= 15
    in_run = np.zeros(n, dtype=bool)
    in_run[a.leaf_ids[np.nonzero(deep)[0]]] = True
    in_run[a.leaf_ids[np.nonzero(deep)[0] + 1]] = True
    assert 3 <= int(in_run.sum()) <= 128 and np.all(np.diff(np.nonzero(deep)[0]) == 1)       # one run
    tied = in_run[taxon_model.quads_in_rank_order(n)].sum(axis=1) >= 3
    only_fix = np.nonzero(((W_l == 1) & (W_r == 0) & tied[:, None]).reshape(-1))[0]
    assert len(only_fix) >= 2
    c = SimpleNamespace(n=n, kind="clamp_general", ref=ref, small=small, total=small.n_trees, want=o.counts().copy())
    return c, only_fix


@pytest.mark.parametrize("half", ["low", "high"])
def test_one_over_in_a_cell_only_the_clamp_correction_increments(eng, monkeypatch, half):
    """clamp_fix_kernel's packed half-word atomics: a cell at 65 535 that only the correction of a clamped tree increments."""
    tune(monkeypatch, eng, CLAMP_ALL)
    c, only_fix = clamp_case()
    cells = only_fix[(only_fix & 1) == (half == "high")]
    assert len(cells)
    _assert_one_over(eng, c, int(cells[len(cells) // 2]), [], clamp=True)
