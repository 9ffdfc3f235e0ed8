"""Split slices of the count step (QS_TUNE_FIX_OVERLAP): a slice whose trees carry depth-clamp corrections is counted in two launches
split at a largest id d_mid, the corrections of [d_mid, d_hi) on a second stream beside the count launch of [d_lo, d_mid). The table
must be bit for bit the one the single launch gives (switch at 0) and the oracle's, whatever d_mid is.

Shapes: 40 taxa, 70-odd trees (three 32-tree groups), ladders and ladder + NNI trees clamped from 6 depth bits to 4 among random
trees, so that correction runs exist on both sides of every d_mid tried; d_mid forced (QS_TUNE_FIX_SPLIT_AT) to d_lo + 1 (the lower
range is empty), to the middle, and to d_hi - 1 (the upper range is a single largest id)."""
import numpy as np
import pytest

from helpers import repeat_trees
from oracle_api import Oracle
from quartetscores_amd import _lib, flatten, ranks, synth

pytestmark = pytest.mark.gpu
N = 40


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    from quartetscores_amd import engine
    return engine


def _ladder(n, order):
    cat = f"(t{order[0]},t{order[1]})"
    for i in order[2:]:
        cat = "(" + cat + f",t{i})"
    return cat + ";"


def _concat(a, b):
    return flatten.TreeBatch(
        a.n_trees + b.n_trees,
        np.concatenate([a.leaf_off, b.leaf_off[1:] + a.leaf_off[-1]]).astype(np.uint32),
        np.concatenate([a.leaf_ids, b.leaf_ids]), np.concatenate([a.adj_depth, b.adj_depth]),
        np.concatenate([a.node_off, b.node_off[1:] + a.node_off[-1]]).astype(np.uint32),
        np.concatenate([a.rng_off, b.rng_off[1:] + a.rng_off[-1]]).astype(np.uint32),
        np.concatenate([a.ranges, b.ranges]))


_CASES = {}


def case(kind):
    """(reference, batch, oracle table) of a tree set, built once. Deep trees are flattened as they are (not re-rooted), so that the
    clamp to 4 bits cuts a run of some 25 leaves out of each."""
    if kind in _CASES:
        return _CASES[kind]
    ref_nw = synth.reference_tree(N, 4000)
    ref = flatten.flatten_reference(ref_nw)
    rng = np.random.default_rng(40)
    if kind == "ladder_top":      # the runs hold the ids 39 .. 14: every correction's largest id is at least 16
        deep = [_ladder(N, list(range(N - 1, -1, -1)))] * 3
        rest = synth.tree_set(N, 64, 4003)
    else:
        kw = {"binary_full": {}, "general_full": {"collapse": 0.2}, "binary_partial": {"dropout": 0.1}, "mixed": {}}[kind]
        deep = [_ladder(N, [int(x) for x in rng.permutation(N)]) for _ in range(3)]
        deep += synth.nni_tree_set(deep[0], 12, 4001, mean_nni=5)
        if kind == "general_full":   # multifurcations inside the cut subtrees as well
            deep += [t.replace("(((t", "((t", 1).replace("),", ",", 1) for t in deep[:3]]
        rest = synth.tree_set(N, 56, 4002, **kw)
        if kind == "mixed":          # four modes at 4 depth bits: one fused launch
            rest = rest[:20] + synth.tree_set(N, 16, 4004, collapse=0.2) + synth.tree_set(N, 12, 4005, dropout=0.1) + synth.tree_set(N, 8, 4006, collapse=0.2, dropout=0.1)
    h = (len(deep) + 1) // 2      # deep trees at both ends of the batch: corrections in its first and in its last panel slice
    trees = deep[:h] + rest + deep[h:]
    batch = _concat(_concat(flatten.flatten_eval_trees(deep[:h], ref.name_to_id, recentre=False), flatten.flatten_eval_trees(rest, ref.name_to_id)),
                    flatten.flatten_eval_trees(deep[h:], ref.name_to_id, recentre=False))
    o = Oracle(ref_nw)
    o.count("\n".join(trees), nthreads=4)
    want = o.counts()
    want.setflags(write=False)
    _CASES[kind] = (ref, batch, want)
    return _CASES[kind]


def context(eng, count_bits, overlap, split_at=0, d_lo=0, d_hi=0, slice_bytes=0, clamp=1000000, impl=None, n=N):
    ctx = eng.Context(n, count_bits, d_lo=d_lo, d_hi=d_hi)
    ctx.set_tuning(_lib.QS_TUNE_DEPTH_CLAMP, clamp)     # any price per bit
    ctx.set_tuning(_lib.QS_TUNE_CLASS_MIN_TREES, 1)
    ctx.set_tuning(_lib.QS_TUNE_CLASS_PCT, 0)
    ctx.set_tuning(_lib.QS_TUNE_FIX_OVERLAP, overlap)
    ctx.set_tuning(_lib.QS_TUNE_FIX_SPLIT_AT, split_at)
    if slice_bytes:
        ctx.set_tuning(_lib.QS_TUNE_PANEL_SLICE_BYTES, slice_bytes)
    if impl is not None:
        ctx.set_tuning(_lib.QS_TUNE_GATHER_IMPL, impl)
    return ctx


def overwrite_then_accumulate(eng, ctx, batch, timed=False):
    """The table after an overwriting count over stale contents, and after a second, accumulating one; the split of each."""
    ctx.table_alloc()
    stale = np.full((ctx.table_tuples, 3), 321, dtype=np.uint32 if ctx.count_bits == 32 else np.uint16)
    ctx.table_upload(stale)
    hb = ctx.batch_upload(batch, with_nodes=False)
    assert ctx.batch_clamp_info(hb)[0] > 0
    flag = eng.QS_COUNT_TIMED if timed else 0
    ctx.count_batch(hb, eng.QS_ALGO_GATHER | eng.QS_COUNT_OVERWRITE | flag)
    ctx.sync()
    s1, v1 = ctx.last_count_split(), ctx.last_count_variant()
    T1 = ctx.table_download()
    ctx.count_batch(hb, eng.QS_ALGO_GATHER | flag)
    ctx.sync()
    s2 = ctx.last_count_split()
    T2 = ctx.table_download()
    assert ctx.trees_counted == 2 * batch.n_trees
    ctx.batch_free(hb)
    return T1, T2, s1, s2, v1


_SERIAL = {}


def serial_tables(eng, kind, count_bits):
    """The switch at 0: one count launch, then the corrections (shared by the cases below)."""
    key = (kind, count_bits)
    if key not in _SERIAL:
        _, batch, want = case(kind)
        T1, T2, s1, s2, v1 = overwrite_then_accumulate(eng, context(eng, count_bits, 0), batch)
        assert s1 == (0, 0) and s2 == (0, 0) and "/overlap" not in v1 and "/clamp:" in v1, v1
        assert (T1.astype(np.uint64) == want).all()
        for T in (T1, T2):
            T.setflags(write=False)
        _SERIAL[key] = (T1, T2)
    return _SERIAL[key]


@pytest.mark.parametrize("split_at", [1, 3, 4, 16, 24, 33, N - 1])
@pytest.mark.parametrize("count_bits", [32, 16])
@pytest.mark.parametrize("kind", ["binary_full", "binary_partial", "general_full", "mixed", "ladder_top"])
def test_split_slices_equal_the_single_launch_and_the_oracle(eng, kind, count_bits, split_at):
    """Overwrite, then accumulate, with d_mid forced: d_lo + 1 and the ids below 4 (nothing in the lower range), the middle (24: d-blocks
    aligned to d_hi, 33 and 16: not aligned; at 16 the ladder_top set has every correction in the upper range) and d_hi - 1."""
    _, batch, want = case(kind)
    S1, S2 = serial_tables(eng, kind, count_bits)
    T1, T2, s1, s2, v1 = overwrite_then_accumulate(eng, context(eng, count_bits, 1, split_at), batch)
    assert s1[0] == split_at and s1[1] >= 1 and s2 == s1 and v1.endswith(f"/overlap:{split_at}"), (s1, s2, v1)
    if kind == "mixed":
        assert "/fused:1" in v1, v1
    assert (T1.astype(np.uint64) == want).all()
    assert (T1 == S1).all() and (T2 == S2).all() and (T2.astype(np.uint64) == 2 * want).all()


@pytest.mark.parametrize("count_bits", [32, 16])
@pytest.mark.parametrize("kind", ["binary_full", "mixed"])
def test_split_slices_with_two_panel_slices_and_timing(eng, kind, count_bits):
    """Two 32-tree groups per panel slice: every slice with corrections is split, a later slice's accumulating launches follow the
    corrections of the one before. With QS_COUNT_TIMED the events sit on the stream their kernel ran on: the call still reports panel,
    count and correction time, and the two count launches of a split slice are one launch in the count."""
    _, batch, want = case(kind)
    S1, S2 = serial_tables(eng, kind, count_bits)
    slice_bytes = (N * (N - 1) // 2) * 5 * 4 * 2      # (groups of up to 5 words per pair)
    ref_ctx = context(eng, count_bits, 0, slice_bytes=slice_bytes)
    R1, _, _, _, _ = overwrite_then_accumulate(eng, ref_ctx, batch, timed=True)
    launches = ref_ctx.last_count_launches()
    ctx = context(eng, count_bits, 1, 24, slice_bytes=slice_bytes)
    T1, T2, s1, s2, v1 = overwrite_then_accumulate(eng, ctx, batch, timed=True)
    assert s1[0] == 24 and s1[1] >= (2 if kind == "binary_full" else 1) and s2 == s1, (s1, s2, v1)
    assert (R1 == S1).all() and (T1 == S1).all() and (T2 == S2).all()
    panel_ms, count_ms, total_ms = ctx.last_count_ms()
    assert panel_ms > 0 and count_ms > 0 and total_ms > 0 and ctx.last_count_fix_ms() > 0
    assert ctx.last_count_launches() == launches >= 2
    kinds = [k for k, _ in ctx.last_count_events()]
    assert kinds.count("count") == launches + s1[1] and kinds.count("fix") >= 2 * s1[1] and all(ms >= 0 for _, ms in ctx.last_count_events())


@pytest.mark.parametrize("split_at", [18, 30, N - 1])
@pytest.mark.parametrize("count_bits", [32, 16])
def test_split_slices_on_a_table_shard(eng, count_bits, split_at):
    """A context that owns the largest ids [17, 40) only."""
    _, batch, want = case("binary_full")
    d_lo = 17
    lo_tuples = ranks.n_quartets(d_lo)
    tables = []
    for overlap, at in ((0, 0), (1, split_at)):
        ctx = context(eng, count_bits, overlap, at, d_lo=d_lo, d_hi=N)
        T1, T2, s1, _, _ = overwrite_then_accumulate(eng, ctx, batch)
        assert s1[0] == at
        assert (T1.astype(np.uint64) == want[lo_tuples:]).all() and (T2.astype(np.uint64) == 2 * want[lo_tuples:]).all()
        tables.append((T1, T2))
    assert (tables[0][0] == tables[1][0]).all() and (tables[0][1] == tables[1][1]).all()


@pytest.mark.parametrize("split_at", [1, 24, N - 1])
def test_split_slices_in_the_wire_format(eng, split_at):
    """QS_COUNT_WIRE16X2: both count launches and both correction launches write the wire words."""
    import torch
    _, batch, want = case("binary_full")
    words = []
    for overlap, at in ((0, 0), (1, split_at)):
        ctx = context(eng, 32, overlap, at)
        w = torch.full((ctx.table_tuples,), 77, dtype=torch.int32, device="cuda")
        ctx.wire_attach(w)
        hb = ctx.batch_upload(batch, with_nodes=False)
        ctx.count_batch(hb, eng.QS_ALGO_GATHER | eng.QS_COUNT_WIRE16X2 | eng.QS_COUNT_OVERWRITE)
        ctx.count_batch(hb, eng.QS_ALGO_GATHER | eng.QS_COUNT_WIRE16X2)
        ctx.sync()
        v = ctx.last_count_variant()
        assert ctx.last_count_split()[0] == at and "wire_u16x2" in v and ("/overlap:" in v) == bool(overlap), v
        ctx.batch_free(hb)
        words.append(w.cpu().numpy().view(np.uint32))
    assert (words[0] == words[1]).all()
    assert ((words[0] & 0xFFFF) == 2 * want[:, 0]).all() and ((words[0] >> 16) == 2 * want[:, 1]).all()


def test_no_split_fallbacks_give_the_single_launch(eng):
    """One count launch per slice: the switch at 0, no corrections (no clamp), the byte-SWAR kernel, a forced d_mid outside the
    shard, and -- with d_mid planned -- a lower launch below one wave population of tiles (40 taxa hold 1 500 tiles in all) or a
    d-range too short to split."""
    _, batch, want = case("binary_full")
    configs = [dict(overlap=0, split_at=24), dict(overlap=1, split_at=24, clamp=0), dict(overlap=1, split_at=24, impl=_lib.QS_IMPL_SWAR),
               dict(overlap=1, split_at=N), dict(overlap=1, split_at=0), dict(overlap=1, split_at=0, d_lo=N - 10, d_hi=N),
               dict(overlap=1, split_at=5, d_lo=17, d_hi=N)]
    for kw in configs:
        ctx = context(eng, 32, **kw)
        ctx.table_alloc()
        hb = ctx.batch_upload(batch, with_nodes=False)
        ctx.count_batch(hb, eng.QS_ALGO_GATHER | eng.QS_COUNT_TIMED)
        ctx.sync()
        v = ctx.last_count_variant()
        assert ctx.last_count_split() == (0, 0) and "/overlap" not in v, (kw, v)
        assert [k for k, _ in ctx.last_count_events()].count("count") == ctx.last_count_launches(), (kw, v)
        lo = ranks.n_quartets(kw.get("d_lo", 0))
        assert (ctx.table_download().astype(np.uint64) == want[lo:]).all(), kw
        ctx.batch_free(hb)


def test_the_scatter_algorithm_is_never_split(eng):
    """QS_ALGO_SCATTER has neither slices nor corrections: one launch, whatever the switch and the forced d_mid say."""
    ref, batch, want = case("binary_full")
    ctx = context(eng, 32, 1, 24)
    ctx.table_alloc()
    hb = ctx.batch_upload(batch)
    ctx.count_batch(hb, eng.QS_ALGO_SCATTER | eng.QS_COUNT_TIMED)
    ctx.sync()
    v = ctx.last_count_variant()
    assert ctx.last_count_split() == (0, 0) and v.startswith("scatter/") and "/overlap" not in v and ctx.last_count_launches() == 1, v
    assert (ctx.table_download().astype(np.uint64) == want).all()
    ctx.batch_free(hb)


_PLANNED = {}


def planned_case(n):
    """Random trees flattened as they are, copied until the slice is large enough for the planner to find a lower launch that holds
    a wave population of tiles and stays below 40 % of the count.
    156 taxa: 32 distinct trees, 32 copies (32 groups); one tree needs 5 depth bits and is cut to 4 (609 corrections).
    204 taxa (the XCD remap of the count kernel starts at 200): 32 distinct trees, 16 copies (16 groups); four are cut (5 202 corrections).
    No oracle table at these sizes (it takes 5 s and more): the table is compared with the single launch's, which the 40-taxon cases
    above hold against the oracle, and the rows of binary trees with all taxa sum to the tree count."""
    if n not in _PLANNED:
        copies, seed, swap = {156: (32, 8, 14), 204: (16, 10, 21)}[n]
        ref_nw = synth.reference_tree(n, 7)
        ref = flatten.flatten_reference(ref_nw)
        trees = synth.tree_set(n, 32, seed)
        trees[swap] = trees[0]        # (the tree with the most corrections: with it the lower launch would have to be too large)
        one = flatten.flatten_eval_trees(trees, ref.name_to_id, recentre=False)
        assert 16 <= int(one.adj_depth.max()) < 32
        _PLANNED[n] = repeat_trees(one, [(t, 1) for t in range(len(trees))] * (copies * 32 // len(trees)), with_nodes=False)
    return _PLANNED[n]


@pytest.mark.parametrize("n,count_bits", [(156, 32), (156, 16), (204, 16)])
def test_the_planned_split_gives_the_same_table(eng, n, count_bits):
    """No forced d_mid: qs_fix_overlap_plan chooses it, the upper launch order is the shard's filtered on the device, the lower one
    is enumerated for its own tiling. d-blocks aligned to d_hi with 32-bit cells; with 16-bit cells C(d,4) is odd at those ids
    (156 mod 8 = 204 mod 8 = 4), so the split sits half a block higher and the upper range starts at a 32-bit word. A second count
    of the same context keeps the split (and its launch orders)."""
    batch = planned_case(n)
    tables = []
    for overlap in (0, 1):
        ctx = context(eng, count_bits, overlap, n=n)
        ctx.table_alloc()
        hb = ctx.batch_upload(batch, with_nodes=False)
        assert ctx.batch_clamp_info(hb)[0] >= batch.n_trees // 32
        ctx.count_batch(hb, eng.QS_ALGO_GATHER | eng.QS_COUNT_OVERWRITE)
        ctx.sync()
        d_mid, slices = ctx.last_count_split()
        if overlap:
            assert slices == 1 and 3 < d_mid < n and (n - d_mid) % 8 == (0 if count_bits == 32 else 4), (d_mid, slices)
            assert count_bits == 32 or ranks.n_quartets(d_mid) % 2 == 0
            assert ctx.last_count_variant().endswith(f"/overlap:{d_mid}")
        else:
            assert (d_mid, slices) == (0, 0)
        tables.append(ctx.table_download())
        if overlap:
            ctx.count_batch(hb, eng.QS_ALGO_GATHER | eng.QS_COUNT_OVERWRITE)
            ctx.sync()
            assert ctx.last_count_split() == (d_mid, 1) and (ctx.table_download() == tables[1]).all()
        ctx.batch_free(hb)
    assert (tables[0] == tables[1]).all()
    assert (tables[1].sum(axis=1, dtype=np.uint64) == batch.n_trees).all()
