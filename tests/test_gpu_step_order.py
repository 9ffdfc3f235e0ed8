"""The two orders of the 32-tree step of count_bitslice3_kernel (QS_TUNE_STEP_ORDER): 1 = prefetch (the next group's panel elements
are requested at the top of the step), 2 = late loads (requested behind the step's first planes, one set of pair registers;
binary_full classes of 4 and 5 depth bits, five waves per SIMD). Both are the same arithmetic: the tables must agree bit for bit, and with the oracle's.

Shapes: 40 taxa -- the smallest tiling in which every instance of the step occurs (checked in tests/test_step_order_tiles.py with the
arithmetic of bs3_decode_tile): both a-columns with all eight d slots live, both a-columns with a cut d-block, one a-block only, diagonal; the shard
[13, 38) adds a d-block below 8 wide. Tree counts 20, 33, 64, 70 and 97 = 1, 2, 2, 3 and 4 groups of 32 trees, the last one partly
filled: the single group (no loop trip, the peeled step alone), the even loop (2, 4 groups) and the peeled odd last step (3 groups)."""
import numpy as np
import pytest

from oracle_api import Oracle
from quartetscores_amd import _lib, flatten, ranks, synth

pytestmark = pytest.mark.gpu
N = 40
PREFETCH, LATE = 1, 2


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    from quartetscores_amd import engine
    return engine


_TREES = {}


def tree_case(kind, m):
    """(reference newick, trees, flattened batch, oracle table), built once per case and left unchanged."""
    key = (kind, m)
    if key in _TREES:
        return _TREES[key]
    ref_nw = synth.reference_tree(N, 4100)
    ref = flatten.flatten_reference(ref_nw)
    recentre = True
    if kind == "b4":          # random binary trees on all taxa: LCA depths 5 .. 9 -> the 4-bit class
        trees = synth.tree_set(N, m, 5100 + m)
    elif kind == "b5":        # a caterpillar and NNI neighbours, re-centred: LCA depths 16 .. 19 -> the 5-bit class
        lad = f"(t{N - 2},t{N - 1})"
        for i in range(N - 3, -1, -1):
            lad = f"(t{i},{lad})"
        trees = [lad + ";"] + list(synth.nni_tree_set(lad + ";", m - 1, 5200 + m))
    elif kind == "clamped":   # the same deep trees, not re-centred (6 bits), among random ones: clamped to 4 bits, corrections on both sides of any split
        rng = np.random.default_rng(41)
        deep = []
        for _ in range(4):
            order = [int(x) for x in rng.permutation(N)]
            cat = f"(t{order[0]},t{order[1]})"
            for i in order[2:]:
                cat = "(" + cat + f",t{i})"
            deep.append(cat + ";")
        trees = deep[:2] + synth.tree_set(N, m - 4, 5300 + m) + deep[2:]
        recentre = False
    else:                     # "mixed": the four kernel modes at 4 depth bits -> one fused launch
        trees = (synth.tree_set(N, m - 36, 5400) + synth.tree_set(N, 16, 5401, collapse=0.2) + synth.tree_set(N, 12, 5402, dropout=0.1)
                 + synth.tree_set(N, 8, 5403, collapse=0.2, dropout=0.1))
    batch = flatten.flatten_eval_trees(trees, ref.name_to_id, recentre=recentre)
    o = Oracle(ref_nw)
    o.count("\n".join(trees), nthreads=4)
    want = o.counts()
    o.close()
    want.setflags(write=False)
    _TREES[key] = (ref_nw, trees, batch, want)
    return _TREES[key]


def context(eng, count_bits, order, d_lo=0, d_hi=0, n=N, **tuning):
    ctx = eng.Context(n, count_bits, d_lo=d_lo, d_hi=d_hi)
    ctx.set_tuning(_lib.QS_TUNE_STEP_ORDER, order)
    for k_, v_ in tuning.items():
        ctx.set_tuning(getattr(_lib, k_), v_)
    return ctx


def count_twice(eng, ctx, batch):
    """The table after an overwriting count over stale contents and after a second, accumulating one; the variant of the first."""
    ctx.table_alloc()
    ctx.table_upload(np.full((ctx.table_tuples, 3), 321, dtype=np.uint32 if ctx.count_bits == 32 else np.uint16))
    hb = ctx.batch_upload(batch, with_nodes=False)
    ctx.count_batch(hb, eng.QS_ALGO_GATHER | eng.QS_COUNT_OVERWRITE)
    ctx.sync()
    variant = ctx.last_count_variant()
    T1 = ctx.table_download()
    ctx.count_batch(hb, eng.QS_ALGO_GATHER)
    ctx.sync()
    T2 = ctx.table_download()
    ctx.batch_free(hb)
    ctx.close()
    return T1, T2, variant


def both_orders(eng, batch, want, count_bits, bits_name, d_lo=0, d_hi=0, **tuning):
    """Count under both orders; late == prefetch bit for bit (overwrite and accumulate), late == the oracle. Returns the two variants."""
    P1, P2, vp = count_twice(eng, context(eng, count_bits, PREFETCH, d_lo, d_hi, **tuning), batch)
    L1, L2, vl = count_twice(eng, context(eng, count_bits, LATE, d_lo, d_hi, **tuning), batch)
    assert "/late" not in vp and f"bitslice_{bits_name}x2" in vp, vp
    assert "/late5" in vl and f"bitslice_{bits_name}x2" in vl, vl
    assert (L1 == P1).all() and (L2 == P2).all(), (vp, vl)
    rows = want[ranks.n_quartets(d_lo): ranks.n_quartets(d_hi or N)]
    assert L1.shape == rows.shape
    assert (L1.astype(np.uint64) == rows).all() and (L2.astype(np.uint64) == 2 * rows).all(), vl
    return vp, vl


@pytest.mark.parametrize("count_bits", [32, 16])
@pytest.mark.parametrize("m", [20, 33, 64, 70, 97])
def test_late_equals_prefetch_and_the_oracle_at_four_bits(eng, m, count_bits):
    _, _, batch, want = tree_case("b4", m)
    both_orders(eng, batch, want, count_bits, "b4", QS_TUNE_DEPTH_CLAMP=0)


@pytest.mark.parametrize("count_bits", [32, 16])
def test_late_equals_prefetch_and_the_oracle_at_five_bits(eng, count_bits):
    _, _, batch, want = tree_case("b5", 70)
    both_orders(eng, batch, want, count_bits, "b5", QS_TUNE_DEPTH_CLAMP=0)


@pytest.mark.parametrize("count_bits", [32, 16])
def test_late_through_a_shard_with_a_narrow_d_block(eng, count_bits):
    _, _, batch, want = tree_case("b4", 70)
    both_orders(eng, batch, want, count_bits, "b4", d_lo=13, d_hi=38, QS_TUNE_DEPTH_CLAMP=0)


@pytest.mark.parametrize("count_bits", [32, 16])
def test_late_with_clamped_trees_and_a_split_launch(eng, count_bits):
    """Deep trees clamped to 4 bits, the slice split at d_mid = 24: both count launches run the late instance, the corrections of the upper
    range beside the lower launch."""
    _, _, batch, want = tree_case("clamped", 70)
    tuning = dict(QS_TUNE_DEPTH_CLAMP=1000000, QS_TUNE_CLASS_MIN_TREES=1, QS_TUNE_CLASS_PCT=0, QS_TUNE_FIX_OVERLAP=1, QS_TUNE_FIX_SPLIT_AT=24)
    vp, vl = both_orders(eng, batch, want, count_bits, "b4", **tuning)
    for v in (vp, vl):
        assert "/clamp:" in v and v.endswith("/overlap:24"), v


def test_late_into_the_wire_format(eng):
    """QS_COUNT_WIRE16X2: one word n0 | n1 << 16 per tuple, overwrite then accumulate; the words of the two orders agree, unpacked they are
    the oracle's table."""
    import torch
    _, _, batch, want = tree_case("b4", 70)
    dev = torch.device("cuda", 0)
    words = {}
    for order in (PREFETCH, LATE):
        ctx = context(eng, 32, order, QS_TUNE_DEPTH_CLAMP=0)
        nt = ctx.table_tuples
        wire = torch.full((nt,), 0x7FFFFFFF, dtype=torch.int32, device=dev)
        ctx.wire_attach(wire)
        hb = ctx.batch_upload(batch, with_nodes=False)
        ctx.count_batch(hb, eng.QS_ALGO_GATHER | eng.QS_COUNT_WIRE16X2 | eng.QS_COUNT_OVERWRITE)
        ctx.count_batch(hb, eng.QS_ALGO_GATHER | eng.QS_COUNT_WIRE16X2)
        ctx.sync()
        variant = ctx.last_count_variant()
        assert ("/late5" in variant) == (order == LATE) and "/wire_u16x2" in variant, variant
        out = torch.zeros((nt * 6 + 3) // 4, dtype=torch.int32, device=dev)
        ctx.unpack16x2(wire, nt, 2 * batch.n_trees, out)
        ctx.sync()
        words[order] = (wire.cpu().numpy().copy(), out.cpu().numpy().view(np.uint16)[: nt * 3].reshape(-1, 3).astype(np.uint64))
        ctx.batch_free(hb)
        ctx.close()
    assert (words[LATE][0] == words[PREFETCH][0]).all()
    assert (words[LATE][1] == 2 * want).all()


@pytest.mark.parametrize("count_bits", [32, 16])
def test_fused_launch_agrees_with_class_by_class_under_late(eng, count_bits):
    """A batch of all four kernel modes with the knob at 2: the fused kernels (which keep the prefetch order) and class-by-class counting
    (whose binary_full class runs the late instance) give the same table, the oracle's."""
    _, _, batch, want = tree_case("mixed", 76)
    tuning = dict(QS_TUNE_DEPTH_CLAMP=0, QS_TUNE_CLASS_MIN_TREES=1, QS_TUNE_CLASS_PCT=0)
    F1, F2, vf = count_twice(eng, context(eng, count_bits, LATE, QS_TUNE_FUSE_CLASSES=1, **tuning), batch)
    C1, C2, vc = count_twice(eng, context(eng, count_bits, LATE, QS_TUNE_FUSE_CLASSES=0, **tuning), batch)
    assert "/fused:1" in vf and "/late" not in vf, vf
    assert "/fused" not in vc and "/late5" in vc and "binary_full.bitslice_b4x2" in vc, vc
    assert (F1 == C1).all() and (F2 == C2).all()
    assert (C1.astype(np.uint64) == want).all() and (C2.astype(np.uint64) == 2 * want).all()


@pytest.mark.parametrize("count_bits", [32, 16])
def test_late_with_the_waves_of_a_workgroup_in_step(eng, count_bits):
    """From 200 taxa on the launcher keeps the four waves of a workgroup in step (one s_barrier per 32-tree step) and remaps the
    workgroups to the XCDs: 204 taxa, the shard [196, 204) (one whole d-block, 10 M tuples), 70 trees. The oracle's whole table is out of
    reach at this size; the prefetch order is the reference (bit for bit), and every tuple of a binary tree set sums to the trees counted."""
    n, m = 204, 70
    ref = flatten.flatten_reference(synth.reference_tree(n, 4200))
    batch = flatten.flatten_eval_trees(synth.tree_set(n, m, 5500), ref.name_to_id)
    P1, P2, vp = count_twice(eng, context(eng, count_bits, PREFETCH, 196, 204, n=n), batch)
    L1, L2, vl = count_twice(eng, context(eng, count_bits, LATE, 196, 204, n=n), batch)
    assert "/late" not in vp and "/late5" in vl, (vp, vl)
    assert L1.shape == (ranks.n_quartets(204) - ranks.n_quartets(196), 3)
    assert (L1 == P1).all() and (L2 == P2).all(), (vp, vl)
    assert (L1.astype(np.uint64).sum(axis=1) == m).all() and (L2.astype(np.uint64).sum(axis=1) == 2 * m).all()


def test_knob_rejects_values_beyond_two(eng):
    ctx = eng.Context(N, 32)
    with pytest.raises(Exception):
        ctx.set_tuning(_lib.QS_TUNE_STEP_ORDER, 3)
    ctx.set_tuning(_lib.QS_TUNE_STEP_ORDER, 0)
    ctx.close()
