"""The six-wave dma instance of count_bitslice3_kernel lays its operands out by VGPR bank (qs_bitslice3.hpp, bs3_staggered): the L
planes travel in a register tuple of their own, the sources of the chains' top plane and of the L differences are permuted (truth
tables permuted with them), results and counters are paired. None of that may change a number: every count table below is the
oracle's, bit for bit, after an overwriting count over stale contents and after a second, accumulating one.

Instances: that one, and the others that share its segment code (bs3_segment, bin_row): binary_full at 4 depth bits under the prefetch
and late orders (QS_TUNE_STEP_ORDER / QS_TUNE_STAGE_SIX), u32 and u16 cells throughout; the 5-bit late and prefetch instances; a fused
launch of a full and a dropout class.

Shapes: 9 taxa = diagonal tiles only; 33 = the first off-diagonal tiles, one a-block only; 66 = every tile variant (both a-columns
with all eight d slots, with a cut d-block, one a-block, diagonal); 208 = the launcher keeps the waves of a workgroup in step (one
s_barrier per 32-tree step) and remaps the workgroups, from 200 taxa on. 33 and 70 trees = one full group of 32 plus a tail, and an odd
number of groups (the dma order runs one step per trip, the other two peel the odd last step).

At 208 taxa the shard [200, 208) is counted: one whole d-block, 11.5 M tuples. The oracle's table of 208 taxa (76 M tuples) is out of
reach in a test, but a quartet's counts depend on the four taxa alone: the oracle counts the trees PRUNED to 44 of the taxa (every
seventh id and the top twelve: a-, b- and c-blocks all over the tile list), and its 55 000 quartets with d >= 200 are looked up in the
shard at their ranks. That is a sample of the shard's cells against the oracle, not all of them; every tuple of the shard must also
sum to the trees counted."""
import numpy as np
import pytest

from oracle_api import Oracle
from quartetscores_amd import flatten, newick, ranks, synth
from test_gpu_step_order import context, count_twice
from test_gpu_step_order import tree_case as tree_case_40

pytestmark = pytest.mark.gpu
PREFETCH, LATE, DMA = "prefetch", "late", "dma"
KNOBS = {PREFETCH: (1, 1), LATE: (2, 1), DMA: (0, 2)}   # (QS_TUNE_STEP_ORDER, QS_TUNE_STAGE_SIX)
BIG, BIG_LO = 208, 200


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    from quartetscores_amd import engine
    return engine


def oracle_table(ref_nw, trees):
    o = Oracle(ref_nw)
    o.count("\n".join(trees), nthreads=4)
    want = o.counts()
    names = list(o.names)
    o.close()
    want.setflags(write=False)
    return names, want


_CASES = {}


def case(kind, n, m):
    """(flattened batch, oracle table) of one tree set, built once and left unchanged."""
    key = (kind, n, m)
    if key not in _CASES:
        ref_nw = synth.reference_tree(n, 6100 + n)
        ref = flatten.flatten_reference(ref_nw)
        if kind == "b4":        # random binary trees on all taxa: the 4-bit class
            trees = synth.tree_set(n, m, 6200 + n + m)
        elif kind == "b5":      # a caterpillar and NNI neighbours, re-centred: the 5-bit class
            lad = f"(t{n - 2},t{n - 1})"
            for i in range(n - 3, -1, -1):
                lad = f"(t{i},{lad})"
            trees = [lad + ";"] + list(synth.nni_tree_set(lad + ";", m - 1, 6300 + n + m))
        else:                   # "fused": a full and a dropout class, both binary
            trees = synth.tree_set(n, m - 24, 6400 + n) + synth.tree_set(n, 24, 6401 + n, dropout=0.1)
        names, want = oracle_table(ref_nw, trees)
        assert names == list(ref.names)
        _CASES[key] = (flatten.flatten_eval_trees(trees, ref.name_to_id), want)
    return _CASES[key]


def ordered(eng, count_bits, order, **kw):
    step_order, six = KNOBS[order]
    return context(eng, count_bits, step_order, QS_TUNE_STAGE_SIX=six, **kw)


def check_variant(variant, order, bits_name):
    assert f"bitslice_{bits_name}x2" in variant, variant
    assert ("/late5" in variant) == (order == LATE) and ("/dma6" in variant) == (order == DMA) and "/late6" not in variant, (order, variant)


@pytest.mark.parametrize("count_bits", [32, 16])
@pytest.mark.parametrize("order", [PREFETCH, LATE, DMA])
@pytest.mark.parametrize("m", [33, 70])
@pytest.mark.parametrize("n", [9, 33, 66])
def test_four_bit_orders_equal_the_oracle(eng, n, m, order, count_bits):
    batch, want = case("b4", n, m)
    T1, T2, variant = count_twice(eng, ordered(eng, count_bits, order, n=n, QS_TUNE_DEPTH_CLAMP=0), batch)
    check_variant(variant, order, "b4")
    assert T1.shape == want.shape
    assert (T1.astype(np.uint64) == want).all() and (T2.astype(np.uint64) == 2 * want).all(), variant


@pytest.mark.parametrize("count_bits", [32, 16])
@pytest.mark.parametrize("order", [PREFETCH, LATE])
@pytest.mark.parametrize("n", [33, 40])
def test_five_bit_orders_equal_the_oracle(eng, n, order, count_bits):
    if n == 40:
        _, _, batch, want = tree_case_40("b5", 70)
    else:
        batch, want = case("b5", n, 70)
    T1, T2, variant = count_twice(eng, ordered(eng, count_bits, order, n=n, QS_TUNE_DEPTH_CLAMP=0), batch)
    check_variant(variant, order, "b5")
    assert (T1.astype(np.uint64) == want).all() and (T2.astype(np.uint64) == 2 * want).all(), variant


@pytest.mark.parametrize("count_bits", [32, 16])
@pytest.mark.parametrize("n,m", [(33, 70), (66, 57)])
def test_fused_full_and_dropout_launch_equals_the_oracle(eng, n, m, count_bits):
    batch, want = case("fused", n, m)
    tuning = dict(QS_TUNE_DEPTH_CLAMP=0, QS_TUNE_CLASS_MIN_TREES=1, QS_TUNE_CLASS_PCT=0, QS_TUNE_FUSE_CLASSES=1)
    T1, T2, variant = count_twice(eng, ordered(eng, count_bits, DMA, n=n, **tuning), batch)
    assert "/fused:1" in variant and "binary_full" in variant and "binary_partial" in variant, variant
    assert (T1.astype(np.uint64) == want).all() and (T2.astype(np.uint64) == 2 * want).all(), variant


_BIG = {}


def big_case(m):
    """208 taxa: (batch, ranks inside the shard [200, 208) of the pruned oracle's quartets with d >= 200, their oracle rows)."""
    if m not in _BIG:
        ref_nw = synth.reference_tree(BIG, 6500)
        ref = flatten.flatten_reference(ref_nw)
        trees = synth.tree_set(BIG, m, 6600 + m)
        keep = [i for i in range(BIG) if i % 7 == 0 or i >= BIG - 12]
        drop = [ref.names[i] for i in range(BIG) if i not in set(keep)]

        def pruned(nw):
            return newick.write(newick.prune(newick.parse_tree(nw), drop))

        small_nw = pruned(ref_nw)
        small = flatten.flatten_reference(small_nw)
        ids = flatten.taxon_restriction(small, ref).astype(np.int64)     # id in the 208-taxon reference of every kept taxon
        assert (np.diff(ids) > 0).all() and sorted(ids.tolist()) == keep
        names, want = oracle_table(small_nw, [pruned(t) for t in trees])
        assert names == list(small.names)
        q = ids[ranks.unrank4_np(np.arange(len(want)))]                   # the oracle's quartets in the ids of the big reference
        top = q[:, 3] >= BIG_LO
        rows = ranks.rank4(q[top, 0], q[top, 1], q[top, 2], q[top, 3]) - ranks.n_quartets(BIG_LO)
        assert len(rows) > 10000
        _BIG[m] = (flatten.flatten_eval_trees(trees, ref.name_to_id), rows, want[top])
    return _BIG[m]


@pytest.mark.parametrize("count_bits", [32, 16])
@pytest.mark.parametrize("order", [PREFETCH, LATE, DMA])
@pytest.mark.parametrize("m", [33, 70])
def test_four_bit_orders_with_the_waves_in_step(eng, m, order, count_bits):
    batch, rows, want = big_case(m)
    ctx = ordered(eng, count_bits, order, d_lo=BIG_LO, d_hi=BIG, n=BIG)
    ctx.table_alloc()
    ctx.table_upload(np.full((ctx.table_tuples, 3), 321, dtype=np.uint32 if count_bits == 32 else np.uint16))
    hb = ctx.batch_upload(batch, with_nodes=False)
    ctx.count_batch(hb, eng.QS_ALGO_GATHER | eng.QS_COUNT_OVERWRITE)
    ctx.count_batch(hb, eng.QS_ALGO_GATHER)
    ctx.sync()
    variant = ctx.last_count_variant()
    T2 = ctx.table_download()
    ctx.batch_free(hb)
    ctx.close()
    check_variant(variant, order, "b4")
    assert T2.shape == (ranks.n_quartets(BIG) - ranks.n_quartets(BIG_LO), 3)
    assert (T2[rows].astype(np.uint64) == 2 * want).all(), variant
    assert (T2.sum(axis=1, dtype=np.uint64) == 2 * m).all(), variant
