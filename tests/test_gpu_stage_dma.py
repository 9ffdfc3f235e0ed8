"""The six-wave instance of count_bitslice3_kernel<4, binary_full> (QS_TUNE_STAGE_SIX = 2): the next group's staged panel elements
go into a raw area of the wave's LDS region by loads that write LDS directly, the R elements are built from there into ONE LDS
image, and the request stands at the top of the 32-tree step. The arithmetic is that of the prefetch instance: the tables must agree
bit for bit, and with the oracle's.

Shapes as in tests/test_gpu_step_order.py: 40 taxa is the smallest tiling in which every instance of the step occurs
(tests/test_step_order_tiles.py) -- it also holds every kind of ABSENT staged element (a-columns and b-columns at or above c, d-rows
outside the block), which the new instance requests at pair 0 instead of beyond the group; 20, 33, 64, 70 and 97 trees are 1, 2, 2, 3
and 4 groups of 32 trees, the last one partly filled. The step loop of the new instance runs one step per trip, so the group counts
stand for "prologue only", "one trip" and "several trips"."""
import numpy as np
import pytest

from quartetscores_amd import _lib, flatten, ranks, synth
from test_gpu_step_order import N, context, count_twice, tree_case

pytestmark = pytest.mark.gpu
PREFETCH = 1
TODAY, SIX = 1, 2


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    from quartetscores_amd import engine
    return engine


def six_segment(variant):
    """The variant names the six-wave instance as ONE segment /dma6 or /late6, in front of /clamp: and /overlap:."""
    segs = [s for s in variant.split("/") if s in ("dma6", "late6")]
    assert len(segs) == 1 and "/late5" not in variant, variant
    tail = variant.split("/" + segs[0], 1)[1]
    assert all(t.startswith(("clamp:", "overlap:")) for t in tail.split("/") if t), variant
    return segs[0]


def six_against_prefetch(eng, batch, want, count_bits, d_lo=0, d_hi=0, n=N, **tuning):
    """Count with the prefetch instance and with the six-wave one; equal bit for bit after the overwriting and after the accumulating
    count; the six-wave table is the oracle's (want = None: not checked). Returns the two variants."""
    P1, P2, vp = count_twice(eng, context(eng, count_bits, PREFETCH, d_lo, d_hi, n=n, QS_TUNE_STAGE_SIX=TODAY, **tuning), batch)
    S1, S2, vs = count_twice(eng, context(eng, count_bits, 0, d_lo, d_hi, n=n, QS_TUNE_STAGE_SIX=SIX, **tuning), batch)
    assert "/late" not in vp and "/dma" not in vp and "bitslice_b4x2" in vp, vp
    six_segment(vs)
    assert "bitslice_b4x2" in vs, vs
    assert (S1 == P1).all() and (S2 == P2).all(), (vp, vs)
    if want is not None:
        rows = want[ranks.n_quartets(d_lo): ranks.n_quartets(d_hi or n)]
        assert S1.shape == rows.shape
        assert (S1.astype(np.uint64) == rows).all() and (S2.astype(np.uint64) == 2 * rows).all(), vs
    return vp, vs


@pytest.mark.parametrize("count_bits", [32, 16])
@pytest.mark.parametrize("m", [20, 33, 64, 70, 97])
def test_six_equals_prefetch_and_the_oracle(eng, m, count_bits):
    _, _, batch, want = tree_case("b4", m)
    six_against_prefetch(eng, batch, want, count_bits, QS_TUNE_DEPTH_CLAMP=0)


@pytest.mark.parametrize("count_bits", [32, 16])
def test_six_through_a_shard_with_a_narrow_d_block(eng, count_bits):
    _, _, batch, want = tree_case("b4", 70)
    six_against_prefetch(eng, batch, want, count_bits, d_lo=13, d_hi=38, QS_TUNE_DEPTH_CLAMP=0)


@pytest.mark.parametrize("count_bits", [32, 16])
def test_six_with_clamped_trees_and_a_split_launch(eng, count_bits):
    """Deep trees clamped to 4 bits, the slice split at d_mid = 24: both count launches run the six-wave instance, the corrections of the
    upper range beside the lower launch."""
    _, _, batch, want = tree_case("clamped", 70)
    tuning = dict(QS_TUNE_DEPTH_CLAMP=1000000, QS_TUNE_CLASS_MIN_TREES=1, QS_TUNE_CLASS_PCT=0, QS_TUNE_FIX_OVERLAP=1, QS_TUNE_FIX_SPLIT_AT=24)
    vp, vs = six_against_prefetch(eng, batch, want, count_bits, **tuning)
    for v in (vp, vs):
        assert "/clamp:" in v and v.endswith("/overlap:24"), v


def test_six_into_the_wire_format(eng):
    """QS_COUNT_WIRE16X2: one word n0 | n1 << 16 per tuple, overwrite then accumulate; the words of the two instances agree, unpacked they
    are twice the oracle's table."""
    import torch
    _, _, batch, want = tree_case("b4", 70)
    dev = torch.device("cuda", 0)
    words = {}
    for six in (TODAY, SIX):
        ctx = context(eng, 32, PREFETCH if six == TODAY else 0, QS_TUNE_STAGE_SIX=six, QS_TUNE_DEPTH_CLAMP=0)
        nt = ctx.table_tuples
        wire = torch.full((nt,), 0x7FFFFFFF, dtype=torch.int32, device=dev)
        ctx.wire_attach(wire)
        hb = ctx.batch_upload(batch, with_nodes=False)
        ctx.count_batch(hb, eng.QS_ALGO_GATHER | eng.QS_COUNT_WIRE16X2 | eng.QS_COUNT_OVERWRITE)
        ctx.count_batch(hb, eng.QS_ALGO_GATHER | eng.QS_COUNT_WIRE16X2)
        ctx.sync()
        variant = ctx.last_count_variant()
        assert "/wire_u16x2" in variant and "/late" not in variant.replace("/late6", ""), variant
        assert (("/dma6" in variant) or ("/late6" in variant)) == (six == SIX), variant
        out = torch.zeros((nt * 6 + 3) // 4, dtype=torch.int32, device=dev)
        ctx.unpack16x2(wire, nt, 2 * batch.n_trees, out)
        ctx.sync()
        words[six] = (wire.cpu().numpy().copy(), out.cpu().numpy().view(np.uint16)[: nt * 3].reshape(-1, 3).astype(np.uint64))
        ctx.batch_free(hb)
        ctx.close()
    assert (words[SIX][0] == words[TODAY][0]).all()
    assert (words[SIX][1] == 2 * want).all()


@pytest.mark.parametrize("count_bits", [32, 16])
def test_six_with_the_waves_of_a_workgroup_in_step(eng, count_bits):
    """From 200 taxa on the launcher keeps the four waves of a workgroup in step (one s_barrier per 32-tree step) and remaps the
    workgroups to the XCDs: 204 taxa, the shard [196, 204), 70 trees. The prefetch instance is the reference (bit for bit), and every tuple
    of a binary tree set sums to the trees counted."""
    n, m = 204, 70
    ref = flatten.flatten_reference(synth.reference_tree(n, 4200))
    batch = flatten.flatten_eval_trees(synth.tree_set(n, m, 5500), ref.name_to_id)
    P1, P2, vp = count_twice(eng, context(eng, count_bits, PREFETCH, 196, 204, n=n, QS_TUNE_STAGE_SIX=TODAY), batch)
    S1, S2, vs = count_twice(eng, context(eng, count_bits, 0, 196, 204, n=n, QS_TUNE_STAGE_SIX=SIX), batch)
    assert "/late" not in vp and "/dma" not in vp, vp
    six_segment(vs)
    assert S1.shape == (ranks.n_quartets(204) - ranks.n_quartets(196), 3)
    assert (S1 == P1).all() and (S2 == P2).all(), (vp, vs)
    assert (S1.astype(np.uint64).sum(axis=1) == m).all() and (S2.astype(np.uint64).sum(axis=1) == 2 * m).all()


def test_knob_range_and_todays_variants(eng):
    """The knob takes 0, 1 and 2. At 1 the variants are those of QS_TUNE_STEP_ORDER alone: no segment at 1 (prefetch), /late5 at 2 and in the
    automatic setting; an explicit QS_TUNE_STEP_ORDER is obeyed with the new knob at 0 as well; at 2 the six-wave instance runs whatever
    QS_TUNE_STEP_ORDER says."""
    ctx = eng.Context(N, 32)
    with pytest.raises(Exception):
        ctx.set_tuning(_lib.QS_TUNE_STAGE_SIX, 3)
    ctx.set_tuning(_lib.QS_TUNE_STAGE_SIX, 0)
    ctx.close()
    _, _, batch, want = tree_case("b4", 33)

    def variant(order, six):
        T1, _, v = count_twice(eng, context(eng, 32, order, QS_TUNE_STAGE_SIX=six, QS_TUNE_DEPTH_CLAMP=0), batch)
        assert (T1.astype(np.uint64) == want).all(), v
        return v

    for six in (TODAY, 0):
        v1, v2 = variant(1, six), variant(2, six)
        assert "/late" not in v1 and "/dma" not in v1, v1
        assert v2.endswith("/late5") and "/dma" not in v2, v2
    va = variant(0, TODAY)
    assert va.endswith("/late5") and "/dma" not in va, va
    for order in (0, 1, 2):
        six_segment(variant(order, SIX))


def test_six_after_another_batch_in_the_same_context(eng):
    """No stored cell may depend on an absent staged element or on what an earlier launch left in LDS: the first count of the batch runs
    right after a DIFFERENT batch (other trees, other group count) was counted by the same context into the same table, and over its
    contents; prefetch instance and oracle are the references."""
    _, _, other, _ = tree_case("b4", 97)
    _, _, batch, want = tree_case("b4", 33)
    tables = {}
    for six in (TODAY, SIX):
        ctx = context(eng, 32, PREFETCH if six == TODAY else 0, QS_TUNE_STAGE_SIX=six, QS_TUNE_DEPTH_CLAMP=0)
        ctx.table_alloc()
        ho = ctx.batch_upload(other, with_nodes=False)
        ctx.count_batch(ho, eng.QS_ALGO_GATHER | eng.QS_COUNT_OVERWRITE)
        hb = ctx.batch_upload(batch, with_nodes=False)
        ctx.count_batch(hb, eng.QS_ALGO_GATHER | eng.QS_COUNT_OVERWRITE)
        ctx.sync()
        if six == SIX:
            six_segment(ctx.last_count_variant())
        tables[six] = ctx.table_download()
        ctx.batch_free(ho)
        ctx.batch_free(hb)
        ctx.close()
    assert (tables[SIX] == tables[TODAY]).all()
    assert (tables[SIX].astype(np.uint64) == want).all()
