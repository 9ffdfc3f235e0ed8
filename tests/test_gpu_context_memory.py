"""The context's device and pinned memory (csrc/qs_devbuf.hpp: every buffer of a qs_ctx is one owning type): nothing is left
behind when contexts go, a context whose buffers had to grow or to be replaced keeps computing what the oracle computes, and a
refused call strands nothing.

24 taxa, 40 evaluation trees of every kind. A depth class beyond the bit-sliced kernel's 10 bits needs a tree at least 1024 inner
nodes deep, which 24 taxa cannot hold (the deepest tree, a ladder that is not re-centred, reaches 22): the ladders here give the
batch a second depth class, and the byte-SWAR kernel with its panel and its own tiling is reached through QS_TUNE_GATHER_IMPL."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import agreement_model
import taxon_model
from helpers import concat_batches, repeat_trees, ulp_diff
from oracle_api import Oracle
from quartetscores_amd import _lib, flatten, newick, synth

pytestmark = pytest.mark.gpu
N, M = 24, 40
GATHER = _lib.QS_ALGO_GATHER


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    from quartetscores_amd import engine
    return engine


def collapsed(ref_nw, every=3):
    """the tree with every `every`-th inner edge contracted: fewer nodes, the same depth-first leaf order (= lookup ids)"""
    root = newick.parse_tree(ref_nw)
    inner = [x for x in newick.preorder(root) if x.children and x.parent is not None]
    for x in inner[::every]:
        kids = x.parent.children
        i = kids.index(x)
        kids[i:i + 1] = x.children
        for ch in x.children:
            ch.parent = x.parent
    return newick.write(root)


class Case:
    pass


@pytest.fixture(scope="module")
def case(eng):
    """The trees, their batches, the device tensors every test writes its results to, and what the oracle says -- computed once."""
    import torch
    k = Case()
    rng = np.random.default_rng(2410)
    nw_b = synth.random_tree(N, rng)                       # B: binary, 2N - 2 nodes
    nw_a = collapsed(nw_b)                                 # A: smaller, same lookup ids -> the same table serves both
    nw_c = synth.random_tree(N, rng, collapse=0.3)         # C: other lookup ids (qs_table_remap)
    k.ref = {"A": flatten.flatten_reference(nw_a), "B": flatten.flatten_reference(nw_b), "C": flatten.flatten_reference(nw_c)}
    assert k.ref["A"].names == k.ref["B"].names and k.ref["A"].n_nodes < k.ref["B"].n_nodes
    assert k.ref["C"].names != k.ref["A"].names
    ladder = "(t0,t1)"
    for i in range(2, N):
        ladder = "(" + ladder + f",t{i})"
    shallow = (synth.tree_set(N, 18, 2411) + synth.tree_set(N, 8, 2412, collapse=0.3) + synth.tree_set(N, 8, 2413, dropout=0.2) +
               synth.tree_set(N, 3, 2414, dropout=0.2, collapse=0.3))
    k.trees = shallow + [ladder + ";"] * 3
    assert len(k.trees) == M
    ids = k.ref["A"].name_to_id
    # (the ladders are not re-centred and keep their depth of N - 2: five depth bits, the other trees need four)
    k.batch = concat_batches(flatten.flatten_eval_trees(shallow, ids), flatten.flatten_eval_trees(k.trees[len(shallow):], ids, recentre=False))
    assert int(k.batch.adj_depth.max()) == N - 2
    k.batch400 = repeat_trees(k.batch, [(t, 10) for t in range(M)], with_nodes=False)
    # the oracle: count table (lookup ids of A = B), scores for A and B, the table under C's ids
    text = "\n".join(k.trees)
    k.oracle, k.scores = {}, {}
    for name, nw in (("A", nw_a), ("B", nw_b), ("C", nw_c)):
        o = Oracle(nw)
        assert o.names == k.ref[name].names
        o.count(text, nthreads=4)
        if name != "C":
            o.score(nthreads=4)
            k.scores[name] = o.scores_by_bipartition()
        k.oracle[name] = o
    k.counts = k.oracle["A"].counts()
    assert (k.counts == k.oracle["B"].counts()).all()
    k.counts_c = k.oracle["C"].counts()
    # tree agreement: every fourth tree and a ladder, as a batch of their own (the model takes a quarter second per tree)
    k.batch_agree = concat_batches(flatten.flatten_eval_trees(shallow[::4], ids), flatten.flatten_eval_trees(k.trees[-1:], ids, recentre=False))
    k.agree = {name: np.array([agreement_model.model_tree(k.ref[name], t) for t in shallow[::4]] +
                              [agreement_model.model_tree(k.ref[name], k.trees[-1], False)], dtype=np.uint64) for name in "AB"}
    k.taxon = taxon_model.model_counts(k.counts, k.ref["A"])
    k.quads = taxon_model.quads_in_rank_order(N)
    k.topo = {name: taxon_model.model_topology(k.ref[name], k.quads) for name in "AB"}
    k.lookup_ids = np.random.default_rng(2415).permuted(np.tile(np.arange(N), (64, 1)), axis=1)[:, :4].astype(np.uint16)
    k.lookup_want = np.array([k.oracle["A"].lookup(*[int(x) for x in q]) for q in k.lookup_ids], dtype=np.uint64)
    # device tensors of the calls below: made once, so that torch's caching allocator takes no part in what the tests measure
    k.agree_buf = torch.zeros(4 * k.batch_agree.n_trees, dtype=torch.int64, device="cuda")
    k.taxon_buf = torch.zeros(6 * N + 1, dtype=torch.int64, device="cuda")
    P = max(int(_lib.load().qs_score_pair_slots(C.byref(eng.Context._ref_struct(k.ref[name])[0]))) for name in "AB")
    k.sums, k.mins, k.cand = (torch.zeros(w * P, dtype=torch.int64, device="cuda") for w in (3, 1, 8))
    torch.cuda.synchronize()
    return k


# ---- the calls, each checked against the oracle -----------------------------------------------------------------------------

def check_table(ctx, case, times=1, counts=None):
    ctx.sync()
    assert (ctx.table_download().astype(np.uint64) == times * (case.counts if counts is None else counts)).all()
    assert ctx.trees_counted == times * M


def scores_of(eng, ref, lq, qp, eqp, bif):
    q = object.__new__(eng.QuartetScoreComputer)   # (only its dictionary of the scores by bipartition)
    q.ref, q._lq, q._qp, q._eqp = ref, lq[1:], (qp[1:] if bif else None), (eqp[1:] if bif else None)
    return q.scores_by_bipartition()


def assert_scores(got, want):
    """0 ulp, as tests/test_gpu_parity.py asks of its scores"""
    assert set(got) == set(want)
    for key, wv in want.items():
        for g, w in zip(got[key], wv):
            assert (g is None) == (w is None)
            assert w is None or int(ulp_diff(g, w)) == 0, (sorted(key), g, w)


def check_score(eng, ctx, case, name, prepare=False):
    ref = case.ref[name]
    if prepare:
        ctx.score_prepare(ref, M)
    assert_scores(scores_of(eng, ref, *ctx.score(ref)), case.scores[name])


def check_agreement(ctx, case, name):
    hb = ctx.batch_upload(case.batch_agree)
    s, keep = ctx._ref_struct(case.ref[name])
    ctx._chk(ctx.L.qs_tree_agreement(ctx.h, C.byref(s), hb, C.c_void_p(case.agree_buf.data_ptr())))
    ctx.sync()
    del keep
    ctx.batch_free(hb)
    assert (case.agree_buf.cpu().numpy().view(np.uint64).reshape(-1, 4) == case.agree[name]).all()


def taxon_support_into(ctx, ref, ptr):
    s, keep = ctx._ref_struct(ref)
    ctx._chk(ctx.L.qs_taxon_support(ctx.h, C.byref(s), C.c_void_p(ptr)))
    ctx.sync()
    del keep


def check_taxon(ctx, case):
    taxon_support_into(ctx, case.ref["A"], case.taxon_buf.data_ptr())
    assert (case.taxon_buf[:6 * N].cpu().numpy().reshape(N, 6) == case.taxon).all()


def check_lookup(ctx, case):
    assert (ctx.lookup(case.lookup_ids) == case.lookup_want).all()


def check_raw_qic(ctx, case, name):
    topo, q = ctx.raw_qic(case.ref[name], 0, len(case.counts))
    assert (topo == case.topo[name]).all()
    res = topo != 255
    # the triple of a resolved quartet starts with the count of the reference's topology and holds the tuple's three cells
    assert (q[res, 0] == np.take_along_axis(case.counts[res], topo[res].astype(np.int64)[:, None], 1)[:, 0]).all()
    assert (np.sort(q[res], axis=1) == np.sort(case.counts[res], axis=1)).all()


def new_context(eng, case, table=True):
    ctx = eng.Context(N, 32)
    ctx.set_tuning(_lib.QS_TUNE_CLASS_MIN_TREES, 1)     # every (mode, depth bits) class of the 40 trees is counted on its own
    ctx.set_tuning(_lib.QS_TUNE_CLASS_PCT, 0)
    if table:
        ctx.table_alloc()
    return ctx


# ---- (a) nothing is left behind --------------------------------------------------------------------------------------------

# Bytes of free device memory that cycles 2 to 5 may cost: what the HIP runtime itself keeps, to be measured with this very test on the
# commit before the buffers became one type, whose qs_destroy freed every pointer by name. No such measurement exists yet
# (profiles/README.md), so nothing is allowed.
RUNTIME_DRIFT_BYTES = 0


def cycle(eng, case, log_cap=8):
    ctx = new_context(eng, case, table=False)
    ctx._chk(ctx.L.qs_prepare(ctx.h, M))                      # staging buffers, launch order, panel
    ctx.table_alloc()
    ctx._chk(ctx.L.qs_prepare(ctx.h, M))                      # ... and, now that there is a table, the first use of the lookup kernel
    hb = ctx.batch_upload(case.batch)
    ctx.count_batch(hb, GATHER | _lib.QS_COUNT_TIMED)
    assert ctx.last_count_ms()[2] > 0 and "mixed" in ctx.last_count_variant()
    ctx.set_tuning(_lib.QS_TUNE_TILE_ORDER, 4 | (16 << 16))   # the launch order is dropped and built again, with the cooperative lists
    ctx.set_tuning(_lib.QS_TUNE_COOP, 1)
    ctx.set_tuning(_lib.QS_TUNE_FUSE_CLASSES, 0)              # (the cooperative kernel takes binary_full classes that are not fused)
    ctx.count_batch(hb, GATHER | _lib.QS_COUNT_TIMED)
    assert ctx.last_count_ms()[2] > 0 and "coop4" in ctx.last_count_variant()
    ctx.set_tuning(_lib.QS_TUNE_GATHER_IMPL, _lib.QS_IMPL_SWAR)   # the byte-SWAR kernel: its own tiling and a panel of 16 bytes per pair
    ctx.count_batch(hb, GATHER)
    assert "depth_u" in ctx.last_count_variant()
    ctx.set_tuning(_lib.QS_TUNE_GATHER_IMPL, _lib.QS_IMPL_AUTO)
    check_table(ctx, case, times=3)
    ctx.table_clear()
    ctx.count_batch(hb, GATHER)
    check_table(ctx, case)
    ctx.set_tuning(_lib.QS_TUNE_SCORE_LOG_CAP, log_cap)
    for passes in (1, 2):                                     # two passes; single read (its log of `log_cap` records overflows: second read)
        ctx.set_tuning(_lib.QS_TUNE_SCORE_PASSES, passes)
        check_score(eng, ctx, case, "A", prepare=True)
    check_score(eng, ctx, case, "B")                          # another node count: reference arrays, bundle plans, accumulators
    check_agreement(ctx, case, "A")
    check_agreement(ctx, case, "B")
    check_taxon(ctx, case)
    ctx2 = new_context(eng, case)
    ctx2.table_remap(ctx, flatten.taxon_permutation(case.ref["C"], case.ref["A"]))
    check_table(ctx2, case, counts=case.counts_c)
    check_lookup(ctx, case)
    check_raw_qic(ctx, case, "B")
    ctx.batch_free(hb)
    ctx.close()
    ctx2.close()


def free_bytes():
    import torch
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def test_nothing_is_left_behind(eng, case):
    """Five cycles of create, qs_prepare, count (timed; launch order rebuilt; byte-SWAR), score (both modes, two references), tree
    agreement (two references), taxon support, remap into a second context, lookup, raw QIC, destroy: the device has as much free
    memory after the fifth as after the first."""
    cycle(eng, case)
    after_1 = free_bytes()
    for _ in range(4):
        cycle(eng, case)
    after_5 = free_bytes()
    print(f"free device memory: after cycle 1 {after_1}, after cycle 5 {after_5}, lost {after_1 - after_5} bytes")
    assert after_1 - after_5 <= RUNTIME_DRIFT_BYTES


# ---- (b) growing leaves a working context ----------------------------------------------------------------------------------

def test_growing_leaves_a_working_context(eng, case):
    ctx = new_context(eng, case)
    ctx.set_tuning(_lib.QS_TUNE_PANEL_SLICE_BYTES, 6000)       # one group of 32 trees (276 pairs x 5 words) per slice: a small panel
    hb = ctx.batch_upload(case.batch)
    ctx.count_batch(hb, GATHER)
    check_table(ctx, case)
    ctx.set_tuning(_lib.QS_TUNE_PANEL_SLICE_BYTES, 0)
    ctx.count_trees(case.batch400, GATHER)                     # 400 trees unsliced: the panel (and the staging buffers) grow
    check_table(ctx, case, times=11)
    ctx.table_clear()
    ctx.count_batch(hb, GATHER)
    check_table(ctx, case)
    for name in "ABA":                                         # B has more nodes than A: every per-reference buffer grows, then is replaced again
        check_score(eng, ctx, case, name)
    for name in "ABA":
        check_agreement(ctx, case, name)
    check_taxon(ctx, case)
    check_table(ctx, case)
    ctx.batch_free(hb)
    ctx.close()


# ---- (c) refusals do not strand memory -------------------------------------------------------------------------------------

def refused(eng, call):
    with pytest.raises(eng.QSError) as ei:
        call()
    return ei.value.code


def test_refusals_leave_a_working_context(eng, case):
    """Calls the host refuses (no kernel is launched for them), each followed by a correct call of the same function."""
    ref = case.ref["A"]
    ctx = new_context(eng, case, table=False)
    P = ctx.score_pair_slots(ref)
    sums, mins, cand = case.sums[:3 * P], case.mins[:P], case.cand[:8 * P]
    assert refused(eng, lambda: ctx.score_pass1(ref, sums, mins)) == _lib.QS_ERR_STATE          # no table
    ctx.table_alloc()
    hb = ctx.batch_upload(case.batch)
    ctx.count_batch(hb, GATHER)
    check_table(ctx, case)
    ctx.score_pass1(ref, sums, mins)
    ctx.score_pass2(ref, mins, cand)
    extra = ctx.score_overflow(ref, mins, cand)
    ctx.sync()
    assert_scores(scores_of(eng, ref, *ctx.score_finish(ref, sums.cpu().numpy(), cand.cpu().numpy().reshape(1, -1), extra=extra)), case.scores["A"])

    bad = case.lookup_ids.copy()
    bad[-1, 2] = N                                                                               # an id out of range
    assert refused(eng, lambda: ctx.lookup(bad)) == _lib.QS_ERR_ARG
    check_lookup(ctx, case)

    assert refused(eng, lambda: taxon_support_into(ctx, ref, case.taxon_buf.data_ptr() + 4)) == _lib.QS_ERR_ARG   # misaligned destination
    check_taxon(ctx, case)

    check_agreement(ctx, case, "B")                                                          # (a tree is cached when the bad one arrives)
    parent = np.array(ref.parent, dtype=np.int32)
    parent[int(np.nonzero(parent >= 0)[0][-1])] = -1                                             # a second root
    two_roots = dataclasses.replace(ref, parent=parent)
    s, keep = ctx._ref_struct(two_roots)
    hb_a = ctx.batch_upload(case.batch_agree)
    assert refused(eng, lambda: ctx._chk(ctx.L.qs_tree_agreement(ctx.h, C.byref(s), hb_a, C.c_void_p(case.agree_buf.data_ptr())))) == _lib.QS_ERR_ARG
    ctx.batch_free(hb_a)
    del keep
    check_agreement(ctx, case, "A")
    check_agreement(ctx, case, "B")
    check_table(ctx, case)
    ctx.batch_free(hb)
    ctx.close()
