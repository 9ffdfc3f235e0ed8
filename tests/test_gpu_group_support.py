"""qs_group_support / Context.group_support: the six words of quad and split hypotheses over the count table, bit for bit against
the numpy model (tests/group_model.py) at both cell widths and across the batching edges, equal to the QP-IC of qs_score when the
four groups are the subtrees beside an edge, exact at counts near 2^32, additive over table shards, repeatable, and without side
effects on the table or the scores."""
import ctypes as C
import functools

import numpy as np
import pytest

import group_model as M
from helpers import binom
from quartetscores_amd import _lib, flatten, synth

pytestmark = pytest.mark.gpu

HG = 8   # hypotheses one read of the table serves (kGroupHyp)


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    from quartetscores_amd import engine
    return engine


def mixed_trees(n, seed):
    """dropout, collapsed edges and rooted trees in one batch (as tests/test_gpu_clade_placement.py)"""
    return (synth.tree_set(n, 12, seed, dropout=0.2) + synth.tree_set(n, 12, seed + 1, collapse=0.3) +
            synth.tree_set(n, 12, seed + 2, rooted=True) + synth.tree_set(n, 6, seed + 3))


def reference(n, kind, seed):
    rng = np.random.default_rng(seed)
    kw = {"binary": {}, "multifurcating": {"collapse": 0.4}, "rooted": {"rooted": True}}[kind]
    return flatten.flatten_reference(synth.random_tree(n, rng, **kw))


def counted(eng, ref, trees, bits):
    ctx = eng.Context(ref.n_taxa, bits)
    ctx.table_alloc()
    ctx.count_trees(flatten.flatten_eval_trees(trees, ref.name_to_id))
    return ctx


@functools.lru_cache(maxsize=2)
def quads(n):
    q = M.quads_in_rank_order(n)
    return q, np.ascontiguousarray(q.T)


def model(table, labels, n):
    q, cols = quads(n)
    return M.model_counts(table, labels, n, quads=q, cols=cols)


def same(got, want):
    return got.shape == want.shape and (got.astype(object) == want).all()


@pytest.mark.parametrize("bits", [16, 32])
@pytest.mark.parametrize("n", [5, 6, 7, 9, 17, 33])
def test_equals_model_of_the_downloaded_table(eng, n, bits):
    ref = reference(n, "binary", 1000 + n)
    ctx = counted(eng, ref, mixed_trees(n, 300 + n), bits)
    labels = M.hypotheses(n, 3 * HG + 2, 40 + n)      # singleton quads, all taxa used, interleaved groups, |S1| = 2, taxa left out
    kinds = [M.kind_of(row) for row in labels]
    assert 0 in kinds and 1 in kinds and (labels == 0).any()
    got = ctx.group_support(labels)
    want = model(ctx.table_download(), labels, n)
    assert got.dtype == np.int64 and same(got, want)
    assert [int(x) for x in got[:, 0]] == [M.whole_table_quartets(row) for row in labels]
    for k in (1, HG, HG + 1):                          # the batching edges: the words do not depend on how hypotheses share a pass
        assert same(ctx.group_support(labels[:k]), want[:k])
    assert same(ctx.group_support(labels[::-1]), want[::-1])


@pytest.mark.parametrize("kind", ["binary", "multifurcating", "rooted"])
@pytest.mark.parametrize("bits", [16, 32])
@pytest.mark.parametrize("n", [65, 130])
def test_rows_longer_than_a_bundle_and_a_chunk(eng, n, bits, kind):
    ref = reference(n, kind, 2000 + n)
    ctx = counted(eng, ref, mixed_trees(n, 500 + n), bits)
    labels = M.hypotheses(n, 6, 60 + n, cap=24)        # (at most 24 taxa per group: the model's counted 4-sets stay few)
    assert same(ctx.group_support(labels), model(ctx.table_download(), labels, n))


def edge_groups(ref):
    """per inner edge of a binary unrooted reference (named by its child node v): the four subtrees beside it as label rows S1 S2 |
    S3 S4 -- S1, S2 the children of v in id order, S3 the subtree that follows S2 in the circular id order, S4 the last one: with
    this order q2 = n(S1 S3 | S2 S4) pairs the smallest with the third-smallest id of every 4-set, which is the cell qs_score
    hands log_score as its second argument -- and the sizes of the edge's two sides"""
    par = np.asarray(ref.parent, dtype=np.int64)
    N, n = len(par), ref.n_taxa
    kids = [[] for _ in range(N)]
    for v in range(N):
        if par[v] >= 0:
            kids[par[v]].append(v)
    below = [None] * N
    for i, v in enumerate(np.asarray(ref.leaf_node, dtype=np.int64)):
        below[v] = np.array([i], dtype=np.int64)

    def leaves(v):
        if below[v] is None:
            below[v] = np.sort(np.concatenate([leaves(c) for c in kids[v]]))
        return below[v]

    out = []
    for v in range(N):
        p = par[v]
        if p < 0 or not kids[v]:
            continue
        assert len(kids[v]) == 2
        x, y = sorted(kids[v], key=lambda c: leaves(c)[0])
        others = [leaves(c) for c in kids[p] if c != v]
        if par[p] >= 0:
            others.append(np.setdiff1d(np.arange(n), leaves(p)))
        assert len(others) == 2
        nxt = (leaves(y)[-1] + 1) % n
        s3, s4 = (others[0], others[1]) if nxt in others[0] else (others[1], others[0])
        row = np.zeros(n, dtype=np.uint8)
        for label, members in enumerate((leaves(x), leaves(y), s3, s4), 1):
            row[members] = label
        out.append((v, row, len(leaves(v))))
    return out


@pytest.mark.parametrize("n", [17, 33])
def test_edge_hypotheses_give_the_edge_qpic_of_qs_score(eng, n):
    ref = reference(n, "binary", 3000 + n)
    ctx = counted(eng, ref, mixed_trees(n, 700 + n), 32)
    edges = edge_groups(ref)
    assert len(edges) == n - 3
    quad = ctx.group_support(np.stack([row for _, row, _ in edges]))
    qpic = ctx.score(ref, eng.QS_SCORE_QP_EXACT64)[1]
    for (v, row, s), w in zip(edges, quad):
        mine = eng.log_score(int(w[1]), int(w[2]), int(w[3]))
        assert np.float64(mine).view(np.int64) == np.float64(qpic[v]).view(np.int64), (v, w, mine, qpic[v])   # 0 ulp
    splits = np.stack([np.where((row == 1) | (row == 2), 1, 2).astype(np.uint8) for _, row, _ in edges])
    got = ctx.group_support(splits)
    assert [int(x) for x in got[:, 0]] == [int(binom(s, 2)) * int(binom(n - s, 2)) for _, _, s in edges]
    assert (got[:, 1] + got[:, 2] + got[:, 3] > 0).all()


def test_counts_at_the_cell_limits_take_the_wide_sums(eng):
    n = 9
    labels = M.hypotheses(n, HG + 3, 77)
    rng = np.random.default_rng(78)
    # 32-bit cells at 2^32 - 1 behind an uploaded table: two of them in one row leave a 32-bit partial sum, so equality with the
    # model shows the 64-bit instance ran (the host picks it from the trees said to be behind the table)
    ctx = eng.Context(n, 32)
    ctx.table_alloc()
    table = np.full((int(binom(n, 4)), 3), 0xFFFFFFFF, dtype=np.uint32)
    table[rng.random(len(table)) < 0.2] = 0
    table[rng.random(len(table)) < 0.2, 1] = 7
    ctx.table_upload(table)
    ctx.set_tuning(_lib.QS_TUNE_TABLE_TREES, 0xFFFFFFFF)
    want = M.model_counts(table, labels, n)
    assert max(int(x) for x in want[:, 1]) > 1 << 34
    assert same(ctx.group_support(labels), want)
    # 16-bit cells at 65535: a row's 32-bit sums hold n x 65535
    ctx16 = eng.Context(n, 16)
    ctx16.table_alloc()
    table16 = np.where(table == 0xFFFFFFFF, 65535, table).astype(np.uint16)
    ctx16.table_upload(table16)
    assert same(ctx16.group_support(labels), M.model_counts(table16, labels, n))


@pytest.mark.parametrize("d_mid", [20, 29])
def test_shards_add_up(eng, d_mid):
    n = 33
    ref = reference(n, "multifurcating", 4000)
    whole = counted(eng, ref, mixed_trees(n, 800), 32)
    labels = M.hypotheses(n, HG + 2, 81)
    want = whole.group_support(labels)
    table = whole.table_download()
    total = np.zeros_like(want)
    for lo, hi in ((0, d_mid), (d_mid, n)):
        shard = eng.Context(n, 32, d_lo=lo, d_hi=hi)
        r0, r1 = int(binom(lo, 4)), int(binom(hi, 4))
        shard.table_alloc()
        assert shard.table_tuples == r1 - r0
        shard.table_upload(table[r0:r1])
        part = shard.group_support(labels)
        assert same(part, M.model_counts(table[r0:r1], labels, n, rank_lo=r0))
        total += part
    assert (total == want).all() and (want[:, 0] > 0).all()


def test_repeatable_and_without_side_effects(eng):
    n = 24
    ref = reference(n, "binary", 12)
    trees = mixed_trees(n, 13)
    ctx = counted(eng, ref, trees, 32)
    labels = M.hypotheses(n, HG + 1, 14)
    before = ctx.table_download()
    scores = [np.asarray(x, dtype=np.float64).view(np.int64) for x in ctx.score(ref)[:3]]
    first = ctx.group_support(labels)
    assert (ctx.group_support(labels) == first).all()
    assert (ctx.table_download() == before).all() and ctx.trees_counted == len(trees)
    for x, y in zip(scores, [np.asarray(x, dtype=np.float64).view(np.int64) for x in ctx.score(ref)[:3]]):
        assert (x == y).all()
    assert (ctx.group_support(labels) == first).all()


def test_error_codes(eng):
    import torch
    n = 12
    ref = reference(n, "binary", 14)
    ctx = counted(eng, ref, mixed_trees(n, 15), 32)
    labels = M.hypotheses(n, 6, 16)
    want = ctx.group_support(labels)

    def code(f, *words):
        with pytest.raises(eng.QSError) as ei:
            f()
        for w in words:
            assert w in str(ei.value), str(ei.value)
        return ei.value.code

    assert code(lambda: eng.Context(n, 32).group_support(labels), "no table") == _lib.QS_ERR_STATE
    buf = torch.zeros(6 * len(labels) + 1, dtype=torch.int64, device="cuda")
    lab = np.ascontiguousarray(labels)
    assert ctx.L.qs_group_support(ctx.h, lab.ctypes.data, len(lab), C.c_void_p(buf.data_ptr() + 4)) == _lib.QS_ERR_ARG   # misaligned
    assert ctx.L.qs_group_support(ctx.h, lab.ctypes.data, len(lab), None) == _lib.QS_ERR_ARG
    assert ctx.L.qs_group_support(ctx.h, None, len(lab), C.c_void_p(buf.data_ptr())) == _lib.QS_ERR_ARG
    assert ctx.L.qs_group_support(ctx.h, lab.ctypes.data, 0, C.c_void_p(buf.data_ptr())) == _lib.QS_ERR_ARG
    bad = labels.copy()
    bad[3, 5] = 5
    assert code(lambda: ctx.group_support(bad), "hypothesis 3", "label 5") == _lib.QS_ERR_ARG
    bad = labels.copy()
    bad[4] = 0
    bad[4, :3] = [1, 2, 3]
    assert code(lambda: ctx.group_support(bad), "hypothesis 4", "no taxon carries label 4") == _lib.QS_ERR_ARG
    bad[4, :3] = [1, 1, 2]
    assert code(lambda: ctx.group_support(bad), "hypothesis 4", "only one taxon carries label 2") == _lib.QS_ERR_ARG
    # C(1500,2)^2 counted 4-sets x (2^32 - 1) does not fit 63 bits; with the trees known it does
    big = eng.Context(3000, 32, d_lo=4, d_hi=6)
    big.table_alloc()
    half = ((np.arange(3000) % 2) + 1).astype(np.uint8)[None, :]
    assert code(lambda: big.group_support(half), "hypothesis 0") == _lib.QS_ERR_OVERFLOW
    big.set_tuning(_lib.QS_TUNE_TABLE_TREES, 1000)
    r0, r1 = int(binom(4, 4)), int(binom(6, 4))
    got = big.group_support(half)                                # 14 tuples, all without a count
    assert same(got, M.model_counts(np.zeros((r1 - r0, 3), dtype=np.uint32), half, 3000, rank_lo=r0)) and got[0, 0] == got[0, 5] > 0
    assert (ctx.group_support(labels) == want).all()            # and the context still works after the refusals
