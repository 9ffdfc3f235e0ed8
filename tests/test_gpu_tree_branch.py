"""qs_tree_branch_support / Context.tree_branch_support and qs_branch_resample / Context.branch_resample: per tree the quartet support
of every reference internode, exact against the per-4-set brute force, against the count table's totals (another kernel), closed forms
at large n, and independent of batching, rooting and repetition; the weighted sums over trees against numpy."""
import ctypes as C

import numpy as np
import pytest

import branch_taxon_model as BM
import tree_branch_model as TB
from quartetscores_amd import _lib, flatten, synth
from tree_branch_model import REF_KINDS, mixed_trees

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    from quartetscores_amd import engine
    return engine


def support(eng, ref, trees, recentre=True, ctx=None):
    ctx = ctx or eng.Context(ref.n_taxa)
    hb = ctx.batch_upload(flatten.flatten_eval_trees(trees, ref.name_to_id, recentre))
    try:
        return ctx.tree_branch_support(ref, hb)
    finally:
        ctx.batch_free(hb)


@pytest.mark.parametrize("ref_kind", sorted(REF_KINDS))
def test_matches_brute_force(eng, ref_kind):
    rng = np.random.default_rng(sorted(REF_KINDS).index(ref_kind) + 1)
    for n in (5, 9, 17, 40, 70):   # 40: more than one bitmap word; 70: more than one block of inner nodes per tree (atomics)
        ref = flatten.flatten_reference(synth.random_tree(n, rng, **REF_KINDS[ref_kind]))
        trees = mixed_trees(n, rng, 12 if n >= 40 else 24)
        got = support(eng, ref, trees)
        assert got.shape == (len(trees), ref.n_nodes, 4) and got.dtype == np.int64
        the_plan = BM.plan(ref)
        for i, t in enumerate(trees):
            want = TB.brute_rows(ref, t, the_plan)
            assert (got[i] == want).all(), (n, ref_kind, i, t, np.nonzero((got[i] != want).any(1))[0])
        if ref_kind == "star":
            assert not got.any()


def test_more_than_one_block_of_nodes(eng):
    """the shapes above do reach the cross-block path: a binary tree of 70 taxa has 68 inner nodes, a workgroup takes at most 64"""
    b = flatten.flatten_eval_trees([synth.random_tree(70, np.random.default_rng(0))], {f"t{i}": i for i in range(70)})
    assert int(b.node_off[1]) > 64


@pytest.mark.parametrize("n,m", [(96, 300), (200, 240)])
def test_sums_agree_with_count_table(eng, n, m):
    rng = np.random.default_rng(n)
    ref = flatten.flatten_reference(synth.random_tree(n, rng, collapse=0.15))
    trees = mixed_trees(n, rng, m)
    ctx = eng.Context(n)
    ctx.table_alloc()
    b = flatten.flatten_eval_trees(trees, ref.name_to_id)
    ctx.count_trees(b)
    _, totals = ctx.branch_taxon_support(ref, taxa=[0])
    assert totals[:, 1:].any()
    got = support(eng, ref, trees, ctx=ctx)
    assert (got.sum(0)[:, 1:4] == totals[:, 1:4]).all()
    full = np.array([int(b.leaf_off[i + 1] - b.leaf_off[i]) == n for i in range(m)])
    assert full.any() and (got[full].sum(0)[:, 0] == totals[:, 0] * int(full.sum())).all()
    assert (got[:, :, 0] <= totals[None, :, 0]).all()
    assert ctx.trees_counted == m   # the call left the table's state alone


def _balanced(names):
    if len(names) == 1:
        return names[0]
    h = len(names) // 2
    return "(" + _balanced(names[:h]) + "," + _balanced(names[h:]) + ")"


def test_closed_forms_large_n(eng):
    n = 1100
    a, b, c = n // 7, n // 5, n // 3
    d = n - a - b - c
    names = [f"t{i}" for i in range(n)]
    A, B, Cc, D = names[:a], names[a:a + b], names[a + b:a + b + c], names[a + b + c:]
    ref_nw = f"({_balanced(A)},{_balanced(B)},({_balanced(Cc)},{_balanced(D)}));"
    nni_nw = f"({_balanced(A)},{_balanced(Cc)},({_balanced(B)},{_balanced(D)}));"
    star_nw = "(" + ",".join(names) + ");"   # one node with more links than a workgroup's LDS holds
    ref = flatten.flatten_reference(ref_nw)
    quartets = BM.closed_form_quartets(ref)
    got = support(eng, ref, [ref_nw, nni_nw, star_nw])
    assert (got[0, :, 0] == quartets).all() and (got[0, :, 1] == quartets).all() and not got[0, :, 2:].any()
    _, _, lo, hi, _, _ = BM.tree_arrays(ref)
    central = [v for v in range(ref.n_nodes) if lo[v] == a + b and hi[v] == n]
    assert len(central) == 1 and quartets[central[0]] == a * b * c * d
    row = got[1, central[0]].tolist()
    assert row[0] == a * b * c * d and row[1] == 0 and sorted(row[2:]) == [0, a * b * c * d]
    assert (got[1, :, 0] == quartets).all()
    assert (got[2, :, 0] == quartets).all() and not got[2, :, 1:].any()


def test_small_trees(eng):
    ref = flatten.flatten_reference(synth.reference_tree(8, 5))
    trees = ["(t0,t1);", "(t0,(t1,t2));", "((t3,t4),t5);", "(t1,t2,t3,t4);"]
    got = support(eng, ref, trees)
    assert not got[:3].any()
    assert not got[3, :, 1:].any() and set(got[3, :, 0].tolist()) <= {0, 1}
    assert (got[3] == TB.model_tree(ref, trees[3])).all()


def test_batching_recentre_and_repeat(eng):
    rng = np.random.default_rng(11)
    n = 70
    ref = flatten.flatten_reference(synth.random_tree(n, rng, rooted=True, collapse=0.2))
    trees = mixed_trees(n, rng, 60)
    ctx = eng.Context(n)
    whole = support(eng, ref, trees, ctx=ctx)
    parts = np.concatenate([support(eng, ref, trees[i:j], ctx=ctx) for i, j in ((0, 7), (7, 60))])
    assert (whole == parts).all()
    assert (support(eng, ref, trees, recentre=False, ctx=ctx) == whole).all()
    assert (support(eng, ref, trees, ctx=ctx) == whole).all()
    the_items = TB.items(ref)
    assert (whole[:8] == np.array([TB.model_tree(ref, t, the_items=the_items) for t in trees[:8]])).all()
    # another reference tree on the same context, then the first one again (the per-context upload is replaced)
    ref2 = flatten.flatten_reference(synth.random_tree(n, rng))
    other = support(eng, ref2, trees[:6], ctx=ctx)
    assert (other == np.array([TB.model_tree(ref2, t) for t in trees[:6]])).all()
    assert (support(eng, ref, trees, ctx=ctx) == whole).all()


def test_branch_resample(eng):
    rng = np.random.default_rng(7)
    n, m, B = 17, 50, 7
    ref = flatten.flatten_reference(synth.random_tree(n, rng, collapse=0.2))
    ctx = eng.Context(n)
    rows = support(eng, ref, mixed_trees(n, rng, m), ctx=ctx)
    assert rows[:, :, 1:].any()
    w = rng.integers(0, 1 << 32, size=(B, m), dtype=np.uint64).astype(np.uint32)
    want = np.einsum("rt,tnk->rnk", w.astype(np.int64), rows)
    got = ctx.branch_resample(rows, w)
    assert got.dtype == np.int64 and (got == want).all()
    half = ctx.branch_resample(rows[:23], w[:, :23])
    assert (ctx.branch_resample(rows[23:], w[:, 23:], out=half) == want).all()
    # more trees than one chunk and more replicates than one pass
    big = np.tile(rows, (7, 1, 1))[:301]
    w2 = rng.integers(0, 5, size=(35, len(big))).astype(np.uint32)
    assert (ctx.branch_resample(big, w2) == np.einsum("rt,tnk->rnk", w2.astype(np.int64), big)).all()


def test_branch_resample_overflow(eng):
    ctx = eng.Context(1100)                       # C(1100,4) = 6.07e10: a replicate of 2e8 trees could leave 63 bits
    rows = np.zeros((1, 3, 4), dtype=np.int64)
    with pytest.raises(eng.QSError) as e:
        ctx.branch_resample(rows, np.array([[1], [200_000_000]], dtype=np.uint32))
    assert e.value.code == _lib.QS_ERR_OVERFLOW
    assert not ctx.branch_resample(rows, np.array([[1], [100_000_000]], dtype=np.uint32)).any()


def test_error_codes(eng):
    import torch
    n = 12
    ref = flatten.flatten_reference(synth.reference_tree(n, 3))
    b = flatten.flatten_eval_trees(synth.tree_set(n, 5, 4), ref.name_to_id)
    ctx = eng.Context(n)
    hb = ctx.batch_upload(b, with_nodes=False)
    with pytest.raises(eng.QSError) as e:
        ctx.tree_branch_support(ref, hb)
    assert e.value.code == _lib.QS_ERR_STATE
    ctx.batch_free(hb)
    hb = ctx.batch_upload(b)
    with pytest.raises(eng.QSError) as e:
        ctx.tree_branch_support(flatten.flatten_reference(synth.reference_tree(n + 1, 3)), hb)
    assert e.value.code == _lib.QS_ERR_ARG
    s, keep = ctx._ref_struct(ref)
    buf = torch.zeros(5 * ref.n_nodes * 4 + 1, dtype=torch.int64, device=f"cuda:{ctx.device}")
    assert ctx.L.qs_tree_branch_support(ctx.h, C.byref(s), hb, C.c_void_p(buf.data_ptr() + 4)) == _lib.QS_ERR_ARG
    assert ctx.L.qs_tree_branch_support(ctx.h, C.byref(s), hb, None) == _lib.QS_ERR_ARG
    assert ctx.L.qs_tree_branch_support(ctx.h, C.byref(s), None, C.c_void_p(buf.data_ptr())) == _lib.QS_ERR_ARG
    w = np.ones((1, 5), dtype=np.uint32)
    assert ctx.L.qs_branch_resample(ctx.h, C.c_void_p(buf.data_ptr()), 5, ref.n_nodes, w.ctypes.data_as(C.c_void_p), 1, C.c_void_p(buf.data_ptr() + 4)) == _lib.QS_ERR_ARG
    assert ctx.L.qs_branch_resample(ctx.h, C.c_void_p(buf.data_ptr()), 5, ref.n_nodes, None, 1, C.c_void_p(buf.data_ptr())) == _lib.QS_ERR_ARG
    ctx.sync()
    assert not buf.cpu().numpy().any()           # a refused call wrote nothing
    del keep
    ctx.batch_free(hb)
    shard = eng.Context(n, d_lo=0, d_hi=n - 2)
    hb = shard.batch_upload(b)
    with pytest.raises(eng.QSError) as e:
        shard.tree_branch_support(ref, hb)
    assert e.value.code == _lib.QS_ERR_UNSUPPORTED
    shard.batch_free(hb)
