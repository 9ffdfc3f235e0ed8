"""qs_tree_agreement / Context.tree_agreement: per-tree quartet agreement with the reference tree, exact against a per-quartet
brute force, consistent with the count table, closed forms at large n, and independent of batching and rooting."""
import numpy as np
import pytest

import agreement_model as M
from helpers import binom
from quartetscores_amd import _lib, flatten, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    from quartetscores_amd import engine
    return engine


def agreement(eng, ref, trees, recentre=True, ctx=None):
    ctx = ctx or eng.Context(ref.n_taxa)
    hb = ctx.batch_upload(flatten.flatten_eval_trees(trees, ref.name_to_id, recentre))
    try:
        return ctx.tree_agreement(ref, hb)
    finally:
        ctx.batch_free(hb)


def mixed_trees(n, rng, k):
    """k evaluation trees of the synth shapes: binary, collapsed (up to a star), dropout (down to < 4 taxa), rooted."""
    out = []
    for i in range(k):
        kind = i % 6
        if kind == 0:
            out.append(synth.random_tree(n, rng))
        elif kind == 1:
            out.append(synth.random_tree(n, rng, collapse=float(rng.uniform(0.2, 1.0))))
        elif kind == 2:
            out.append(synth.random_tree(n, rng, dropout=float(rng.uniform(0.1, 0.9)), min_taxa=int(rng.integers(1, 5))))
        elif kind == 3:
            out.append(synth.random_tree(n, rng, rooted=True))
        elif kind == 4:
            out.append(synth.random_tree(n, rng, rooted=True, collapse=0.4, dropout=0.3))
        else:
            out.append(synth.random_tree(n, rng, dropout=0.2, collapse=0.3))
    return out


@pytest.mark.parametrize("ref_kind", ["binary", "multifurcating", "rooted", "star"])
def test_matches_brute_force(eng, ref_kind):
    rng = np.random.default_rng({"binary": 1, "multifurcating": 2, "rooted": 3, "star": 4}[ref_kind])
    for n in (5, 9, 17, 40):
        kw = {"binary": {}, "multifurcating": {"collapse": 0.4}, "rooted": {"rooted": True}, "star": {"collapse": 1.0}}[ref_kind]
        ref_nw = synth.random_tree(n, rng, **kw)
        ref = flatten.flatten_reference(ref_nw)
        trees = mixed_trees(n, rng, 12 if n == 40 else 24)
        got = agreement(eng, ref, trees)
        want = np.array([M.brute_counts(ref_nw, ref.names, t) for t in trees], dtype=np.uint64)
        assert (got == want).all(), (n, ref_kind, np.nonzero((got != want).any(1))[0])


def test_small_trees_give_zeros(eng):
    ref_nw = synth.reference_tree(8, 5)
    ref = flatten.flatten_reference(ref_nw)
    trees = ["(t0,t1);", "(t0,(t1,t2));", "((t3,t4),t5);", "(t1,t2,t3,t4);"]
    got = agreement(eng, ref, trees)
    assert (got[:3] == 0).all()
    assert got[3].tolist() == [0, 0, 0, 1]   # a star of 4 taxa resolves nothing; the reference resolves its quartet


@pytest.mark.parametrize("n,m", [(96, 300), (200, 240)])
def test_sums_agree_with_count_table(eng, n, m):
    rng = np.random.default_rng(n)
    ref_nw = synth.random_tree(n, rng, collapse=0.15)
    ref = flatten.flatten_reference(ref_nw)
    trees = mixed_trees(n, rng, m)
    ctx = eng.Context(n)
    ctx.table_alloc()
    b = flatten.flatten_eval_trees(trees, ref.name_to_id)
    ctx.count_trees(b)
    T = ctx.table_download().reshape(-1, 3).astype(np.int64)
    got = agreement(eng, ref, trees, ctx=ctx).astype(np.int64)
    conc = disc = eval_only = 0
    step = 1 << 23
    for r0 in range(0, len(T), step):
        nq = min(step, len(T) - r0)
        topo, _ = ctx.raw_qic(ref, r0, nq)
        Tc = T[r0:r0 + nq]
        res = topo != 255
        ref_cell = np.take_along_axis(Tc[res], topo[res].astype(np.int64)[:, None], 1)[:, 0]
        conc += int(ref_cell.sum())
        disc += int(Tc[res].sum() - ref_cell.sum())
        eval_only += int(Tc[~res].sum())
    s = got.sum(0)
    assert int(s[0]) == conc
    assert int(s[1]) == disc
    assert int(s[2] - s[0] - s[1]) == eval_only
    assert ctx.trees_counted == m   # the agreement call left the table's state alone


def _balanced(names):
    if len(names) == 1:
        return names[0]
    h = len(names) // 2
    return "(" + _balanced(names[:h]) + "," + _balanced(names[h:]) + ")"


@pytest.mark.parametrize("n", [1100, 2259])   # 2259 = the most taxa of a whole-table context (qs_create)
def test_closed_forms_large_n(eng, n):
    a, b, c = n // 7, n // 5, n // 3
    d = n - a - b - c
    names = [f"t{i}" for i in range(n)]
    A, B, C, D = names[:a], names[a:a + b], names[a + b:a + b + c], names[a + b + c:]
    ref_nw = f"({_balanced(A)},{_balanced(B)},({_balanced(C)},{_balanced(D)}));"
    nni_nw = f"({_balanced(A)},{_balanced(C)},({_balanced(B)},{_balanced(D)}));"
    ref = flatten.flatten_reference(ref_nw)
    star_nw = "(" + ",".join(names) + ");"   # one node with more links than a workgroup's LDS holds
    got = agreement(eng, ref, [ref_nw, nni_nw, star_nw]).astype(object)
    full = binom(n, 4)
    assert got[0].tolist() == [full, 0, full, full]
    assert got[1].tolist() == [full - a * b * c * d, a * b * c * d, full, full]
    assert got[2].tolist() == [0, 0, 0, full]
    assert agreement(eng, flatten.flatten_reference(star_nw), [nni_nw]).astype(object)[0].tolist() == [0, 0, full, 0]


def test_batching_recentre_and_repeat(eng):
    rng = np.random.default_rng(11)
    n = 60
    ref = flatten.flatten_reference(synth.random_tree(n, rng, rooted=True, collapse=0.2))
    trees = mixed_trees(n, rng, 90)
    ctx = eng.Context(n)
    whole = agreement(eng, ref, trees, ctx=ctx)
    parts = np.concatenate([agreement(eng, ref, trees[i:j], ctx=ctx) for i, j in ((0, 7), (7, 50), (50, 90))])
    assert (whole == parts).all()
    assert (agreement(eng, ref, trees, recentre=False, ctx=ctx) == whole).all()
    assert (agreement(eng, ref, trees, ctx=ctx) == whole).all()
    # another reference tree on the same context, then the first one again (the per-context upload is replaced)
    ref2 = flatten.flatten_reference(synth.random_tree(n, rng))
    other = agreement(eng, ref2, trees, ctx=ctx)
    want2 = np.array([M.model_tree(ref2, t) for t in trees[:10]], dtype=np.uint64)
    assert (other[:10] == want2).all()
    assert (agreement(eng, ref, trees, ctx=ctx) == whole).all()


def test_error_codes(eng):
    n = 12
    ref = flatten.flatten_reference(synth.reference_tree(n, 3))
    trees = synth.tree_set(n, 5, 4)
    b = flatten.flatten_eval_trees(trees, ref.name_to_id)
    ctx = eng.Context(n)
    hb = ctx.batch_upload(b, with_nodes=False)
    with pytest.raises(eng.QSError) as e:
        ctx.tree_agreement(ref, hb)
    assert e.value.code == _lib.QS_ERR_STATE
    ctx.batch_free(hb)
    hb = ctx.batch_upload(b)
    other = flatten.flatten_reference(synth.reference_tree(n + 1, 3))
    with pytest.raises(eng.QSError) as e:
        ctx.tree_agreement(other, hb)
    assert e.value.code == _lib.QS_ERR_ARG
    bad = flatten.flatten_reference(synth.reference_tree(n, 3))
    bad.leaf_node = bad.leaf_node.copy()
    bad.leaf_node[[0, n - 1]] = bad.leaf_node[[n - 1, 0]]   # ids 0 and n-1 swapped: not depth-first any more
    with pytest.raises(eng.QSError) as e:
        ctx.tree_agreement(bad, hb)
    assert e.value.code == _lib.QS_ERR_ARG
    ctx.batch_free(hb)
    shard = eng.Context(n, d_lo=0, d_hi=n - 2)
    hb = shard.batch_upload(b)
    with pytest.raises(eng.QSError) as e:
        shard.tree_agreement(ref, hb)
    assert e.value.code == _lib.QS_ERR_UNSUPPORTED
    shard.batch_free(hb)
    # the model agrees with the device on this set too
    ok = ctx.batch_upload(b)
    assert (ctx.tree_agreement(ref, ok) == np.array([M.model_tree(ref, t) for t in trees], dtype=np.uint64)).all()
    ctx.batch_free(ok)
