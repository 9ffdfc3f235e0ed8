"""qs_tree_taxon_agreement / Context.tree_taxon_agreement: per tree and taxon the quartet agreement with the reference, word for word
against the numpy model (tests/tree_taxon_model.py, itself held against a per-4-set brute force), against qs_tree_agreement (row
sums) and qs_taxon_support (sums over trees) -- two other kernels --, through the rounds and the leaf-list path of its plan, at the
plan's limit, and independent of batching and repetition."""
import ctypes as C

import numpy as np
import pytest

import tree_taxon_model as M
from quartetscores_amd import _lib, flatten, synth
from tree_branch_model import mixed_trees

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    from quartetscores_amd import engine
    return engine


def words(eng, ref, trees, ctx=None, recentre=True):
    ctx = ctx or eng.Context(ref.n_taxa)
    hb = ctx.batch_upload(flatten.flatten_eval_trees(trees, ref.name_to_id, recentre))
    try:
        return ctx.tree_taxon_agreement(ref, hb)
    finally:
        ctx.batch_free(hb)


def c3(x):
    return x * (x - 1) * (x - 2) // 6


def check_against_model(eng, ref, trees, what):
    got = words(eng, ref, trees)
    assert got.shape == (len(trees), ref.n_taxa, 4) and got.dtype == np.int64
    for i, t in enumerate(trees):
        want = M.model_tree(ref, t)
        assert (got[i] == want).all(), (what, i, t, np.nonzero((got[i] != want).any(1))[0][:8], got[i][(got[i] != want).any(1)][:4], want[(got[i] != want).any(1)][:4])
    return got


@pytest.mark.parametrize("n", [8, 33, 70, 131])   # 70: more than 64 inner nodes, two node blocks (atomics); 131: rows longer than two wave steps
def test_matches_model(eng, n):
    rng = np.random.default_rng(n)
    names = [f"t{i}" for i in range(n)]
    refs = {"binary": synth.random_tree(n, rng), "collapsed": synth.random_tree(n, rng, collapse=0.2), "rooted": synth.random_tree(n, rng, rooted=True)}
    kinds = {
        "full": [synth.random_tree(n, rng) for _ in range(3)],
        "dropped": [synth.random_tree(n, rng, dropout=0.1), synth.random_tree(n, rng, dropout=0.5), synth.random_tree(n, rng, dropout=0.5, rooted=True)],
        "collapsed": [synth.random_tree(n, rng, collapse=0.2), synth.random_tree(n, rng, collapse=0.2, dropout=0.1)],
        "tiny": ["(t0,t2,(t1,t3));", "(t1,(t2,t4));", "((t0,t5),(t3,t6));"],
        "star": [M.star(names)],
        "ladder": [M.ladder([names[i] for i in rng.permutation(n)])],
    }
    for ref_kind, ref_nw in refs.items():
        ref = flatten.flatten_reference(ref_nw)
        for kind, trees in kinds.items():
            if ref_kind != "binary" and kind in ("tiny", "star", "ladder"):
                continue
            got = check_against_model(eng, ref, trees, (n, ref_kind, kind))
            if kind == "tiny":
                assert not got[1].any() and got[0].sum(0).tolist()[2] <= 4      # three taxa: zeros; four taxa: one 4-set
                assert (got[0][[ref.name_to_id[f"t{i}"] for i in range(4)], 2] == 1).all()
            if kind == "star":
                assert not got[0][:, :3].any() and (got[0][:, 3] == M.star_resolved_ref(ref, range(n))).all()
                assert (got[0][:, 3] == c3(n - 1)).all()                        # (the binary reference resolves every 4-set)
    # the multifurcating reference against a star: resolved_ref from the closed form alone
    ref = flatten.flatten_reference(refs["collapsed"])
    got = words(eng, ref, kinds["star"])
    assert (got[0][:, 3] == M.star_resolved_ref(ref, range(n))).all() and (got[0][:, 3] < c3(n - 1)).any() and not got[0][:, :3].any()
    # ladders on both sides
    lad_ref = flatten.flatten_reference(M.ladder(names))
    got = check_against_model(eng, lad_ref, kinds["ladder"] + [M.ladder(names)], (n, "ladders"))
    assert not got[1][:, 1].any() and (got[1][:, 0] == c3(n - 1)).all()         # identical: all concordant


def test_more_than_one_block_of_nodes():
    b = flatten.flatten_eval_trees([synth.random_tree(70, np.random.default_rng(0))], {f"t{i}": i for i in range(70)})
    assert int(b.node_off[1]) > M.NODES


def test_plan_is_the_models(eng):
    for n in (4, 33, 512, 1100, M.max_taxa(), M.max_taxa() + 1, 4000):
        p = eng.tree_taxa_plan(n)
        assert p["max_taxa"] == M.max_taxa() and p["flight"] == M.FLIGHT
        want = M.plan(n)
        assert p["supported"] == (want is not None)
        if want:
            assert (p["W"], p["cap"], p["nb"], p["lds_bytes"]) == want


def test_rounds_and_node_above_the_cap(eng):
    """1100 taxa: 44 link bitmaps in a round. The fan tree's blocks take several rounds; the hub has 46 links and no bitmaps."""
    n = 1100
    names = M.names_of(n)
    ref = flatten.flatten_reference(synth.random_tree(n, np.random.default_rng(1)))
    shapes = M.plan_shapes(names)
    got = check_against_model(eng, ref, list(shapes.values()), "plan shapes")
    assert got[:, :, 1].any()


def test_star_at_1100_taxa(eng):
    n = 1100
    names = M.names_of(n)
    ref = flatten.flatten_reference(synth.random_tree(n, np.random.default_rng(2)))
    got = words(eng, ref, [M.star(names), M.star(names[5:900:3])])
    assert not got[:, :, :3].any()
    assert (got[0][:, 3] == c3(n - 1)).all()
    some = [ref.name_to_id[nm] for nm in names[5:900:3]]
    want = np.zeros(n, dtype=np.int64)
    want[some] = c3(len(some) - 1)
    assert (got[1][:, 3] == want).all()


def test_one_taxon_above_the_limit(eng):
    n = M.max_taxa() + 1
    ref = flatten.flatten_reference(synth.random_tree(n, np.random.default_rng(3)))
    ctx = eng.Context(n)
    hb = ctx.batch_upload(flatten.flatten_eval_trees(["(t0,t1,(t2,t3));"], ref.name_to_id))
    with pytest.raises(eng.QSError) as e:
        ctx.tree_taxon_agreement(ref, hb)
    assert e.value.code == _lib.QS_ERR_UNSUPPORTED
    ctx.batch_free(hb)
    # ... and the limit itself runs
    n = M.max_taxa()
    ref = flatten.flatten_reference(M.ladder(M.names_of(n)))
    got = check_against_model(eng, ref, ["(t0,t1,(t2,t3));", f"((t0,t{n - 1}),t7,(t400,t{n - 2}));"], "the limit")
    assert got[0].sum(0).tolist() == [4, 0, 4, 4] and got[1].sum(0).tolist() == [4 * 1, 4 * 4, 4 * 5, 4 * 5]


def test_row_sums_are_four_times_the_tree_agreement(eng):
    """no model: two kernels that share only the bitmaps"""
    rng = np.random.default_rng(128)
    n = 128
    ref = flatten.flatten_reference(synth.random_tree(n, rng, collapse=0.15))
    trees = mixed_trees(n, rng, 200)
    ctx = eng.Context(n)
    hb = ctx.batch_upload(flatten.flatten_eval_trees(trees, ref.name_to_id))
    got = ctx.tree_taxon_agreement(ref, hb)
    agree = ctx.tree_agreement(ref, hb).astype(np.int64)
    ctx.batch_free(hb)
    assert agree[:, :2].any() and (got.sum(1) == 4 * agree).all()


def test_sums_over_trees_are_the_taxon_support(eng):
    """a third route, through the count kernel and the table"""
    rng = np.random.default_rng(64)
    n = 64
    ref = flatten.flatten_reference(synth.random_tree(n, rng, collapse=0.15))
    trees = mixed_trees(n, rng, 300)
    ctx = eng.Context(n)
    ctx.table_alloc()
    b = flatten.flatten_eval_trees(trees, ref.name_to_id)
    ctx.count_trees(b)
    support = ctx.taxon_support(ref)
    col = {name: support[:, k] for k, name in enumerate(eng.TAXON_FIELDS)}
    hb = ctx.batch_upload(b)
    got = ctx.tree_taxon_agreement(ref, hb).sum(0)
    ctx.batch_free(hb)
    assert col["discordant"].any()
    assert (got[:, 0] == col["concordant"]).all() and (got[:, 1] == col["discordant"]).all()
    assert (got[:, 2] - got[:, 0] - got[:, 1] == col["eval_only"]).all()
    assert ctx.trees_counted == 300   # the call left the table's state alone


def test_batching_and_repetition(eng):
    rng = np.random.default_rng(12)
    n = 70
    ref = flatten.flatten_reference(synth.random_tree(n, rng, rooted=True, collapse=0.2))
    trees = mixed_trees(n, rng, 30)
    ctx = eng.Context(n)
    whole = words(eng, ref, trees, ctx=ctx)
    assert (words(eng, ref, trees, ctx=ctx) == whole).all()
    assert (np.concatenate([words(eng, ref, trees[i:i + 7], ctx=ctx) for i in range(0, 30, 7)]) == whole).all()
    assert (np.concatenate([words(eng, ref, trees[i:i + 1], ctx=ctx) for i in range(30)]) == whole).all()
    assert (words(eng, ref, trees, ctx=ctx, recentre=False) == whole).all()
    # another reference on the same context, then the first again (qs_tree_agreement's cache is shared and replaced)
    ref2 = flatten.flatten_reference(synth.random_tree(n, rng))
    assert (words(eng, ref2, trees[:4], ctx=ctx) == M.model_trees(ref2, trees[:4])).all()
    assert (words(eng, ref, trees, ctx=ctx) == whole).all()


def test_error_codes(eng):
    import torch
    n = 12
    ref = flatten.flatten_reference(synth.reference_tree(n, 3))
    b = flatten.flatten_eval_trees(synth.tree_set(n, 5, 4), ref.name_to_id)
    ctx = eng.Context(n)
    hb = ctx.batch_upload(b, with_nodes=False)
    with pytest.raises(eng.QSError) as e:
        ctx.tree_taxon_agreement(ref, hb)
    assert e.value.code == _lib.QS_ERR_STATE
    ctx.batch_free(hb)
    hb = ctx.batch_upload(b)
    with pytest.raises(eng.QSError) as e:
        ctx.tree_taxon_agreement(flatten.flatten_reference(synth.reference_tree(n + 1, 3)), hb)
    assert e.value.code == _lib.QS_ERR_ARG
    s, keep = ctx._ref_struct(ref)
    buf = torch.zeros(5 * n * 4 + 1, dtype=torch.int64, device=f"cuda:{ctx.device}")
    call = ctx.L.qs_tree_taxon_agreement
    assert call(ctx.h, C.byref(s), hb, C.c_void_p(buf.data_ptr() + 4)) == _lib.QS_ERR_ARG
    assert call(ctx.h, C.byref(s), hb, None) == _lib.QS_ERR_ARG
    assert call(ctx.h, C.byref(s), None, C.c_void_p(buf.data_ptr())) == _lib.QS_ERR_ARG
    assert call(ctx.h, None, hb, C.c_void_p(buf.data_ptr())) == _lib.QS_ERR_ARG
    # ids not in depth-first order: two leaves of the reference swapped
    swapped = ref.leaf_node.copy()
    swapped[[0, n - 1]] = swapped[[n - 1, 0]]
    bad = _lib.RefTreeC(ref.n_nodes, n, ref.parent.ctypes.data, swapped.ctypes.data)
    assert call(ctx.h, C.byref(bad), hb, C.c_void_p(buf.data_ptr())) == _lib.QS_ERR_ARG
    ctx.sync()
    assert not buf.cpu().numpy().any()           # a refused call wrote nothing
    del keep
    ctx.batch_free(hb)
    shard = eng.Context(n, d_lo=0, d_hi=n - 2)
    hb = shard.batch_upload(b)
    with pytest.raises(eng.QSError) as e:
        shard.tree_taxon_agreement(ref, hb)
    assert e.value.code == _lib.QS_ERR_UNSUPPORTED
    shard.batch_free(hb)
