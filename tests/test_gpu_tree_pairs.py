"""qs_tree_pair_agreement / Context.tree_pair_agreement: quartet agreement of the evaluation trees with each other, exact against a
per-quartet brute force and the numpy model, consistent with qs_tree_agreement, independent of how a square is cut into calls,
closed forms at large n, and the error table. All comparisons are exact integers."""
import ctypes as C

import numpy as np
import pytest

import agreement_model as M
import tree_pairs_model as P
from helpers import binom
from quartetscores_amd import _lib, flatten, synth
from test_gpu_tree_agreement import _balanced, mixed_trees

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    from quartetscores_amd import engine
    return engine


def names_of(n):
    return [f"t{i}" for i in range(n)]


def ids_of(n):
    return {nm: i for i, nm in enumerate(names_of(n))}


def square(eng, n, trees, ctx=None, recentre=True, **kw):
    ctx = ctx or eng.Context(n)
    hb = ctx.batch_upload(flatten.flatten_eval_trees(trees, ids_of(n), recentre))
    try:
        return ctx.tree_pair_agreement(hb, **kw).astype(np.int64)
    finally:
        ctx.batch_free(hb)


@pytest.mark.parametrize("n", [5, 9, 17])
def test_matches_brute_force(eng, n):
    rng = np.random.default_rng(300 + n)
    trees = mixed_trees(n, rng, 12)
    got = square(eng, n, trees)
    want = np.array([[P.brute_pair(names_of(n), s, t) for t in trees] for s in trees], dtype=np.int64)
    assert (got == want).all(), (n, np.argwhere((got != want).any(2)))
    d = got[np.arange(12), np.arange(12)]   # the diagonal: nothing discordant, everything resolved is concordant
    assert (d[:, 1] == 0).all() and (d[:, 0] == d[:, 2]).all() and (d[:, 0] == d[:, 3]).all()


def test_matches_brute_force_40(eng):
    n = 40
    rng = np.random.default_rng(340)
    trees = mixed_trees(n, rng, 6)
    got = square(eng, n, trees, upper=True)
    for a in range(6):
        for b in range(6):
            want = P.brute_pair(names_of(n), trees[a], trees[b]) if a < b else (0, 0, 0, 0, 0)
            assert tuple(got[a, b]) == want, (a, b)


@pytest.fixture(scope="module")
def dropout_96(eng):
    """five trees of 96 taxa that all lack taxa (several bitmap words; the largest needs two node blocks), and their square"""
    n = 96
    rng = np.random.default_rng(96)
    trees = [synth.random_tree(n, rng, dropout=0.1), synth.random_tree(n, rng, dropout=0.15, collapse=0.1),
             synth.random_tree(n, rng, dropout=0.3, rooted=True), synth.random_tree(n, rng, dropout=0.2, collapse=0.3),
             synth.random_tree(n, rng, dropout=0.12, rooted=True, collapse=0.05)]
    b = flatten.flatten_eval_trees(trees, ids_of(n))
    assert (np.diff(b.leaf_off) < n).all()
    assert np.diff(b.node_off).max() > 64   # agree_plan: 64 inner nodes per workgroup
    return trees, square(eng, n, trees)


@pytest.mark.parametrize("part", [0, 1])
def test_matches_model_96(dropout_96, part):
    trees, got = dropout_96
    pairs = [(a, b) for a in range(5) for b in range(a + 1, 5)]
    assert len(pairs) == 10
    for k, (a, b) in enumerate(pairs[5 * part:5 * part + 5]):
        s, t = (a, b) if k % 2 == 0 else (b, a)   # both orders take part
        assert tuple(got[s, t]) == P.model_pair(96, ids_of(96), trees[s], trees[t]), (s, t)


@pytest.mark.parametrize("n", [96, 200])
def test_consistent_with_tree_agreement(eng, n):
    rng = np.random.default_rng(400 + n)
    trees = mixed_trees(n, rng, 24)
    ctx = eng.Context(n)
    sq = square(eng, n, trees, ctx=ctx)
    assert (sq == P.swapped(sq.transpose(1, 0, 2))).all()
    complete = [i for i in range(24) if sq[i, i, 4] == n]
    assert len(complete) >= 8
    for i in complete:
        ref = flatten.flatten_reference(trees[i])
        hb = ctx.batch_upload(flatten.flatten_eval_trees(trees, ref.name_to_id))
        want = ctx.tree_agreement(ref, hb).astype(np.int64)
        ctx.batch_free(hb)
        assert (sq[i][:, [0, 1, 3, 2]] == want).all(), (n, i)


def test_independent_of_decomposition(eng):
    n, m = 60, 30
    rng = np.random.default_rng(60)
    trees = mixed_trees(n, rng, m)
    ctx = eng.Context(n)
    ids = ids_of(n)
    hb = ctx.batch_upload(flatten.flatten_eval_trees(trees, ids))
    whole = ctx.tree_pair_agreement(hb)
    assert whole.shape == (m, m, 5)
    tiles = np.zeros_like(whole)
    for r0, r1 in ((0, 7), (7, 19), (19, 30)):
        for c0, c1 in ((0, 11), (11, 30)):
            tiles[r0:r1, c0:c1] = ctx.tree_pair_agreement(hb, rows=(r0, r1), cols=(c0, c1))
    assert (tiles == whole).all()
    assert (ctx.tree_pair_agreement(hb) == whole).all()   # a repeated call
    # two separately uploaded batches as rows and columns
    hr = ctx.batch_upload(flatten.flatten_eval_trees(trees[3:17], ids))
    hc = ctx.batch_upload(flatten.flatten_eval_trees(trees[10:], ids))
    assert (ctx.tree_pair_agreement(hr, hc) == whole[3:17, 10:]).all()
    assert (ctx.tree_pair_agreement(hr, hc, rows=(2, 9), cols=(1, 20)) == whole[5:12, 11:30]).all()
    ctx.batch_free(hr)
    ctx.batch_free(hc)
    # another rooting of every tree
    hn = ctx.batch_upload(flatten.flatten_eval_trees(trees, ids, recentre=False))
    assert (ctx.tree_pair_agreement(hn) == whole).all()
    assert (ctx.tree_pair_agreement(hn, hb) == whole).all()
    ctx.batch_free(hn)
    # the upper triangle
    up = ctx.tree_pair_agreement(hb, upper=True)
    above = np.triu(np.ones((m, m), dtype=bool), 1)
    assert (up[above] == whole[above]).all() and (up[~above] == 0).all()
    part = ctx.tree_pair_agreement(hb, rows=(4, 13), cols=(2, 25), upper=True)
    assert (part == up[4:13, 2:25]).all()
    assert ctx.tree_pair_agreement(hb, rows=(5, 5)).shape == (0, m, 5)   # an empty range is no error
    ctx.batch_free(hb)


def _closed_form_trees(n):
    a, b, c = n // 7, n // 5, n // 3
    d = n - a - b - c
    names = names_of(n)
    A, B, Cc, D = names[:a], names[a:a + b], names[a + b:a + b + c], names[a + b + c:]
    bal = f"({_balanced(A)},{_balanced(B)},({_balanced(Cc)},{_balanced(D)}));"
    nni = f"({_balanced(A)},{_balanced(Cc)},({_balanced(B)},{_balanced(D)}));"
    star = "(" + ",".join(names) + ");"
    return bal, nni, star, a * b * c * d


def test_closed_forms_600(eng):
    # a star of 600 leaves has more links than one round's LDS budget (agree_plan: 256 links at this size): the unstored path
    n = 600
    bal, nni, star, abcd = _closed_form_trees(n)
    full = binom(n, 4)
    ctx = eng.Context(n)
    hb = ctx.batch_upload(flatten.flatten_eval_trees([bal, nni, star], ids_of(n)))
    top = ctx.tree_pair_agreement(hb, rows=(0, 2), cols=(0, 3)).astype(object)    # the two rectangles leave out (star, star)
    bottom = ctx.tree_pair_agreement(hb, rows=(2, 3), cols=(0, 2)).astype(object)
    ctx.batch_free(hb)
    assert top[0, 0].tolist() == [full, 0, full, full, n]
    assert top[0, 1].tolist() == [full - abcd, abcd, full, full, n]
    assert top[1, 0].tolist() == [full - abcd, abcd, full, full, n]
    for r in range(2):
        assert top[r, 2].tolist() == [0, 0, full, 0, n]       # the star as column
        assert bottom[0, r].tolist() == [0, 0, 0, full, n]    # the star as row


def test_closed_forms_2259(eng):
    n = 2259   # the most taxa of a whole-table context (qs_create)
    bal, nni, _, abcd = _closed_form_trees(n)
    full = binom(n, 4)
    ctx = eng.Context(n)
    hb = ctx.batch_upload(flatten.flatten_eval_trees([bal, nni], ids_of(n)))
    got = ctx.tree_pair_agreement(hb, rows=(0, 1), cols=(1, 2)).astype(object)
    ctx.batch_free(hb)
    assert got[0, 0].tolist() == [full - abcd, abcd, full, full, n]


def test_few_shared_taxa_give_zeros(eng):
    n = 10
    trees = ["(t0,t1);", "(t0,(t1,t2));", "((t0,t1),(t2,t3),(t4,t5));", "((t4,t5),(t6,t7),t3);", "((t6,t7),(t8,t9));",
             "((t0,t2),(t1,t3),(t4,t6),(t5,t7));"]
    got = square(eng, n, trees)
    sets = [P.taxa_of(t, ids_of(n)) for t in trees]
    for a in range(len(trees)):
        for b in range(len(trees)):
            shared = len(sets[a] & sets[b])
            assert got[a, b, 4] == shared
            if shared < 4:
                assert (got[a, b, :4] == 0).all(), (a, b)
            assert tuple(got[a, b]) == P.brute_pair(names_of(n), trees[a], trees[b]), (a, b)
    assert got[2, 3].tolist() == [0, 0, 0, 0, 3] and got[3, 4].tolist() == [0, 0, 0, 0, 2] and got[0, 4].tolist() == [0, 0, 0, 0, 0]
    assert got[2, 5, 4] == 6 and got[2, 5, :4].any()


def _replicated(b, k):
    """k copies of the one tree of batch b, without flattening k trees"""
    L, nn, nl = int(b.leaf_off[1]), int(b.node_off[1]), int(b.rng_off[-1])
    rng_off = (np.arange(k, dtype=np.int64)[:, None] * nl + b.rng_off[None, :-1].astype(np.int64)).reshape(-1)
    return flatten.TreeBatch(k, (np.arange(k + 1) * L).astype(np.uint32), np.tile(b.leaf_ids, k), np.tile(b.adj_depth, k),
                             (np.arange(k + 1) * nn).astype(np.uint32), np.concatenate([rng_off, [k * nl]]).astype(np.uint32),
                             np.tile(b.ranges, k))


def test_error_codes(eng):
    import torch
    n = 12
    ids = ids_of(n)
    trees = synth.tree_set(n, 5, 4)
    b = flatten.flatten_eval_trees(trees, ids)
    ctx = eng.Context(n)
    ctx.table_alloc()
    ctx.count_trees(b)
    table = ctx.table_download().copy()
    hb = ctx.batch_upload(b)
    other = ctx.batch_upload(b)
    bare = ctx.batch_upload(b, with_nodes=False)
    buf = torch.zeros(5 * 25 + 1, dtype=torch.int64, device="cuda")

    def code(call):
        with pytest.raises(eng.QSError) as e:
            call()
        return e.value.code

    def raw(rows, r0, r1, cols, c0, c1, flags, ptr):
        ctx._chk(ctx.L.qs_tree_pair_agreement(ctx.h, rows, r0, r1, cols, c0, c1, flags, C.c_void_p(ptr)))

    assert code(lambda: ctx.tree_pair_agreement(bare)) == _lib.QS_ERR_STATE
    assert code(lambda: ctx.tree_pair_agreement(hb, bare)) == _lib.QS_ERR_STATE
    assert code(lambda: ctx.tree_pair_agreement(bare, hb)) == _lib.QS_ERR_STATE
    assert code(lambda: raw(hb, 0, 5, hb, 0, 5, 0, None)) == _lib.QS_ERR_ARG
    assert code(lambda: raw(None, 0, 5, hb, 0, 5, 0, buf.data_ptr())) == _lib.QS_ERR_ARG
    assert code(lambda: raw(hb, 0, 5, None, 0, 5, 0, buf.data_ptr())) == _lib.QS_ERR_ARG
    assert code(lambda: raw(hb, 0, 5, hb, 0, 5, 0, buf.data_ptr() + 4)) == _lib.QS_ERR_ARG
    assert code(lambda: ctx.tree_pair_agreement(hb, rows=(3, 2))) == _lib.QS_ERR_ARG
    assert code(lambda: ctx.tree_pair_agreement(hb, rows=(0, 6))) == _lib.QS_ERR_ARG
    assert code(lambda: ctx.tree_pair_agreement(hb, cols=(3, 2))) == _lib.QS_ERR_ARG
    assert code(lambda: ctx.tree_pair_agreement(hb, cols=(0, 6))) == _lib.QS_ERR_ARG
    assert code(lambda: raw(hb, 0, 5, hb, 0, 5, 2, buf.data_ptr())) == _lib.QS_ERR_ARG
    assert code(lambda: raw(hb, 0, 5, hb, 0, 5, 1 | 4, buf.data_ptr())) == _lib.QS_ERR_ARG
    assert code(lambda: ctx.tree_pair_agreement(hb, other, upper=True)) == _lib.QS_ERR_ARG
    # more than 2^28 pairs: 16385 x 16385 trees (refused before anything is allocated or launched)
    many = ctx.batch_upload(_replicated(flatten.flatten_eval_trees(trees[:1], ids), 16385))
    assert code(lambda: raw(many, 0, 16385, many, 0, 16385, 0, buf.data_ptr())) == _lib.QS_ERR_ARG
    assert code(lambda: raw(many, 0, 16385, many, 0, 16385, _lib.QS_PAIRS_UPPER, buf.data_ptr())) == _lib.QS_ERR_ARG
    raw(many, 16380, 16385, many, 3, 8, 0, buf.data_ptr())   # a window of it is fine
    ctx.sync()
    ctx.batch_free(many)
    shard = eng.Context(n, d_lo=0, d_hi=n - 2)
    hs = shard.batch_upload(b)
    assert code(lambda: shard.tree_pair_agreement(hs)) == _lib.QS_ERR_UNSUPPORTED
    shard.batch_free(hs)
    # after all the refusals the context still answers, and neither the table nor trees-counted has changed
    got = ctx.tree_pair_agreement(hb, other).astype(np.int64)
    want = np.array([[P.model_pair(n, ids, s, t) for t in trees] for s in trees], dtype=np.int64)
    assert (got == want).all()
    assert ctx.trees_counted == 5
    assert (ctx.table_download() == table).all()
    for h in (hb, other, bare):
        ctx.batch_free(h)
