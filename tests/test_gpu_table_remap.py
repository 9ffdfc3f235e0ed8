"""qs_table_remap: a count table re-indexed into the lookup-id order of another reference tree over the same taxa
equals the table counted with that tree, bit for bit, and scores like it."""
import numpy as np
import pytest

import helpers
from helpers import binom
from oracle_api import Oracle
from quartetscores_amd import _lib, flatten, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    from quartetscores_amd import engine
    return engine


def quads_in_rank_order_fast(n):
    """helpers.quads_in_rank_order without the Python loop (C(130,4) = 11.6 M rows)."""
    ks = np.arange(n + 1)
    c4, c3, c2 = binom(ks, 4), binom(ks, 3), binom(ks, 2)
    r = np.arange(int(c4[n]), dtype=np.int64)
    d = np.searchsorted(c4, r, side="right") - 1
    r = r - c4[d]
    c = np.searchsorted(c3, r, side="right") - 1
    r = r - c3[c]
    b = np.searchsorted(c2, r, side="right") - 1
    return np.stack([r - c2[b], b, c, d], axis=1)


@pytest.fixture
def model(monkeypatch):
    """helpers.remap_table (the specification), with the vectorised quartet list."""
    assert (quads_in_rank_order_fast(9) == helpers.quads_in_rank_order(9)).all()
    monkeypatch.setattr(helpers, "quads_in_rank_order", quads_in_rank_order_fast)
    return helpers.remap_table


def mixed_trees(n, seed):
    """dropout, collapsed edges and rooted trees in one batch"""
    return (synth.tree_set(n, 12, seed, dropout=0.2) + synth.tree_set(n, 12, seed + 1, collapse=0.3) +
            synth.tree_set(n, 12, seed + 2, rooted=True) + synth.tree_set(n, 6, seed + 3))


def counted(eng, ref, trees, bits):
    ctx = eng.Context(ref.n_taxa, bits)
    ctx.table_alloc()
    ctx.count_trees(flatten.flatten_eval_trees(trees, ref.name_to_id))
    return ctx


def remapped(eng, src, ref_dst, ref_src, bits=None):
    dst = eng.Context(ref_dst.n_taxa, bits or src.count_bits)
    dst.table_alloc()
    dst.table_remap(src, flatten.taxon_permutation(ref_dst, ref_src))
    dst.sync()
    return dst


@pytest.mark.parametrize("bits", [16, 32])
@pytest.mark.parametrize("n", [4, 5, 7, 9, 17, 33, 64, 130])
def test_remapped_table_equals_model_and_direct_count(eng, model, n, bits):
    ref_a = flatten.flatten_reference(synth.reference_tree(n, 100 + n))
    ref_b = flatten.flatten_reference(synth.reference_tree(n, 200 + n))
    trees = mixed_trees(n, 300 + n)
    src = counted(eng, ref_a, trees, bits)
    dst = remapped(eng, src, ref_b, ref_a)
    got = dst.table_download()
    perm = flatten.taxon_permutation(ref_b, ref_a)
    assert (got == model(src.table_download(), perm)).all()
    assert (got == counted(eng, ref_b, trees, bits).table_download()).all()
    assert dst.trees_counted == src.trees_counted == len(trees)


def test_identity_permutation_copies(eng):
    n = 21
    ref = flatten.flatten_reference(synth.reference_tree(n, 5))
    src = counted(eng, ref, mixed_trees(n, 6), 32)
    dst = eng.Context(n, 32)
    dst.table_alloc()
    dst.table_remap(src, np.arange(n))
    dst.sync()
    assert (dst.table_download() == src.table_download()).all()


def test_second_remap_into_the_same_destination_leaves_nothing_of_the_first(eng, model):
    n = 26
    ref_a, ref_b1, ref_b2 = (flatten.flatten_reference(synth.reference_tree(n, s)) for s in (11, 12, 13))
    trees = mixed_trees(n, 14)
    src = counted(eng, ref_a, trees, 16)
    dst = eng.Context(n, 16)
    dst.table_alloc()
    dst.table_remap(src, flatten.taxon_permutation(ref_b1, ref_a))
    dst.table_remap(src, flatten.taxon_permutation(ref_b2, ref_a))
    dst.sync()
    got = dst.table_download()
    assert (got == model(src.table_download(), flatten.taxon_permutation(ref_b2, ref_a))).all()
    assert (got == counted(eng, ref_b2, trees, 16).table_download()).all()


def test_widening_16_to_32(eng, model):
    n = 19
    ref_a, ref_b = (flatten.flatten_reference(synth.reference_tree(n, s)) for s in (21, 22))
    trees = mixed_trees(n, 23)
    src = counted(eng, ref_a, trees, 16)
    dst = remapped(eng, src, ref_b, ref_a, bits=32)
    got = dst.table_download()
    assert got.dtype == np.uint32
    assert (got == model(src.table_download().astype(np.uint32), flatten.taxon_permutation(ref_b, ref_a))).all()
    assert (got == counted(eng, ref_b, trees, 32).table_download()).all()


def _by_bipartition(eng, ref, lq, qp, eqp, bif):
    q = eng.QuartetScoreComputer.__new__(eng.QuartetScoreComputer)
    q.ref, q._lq, q._qp, q._eqp = ref, lq[1:], (qp[1:] if bif else None), (eqp[1:] if bif else None)
    return q.scores_by_bipartition()


@pytest.mark.parametrize("kind", ["bifurcating", "multifurcating", "rooted"])
def test_scores_of_the_remapped_table_equal_the_oracle(eng, kind):
    n = 23
    rng = np.random.default_rng(41)
    ref_a_nw = synth.reference_tree(n, 40)
    ref_b_nw = {"bifurcating": synth.random_tree(n, rng), "multifurcating": synth.random_tree(n, rng, collapse=0.4),
                "rooted": synth.random_tree(n, rng, rooted=True)}[kind]
    ref_a, ref_b = flatten.flatten_reference(ref_a_nw), flatten.flatten_reference(ref_b_nw)
    trees = mixed_trees(n, 42)
    src = counted(eng, ref_a, trees, 16)
    dst = remapped(eng, src, ref_b, ref_a)
    o = Oracle(ref_b_nw)
    o.count("\n".join(trees))
    for exact in (False, True):
        o.score(qp_exact64=exact)
        flags = eng.QS_SCORE_QP_EXACT64 if exact else eng.QS_SCORE_QP_WRAP32
        lq, qp, eqp, bif = dst.score(ref_b, flags)
        assert bif == o.bifurcating == (kind != "multifurcating")
        got, want = _by_bipartition(eng, ref_b, lq, qp, eqp, bif), o.scores_by_bipartition()
        assert set(got) == set(want)
        for k in want:
            for g, w in zip(got[k], want[k]):
                assert (g is None and w is None) or int(helpers.ulp_diff(g, w)) == 0, (exact, sorted(k), got[k], want[k])
        # --root-as-edge: the same scores as the table counted with ref_b directly
        direct = counted(eng, ref_b, trees, 16)
        flags |= eng.QS_SCORE_ROOT_AS_EDGE
        for x, y in zip(dst.score(ref_b, flags)[:3], direct.score(ref_b, flags)[:3]):
            assert (x.view(np.int64) == y.view(np.int64)).all()


def test_error_codes(eng):
    n = 12
    ref = flatten.flatten_reference(synth.reference_tree(n, 51))
    src = counted(eng, ref, mixed_trees(n, 52), 32)
    ident = np.arange(n)

    def code(dst, perm=ident, source=src):
        with pytest.raises(eng.QSError) as ei:
            dst.table_remap(source, perm)
        return ei.value.code

    dst = eng.Context(n, 32)
    dst.table_alloc()
    bad = ident.copy(); bad[3] = bad[4]
    assert code(dst, bad) == _lib.QS_ERR_ARG                      # not a permutation (repeat)
    bad = ident.copy(); bad[0] = n
    assert code(dst, bad) == _lib.QS_ERR_ARG                      # not a permutation (out of range)
    other = eng.Context(n + 1, 32)
    other.table_alloc()
    assert code(other, np.arange(n + 1)) == _lib.QS_ERR_ARG       # n mismatch
    shard = eng.Context(n, 32, d_lo=0, d_hi=n - 2)
    shard.table_alloc()
    assert code(shard) == _lib.QS_ERR_UNSUPPORTED                 # table shard as destination
    assert code(dst, source=shard) == _lib.QS_ERR_UNSUPPORTED     # ... and as source
    assert code(eng.Context(n, 32)) == _lib.QS_ERR_STATE          # destination without a table
    assert code(dst, source=eng.Context(n, 32)) == _lib.QS_ERR_STATE
    narrow = eng.Context(n, 16)
    narrow.table_alloc()
    assert code(narrow) == _lib.QS_ERR_ARG                        # 32 -> 16 bits
    assert code(dst, source=dst) == _lib.QS_ERR_ARG               # in place
    dst.table_remap(src, ident)                                   # and the context still works after the refusals
    dst.sync()
    assert (dst.table_download() == src.table_download()).all()


def test_trees_counted_is_carried_over(eng):
    n = 10
    ref_a, ref_b = (flatten.flatten_reference(synth.reference_tree(n, s)) for s in (61, 62))
    src = counted(eng, ref_a, synth.tree_set(n, 37, 63), 16)
    dst = eng.Context(n, 16)
    dst.table_alloc()
    assert dst.trees_counted == 0
    dst.table_remap(src, flatten.taxon_permutation(ref_b, ref_a))
    assert dst.trees_counted == 37
    # the 16-bit guard of a later count in dst sees the carried-over trees
    dst.count_trees(flatten.flatten_eval_trees(synth.tree_set(n, 3, 64), ref_b.name_to_id))
    assert dst.trees_counted == 40


def test_full_size_512_taxa_u16_lookups(eng):
    n = 512
    ref_a, ref_b = (flatten.flatten_reference(synth.reference_tree(n, s)) for s in (71, 72))
    trees = synth.tree_set(n, 24, 73, dropout=0.05) + synth.tree_set(n, 24, 74)
    src = counted(eng, ref_a, trees, 16)
    dst = remapped(eng, src, ref_b, ref_a)
    perm = flatten.taxon_permutation(ref_b, ref_a).astype(np.int64)
    rng = np.random.default_rng(75)
    q = np.stack([rng.choice(n, 4, replace=False) for _ in range(100000)])
    got = dst.lookup(q)
    want = src.lookup(perm[q])          # (#ab|cd, #ac|bd, #ad|bc) in argument order: the slots follow the ids
    assert (got == want).all()
    assert got.sum() > 0
