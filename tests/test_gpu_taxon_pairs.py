"""qs_taxon_pair_support / Context.taxon_pair_support: the eight words of every taxon pair, bit for bit against the numpy model of the
downloaded table (tests/taxon_pair_model.py), on the reference shapes that matter, for lists, at 512 taxa through the identities
with qs_taxon_support, with counts near 2^32, repeatable, without side effects, and every error code."""
import ctypes as C

import numpy as np
import pytest

import taxon_model
import taxon_pair_model as M
from helpers import binom
from quartetscores_amd import _lib, flatten, synth
from test_gpu_taxon_placement import counted, mixed_trees, reference, special_reference

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    from quartetscores_amd import engine
    return engine


def reference_of_kind(n, kind):
    """the first random reference of the kind, from seed 1000 + n on, that leaves a 4-set unresolved exactly if it is multifurcating"""
    for seed in range(1000 + n, 1100 + n):
        ref = reference(n, kind, seed)
        if (taxon_model.resolved_quartets(ref) < int(binom(n, 4))) == (kind == "multifurcating"):
            return ref
    raise AssertionError((n, kind))


@pytest.mark.parametrize("kind", ["binary", "multifurcating", "rooted"])
@pytest.mark.parametrize("bits", [16, 32])
@pytest.mark.parametrize("n", [4, 5, 7, 9, 17, 33, 65, 66, 130])
def test_equals_model_of_the_downloaded_table(eng, n, bits, kind):
    ref = reference_of_kind(n, kind)
    ctx = counted(eng, ref, mixed_trees(n, 300 + n), bits)
    got = ctx.taxon_pair_support(ref)
    assert got.dtype == np.int64 and got.shape == (n, n, 8)
    want = M.pair_counts(ctx.table_download(), ref)
    assert want.any()
    if kind == "multifurcating":
        assert (want[..., 6] - want[..., 2] - want[..., 4]).any()
    assert (got == want).all()


@pytest.mark.parametrize("bits", [16, 32])
@pytest.mark.parametrize("shape", ["ladder", "star", "wide_node"])
def test_special_reference_shapes(eng, shape, bits):
    n = 40
    ref = flatten.flatten_reference(special_reference(shape, n))
    if shape == "wide_node":
        assert np.bincount(ref.parent[ref.parent >= 0]).max() >= 5
    ctx = counted(eng, ref, mixed_trees(n, 77), bits)
    got = ctx.taxon_pair_support(ref)
    assert (got == M.pair_counts(ctx.table_download(), ref)).all()
    if shape == "star":                      # no 4-set is resolved
        assert not got[..., :6].any() and got[..., 6].any() and got[..., 7].any()


def test_symmetry_and_lists(eng):
    n = 37
    ref = reference(n, "multifurcating", 21)
    ctx = counted(eng, ref, mixed_trees(n, 22), 16)
    every = ctx.taxon_pair_support(ref)
    assert (every == every.transpose(1, 0, 2)).all() and every.any()
    assert not every[np.arange(n), np.arange(n)].any()
    for taxa in ([30, 2, 17, 36, 0, 9], [11], [0], [n - 1], list(range(n))[::-1]):
        got = ctx.taxon_pair_support(ref, taxa)
        assert got.shape == (len(taxa), n, 8)
        assert (got == every[taxa]).all(), taxa


def test_identities_at_512_taxa(eng):
    # no model at this size: the identities with qs_taxon_support, from a small count into 16-bit cells
    n = 512
    ref = reference(n, "multifurcating", 2512)
    ctx = counted(eng, ref, mixed_trees(n, 912), 16)
    pairs = ctx.taxon_pair_support(ref)
    support = ctx.taxon_support(ref)
    M.check_identities(pairs, support)
    assert support[:, 1].min() > 0 and support[:, 3].sum() > 0 and (pairs >= 0).all()


def test_large_counts_take_the_wide_sums(eng):
    # counts close to 2^32 behind an uploaded 32-bit table (trees unknown): 64-bit partial sums
    n = 40
    ref = reference(n, "multifurcating", 10)
    ctx = eng.Context(n, 32)
    ctx.table_alloc()
    rng = np.random.default_rng(11)
    table = rng.integers(0, 1 << 32, size=(int(binom(n, 4)), 3), dtype=np.uint64).astype(np.uint32)
    table[rng.random(len(table)) < 0.2] = 0
    ctx.table_upload(table)
    want = M.pair_counts(table, ref)
    assert want.max() > 1 << 40
    assert (ctx.taxon_pair_support(ref) == want).all()
    # the same table, said to hold few trees (every count masked below the hint): the 32-bit partial sums
    small = (table & 0xFFF).astype(np.uint32)
    ctx.table_upload(small)
    ctx.set_tuning(_lib.QS_TUNE_TABLE_TREES, 0xFFF)
    assert (ctx.taxon_pair_support(ref) == M.pair_counts(small, ref)).all()


def test_repeatable_and_without_side_effects(eng):
    n = 48
    ref = reference(n, "binary", 12)
    trees = mixed_trees(n, 13)
    ctx = counted(eng, ref, trees, 32)
    before = ctx.table_download()
    score_before = [np.asarray(x, dtype=np.float64).view(np.int64) for x in ctx.score(ref)[:3]]
    first = ctx.taxon_pair_support(ref)
    assert (first == M.pair_counts(before, ref)).all()
    assert (ctx.taxon_pair_support(ref) == first).all()
    assert (ctx.taxon_pair_support(ref, [5, 40]) == first[[5, 40]]).all()
    assert (ctx.taxon_pair_support(ref) == first).all()
    assert (ctx.table_download() == before).all() and ctx.trees_counted == len(trees)
    for x, y in zip(score_before, [np.asarray(x, dtype=np.float64).view(np.int64) for x in ctx.score(ref)[:3]]):
        assert (x == y).all()
    # another reference tree over the same table, then the first one again: the cached reference follows the tree
    other = reference(n, "multifurcating", 99)
    perm = flatten.taxon_permutation(other, ref)
    moved = eng.Context(n, 32)
    moved.table_alloc()
    moved.table_remap(ctx, perm)
    assert (moved.taxon_pair_support(other) == M.pair_counts(moved.table_download(), other)).all()
    assert (ctx.taxon_pair_support(ref) == first).all()


def test_error_codes(eng):
    import torch
    n = 12
    ref = reference(n, "binary", 14)
    ctx = counted(eng, ref, mixed_trees(n, 15), 32)
    want = ctx.taxon_pair_support(ref)

    def code(f):
        with pytest.raises(eng.QSError) as ei:
            f()
        return ei.value.code

    assert code(lambda: eng.Context(n, 32).taxon_pair_support(ref)) == _lib.QS_ERR_STATE            # no table
    assert code(lambda: ctx.taxon_pair_support(reference(n + 1, "binary", 14))) == _lib.QS_ERR_ARG    # n_taxa differs
    bad = reference(n, "binary", 14)
    bad.leaf_node = bad.leaf_node.copy()
    bad.leaf_node[[0, n - 1]] = bad.leaf_node[[n - 1, 0]]   # ids 0 and n-1 swapped: not depth-first any more
    assert code(lambda: ctx.taxon_pair_support(bad)) == _lib.QS_ERR_ARG
    malformed = reference(n, "binary", 14)
    malformed.parent = np.full_like(malformed.parent, -1)
    assert code(lambda: ctx.taxon_pair_support(malformed)) == _lib.QS_ERR_ARG
    assert code(lambda: ctx.taxon_pair_support(ref, [3, n])) == _lib.QS_ERR_ARG                        # an id >= n
    assert code(lambda: ctx.taxon_pair_support(ref, [3, 5, 3])) == _lib.QS_ERR_ARG                     # repeated
    assert code(lambda: ctx.taxon_pair_support(ref, [65536 + 3])) == _lib.QS_ERR_ARG                   # (not wrapped into a 16-bit id)
    assert code(lambda: ctx.taxon_pair_support(ref, [])) == _lib.QS_ERR_ARG                            # n_list = 0
    assert code(lambda: ctx.taxon_pair_support(ref, list(range(n)) + [0])) == _lib.QS_ERR_ARG          # n_list > n_taxa
    ids = np.array([3, n], dtype=np.uint16)
    out = torch.zeros(2 * n * 8, dtype=torch.int64, device="cuda")
    s_, keep_ = ctx._ref_struct(ref)
    assert ctx.L.qs_taxon_pair_support(ctx.h, C.byref(s_), ids.ctypes.data_as(C.c_void_p), 2, C.c_void_p(out.data_ptr())) == _lib.QS_ERR_ARG   # the library's own check
    ids[1] = 3
    assert ctx.L.qs_taxon_pair_support(ctx.h, C.byref(s_), ids.ctypes.data_as(C.c_void_p), 2, C.c_void_p(out.data_ptr())) == _lib.QS_ERR_ARG
    buf = torch.zeros(n * n * 8 + 1, dtype=torch.int64, device="cuda")
    s, keep = ctx._ref_struct(ref)
    assert ctx.L.qs_taxon_pair_support(ctx.h, C.byref(s), None, n, C.c_void_p(buf.data_ptr() + 4)) == _lib.QS_ERR_ARG   # misaligned
    assert ctx.L.qs_taxon_pair_support(ctx.h, C.byref(s), None, n, None) == _lib.QS_ERR_ARG
    assert ctx.L.qs_taxon_pair_support(ctx.h, C.byref(s), None, n - 1, C.c_void_p(buf.data_ptr())) == _lib.QS_ERR_ARG   # NULL list: all taxa
    shard = eng.Context(n, 32, d_lo=4, d_hi=8)
    shard.table_alloc()
    assert code(lambda: shard.taxon_pair_support(ref)) == _lib.QS_ERR_UNSUPPORTED                      # a table shard
    with pytest.raises(eng.QSError, match="table-shard"):
        shard.taxon_pair_support(ref)
    # 3000 x 8 words do not fit the LDS (only a shard of such a table can exist: the size is looked at first)
    big_ref = reference(3000, "binary", 16)
    big = eng.Context(3000, 32, d_lo=4, d_hi=6)
    big.table_alloc()
    assert code(lambda: big.taxon_pair_support(big_ref, [0])) == _lib.QS_ERR_UNSUPPORTED
    with pytest.raises(eng.QSError, match="2560 taxa"):
        big.taxon_pair_support(big_ref, [0])
    assert (ctx.taxon_pair_support(ref) == want).all()            # and the context still works after the refusals
