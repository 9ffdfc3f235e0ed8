"""qs_table_restrict: a count table cut down to a subset of its taxa equals the specification (tests/restrict_model.py)
cell for cell, equals the table counted from the pruned trees under the pruned reference tree, and scores like it."""
import functools

import numpy as np
import pytest

import helpers
from oracle_api import Oracle
from restrict_model import restrict_table
from quartetscores_amd import _lib, flatten, newick, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    from quartetscores_amd import engine
    return engine


# ---- addressing: every cell of a table that names its own (rank, slot) -------------------------------------------------

@functools.lru_cache(maxsize=None)
def hashed_table(n, bits):
    """(C(n,4), 3): cell (rank, slot) = a hash of (rank, slot) reduced to the cell width, so that a tuple or a slot that came
    from the wrong place shows"""
    cell = np.arange(3 * int(helpers.binom(n, 4)), dtype=np.uint64)
    h = (cell + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
    h ^= h >> np.uint64(29)
    t = (h >> np.uint64(13)).astype(np.uint32 if bits == 32 else np.uint16).reshape(-1, 3)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def uploaded(eng, n, bits):
    ctx = eng.Context(n, bits)
    ctx.table_alloc()
    ctx.table_upload(hashed_table(n, bits))
    return ctx


def kept_ids(n_src, n_dst, kind):
    ids = np.arange(n_src)
    if kind == "first":
        return ids[1:]
    if kind == "last":
        return ids[:-1]
    if kind == "middle":
        return np.delete(ids, n_src // 2)
    if kind == "second":
        return ids[::2]
    assert kind == "random"
    return np.sort(np.random.default_rng(1000 * n_src + n_dst).choice(n_src, size=n_dst, replace=False))


def restricted(eng, src, ids, bits=None):
    dst = eng.Context(len(ids), bits or src.count_bits)
    dst.table_alloc()
    dst.table_restrict(src, ids)
    dst.sync()
    return dst


SIZES = [(5, 4), (9, 9), (9, 6), (33, 23), (70, 67), (131, 129)]   # one tuple; a copy; ...; C(23,4) = 8855 crosses the first workgroup's
CELLS = [(32, 32), (16, 16), (16, 32)]                              # 8192 ranks; rows longer than a wave step; 1.1e7 tuples, rows over 128


def addressing_cases():
    def case(n_src, n_dst, kind, shuffled, cells):
        return pytest.param(n_src, n_dst, kind, shuffled, cells, id=f"{n_src}-{n_dst}-{kind}-{'any' if shuffled else 'inc'}-{cells[0]}to{cells[1]}")
    for n_src, n_dst in SIZES:                                       # the listed sizes: a seeded random kept set, every cell width
        for shuffled in (False, True):
            for cells in CELLS:
                yield case(n_src, n_dst, "random", shuffled, cells)
    for n_src in (5, 9, 33, 70, 131):                                # the named drop sets, in the source's order and in any, every width
        for kind in ("first", "last", "middle", "second"):
            n_dst = len(kept_ids(n_src, 0, kind))
            if n_dst < 4:
                continue                                             # (every second id of five taxa: three are left, no table)
            for shuffled in (False, True):
                for cells in CELLS:
                    yield case(n_src, n_dst, kind, shuffled, cells)


@pytest.mark.parametrize("n_src,n_dst,kind,shuffled,cells", list(addressing_cases()))
def test_every_cell_comes_from_the_right_place(eng, n_src, n_dst, kind, shuffled, cells):
    ids = kept_ids(n_src, n_dst, kind)
    assert len(ids) == n_dst
    if shuffled:                                                     # the general instance: any order, slots permuted
        ids = np.random.default_rng(n_src + len(ids)).permutation(ids)
        if (np.diff(ids) > 0).all():                                 # (a short permutation may come out sorted, whatever the seed)
            ids[[0, -1]] = ids[[-1, 0]]
        assert (np.diff(ids) < 0).any()
    src = uploaded(eng, n_src, cells[0])
    got = restricted(eng, src, ids, cells[1]).table_download()
    want = restrict_table(hashed_table(n_src, cells[0]), n_src, ids)
    assert got.dtype == (np.uint32 if cells[1] == 32 else np.uint16) and got.shape == want.shape
    assert (got == want).all()


def test_identity_is_a_copy(eng):
    src = uploaded(eng, 9, 32)
    assert (restricted(eng, src, np.arange(9)).table_download() == hashed_table(9, 32)).all()


@pytest.mark.parametrize("dst_bits", [16, 32])
def test_source_cells_at_65535(eng, dst_bits):
    n_src, ids = 33, kept_ids(33, 23, "random")
    src = eng.Context(n_src, 16)
    src.table_alloc()
    src.table_upload(np.full((int(helpers.binom(n_src, 4)), 3), 65535, dtype=np.uint16))
    for order in (ids, ids[::-1]):
        got = restricted(eng, src, order, dst_bits).table_download()
        assert got.shape == (8855, 3) and (got == 65535).all()


def test_a_permutation_equals_remap(eng):
    n = 33
    perm = np.random.default_rng(33).permutation(n)
    for bits in (16, 32):
        src = uploaded(eng, n, bits)
        a = restricted(eng, src, perm)
        b = eng.Context(n, bits)
        b.table_alloc()
        b.table_remap(src, perm)
        b.sync()
        assert (a.table_download() == b.table_download()).all()


# ---- against a recount of the pruned trees ------------------------------------------------------------------------------

def mixed_trees(n, seed):
    """dropout, collapsed edges and rooted trees in one batch"""
    return (synth.tree_set(n, 12, seed, dropout=0.2) + synth.tree_set(n, 12, seed + 1, collapse=0.3) +
            synth.tree_set(n, 12, seed + 2, rooted=True) + synth.tree_set(n, 6, seed + 3))


def pruned(nw, drop):
    """the tree without the taxa in `drop` as Newick text; None when fewer than four taxa are left (it holds no quartet)"""
    root = newick.prune(newick.parse_tree(nw), drop)
    if root is None or sum(x.is_leaf for x in newick.preorder(root)) < 4:
        return None
    return newick.write(root)


def counted(eng, ref, trees, bits=16):
    ctx = eng.Context(ref.n_taxa, bits)
    ctx.table_alloc()
    ctx.count_trees(flatten.flatten_eval_trees(trees, ref.name_to_id))
    return ctx


def test_restricted_table_equals_a_recount_of_the_pruned_trees(eng):
    n = 33
    ref_nw = synth.reference_tree(n, 81)
    ref = flatten.flatten_reference(ref_nw)
    trees = mixed_trees(n, 82)
    drop = [ref.names[i] for i in np.random.default_rng(83).choice(n, size=9, replace=False)]
    small_nw = pruned(ref_nw, drop)
    small = flatten.flatten_reference(small_nw)
    small_trees = [t for t in (pruned(nw, drop) for nw in trees) if t]
    for bits in (16, 32):
        src = counted(eng, ref, trees, bits)
        ids = flatten.taxon_restriction(small, ref)
        assert (np.diff(ids.astype(np.int64)) > 0).all()
        dst = restricted(eng, src, ids)
        got = dst.table_download()
        assert (got == counted(eng, small, small_trees, bits).table_download()).all()
        o = Oracle(small_nw)
        o.count("\n".join(small_trees))
        assert o.names == small.names and (got.astype(np.uint64) == o.counts()).all()
        assert dst.trees_counted == src.trees_counted == len(trees)
        assert (got == restrict_table(src.table_download(), n, ids)).all()


def by_bipartition(eng, ref, lq, qp, eqp, bif):
    q = eng.QuartetScoreComputer.__new__(eng.QuartetScoreComputer)
    q.ref, q._lq, q._qp, q._eqp = ref, lq[1:], (qp[1:] if bif else None), (eqp[1:] if bif else None)
    return q.scores_by_bipartition()


def assert_scores_equal(eng, ref, got, want, what):
    got = by_bipartition(eng, ref, *got)
    assert set(got) == set(want)
    for k in want:
        for g, w in zip(got[k], want[k]):
            assert (g is None and w is None) or int(helpers.ulp_diff(g, w)) == 0, (what, sorted(k), got[k], want[k])


@pytest.mark.parametrize("kind", ["bifurcating", "multifurcating", "rooted", "root_subtree"])
def test_scores_of_the_restricted_table_equal_the_oracle_on_the_pruned_inputs(eng, kind):
    n = 23
    rng = np.random.default_rng(91)
    ref_nw = {"bifurcating": synth.random_tree(n, rng), "multifurcating": synth.random_tree(n, rng, collapse=0.4),
              "rooted": synth.random_tree(n, rng, rooted=True), "root_subtree": synth.random_tree(n, rng)}[kind]
    ref = flatten.flatten_reference(ref_nw)
    if kind == "root_subtree":      # a whole subtree of the unrooted reference's root goes: the pruner keeps the root at degree >= 3
        sub = next(c for c in ref.root.children if 2 <= sum(x.is_leaf for x in newick.preorder(c)) <= n - 4)
        drop = [x.name for x in newick.preorder(sub) if x.is_leaf]
    else:
        drop = [ref.names[i] for i in rng.choice(n, size=6, replace=False)]
    small_nw = pruned(ref_nw, drop)
    small = flatten.flatten_reference(small_nw)
    assert len(small.root.children) == 2 if kind == "rooted" else len(small.root.children) >= 3
    trees = mixed_trees(n, 92)
    small_trees = [t for t in (pruned(nw, drop) for nw in trees) if t]
    src = counted(eng, ref, trees)
    dst = restricted(eng, src, flatten.taxon_restriction(small, ref))
    o = Oracle(small_nw)
    o.count("\n".join(small_trees))
    o.score(qp_exact64=False)
    got = dst.score(small, eng.QS_SCORE_QP_WRAP32)
    assert got[3] == o.bifurcating == (kind != "multifurcating")
    assert_scores_equal(eng, small, got, o.scores_by_bipartition(), "wrap32")
    o.score(qp_exact64=True)
    both = eng.QS_SCORE_QP_EXACT64 | eng.QS_SCORE_ROOT_AS_EDGE
    if kind == "rooted":
        # the oracle scores a degree-2 root the reference's way only: exact64 alone against it, and with ROOT_AS_EDGE the table
        # counted from the pruned trees, bit for bit
        assert_scores_equal(eng, small, dst.score(small, eng.QS_SCORE_QP_EXACT64), o.scores_by_bipartition(), "exact64")
        direct = counted(eng, small, small_trees)
        for x, y in zip(dst.score(small, both)[:3], direct.score(small, both)[:3]):
            assert (x.view(np.int64) == y.view(np.int64)).all()
    else:                           # no degree-2 root: ROOT_AS_EDGE changes nothing, the oracle is the yardstick
        assert_scores_equal(eng, small, dst.score(small, both), o.scores_by_bipartition(), "exact64 | root_as_edge")


# ---- re-use of a destination ------------------------------------------------------------------------------------------

def test_second_restrict_and_score_leave_nothing_of_the_first(eng):
    n = 26
    ref_nw = synth.reference_tree(n, 101)
    ref = flatten.flatten_reference(ref_nw)
    trees = mixed_trees(n, 102)
    src = counted(eng, ref, trees)
    rng = np.random.default_rng(103)
    drops = [[ref.names[i] for i in rng.choice(n, size=6, replace=False)] for _ in range(2)]   # both leave 20 taxa
    dst = eng.Context(n - 6, 16)
    dst.table_alloc()
    for drop in drops:
        small_nw = pruned(ref_nw, drop)
        small = flatten.flatten_reference(small_nw)
        ids = flatten.taxon_restriction(small, ref)
        dst.table_restrict(src, ids)
        dst.sync()
        assert (dst.table_download() == restrict_table(src.table_download(), n, ids)).all()
        o = Oracle(small_nw)
        o.count("\n".join(t for t in (pruned(nw, drop) for nw in trees) if t))
        o.score()
        assert_scores_equal(eng, small, dst.score(small), o.scores_by_bipartition(), drop)   # (not the log of the earlier score)
    assert drops[0] != drops[1]


# ---- refusals ---------------------------------------------------------------------------------------------------------

def test_error_codes(eng):
    n = 12
    src = uploaded(eng, n, 32)
    ids = np.arange(1, n - 1)

    def code(dst, ids=ids, source=src):
        with pytest.raises(eng.QSError) as ei:
            dst.table_restrict(source, ids)
        return ei.value.code

    dst = eng.Context(n - 2, 32)
    dst.table_alloc()
    mark = np.full((int(helpers.binom(n - 2, 4)), 3), 7, dtype=np.uint32)
    dst.table_upload(mark)
    bad = ids.copy(); bad[3] = bad[4]
    assert code(dst, bad) == _lib.QS_ERR_ARG                            # a repeated id
    bad = ids.copy(); bad[0] = n
    assert code(dst, bad) == _lib.QS_ERR_ARG                            # an id >= n_src
    larger = eng.Context(n + 1, 32)
    larger.table_alloc()
    assert code(larger, np.arange(n + 1)) == _lib.QS_ERR_ARG            # n_dst > n_src
    narrow = eng.Context(n - 2, 16)
    narrow.table_alloc()
    assert code(narrow) == _lib.QS_ERR_ARG                              # 32 -> 16 bits
    shard = eng.Context(n - 2, 32, d_lo=0, d_hi=n - 4)
    shard.table_alloc()
    assert code(shard) == _lib.QS_ERR_UNSUPPORTED                       # a table shard as destination
    src_shard = eng.Context(n, 32, d_lo=0, d_hi=n - 2)
    src_shard.table_alloc()
    assert code(dst, source=src_shard) == _lib.QS_ERR_UNSUPPORTED       # ... and as source
    assert code(eng.Context(n - 2, 32)) == _lib.QS_ERR_STATE            # a destination without a table
    assert code(dst, source=eng.Context(n, 32)) == _lib.QS_ERR_STATE    # a source without one
    dst.sync()
    assert (dst.table_download() == mark).all() and dst.trees_counted == 0   # unchanged by the refused calls
    dst.table_restrict(src, ids)                                        # and the context still works
    dst.sync()
    assert (dst.table_download() == restrict_table(hashed_table(n, 32), n, ids)).all()
