"""qs_branch_taxon_support / Context.branch_taxon_support: the four words of every (taxon, internode) and the totals, bit for bit
against the numpy model of the downloaded table (tests/branch_taxon_model.py), on the reference shapes that matter, for lists,
against qs_group_support and against the route of --without-taxa on the device, at 512 taxa through identities, with counts near
2^32, repeatable, without side effects, and every error code."""
import ctypes as C
import functools

import numpy as np
import pytest

import branch_taxon_model as M
from helpers import binom
from quartetscores_amd import _lib, flatten, newick, synth
from test_gpu_taxon_pairs import reference_of_kind
from test_gpu_taxon_placement import counted, mixed_trees, reference, special_reference

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    from quartetscores_amd import engine
    return engine


@functools.lru_cache(maxsize=None)
def planned(n, kind):
    """the reference of test_equals_model_of_the_downloaded_table and what the model derives from the tree alone: once for both cell widths"""
    ref = reference_of_kind(n, kind)
    return ref, M.plan(ref)


@pytest.mark.parametrize("kind", ["binary", "multifurcating", "rooted"])
@pytest.mark.parametrize("bits", [16, 32])
@pytest.mark.parametrize("n", [4, 5, 7, 9, 17, 33, 65, 66, 130])
def test_equals_model_of_the_downloaded_table(eng, n, bits, kind):
    ref, the_plan = planned(n, kind)
    ctx = counted(eng, ref, mixed_trees(n, 300 + n), bits)
    rows, totals = ctx.branch_taxon_support(ref)
    assert rows.dtype == np.int64 and rows.shape == (n, ref.n_nodes, 4) and totals.dtype == np.int64 and totals.shape == (ref.n_nodes, 4)
    want_rows, want_totals = M.model(ctx.table_download(), ref, the_plan)
    if n >= 5:
        assert want_rows.any() and want_totals.any()
    assert (totals == want_totals).all()
    assert (rows == want_rows).all()
    if kind == "rooted" and n >= 7:
        through = [v for v, w in M.internodes(ref) if ref.parent[v] != w]           # the edge through the root, at both children
        assert len(through) in (0, 2)
        if through:
            assert (rows[:, through[0]] == rows[:, through[1]]).all() and (totals[through[0]] == totals[through[1]]).all() and totals[through[0], 0] > 0


@pytest.mark.parametrize("bits", [16, 32])
@pytest.mark.parametrize("shape", ["ladder", "star", "wide_node"])
def test_special_reference_shapes(eng, shape, bits):
    n = 40
    ref = flatten.flatten_reference(special_reference(shape, n))
    if shape == "wide_node":
        assert np.bincount(ref.parent[ref.parent >= 0]).max() >= 5
    ctx = counted(eng, ref, mixed_trees(n, 77), bits)
    rows, totals = ctx.branch_taxon_support(ref)
    want_rows, want_totals = M.model(ctx.table_download(), ref)
    assert (rows == want_rows).all() and (totals == want_totals).all()
    if shape == "star":                      # no internode at all
        assert not rows.any() and not totals.any()
    else:
        assert rows.any()


def test_lists_give_the_rows_of_the_full_call(eng):
    n = 37
    ref = reference(n, "multifurcating", 21)
    ctx = counted(eng, ref, mixed_trees(n, 22), 16)
    every, totals = ctx.branch_taxon_support(ref)
    assert every.any() and (every.sum(axis=0) == 4 * totals).all()
    for taxa in ([30, 2, 17, 36, 0, 9], [11], [0], [n - 1], list(range(n))[::-1]):
        got, tot = ctx.branch_taxon_support(ref, taxa)
        assert got.shape == (len(taxa), ref.n_nodes, 4)
        assert (got == every[taxa]).all() and (tot == totals).all(), taxa


def test_repeatable_and_without_side_effects(eng):
    n = 48
    ref = reference(n, "binary", 12)
    trees = mixed_trees(n, 13)
    ctx = counted(eng, ref, trees, 32)
    before = ctx.table_download()
    score_before = [np.asarray(x, dtype=np.float64).view(np.int64) for x in ctx.score(ref)[:3]]
    first, totals = ctx.branch_taxon_support(ref)
    want = M.model(before, ref)
    assert (first == want[0]).all() and (totals == want[1]).all()
    again = ctx.branch_taxon_support(ref)
    assert (again[0] == first).all() and (again[1] == totals).all()
    assert (ctx.branch_taxon_support(ref, [5, 40])[0] == first[[5, 40]]).all()
    assert (ctx.branch_taxon_support(ref)[0] == first).all()
    assert (ctx.table_download() == before).all() and ctx.trees_counted == len(trees)
    for x, y in zip(score_before, [np.asarray(x, dtype=np.float64).view(np.int64) for x in ctx.score(ref)[:3]]):
        assert (x == y).all()
    # another reference tree over the same table, then the first one again: the cached reference follows the tree
    other = reference(n, "multifurcating", 99)
    perm = flatten.taxon_permutation(other, ref)
    moved = eng.Context(n, 32)
    moved.table_alloc()
    moved.table_remap(ctx, perm)
    got = moved.branch_taxon_support(other)
    want = M.model(moved.table_download(), other)
    assert (got[0] == want[0]).all() and (got[1] == want[1]).all()
    assert (ctx.branch_taxon_support(ref)[0] == first).all()


def test_against_group_support_on_the_device(eng):
    # the 4-sets around a binary internode without x are the quad hypothesis of its four links with x's label set to 0
    n = 33
    ref = reference_of_kind(n, "binary")
    ctx = counted(eng, ref, mixed_trees(n, 41), 32)
    rows, totals = ctx.branch_taxon_support(ref)
    edges = M.internodes(ref)
    rng = np.random.default_rng(42)
    labels, picks = [], []
    while len(picks) < 8:
        v, w = edges[int(rng.integers(len(edges)))]
        x = int(rng.integers(n))
        row = M.cyclic_labels(n, (tuple(M.links_at(ref, v, w)), tuple(M.links_at(ref, w, v))))
        row[x] = 0
        if all((row == k).any() for k in (1, 2, 3, 4)):
            labels.append(row)
            picks.append((v, x))
    got = ctx.group_support(np.stack(labels))
    for (v, x), words in zip(picks, got):
        assert (words[:4] == totals[v] - rows[x, v]).all(), (v, x)
    assert (got[:, 0] > 0).all()


def test_against_the_route_of_without_taxa(eng):
    """Per dropped taxon x: qs_table_restrict onto the kept ids, then qs_score of the pruned tree with exact QP sums (and the root as an
    edge, which only matters where x was a leaf at the root and the pruned root has two children: those internodes dissolve and are
    not compared). Every internode of the full tree in which x is not alone in its link keeps its id interval minus x in the
    pruned tree; its QP-IC there equals log_score(totals - row) bit for bit."""
    n = 17
    rng = np.random.default_rng(52)
    ref_nw = synth.random_tree(n, rng)
    ref = flatten.flatten_reference(ref_nw)
    parent, _, lo, hi, kids, root = M.tree_arrays(ref)
    assert len(kids[root]) == 3 and M.is_bifurcating(ref)
    ctx = counted(eng, ref, mixed_trees(n, 53), 32)
    rows, totals = ctx.branch_taxon_support(ref)
    full_qp = ctx.score(ref, eng.QS_SCORE_QP_EXACT64)[1]
    edges = M.internodes(ref)
    for v, _ in edges:
        assert np.float64(eng.log_score(*(int(z) for z in totals[v, 1:]))).view(np.int64) == np.float64(full_qp[v]).view(np.int64), v
    compared = 0
    for x in range(n):
        small = flatten.flatten_reference(newick.write(newick.prune(newick.parse_tree(ref_nw), [ref.names[x]])))
        ids = flatten.taxon_restriction(small, ref)
        dst = eng.Context(n - 1, 32)
        dst.table_alloc()
        dst.table_restrict(ctx, ids)
        qp = dst.score(small, eng.QS_SCORE_QP_EXACT64 | eng.QS_SCORE_ROOT_AS_EDGE)[1]
        _, _, slo, shi, skids, sroot = M.tree_arrays(small)
        below = {frozenset(int(i) for i in ids[slo[u]:shi[u]]): u for u in range(small.n_nodes) if skids[u] and u != sroot}
        lines = {line[2]: line for line in M.columns(ref, [x], rows[[x]], totals)}
        for v, _ in edges:
            if lines[v][5] == 1:                 # group: x alone in its link, the internode dissolves
                continue
            u = below[frozenset(range(int(lo[v]), int(hi[v]))) - {x}]
            left = [int(z) for z in totals[v] - rows[x, v]]
            got, want = np.float64(eng.log_score(*left[1:])), np.float64(qp[u])
            assert got.view(np.int64) == want.view(np.int64), (x, v, u, float(got), float(want))
            compared += 1
    assert compared >= n * (len(edges) - 2) > 0


def test_identities_at_512_taxa(eng):
    # no model at this size: every 4-set around an internode has two taxa at either end, one behind each of two links; from a small
    # count into 16-bit cells
    n = 512
    ref = reference(n, "multifurcating", 2512)
    ctx = counted(eng, ref, mixed_trees(n, 912), 16)
    rows, totals = ctx.branch_taxon_support(ref)
    assert (rows >= 0).all() and (totals >= 0).all()
    assert (totals[:, 0] == M.closed_form_quartets(ref)).all()
    assert (rows.sum(axis=0) == 4 * totals).all()
    _, _, lo, hi, _, _ = M.tree_arrays(ref)
    edges = M.internodes(ref)
    degree3 = wide = 0
    for v, w in edges:
        inside = rows[lo[v]:hi[v], v].sum(axis=0)
        assert (inside == 2 * totals[v]).all() and (rows[:, v].sum(axis=0) - inside == 2 * totals[v]).all(), v
        for end, away in ((v, w), (w, v)):
            links = M.links_at(ref, end, away)
            per_link = [rows[m, v].sum(axis=0) for m in links]
            if len(links) == 2:              # an end of degree 3: every 4-set around the internode passes through both links
                assert all((s == totals[v]).all() for s in per_link), (v, end)
                degree3 += 1
            else:
                assert (sum(per_link) == 2 * totals[v]).all() and all((s <= totals[v]).all() for s in per_link), (v, end)
                wide += 1
    on = np.zeros(ref.n_nodes, dtype=bool)
    on[[v for v, _ in edges]] = True
    assert not rows[:, ~on].any() and not totals[~on].any() and totals[on, 1].min() > 0 and degree3 and wide


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
    the_plan = M.plan(ref)
    want = M.model(table, ref, the_plan)
    assert want[0].max() > 1 << 40
    got = ctx.branch_taxon_support(ref)
    assert (got[0] == want[0]).all() and (got[1] == want[1]).all()
    # the same table, said to hold few trees (every count masked below the hint): the 32-bit partial sums
    small = (table & 0xFFF).astype(np.uint32)
    ctx.table_upload(small)
    ctx.set_tuning(_lib.QS_TUNE_TABLE_TREES, 0xFFF)
    want = M.model(small, ref, the_plan)
    got = ctx.branch_taxon_support(ref)
    assert (got[0] == want[0]).all() and (got[1] == want[1]).all()


def test_error_codes(eng):
    import torch
    n = 12
    ref = reference(n, "binary", 14)
    ctx = counted(eng, ref, mixed_trees(n, 15), 32)
    want = ctx.branch_taxon_support(ref)

    def code(f):
        with pytest.raises(eng.QSError) as ei:
            f()
        return ei.value.code

    assert code(lambda: eng.Context(n, 32).branch_taxon_support(ref)) == _lib.QS_ERR_STATE            # no table
    assert code(lambda: ctx.branch_taxon_support(reference(n + 1, "binary", 14))) == _lib.QS_ERR_ARG    # n_taxa differs
    bad = reference(n, "binary", 14)
    bad.leaf_node = bad.leaf_node.copy()
    bad.leaf_node[[0, n - 1]] = bad.leaf_node[[n - 1, 0]]   # ids 0 and n-1 swapped: not depth-first any more
    assert code(lambda: ctx.branch_taxon_support(bad)) == _lib.QS_ERR_ARG
    malformed = reference(n, "binary", 14)
    malformed.parent = np.full_like(malformed.parent, -1)
    assert code(lambda: ctx.branch_taxon_support(malformed)) == _lib.QS_ERR_ARG
    assert code(lambda: ctx.branch_taxon_support(ref, [3, n])) == _lib.QS_ERR_ARG                        # an id >= n
    assert code(lambda: ctx.branch_taxon_support(ref, [3, 5, 3])) == _lib.QS_ERR_ARG                     # repeated
    assert code(lambda: ctx.branch_taxon_support(ref, [65536 + 3])) == _lib.QS_ERR_ARG                   # (not wrapped into a 16-bit id)
    assert code(lambda: ctx.branch_taxon_support(ref, [])) == _lib.QS_ERR_ARG                            # n_list = 0
    assert code(lambda: ctx.branch_taxon_support(ref, list(range(n)) + [0])) == _lib.QS_ERR_ARG          # n_list > n_taxa
    width = ref.n_nodes * 4
    ids = np.array([3, n], dtype=np.uint16)
    out = torch.zeros(3 * width, dtype=torch.int64, device="cuda")
    s, keep = ctx._ref_struct(ref)
    call = lambda taxa, k, rows, totals: ctx.L.qs_branch_taxon_support(ctx.h, C.byref(s), taxa, k, rows, totals)
    assert call(ids.ctypes.data_as(C.c_void_p), 2, C.c_void_p(out.data_ptr()), None) == _lib.QS_ERR_ARG   # the library's own check
    ids[1] = 3
    assert call(ids.ctypes.data_as(C.c_void_p), 2, C.c_void_p(out.data_ptr()), None) == _lib.QS_ERR_ARG
    buf = torch.zeros((n + 1) * width + 1, dtype=torch.int64, device="cuda")
    assert call(None, n, C.c_void_p(buf.data_ptr() + 4), None) == _lib.QS_ERR_ARG                        # misaligned rows
    assert call(None, n, C.c_void_p(buf.data_ptr()), C.c_void_p(buf.data_ptr() + n * width * 8 + 4)) == _lib.QS_ERR_ARG   # misaligned totals
    assert call(None, n, None, None) == _lib.QS_ERR_ARG
    assert call(None, n - 1, C.c_void_p(buf.data_ptr()), None) == _lib.QS_ERR_ARG                        # NULL list: all taxa
    # totals may be NULL: the rows alone
    assert call(None, n, C.c_void_p(buf.data_ptr()), None) == _lib.QS_OK
    ctx.sync()
    assert (buf[: n * width].cpu().numpy().reshape(n, ref.n_nodes, 4) == want[0]).all()
    shard = eng.Context(n, 32, d_lo=4, d_hi=8)
    shard.table_alloc()
    assert code(lambda: shard.branch_taxon_support(ref)) == _lib.QS_ERR_UNSUPPORTED                      # a table shard
    with pytest.raises(eng.QSError, match="table-shard"):
        shard.branch_taxon_support(ref)
    # C(2999,3) x (2^32 - 1) does not fit 63 bits (only a shard of such a table can exist: the bound is looked at first)
    big_ref = reference(3000, "binary", 16)
    big = eng.Context(3000, 32, d_lo=4, d_hi=6)
    big.table_alloc()
    assert code(lambda: big.branch_taxon_support(big_ref, [0])) == _lib.QS_ERR_OVERFLOW
    del keep
    got = ctx.branch_taxon_support(ref)                        # and the context still works after the refusals
    assert (got[0] == want[0]).all() and (got[1] == want[1]).all()
