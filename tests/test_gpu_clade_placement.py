"""qs_clade_placement / Context.clade_placement: the link sums of the quartet placement of clades, bit for bit against the numpy
model of the downloaded table (tests/clade_placement_model.py): every eligible clade at small sizes, chosen clades at 65 and 130
taxa, the reference shapes whose runs span the jumped interval, lists, a list whose clades hold more than 65535 taxa together,
counts near 2^32, repeatable, without side effects, and every error code."""
import ctypes as C

import numpy as np
import pytest

import clade_placement_model as CM
import placement_model as P
from helpers import binom
from quartetscores_amd import _lib, flatten, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    from quartetscores_amd import engine
    return engine


def mixed_trees(n, seed):
    """dropout, collapsed edges and rooted trees in one batch (as tests/test_gpu_taxon_placement.py)"""
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


def movable(ref):
    """every non-root node with at least three taxa outside it, leaves included, and the tree's shape"""
    S = P.Shape(ref)
    return [v for v in range(S.N) if v != S.root and S.n - (S.hi[v] - S.lo[v]) >= 3], S


@pytest.mark.parametrize("kind", ["binary", "multifurcating", "rooted"])
@pytest.mark.parametrize("bits", [16, 32])
@pytest.mark.parametrize("n", [5, 6, 7, 9, 17, 33])
def test_every_eligible_clade_equals_the_model_of_the_downloaded_table(eng, n, bits, kind):
    ref = reference(n, kind, 1000 + n)
    ctx = counted(eng, ref, mixed_trees(n, 300 + n), bits)
    nodes = CM.eligible(ref) + [int(ref.leaf_node[1]), int(ref.leaf_node[n - 1])]
    assert list(eng.eligible_clades(ref)) == nodes[:-2]
    got = ctx.clade_placement(ref, nodes)
    assert got.dtype == np.int64 and got.shape == (len(nodes), 2 * ref.n_nodes)
    want = CM.link_sums(ctx.table_download(), ref, nodes)
    assert (got == want).all()
    assert want.sum() > 0
    if len(nodes) > 2:
        assert (ctx.clade_placement(ref) == want[:-2]).all()         # the default list: the eligible clades in node order


def six_clades(ref):
    """the smallest and the largest eligible clade, one with lo = 0, one with hi = n (the largest such nodes that may move: a leaf
    where the tree offers no other), and two eligible ones in the middle"""
    nodes, S = movable(ref)
    size = lambda v: int(S.hi[v] - S.lo[v])
    el = sorted(CM.eligible(ref), key=lambda v: (size(v), v))
    first = max((v for v in nodes if S.lo[v] == 0), key=size)
    last = max((v for v in nodes if S.hi[v] == S.n), key=size)
    inside = [v for v in el if S.lo[v] > 0 and S.hi[v] < S.n and v not in (el[0], el[-1])]
    picked = [el[0], el[-1], first, last, inside[len(inside) // 2], inside[-1]]
    out = []
    for v in picked:                                                 # distinct: a tree may offer one node for two roles
        out.append(v if v not in out else next(w for w in el if w not in out and w not in picked))
    return out, S


@pytest.mark.parametrize("kind", ["binary", "multifurcating", "rooted"])
@pytest.mark.parametrize("bits", [16, 32])
@pytest.mark.parametrize("n", [65, 130])
def test_six_clades_equal_the_model_of_the_downloaded_table(eng, n, bits, kind):
    ref = reference(n, kind, 1000 + n)
    ctx = counted(eng, ref, mixed_trees(n, 300 + n), bits)
    nodes, S = six_clades(ref)
    assert len(set(nodes)) == 6 and min(S.lo[v] for v in nodes) == 0 and max(S.hi[v] for v in nodes) == n
    got = ctx.clade_placement(ref, nodes)
    want = CM.link_sums(ctx.table_download(), ref, nodes)
    assert (got == want).all()
    assert (want.sum(axis=1) > 0).all()


def special_reference(shape, n):
    names = [f"t{i}" for i in np.random.default_rng(5).permutation(n)]
    if shape == "ladder":            # every clade is a suffix of the ids: hi = n, no second stretch
        return P.caterpillar(names) + ";"
    if shape == "ladder_left":       # every clade is a prefix of the ids: lo = 0, no first stretch
        text = names[0]
        for x in names[1:]:
            text = "(" + text + "," + x + ")"
        return text + ";"
    # a node with six children, every child a small clade, beside a caterpillar: seen from the caterpillar the child of the root
    # that holds p is the same on both sides of such a clade, and the clades' parent is a multifurcation
    clades = ["(" + ",".join(names[i:i + 4]) + ")" for i in range(0, 24, 4)]
    return "((" + ",".join(clades) + ")," + P.caterpillar(names[24:]) + ");"


def run_spans(S, node):
    """is there a middle id q behind the clade for which the run of place_next that holds the last id before the clade goes on
    behind it: the same lca(p,q) and the same child of it towards p on both sides of the jumped interval"""
    lo, hi = int(S.lo[node]), int(S.hi[node])
    if lo == 0 or hi >= S.n - 1:
        return False
    return any(S.lca[lo - 1, q] == S.lca[hi, q] and S.child_to[S.lca[hi, q], lo - 1] == S.child_to[S.lca[hi, q], hi] for q in range(hi + 1, S.n - 1))


@pytest.mark.parametrize("bits", [16, 32])
@pytest.mark.parametrize("shape", ["ladder", "ladder_left", "wide_node"])
def test_special_reference_shapes(eng, shape, bits):
    n = 40
    ref = flatten.flatten_reference(special_reference(shape, n))
    el, S = CM.eligible(ref), P.Shape(ref)
    if shape == "wide_node":
        nodes = el
        wide = int(np.argmax(S.nchild))
        assert S.nchild[wide] == 6 and sum(S.parent[v] == wide for v in nodes) == 6      # clades below a multifurcation
        assert sum(run_spans(S, v) for v in nodes) >= 4                                  # runs that cross the jumped interval
    else:
        by_size = sorted(el, key=lambda v: S.hi[v] - S.lo[v])
        nodes = by_size[:3] + by_size[len(el) // 2 - 1:len(el) // 2 + 2] + by_size[-3:]  # both ends and the middle
        assert all((S.hi[v] == n) if shape == "ladder" else (S.lo[v] == 0) for v in nodes)
    ctx = counted(eng, ref, mixed_trees(n, 77), bits)
    got = ctx.clade_placement(ref, nodes)
    assert (got == CM.link_sums(ctx.table_download(), ref, nodes)).all()


def test_list_semantics(eng):
    n = 37
    ref = reference(n, "multifurcating", 21)
    ctx = counted(eng, ref, mixed_trees(n, 22), 16)
    nodes, S = movable(ref)
    every = ctx.clade_placement(ref, nodes)
    assert (every == CM.link_sums(ctx.table_download(), ref, nodes)).all()
    row = {v: i for i, v in enumerate(nodes)}
    el = CM.eligible(ref)
    for part in (el[::3], [el[-1]], [el[0]], nodes[::-1], [nodes[5], nodes[1], nodes[-1]]):
        got = ctx.clade_placement(ref, part)
        assert got.shape == (len(part), 2 * ref.n_nodes)
        assert (got == every[[row[v] for v in part]]).all(), part
    # a leaf's row is the taxon's row of qs_taxon_placement
    taxa = [0, 9, 17, n - 1]
    leaves = [int(ref.leaf_node[x]) for x in taxa]
    assert (ctx.clade_placement(ref, leaves) == ctx.taxon_placement(ref, taxa)).all()


def test_more_than_65535_clade_taxa_in_one_call(eng):
    # a 380-taxon ladder: the clades of the list hold about 72 000 taxa together, more than a grid dimension of (clade, x) could be.
    # A constant table of 3 in 16-bit cells, attached (nothing is uploaded), against the closed form
    import torch
    n = 380
    ref = flatten.flatten_reference(P.caterpillar([f"t{i}" for i in range(n)]) + ";")
    S = P.Shape(ref)
    nodes = CM.eligible(ref)
    assert sum(int(S.hi[v] - S.lo[v]) for v in nodes) > 65535
    ctx = eng.Context(n, 16)
    assert ctx.table_bytes == int(binom(n, 4)) * 3 * 2
    table = torch.full(((ctx.table_bytes + 3) // 4 * 2,), 3, dtype=torch.int16, device="cuda")   # (a multiple of 4 bytes)
    ctx.table_attach(table)
    got = ctx.clade_placement(ref)
    want = np.stack([CM.constant_links(ref, v, 3, S) for v in nodes])
    assert got.shape == want.shape and (got == want).all()
    ctx.table_attach(None)


def test_large_counts_take_the_wide_sums(eng):
    # counts close to 2^32 behind an uploaded 32-bit table (trees unknown): 64-bit partial sums
    n = 40
    ref = reference(n, "multifurcating", 10)
    nodes, S = movable(ref)
    big = max(nodes, key=lambda v: (S.hi[v] - S.lo[v]) * (n - (S.hi[v] - S.lo[v])))
    size = int(S.hi[big] - S.lo[big])
    assert size >= 8
    ctx = eng.Context(n, 32)
    ctx.table_alloc()
    rng = np.random.default_rng(11)
    table = rng.integers(0, 1 << 32, size=(int(binom(n, 4)), 3), dtype=np.uint64).astype(np.uint32)
    table[rng.random(len(table)) < 0.2] = 0
    ctx.table_upload(table)
    want = CM.link_sums(table, ref, nodes)                           # (exact int64 sums)
    assert want.max() > 1 << 40
    assert (ctx.clade_placement(ref, nodes) == want).all()
    # the same table, said to hold few trees (every count masked below the hint): the 32-bit partial sums
    small = (table & 0xFFF).astype(np.uint32)
    ctx.table_upload(small)
    ctx.set_tuning(_lib.QS_TUNE_TABLE_TREES, 0xFFF)
    assert (ctx.clade_placement(ref, nodes) == CM.link_sums(small, ref, nodes)).all()
    # counts below 2^27: a walk of one x would still fit 32 bits ((n - |C|) x 2^27 < 2^32), the sums over the large clade's x
    # would not (x |C|, at half the largest count on average), so the host's bound has to count the clade's taxa
    assert (n - size) << 27 < 1 << 32 <= ((n - size) * size) << 26
    mid = (table & 0x7FFFFFF).astype(np.uint32)
    ctx.table_upload(mid)
    ctx.set_tuning(_lib.QS_TUNE_TABLE_TREES, 0x7FFFFFF)
    want = CM.link_sums(mid, ref, [big])
    assert want.max() > 1 << 32
    assert (ctx.clade_placement(ref, [big]) == want).all()


def test_repeatable_and_without_side_effects(eng):
    n = 48
    ref = reference(n, "binary", 12)
    trees = mixed_trees(n, 13)
    ctx = counted(eng, ref, trees, 32)
    before = ctx.table_download()
    score_before = [np.asarray(x, dtype=np.float64).view(np.int64) for x in ctx.score(ref)[:3]]
    taxa_before = ctx.taxon_placement(ref)
    nodes = CM.eligible(ref)
    first = ctx.clade_placement(ref)
    assert (first == CM.link_sums(before, ref, nodes)).all()
    assert (ctx.clade_placement(ref) == first).all()
    assert (ctx.clade_placement(ref, [nodes[5], nodes[20]]) == first[[5, 20]]).all()
    assert (ctx.taxon_placement(ref) == taxa_before).all()
    assert (ctx.clade_placement(ref) == first).all()
    assert (ctx.table_download() == before).all() and ctx.trees_counted == len(trees)
    for x, y in zip(score_before, [np.asarray(x, dtype=np.float64).view(np.int64) for x in ctx.score(ref)[:3]]):
        assert (x == y).all()
    # another reference tree over the same table, then the first one again: the cached link lookups follow the tree
    other = reference(n, "multifurcating", 99)
    perm = flatten.taxon_permutation(other, ref)
    moved = eng.Context(n, 32)
    moved.table_alloc()
    moved.table_remap(ctx, perm)
    assert (moved.clade_placement(other) == CM.link_sums(moved.table_download(), other, CM.eligible(other))).all()
    assert (ctx.clade_placement(ref) == first).all()


def test_error_codes(eng):
    import torch
    n = 12
    ref = reference(n, "binary", 14)
    ctx = counted(eng, ref, mixed_trees(n, 15), 32)
    want = ctx.clade_placement(ref)
    nodes, S = movable(ref)
    el = CM.eligible(ref)

    def code(f):
        with pytest.raises(eng.QSError) as ei:
            f()
        return ei.value.code

    assert code(lambda: eng.Context(n, 32).clade_placement(ref)) == _lib.QS_ERR_STATE            # no table
    assert code(lambda: ctx.clade_placement(reference(n + 1, "binary", 14))) == _lib.QS_ERR_ARG    # n_taxa differs
    bad = reference(n, "binary", 14)
    bad.leaf_node = bad.leaf_node.copy()
    bad.leaf_node[[0, n - 1]] = bad.leaf_node[[n - 1, 0]]   # ids 0 and n-1 swapped: not depth-first any more
    assert code(lambda: ctx.clade_placement(bad, el[:1])) == _lib.QS_ERR_ARG
    malformed = reference(n, "binary", 14)
    malformed.parent = np.full_like(malformed.parent, -1)
    assert code(lambda: ctx.clade_placement(malformed, el[:1])) == _lib.QS_ERR_ARG
    assert code(lambda: ctx.clade_placement(ref, [el[0], ref.n_nodes])) == _lib.QS_ERR_ARG          # a node index >= n_nodes
    assert code(lambda: ctx.clade_placement(ref, [el[0], S.root])) == _lib.QS_ERR_ARG               # the root
    assert code(lambda: ctx.clade_placement(ref, [el[0], el[1], el[0]])) == _lib.QS_ERR_ARG         # repeated
    few = [v for v in range(S.N) if v != S.root and n - (S.hi[v] - S.lo[v]) < 3]
    assert few
    assert code(lambda: ctx.clade_placement(ref, [el[0], few[0]])) == _lib.QS_ERR_ARG               # fewer than three taxa outside
    assert code(lambda: ctx.clade_placement(ref, [])) == _lib.QS_ERR_ARG                            # an empty list
    ids = np.array([el[0], ref.n_nodes], dtype=np.uint32)
    out = torch.zeros(2 * 2 * ref.n_nodes + 1, dtype=torch.int64, device="cuda")
    s, keep = ctx._ref_struct(ref)
    call = lambda lst, k, dst: ctx.L.qs_clade_placement(ctx.h, C.byref(s), None if lst is None else lst.ctypes.data_as(C.c_void_p), k, dst)
    assert call(ids, 2, C.c_void_p(out.data_ptr())) == _lib.QS_ERR_ARG                              # the library's own check
    assert call(ids, 1, C.c_void_p(out.data_ptr() + 4)) == _lib.QS_ERR_ARG                          # misaligned
    assert call(ids, 1, None) == _lib.QS_ERR_ARG
    assert call(None, 1, C.c_void_p(out.data_ptr())) == _lib.QS_ERR_ARG                             # NULL list
    assert call(ids, 0, C.c_void_p(out.data_ptr())) == _lib.QS_ERR_ARG                              # n_list = 0
    assert call(ids, 1, C.c_void_p(out.data_ptr())) == _lib.QS_OK
    shard = eng.Context(n, 32, d_lo=4, d_hi=8)
    shard.table_alloc()
    assert code(lambda: shard.clade_placement(ref)) == _lib.QS_ERR_UNSUPPORTED                      # a table shard
    # 2 x C(2998,3) x (2^32 - 1) does not fit 63 bits (only a shard of such a table can exist: the bound is looked at first)
    big_ref = reference(3000, "binary", 16)
    cherry = next(v for v in eng.eligible_clades(big_ref) if np.count_nonzero(big_ref.parent == v) == 2 and
                  all(np.count_nonzero(big_ref.parent == w) == 0 for w in np.nonzero(big_ref.parent == v)[0]))
    big = eng.Context(3000, 32, d_lo=4, d_hi=6)
    big.table_alloc()
    assert code(lambda: big.clade_placement(big_ref, [cherry])) == _lib.QS_ERR_OVERFLOW
    big.set_tuning(_lib.QS_TUNE_TABLE_TREES, 1000)
    assert code(lambda: big.clade_placement(big_ref, [cherry])) == _lib.QS_ERR_UNSUPPORTED
    assert (ctx.clade_placement(ref) == want).all()            # and the context still works after the refusals
