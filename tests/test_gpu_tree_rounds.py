"""tree_agree_kernel, tree_branch_kernel and tree_pair_kernel on trees that take the paths of their shared LDS plan which ordinary
trees never take: blocks of several rounds, a node with more links than the round's budget (no bitmaps: every interval count is
taken from the tree's leaf list) between, before and after stored rounds, two such nodes in a row, and the smaller budgets from 992
taxa on. The shapes come from tests/agree_rounds.py; tests/test_agree_rounds.py asserts (without a GPU) that each holds the rounds
it is named for, and every test here asserts it again on the batch it uploads.

All comparisons are exact integers. The references are the numpy models (agreement_model, tree_branch_model, tree_pairs_model:
prefix sums over ids or positions, no rounds, no bitmaps, no leaf-list walk): EVERY row a test computes is compared with them. The
second reference is the count table, through kernels that share nothing with these three (qs_taxon_support,
qs_branch_taxon_support).

The models cost seconds per tree (an ordinary binary tree of 340 taxa four times a hub tree), and this file should not take longer
than the three files of the kernels it tests. What was cut for that, in the order the cuts are meant to be made: first the ordinary
trees of mixed_trees beside the shapes, all of them (what stands beside the shapes instead is "partial", a fan tree that lacks 30 %
of the taxa and is cheap in every model), then whole kinds of reference: tree_agreement runs with multifurcating references only;
tree_branch_support with a multifurcating one at 340 and 550 taxa (frame 1), a rooted binary one at 1100 (frame 0 with the swapped
pieces, the duplicated node under the root) and a binary one at 2259. Another rooting of the trees is run where a shape is named for
it and for the two kernels' batches of 340 taxa. No named shape is left out anywhere. With all that the file still takes about twice
its yardstick (profiles/README.md has both figures): what is left is the named shapes under one reference each.
"""
import contextlib
import functools

import numpy as np
import pytest

import agree_rounds as AR
import agreement_model as M
import branch_taxon_model as BM
import tree_branch_model as TB
import tree_pairs_model as P
from quartetscores_amd import flatten, synth

pytestmark = pytest.mark.gpu

REF_KINDS = {"binary": {}, "multifurcating": {"collapse": 0.2}, "rooted": {"rooted": True}}
# the kinds of reference each kernel is run with at 340 taxa. A multifurcating reference holds nodes of 3 to 7 links, so the unrolled
# binary pair and the general loops of tree_agree_kernel both run
AGREE_KINDS = ["multifurcating"]
BRANCH_KINDS = ["multifurcating"]
HUBS = ["hub257_mid", "hub256", "hub_first", "hub_last", "hub_dropout"]


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    from quartetscores_amd import engine
    return engine


def reference(n, seed, **kw):
    """a reference of synth.random_tree(n, ., **kw) whose taxon t<i> has the id i, so that one flattened batch serves every reference
    and the pair kernel"""
    ref = flatten.flatten_reference(AR.relabel_in_order(synth.random_tree(n, np.random.default_rng(seed), **kw)))
    assert ref.names == AR.names_of(n)
    return ref


def ref_max_links(ref):
    return max(len(bnd) - 1 + bool(par) for bnd, par in M.ref_links(ref))


@functools.lru_cache(maxsize=None)
def reference_340(kind):
    ref = reference(340, 3400 + sorted(REF_KINDS).index(kind), **REF_KINDS[kind])
    # a pair costs O(min(k,l) k l) interval counts, and on the unstored side every count walks a leaf list
    assert ref_max_links(ref) <= 8
    assert (ref_max_links(ref) > 3) == (kind == "multifurcating") and (len(ref.root.children) == 2) == (kind == "rooted")
    return ref


class Batch:
    """named shapes interleaved with other trees, flattened with both rootings"""

    def __init__(self, n, shapes, ordinary):
        self.n, self.ids = n, {nm: i for i, nm in enumerate(AR.names_of(n))}
        shapes, ordinary = list(shapes.items()), list(ordinary.items())
        self.labels, self.trees = [], []
        for k in range(max(len(shapes), len(ordinary))):
            for label, tree in shapes[k:k + 1] + ordinary[k:k + 1]:
                self.labels.append(label)
                self.trees.append(tree)
        self.flat = flatten.flatten_eval_trees(self.trees, self.ids)
        self.flat_as_written = flatten.flatten_eval_trees(self.trees, self.ids, recentre=False)
        self.links = AR.max_links(self.flat)

    def index(self, label):
        return self.labels.index(label)

    def kinds(self, label, as_written=False):
        """the rounds of the tree's blocks, e.g. ["S", "SUS"]"""
        blocks = AR.rounds(self.flat_as_written if as_written else self.flat, self.n)[self.index(label)]
        return [AR.kinds(x) for x in blocks]

    def taxa(self, label):
        i = self.index(label)
        return set(self.flat.leaf_ids[self.flat.leaf_off[i]:self.flat.leaf_off[i + 1]].tolist())


def on_device(ctx, flat, call):
    hb = ctx.batch_upload(flat)
    try:
        return call(hb)
    finally:
        ctx.batch_free(hb)


def check_rows(batch, got, model):
    """every row equals model(tree)"""
    assert len(got) == len(batch.trees)
    for i, label in enumerate(batch.labels):
        want = np.asarray(model(batch.trees[i])).astype(np.int64)
        assert (np.asarray(got[i]).astype(np.int64) == want).all(), (label, np.asarray(got[i]).tolist(), want.tolist())


def pair(ctx, hb, batch, row, col):
    """the five words of (row tree, column tree), by their labels: a rectangle of one pair"""
    r, c = batch.index(row), batch.index(col)
    assert min(batch.links[r], batch.links[c]) <= 64   # two nodes of hundreds of links meeting are 1e7 counts in one lane
    got = ctx.tree_pair_agreement(hb, rows=(r, r + 1), cols=(c, c + 1)).astype(np.int64)
    assert got.shape == (1, 1, 5)
    return tuple(got[0, 0].tolist())


def model_pair(batch, row, col):
    return P.model_pair(batch.n, batch.ids, batch.trees[batch.index(row)], batch.trees[batch.index(col)])


# ---- 340 taxa: plan (11, 256, 64) -----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def batch_340():
    n = 340
    rng = np.random.default_rng(n)
    kept = [nm for nm in AR.names_of(n) if rng.random() >= 0.3]
    b = Batch(n, AR.SHAPES_340(AR.names_of(n)), {"partial": AR.fan_tree(kept, 7, rng)})
    assert AR.plan(n) == (11, 256, 64) and b.labels[:3] == ["hub257_mid", "partial", "hub256"] and len(b.trees) == 8
    for w in (False, True):
        assert b.kinds("hub257_mid", w) == ["S", "SUS"] and b.kinds("hub256", w) == ["S", "SSS"]
        assert b.kinds("hub_first", w)[0].startswith("US") and b.kinds("hub_last", w)[-1].endswith("SU")
        assert b.kinds("hub_dropout", w) == ["SUS"]
        assert "SS" in b.kinds("fans7", w) and "SS" in b.kinds("fans5", w)
    assert [b.links[b.index(s)] for s in HUBS] == [257, 256, 257, 257, 259]
    assert max(b.links[b.index(s)] for s in b.labels if s not in HUBS) <= 64
    return b


@pytest.fixture(scope="module")
def counted_340(eng, batch_340):
    """a context of 340 taxa whose table (16-bit cells) holds the trees of the batch"""
    ctx = eng.Context(340, 16)
    ctx.table_alloc()
    ctx.count_trees(batch_340.flat)
    yield ctx
    ctx.close()


@pytest.mark.parametrize("kind", AGREE_KINDS)
def test_tree_agreement_340(eng, batch_340, counted_340, kind):
    b, ctx = batch_340, counted_340
    ref = reference_340(kind)
    got = on_device(ctx, b.flat, lambda hb: ctx.tree_agreement(ref, hb))
    check_rows(b, got, lambda t: M.model_tree(ref, t))
    assert (on_device(ctx, b.flat_as_written, lambda hb: ctx.tree_agreement(ref, hb)) == got).all()
    # the count table of the same trees (test_identities_against_the_per_tree_agreement)
    a = got.astype(np.int64)
    sup = ctx.taxon_support(ref)
    assert int(sup[:, 1].sum()) == 4 * int(a[:, 0].sum()) > 0
    assert int(sup[:, 2].sum()) == 4 * int(a[:, 1].sum()) > 0
    assert int(sup[:, 3].sum()) == 4 * int((a[:, 2] - a[:, 0] - a[:, 1]).sum())
    assert ctx.trees_counted == len(b.trees)


@pytest.mark.parametrize("kind", BRANCH_KINDS)
def test_tree_branch_support_340(eng, batch_340, counted_340, kind):
    b, ctx = batch_340, counted_340
    ref = reference_340(kind)
    assert BM.is_bifurcating(ref) == (kind != "multifurcating")   # frame 0 with the swapped pieces, or frame 1
    the_items = TB.items(ref)
    got = on_device(ctx, b.flat, lambda hb: ctx.tree_branch_support(ref, hb))
    assert got.shape == (len(b.trees), ref.n_nodes, 4)
    check_rows(b, got, lambda t: TB.model_tree(ref, t, the_items=the_items))
    assert (on_device(ctx, b.flat_as_written, lambda hb: ctx.tree_branch_support(ref, hb)) == got).all()
    # the count table of the same trees (test_sums_agree_with_count_table of tests/test_gpu_tree_branch.py)
    _, totals = ctx.branch_taxon_support(ref, taxa=[0])
    assert totals[:, 1:].any() and (got.sum(0)[:, 1:4] == totals[:, 1:4]).all()


@pytest.mark.parametrize("hub", HUBS)
def test_tree_pairs_340_hub(eng, batch_340, counted_340, hub):
    """the hub tree as column: the unstored list_count path; as row: the general pair_terms with the long side inside. Its partner is
    fans7; hub_dropout also meets the partial tree, which lacks other taxa than it does, so that positions the row tree lacks occur
    inside the unstored links, and it is run from both rootings (the words do not depend on them)."""
    b, ctx = batch_340, counted_340
    want = model_pair(b, "fans7", hub), model_pair(b, hub, "fans7")
    for flat in (b.flat, b.flat_as_written) if hub == "hub_dropout" else (b.flat,):
        assert on_device(ctx, flat, lambda hb: (pair(ctx, hb, b, "fans7", hub), pair(ctx, hb, b, hub, "fans7"))) == want
    if hub == "hub_dropout":
        other = "partial"
        assert len(b.taxa(hub) - b.taxa(other)) > 50 and len(b.taxa(other) - b.taxa(hub)) > 10
        want = model_pair(b, other, hub)
        assert want[4] == len(b.taxa(hub) & b.taxa(other)) and want[1] > 0
        want = want, tuple(P.swapped(want))   # the same quartets, the trees exchanged
        for flat in (b.flat, b.flat_as_written):
            assert on_device(ctx, flat, lambda hb: (pair(ctx, hb, b, other, hub), pair(ctx, hb, b, hub, other))) == want


def test_tree_pairs_340_fans(eng, batch_340, counted_340):
    """column trees whose blocks take several stored rounds, and the same trees as rows"""
    b, ctx = batch_340, counted_340
    want = model_pair(b, "fans7", "fans5"), model_pair(b, "fans5", "fans7")
    for flat in (b.flat, b.flat_as_written):
        assert on_device(ctx, flat, lambda hb: (pair(ctx, hb, b, "fans7", "fans5"), pair(ctx, hb, b, "fans5", "fans7"))) == want


# ---- 550 taxa: two unstored nodes in a row --------------------------------------------------------------------------------------

def test_two_hubs(eng):
    """tree_branch_support and tree_pair_agreement (tree_agreement is left to the other shapes: its model costs most)"""
    n = 550
    b = Batch(n, {"two_hubs": AR.two_hubs(AR.names_of(n)), "fans7": AR.fan_tree(AR.names_of(n), 7, np.random.default_rng(5507))}, {})
    assert AR.plan(n) == (18, 256, 64)
    assert b.kinds("two_hubs") == ["SUUS"] and b.kinds("two_hubs", True) == ["SUUS"] and b.links == [257, 7]
    ref = reference(n, 5500, collapse=0.2)
    assert 3 < ref_max_links(ref) <= 8
    with contextlib.closing(eng.Context(n)) as ctx:
        got = on_device(ctx, b.flat, lambda hb: ctx.tree_branch_support(ref, hb))
        assert (got[0] == TB.model_tree(ref, b.trees[0])).all() and got[0, :, 1:].any()
        as_col, as_row = on_device(ctx, b.flat, lambda hb: (pair(ctx, hb, b, "fans7", "two_hubs"), pair(ctx, hb, b, "two_hubs", "fans7")))
        assert as_col == model_pair(b, "fans7", "two_hubs") and as_row == model_pair(b, "two_hubs", "fans7")


# ---- 1100 and 2259 taxa: plans (35, 232, 58) and (71, 112, 28) ------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def sparse(n):
    """hub, small, fans7: the sparse shapes of n taxa and between them one small tree of synth.random_tree (rooted, 40 % of the edges
    collapsed, 30 % of its 60 taxa dropped; the models' cost grows with the size of the tree)"""
    W, cap, nb = AR.plan(n)
    assert (W, cap, nb) == {1100: (35, 232, 58), 2259: (71, 112, 28)}[n]
    names, rng = AR.names_of(n), np.random.default_rng(n)
    small = synth.random_tree(60, rng, names=AR.spread_names(names, 60, rng), rooted=True, collapse=0.4, dropout=0.3)
    b = Batch(n, AR.sparse_shapes(names), {"small": small})
    assert b.labels == ["hub", "small", "fans7"]
    for w in (False, True):
        assert b.kinds("hub", w)[:2] == ["S", "SUS"] and "U" not in "".join(b.kinds("hub", w)[2:])
        assert sum("SS" in k for k in b.kinds("fans7", w)) >= 1 and "U" not in "".join(b.kinds("fans7", w))
    assert b.links[0] == cap + 1 and max(b.links[1:]) <= 64
    for label in ("hub", "fans7"):   # every word of the bitmaps is in use
        assert len({x >> 5 for x in b.taxa(label)}) == W
    return b


@pytest.mark.parametrize("n", [1100, 2259])
def test_large_plan_branch_support(eng, n):
    b = sparse(n)
    ref = reference(n, n + 10, rooted=(n == 1100))   # frame 0 with the swapped pieces; at 1100 taxa the duplicated node under the root
    assert BM.is_bifurcating(ref) and (len(ref.root.children) == 2) == (n == 1100)
    the_items = TB.items(ref)
    with contextlib.closing(eng.Context(n)) as ctx:
        got = on_device(ctx, b.flat, lambda hb: ctx.tree_branch_support(ref, hb))
        check_rows(b, got, lambda t: TB.model_tree(ref, t, the_items=the_items))
        assert got[b.index("hub"), :, 1:].any()


def test_large_plan_agreement(eng):
    """at 1100 taxa only: the model of one 320-taxon tree against a reference of 2259 taxa takes most of a minute"""
    n = 1100
    b = sparse(n)
    ref = reference(n, n + 20, collapse=0.6)   # fewer reference nodes: the model's cost; its degrees stay far below the hub's
    assert 8 < ref_max_links(ref) <= 64
    with contextlib.closing(eng.Context(n)) as ctx:
        got = on_device(ctx, b.flat, lambda hb: ctx.tree_agreement(ref, hb))
        check_rows(b, got, lambda t: M.model_tree(ref, t))


@pytest.mark.parametrize("n", [1100, 2259])
def test_large_plan_pairs(eng, n):
    """the hub tree as column and as row of fans7, fans7 as column of the small tree, the hub tree as column of the small tree (most of
    whose taxa it lacks)"""
    b = sparse(n)
    pairs = [("fans7", "hub"), ("hub", "fans7"), ("small", "fans7"), ("small", "hub")]
    with contextlib.closing(eng.Context(n)) as ctx:
        got = on_device(ctx, b.flat, lambda hb: [pair(ctx, hb, b, r, c) for r, c in pairs])
    for (r, c), words in zip(pairs, got):
        assert words == model_pair(b, r, c), (r, c)
    assert 4 <= got[3][4] < len(b.taxa("small"))
