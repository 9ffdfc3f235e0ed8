"""Per-tree quartet agreement of every taxon without a GPU: the node-pair sums and difference arrays of tests/tree_taxon_model.py (the
model of qs_tree_taxa.hip) against a per-4-set brute force, the two forms of the pair sums against each other, the worked example,
the derived columns and the plan."""
import math

import numpy as np

import agreement_model as AM
import tree_taxon_model as M
from quartetscores_amd import engine, flatten, synth


def c3(x):
    return x * (x - 1) * (x - 2) // 6


def random_pairs(count, seed):
    """(reference, tree) of 5 to 12 taxa: binary and multifurcating on both sides, rooted and unrooted references, 0 to 50 % dropped"""
    rng = np.random.default_rng(seed)
    for i in range(count):
        n = int(rng.integers(5, 13))
        ref_kw = [{}, {"rooted": True}, {"collapse": 0.3}, {"rooted": True, "collapse": 0.5}, {"collapse": 1.0}][i % 5]
        ev_kw = [{}, {"collapse": float(rng.uniform(0.1, 0.8))}, {"dropout": float(rng.uniform(0.05, 0.5))}, {"rooted": True},
                 {"rooted": True, "collapse": 0.3, "dropout": 0.3}, {"collapse": 1.0}, {"dropout": 0.5, "min_taxa": 3}][i % 7]
        yield n, synth.random_tree(n, rng, **ref_kw), synth.random_tree(n, rng, **ev_kw)


def test_model_matches_brute_force():
    multi = dropped = small = 0
    for n, ref_nw, ev_nw in random_pairs(140, 23):
        ref = flatten.flatten_reference(ref_nw)
        want = M.brute_words(ref_nw, ref.names, ev_nw)
        got = M.model_tree(ref, ev_nw)
        assert (got == want).all(), (ref_nw, ev_nw)
        assert (M.model_tree(ref, ev_nw, recentre=False) == want).all()
        assert (M.model_tree(ref, ev_nw, w_of_pairs=M.pair_w_definition) == want).all()
        # every 4-set has four members
        assert (want.sum(0) == 4 * np.array(AM.brute_counts(ref_nw, ref.names, ev_nw))).all()
        L = ev_nw.count(",") + 1
        multi += L >= 4 and int(want[:, 2].sum()) < 4 * math.comb(L, 4)
        dropped += 4 <= L < n
        small += L < 4
        if L < 4:
            assert not want.any()
    assert multi and dropped and small


def test_pair_sums_both_forms():
    rng = np.random.default_rng(5)
    for k, K in ((3, 3), (3, 5), (6, 4), (7, 7), (1, 3), (3, 2)):
        I = rng.integers(0, 5, size=(9, k, K)) * (rng.random((9, k, K)) < 0.7)
        a, b = M.pair_w(I), M.pair_w_definition(I)
        assert (a[0] == b[0]).all() and (a[1] == b[1]).all()
        if min(k, K) < 3:
            assert not a[0].any() and not a[1].any()


def test_special_shapes():
    names = [f"t{i}" for i in range(11)]
    rng = np.random.default_rng(2)
    ref_nw = synth.random_tree(11, rng)
    ref = flatten.flatten_reference(ref_nw)
    # identical: nothing discordant, everything concordant
    same = M.model_tree(ref, ref_nw)
    assert (same == M.brute_words(ref_nw, ref.names, ref_nw)).all()
    assert not same[:, 1].any() and (same[:, 0] == c3(10)).all() and (same[:, 2:] == c3(10)).all()
    # a star resolves nothing; resolved_ref is the reference's own
    st = M.model_tree(ref, M.star(names))
    assert (st == M.brute_words(ref_nw, ref.names, M.star(names))).all()
    assert not st[:, :3].any() and (st[:, 3] == c3(10)).all()
    assert (st[:, 3] == M.star_resolved_ref(ref, range(11))).all()
    # ladders on both sides, in different orders
    lad_ref = M.ladder(names)
    ref2 = flatten.flatten_reference(lad_ref)
    lad = M.ladder([names[i] for i in rng.permutation(11)])
    assert (M.model_tree(ref2, lad) == M.brute_words(lad_ref, ref2.names, lad)).all()
    # a multifurcating tree identical to a multifurcating reference
    mref_nw = synth.random_tree(11, rng, collapse=0.4)
    mref = flatten.flatten_reference(mref_nw)
    got = M.model_tree(mref, mref_nw)
    assert (got == M.brute_words(mref_nw, mref.names, mref_nw)).all()
    assert not got[:, 1].any() and (got[:, 0] == got[:, 2]).all() and (got[:, 0] == got[:, 3]).all() and (got[:, 0] < c3(10)).any()


def test_worked_example():
    ref_nw, ev_nw = "(((((A,B),C),D),E),F);", "((((B,C),D),E),(A,F));"
    ref = flatten.flatten_reference(ref_nw)
    got = M.model_tree(ref, ev_nw)
    assert (got == M.brute_words(ref_nw, ref.names, ev_nw)).all()
    by_name = {nm: got[i].tolist() for i, nm in enumerate(ref.names)}
    assert by_name["A"] == [0, 10, 10, 10]
    for nm in "BCDEF":
        assert by_name[nm] == [4, 6, 10, 10]
    b = flatten.flatten_eval_trees([ev_nw], ref.name_to_id)
    cols = engine.tree_taxon_columns(ref.names, got[None], b)
    assert list(cols) == list(engine.TREE_TAXA_COLUMNS) and cols["name"] == ref.names
    assert (cols["quartets"] == 10).all() and not cols["eval_only"].any() and not cols["unresolved"].any()
    assert np.allclose(cols["tree_concordance"], 1 / 3)
    a = ref.names.index("A")
    for i in range(6):
        assert math.isclose(cols["gain"][i], 2 / 3 if i == a else -2 / 15)
        assert math.isclose(cols["concordance_without"][i], 1.0 if i == a else 0.2)
        assert math.isclose(cols["concordance"][i], 0.0 if i == a else 0.4)
    # the filters
    only = engine.tree_taxon_columns(ref.names, got[None], b, only=[a, 2])
    assert only["taxon"].tolist() == sorted([a, 2])
    rogue = engine.tree_taxon_columns(ref.names, got[None], b, first_tree=7, min_gain=0.5)
    assert rogue["taxon"].tolist() == [a] and rogue["tree"].tolist() == [7]


def test_columns_of_partial_and_small_trees():
    rng = np.random.default_rng(8)
    ref_nw = synth.random_tree(9, rng)
    ref = flatten.flatten_reference(ref_nw)
    partial = synth.random_tree(9, rng, dropout=0.4)
    while not 5 <= partial.count(",") + 1 < 9:    # (binary, five taxa or more: no ratio of it is nan)
        partial = synth.random_tree(9, rng, dropout=0.4)
    trees = ["(t0,t1,t2);", partial, M.star([f"t{i}" for i in range(9)])]
    b = flatten.flatten_eval_trees(trees, ref.name_to_id)
    w = M.model_trees(ref, trees)
    cols = engine.tree_taxon_columns(ref.names, w, b)
    L1 = int(b.leaf_off[2] - b.leaf_off[1])
    assert 5 <= L1 < 9 and cols["tree"].tolist() == [1] * L1 + [2] * 9        # the 3-taxon tree writes no line
    assert (cols["quartets"][:L1] == c3(L1 - 1)).all() and (cols["quartets"][L1:] == c3(8)).all()
    assert sorted(cols["taxon"][:L1].tolist()) == sorted(int(x) for x in b.leaf_ids[3:3 + L1])
    assert np.isnan(cols["gain"][L1:]).all() and np.isnan(cols["tree_concordance"][L1:]).all()    # the star resolves nothing
    assert (cols["ref_only"][L1:] == c3(8)).all()
    assert len(engine.tree_taxon_columns(ref.names, w, b, min_gain=-1.0)["tree"]) == L1           # nan gains are dropped


def test_plan():
    assert M.max_taxa() >= 1100
    W, cap, nb, lds = M.plan(1100)
    assert W == 35 and cap >= M.MIN_CAP and nb == 64 and lds <= M.LDS_BYTES
    assert M.plan(512)[1] == 192 and 3 * M.plan(512)[3] <= 160 * 1024          # three workgroups in a CU's LDS
    assert M.plan(M.max_taxa()) is not None and M.plan(M.max_taxa() + 1) is None
    for n in (4, 8, 131, 512, 1100, M.max_taxa()):
        W, cap, nb, lds = M.plan(n)
        assert lds == M.FLIGHT * 2 * (n + 1) * 8 + (1 + cap) * W * 8 <= M.LDS_BYTES and cap <= M.MAX_CAP


def test_plan_shapes_reach_their_rounds():
    """the trees tests/test_gpu_tree_taxa.py runs for the plan: a block of several stored rounds, and a node above the link cap"""
    n = 1100
    _, cap, nb, _ = M.plan(n)
    names = M.names_of(n)
    ref = flatten.flatten_reference(synth.random_tree(n, np.random.default_rng(1)))
    shapes = M.plan_shapes(names)
    b = flatten.flatten_eval_trees(list(shapes.values()), ref.name_to_id)
    r = dict(zip(shapes, M.rounds(b, n)))
    assert all(len(blk) >= 2 and set(x[0] for x in blk) == {"S"} for blk in r["fans7"])
    assert any(("U",) in blk for blk in r["hub"]) and max(int(x) for x in np.diff(b.rng_off)) == cap + 2

