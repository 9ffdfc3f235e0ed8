"""tests/restrict_model.py (the specification of qs_table_restrict) against the brute-force counter: the restriction of the
table of a tree set equals the table of the pruned trees (newick.prune), because what a tree displays for a 4-set does not
depend on its other taxa."""
import numpy as np
import pytest

import bruteforce
from restrict_model import four_sets, restrict_table
from quartetscores_amd import newick, synth


def pruned_trees(trees, drop):
    """the trees without the taxa in `drop`; a tree left with fewer than four taxa holds no quartet and is left out"""
    out = []
    for nw in trees:
        root = newick.prune(newick.parse_tree(nw), drop)
        if root is not None and sum(x.is_leaf for x in newick.preorder(root)) >= 4:
            out.append(newick.write(root))
    return out


def test_four_sets_are_in_rank_order():
    for n in (4, 5, 9):
        assert four_sets(n).tolist() == [list(q) for q in bruteforce.rank_order_quads(n)]


@pytest.mark.parametrize("n", [9, 10, 11, 12])
def test_restriction_of_the_brute_force_table_is_the_table_of_the_pruned_trees(n):
    names = [f"t{i}" for i in range(n)]
    trees = (synth.tree_set(n, 6, 10 * n, dropout=0.25) + synth.tree_set(n, 6, 10 * n + 1, collapse=0.3) +
             synth.tree_set(n, 6, 10 * n + 2, rooted=True) + synth.tree_set(n, 4, 10 * n + 3))
    table = bruteforce.count_table(names, trees)
    rng = np.random.default_rng(n)
    kept_sets = [np.arange(1, n), np.arange(n - 1), np.delete(np.arange(n), n // 2), np.arange(0, n, 2),
                 np.sort(rng.choice(n, size=n - 3, replace=False)), np.arange(n)]
    for kept in kept_sets:
        for ids in (kept, rng.permutation(kept)):          # in the source's order (pruning), and in any order
            drop = {names[i] for i in range(n) if i not in set(ids.tolist())}
            want = bruteforce.count_table([names[i] for i in ids], pruned_trees(trees, drop))
            got = restrict_table(table, n, ids)
            assert got.shape == want.shape and (got == want).all(), (n, ids.tolist())
    assert table.sum() > 0


def test_a_tree_pruned_below_four_taxa_contributes_nothing():
    names = [f"t{i}" for i in range(9)]
    small = "((t0,t1),(t2,t3),t8);"                          # two of its taxa are kept
    trees = synth.tree_set(9, 5, 3) + [small]
    kept = np.array([0, 1, 4, 5, 6, 7])
    drop = {"t2", "t3", "t8"}
    assert len(pruned_trees(trees, drop)) == 5
    got = restrict_table(bruteforce.count_table(names, trees), 9, kept)
    assert (got == bruteforce.count_table([names[i] for i in kept], pruned_trees(trees, drop))).all()
    assert (got == restrict_table(bruteforce.count_table(names, trees[:5]), 9, kept)).all()
