"""tree_pairs_model (the numpy model of qs_tree_pair_agreement) against the per-quartet brute force, against itself with the two trees
exchanged, and against agreement_model where the row tree holds every taxon. No GPU."""
import numpy as np
import pytest

import agreement_model as M
import tree_pairs_model as P
from quartetscores_amd import flatten
from test_gpu_tree_agreement import mixed_trees


def names_of(n):
    return [f"t{i}" for i in range(n)]


@pytest.mark.parametrize("n", [5, 9, 17])
def test_model_matches_brute_force_and_swap(n):
    rng = np.random.default_rng(100 + n)
    names = names_of(n)
    ids = {nm: i for i, nm in enumerate(names)}
    trees = mixed_trees(n, rng, 12)
    flats = [P.flat(t, ids) for t in trees]
    got = np.array([[P.model_counts(n, fs, ft) for ft in flats] for fs in flats], dtype=np.int64)
    want = np.array([[P.brute_pair(names, s, t) for t in trees] for s in trees], dtype=np.int64)
    assert (got == want).all(), (n, np.argwhere((got != want).any(2)))
    assert (got == P.swapped(got.transpose(1, 0, 2))).all()
    # the diagonal: a tree agrees with itself on everything it resolves
    d = got[np.arange(12), np.arange(12)]
    assert (d[:, 1] == 0).all() and (d[:, 0] == d[:, 2]).all() and (d[:, 0] == d[:, 3]).all()


@pytest.mark.parametrize("n", [17, 40])
def test_complete_row_tree_equals_agreement_model(n):
    rng = np.random.default_rng(200 + n)
    names = names_of(n)
    ids = {nm: i for i, nm in enumerate(names)}
    trees = mixed_trees(n, rng, 12)
    rows = [s for s in trees if len(P.taxa_of(s, ids)) == n]
    assert len(rows) >= 3
    for s in rows[:4]:
        ref = flatten.flatten_reference(s)
        for t in trees:
            a = M.model_tree(ref, t)
            assert P.model_pair(n, ref.name_to_id, s, t)[:4] == (a[0], a[1], a[3], a[2])


def test_rooting_does_not_matter():
    rng = np.random.default_rng(7)
    n = 17
    ids = {nm: i for i, nm in enumerate(names_of(n))}
    trees = mixed_trees(n, rng, 6)
    for s in trees:
        for t in trees:
            assert P.model_pair(n, ids, s, t, recentre=True) == P.model_pair(n, ids, s, t, recentre=False)
