"""Quartet support of taxon pairs without a GPU: the numpy model of qs_taxon_pairs.hip (tests/taxon_pair_model.py) against a brute
force in plain loops, the identities of the eight words with the per-taxon sums (tests/taxon_model.py), and the columns."""
import numpy as np

import bruteforce
import taxon_model
import taxon_pair_model as M
from quartetscores_amd import flatten, synth


def random_cases(count, seed):
    rng = np.random.default_rng(seed)
    for i in range(count):
        n = int(rng.integers(5, 11))
        ref_kw = [{}, {"collapse": 0.3}, {"rooted": True}, {"collapse": 1.0}, {"rooted": True, "collapse": 0.5}, {"collapse": 0.7}][i % 6]
        ref_nw = synth.random_tree(n, rng, **ref_kw)
        trees = []
        for k in range(int(rng.integers(1, 8))):
            ev_kw = [{}, {"collapse": float(rng.uniform(0.1, 1.0))}, {"dropout": float(rng.uniform(0.1, 0.8)), "min_taxa": int(rng.integers(1, 5))},
                     {"rooted": True}, {"rooted": True, "collapse": 0.3, "dropout": 0.3}][(i + k) % 5]
            trees.append(synth.random_tree(n, rng, **ev_kw))
        yield n, ref_nw, trees


def test_model_matches_brute_force_and_the_identities():
    cases = unresolved = apart = stars = 0
    for n, ref_nw, trees in random_cases(48, 31):
        ref = flatten.flatten_reference(ref_nw)
        table = bruteforce.count_table(ref.names, trees)
        got, want = M.pair_counts(table, ref), M.brute_counts(ref_nw, ref.names, trees)
        assert got.dtype == np.int64 and got.shape == (n, n, 8) and (got == want).all(), (ref_nw, trees)
        M.check_identities(got, taxon_model.model_counts(table, ref))
        M.check_identities(got, taxon_model.brute_counts(ref_nw, ref.names, trees))
        # the two classes and the rest partition the C(n-2,2) 4-sets of a pair; t is part of s
        off = ~np.eye(n, dtype=bool)
        assert (got[off][:, 0] + got[off][:, 1] <= (n - 2) * (n - 3) // 2).all()
        assert (got[..., 2] <= got[..., 3]).all() and (got[..., 4] <= got[..., 5]).all() and (got[..., 6] <= got[..., 7]).all()
        assert (got[..., 3] + got[..., 5] <= got[..., 7]).all()
        cases += 1
        unresolved += int((got[..., 6] - got[..., 2] - got[..., 4]).sum() > 0)
        apart += int(got[..., 4].sum() > 0)
        stars += int(got[..., :2].sum() == 0 and got[..., 6].sum() > 0)
    assert cases >= 40 and unresolved and apart and stars


def test_a_list_gives_rows_of_the_matrix():
    n, ref_nw, trees = next(random_cases(1, 5))
    ref = flatten.flatten_reference(ref_nw)
    table = bruteforce.count_table(ref.names, trees)
    every = M.pair_counts(table, ref)
    assert (M.pair_counts(table, ref, [n - 1, 0, 2]) == every[[n - 1, 0, 2]]).all()


def test_columns_by_hand():
    # four taxa, one 4-set with cells (5, 2, 1); the reference shows 01|23
    names = ["a", "b", "c", "d"]
    ref = flatten.flatten_reference("((a,b),(c,d));")
    assert ref.names == names
    cols = M.columns(M.pair_counts(np.array([[5, 2, 1]]), ref), names)
    assert list(cols) == list(M.COLUMNS)
    assert cols["a"].tolist() == [0, 0, 0, 1, 1, 2] and cols["b"].tolist() == [1, 2, 3, 2, 3, 3]
    assert cols["name_a"] == ["a", "a", "a", "b", "b", "c"] and cols["name_b"] == ["b", "c", "d", "c", "d", "d"]
    assert cols["quartets"].tolist() == [1] * 6
    assert cols["ref_together"].tolist() == [1, 0, 0, 0, 0, 1] and cols["ref_apart"].tolist() == [0, 1, 1, 1, 1, 0]
    assert cols["together"].tolist() == [5, 2, 1, 1, 2, 5] and cols["apart"].tolist() == [3, 6, 7, 7, 6, 3]
    assert cols["affinity"].tolist() == [5 / 8, 2 / 8, 1 / 8, 1 / 8, 2 / 8, 5 / 8]
    assert cols["kept"][0] == 5 / 8 and np.isnan(cols["kept"][1:5]).all() and cols["kept"][5] == 5 / 8
    assert np.isnan(cols["joined"][[0, 5]]).all() and cols["joined"][1:5].tolist() == [2 / 8, 1 / 8, 1 / 8, 2 / 8]
    # a list: the pairs with a listed taxon, in the same order, from the listed rows alone
    part = M.columns(M.pair_counts(np.array([[5, 2, 1]]), ref, [2]), names, [2])
    assert part["a"].tolist() == [0, 1, 2] and part["b"].tolist() == [2, 2, 3] and part["together"].tolist() == [2, 1, 5]
    # an empty table: every ratio is nan
    zero = M.columns(np.zeros((4, 4, 8), dtype=np.int64), names)
    assert np.isnan(zero["affinity"]).all() and np.isnan(zero["kept"]).all() and np.isnan(zero["joined"]).all()
