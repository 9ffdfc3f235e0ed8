"""tests/species_model.py (the specification of qs_table_collapse) against the definition of the multi-individual quartet
count, and flatten.parse_species_map / flatten.species_layout (no GPU)."""
import itertools

import numpy as np
import pytest

import bruteforce
from species_model import collapse_table, individuals_of, with_clades
from quartetscores_amd import flatten, synth


def mixed_trees(n, seed):
    return (synth.tree_set(n, 5, seed, dropout=0.25) + synth.tree_set(n, 5, seed + 1, collapse=0.3) +
            synth.tree_set(n, 3, seed + 2, rooted=True) + synth.tree_set(n, 3, seed + 3))


@pytest.mark.parametrize("sizes", [(2, 2, 2, 3, 1), (1, 3, 1, 2, 2, 2), (4, 1, 1, 3, 1, 2), (1, 1, 2, 2, 3, 3)])
def test_collapse_equals_the_sum_over_one_individual_per_species(sizes):
    n = sum(sizes)
    assert 10 <= n <= 12 and 5 <= len(sizes) <= 6
    first = np.concatenate([[0], np.cumsum(sizes)])
    names = [f"t{i}" for i in range(n)]
    trees = mixed_trees(n, 100 * n + len(sizes))
    got = collapse_table(bruteforce.count_table(names, trees), n, first)
    assert got.shape == (len(list(itertools.combinations(range(len(sizes)), 4))), 3)
    groups = [range(first[i], first[i + 1]) for i in range(len(sizes))]
    for r, species in enumerate(bruteforce.rank_order_quads(len(sizes))):
        choices = list(itertools.product(*(groups[s] for s in species)))      # one individual per species, ids ascending
        want = bruteforce.quartet_counts_for(trees, names, choices).sum(axis=0)
        assert (got[r] == want).all(), (sizes, species)
    assert got.sum() > 0


def test_singleton_groups_give_the_input():
    n = 10
    table = bruteforce.count_table([f"t{i}" for i in range(n)], mixed_trees(n, 7))
    assert (collapse_table(table, n, np.arange(n + 1)) == table).all()


@pytest.mark.parametrize("k,n_species", [(2, 6), (3, 4), (1, 7)])
def test_species_that_are_clades_count_k_to_the_fourth(k, n_species):
    species = [f"t{i}" for i in range(n_species)]
    rng = np.random.default_rng(10 * k + n_species)
    species_trees = (synth.tree_set(n_species, 4, 31 + k) + synth.tree_set(n_species, 4, 32 + k, collapse=0.4) +
                     synth.tree_set(n_species, 4, 33 + k, dropout=0.2))
    gene_trees = [with_clades(nw, k, rng) for nw in species_trees]
    individuals = [x for s in species for x in individuals_of(s, k)]
    got = collapse_table(bruteforce.count_table(individuals, gene_trees), len(individuals), np.arange(n_species + 1) * k)
    want = bruteforce.count_table(species, species_trees) * np.uint64(k ** 4)
    assert (got == want).all() and want.sum() > 0


# ---- the species map ----------------------------------------------------------------------------------------------------

REF = "((A,B),(C,(D,E)),F);"


def test_parse_species_map():
    text = "# individuals\n\n  A : a1 , a2,a3 \nC:c1\n   \n#E:e\nE:E,e2\n"
    assert flatten.parse_species_map(text) == {"A": ["a1", "a2", "a3"], "C": ["c1"], "E": ["E", "e2"]}
    assert list(flatten.parse_species_map(text)) == ["A", "C", "E"]
    assert flatten.parse_species_map("") == {}


def test_species_layout_orders_species_by_lookup_id_and_individuals_by_the_map():
    ref = flatten.flatten_reference(REF)
    lay = flatten.species_layout(ref, flatten.parse_species_map("E:e2,E,e1\nA:a2,a1\nC:c1\n"))
    assert ref.names == ["A", "B", "C", "D", "E", "F"]
    assert lay.names == ["a2", "a1", "B", "c1", "D", "e2", "E", "e1", "F"]
    assert lay.name_to_id == {nm: i for i, nm in enumerate(lay.names)}
    assert lay.first_id.dtype == np.uint16 and lay.first_id.tolist() == [0, 2, 3, 4, 5, 8, 9]
    plain = flatten.species_layout(ref, {})
    assert plain.names == ref.names and plain.first_id.tolist() == list(range(7))


@pytest.mark.parametrize("text,label", [
    ("X:x1,x2\n", "X"),                 # a species that is no leaf of the reference tree
    ("A:a1,a2,a1\n", "a1"),             # an individual listed twice under one species
    ("A:a1,a2\nC:c1,a2\n", "a2"),       # ... and under two species
    ("A:a1,B\n", "B"),                  # an individual with the name of an unlisted species
    ("A:\n", "A"),                      # an empty individual list
    ("A:a1,,a2\n", "A"),                # an empty name in the list
    ("A:a1\nA:a2\n", "A"),              # a species with two lines
    ("A a1 a2\n", "A a1 a2"),           # no colon
])
def test_species_map_errors_name_the_label(text, label):
    ref = flatten.flatten_reference(REF)
    with pytest.raises(ValueError) as ei:
        flatten.species_layout(ref, flatten.parse_species_map(text))
    assert f"'{label}'" in str(ei.value)


def test_an_empty_list_in_a_mapping_is_refused_too():
    with pytest.raises(ValueError, match="'A'.*empty"):
        flatten.species_layout(flatten.flatten_reference(REF), {"A": []})


def test_too_many_individuals_and_too_few_species():
    ref = flatten.flatten_reference(REF)
    with pytest.raises(ValueError, match="4097 individuals"):
        flatten.species_layout(ref, {"A": [f"a{i}" for i in range(4092)]})
    assert len(flatten.species_layout(ref, {"A": [f"a{i}" for i in range(4091)]}).names) == 4096
    with pytest.raises(ValueError, match="fewer than 4 species"):
        flatten.species_layout(flatten.flatten_reference("(A,B,C);"), {"A": ["a1", "a2"]})
