"""The specification of qs_table_collapse in numpy, with no cleverness (it shares no code with the library, the C++ host or
tests/helpers.py): the count table of species, summed out of the table counted over their individuals.

A table is a (C(n,4), 3) array in rank order (tests/restrict_model.py). Species i owns the source ids
[first_id[i], first_id[i + 1]); the tuple of the species S0 < S1 < S2 < S3 is the sum of the source tuples a < b < c < d with
a in S0, b in S1, c in S2, d in S3 -- the groups are consecutive and in order, so the slots carry over unchanged."""
import re

import numpy as np

from restrict_model import _choose, four_sets
from quartetscores_amd import synth


def collapse_table(table, n_src, first_id):
    """(C(n_dst,4), 3) uint64: for every source rank whose four ids lie in four different groups, np.add.at into the rank of
    the four groups."""
    first = np.asarray(first_id, dtype=np.int64)
    table = np.asarray(table)
    assert table.shape == (int(_choose(n_src, 4)), 3), table.shape
    assert first[0] == 0 and first[-1] == n_src and (np.diff(first) > 0).all(), "first_id must run from 0 to n_src, strictly increasing"
    n_dst = len(first) - 1
    group = np.repeat(np.arange(n_dst), np.diff(first))              # group[a] = the species that owns source id a
    g = group[four_sets(n_src)]                                      # (C(n_src,4), 4), non-decreasing along a row
    use = (g[:, 0] < g[:, 1]) & (g[:, 1] < g[:, 2]) & (g[:, 2] < g[:, 3])
    g = g[use]
    rank = _choose(g[:, 3], 4) + _choose(g[:, 2], 3) + _choose(g[:, 1], 2) + g[:, 0]
    out = np.zeros((int(_choose(n_dst, 4)), 3), dtype=np.uint64)
    np.add.at(out, rank, table[use].astype(np.uint64))
    return out


def individuals_of(species, k):
    return [f"{species}x{j}" for j in range(k)]


def with_clades(species_newick, k, rng):
    """the species tree with every leaf replaced by a random binary subtree of its k individuals (the leaf itself for k = 1,
    under the name individuals_of gives it): a gene tree in which every species is a clade"""
    def clade(m):
        inds = individuals_of(m.group(0), k)
        return inds[0] if k == 1 else synth._to_newick(synth._join_random([inds[i] for i in rng.permutation(k)], rng, stop_at=2))
    return re.sub(r"[A-Za-z_][A-Za-z_0-9]*", clade, species_newick)
