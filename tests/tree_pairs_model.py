"""Quartet agreement of two evaluation trees (qs_tree_pair_agreement): a numpy model of the node-pair formulas in the row tree's
position space, and a per-quartet brute force over the shared taxa.

For row tree s (taxa P_s) and column tree t (taxa P_t), S = P_s & P_t, N = |S|, both trees restricted to S, the five words are
(concordant, discordant, resolved_row, resolved_col, N). The model does what the kernel does: pos_s maps a taxon to its
position in s's leaf tour; the leaves of t (and of every link of t) that have a position in s become prefix counts over s-positions;
a link of s is a circular arc [st, en) of positions, and its count in such a set is cnt(en) - cnt(st), plus the set's total when the
arc wraps (an end stored as 0 is L_s and wraps the same way). The node-pair terms are agreement_model.pair_terms /
resolved_of_node, unchanged. The brute force applies agreement_model._topologies to both trees with taxa = the intersection
(agreement_model.brute_counts assumes that the reference holds every taxon) and shares no code with the model.
"""
import numpy as np

import agreement_model as M
import bruteforce
from quartetscores_amd import flatten, newick

NO_POS = -1


def flat(tree_newick, name_to_id, recentre=True):
    """(leaf_ids, node_ranges) of one tree, as flatten.flatten_eval_trees puts them into a batch."""
    leaf_ids, _, node_ranges = flatten.flatten_tree(newick.parse_tree(tree_newick), name_to_id, recentre)
    return leaf_ids, node_ranges


def position_map(n_taxa, leaf_ids):
    pos = np.full(n_taxa, NO_POS, dtype=np.int64)
    pos[np.asarray(leaf_ids, dtype=np.int64)] = np.arange(len(leaf_ids))
    return pos


def prefix_counts(pos, Ls, taxa):
    """pre[x] = how many of `taxa` sit at s-positions < x, x = 0 .. Ls (pre[Ls] = how many of them s holds at all)."""
    m = np.zeros(Ls + 1, dtype=np.int64)
    q = pos[np.asarray(taxa, dtype=np.int64)]
    m[q[q != NO_POS]] = 1
    return np.concatenate([[0], np.cumsum(m)])[: Ls + 1]


def arc_count(pre, st, en):
    d = int(pre[en] - pre[st])
    return d if st <= en else int(pre[-1]) + d


def model_counts(n_taxa, s_flat, t_flat):
    """The five words from two flattened trees (flat)."""
    ids_s, nodes_s = s_flat
    ids_t, nodes_t = t_flat
    Ls, Lt = len(ids_s), len(ids_t)
    pos = position_map(n_taxa, ids_s)
    pres = prefix_counts(pos, Ls, ids_t)
    N = int(pres[-1])
    if N < 4:
        return (0, 0, 0, 0, N)
    ids_t = np.asarray(ids_t, dtype=np.int64)
    cols = []      # per node of t: the prefix counts of its links
    res_col = 0
    for rl in nodes_t:
        pref = [prefix_counts(pos, Ls, ids_t[[(s + i) % Lt for i in range((e - s) % Lt)]]) for (s, e) in rl]
        cols.append(pref)
        res_col += M.resolved_of_node([p[-1] for p in pref], N)
    same = disc = res_row = 0
    for arcs in nodes_s:
        R = [arc_count(pres, st, en) for (st, en) in arcs]
        res_row += M.resolved_of_node(R, N)
        for pref in cols:
            I = np.array([[arc_count(p, st, en) for p in pref] for (st, en) in arcs], dtype=np.int64)
            s4, d4 = M.pair_terms(I, N)
            same += s4
            disc += d4
    assert same % 4 == 0 and disc % 4 == 0 and res_row % 2 == 0 and res_col % 2 == 0
    return (same // 4, disc // 4, res_row // 2, res_col // 2, N)


def model_pair(n_taxa, name_to_id, s_newick, t_newick, recentre=True):
    return model_counts(n_taxa, flat(s_newick, name_to_id, recentre), flat(t_newick, name_to_id, recentre))


def taxa_of(tree_newick, ids):
    _, allv = bruteforce.splits_of(bruteforce.parse_newick(tree_newick), ids)
    return {int(x) for x in np.nonzero(allv)[0]}


def brute_pair(names, s_newick, t_newick):
    """The five words by enumerating the quartets of the shared taxa (split-based, bruteforce.splits_of)."""
    ids = {nm: i for i, nm in enumerate(names)}
    taxa = sorted(taxa_of(s_newick, ids) & taxa_of(t_newick, ids))
    if len(taxa) < 4:
        return (0, 0, 0, 0, len(taxa))
    ts = M._topologies(s_newick, ids, taxa)
    tt = M._topologies(t_newick, ids, taxa)
    conc = sum(1 for q, v in ts.items() if tt.get(q) == v)
    disc = sum(1 for q, v in ts.items() if q in tt and tt[q] != v)
    return (conc, disc, len(ts), len(tt), len(taxa))


def swapped(words):
    """(s,t) -> (t,s): the two resolved words change places."""
    a = np.asarray(words)
    return a[..., [0, 1, 3, 2, 4]]
