"""Quartet support of taxon pairs (qs_taxon_pair_support) without a GPU.

pair_counts: the numpy model of qs_taxon_pairs.hip on a downloaded count table and a flatten.RefTree, over the quartets in rank
order. Every 4-set gives each of its four taxa x three partners, one per pairing; t = the pairing's count, s = the tuple sum. The
reference's topology of the 4-set comes from the LCA depths of all six pairs (placement_model.Shape: LCA nodes from leaf intervals):
the pairing whose two LCAs lie deepest in sum is the displayed one (the four-point condition on a rooted tree), none if the three
sums are equal -- not the kernel's comparison of three adjacent pairs in sorted order.
brute_counts: the same from plain loops over all 4-sets, the reference's topology read from bruteforce.count_table of the reference
alone (the cell that holds 1).
columns: the columns of QuartetScores --taxon-pairs, by definition.
"""
import itertools

import numpy as np

import bruteforce
from placement_model import Shape, _quad_columns
from quartetscores_amd import newick, synth

FIELDS = ("n_rt", "n_ra", "T_rt", "S_rt", "T_ra", "S_ra", "T_all", "S_all")
COLUMNS = ("a", "b", "name_a", "name_b", "quartets", "ref_together", "ref_apart", "together", "apart", "affinity", "kept", "joined")
PAIRINGS = (((0, 1), (2, 3)), ((0, 2), (1, 3)), ((0, 3), (1, 2)))   # the tuple's three cells, ids in sorted order


def reference_topology(ref, quads):
    """per 4-set 0, 1, 2 = the pairing the reference displays, 255 = unresolved"""
    S = Shape(ref)
    D = S.depth[S.lca].astype(np.int32)                         # (n, n) depth of the LCA (the diagonal is never read)
    q = quads if isinstance(quads, tuple) else [quads[:, k] for k in range(4)]
    sums = np.stack([D[q[a], q[b]] + D[q[c], q[d]] for (a, b), (c, d) in PAIRINGS], axis=1)
    best = sums.argmax(axis=1)
    top, low = sums.max(axis=1), sums.min(axis=1)
    # (a tree: the two smaller sums are equal; all three equal = the four taxa behind four links of one node)
    assert (sums.sum(axis=1) - top - low == low).all()
    return np.where(top > low, best, 255).astype(np.uint8)


def pair_counts(table, ref, taxa=None):
    """(len(taxa), n, 8) int64 in FIELDS order: the rows of the listed taxa (default: all, in id order) from the whole count table"""
    n = len(ref.leaf_node)
    T = np.asarray(table).reshape(-1, 3)
    quads = _quad_columns(n)                                    # four int32 columns, cached
    assert len(T) == len(quads[0])
    topo = reference_topology(ref, quads)
    res = topo != 255
    exact = int(T.max(initial=0)) * len(T) * 3 >= 2 ** 52      # float64 weights of bincount stay exact below that
    Ti = T.astype(np.int64)
    s = Ti.sum(axis=1)
    # per (pair, class of the 4-set for the pair: 0 rt, 1 ra, 2 unresolved): the 4-sets, the sum of t and the sum of s
    cnt, sum_t, sum_s = (np.zeros(n * n * 3, dtype=np.int64) for _ in range(3))

    def add(acc, idx, w):
        if exact:
            np.add.at(acc, idx, w)
        else:
            acc += np.bincount(idx, weights=w.astype(np.float64), minlength=len(acc)).astype(np.int64)

    unresolved_or_apart = np.where(res, 1, 2).astype(np.int32)
    for k in range(4):
        for slot in range(3):
            cls = np.where(topo == slot, 0, unresolved_or_apart)
            idx = (quads[k] * n + quads[k ^ (slot + 1)]) * 3 + cls          # x's partner in the slot's pairing
            cnt += np.bincount(idx, minlength=len(cnt))
            add(sum_t, idx, Ti[:, slot])
            add(sum_s, idx, s)
    cnt, sum_t, sum_s = (a.reshape(n * n, 3) for a in (cnt, sum_t, sum_s))
    out = np.stack([cnt[:, 0], cnt[:, 1], sum_t[:, 0], sum_s[:, 0], sum_t[:, 1], sum_s[:, 1], sum_t.sum(axis=1), sum_s.sum(axis=1)], axis=1)
    out = out.reshape(n, n, 8)
    return out if taxa is None else out[np.asarray(taxa, dtype=np.int64)]


def brute_counts(ref_newick, names, eval_newicks):
    """(n, n, 8) int64 by plain loops: names = the taxa in lookup-id order"""
    n = len(names)
    shown = bruteforce.count_table(names, [ref_newick]).astype(np.int64)
    table = bruteforce.count_table(names, eval_newicks).astype(np.int64)
    out = np.zeros((n, n, 8), dtype=np.int64)
    for rank, ids in enumerate(bruteforce.rank_order_quads(n)):
        cells, ref_cells = table[rank], shown[rank]
        assert ref_cells.sum() <= 1
        s = int(cells.sum())
        for slot, halves in enumerate(PAIRINGS):
            t = int(cells[slot])
            for u, v in halves:
                for x, j in ((ids[u], ids[v]), (ids[v], ids[u])):
                    w = out[x, j]
                    if ref_cells[slot]:
                        w[0] += 1; w[2] += t; w[3] += s
                    elif ref_cells.sum():
                        w[1] += 1; w[4] += t; w[5] += s
                    w[6] += t; w[7] += s
    return out


def check_identities(counts, support):
    """the matrix (n, n, 8) against itself and against the six words per taxon of qs_taxon_support (n, 6)"""
    M = np.asarray(counts, dtype=np.int64)
    sup = np.asarray(support, dtype=np.int64)
    n = len(M)
    assert (M == M.transpose(1, 0, 2)).all()                    # symmetric, word for word
    assert (M[np.arange(n), np.arange(n)] == 0).all()
    row = M.sum(axis=1)
    resolved, conc, disc, eval_only = sup[:, 0], sup[:, 1], sup[:, 2], sup[:, 3]
    assert (row[:, 0] == resolved).all() and (row[:, 1] == 2 * resolved).all()
    assert (row[:, 2] == conc).all() and (row[:, 4] == disc).all()
    assert (row[:, 6] - row[:, 2] - row[:, 4] == eval_only).all()
    assert (row[:, 7] == 3 * (conc + disc + eval_only)).all()
    assert (row[:, 3] == conc + disc).all()


def columns(counts, names, taxa=None):
    """the columns of --taxon-pairs in COLUMNS order: one entry per unordered pair a < b of lookup ids with at least one listed taxon
    (taxa = the lookup ids of the rows of counts; default all, in id order), row-major"""
    n = len(names)
    taxa = list(range(n)) if taxa is None else [int(x) for x in taxa]
    M = np.asarray(counts, dtype=np.int64).reshape(len(taxa), n, 8)
    row_of = {x: i for i, x in enumerate(taxa)}
    out = {name: [] for name in COLUMNS}
    ratio = lambda num, den: num / den if den else float("nan")
    for a, b in itertools.combinations(range(n), 2):
        if a in row_of:
            w = M[row_of[a], b]
        elif b in row_of:
            w = M[row_of[b], a]
        else:
            continue
        n_rt, n_ra, T_rt, S_rt, T_ra, S_ra, T_all, S_all = (int(v) for v in w)
        vals = (a, b, names[a], names[b], (n - 2) * (n - 3) // 2, n_rt, n_ra, T_all, S_all - T_all,
                ratio(T_all, S_all), ratio(T_rt, S_rt), ratio(T_ra, S_ra))
        for name, v in zip(COLUMNS, vals):
            out[name].append(v)
    kinds = {"name_a": None, "name_b": None, "affinity": np.float64, "kept": np.float64, "joined": np.float64}
    return {k: (v if kinds.get(k, np.int64) is None else np.array(v, dtype=kinds.get(k, np.int64))) for k, v in out.items()}


def planted(n=24, seed=6, moved=28, kept=8, noise=4):
    """a random binary reference of n taxa and moved + kept + noise evaluation trees: in `moved` of them taxon u, the first leaf of
    the reference, is pruned and regrafted as the sister of v, the leaf most nodes away from it; `kept` are the reference itself,
    `noise` are random trees -> (reference, trees, u, v)"""
    ref_nw = synth.random_tree(n, np.random.default_rng(seed))
    root = newick.parse_tree(ref_nw)
    leaves = [x for x in newick.preorder(root) if x.is_leaf]

    def ancestors(x):
        out = []
        while x is not None:
            out.append(id(x))
            x = x.parent
        return out

    up = ancestors(leaves[0])
    far = max(leaves[1:], key=lambda x: len(set(up) ^ set(ancestors(x))))
    u, v = leaves[0].name, far.name
    pruned = newick.prune(newick.parse_tree(ref_nw), [u])
    at = next(x for x in newick.preorder(pruned) if x.is_leaf and x.name == v)
    i = at.parent.children.index(at)
    at.parent.children[i] = newick.Node(children=[at, newick.Node(u)])
    trees = [newick.write(pruned)] * moved + [ref_nw] * kept + synth.tree_set(n, noise, seed + 1)
    return ref_nw, trees, u, v
