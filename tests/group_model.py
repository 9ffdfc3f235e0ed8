"""Quartet support of taxon groups (qs_group_support) without a GPU.

model_counts: the six words of every hypothesis from a downloaded count table and a label matrix, by walking the 4-sets in rank
order (taxon_model.quads_in_rank_order) -- no rows, no needed label, no permutation of cells as in qs_groups.hip: every 4-set is
sorted by label, the three pairings the hypothesis names are written down as id pairs and looked up with slot_of_pairing.
brute_counts: the same words straight from Newick strings, asking every tree which pairing of a counted 4-set one of its
bipartitions displays (bruteforce.splits_of); the count table plays no part.
"""
import numpy as np

import bruteforce
from taxon_model import quads_in_rank_order

FIELDS = ("quartets", "q1", "q2", "q3", "outvoted", "uninformed")


def kind_of(row):
    """0 quad, 1 split, None = neither"""
    cnt = np.bincount(np.asarray(row, dtype=np.int64), minlength=5)
    if len(cnt) > 5:
        return None
    if cnt[3] or cnt[4]:
        return 0 if cnt[1:5].all() else None
    return 1 if cnt[1] >= 2 and cnt[2] >= 2 else None


def whole_table_quartets(row):
    cnt = np.bincount(np.asarray(row, dtype=np.int64), minlength=5).astype(object)
    if kind_of(row) == 0:
        return int(cnt[1] * cnt[2] * cnt[3] * cnt[4])
    return int(cnt[1] * (cnt[1] - 1) // 2 * (cnt[2] * (cnt[2] - 1) // 2))


def slot_of_pairing(x, y, z, w):
    """cell of the pairing xy|zw in the tuple of the 4-set {x,y,z,w}: the rank of the smallest id's partner among the other three"""
    ids = np.stack([x, y, z, w], axis=1)
    partner = np.stack([y, x, w, z], axis=1)
    first = ids.argmin(axis=1)
    p = partner[np.arange(len(ids)), first]
    return (ids < p[:, None]).sum(axis=1) - 1


def counted_mask(cols, row, kind):
    """which 4-sets (cols = their four id columns) a hypothesis counts: one taxon of every label (quad), two of label 1 and two of
    label 2 (split) -- by a code per label whose sum over the four taxa is attained by that pattern alone"""
    code = np.array([0, 2, 4, 8, 16] if kind == 0 else [64, 1, 8, 64, 64], dtype=np.int32)[np.asarray(row, dtype=np.int64)]
    return (code[cols[0]] + code[cols[1]] + code[cols[2]] + code[cols[3]]) == (30 if kind == 0 else 18)


def counted_pairings(quads, row, cols=None):
    """The 4-sets of `quads` (ids in any order per line) a hypothesis counts and, per counted 4-set, the id pairs (x, y, z, w) of
    q1, q2, q3 = n(xy|zw): -> (mask over quads, three (m, 4) id arrays)"""
    row = np.asarray(row, dtype=np.int64)
    kind = kind_of(row)
    assert kind is not None
    mask = counted_mask(quads.T if cols is None else cols, row, kind)
    q = quads[mask]
    l = row[q]
    if kind == 0:
        order = np.argsort(l, axis=1)                       # taxa of S1, S2, S3, S4
        a, b, c, d = (np.take_along_axis(q, order[:, k:k + 1], axis=1)[:, 0] for k in range(4))
        return mask, [np.stack(x, axis=1) for x in ((a, b, c, d), (a, c, b, d), (a, d, b, c))]
    key = np.argsort(l * (len(row) + 1) + q, axis=1)        # by label, then by id: g1 < g2, h1 < h2
    g1, g2, h1, h2 = (np.take_along_axis(q, key[:, k:k + 1], axis=1)[:, 0] for k in range(4))
    return mask, [np.stack(x, axis=1) for x in ((g1, g2, h1, h2), (g1, h1, g2, h2), (g1, h2, g2, h1))]


def model_counts(table, labels, n, rank_lo=0, quads=None, cols=None):
    """(H, 6) python-int words (object array: exact at any count) of the hypotheses `labels` (H, n) over the tuples `table` holds:
    the ranks [rank_lo, rank_lo + len(table)); quads = quads_in_rank_order(n, rank_lo, len(table)) and cols = its contiguous
    transpose if the caller has them"""
    labels = np.asarray(labels).reshape(-1, n)
    table = np.asarray(table)
    if quads is None:
        quads = quads_in_rank_order(n, rank_lo, len(table))
    if cols is None:
        cols = np.ascontiguousarray(quads.T)
    # int64 where no sum can leave it, python ints otherwise
    exact = np.int64 if int(table.max(initial=0)) * 3 * max(len(table), 1) < 2 ** 62 else object
    out = np.zeros((len(labels), 6), dtype=object)
    for h, row in enumerate(labels):
        mask, pairings = counted_pairings(quads, row, cols)
        t = table[mask]
        idx = np.arange(len(t))
        q = [t[idx, slot_of_pairing(*p.T)].astype(exact) for p in pairings]
        out[h] = [int(mask.sum()), int(q[0].sum()), int(q[1].sum()), int(q[2].sum()),
                  int((np.maximum(q[1], q[2]) > q[0]).sum()), int(((q[0] + q[1] + q[2]) == 0).sum())]
    return out


def brute_counts(names, eval_newicks, labels):
    """The same words from the trees themselves: per tree and counted 4-set, which of the three pairings a bipartition displays"""
    n = len(names)
    ids = {nm: i for i, nm in enumerate(names)}
    labels = np.asarray(labels).reshape(-1, n)
    quads = np.array(list(bruteforce.all_quartets(n)), dtype=np.int64).reshape(-1, 4)
    out = np.zeros((len(labels), 6), dtype=object)
    for h, row in enumerate(labels):
        mask, pairings = counted_pairings(quads, row)
        q = np.zeros((int(mask.sum()), 3), dtype=np.int64)
        for nw in eval_newicks:
            splits, present = bruteforce.splits_of(bruteforce.parse_newick(nw), ids)
            S = np.array(splits, dtype=bool)
            for k, p in enumerate(pairings):
                X, Y, Z, W = (S[:, p[:, i]] for i in range(4))
                shown = ((X == Y) & (Z == W) & (X != Z)).any(axis=0)
                q[:, k] += shown & present[p].all(axis=1)
        out[h] = [len(q), int(q[:, 0].sum()), int(q[:, 1].sum()), int(q[:, 2].sum()),
                  int((np.maximum(q[:, 1], q[:, 2]) > q[:, 0]).sum()), int((q.sum(axis=1) == 0).sum())]
    return out


def random_hypothesis(rng, n, kind, use_all=False):
    """one label row: kind 0 quad, 1 split; use_all: no taxon gets label 0"""
    while True:
        if kind == 0:
            row = rng.integers(1 if use_all else 0, 5, size=n)
        else:
            row = rng.integers(1 if use_all else 0, 3, size=n)
        if kind_of(row) == kind:
            return row.astype(np.uint8)


def hypotheses(n, count, seed, cap=None):
    """`count` hypotheses of both kinds mixed (count >= 6), the first six of them the edge cases: a quad of four singletons, a quad
    that uses all n taxa, a quad and a split whose groups interleave in id order, a split with |S1| = 2, a split of all taxa.
    cap: no group keeps more than `cap` taxa (the others get label 0), which bounds the counted 4-sets at many taxa"""
    rng = np.random.default_rng(seed)
    rows = []
    single = np.zeros(n, dtype=np.uint8)
    single[rng.choice(n, 4, replace=False)] = [1, 2, 3, 4]
    rows.append(single)
    rows.append(random_hypothesis(rng, n, 0, use_all=True))
    rows.append(((np.arange(n) % 4) + 1).astype(np.uint8) if n >= 8 else random_hypothesis(rng, n, 0))
    rows.append(((np.arange(n) % 2) + 1).astype(np.uint8))
    two = np.zeros(n, dtype=np.uint8)
    pick = rng.choice(n, min(n, 2 + max(2, n // 2)), replace=False)
    two[pick[:2]], two[pick[2:]] = 1, 2
    rows.append(two)
    rows.append(random_hypothesis(rng, n, 1, use_all=True))
    while len(rows) < count:
        rows.append(random_hypothesis(rng, n, len(rows) % 2))
    rows = np.stack(rows[:count])
    if cap is not None:
        for row in rows:
            for label in range(1, 5):
                members = np.nonzero(row == label)[0]
                if len(members) > cap:
                    row[rng.choice(members, len(members) - cap, replace=False)] = 0
    return rows
