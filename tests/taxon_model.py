"""Per-taxon quartet support (qs_taxon_support) without a GPU.

model_counts: the numpy model of qs_taxon.hip on a downloaded count table and a flatten.RefTree: the reference's topology of
a 4-set a<b<c<d from the depths of the LCAs of its three adjacent pairs, as classify() in qs_score.hip decides it.
brute_counts: the same six sums from bipartitions alone (tests/bruteforce.py): the reference displays ab|cd iff one of
its splits has a,b on one side and c,d on the other; the counts come from bruteforce.count_table.
"""
import numpy as np

import bruteforce
from helpers import binom

FIELDS = ("ref_resolved", "concordant", "discordant", "eval_only", "outvoted", "uninformed")


def quads_in_rank_order(n, r0=0, nq=None):
    """ids (a, b, c, d) of the ranks [r0, r0 + nq): rank = C(d,4) + C(c,3) + C(b,2) + a"""
    ks = np.arange(n + 1)
    c4, c3, c2 = binom(ks, 4), binom(ks, 3), binom(ks, 2)
    nq = int(c4[n]) - r0 if nq is None else nq
    r = np.arange(r0, r0 + nq, dtype=np.int64)
    d = np.searchsorted(c4, r, side="right") - 1
    r = r - c4[d]
    c = np.searchsorted(c3, r, side="right") - 1
    r = r - c3[c]
    b = np.searchsorted(c2, r, side="right") - 1
    return np.stack([r - c2[b], b, c, d], axis=1)


def lca_depths(ref):
    """(n, n) depth of the LCA of two leaves by lookup id (ids are the depth-first leaf order: the LCA of i < j is the
    shallowest LCA of the adjacent pairs between them)"""
    parent = np.asarray(ref.parent, dtype=np.int64)
    depth = np.zeros(len(parent), dtype=np.int64)
    for v in range(len(parent)):
        x, k = v, 0
        while parent[x] >= 0:
            x, k = parent[x], k + 1
        depth[v] = k
    n = len(ref.leaf_node)
    adj = np.zeros(max(n - 1, 0), dtype=np.int64)
    for i in range(n - 1):
        x, y = int(ref.leaf_node[i]), int(ref.leaf_node[i + 1])
        while x != y:
            if depth[x] >= depth[y]:
                x = int(parent[x])
            else:
                y = int(parent[y])
        adj[i] = depth[x]
    D = np.zeros((n, n), dtype=np.int64)
    for i in range(n - 1):
        D[i, i + 1:] = np.minimum.accumulate(adj[i:])
    return D + D.T


def _accumulate(n, quads, terms):
    """terms (nq, 6) of the quartets -> (n, 6) int64: every quartet's terms go to its four taxa"""
    out = np.zeros((n, 6), dtype=np.int64)
    for k in range(6):
        w = terms[:, k].astype(np.float64)
        assert w.sum() < 2 ** 52   # float64 weights stay exact
        for x in range(4):
            out[:, k] += np.bincount(quads[:, x], weights=w, minlength=n).astype(np.int64)
    return out


def _terms(T, topo):
    """per quartet the six words; T (nq, 3) counts, topo 0 (s0s1|s2s3), 2 (s0s3|s1s2) or 255 (unresolved)"""
    T = np.asarray(T).astype(np.int64)
    res = topo != 255
    q1 = np.where(topo == 0, T[:, 0], T[:, 2])
    alt = np.maximum(T[:, 1], np.where(topo == 0, T[:, 2], T[:, 0]))
    s = T.sum(1)
    z = np.zeros_like(s)
    return np.stack([res.astype(np.int64), np.where(res, q1, z), np.where(res, s - q1, z), np.where(res, z, s),
                     (res & (alt > q1)).astype(np.int64), (res & (s == 0)).astype(np.int64)], axis=1)


def model_topology(ref, quads):
    D = lca_depths(ref)
    a, b, c, d = quads.T
    d01, d12, d23 = D[a, b], D[b, c], D[c, d]
    mx = np.maximum(d01, d23)
    return np.where(d12 < mx, 0, np.where(d12 > mx, 2, 255)).astype(np.uint8)


def model_counts(table, ref, rank_lo=0):
    """(n, 6) int64 in FIELDS order from the tuples [rank_lo, rank_lo + len(table)) of the count table"""
    n = len(ref.leaf_node)
    table = np.asarray(table).reshape(-1, 3)
    quads = quads_in_rank_order(n, rank_lo, len(table))
    return _accumulate(n, quads, _terms(table, model_topology(ref, quads)))


def brute_counts(ref_newick, names, eval_newicks):
    """the same from bipartitions: names = the taxa in lookup-id order"""
    n = len(names)
    ids = {nm: i for i, nm in enumerate(names)}
    quads = np.array(bruteforce.rank_order_quads(n), dtype=np.int64).reshape(-1, 4)
    splits, _ = bruteforce.splits_of(bruteforce.parse_newick(ref_newick), ids)
    S = np.array(splits, dtype=bool)
    A, B, C, D = (S[:, quads[:, i]] for i in range(4))
    t0 = ((A == B) & (C == D) & (A != C)).any(axis=0)
    t1 = ((A == C) & (B == D) & (A != B)).any(axis=0)
    t2 = ((A == D) & (B == C) & (A != B)).any(axis=0)
    assert not t1.any()   # ids in depth-first order: the crossing pairing is never the reference's
    topo = np.where(t0, 0, np.where(t2, 2, 255)).astype(np.uint8)
    return _accumulate(n, quads, _terms(bruteforce.count_table(names, eval_newicks), topo))


def resolved_quartets(ref):
    """number of 4-sets the reference resolves, closed form: a 4-set is unresolved iff its taxa lie behind four different
    links of one node, so C(n,4) minus the fourth elementary symmetric polynomial of every node's link sizes"""
    parent = np.asarray(ref.parent, dtype=np.int64)
    n = len(ref.leaf_node)
    below = np.zeros(len(parent), dtype=object)
    for i in range(n):
        x = int(ref.leaf_node[i])
        while x >= 0:
            below[x] += 1
            x = int(parent[x])
    unresolved = 0
    for v in range(len(parent)):
        links = [int(below[u]) for u in np.nonzero(parent == v)[0]]
        if not links:
            continue
        if parent[v] >= 0:
            links.append(n - int(below[v]))
        e = [1, 0, 0, 0, 0]
        for x in links:
            for k in range(4, 0, -1):
                e[k] += e[k - 1] * x
        unresolved += e[4]
    return int(binom(n, 4)) - unresolved
