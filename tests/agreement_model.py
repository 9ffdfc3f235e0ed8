"""Per-tree quartet agreement (qs_tree_agreement): a numpy model of the node-pair formulas and a per-quartet brute force.

For evaluation tree t with taxon set P_t (N = |P_t|), compared with the reference restricted to P_t, the four counts are
(concordant, discordant, resolved_eval, resolved_ref). The model walks node pairs (u of the reference, v of t) with the
matrix I[r][c] = |A_r & B_c & P_t| over their links, exactly as the kernel does, using the row/column aggregates of
DESIGN.md 9. The brute force enumerates the C(N,4) quartets with bruteforce.splits_of and shares no code with it.
"""
import itertools

import numpy as np

import bruteforce
from quartetscores_amd import flatten


def c2(x):
    x = np.asarray(x, dtype=np.int64)
    return x * (x - 1) // 2


def resolved_of_node(S, N):
    """2 x (the quartets this node claims): sum_r C(S_r,2) (C(N-S_r,2) - sum_{r' != r} C(S_r',2))."""
    S = np.asarray(S, dtype=np.int64)
    s2 = c2(S)
    return int((s2 * (c2(N - S) - (s2.sum() - s2))).sum())


def pair_terms(I, N):
    """(same + mixed, disc) of one node pair = 4 x its share of concordant / discordant."""
    I = np.asarray(I, dtype=np.int64)
    R, C = I.sum(1), I.sum(0)
    CI = c2(I)
    T2 = CI.sum()
    rowC2, colC2 = CI.sum(1), CI.sum(0)
    rowX = c2(C[None, :] - I).sum(1)
    colX = c2(R[:, None] - I).sum(0)
    rowIC = (I * C[None, :]).sum(1)
    colIR = (I * R[:, None]).sum(0)
    rowSq, colSq = (I * I).sum(1), (I * I).sum(0)
    Rr, Cc = R[:, None], C[None, :]
    X = N - Rr - Cc + I
    D = c2(X) - (colX[None, :] - c2(Rr - I)) - (rowX[:, None] - c2(Cc - I)) + (T2 - rowC2[:, None] - colC2[None, :] + CI)
    same = (CI * D).sum()
    mixed = ((c2(Rr - I) - (rowC2[:, None] - CI)) * (c2(Cc - I) - (colC2[None, :] - CI))).sum()
    A, B = Rr - I, Cc - I
    BR = colIR[None, :] - I * Rr
    AC = rowIC[:, None] - I * Cc
    A2, B2 = rowSq[:, None] - I * I, colSq[None, :] - I * I
    disc = (I * (X * A * B - A * BR - AC * B + A2 * B + A * B2)).sum()
    G = I @ I.T                                   # G[r][i] = sum_c I_rc I_ic
    H = (I * I) @ (I * I).T
    Q = (G * G - H).sum() - (np.diag(G) ** 2 - np.diag(H)).sum()
    return int(same + mixed), int(disc + Q)


def ref_links(ref: flatten.RefTree):
    """Per inner reference node with >= 3 links: (child id boundaries b_0 < ... < b_m, has_parent). Child j holds the ids
    [b_j, b_{j+1}); the parent link (if any) holds the rest."""
    n_nodes = ref.n_nodes
    lo = np.full(n_nodes, 1 << 30, dtype=np.int64)
    hi = np.zeros(n_nodes, dtype=np.int64)
    for i, v in enumerate(ref.leaf_node):
        lo[v], hi[v] = i, i + 1
    for v in range(n_nodes - 1, 0, -1):           # preorder: children behind their parent
        p = ref.parent[v]
        lo[p], hi[p] = min(lo[p], lo[v]), max(hi[p], hi[v])
    kids = [[] for _ in range(n_nodes)]
    for v in range(1, n_nodes):
        kids[ref.parent[v]].append(v)
    out = []
    for u in range(n_nodes):
        ks = sorted(kids[u], key=lambda v: lo[v])
        has_parent = ref.parent[u] >= 0
        if len(ks) + has_parent < 3:
            continue
        out.append(([int(lo[v]) for v in ks] + [int(hi[ks[-1]])], has_parent))
    return out


def model_counts(ref: flatten.RefTree, leaf_ids, node_ranges):
    """(concordant, discordant, resolved_eval, resolved_ref) from the flattened evaluation tree (flatten.flatten_tree)."""
    L = len(leaf_ids)
    N = L
    if N < 4:
        return (0, 0, 0, 0)
    ids = np.asarray(leaf_ids, dtype=np.int64)
    present = np.zeros(ref.n_taxa + 1, dtype=np.int64)
    present[ids] = 1
    pre = np.concatenate([[0], np.cumsum(present)])

    def positions(s, e):
        return [(s + i) % L for i in range((e - s) % L)]

    cols = []     # per eval node: per link, id membership prefix counts
    res_eval = 0
    for rl in node_ranges:
        pref = []
        for (s, e) in rl:
            m = np.zeros(ref.n_taxa + 1, dtype=np.int64)
            m[ids[positions(s, e)]] = 1
            pref.append(np.concatenate([[0], np.cumsum(m)]))
        cols.append(pref)
        res_eval += resolved_of_node([p[-1] for p in pref], N)
    same = disc = res_ref = 0
    for bnd, has_parent in ref_links(ref):
        m = len(bnd) - 1
        R = [pre[bnd[j + 1]] - pre[bnd[j]] for j in range(m)]
        if has_parent:
            R.append(N - (pre[bnd[m]] - pre[bnd[0]]))
        res_ref += resolved_of_node(R, N)
        for pref in cols:
            I = np.zeros((len(R), len(pref)), dtype=np.int64)
            for c, p in enumerate(pref):
                for j in range(m):
                    I[j, c] = p[bnd[j + 1]] - p[bnd[j]]
                if has_parent:
                    I[m, c] = p[-1] - (p[bnd[m]] - p[bnd[0]])
            s, d = pair_terms(I, N)
            same += s
            disc += d
    assert same % 4 == 0 and disc % 4 == 0 and res_eval % 2 == 0 and res_ref % 2 == 0
    return (same // 4, disc // 4, res_eval // 2, res_ref // 2)


def model_tree(ref: flatten.RefTree, newick_text, recentre=True):
    from quartetscores_amd import newick
    leaf_ids, _, node_ranges = flatten.flatten_tree(newick.parse_tree(newick_text), ref.name_to_id, recentre)
    return model_counts(ref, leaf_ids, node_ranges)


def _topologies(tree_newick, ids, taxa):
    """quartet (sorted id tuple) -> its pairing slot (0: ab|cd, 1: ac|bd, 2: ad|bc) for every quartet of `taxa` the tree resolves."""
    n = len(ids)
    splits, _ = bruteforce.splits_of(bruteforce.parse_newick(tree_newick), ids)
    mask = np.zeros(n, dtype=bool)
    mask[taxa] = True
    out = {}
    for sp in splits:
        a_side = [x for x in taxa if sp[x]]
        b_side = [x for x in taxa if not sp[x]]
        if len(a_side) < 2 or len(b_side) < 2:
            continue
        for p in itertools.combinations(a_side, 2):
            for q in itertools.combinations(b_side, 2):
                quad = tuple(sorted(p + q))
                partner = p[1] if p[0] == quad[0] else p[0] if p[1] == quad[0] else q[1] if q[0] == quad[0] else q[0]
                out[quad] = quad.index(partner) - 1
    return out


def brute_counts(ref_newick, names, tree_newick):
    """The four counts by enumerating the quartets of the evaluation tree's taxa (split-based, bruteforce.splits_of)."""
    ids = {nm: i for i, nm in enumerate(names)}
    _, allv = bruteforce.splits_of(bruteforce.parse_newick(tree_newick), ids)
    taxa = [int(x) for x in np.nonzero(allv)[0]]
    if len(taxa) < 4:
        return (0, 0, 0, 0)
    te = _topologies(tree_newick, ids, taxa)
    tr = _topologies(ref_newick, ids, taxa)
    conc = sum(1 for q, s in te.items() if tr.get(q) == s)
    disc = sum(1 for q, s in te.items() if q in tr and tr[q] != s)
    return (conc, disc, len(te), len(tr))


def derived(counts, taxa):
    """(n, 4) counts + (n,) taxa -> dict of the derived columns (quartets, eval_only, ref_only, unresolved, concordance)."""
    return _derived(np.asarray(counts, dtype=np.int64), np.asarray(taxa, dtype=np.int64))


def _derived(a, n):
    from quartetscores_amd.engine import agreement_columns
    return agreement_columns(a, n)
