"""Quartet placement of taxa on the reference tree (qs_taxon_placement / qs_placement_scores) without a GPU.

link_sums: the numpy model of qs_place.hip on a downloaded count table and a flatten.RefTree, over the quartets in rank order:
every 4-set gives each of its four taxa x three counts n(x t|..), one per partner t, which go to the link of the median node of
the three other taxa that leads towards t. The median is taken as the deepest of the three pairwise LCAs and the link from the
leaf interval of the node -- not the kernel's case analysis over lca(p,q) and lca(q,r).
scores: the preorder recurrence over the link sums. columns: the columns of QuartetScores --place-taxa, by definition.
brute_scores: x really re-inserted on every edge of newick.prune(ref, [x]), the displayed topologies read from bipartitions
(bruteforce.count_table of the one tree).
"""
import functools

import numpy as np

import bruteforce
from quartetscores_amd import newick
from taxon_model import quads_in_rank_order

COLUMNS = ("taxon", "name", "current", "best", "gain", "n_best", "best_node", "best_lo", "best_hi", "distance")


class Shape:
    """the reference tree as arrays: depth, children counts, leaf interval [lo, lo + cnt) and LCA node of every leaf pair"""

    def __init__(self, ref):
        self.parent = np.asarray(ref.parent, dtype=np.int64)
        self.leaf_node = np.asarray(ref.leaf_node, dtype=np.int64)
        N, n = len(self.parent), len(self.leaf_node)
        self.N, self.n = N, n
        self.root = int(np.nonzero(self.parent < 0)[0][0])
        self.depth = np.zeros(N, dtype=np.int64)
        for v in range(N):
            x, k = v, 0
            while self.parent[x] >= 0:
                x, k = self.parent[x], k + 1
            self.depth[v] = k
        self.nchild = np.bincount(self.parent[self.parent >= 0], minlength=N)
        self.links = self.nchild + (self.parent >= 0)
        self.lo = np.full(N, n, dtype=np.int64)
        self.hi = np.zeros(N, dtype=np.int64)
        self.child_to = np.full((N, n), -1, dtype=np.int64)   # [m, leaf] = the child of m that holds the leaf (-1: not below m)
        for i in range(n):
            x = int(self.leaf_node[i])
            while True:
                self.lo[x], self.hi[x] = min(self.lo[x], i), max(self.hi[x], i + 1)
                p = int(self.parent[x])
                if p < 0:
                    break
                self.child_to[p, i] = x
                x = p
        self.lca = np.zeros((n, n), dtype=np.int64)
        for m in np.argsort(self.depth, kind="stable"):       # deeper nodes overwrite: the deepest node above both leaves
            if self.nchild[m]:
                self.lca[self.lo[m]:self.hi[m], self.lo[m]:self.hi[m]] = m


@functools.lru_cache(maxsize=2)
def _quad_columns(n):
    return tuple(np.ascontiguousarray(col, dtype=np.int32) for col in quads_in_rank_order(n).T)


def link_sums(table, ref, taxa=None):
    """(len(taxa), 2 N) int64: W_x of every listed taxon (default: all, in id order) from the whole count table"""
    S = Shape(ref)
    n, N = S.n, S.N
    T = np.asarray(table).reshape(-1, 3)
    quads = _quad_columns(n)
    assert len(T) == len(quads[0])
    exact = int(T.max(initial=0)) * len(T) * 3 >= 2 ** 52      # float64 weights of bincount stay exact below that
    weights = [T[:, slot].astype(np.int64 if exact else np.float64) for slot in range(3)]
    lca, depth, child_to = S.lca.astype(np.int32), S.depth.astype(np.int32), S.child_to.astype(np.int32).ravel()
    out = np.zeros(n * 2 * N, dtype=np.int64)
    for k in range(4):
        x = quads[k]
        o = [quads[j] for j in range(4) if j != k]
        m = lca[o[0], o[1]]                                    # median of three leaves: the deepest of the pairwise LCAs
        for a, b in ((1, 2), (0, 2)):
            other = lca[o[a], o[b]]
            m = np.where(depth[other] > depth[m], other, m)
        base = x.astype(np.int64) * (2 * N)
        for slot in range(3):
            t = quads[k ^ (slot + 1)]                          # x's partner in the slot's pairing
            down = child_to[m * n + t]                         # the child of m that holds t, or -1: m's parent link
            idx = base + np.where(down >= 0, down, N + m)
            if exact:
                np.add.at(out, idx, weights[slot])
            else:
                out += np.bincount(idx, weights=weights[slot], minlength=len(out)).astype(np.int64)
    out = out.reshape(n, 2 * N)
    return out if taxa is None else out[np.asarray(taxa, dtype=np.int64)]


def scores(ref, links):
    """(rows, N) int64: the score of the edge above every node (the root's entry is 0) from rows of link sums"""
    S = Shape(ref)
    W = np.asarray(links, dtype=np.int64).reshape(-1, 2 * S.N)
    out = np.zeros((len(W), S.N), dtype=np.int64)
    out[:, S.root] = W[:, S.N:].sum(axis=1)
    for v in np.argsort(S.depth, kind="stable"):
        p = int(S.parent[v])
        if p >= 0:
            out[:, v] = out[:, p] - W[:, S.N + p] + W[:, v]
    out[:, S.root] = 0
    return out


def position_keys(S, x):
    """per node v the position of the edge above it for taxon x: the bipartition it induces among the OTHER taxa, as the id
    interval (in the others' numbering) of the side without the smallest other taxon; (0, 0) = all others on one side. x's own
    pendant edge takes the position of the other two edges at its parent when that parent has three links. None at the root."""
    keys = [None] * S.N
    for v in range(S.N):
        if v == S.root:
            continue
        lo, hi = int(S.lo[v]), int(S.hi[v])
        lo, hi = lo - (lo > x), hi - (hi > x)                  # the others' numbering skips x
        if lo == 0 and hi > 0:
            lo, hi = hi, S.n - 1                               # the other side
        keys[v] = (lo, hi) if hi > lo else (0, 0)
    own = int(S.leaf_node[x])
    u = int(S.parent[own])
    if S.links[u] == 3:
        keys[own] = next(keys[w] for w in range(S.N) if w != own and S.parent[w] == u)
    return keys


def path(S, a, b):
    """nodes on the path from a to b, both inclusive"""
    left, right = [a], [b]
    while left[-1] != right[-1]:
        if S.depth[left[-1]] >= S.depth[right[-1]]:
            left.append(int(S.parent[left[-1]]))
        else:
            right.append(int(S.parent[right[-1]]))
    return left + right[-2::-1]


def columns(ref, taxa, sc):
    """the columns of --place-taxa for the listed taxa (lookup ids) and their rows of scores, in COLUMNS order"""
    S = Shape(ref)
    sc = np.asarray(sc, dtype=np.int64).reshape(len(taxa), S.N)
    out = {name: [] for name in COLUMNS}
    nodes = [v for v in range(S.N) if v != S.root]
    for row, x in zip(sc, taxa):
        x = int(x)
        keys = position_keys(S, x)
        own = int(S.leaf_node[x])
        current, best = int(row[own]), int(row[nodes].max())
        members = {}
        for v in nodes:
            members.setdefault(keys[v], []).append(v)
        top = {keys[v] for v in nodes if row[v] == best}
        for k in top:
            assert all(row[v] == best for v in members[k])      # one position, one score
        pick = keys[own] if current == best else min(top, key=lambda k: min(members[k]))
        node = min(members[pick])
        if pick == keys[own]:
            dist = 0
        else:
            u = int(S.parent[own])
            near = min((path(S, u, node), path(S, u, int(S.parent[node]))), key=len)
            dist = sum(1 for w in near if S.links[w] - (w == u) >= 3)
        for name, val in zip(COLUMNS, (x, ref.names[x], current, best, best - current, len(top), node, int(S.lo[node]), int(S.hi[node]), dist)):
            out[name].append(val)
    return {k: (v if k == "name" else np.array(v, dtype=np.int64)) for k, v in out.items()}


def brute_scores(ref_newick, names, table, x):
    """{position key: score} of taxon x (lookup id) re-inserted on every edge of the reference tree pruned of x; keys as
    position_keys; the position with all others on one side is not an edge of the pruned tree and is left out"""
    n = len(names)
    table = np.asarray(table).reshape(-1, 3).astype(np.int64)
    holds_x = (np.array(bruteforce.rank_order_quads(n), dtype=np.int64).reshape(-1, 4) == x).any(axis=1)
    others = [i for i in range(n) if i != x]
    renum = {names[i]: k for k, i in enumerate(others)}
    pruned = newick.prune(newick.parse_tree(ref_newick), [names[x]])
    out = {}
    for w in newick.preorder(pruned)[1:]:
        below = sorted(renum[leaf.name] for leaf in newick.preorder(w) if leaf.is_leaf)
        side = below if 0 not in below else [k for k in range(n - 1) if k not in set(below)]
        if not side:
            continue
        assert side == list(range(side[0], side[-1] + 1))       # depth-first ids: an interval
        par, i = w.parent, w.parent.children.index(w)
        par.children[i] = newick.Node(children=[w, newick.Node(names[x])])
        shown = bruteforce.count_table(names, [newick.write(pruned)]).astype(np.int64)
        par.children[i] = w
        assert (shown[holds_x].sum(axis=1) <= 1).all()
        score = int((shown[holds_x] * table[holds_x]).sum())
        key = (side[0], side[-1] + 1)
        assert out.setdefault(key, score) == score
    return out


def caterpillar(names):
    return names[0] if len(names) == 1 else "(" + names[0] + "," + caterpillar(names[1:]) + ")"


def planted(true_at=3, ref_at=6):
    """twelve taxa on a caterpillar; in the reference tx hangs ref_at - true_at nodes away from where every evaluation tree has it"""
    others = [f"o{i}" for i in range(11)]
    true = caterpillar(others[:true_at] + ["tx"] + others[true_at:]) + ";"
    ref = caterpillar(others[:ref_at] + ["tx"] + others[ref_at:]) + ";"
    return ref, [true] * 7, set(others[true_at:]), ref_at - true_at
