"""Quartet placement of clades on the reference tree (qs_clade_placement) without a GPU.

clade_link_sums: the numpy model of qs_place_clade.hip on a downloaded count table and a flatten.RefTree. The clade below `node`
holds the lookup ids [lo, hi); the mask is "exactly one taxon of the 4-set in [lo, hi)", and that taxon's three counts go to the
links of the median node of the three others that lead towards its partners. The median is the deepest of the three pairwise LCAs
and the links come from leaf intervals (placement_model.Shape) -- not the kernel's case analysis.
constant_links: the closed form for a table whose every cell is t. columns: the columns of QuartetScores --place-clades, by
definition. brute_scores: the clade really pruned (newick.prune) and its subtree re-inserted on every edge of the pruned tree, the
displayed topologies read from bipartitions (bruteforce.count_table of the one tree).
"""
import numpy as np

import bruteforce
import placement_model as P
from quartetscores_amd import newick
from placement_model import Shape, _quad_columns, path

COLUMNS = ("clade", "node", "lo", "hi", "size", "current", "best", "gain", "n_best", "best_node", "best_lo", "best_hi", "distance")


def eligible(ref):
    """the inner non-root nodes with at least three taxa outside, in node order: the default list"""
    S = Shape(ref)
    return [v for v in range(S.N) if v != S.root and S.nchild[v] and S.n - (S.hi[v] - S.lo[v]) >= 3]


def clade_link_sums(table, ref, node):
    """(2 N,) int64: W_C of the clade below `node` from the whole count table"""
    S = Shape(ref)
    n, N = S.n, S.N
    lo, hi = int(S.lo[node]), int(S.hi[node])
    T = np.asarray(table).reshape(-1, 3)
    quads = _quad_columns(n)
    assert len(T) == len(quads[0])
    inside = [(q >= lo) & (q < hi) for q in quads]
    one = (inside[0].astype(np.int8) + inside[1] + inside[2] + inside[3]) == 1
    lca, depth, child_to = S.lca, S.depth, S.child_to.ravel()
    out = np.zeros(2 * N, dtype=np.int64)
    for k in range(4):
        rows = np.nonzero(one & inside[k])[0]
        o = [quads[j][rows].astype(np.int64) for j in range(4) if j != k]
        m = lca[o[0], o[1]]                                    # median of three leaves: the deepest of the pairwise LCAs
        for a, b in ((1, 2), (0, 2)):
            other = lca[o[a], o[b]]
            m = np.where(depth[other] > depth[m], other, m)
        for slot in range(3):
            t = quads[k ^ (slot + 1)][rows].astype(np.int64)   # the partner of the clade's taxon in the slot's pairing
            down = child_to[m * n + t]                         # the child of m that holds t, or -1: m's parent link
            np.add.at(out, np.where(down >= 0, down, N + m), T[rows, slot].astype(np.int64))
    return out


def link_sums(table, ref, nodes):
    return np.stack([clade_link_sums(table, ref, v) for v in nodes]) if len(nodes) else np.zeros((0, 2 * ref.n_nodes), dtype=np.int64)


def constant_links(ref, node, t, S=None):
    """W_C for a table whose every cell is t: a node m outside the clade with s_i taxa outside the clade in direction i gives
    link l the value |C| t s_l sum_{i<j; i,j != l} s_i s_j (the triples with median m: one taxon in l, two in two others)"""
    S = S or Shape(ref)
    lo, hi = int(S.lo[node]), int(S.hi[node])
    size, outside = hi - lo, S.n - (hi - lo)
    above = (S.lo <= lo) & (hi <= S.hi)                        # the clade's node and its ancestors
    below = (S.hi - S.lo) - np.where(above, size, 0)           # outside taxa below every node
    kids = [[] for _ in range(S.N)]
    for v in range(S.N):
        if S.parent[v] >= 0:
            kids[int(S.parent[v])].append(v)
    out = np.zeros(2 * S.N, dtype=np.int64)
    for m in range(S.N):
        if not kids[m] or (S.lo[m] >= lo and S.hi[m] <= hi):
            continue                                           # leaves and the clade's own nodes are no medians
        links = [(v, int(below[v])) for v in kids[m]] + [(S.N + m, outside - int(below[m]))]
        total, squares = sum(s for _, s in links), sum(s * s for _, s in links)
        for l, sl in links:
            out[l] = size * t * sl * (((total - sl) ** 2 - (squares - sl * sl)) // 2)
    return out


def position_keys(S, node):
    """per node v the position of the edge above it for the clade below `node`: the bipartition it induces among the taxa OUTSIDE
    the clade, as the id interval (in their numbering) of the side without the smallest of them; (0, 0) = all of them on one side.
    The clade's own edge takes the position of the other two edges at its parent when that parent has three links. None at the
    root and at the nodes strictly inside the clade (no positions)."""
    lo, hi = int(S.lo[node]), int(S.hi[node])
    size = hi - lo
    keys = [None] * S.N
    for v in range(S.N):
        if v == S.root or (v != node and S.lo[v] >= lo and S.hi[v] <= hi):
            continue
        a, b = int(S.lo[v]), int(S.hi[v])
        a, b = a - (size if a >= hi else 0), b - (size if b >= hi else 0)
        if a == 0 and b > 0:
            a, b = b, S.n - size                               # the other side
        keys[v] = (a, b) if b > a else (0, 0)
    u = int(S.parent[node])
    if S.links[u] == 3:
        keys[node] = next(keys[w] for w in range(S.N) if w != node and S.parent[w] == u)
    return keys


def columns(ref, nodes, sc):
    """the columns of --place-clades for the listed nodes and their rows of scores, in COLUMNS order"""
    S = Shape(ref)
    sc = np.asarray(sc, dtype=np.int64).reshape(len(nodes), S.N)
    out = {name: [] for name in COLUMNS}
    for k, (row, c) in enumerate(zip(sc, nodes)):
        c = int(c)
        keys = position_keys(S, c)
        edges = [v for v in range(S.N) if keys[v] is not None]
        current, best = int(row[c]), int(row[edges].max())
        members = {}
        for v in edges:
            members.setdefault(keys[v], []).append(v)
        top = {keys[v] for v in edges if row[v] == best}
        for key in top:
            assert all(row[v] == best for v in members[key])    # one position, one score
        pick = keys[c] if current == best else min(top, key=lambda key: min(members[key]))
        node = min(members[pick])
        if pick == keys[c]:
            dist = 0
        else:
            u = int(S.parent[c])
            near = min((path(S, u, node), path(S, u, int(S.parent[node]))), key=len)
            dist = sum(1 for w in near if S.links[w] - (w == u) >= 3)
        vals = (k, c, int(S.lo[c]), int(S.hi[c]), int(S.hi[c] - S.lo[c]), current, best, best - current, len(top), node, int(S.lo[node]), int(S.hi[node]), dist)
        for name, val in zip(COLUMNS, vals):
            out[name].append(val)
    return {k: np.array(v, dtype=np.int64) for k, v in out.items()}


def _copy(x):
    y = newick.Node(x.name, x.length, [_copy(k) for k in x.children])
    for k in y.children:
        k.parent = y
    return y


def brute_scores(ref, table, node):
    """({position key: score}, rest) of the clade below `node` re-inserted, unchanged inside, on every edge of the reference tree
    pruned of it. score = the part of the total quartet score from the 4-sets with exactly one taxon of the clade, rest = the
    other part, asserted to be the same at every position and in the reference tree itself. Keys as position_keys; the position
    with all outside taxa on one side is not an edge of the pruned tree and is left out."""
    S = Shape(ref)
    n, names = S.n, ref.names
    lo, hi = int(S.lo[node]), int(S.hi[node])
    table = np.asarray(table).reshape(-1, 3).astype(np.int64)
    quads = np.array(bruteforce.rank_order_quads(n), dtype=np.int64).reshape(-1, 4)
    one = ((quads >= lo) & (quads < hi)).sum(axis=1) == 1
    others = [i for i in range(n) if not lo <= i < hi]
    renum = {names[i]: k for k, i in enumerate(others)}
    clade = _copy(ref.nodes[node])
    pruned = newick.prune(ref.root, [names[i] for i in range(lo, hi)])
    shown = bruteforce.count_table(names, [newick.write(ref.root)]).astype(np.int64)
    rest = int((shown[~one] * table[~one]).sum())
    out = {}
    for w in newick.preorder(pruned)[1:]:
        below = sorted(renum[leaf.name] for leaf in newick.preorder(w) if leaf.is_leaf)
        side = below if 0 not in below else [k for k in range(len(others)) if k not in set(below)]
        if not side:
            continue
        assert side == list(range(side[0], side[-1] + 1))       # depth-first ids: an interval
        par, i = w.parent, w.parent.children.index(w)
        par.children[i] = newick.Node(children=[w, clade])
        shown = bruteforce.count_table(names, [newick.write(pruned)]).astype(np.int64)
        par.children[i] = w
        assert (shown.sum(axis=1) <= 1).all()
        assert int((shown[~one] * table[~one]).sum()) == rest   # what does not hold exactly one taxon of the clade does not see the move
        score = int((shown[one] * table[one]).sum())
        key = (side[0], side[-1] + 1)
        assert out.setdefault(key, score) == score
    return out, rest


def planted(true_at=3, ref_at=6):
    """eleven taxa on a caterpillar and the clade (ca,(cb,cc)); in the reference the clade hangs ref_at - true_at nodes away from
    where every evaluation tree has it"""
    others = [f"o{i}" for i in range(11)]
    clade = "(ca,(cb,cc))"
    true = P.caterpillar(others[:true_at] + [clade] + others[true_at:]) + ";"
    ref = P.caterpillar(others[:ref_at] + [clade] + others[ref_at:]) + ";"
    return ref, [true] * 7, set(others[true_at:]), ref_at - true_at
