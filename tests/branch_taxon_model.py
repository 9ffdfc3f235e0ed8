"""Per-branch quartet sums through every taxon (qs_branch_taxon_support) without a GPU.

model: rows (n, n_nodes, 4) and totals (n_nodes, 4) from a downloaded count table and a flatten.RefTree, by walking the 4-sets in rank
order (taxon_model.quads_in_rank_order): topology and the two junction nodes of a 4-set a<b<c<d from the LCAs of its three adjacent
pairs as classify() in qs_score.hip decides them, (q1, q2, q3) in the order qs_score uses without flags; a 4-set counts for the
internode between its junctions if one is the other's parent -- or if they are the two children of a degree-2 root, whose entries
both get it. plan() is the part that depends on the tree alone, so that tests share it between tables.
closed_form_quartets: the number of 4-sets around every internode from the link sizes at its two ends.
columns: the lines of QuartetScores --drop-one, written down per line.
cyclic_labels: four links of an internode as a quad hypothesis of tests/group_model.py, labelled in the cyclic order of the ids.
"""
import math

import numpy as np

from taxon_model import lca_depths, quads_in_rank_order

FIELDS = ("quartets", "q1", "q2", "q3")


def tree_arrays(ref):
    """parent, depth, [lo, hi) per node, children per node ordered by lo, root (kept with the tree they were derived from)"""
    kept = getattr(ref, "_branch_taxon_arrays", None)
    if kept is not None and kept[0] is ref.parent and kept[1] is ref.leaf_node:
        return kept[2]
    parent = np.asarray(ref.parent, dtype=np.int64)
    N, n = len(parent), len(ref.leaf_node)
    depth = np.zeros(N, dtype=np.int64)
    for v in range(N):
        x = v
        while parent[x] >= 0:
            x = parent[x]
            depth[v] += 1
    lo, hi = np.full(N, n, dtype=np.int64), np.zeros(N, dtype=np.int64)
    for i in range(n):
        v = int(ref.leaf_node[i])
        while v >= 0:
            lo[v], hi[v] = min(lo[v], i), max(hi[v], i + 1)
            v = int(parent[v])
    kids = [sorted(np.nonzero(parent == v)[0].tolist(), key=lambda k: lo[k]) for v in range(N)]
    out = parent, depth, lo, hi, kids, int(np.nonzero(parent < 0)[0][0])
    ref._branch_taxon_arrays = (ref.parent, ref.leaf_node, out)
    return out


def is_bifurcating(ref):
    """the reference's test: the largest (degree - 1) over all nodes is 2"""
    parent, _, _, _, kids, _ = tree_arrays(ref)
    return max(len(kids[v]) + (1 if parent[v] >= 0 else 0) - 1 for v in range(len(parent))) == 2


def lca_nodes(ref):
    """(n, n) node of the LCA of two leaves by lookup id: among the LCAs of the adjacent pairs between them the shallowest one"""
    parent, depth, _, _, _, _ = tree_arrays(ref)
    n, N = len(ref.leaf_node), len(parent)
    adj = np.zeros(max(n - 1, 0), dtype=np.int64)
    for i in range(n - 1):
        x, y = int(ref.leaf_node[i]), int(ref.leaf_node[i + 1])
        while x != y:
            if depth[x] >= depth[y]:
                x = int(parent[x])
            else:
                y = int(parent[y])
        adj[i] = depth[x] * N + x
    L = np.zeros((n, n), dtype=np.int64)
    for i in range(n - 1):
        L[i, i + 1:] = np.minimum.accumulate(adj[i:]) % N
    return L + L.T


def internodes(ref):
    """[(child node v, other end w)] in node order: both ends inner nodes, w = v's parent -- or, under a degree-2 root, the root's other
    child (then the edge appears at both children)"""
    parent, _, _, _, kids, root = tree_arrays(ref)
    out = []
    for v in range(len(parent)):
        if v == root or not kids[v]:
            continue
        u = int(parent[v])
        if u == root and len(kids[u]) == 2:
            w = kids[u][1] if kids[u][0] == v else kids[u][0]
            if kids[w]:
                out.append((v, w))
        else:
            out.append((v, u))
    return out


def links_at(ref, end, away):
    """the id sets (boolean rows over the taxa) behind the links of node `end` other than the one towards node `away`"""
    parent, _, lo, hi, kids, root = tree_arrays(ref)
    n = len(ref.leaf_node)
    rows = []
    for k in kids[end]:
        if k != away:
            m = np.zeros(n, dtype=bool)
            m[lo[k]:hi[k]] = True
            rows.append(m)
    through_root = away is not None and parent[end] >= 0 and parent[away] == parent[end]   # (the two children of a degree-2 root)
    if parent[end] >= 0 and int(parent[end]) != away and not through_root:
        m = np.ones(n, dtype=bool)
        m[lo[end]:hi[end]] = False
        rows.append(m)
    return rows


def cyclic_labels(n, groups):
    """label row 1..4 for four disjoint id sets, two ends x two links, in the cyclic order of their first id after the largest gap
    -- the first two labels at one end, the last two at the other"""
    (a, b), (c, d) = groups
    row = np.zeros(n, dtype=np.uint8)
    # walk the ids from the first taxon of a's end; a set whose ids wrap around n - 1 -> 0 (a parent's side) is one cyclic interval
    def start(m):
        idx = np.nonzero(m)[0]
        wraps = m[0] and m[n - 1] and not m.all()
        return int(idx[np.nonzero(np.diff(idx) > 1)[0][-1] + 1]) if wraps and (np.diff(idx) > 1).any() else int(idx[0])
    order = sorted([(start(a), 0, a), (start(b), 0, b), (start(c), 1, c), (start(d), 1, d)], key=lambda t: t[0])
    # rotate so that the two sets of one end come first
    while not (order[0][1] == order[1][1]):
        order = order[1:] + order[:1]
    for label, (_, _, m) in enumerate(order, start=1):
        row[m] = label
    return row


def closed_form_quartets(ref):
    """(n_nodes,) the number of 4-sets around the internode above every node (0 where there is none): pairs of different links at one
    end times pairs of different links at the other"""
    out = np.zeros(len(ref.parent), dtype=np.int64)
    for v, w in internodes(ref):
        e2 = []
        for end, away in ((v, w), (w, v)):
            sizes = [int(m.sum()) for m in links_at(ref, end, away)]
            e2.append((sum(sizes) ** 2 - sum(s * s for s in sizes)) // 2)
        out[v] = e2[0] * e2[1]
    return out


def plan(ref):
    """what the tree alone decides: (quads (m, 4) ids of the counted 4-sets in rank order, their ranks, the child node of their
    internode, -1 or the second node under a degree-2 root, the column of the table that is q1, q2, q3)"""
    n = len(ref.leaf_node)
    parent, depth, _, _, kids, root = tree_arrays(ref)
    quads = quads_in_rank_order(n)
    L = lca_nodes(ref)
    a, b, c, d = quads.T
    n01, n12, n23 = L[a, b], L[b, c], L[c, d]
    d01, d12, d23 = depth[n01], depth[n12], depth[n23]
    assert (lca_depths(ref)[a, b] == d01).all()
    mx = np.maximum(d01, d23)
    ab, ad = d12 < mx, d12 > mx
    j1 = np.where(ab, np.where(d01 > d12, n01, n12), n12)
    j2 = np.where(ab, np.where(d23 > d12, n23, n12), np.where(d01 >= d23, n01, n23))
    child = np.where(parent[j1] == j2, j1, np.where(parent[j2] == j1, j2, -1))
    second = np.full(len(quads), -1, dtype=np.int64)
    if len(kids[root]) == 2:
        r1, r2 = kids[root]
        through = ((j1 == r1) & (j2 == r2)) | ((j1 == r2) & (j2 == r1))
        child = np.where(through, r1, child)
        second = np.where(through, r2, second)
    keep = (ab | ad) & (child >= 0)
    frame1 = not is_bifurcating(ref)
    # ab|cd: (n0, n1, n2); ad|bc: (n2, n1, n0) in the node-pair frame of a bifurcating tree, (n2, n0, n1) otherwise
    cols = np.where(ab[:, None], np.array([0, 1, 2]), np.array([2, 0, 1] if frame1 else [2, 1, 0]))
    return quads[keep], np.nonzero(keep)[0], child[keep], second[keep], cols[keep]


def _exact_bincount(idx, w, size):
    """bincount with int64 weights of any size: in two halves that float64 sums exactly"""
    w = np.asarray(w, dtype=np.int64)
    assert len(w) < 2 ** 26
    lo = np.bincount(idx, weights=(w & 0xFFFFF).astype(np.float64), minlength=size).astype(np.int64)
    hi = np.bincount(idx, weights=(w >> 20).astype(np.float64), minlength=size).astype(np.int64)
    return lo + (hi << 20)


def model(table, ref, the_plan=None):
    """(rows (n, n_nodes, 4), totals (n_nodes, 4)) int64 from the whole count table"""
    n, N = len(ref.leaf_node), len(ref.parent)
    table = np.asarray(table).reshape(-1, 3).astype(np.int64)
    quads, ranks, child, second, cols = plan(ref) if the_plan is None else the_plan
    t = table[ranks]
    idx = np.arange(len(t))
    words = [np.ones(len(t), dtype=np.int64)] + [t[idx, cols[:, k]] for k in range(3)]
    rows = np.zeros((n, N, 4), dtype=np.int64)
    totals = np.zeros((N, 4), dtype=np.int64)
    dup = second >= 0
    for k, w in enumerate(words):
        totals[:, k] = _exact_bincount(child, w, N)
        if dup.any():
            totals[:, k] += _exact_bincount(second[dup], w[dup], N)
        for pos in range(4):
            rows[:, :, k] += _exact_bincount(quads[:, pos] * N + child, w, n * N).reshape(n, N)
            if dup.any():
                rows[:, :, k] += _exact_bincount(quads[dup, pos] * N + second[dup], w[dup], n * N).reshape(n, N)
    return rows, totals


def log_score(q1, q2, q3):
    """QuartetScoreComputer.hpp:135-159"""
    if q1 == 0 and q2 == 0 and q3 == 0:
        return 0.0
    s = q1 + q2 + q3
    qic = 1.0
    for q in (q1, q2, q3):
        if q:
            qic += (q / s) * math.log(q / s) / math.log(3)
    return -qic if (q1 < q2 or q1 < q3) else qic


def columns(ref, taxa, rows, totals):
    """the lines of --drop-one as tuples (taxon, name, node, lo, hi, group, quartets, q1, q2, q3, qpic, qpic_without, delta), the three
    scores as the CLI prints them; rows = one per entry of taxa"""
    parent, _, lo, hi, kids, root = tree_arrays(ref)
    deg2 = len(kids[root]) == 2
    lines = []
    for k, x in enumerate(taxa):
        for v, w in internodes(ref):
            if deg2 and int(parent[v]) == root and v != kids[root][0]:
                continue                                     # the edge through the root: once, at the first child
            group = [int(m.sum()) for end, away in ((v, w), (w, v)) for m in links_at(ref, end, away) if m[x]]
            assert len(group) == 1
            r, t = [int(z) for z in rows[k][v]], [int(z) for z in totals[v]]
            qpic = log_score(*t[1:])
            left = t[0] - r[0]
            without = log_score(t[1] - r[1], t[2] - r[2], t[3] - r[3]) if left else math.nan
            fmt = lambda z: "nan" if math.isnan(z) else "%.6f" % z
            lines.append((x, ref.names[x], v, int(lo[v]), int(hi[v]), group[0], r[0], r[1], r[2], r[3], fmt(qpic), fmt(without), fmt(without - qpic)))
    return lines
