"""Per-tree quartet support of every reference internode (qs_tree_branch_support) without a GPU.

model_counts: the (n_nodes, 4) words (present, q1, q2, q3) of one flattened evaluation tree from closed forms over pairs (reference
internode, tree node); no 4-set is enumerated. The groups at the two ends of an internode are id intervals (items()), a tree node's
links are id sets, and everything below is a sum over the links c of products of four intersections with P_t:
  xs_c  the lower end's groups in front of group i      ya_c  group i of the lower end
  zs_c  upper-end taxa in front (by id) of piece j      wg_c  piece j of the upper end, never in zs's group
A 4-set x < y (lower end), z < w (upper end) that t shows as pq|rs is claimed at ONE node: where p and q lie in different links and r, s
together in a third. With S. the sums over the links and P.. the sums of products of two, A = sum ya zs wg, B = sum xs zs wg,
C = sum xs ya wg, Q = sum xs ya zs wg:
  xy|zw  P_zw (S_x S_y - P_xy) - S_x A - S_y B + 2 Q      (claimed where x, y part)
  xz|yw  P_yw (S_x S_z - P_xz) - S_x A - S_z C + 2 Q      (claimed where x, z part)
  xw|yz  P_xw (S_y S_z - P_yz) - S_y B - S_z C + 2 Q      (claimed where y, z part)
In the multifurcating frame q2 = xz|yw and q3 = xw|yz with z < w by id; in the node-pair frame of a bifurcating reference the two
exchange where z and w lie on opposite sides of the lower end's interval (then xw|yz is the pairing that crosses in the cyclic order).
brute_rows: the same words from a per-4-set table of the tree alone, as branch_taxon_model.model(...)[1] sums them (above 30 taxa the
table holds only the plan's 4-sets, from bruteforce.quartet_counts_for: the same split test on packed bits).
REF_KINDS, mixed_trees (of tests/test_gpu_tree_agreement.py): the reference kinds and evaluation-tree shapes the CPU and GPU tests share.
"""
import numpy as np

import branch_taxon_model as BM
import bruteforce
from quartetscores_amd import flatten, newick
from test_gpu_tree_agreement import mixed_trees  # noqa: F401  (the evaluation-tree shapes: binary, collapsed up to a star, dropout below 4 taxa, rooted)

REF_KINDS = {"binary": {}, "multifurcating": {"collapse": 0.4}, "rooted": {"rooted": True}, "star": {"collapse": 1.0}}


def items(ref):
    """per internode (v, w) of branch_taxon_model.internodes: (v, lower boundaries b_0 < ... < b_p, [(wg, zs, opposite)]), wg and zs
    id intervals [s, e) of the upper end; (upper groups as lists of intervals) for the `present` word"""
    parent, _, lo, hi, kids, root = BM.tree_arrays(ref)
    n = len(ref.leaf_node)
    out = []
    for v, w in BM.internodes(ref):
        b = [int(lo[k]) for k in kids[v]] + [int(hi[v])]
        lo_v, hi_v, lo_w, hi_w = b[0], b[-1], int(lo[w]), int(hi[w])
        merged = int(parent[v]) != w                        # the two children of a degree-2 root
        par = parent[w] >= 0 and not merged
        zl = 0 if par else lo_w
        its, groups = [], []
        for k in kids[w]:
            if k == v:
                continue
            s, e = int(lo[k]), int(hi[k])
            groups.append([(s, e)])
            if e <= lo_v:
                its.append(((s, e), (zl, s), False))
            else:
                its.append(((s, e), (hi_v, s), False))
                its.append(((s, e), (zl, lo_v), True))
        if par:
            groups.append([(0, lo_w), (hi_w, n)])
            its.append(((hi_w, n), (hi_v, hi_w), False))
            its.append(((hi_w, n), (lo_w, lo_v), True))
        its = [(wg, zs, opp) for wg, zs, opp in its if wg[1] > wg[0] and zs[1] > zs[0]]
        out.append((v, b, its, groups))
    return out


def model_counts(ref, leaf_ids, node_ranges, the_items=None):
    N, n = len(ref.parent), len(ref.leaf_node)
    out = np.zeros((N, 4), dtype=np.int64)
    L = len(leaf_ids)
    if L < 4:
        return out
    ids = np.asarray(leaf_ids, dtype=np.int64)
    pres = np.zeros(n + 1, dtype=np.int64)
    pres[ids + 1] = 1
    pres = np.cumsum(pres)
    # per tree node: (links, n + 1) prefix counts of every link's ids
    prefs = []
    for rl in node_ranges:
        P = np.zeros((len(rl), n + 1), dtype=np.int64)
        for c, (s, e) in enumerate(rl):
            P[c, ids[[(s + i) % L for i in range((e - s) % L)]] + 1] = 1
        prefs.append(np.cumsum(P, axis=1))
    frame0 = BM.is_bifurcating(ref)
    cnt = lambda P, iv: P[..., iv[1]] - P[..., iv[0]]
    pairs = lambda sizes: (sum(sizes) ** 2 - sum(s * s for s in sizes)) // 2
    for v, b, its, groups in (items(ref) if the_items is None else the_items):
        low = pairs([int(cnt(pres, (b[i], b[i + 1]))) for i in range(len(b) - 1)])
        up = pairs([sum(int(cnt(pres, iv)) for iv in g) for g in groups])
        q = np.zeros(3, dtype=np.int64)
        for P in prefs:
            for i in range(1, len(b) - 1):
                xs, ya = cnt(P, (b[0], b[i])), cnt(P, (b[i], b[i + 1]))
                Sx, Sy, Pxy = xs.sum(), ya.sum(), (xs * ya).sum()
                if Sx == 0 or Sy == 0:
                    continue
                for wg_iv, zs_iv, opp in its:
                    wg, zs = cnt(P, wg_iv), cnt(P, zs_iv)
                    Sz = zs.sum()
                    A, B, C, Q = (ya * zs * wg).sum(), (xs * zs * wg).sum(), (xs * ya * wg).sum(), (xs * ya * zs * wg).sum()
                    t1 = (zs * wg).sum() * (Sx * Sy - Pxy) - Sx * A - Sy * B + 2 * Q
                    tc = (ya * wg).sum() * (Sx * Sz - (xs * zs).sum()) - Sx * A - Sz * C + 2 * Q
                    tn = (xs * wg).sum() * (Sy * Sz - (ya * zs).sum()) - Sy * B - Sz * C + 2 * Q
                    if frame0 and opp:
                        tc, tn = tn, tc
                    q += (t1, tc, tn)
        out[v] = (low * up, q[0], q[1], q[2])
    return out


def model_tree(ref, newick_text, recentre=True, the_items=None):
    leaf_ids, _, node_ranges = flatten.flatten_tree(newick.parse_tree(newick_text), ref.name_to_id, recentre)
    return model_counts(ref, leaf_ids, node_ranges, the_items)


def brute_rows(ref, tree_newick, the_plan=None, table=None):
    """(n_nodes, 4) from the per-4-set table of the tree alone: what branch_taxon_model.model(table, ref)[1] sums, with word 0 restricted
    to the 4-sets inside the tree's taxon set"""
    n, N = len(ref.leaf_node), len(ref.parent)
    quads, ranks, child, second, cols = BM.plan(ref) if the_plan is None else the_plan
    if table is None:
        if n <= 30:
            table = bruteforce.count_table(ref.names, [tree_newick])
        else:
            table = bruteforce.quartet_counts_for([tree_newick], ref.names, quads)
            ranks = np.arange(len(quads))
    t = np.asarray(table).reshape(-1, 3).astype(np.int64)[ranks]
    _, allv = bruteforce.splits_of(bruteforce.parse_newick(tree_newick), ref.name_to_id)
    inside = allv[quads].all(axis=1).astype(np.int64) if len(quads) else np.zeros(0, dtype=np.int64)
    idx = np.arange(len(t))
    words = [inside] + [t[idx, cols[:, k]] for k in range(3)]
    out = np.zeros((N, 4), dtype=np.int64)
    dup = second >= 0
    for k, w in enumerate(words):
        out[:, k] = np.bincount(child, weights=w, minlength=N).astype(np.int64)
        if dup.any():
            out[:, k] += np.bincount(second[dup], weights=w[dup], minlength=N).astype(np.int64)
    return out
