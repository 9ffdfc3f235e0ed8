"""Per-tree quartet agreement of every taxon (qs_tree_taxon_agreement): a numpy model of the node-pair sums with their difference
arrays, a per-4-set brute force, and the LDS plan of the kernel restated on the host. No GPU.

For evaluation tree t with taxon set P_t (L = |P_t|), the reference restricted to P_t and a taxon x of P_t the four words
(concordant, discordant, resolved_eval, resolved_ref) count the C(L-1,3) 4-sets of P_t that hold x. A resolved 4-set {x,b,c,d} shown
as xb|cd is claimed at one node of a tree, the junction on x's side: x, b and {c,d} lie behind three different links. So for a node
u of t (links i) and a reference node v (groups j: child intervals and, where it has one, the rest), with I[i][j] = |link i & group j
& P_t|, a leaf in cell (i1, j1) receives

    Wc[i1][j1] = sum  I[i2][j2] c2(I[i3][j3])              i2, i3 distinct from i1 and each other; j2, j3 likewise
    Wd[i1][j1] = sum  I[i2][j3] I[i3][j2] I[i3][j3]

and its words are the sums over all pairs (u, v). pair_w_definition evaluates these sums as they stand; pair_w is the form the kernel
uses, with the sums over i2 and j2 done from the link and group sizes. The values do not go to the leaves directly: as in the kernel,
every reference node adds the differences of its groups' values at its child boundaries into a difference array over the ids, one per
link of u and per word, a prefix sum follows, and a leaf of link i reads the entry of its own id (words). resolved_ref is one such
array per tree, resolved_eval a constant per link:

    res[i1] = sum over i2 != i1 of S[i2] (sum over i3 not in {i1, i2} of c2(S[i3]))

brute_words enumerates the 4-sets with bruteforce.quartet_counts_for and shares no code with the model.

plan(n) is tree_taxa_plan of qs_tree_taxa.hip, rounds() the walk of a block's nodes it shares with qs_agree.hip (tests/agree_rounds.py
restates that one for its plan); the tree shapes come from agree_rounds.
"""
import itertools

import numpy as np

import agree_rounds
import bruteforce
from agreement_model import c2, ref_links
from quartetscores_amd import flatten, newick

# ---- the plan of the kernel ------------------------------------------------------------------------------------------------------

LDS_BYTES = 65536      # kTaxaLdsBytes
FLIGHT = 3             # kTaxaFlight: links of a node whose two difference arrays are in LDS at once
THREADS, OWN = 256, 6  # kTaxaThreads, kTaxaOwn: a lane owns at most OWN leaf positions
MIN_CAP = 12           # kTaxaMinCap
NODES = 64             # kTaxaNodes
MAX_CAP = 3 * NODES    # kTaxaMaxCap: the links of a block of binary nodes


def plan(n):
    """(W, cap, nb, lds_bytes) of a launch for n taxa, or None where the kernel refuses n"""
    W = n // 32 + 1
    diff = FLIGHT * 2 * (n + 1) * 8
    if n > THREADS * OWN or diff + (1 + MIN_CAP) * W * 8 > LDS_BYTES:
        return None
    cap = min(MAX_CAP, (LDS_BYTES - diff) // 8 // W - 1)
    return W, cap, NODES, diff + (1 + cap) * W * 8


def max_taxa():
    n = 4
    while plan(n + 1) is not None:
        n += 1
    return n


def rounds(batch, n):
    """per tree, per block of its inner nodes: the rounds as agree_rounds.rounds gives them, for this kernel's plan"""
    _, cap, nb, _ = plan(n)
    node_off, rng_off = batch.node_off.astype(np.int64), batch.rng_off.astype(np.int64)
    out = []
    for t in range(batch.n_trees):
        blocks = []
        if int(batch.leaf_off[t + 1]) - int(batch.leaf_off[t]) >= 4:
            for v_lo in range(int(node_off[t]), int(node_off[t + 1]), nb):
                v_hi = min(v_lo + nb, int(node_off[t + 1]))
                rl, v0 = [], v_lo
                while v0 < v_hi:
                    v1 = v0
                    while v1 < v_hi and rng_off[v1 + 1] - rng_off[v0] <= cap:
                        v1 += 1
                    rl.append(("S", v1 - v0) if v1 > v0 else ("U",))
                    v0 = max(v1, v0 + 1)
                blocks.append(rl)
        out.append(blocks)
    return out


# ---- the node-pair sums ----------------------------------------------------------------------------------------------------------

def _distinct3(k):
    """M[a][p][r] = 1 where a, p, r are pairwise different"""
    e = 1 - np.eye(k, dtype=np.int64)
    return e[:, :, None] * e[:, None, :] * e[None, :, :]


def pair_w_definition(I):
    """(Wc, Wd) of node pairs, I of shape (..., k, K): the sums of the definition as they stand"""
    I = np.asarray(I, dtype=np.int64)
    Mk, MK = _distinct3(I.shape[-2]), _distinct3(I.shape[-1])
    Wc = np.einsum("...pq,...rs,apr,bqs->...ab", I, c2(I), Mk, MK, optimize=True)
    Wd = np.einsum("...ps,...rq,...rs,apr,bqs->...ab", I, I, I, Mk, MK, optimize=True)
    return Wc, Wd


def pair_w(I):
    """(Wc, Wd) of node pairs, I of shape (..., k, K): the sums over i2 and j2 from the link sizes C and group sizes R,
        Wc[a][b] = sum over r != a, s != b of c2(I[r][s]) (N - C_a - C_r - R_b - R_s + I[a][b] + I[a][s] + I[r][b] + I[r][s])
        Wd[a][b] = sum over r != a, s != b of I[r][s] (R_s - I[a][s] - I[r][s]) (C_r - I[r][b] - I[r][s])"""
    I = np.asarray(I, dtype=np.int64)
    k, K = I.shape[-2:]
    lead = I.shape[:-2]
    I = I.reshape((-1, k, K))
    Wc, Wd = np.zeros_like(I), np.zeros_like(I)
    off = ((1 - np.eye(k, dtype=np.int64))[:, None, :, None] * (1 - np.eye(K, dtype=np.int64))[None, :, None, :])[None]   # [a][b][r][s]
    step = max(1, (1 << 21) // (k * K * k * K))
    for g in range(0, len(I), step):
        J = I[g:g + step]
        C, R, N = J.sum(2), J.sum(1), J.sum((1, 2))
        Iab, Ias, Irs = J[:, :, :, None, None], J[:, :, None, None, :], J[:, None, None, :, :]   # axes [.][a][b][r][s]
        Irb = J.transpose(0, 2, 1)[:, None, :, :, None]
        Ca, Cr, Rb, Rs = C[:, :, None, None, None], C[:, None, None, :, None], R[:, None, :, None, None], R[:, None, None, None, :]
        Wc[g:g + step] = (off * c2(Irs) * (N[:, None, None, None, None] - Ca - Cr - Rb - Rs + Iab + Ias + Irb + Irs)).sum((3, 4))
        Wd[g:g + step] = (off * Irs * (Rs - Ias - Irs) * (Cr - Irb - Irs)).sum((3, 4))
    return Wc.reshape(lead + (k, K)), Wd.reshape(lead + (k, K))


def node_resolved(S):
    """res[i1] of nodes from their link sizes S (..., k)"""
    S = np.asarray(S, dtype=np.int64)
    Q = c2(S)
    e = 1 - np.eye(S.shape[-1], dtype=np.int64)
    return (e * S[..., None, :] * (Q.sum(-1)[..., None, None] - Q[..., :, None] - Q[..., None, :])).sum(-1)


def _scatter(diff, B, has_parent, V):
    """reference nodes of one shape (child boundaries B (nodes, m + 1), with or without a parent link) add their groups' values V
    (nodes, ..., K) to the difference arrays diff (n + 1, ...): the rest (group m; 0 without a parent link) from id 0 on, and their
    differences at the child boundaries b_0 .. b_m"""
    m = B.shape[1] - 1
    rest = V[..., m] if has_parent else np.zeros_like(V[..., 0])
    diff[0] += rest.sum(0)
    prev = rest
    for j in range(m):
        np.add.at(diff, B[:, j], V[..., j] - prev)
        prev = V[..., j]
    np.add.at(diff, B[:, m], rest - prev)


def words(ref: flatten.RefTree, leaf_ids, node_ranges, w_of_pairs=pair_w):
    """int64 (n_taxa, 4): the four words of every taxon from the flattened evaluation tree (flatten.flatten_tree)"""
    n, L = ref.n_taxa, len(leaf_ids)
    out = np.zeros((n, 4), dtype=np.int64)
    if L < 4:
        return out
    ids = np.asarray(leaf_ids, dtype=np.int64)
    present = np.zeros(n, dtype=np.int64)
    present[ids] = 1
    pre = np.concatenate([[0], np.cumsum(present)])
    # reference nodes of one shape (children, parent link or none) go together
    shapes = {}
    for bnd, has_parent in ref_links(ref):
        shapes.setdefault((len(bnd) - 1, has_parent), []).append(bnd)
    shapes = {key: np.asarray(bnds, dtype=np.int64) for key, bnds in shapes.items()}

    def cells(P):
        """I (nodes, links, groups) of every shape from the prefix counts P (links, n + 1) of the links"""
        for (m, has_parent), B in shapes.items():
            I = (P[:, B[:, 1:]] - P[:, B[:, :-1]]).transpose(1, 0, 2)
            if has_parent:
                I = np.concatenate([I, (P[:, -1][None, :] - I.sum(2))[:, :, None]], axis=2)
            yield B, has_parent, I

    # resolved_ref: one difference array
    diff = np.zeros(n + 1, dtype=np.int64)
    for B, has_parent, I in cells(pre[None, :]):
        _scatter(diff, B, has_parent, node_resolved(I[:, 0, :]))
    out[ids, 3] = np.cumsum(diff)[ids]
    for rl in node_ranges:
        k = len(rl)
        pos = [[(s + i) % L for i in range((e - s) % L)] for (s, e) in rl]
        member = np.zeros((k, n), dtype=np.int64)
        for i, p in enumerate(pos):
            member[i, ids[p]] = 1
        P = np.concatenate([np.zeros((k, 1), dtype=np.int64), np.cumsum(member, axis=1)], axis=1)   # P[i][x] = ids < x behind link i
        res_e = node_resolved(P[:, -1])
        diff = np.zeros((n + 1, 2, k), dtype=np.int64)                              # per id: word, link
        for B, has_parent, I in cells(P):
            _scatter(diff, B, has_parent, np.stack(w_of_pairs(I), axis=1))          # (nodes, word, link, group)
        value = np.cumsum(diff, axis=0)
        for i, p in enumerate(pos):
            x = ids[p]
            out[x, 0] += value[x, 0, i]
            out[x, 1] += value[x, 1, i]
            out[x, 2] += res_e[i]
    return out


def model_tree(ref: flatten.RefTree, newick_text, recentre=True, w_of_pairs=pair_w):
    leaf_ids, _, node_ranges = flatten.flatten_tree(newick.parse_tree(newick_text), ref.name_to_id, recentre)
    return words(ref, leaf_ids, node_ranges, w_of_pairs)


def model_trees(ref, trees):
    return np.array([model_tree(ref, t) for t in trees]).reshape(len(trees), ref.n_taxa, 4)


def brute_words(ref_newick, names, tree_newick):
    """int64 (len(names), 4): the four words of every taxon, accumulated 4-set by 4-set"""
    out = np.zeros((len(names), 4), dtype=np.int64)
    _, allv = bruteforce.splits_of(bruteforce.parse_newick(tree_newick), {nm: i for i, nm in enumerate(names)})
    taxa = [int(x) for x in np.nonzero(allv)[0]]
    if len(taxa) < 4:
        return out
    quads = np.array(list(itertools.combinations(taxa, 4)), dtype=np.int64)
    te = bruteforce.quartet_counts_for([tree_newick], names, quads) > 0
    tr = bruteforce.quartet_counts_for([ref_newick], names, quads) > 0
    res_e, res_r, conc = te.any(1), tr.any(1), (te & tr).any(1)
    for k, hit in enumerate((conc, res_e & res_r & ~conc, res_e, res_r)):
        np.add.at(out[:, k], quads[hit].ravel(), 1)
    return out


def star_resolved_ref(ref: flatten.RefTree, taxa):
    """resolved_ref of every taxon of `taxa` from the closed form alone: the restricted reference's nodes, res[] of each, added to the
    taxa of each group directly (no difference array)"""
    n = ref.n_taxa
    present = np.zeros(n, dtype=np.int64)
    present[list(taxa)] = 1
    out = np.zeros(n, dtype=np.int64)
    for bnd, has_parent in ref_links(ref):
        groups = [np.arange(bnd[j], bnd[j + 1]) for j in range(len(bnd) - 1)]
        if has_parent:
            groups.append(np.concatenate([np.arange(0, bnd[0]), np.arange(bnd[-1], n)]))
        res = node_resolved([int(present[g].sum()) for g in groups])
        for g, r in zip(groups, res):
            out[g] += r * present[g]
    return out


def gains(tree_words, ids):
    """lookup id -> gain of QuartetScores --tree-taxa for the taxa `ids` of one tree from its words (n, 4): the tree's concordance
    over the 4-sets that do not hold the taxon minus its concordance over all (nan where either has no resolved 4-set)"""
    w = np.asarray(tree_words, dtype=np.int64)
    conc, disc = int(w[:, 0].sum()) // 4, int(w[:, 1].sum()) // 4
    ratio = lambda num, den: num / den if den else float("nan")
    return {int(x): ratio(conc - int(w[x, 0]), conc - int(w[x, 0]) + disc - int(w[x, 1])) - ratio(conc, conc + disc) for x in ids}


# ---- tree shapes -----------------------------------------------------------------------------------------------------------------

def ladder(names):
    t = names[0]
    for nm in names[1:]:
        t = f"({t},{nm})"
    return t + ";"


def star(names):
    return "(" + ",".join(names) + ");"


def regraft_far(tree_newick, name, rng):
    """the tree with the leaf `name` pruned and regrafted as the sister of a random leaf that is not its neighbour"""
    root = newick.parse_tree(tree_newick)

    def nested(x):
        return x.name if x.is_leaf else tuple(nested(c) for c in x.children)

    def prune(t):
        if not isinstance(t, tuple):
            return None if t == name else t
        kids = [k for k in (prune(c) for c in t) if k is not None]
        return kids[0] if len(kids) == 1 else tuple(kids)

    def leaves(t):
        return [t] if not isinstance(t, tuple) else [x for c in t for x in leaves(c)]

    def sister(t):   # the leaves that share the parent of `name`, or the leaves of its sister subtrees
        if not isinstance(t, tuple):
            return None
        if name in t:
            return [x for c in t if c != name for x in leaves(c)]
        for c in t:
            s = sister(c)
            if s is not None:
                return s
        return None

    def graft(t, at):
        if not isinstance(t, tuple):
            return (t, name) if t == at else t
        return tuple(graft(c, at) for c in t)

    full = nested(root)
    near = set(sister(full))
    far = [x for x in leaves(full) if x != name and x not in near]
    at = far[int(rng.integers(len(far)))]
    to_text = lambda t: "(" + ",".join(to_text(c) for c in t) + ")" if isinstance(t, tuple) else t
    return to_text(graft(prune(full), at)) + ";"


def plan_shapes(names):
    """name -> Newick text of two trees of 120 taxa spread over all len(names) ids, for a plan whose cap is below a binary block's 192 links (1100 taxa: 44):
    a hub of cap + 2 links, which gets no bitmaps, behind stored nodes of its block, and a fan tree whose blocks take several stored
    rounds. tests/test_tree_taxon_model.py checks the rounds, tests/test_gpu_tree_taxa.py runs the trees."""
    n = len(names)
    _, cap, _, _ = plan(n)
    assert cap < MAX_CAP
    g = np.random.default_rng
    return {"hub": hub_tree(spread_names(names, 120, g(n + 1)), 30, cap + 1, 8, g(n + 2)),
            "fans7": fan_tree(spread_names(names, 120, g(n + 3)), 7, g(n + 4))}


hub_tree, fan_tree, spread_names, names_of = agree_rounds.hub_tree, agree_rounds.fan_tree, agree_rounds.spread_names, agree_rounds.names_of
