"""The LDS plan and the round walk of the kernels that walk (reference or row-tree node, node of one evaluation tree) pairs --
tree_agree_kernel (qs_agree.hip), tree_pair_kernel (qs_agree_pairs.hip), tree_branch_kernel (qs_tree_branch.hip) -- restated on the
host, and the tree shapes that put a chosen node into a chosen round. No GPU.

plan(n) is agree_plan: W words per bitmap, at most `cap` link bitmaps in a round, at most `nb` inner nodes in a workgroup. rounds()
is the v0 / v1 walk the three kernels share: a block's nodes are taken while their links fit into `cap`; a node with more than `cap`
links is taken alone and gets no bitmaps (its interval counts come from the tree's leaf list). A stored round is ("S", nodes), an
unstored node ("U",).

flatten.py numbers the inner nodes of a tree in the preorder of its Newick text, whatever the rooting it flattens from, so the text
decides the block and the round of a node. The generators below return such texts over a list of names; a numpy Generator seeds
them. SHAPES_340, two_hubs and sparse_shapes are the calls tests/test_gpu_tree_rounds.py runs on the device and
tests/test_agree_rounds.py checks for the rounds they are named for: both use these functions, so they see the same trees.
"""
import re

import numpy as np

LDS_BYTES = 65536      # kAgreeLdsBytes


def plan(n):
    """(W, cap, nb) of a launch for n taxa, as agree_plan computes them"""
    W = n // 32 + 1
    cap_max = (LDS_BYTES // 8 - W) // W
    nb = max(1, min(64, cap_max // 4))
    cap = min(cap_max, 4 * nb)
    return W, cap, nb


def rounds(batch, n):
    """per tree of the flatten.TreeBatch, per block of its inner nodes: the list of rounds. A tree of fewer than 4 leaves gives []
    (the kernels return before the walk)."""
    _, cap, nb = plan(n)
    node_off, rng_off = batch.node_off.astype(np.int64), batch.rng_off.astype(np.int64)
    out = []
    for t in range(batch.n_trees):
        blocks = []
        v_first, v_all = int(node_off[t]), int(node_off[t + 1])
        if int(batch.leaf_off[t + 1]) - int(batch.leaf_off[t]) >= 4:
            for v_lo in range(v_first, v_all, nb):
                v_hi = min(v_lo + nb, v_all)
                rl = []
                v0 = v_lo
                while v0 < v_hi:
                    k_base = rng_off[v0]
                    v1 = v0
                    while v1 < v_hi and rng_off[v1 + 1] - k_base <= cap:
                        v1 += 1
                    if v1 > v0:
                        rl.append(("S", v1 - v0))
                    else:
                        v1 = v0 + 1
                        rl.append(("U",))
                    v0 = v1
                blocks.append(rl)
        out.append(blocks)
    return out


def kinds(block):
    """the rounds of one block as a string: "S" per stored round, "U" per unstored node"""
    return "".join(r[0] for r in block)


def max_links(batch):
    """per tree the most links of one of its inner nodes (0: no inner node)"""
    d = np.diff(batch.rng_off.astype(np.int64))
    return [int(d[batch.node_off[t]:batch.node_off[t + 1]].max(initial=0)) for t in range(batch.n_trees)]


# ---- tree shapes ----------------------------------------------------------------------------------------------------------------

def names_of(n):
    return [f"t{i}" for i in range(n)]


def relabel_in_order(text):
    """the same tree with its leaves named t0, t1, ... in the order of the text: as a reference it gives every taxon t<i> the id i"""
    k = iter(range(1 << 30))
    return re.sub(r"t\d+", lambda m: f"t{next(k)}", text)


def _newick(t):
    return "(" + ",".join(_newick(c) for c in t) + ")" if isinstance(t, tuple) else t


def _joined(items, rng, arity, stop_at):
    """random joins of `arity` items into one until at most stop_at are left"""
    items = list(items)
    while len(items) > stop_at:
        pick = sorted(rng.choice(len(items), size=arity, replace=False).tolist(), reverse=True)
        items.append(tuple(items.pop(i) for i in pick))
    return items


def _binary(leaves, rng):
    """a random binary subtree (every node two children) over the leaves; one leaf is itself"""
    return _joined(leaves, rng, 2, 1)[0]


def _hub(leaves, children, cherries, rng, extra=()):
    """one node with `children` child links: `cherries` two-leaf subtrees, the subtrees `extra` and leaves, shuffled"""
    n_leaf = children - cherries - len(extra)
    assert n_leaf >= 0 and len(leaves) == n_leaf + 2 * cherries, (len(leaves), children, cherries)
    kids = [(leaves[2 * i], leaves[2 * i + 1]) for i in range(cherries)] + list(leaves[2 * cherries:]) + list(extra)
    return tuple(kids[i] for i in rng.permutation(len(kids)))


def hub_tree(names, before, children, cherries, rng, rooted=False):
    """In the preorder of the text: a random binary subtree of `before` leaves, then one node (the hub) with `children` child links,
    then the other names as a binary subtree. `cherries` of the hub's child links are two-leaf subtrees, the others leaves. The three
    hang on one top node (the hub has children + 1 links); without other names the first subtree's two halves and the hub do, and the
    hub is the last inner node. before = 0: the hub is the root of the text, has no parent link, and the other names' subtree is one
    of its `children` links. rooted: the text has a degree-2 root above (first subtree + hub) and the rest."""
    names = [names[i] for i in rng.permutation(len(names))]
    n_hub = children + cherries - (1 if before == 0 and len(names) > children + cherries else 0)   # leaves directly below the hub
    first, under, rest = names[:before], names[before:before + n_hub], names[before + n_hub:]
    assert len(under) == n_hub, "before + children + cherries exceed the names"
    if before == 0:
        return _newick(_hub(under, children, cherries, rng, extra=[_binary(rest, rng)] if rest else [])) + ";"
    B, H = _binary(first, rng), _hub(under, children, cherries, rng)
    if rooted:
        assert rest
        return _newick(((B, H), _binary(rest, rng))) + ";"
    if rest:
        return _newick((B, H, _binary(rest, rng))) + ";"
    assert isinstance(B, tuple)
    return _newick(B + (H,)) + ";"


def two_hub_tree(names, before, children, rng):
    """hub_tree with a second hub as the first inner node below the first: two nodes of children + 1 links next to each other in
    preorder; all their other child links are leaves"""
    names = [names[i] for i in rng.permutation(len(names))]
    first, a, b, rest = (names[:before], names[before:before + children - 1], names[before + children - 1:before + 2 * children - 1],
                         names[before + 2 * children - 1:])
    assert len(b) == children and len(rest) >= 1
    inner = _hub(b, children, 0, rng)
    return _newick((_binary(first, rng), _hub(a, children, 0, rng, extra=[inner]), _binary(rest, rng))) + ";"


def fan_tree(names, deg, rng):
    """every inner node about `deg` links: random joins of deg - 1 subtrees; the top node takes what is left, 3 .. deg of them"""
    names = [names[i] for i in rng.permutation(len(names))]
    assert len(names) > deg >= 4
    return _newick(tuple(_joined(names, rng, deg - 1, deg))) + ";"


def spread_names(names, k, rng):
    """k of the names, one from each of k equal stretches of the list: as ids they fall into every 32-id word of a bitmap"""
    edges = np.linspace(0, len(names), k + 1).astype(np.int64)
    return [names[int(rng.integers(lo, hi))] for lo, hi in zip(edges, edges[1:])]


def SHAPES_340(names):
    """name -> Newick text of the 340-taxon shapes (plan 11, 256, 64); hub_dropout lacks 8 - 10 % of the names"""
    assert len(names) == 340
    g = np.random.default_rng
    kept = [names[i] for i in sorted(g(3405).choice(340, size=310, replace=False).tolist())]
    return {
        "hub257_mid": hub_tree(names, 70, 256, 4, g(3401)),
        "hub256": hub_tree(names, 70, 255, 4, g(3402)),
        "hub_first": hub_tree(names, 0, 257, 10, g(3403)),
        "hub_last": hub_tree(names, 84, 256, 0, g(3404)),
        "hub_dropout": hub_tree(kept, 20, 258, 6, g(3405), rooted=True),
        "fans7": fan_tree(names, 7, g(3407)),
        "fans5": fan_tree(names, 5, g(3408)),
    }


def two_hubs(names):
    """the 550-taxon shape (plan 18, 256, 64): two nodes of 257 links, one behind the other in preorder"""
    assert len(names) == 550
    return two_hub_tree(names, 20, 256, np.random.default_rng(5501))


def sparse_shapes(names):
    """name -> Newick text of two trees of 320 taxa spread over all len(names) ids, for the plans of 992 taxa and more: a hub of
    cap + 1 links behind more than one stored node of its block, and a fan tree whose blocks take several stored rounds"""
    n = len(names)
    _, cap, nb = plan(n)
    assert cap < 256
    g = np.random.default_rng
    return {
        "hub": hub_tree(spread_names(names, 320, g(n + 1)), nb + 12, cap, 8, g(n + 2)),
        "fans7": fan_tree(spread_names(names, 320, g(n + 3)), 7, g(n + 4)),
    }
