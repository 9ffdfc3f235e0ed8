"""Flatten trees into the plain arrays the C-ABI takes (include/quartetscores_hip.h).

Reference tree  -> qs_ref_tree   (parent[], leaf_node[]; lookup ids = depth-first leaf order,
                                  QuartetCounterLookup.hpp:252-258)
Evaluation trees -> qs_tree_batch (leaf_ids / adj_depth per tree = the tour of
                                  QuartetCounterLookup.hpp:211-221 plus LCA depths; and, for the
                                  scatter kernel, the circular leaf ranges behind every link of
                                  every inner node = subtreeLeafIndices, :117-121)

Every evaluation tree is re-rooted at its centre so that LCA depths stay small (the gather
kernel compares 4 trees per 32-bit lane while depths are <= 63); counts do not depend on
the rooting.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Sequence

import numpy as np

from . import newick


class UnknownTaxonError(KeyError):
    """An evaluation tree holds a label the reference tree lacks (the reference program dies
    with an uncaught std::out_of_range, QuartetCounterLookup.hpp:218)."""


@dataclass
class RefTree:
    root: newick.Node
    nodes: List[newick.Node]        # preorder; index == node.index
    parent: np.ndarray              # int32[n_nodes]
    leaf_node: np.ndarray           # uint32[n_taxa]: node index of lookup id i
    names: List[str]                # lookup id -> taxon name
    name_to_id: Dict[str, int]

    @property
    def n_taxa(self):
        return len(self.names)

    @property
    def n_nodes(self):
        return len(self.nodes)


def flatten_reference(text_or_node) -> RefTree:
    root = newick.parse_tree(text_or_node) if isinstance(text_or_node, str) else text_or_node
    nodes = newick.preorder(root)
    for i, x in enumerate(nodes):
        x.index = i
    parent = np.array([x.parent.index if x.parent is not None else -1 for x in nodes], dtype=np.int32)
    leaves = [x for x in nodes if x.is_leaf]  # preorder restricted to leaves = depth-first leaf order
    names = [x.name for x in leaves]
    if len(set(names)) != len(names):
        raise ValueError("duplicate taxon name in the reference tree")
    leaf_node = np.array([x.index for x in leaves], dtype=np.uint32)
    return RefTree(root, nodes, parent, leaf_node, names, {nm: i for i, nm in enumerate(names)})


def taxon_permutation(ref_dst: RefTree, ref_src: RefTree) -> np.ndarray:
    """uint16[n]: entry i = lookup id under ref_src of the taxon whose lookup id under ref_dst is i -- the src_id_of of
    qs_table_remap, which turns a table counted with ref_src into the table ref_dst would have counted. Raises ValueError
    naming the missing and the extra taxa when the two trees do not hold the same taxa."""
    missing = sorted(set(ref_src.names) - set(ref_dst.names))
    extra = sorted(set(ref_dst.names) - set(ref_src.names))
    if missing or extra:
        raise ValueError("the reference trees hold different taxa: missing " + (", ".join(missing) or "none") +
                         "; extra " + (", ".join(extra) or "none"))
    return np.array([ref_src.name_to_id[nm] for nm in ref_dst.names], dtype=np.uint16)


def taxon_restriction(ref_dst: RefTree, ref_src: RefTree) -> np.ndarray:
    """uint16[n_dst]: entry i = lookup id under ref_src of the taxon whose lookup id under ref_dst is i -- the src_id_of of
    qs_table_restrict. Like taxon_permutation, but ref_dst's taxa may be a subset of ref_src's; strictly increasing when
    ref_dst is ref_src pruned (newick.prune keeps the leaf order). Raises ValueError naming the taxa of ref_dst that
    ref_src lacks."""
    extra = sorted(set(ref_dst.names) - set(ref_src.names))
    if extra:
        raise ValueError("the reference trees hold different taxa: missing none; extra " + ", ".join(extra) +
                         " (taxa of ref_dst that ref_src lacks; ref_dst may hold fewer taxa, not others)")
    return np.array([ref_src.name_to_id[nm] for nm in ref_dst.names], dtype=np.uint16)


def parse_species_map(text: str) -> Dict[str, List[str]]:
    """The text of a species map in ASTRAL's format -> {species: [individuals]} in file order. One line per species,
    `species:ind1,ind2,...`; blank lines and lines that start with `#` are ignored, surrounding blanks are trimmed. Raises
    ValueError naming the offending label for a line without a colon, an empty name, an empty individual list and a species
    that has two lines (what the map means beside a reference tree is species_layout's business)."""
    mapping: Dict[str, List[str]] = {}
    for no, line in enumerate(text.splitlines(), 1):
        line = line.strip()
        if not line or line.startswith("#"):
            continue
        if ":" not in line:
            raise ValueError(f"species map line {no}: no ':' in '{line}'")
        species, rest = (x.strip() for x in line.split(":", 1))
        if not species:
            raise ValueError(f"species map line {no}: no species name in front of ':'")
        inds = [x.strip() for x in rest.split(",")] if rest.strip() else []
        if not inds:
            raise ValueError(f"species map line {no}: species '{species}' has an empty individual list")
        if any(not x for x in inds):
            raise ValueError(f"species map line {no}: species '{species}' lists an empty individual name")
        if species in mapping:
            raise ValueError(f"species map line {no}: species '{species}' has two lines")
        mapping[species] = inds
    return mapping


@dataclass
class SpeciesLayout:
    names: List[str]                # counting id -> individual's name
    name_to_id: Dict[str, int]
    first_id: np.ndarray            # uint16[n_species + 1]: species i (the reference's lookup id) owns ids [first_id[i], first_id[i + 1])


MAX_INDIVIDUALS = 4096              # qs_create's cap on n_taxa


def species_layout(ref: RefTree, mapping: Dict[str, Sequence[str]]) -> SpeciesLayout:
    """The counting order of the individuals behind the species tree `ref`: species in ref's lookup-id order, individuals in
    map order within a species; a leaf of ref without an entry is a species with one individual of the same name. Raises
    ValueError naming the label for a species that is no leaf of ref, an individual listed twice (under one species or two),
    an individual named like an unlisted species, an empty individual list, more than 4096 individuals and fewer than 4
    species."""
    owner: Dict[str, str] = {}
    for species, inds in mapping.items():
        if species not in ref.name_to_id:
            raise ValueError(f"species map: species '{species}' is not a leaf of the reference tree")
        if len(inds) == 0:
            raise ValueError(f"species map: species '{species}' has an empty individual list")
        for ind in inds:
            if ind in owner:
                raise ValueError(f"species map: individual '{ind}' is listed twice (species '{owner[ind]}' and '{species}')")
            if ind in ref.name_to_id and ind not in mapping:
                raise ValueError(f"species map: individual '{ind}' of species '{species}' has the name of the unlisted species '{ind}'")
            owner[ind] = species
    if ref.n_taxa < 4:
        raise ValueError(f"species map: fewer than 4 species ({ref.n_taxa}) in the reference tree")
    names: List[str] = []
    first = [0]
    for species in ref.names:
        names.extend(mapping.get(species, [species]))
        first.append(len(names))
    if len(names) > MAX_INDIVIDUALS:
        raise ValueError(f"species map: {len(names)} individuals in all, more than {MAX_INDIVIDUALS}")
    return SpeciesLayout(names, {nm: i for i, nm in enumerate(names)}, np.asarray(first, dtype=np.uint16))


@dataclass
class TreeBatch:
    n_trees: int
    leaf_off: np.ndarray   # uint32[n_trees+1]
    leaf_ids: np.ndarray   # uint16
    adj_depth: np.ndarray  # uint16
    node_off: np.ndarray   # uint32[n_trees+1]
    rng_off: np.ndarray    # uint32[n_nodes+1]
    ranges: np.ndarray     # uint16[2*n_links]

    def slice(self, lo, hi) -> "TreeBatch":
        """Trees [lo, hi) as an independent batch (used to shard trees over GPUs)."""
        l0, l1 = int(self.leaf_off[lo]), int(self.leaf_off[hi])
        v0, v1 = int(self.node_off[lo]), int(self.node_off[hi])
        k0, k1 = int(self.rng_off[v0]), int(self.rng_off[v1])
        return TreeBatch(hi - lo, (self.leaf_off[lo:hi + 1] - l0).astype(np.uint32), self.leaf_ids[l0:l1].copy(),
                         self.adj_depth[l0:l1].copy(), (self.node_off[lo:hi + 1] - v0).astype(np.uint32),
                         (self.rng_off[v0:v1 + 1] - k0).astype(np.uint32), self.ranges[2 * k0:2 * k1].copy())


def _centre(adj: List[List[int]], start: int) -> int:
    def bfs(src):
        dist = [-1] * len(adj)
        prev = [-1] * len(adj)
        dist[src] = 0
        order = [src]
        for x in order:
            for y in adj[x]:
                if dist[y] < 0:
                    dist[y] = dist[x] + 1
                    prev[y] = x
                    order.append(y)
        far = order[-1]
        return far, dist, prev

    u, _, _ = bfs(start)
    v, dist, prev = bfs(u)
    path = [v]
    while path[-1] != u:
        path.append(prev[path[-1]])
    return path[len(path) // 2]


def flatten_tree(root: newick.Node, name_to_id: Dict[str, int], recentre: bool = True):
    """-> (leaf_ids, adj_depth, node_ranges) for one evaluation tree.

    node_ranges: list over inner nodes (degree >= 3) of lists of (start, end) circular ranges,
    one per link, parent side first, like the cycle link().next() walks
    (QuartetCounterLookup.hpp:170-176)."""
    nodes = newick.preorder(root)
    for i, x in enumerate(nodes):
        x.index = i
    adj: List[List[int]] = [[] for _ in nodes]
    for x in nodes:
        if x.parent is not None:
            adj[x.parent.index].append(x.index)  # filled below in child order
    # neighbour order = [parent, children...] (cyclic link order of the reference's tree model)
    adj = [([x.parent.index] if x.parent is not None else []) + [c.index for c in x.children] for x in nodes]
    r = root.index
    if recentre and len(nodes) > 2:
        r = _centre(adj, r)
        if len(adj[r]) == 1:  # centre landed on a leaf (2-leaf tree)
            r = adj[r][0]
    # iterative DFS from r following the cyclic neighbour order starting after the entry link
    L = 0
    leaf_ids: List[int] = []
    adj_depth: List[int] = []
    start = [0] * len(nodes)
    end = [0] * len(nodes)
    depth = [0] * len(nodes)
    order_children: List[List[int]] = [[] for _ in nodes]
    cur_min = 0
    stack = [(r, -1, 0)]
    depth[r] = 0
    while stack:
        x, par, k = stack.pop()
        nb = adj[x]
        if k == 0:
            start[x] = L
            if par >= 0:
                i = nb.index(par)
                order_children[x] = nb[i + 1:] + nb[:i]
            else:
                order_children[x] = list(nb)
            if not order_children[x]:
                nm = nodes[x].name
                if nm not in name_to_id:
                    raise UnknownTaxonError(nm)
                if L > 0:
                    adj_depth.append(cur_min)
                cur_min = 1 << 30
                leaf_ids.append(name_to_id[nm])
                L += 1
                end[x] = L
                continue
        ch = order_children[x]
        if k < len(ch):
            stack.append((x, par, k + 1))
            cur_min = min(cur_min, depth[x])
            depth[ch[k]] = depth[x] + 1
            stack.append((ch[k], x, 0))
        else:
            end[x] = L
    adj_depth.append(0)
    if L == 0:
        adj_depth = []
    node_ranges = []
    for x in range(len(nodes)):
        ch = order_children[x]
        nlinks = len(ch) + (1 if x != r else 0)
        if not ch or nlinks < 3 or L == 0:
            continue
        rl = []
        if x != r:
            rl.append((end[x] % L, start[x] % L))
        for c in ch:
            rl.append((start[c] % L, end[c] % L))
        node_ranges.append(rl)
    return leaf_ids, adj_depth, node_ranges


def flatten_eval_trees(trees: Sequence, name_to_id: Dict[str, int], recentre: bool = True) -> TreeBatch:
    """trees: iterable of Newick strings (one or many trees each) or parsed newick.Node."""
    leaf_off, node_off, rng_off = [0], [0], [0]
    ids: List[int] = []
    dep: List[int] = []
    rng: List[int] = []
    n_trees = 0

    def add(root):
        nonlocal n_trees
        li, ad, nr = flatten_tree(root, name_to_id, recentre)
        if len(set(li)) != len(li):
            raise ValueError(f"evaluation tree {n_trees}: duplicate taxon")
        ids.extend(li)
        dep.extend(ad)
        leaf_off.append(len(ids))
        for rl in nr:
            for (s, e) in rl:
                rng.extend((s, e))
            rng_off.append(len(rng) // 2)
        node_off.append(len(rng_off) - 1)
        n_trees += 1

    for t in trees:
        if isinstance(t, str):
            for root in newick.parse_trees(t):
                add(root)
        else:
            add(t)
    return TreeBatch(n_trees, np.asarray(leaf_off, dtype=np.uint32), np.asarray(ids, dtype=np.uint16),
                     np.asarray(dep, dtype=np.uint16), np.asarray(node_off, dtype=np.uint32),
                     np.asarray(rng_off, dtype=np.uint32), np.asarray(rng, dtype=np.uint16))
