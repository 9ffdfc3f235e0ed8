"""Shared test helpers: table remapping between taxon-id orders, ulp distance, D5 trees, batches of repeated trees."""
import numpy as np


def binom(n, k):
    n = np.asarray(n, dtype=np.int64)
    if k == 2:
        return n * (n - 1) // 2
    if k == 3:
        return n * (n - 1) * (n - 2) // 6
    if k == 4:
        return n * (n - 1) * (n - 2) * (n - 3) // 24
    raise ValueError(k)


def rank4(s0, s1, s2, s3):
    """rank of sorted ids s0<s1<s2<s3 (quartet_lookup_table.hpp:161-165)."""
    return binom(s3, 4) + binom(s2, 3) + binom(s1, 2) + np.asarray(s0, dtype=np.int64)


def quads_in_rank_order(n):
    q = np.array([(a, b, c, d) for d in range(n) for c in range(d) for b in range(c) for a in range(b)],
                 dtype=np.int64).reshape(-1, 4)
    return q


def remap_table(T_src, perm):
    """T_dst over target ids 0..n-1 where target id i is source id perm[i].

    T_* are (C(n,4),3) arrays in rank order with slots (s0s1|s2s3, s0s2|s1s3, s0s3|s1s2)."""
    perm = np.asarray(perm, dtype=np.int64)
    n = len(perm)
    q = quads_in_rank_order(n)                    # target quartets x<y<z<w
    s = perm[q]                                   # source ids, same column roles
    order = np.argsort(s, axis=1)
    ss = np.take_along_axis(s, order, axis=1)
    r = rank4(ss[:, 0], ss[:, 1], ss[:, 2], ss[:, 3])
    pos = np.argsort(order, axis=1)               # pos[:,j] = sorted position of column j
    out = np.zeros_like(T_src[: len(q)])
    # target slot k pairs column 0 with column k+1; source slot = partner position of the min - 1
    for k in range(3):
        partner_col = k + 1
        p0, pp = pos[:, 0], pos[:, partner_col]
        others = [c for c in (1, 2, 3) if c != partner_col]
        po1, po2 = pos[:, others[0]], pos[:, others[1]]
        # the pair containing sorted position 0
        in_first = (p0 == 0) | (pp == 0)
        partner_of_min = np.where(p0 == 0, pp, np.where(pp == 0, p0, np.where(po1 == 0, po2, po1)))
        del in_first
        src_slot = partner_of_min - 1
        out[:, k] = T_src[r, src_slot]
    return out


def ulp_diff(a, b):
    """Distance in units in the last place between two float64 arrays (inf==inf -> 0)."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    ia = a.view(np.int64).copy()
    ib = b.view(np.int64).copy()
    ia = np.where(ia < 0, np.int64(-(2 ** 63)) - ia, ia)
    ib = np.where(ib < 0, np.int64(-(2 ** 63)) - ib, ib)
    return np.abs(ia - ib)


def d5_trees(n=64, block=16):
    from quartetscores_amd.synth import balanced_block
    X = [balanced_block(k * block, (k + 1) * block) for k in range(n // block)]
    ref = f"({X[0]},{X[1]},({X[2]},{X[3]}));"
    alt = f"({X[0]},{X[2]},({X[1]},{X[3]}));"
    return ref, alt


def repeat_trees(batch, reps, with_nodes=True):
    """A flattened batch whose trees are those of `batch` repeated: reps = [(tree index, copies), ...] in the order wanted
    (a tree may appear several times). with_nodes=False leaves the inner-node arrays empty (gather counting needs none)."""
    from quartetscores_amd.flatten import TreeBatch
    one = [batch.slice(t, t + 1) for t, _ in reps]
    k = [int(c) for _, c in reps]
    m = sum(k)

    def offsets(sizes):
        return np.concatenate([[0], np.cumsum(np.concatenate(sizes))]).astype(np.uint32) if sizes else np.zeros(1, np.uint32)
    leaf_off = offsets([np.full(c, len(s.leaf_ids), dtype=np.int64) for s, c in zip(one, k)])
    ids = np.concatenate([np.tile(s.leaf_ids, c) for s, c in zip(one, k)])
    dep = np.concatenate([np.tile(s.adj_depth, c) for s, c in zip(one, k)])
    if not with_nodes:
        return TreeBatch(m, leaf_off, ids, dep, np.zeros(m + 1, dtype=np.uint32), np.zeros(1, dtype=np.uint32), np.zeros(0, dtype=np.uint16))
    node_off = offsets([np.full(c, int(s.node_off[1]), dtype=np.int64) for s, c in zip(one, k)])
    rng_off = offsets([np.tile(np.diff(s.rng_off.astype(np.int64)), c) for s, c in zip(one, k)])
    ranges = np.concatenate([np.tile(s.ranges, c) for s, c in zip(one, k)])
    return TreeBatch(m, leaf_off, ids, dep, node_off, rng_off, ranges)


def concat_batches(a, b):
    """the trees of two flattened batches (with their inner-node arrays) as one batch"""
    from quartetscores_amd.flatten import TreeBatch
    return TreeBatch(
        a.n_trees + b.n_trees,
        np.concatenate([a.leaf_off, b.leaf_off[1:] + a.leaf_off[-1]]).astype(np.uint32),
        np.concatenate([a.leaf_ids, b.leaf_ids]), np.concatenate([a.adj_depth, b.adj_depth]),
        np.concatenate([a.node_off, b.node_off[1:] + a.node_off[-1]]).astype(np.uint32),
        np.concatenate([a.rng_off, b.rng_off[1:] + a.rng_off[-1]]).astype(np.uint32),
        np.concatenate([a.ranges, b.ranges]))


def key_of(csv_names):
    return frozenset(csv_names.split(","))
