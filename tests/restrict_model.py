"""The specification of qs_table_restrict in numpy, written from the rank formula alone (it shares no code with the
library, the C++ host or tests/helpers.py): the count table over a subset of the taxa, in any id order.

A table is a (C(n,4), 3) array in rank order: the 4-set a < b < c < d sits at rank C(d,4) + C(c,3) + C(b,2) + a, and its
slots count the topologies ab|cd, ac|bd, ad|bc -- slot k pairs the smallest id with the (k+2)-th smallest."""
import functools

import numpy as np


def _choose(x, k):
    x = np.asarray(x, dtype=np.int64)
    out = np.ones_like(x)
    for i in range(k):
        out = out * (x - i)
    for i in range(2, k + 1):
        out = out // i
    return out


@functools.lru_cache(maxsize=4)
def four_sets(n):
    """(C(n,4), 4) int32: the 4-sets a < b < c < d of range(n), row r = the one of rank r."""
    top = np.arange(n + 1)
    r = np.arange(int(_choose(n, 4)), dtype=np.int64)
    cols = []
    for k in (4, 3, 2):
        x = np.searchsorted(_choose(top, k), r, side="right") - 1
        r = r - _choose(x, k)
        cols.append(x)
    d, c, b = cols
    out = np.stack([r, b, c, d], axis=1).astype(np.int32)
    out.setflags(write=False)
    return out


def restrict_table(table, n_src, src_id_of):
    """The table over the taxa src_id_of[0], src_id_of[1], ... (ids of the source table's n_src taxa, all different) with
    ids 0, 1, ... in that order. Destination 4-set t0 < t1 < t2 < t3 has the source ids u_k = src_id_of[t_k]; its tuple is the
    source tuple of the sorted u, and its slot k -- t0 with t_{k+1} against the other two -- is the source slot of the same
    split of the u: the one named by the partner of the smallest u."""
    ids = np.asarray(src_id_of, dtype=np.int64)
    table = np.asarray(table)
    assert table.shape == (int(_choose(n_src, 4)), 3), table.shape
    assert len(set(ids.tolist())) == len(ids) and (ids >= 0).all() and (ids < n_src).all(), "src_id_of must be injective into range(n_src)"
    t = four_sets(len(ids))
    u = [ids[t[:, k]] for k in range(4)]                 # u[k] = source id of t_k
    # place[k] = position of u_k among the sorted u; the sorted u at position p adds C(u, p + 1) to the source rank
    place = [sum((u[j] < u[k]).astype(np.int8) for j in range(4) if j != k) for k in range(4)]
    term = np.stack([_choose(np.arange(n_src), p + 1) for p in range(4)])          # term[p, x] = C(x, p + 1)
    rank = sum(term[place[k], u[k]] for k in range(4))
    out = np.empty((len(t), 3), dtype=table.dtype)
    for k in range(3):
        x, y = [c for c in (1, 2, 3) if c != k + 1]      # the split t0 t_{k+1} | t_x t_y
        # the partner of the smallest u: the other one of its pair
        partner = np.where(place[0] == 0, place[k + 1], np.where(place[k + 1] == 0, place[0], np.where(place[x] == 0, place[y], place[x])))
        out[:, k] = table[rank, partner - 1]
    return out
