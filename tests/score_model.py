"""Vectorised per-node-pair model of the score passes (TEST-ONLY; never shipped or timed).

What qs_score_pass1 / qs_score_pass2 / qs_score_overflow hand to the collectives of a multi-GPU run -- per node pair the
64-bit sums, the minimum QIC and the near-minimal count triples with their swap flag -- computed in plain numpy from
nothing but a flatten.RefTree and the tuples [rank_lo, rank_lo + k) of a count table. No code is shared with the library
except engine.log_score (the host restatement of the reference's formula) and helpers.quads_in_rank_order.

Layout of the outputs (the interface under test, include/quartetscores_hip.h): inner nodes are numbered in node order,
n_inner of them; a node pair's key is min(i1, i2) * n_inner + max(i1, i2); P = n_inner^2 slots.

The two margins the GPU tests assert, both from the project's own contract and not from a measurement
---------------------------------------------------------------------------------------------------
Pass 2 keeps every quartet whose DEVICE QIC lies within tol (1e-12 unless QS_TUNE_SCORE_TOL_EXP says otherwise) of the
pair's DEVICE minimum, and the host then takes the exact minimum of log_score over what was kept. Let e bound the error of
the device QIC against the exact value. The exact minimiser x has device(x) <= exact(x) + e = exact_min + e, and the device
minimum is device(y) >= exact(y) - e >= exact_min - e for the quartet y that attains it: device(x) - device_min <= 2 e. So
the exact minimiser is kept for certain only if 2 e <= tol, i.e. e <= tol / 2 = 5e-13 at the default tolerance. Hence

    |sortable_to_f64(min_dev[key]) - exact_min[key]| <= MIN_MARGIN = 5e-13               (the minimum of values within e)
    must[key]  <=  device candidates of key  <=  may[key]

with must = the quartets whose exact QIC EQUALS exact_min and may = those with exact QIC <= exact_min + tol + 2 * 5e-13:
a kept quartet z has device(z) <= device_min + tol, so exact(z) <= device(z) + e <= exact_min + e + tol + e. At the default
tolerance that is MAY_MARGIN = 2e-12; with QS_TUNE_SCORE_TOL_EXP = x it is 10^-x + 1e-12 (may_margin()).
"""
import functools
import math

import numpy as np

from helpers import quads_in_rank_order
from quartetscores_amd.engine import log_score

KSORT_MAX = 0x7F7F7F7F7F7F7F7F        # "no quartet": what hipMemset(0x7F) leaves in min_dev
MIN_MARGIN = 5e-13
MAY_MARGIN = 2e-12
CAND_SLOTS = 8
_BAND = 1e-9                          # numpy's float64 QIC against log_score: far below this, far above their difference
_FIELD = (1 << 21) - 1
_CAND_OVERFLOW = -2                   # int64 view of the marker in a pair's last slot
_SWAP_SLOT = 1 << 63
_SWAP_LIST = 1 << 32


def may_margin(tol_exp=12):
    return 10.0 ** -tol_exp + 1e-12


def f64_to_sortable(v):
    """qs_common.hpp f64_to_sortable: an int64 that orders like the float64."""
    i = np.ascontiguousarray(v, dtype=np.float64).view(np.int64)
    flipped = (np.uint64(1 << 63) - i.view(np.uint64)).view(np.int64)
    return np.where(i < 0, flipped, i)


def sortable_to_f64(s):
    s = np.ascontiguousarray(s, dtype=np.int64)
    flipped = (np.uint64(1 << 63) - s.view(np.uint64)).view(np.int64)
    return np.where(s < 0, flipped, s).view(np.float64)


@functools.lru_cache(maxsize=4)
def _quads(n):
    q = quads_in_rank_order(n)
    q.setflags(write=False)
    return q


def _c2(x):
    return x * (x - 1) // 2


def _c3(x):
    return x * (x - 1) * (x - 2) // 6


def _c4(x):
    return x * (x - 1) * (x - 2) * (x - 3) // 24


class Passes:
    """Result of ScoreModel.passes(): sums int64[3P], exact_min float64[P] (nan where no quartet), mins int64[P] (encoded,
    KSORT_MAX where no quartet), and the candidate sets on demand."""

    def __init__(self, P, sums, exact_min, near, margins):
        self.P, self.sums, self.exact_min, self.margins = P, sums, exact_min, margins
        self.mins = np.where(np.isnan(exact_min), np.int64(KSORT_MAX), f64_to_sortable(np.nan_to_num(exact_min)))
        self._near = near      # rows (key, r1, r2, r3, swap, exact QIC) of every distinct candidate close to the minimum or the margin
        self.populated = np.flatnonzero(~np.isnan(exact_min))

    def sets(self, margin):
        """{key: {((r1, r2, r3), swap)}} of the quartets whose exact QIC is at most the key's exact minimum + margin."""
        assert margin in self.margins, "passes() was not asked for this margin"
        ref = self.exact_min
        out = {}
        for key, r1, r2, r3, swp, qic in self._near:
            if qic <= ref[key] + margin:
                out.setdefault(key, set()).add(((r1, r2, r3), swp))
        return out

    @property
    def must(self):
        return self.sets(0.0)

    def may(self, margin=MAY_MARGIN):
        return self.sets(margin)


class ScoreModel:
    def __init__(self, ref):
        par = np.asarray(ref.parent, dtype=np.int64)
        N, n = len(par), ref.n_taxa
        self.n, self.N = n, N
        kids = [[] for _ in range(N)]
        for v in range(N):
            if par[v] >= 0:
                kids[par[v]].append(v)
        root = int(np.flatnonzero(par < 0)[0])
        depth = np.zeros(N, dtype=np.int64)
        order, stack = [], [root]
        while stack:                      # any numbering of the nodes: walk down from the root
            v = stack.pop()
            order.append(v)
            for c in kids[v]:
                depth[c] = depth[v] + 1
                stack.append(c)
        nchild = np.array([len(k) for k in kids])
        self.inner_id = -np.ones(N, dtype=np.int64)
        self.inner_id[nchild > 0] = np.arange(int((nchild > 0).sum()))
        self.n_inner = int((nchild > 0).sum())
        self.P = self.n_inner ** 2
        self.bifurcating = int((nchild + (par >= 0)).max()) - 1 == 2
        self.frame = 0 if self.bifurcating else 1
        # leaf interval of every node; lca(i, j) = the deepest node whose interval holds both
        lo, hi = np.full(N, n, dtype=np.int64), np.full(N, -1, dtype=np.int64)
        lo[np.asarray(ref.leaf_node, dtype=np.int64)] = hi[np.asarray(ref.leaf_node, dtype=np.int64)] = np.arange(n)
        for v in reversed(order):
            if par[v] >= 0:
                lo[par[v]], hi[par[v]] = min(lo[par[v]], lo[v]), max(hi[par[v]], hi[v])
        self.lo, self.hi = lo, hi
        lca = np.zeros((n, n), dtype=np.int64)
        for v in sorted(range(N), key=lambda x: depth[x]):
            lca[lo[v]:hi[v] + 1, lo[v]:hi[v] + 1] = v
        self.lca, self.depth = lca, depth
        # degree-2 root of a bifurcating reference: ids [0, root_split) under its first child, and the node pairs (root, v)
        self.root_split, self.root_pairs = 0, []
        if self.bifurcating and nchild[root] == 2:
            rx, ry = sorted(kids[root], key=lambda x: lo[x])
            self.root_split = int(hi[rx] - lo[rx] + 1)
            for v in range(N):
                if v == root or nchild[v] != 2:
                    continue
                mine, other = (rx, ry) if lo[rx] <= lo[v] <= hi[rx] else (ry, rx)
                c3, c4 = sorted(kids[v], key=lambda x: lo[x])
                i1, i2 = sorted((int(self.inner_id[root]), int(self.inner_id[v])))
                rng = lambda x: np.arange(lo[x], hi[x] + 1)
                self.root_pairs.append((i1 * self.n_inner + i2, rng(other), rng(mine), rng(c3), rng(c4)))

    # ---- classification of the quartets of a rank range ----
    def classify(self, rank_lo, k):
        """-> key int64[k] (-1: the reference does not resolve the quartet), code (0: ab|cd, 1: ad|bc), swap flags."""
        q = _quads(self.n)[rank_lo:rank_lo + k]
        a, b, c, d = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        e01, e12, e23 = self.lca[a, b], self.lca[b, c], self.lca[c, d]
        d01, d12, d23 = self.depth[e01], self.depth[e12], self.depth[e23]
        mx = np.maximum(d01, d23)
        abcd, adbc = d12 < mx, d12 > mx
        j1 = np.where(abcd, np.where(d01 > d12, e01, e12), e12)
        j2 = np.where(abcd, np.where(d23 > d12, e23, e12), np.where(d01 >= d23, e01, e23))
        i1, i2 = self.inner_id[j1], self.inner_id[j2]
        key = np.where(abcd | adbc, np.minimum(i1, i2) * self.n_inner + np.maximum(i1, i2), -1)
        code = np.where(adbc, 1, 0)
        ks = self.root_split
        swap = np.zeros(len(q), dtype=bool)
        if ks:     # the rule above root_swapped in qs_score.hip
            swap = (adbc & (a < ks) & (b >= ks)) | (abcd & (c < ks) & (d >= ks))
        return key, code, swap

    def permuted(self, T, code):
        """(q1, q2, q3): the counts in the reference's log_score argument order."""
        T = np.asarray(T, dtype=np.int64)
        alt = T[:, [2, 1, 0]] if self.frame == 0 else T[:, [2, 0, 1]]
        return np.where((code == 1)[:, None], alt, T)

    # ---- the sums of the pairs (root, v) of a degree-2 root: the reference's own enumeration S1 x S2 x S3 x S4 ----
    def _root_pair_sums(self, T, rank_lo, sums):
        k = len(T)
        for key, S1, S2, S3, S4 in self.root_pairs:
            X = np.stack([g.reshape(-1) for g in np.meshgrid(S1, S2, S3, S4, indexing="ij")], axis=1)
            X = X[(X[:, 1] != X[:, 2]) & (X[:, 1] != X[:, 3])]        # a repeated argument reads (0, 0, 0)
            order = np.argsort(X, axis=1)
            pos = np.argsort(order, axis=1)                          # sorted position of every argument
            s = np.take_along_axis(X, order, axis=1)
            r = _c4(s[:, 3]) + _c3(s[:, 2]) + _c2(s[:, 1]) + s[:, 0] - rank_lo
            inside = (r >= 0) & (r < k)
            X, pos, r = X[inside], pos[inside], r[inside]
            if not len(r):
                continue
            first = np.argmin(pos, axis=1)                           # which argument is the smallest id
            rows = np.arange(len(r))
            for j in (1, 2, 3):                                      # pairing: argument 0 with argument j
                o1, o2 = [c for c in (1, 2, 3) if c != j]
                mate = np.zeros(4, dtype=np.int64)
                mate[0], mate[j], mate[o1], mate[o2] = j, 0, o2, o1
                slot = pos[rows, mate[first]] - 1                    # the table's slot: sorted position of the minimum's partner - 1
                sums[3 * key + j - 1] += int(np.asarray(T, dtype=np.int64)[r, slot].sum())

    # ---- passes 1 and 2 ----
    def passes(self, T, rank_lo=0, margins=(MAY_MARGIN,)):
        """T: (k, 3) counts of ranks [rank_lo, rank_lo + k). margins: every may-margin that will be asked of .sets()."""
        T = np.asarray(T, dtype=np.int64).reshape(-1, 3)
        k, P = len(T), self.P
        key, code, swap = self.classify(rank_lo, k)
        res = key >= 0
        key, swap, Q = key[res], swap[res], self.permuted(T, code)[res]
        sums = np.zeros(3 * P, dtype=np.int64)
        for j in range(3):
            np.add.at(sums, 3 * key + j, Q[:, j])
        self._root_pair_sums(T, rank_lo, sums)
        # float64 QIC of every quartet
        s = Q.sum(axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            p = Q / np.maximum(s, 1)[:, None]
            plogp = np.where(Q > 0, p * np.log(p), 0.0)
        qic = np.where(s > 0, 1.0 + plogp.sum(axis=1) / math.log(3), 0.0)
        qic = np.where((Q[:, 0] < Q[:, 1]) | (Q[:, 0] < Q[:, 2]), -qic, qic)
        npmin = np.full(P, np.inf)
        np.minimum.at(npmin, key, qic)
        # exact values where they matter: around the minimum and around every margin asked for; a quartet more than
        # _BAND inside a margin is inside whichever of the two values decides, and keeps numpy's
        off = qic - npmin[key]
        widest = max(margins) if len(margins) else 0.0
        close = off <= _BAND
        for m in margins:
            close |= np.abs(off - m) <= _BAND
        keep = close | (off < widest)
        g = np.gcd(np.gcd(Q[:, 0], Q[:, 1]), Q[:, 2])
        R = Q // np.maximum(g, 1)[:, None]
        rows, first = np.zeros((0, 5), dtype=np.int64), np.zeros(0, dtype=np.int64)
        if keep.any():
            rows, first = np.unique(np.column_stack([key, R, swap.astype(np.int64)])[keep], axis=0, return_index=True)
        is_close, approx = close[keep][first], qic[keep][first]
        exact = {t: log_score(*t) for t in map(tuple, np.unique(rows[is_close][:, 1:4], axis=0).tolist())}   # distinct triples
        exact_min = np.full(P, np.nan)
        near = []
        for (kk, r1, r2, r3, sw), cl, ap in zip(rows.tolist(), is_close.tolist(), approx.tolist()):
            v = exact[(r1, r2, r3)] if cl else ap
            near.append((kk, r1, r2, r3, bool(sw), v))
            if cl and not v >= exact_min[kk]:
                exact_min[kk] = v
        out = Passes(P, sums, exact_min, near, (0.0,) + tuple(margins))
        out.quartet_key = np.full(k, -1, dtype=np.int64)      # per quartet of the range: its node pair, -1 = unresolved
        out.quartet_key[res] = key
        return out


# ---- the device's candidate outputs <-> sets ----

def decode_candidates(cand, extra, P):
    """cand_dev (int64[8P]) and the qs_score_overflow list ((k, 4) int64) -> ({key: {((r1, r2, r3), swap)}}, the keys whose
    last slot carries the overflow marker). A slot is a << 42 | b << 21 | c with bit 63 = swap, -1 = empty; slots are taken as
    they are (pass 2 stores reduced triples), list rows (key | swap << 32, q1, q2, q3) are reduced by their gcd here."""
    cand = np.asarray(cand, dtype=np.int64).reshape(P, CAND_SLOTS)
    out = {}
    keys, slots = np.nonzero((cand != -1) & (cand != _CAND_OVERFLOW))
    for key, w in zip(keys.tolist(), cand[keys, slots].tolist()):
        w &= (1 << 64) - 1
        out.setdefault(key, set()).add((((w >> 42) & _FIELD, (w >> 21) & _FIELD, w & _FIELD), bool(w & _SWAP_SLOT)))
    for k0, q1, q2, q3 in np.asarray(extra, dtype=np.int64).reshape(-1, 4).tolist():
        g = math.gcd(math.gcd(q1, q2), q3) or 1
        out.setdefault(k0 & 0xFFFFFFFF, set()).add(((q1 // g, q2 // g, q3 // g), bool(k0 & _SWAP_LIST)))
    marked = set(np.flatnonzero((cand == _CAND_OVERFLOW).any(axis=1)).tolist())
    return out, marked


def encode_candidates(sets, P):
    """{key: {((r1, r2, r3), swap)}} -> (cand int64[1, 8P], extra (k, 4) int64) as qs_score_finish reads them: packed slots
    where a pair's set fits them, list rows otherwise."""
    cand = -np.ones((P, CAND_SLOTS), dtype=np.int64)
    extra = []
    for key, members in sets.items():
        members = sorted(members)
        packed = [(a << 42) | (b << 21) | c | (_SWAP_SLOT if sw else 0) for (a, b, c), sw in members]
        fits = len(members) <= CAND_SLOTS and all(max(t) <= _FIELD for t, _ in members) and all(w < (1 << 64) - 2 for w in packed)
        if fits:
            cand[key, :len(packed)] = np.array(packed, dtype=np.uint64).view(np.int64)
        else:
            extra += [[key | (_SWAP_LIST if sw else 0), a, b, c] for (a, b, c), sw in members]
    return cand.reshape(1, -1), np.array(extra, dtype=np.int64).reshape(-1, 4)


# ---- inputs shared by test_score_model.py (which asserts that they exercise what is claimed) and test_gpu_score_passes.py ----

def n_quartets(n):
    return _c4(n)


def _names(lo, hi):
    return [f"t{i}" for i in range(lo, hi)]


def _random_clade(names, rng):
    """a random rooted binary subtree on the names, in Newick without the semicolon"""
    from quartetscores_amd import synth
    if len(names) == 1:
        return names[0]
    if len(names) == 2:
        return "(" + names[0] + "," + names[1] + ")"
    return synth.random_tree(len(names), rng, names=list(names), rooted=True)[:-1]


def reference(kind, n, seed=0):
    """Newick of the reference trees of the GPU test (taxa t0..t{n-1})."""
    from quartetscores_amd import synth
    rng = np.random.default_rng(9000 + seed)
    if kind == "random":
        return synth.reference_tree(n, 9100 + seed)
    if kind == "caterpillar":        # lca(a, b) changes with every a, depths up to n - 2
        nw = "(t%d,t%d)" % (n - 2, n - 1)
        for i in range(n - 3, 1, -1):
            nw = "(t%d,%s)" % (i, nw)
        return "(t0,t1,%s);" % nw
    if kind == "balanced":           # long runs between the changes of lca(a, b)
        return "(%s,%s,%s);" % (synth.balanced_block(0, n // 4), synth.balanced_block(n // 4, n // 2), synth.balanced_block(n // 2, n))
    if kind == "multif":
        return synth.tree_set(n, 1, 9200 + seed, collapse=0.3)[0]
    if kind == "star":               # one node of degree >= 8: most quartets are unresolved
        k = n - 16
        return "(%s,%s,%s);" % (",".join(_names(0, k)), _random_clade(_names(k, k + 8), rng), _random_clade(_names(k + 8, n), rng))
    if kind.startswith("rooted"):    # degree-2 root whose first child holds `first` taxa: rooted1, rooted12, ...
        first = int(kind[6:])
        return "(%s,%s);" % (_random_clade(_names(0, first), rng), _random_clade(_names(first, n), rng))
    raise ValueError(kind)


def table(kind, n, seed=0):
    """-> ((C(n,4), 3) uint32 counts, cell bits). Every tuple's sum stays below 2^32."""
    rng = np.random.default_rng(9500 + seed)
    nq = n_quartets(n)
    cols = lambda k: rng.permuted(np.tile(np.arange(3), (k, 1)), axis=1)
    if kind in ("multi", "ties"):
        m = 5000
        T = rng.multinomial(m, [0.6, 0.3, 0.1], size=nq).astype(np.uint32)
        T = np.take_along_axis(T, cols(nq), axis=1)
        T[rng.random(nq) < 0.05] = 0
        if kind == "ties":
            tie = rng.random(nq) < 0.7
            T[tie] = np.array([m, 0, 0], dtype=np.uint32)[cols(int(tie.sum()))]
        return T, 16
    if kind == "lds_edge":           # sums on both sides of the 15 744-entry LDS copy of the log table
        T = rng.multinomial(rng.integers(15000, 17001, size=nq), [0.5, 0.3, 0.2]).astype(np.uint32)
        return np.take_along_axis(T, cols(nq), axis=1), 32
    if kind == "u16_max":
        T = rng.integers(0, 65536, size=(nq, 3)).astype(np.uint32)
        T[rng.random((nq, 3)) < 0.3] = 65535
        return T, 16
    if kind == "u32_big":
        return rng.integers(100_000_000, 900_000_000, size=(nq, 3)).astype(np.uint32), 32
    if kind == "wide":               # reduced triples beyond 21 bits
        T = rng.integers(2_200_000, 9_000_000, size=(nq, 3)).astype(np.uint32)
        T[rng.random(nq) < 0.3] //= 1000
        return T | 1, 32
    if kind == "overflow":           # nearly uniform tuples: QIC ~ +-1e-13 for all of them, dozens of distinct triples within the tolerance
        return (2_000_000 + rng.integers(0, 3, size=(nq, 3))).astype(np.uint32), 32
    if kind == "zero":
        return np.zeros((nq, 3), dtype=np.uint32), 16
    raise ValueError(kind)


def ragged_views(n, bits):
    """(first rank, tuples) of the views of the GPU test; with 16-bit cells a view starts at an even rank (4-byte aligned)."""
    nq = n_quartets(n)
    even = (lambda r: r & ~1) if bits == 16 else (lambda r: r)
    last_row = nq - (n - 3)                                   # row (b, c, d) = (n-3, n-2, n-1): n - 3 tuples
    tail = 5 if bits == 32 or (nq - 5) % 2 == 0 else 6      # the last five tuples (six where five would start at an odd rank)
    views = [(even(nq // 3 + 1), nq // 2),                    # starts and ends inside a row
             (even(last_row + 1), min(5, n - 3 - 3)),         # inside one row
             (0, 1), (even(nq // 2 + 1), 1), (nq - tail, tail)]
    if 7 + 8192 + 9 <= nq:
        views.append((even(7), 8192 + 9))
    return views


def partition(n, bits):
    """views that split the whole table, cut inside rows"""
    nq = n_quartets(n)
    cuts = sorted({0, (nq // 7 + 1) & ~1, (nq // 2 + 3) & ~1, (nq - 3) & ~1, nq})
    return [(lo, hi - lo) for lo, hi in zip(cuts[:-1], cuts[1:])]


# the reference trees of the GPU test by name: (kind, taxa, seed). The sizes are the smallest at which each mechanism engages.
REFERENCES = {"random24": ("random", 24, 0), "caterpillar33": ("caterpillar", 33, 0), "balanced32": ("balanced", 32, 0),
              "multif41": ("multif", 41, 0), "star41": ("star", 41, 0), "rooted1": ("rooted1", 24, 0), "rooted12": ("rooted12", 24, 0),
              "rooted23": ("rooted23", 24, 0), "random70": ("random", 70, 0), "random9": ("random", 9, 1)}


@functools.lru_cache(maxsize=None)
def ref_case(name):
    """-> (flatten.RefTree, ScoreModel) of a named reference"""
    from quartetscores_amd import flatten
    kind, n, seed = REFERENCES[name]
    ref = flatten.flatten_reference(reference(kind, n, seed))
    return ref, ScoreModel(ref)
