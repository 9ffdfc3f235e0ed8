"""Python host above the C-ABI, mirroring the reference's interface for the hot path.

    QuartetCounterLookup  <->  QuartetCounterLookup<CINT>   (QuartetCounterLookup.hpp:24-53)
    QuartetScoreComputer  <->  QuartetScoreComputer<CINT>   (QuartetScoreComputer.hpp:43-80)

Same names, argument meaning and error behaviour, so that the parity tests read like tests
of the reference. All computation happens in libquartetscores_hip.so (HIP, gfx950); this
file only marshals arrays. torch is optional here: it is used when the caller wants the
count table inside a torch tensor (multi-GPU all-reduce over RCCL, see distributed.py).
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import List, Optional, Tuple, Union

import numpy as np

from . import _lib, flatten, newick
from ._lib import (QS_ALGO_AUTO, QS_ALGO_GATHER, QS_ALGO_SCATTER, QS_COUNT_OVERWRITE, QS_COUNT_TIMED, QS_COUNT_WIRE16X2, QS_SCORE_QP_EXACT64,  # noqa: F401
                   QS_SCORE_QP_WRAP32, QS_SCORE_ROOT_AS_EDGE, QS_SCORE_SAVEMEM_LOOKUPS)


class QSError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"[qs {code}] {msg}")
        self.code = code


def count_bits_for(m: int) -> int:
    """Counter width for m evaluation trees. The reference picks u8/u16/u32/u64 by m
    (QuartetScores.cpp:115-147); the GPU table has 16- and 32-bit cells."""
    return 16 if m < (1 << 16) else 32


# qs_set_tuning values applied to every new Context (tests and A/B runs set entries here; empty in production)
DEFAULT_TUNING = {}
# A/B runs of whole test files / tools without editing them: QS_PY_TUNING="14=1,10=2" (key=value pairs of qs_set_tuning). This is
# the PYTHON harness' switch; the library itself reads no environment variables.
for _kv in filter(None, os.environ.get("QS_PY_TUNING", "").split(",")):
    DEFAULT_TUNING[int(_kv.split("=")[0])] = int(_kv.split("=")[1])


AGREEMENT_FIELDS = ("concordant", "discordant", "resolved_eval", "resolved_ref")


def agreement_columns(counts, taxa) -> dict:
    """The derived columns of Context.tree_agreement: counts (n, 4) uint64 in AGREEMENT_FIELDS order, taxa (n,) = n_t per tree
    -> dict of int64 arrays quartets = C(n_t,4), concordant, discordant, eval_only, ref_only, unresolved, and the float64
    array concordance = concordant / (concordant + discordant) (nan where that sum is 0)."""
    a = np.asarray(counts, dtype=np.int64).reshape(-1, 4)
    n = np.asarray(taxa, dtype=np.int64)
    conc, disc, res_e, res_r = a[:, 0], a[:, 1], a[:, 2], a[:, 3]
    quartets = np.where(n >= 4, n * (n - 1) * (n - 2) * (n - 3) // 24, 0)
    eval_only, ref_only = res_e - conc - disc, res_r - conc - disc
    both = conc + disc
    with np.errstate(invalid="ignore", divide="ignore"):
        concordance = np.where(both > 0, conc / np.maximum(both, 1), np.nan)
    return {"quartets": quartets, "concordant": conc, "discordant": disc, "eval_only": eval_only, "ref_only": ref_only,
            "unresolved": quartets - both - eval_only - ref_only, "concordance": concordance}


TREE_TAXA_COLUMNS = ("tree", "taxon", "name", "quartets", "concordant", "discordant", "eval_only", "ref_only", "unresolved", "concordance",
                     "tree_concordance", "concordance_without", "gain")
TREE_TAXA_FLOATS = ("concordance", "tree_concordance", "concordance_without", "gain")


def tree_taxon_columns(names, words, batch: flatten.TreeBatch, first_tree=0, only=None, min_gain=None) -> dict:
    """The columns of QuartetScores --tree-taxa from Context.tree_taxon_agreement: words (m, n, 4) int64 in AGREEMENT_FIELDS order,
    batch = the flattened trees the words came from (it says which taxa a tree holds), first_tree = the index of words[0] among all
    evaluation trees -> dict in TREE_TAXA_COLUMNS order with one entry per tree of at least four taxa and taxon it holds, by tree and
    lookup id: quartets = C(L-1,3) for a tree of L taxa, eval_only / ref_only / unresolved as agreement_columns has them, concordance
    = concordant / (concordant + discordant), tree_concordance = the same ratio over all 4-sets of the tree (the sums over its taxa
    / 4), concordance_without = the ratio over the 4-sets of the tree that do not hold the taxon, gain = concordance_without -
    tree_concordance; nan where a denominator is 0. only = lookup ids to keep (--tree-taxa-only); min_gain = keep the entries with
    gain >= min_gain, which drops those whose gain is nan (--tree-taxa-min-gain). `name` is a list of str."""
    n = len(names)
    w = np.asarray(words, dtype=np.int64).reshape(-1, n, 4)
    keep = None if only is None else set(int(x) for x in only)
    out = {name: [] for name in TREE_TAXA_COLUMNS}
    ratio = lambda num, den: num / den if den else math.nan
    for t in range(len(w)):
        ids = sorted(int(x) for x in batch.leaf_ids[int(batch.leaf_off[t]):int(batch.leaf_off[t + 1])])
        L = len(ids)
        if L < 4:
            continue
        quartets = (L - 1) * (L - 2) * (L - 3) // 6
        conc_t, disc_t = int(w[t, :, 0].sum()) // 4, int(w[t, :, 1].sum()) // 4
        tree_conc = ratio(conc_t, conc_t + disc_t)
        for x in ids:
            c, d, re, rr = (int(z) for z in w[t, x])
            without = ratio(conc_t - c, conc_t - c + disc_t - d)
            gain = without - tree_conc
            if keep is not None and x not in keep:
                continue
            if min_gain is not None and not gain >= min_gain:
                continue
            eo, ro = re - c - d, rr - c - d
            for name, val in zip(TREE_TAXA_COLUMNS, (first_tree + t, x, names[x], quartets, c, d, eo, ro, quartets - c - d - eo - ro, ratio(c, c + d),
                                                     tree_conc, without, gain)):
                out[name].append(val)
    return {name: col if name == "name" else np.asarray(col, dtype=np.float64 if name in TREE_TAXA_FLOATS else np.int64) for name, col in out.items()}


PAIR_FIELDS = ("concordant", "discordant", "resolved_row", "resolved_col", "shared")


def pair_columns(counts) -> dict:
    """The derived columns of Context.tree_pair_agreement: counts (..., 5) uint64 in PAIR_FIELDS order -> dict of int64 arrays (of the
    leading shape) shared, quartets = C(shared,4), concordant, discordant, row_only = resolved_row - concordant - discordant,
    col_only likewise, unresolved = the rest, and the float64 arrays concordance = concordant / (concordant + discordant) (nan where
    that sum is 0) and distance = (discordant + row_only + col_only) / quartets, the normalised quartet distance in which
    "unresolved" is a topology of its own (nan where quartets = 0)."""
    a = np.asarray(counts).astype(np.int64)
    conc, disc, res_r, res_c, n = (a[..., k] for k in range(5))
    quartets = np.where(n >= 4, n * (n - 1) * (n - 2) * (n - 3) // 24, 0)
    row_only, col_only = res_r - conc - disc, res_c - conc - disc
    both, differ = conc + disc, disc + row_only + col_only
    with np.errstate(invalid="ignore", divide="ignore"):
        concordance = np.where(both > 0, conc / np.maximum(both, 1), np.nan)
        distance = np.where(quartets > 0, differ / np.maximum(quartets, 1), np.nan)
    return {"shared": n, "quartets": quartets, "concordant": conc, "discordant": disc, "row_only": row_only, "col_only": col_only,
            "unresolved": quartets - both - row_only - col_only, "concordance": concordance, "distance": distance}


TAXON_FIELDS = ("ref_resolved", "concordant", "discordant", "eval_only", "outvoted", "uninformed")


def taxon_columns(counts) -> dict:
    """The named columns of Context.taxon_support: counts (n, 6) int64 in TAXON_FIELDS order (the sum over the shards of a
    sharded table) -> dict of int64 arrays quartets = C(n-1,3) and the six fields, and the float64 arrays concordance =
    concordant / (concordant + discordant) and concordance_without = the same ratio over the quartets that do NOT hold the
    taxon (every quartet holds four taxa: the table's totals are the column sums / 4); nan where a denominator is 0."""
    a = np.asarray(counts, dtype=np.int64).reshape(-1, 6)
    n = len(a)
    out = {"quartets": np.full(n, (n - 1) * (n - 2) * (n - 3) // 6 if n >= 4 else 0, dtype=np.int64)}
    out.update({name: a[:, k] for k, name in enumerate(TAXON_FIELDS)})
    conc, disc = a[:, 1], a[:, 2]
    rest_c, rest_d = int(conc.sum()) // 4 - conc, int(disc.sum()) // 4 - disc
    with np.errstate(invalid="ignore", divide="ignore"):
        out["concordance"] = np.where(conc + disc > 0, conc / np.maximum(conc + disc, 1), np.nan)
        out["concordance_without"] = np.where(rest_c + rest_d > 0, rest_c / np.maximum(rest_c + rest_d, 1), np.nan)
    return out


TAXON_PAIR_FIELDS = ("n_rt", "n_ra", "T_rt", "S_rt", "T_ra", "S_ra", "T_all", "S_all")
TAXON_PAIR_COLUMNS = ("a", "b", "name_a", "name_b", "quartets", "ref_together", "ref_apart", "together", "apart", "affinity", "kept", "joined")


def taxon_pair_columns(counts, names, taxa=None) -> dict:
    """The columns of QuartetScores --taxon-pairs from Context.taxon_pair_support: counts (len(taxa), n, 8) int64 in
    TAXON_PAIR_FIELDS order, names = the n taxa in lookup-id order, taxa = the lookup ids of the rows (None = all, in id order) ->
    dict in TAXON_PAIR_COLUMNS order with one entry per unordered pair a < b that has a listed taxon, row-major: int64 arrays a, b,
    quartets = C(n-2,2), ref_together = n_rt, ref_apart = n_ra, together = T_all, apart = S_all - T_all, lists name_a, name_b and the
    float64 arrays affinity = T_all / S_all, kept = T_rt / S_rt (where the reference pairs them, how often the trees do), joined =
    T_ra / S_ra (where it separates them, how often the trees pair them anyway); nan where a denominator is 0."""
    n = len(names)
    rows = np.arange(n, dtype=np.int64) if taxa is None else np.asarray(taxa, dtype=np.int64).reshape(-1)
    m = np.asarray(counts, dtype=np.int64).reshape(len(rows), n, 8)
    row_of = np.full(n, -1, dtype=np.int64)
    row_of[rows] = np.arange(len(rows))
    a, b = np.triu_indices(n, 1)                                  # row-major pairs a < b
    keep = (row_of[a] >= 0) | (row_of[b] >= 0)
    a, b = a[keep].astype(np.int64), b[keep].astype(np.int64)
    w = np.where((row_of[a] >= 0)[:, None], m[np.maximum(row_of[a], 0), b], m[np.maximum(row_of[b], 0), a])   # (the matrix is symmetric)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = lambda num, den: np.where(den > 0, num / np.maximum(den, 1), np.nan)
        out = {"a": a, "b": b, "name_a": [names[i] for i in a], "name_b": [names[i] for i in b],
               "quartets": np.full(len(a), (n - 2) * (n - 3) // 2 if n >= 4 else 0, dtype=np.int64),
               "ref_together": w[:, 0], "ref_apart": w[:, 1], "together": w[:, 6], "apart": w[:, 7] - w[:, 6],
               "affinity": ratio(w[:, 6], w[:, 7]), "kept": ratio(w[:, 2], w[:, 3]), "joined": ratio(w[:, 4], w[:, 5])}
    return out


BRANCH_TAXON_FIELDS = ("quartets", "q1", "q2", "q3")
DROP_ONE_COLUMNS = ("taxon", "name", "node", "lo", "hi", "group", "quartets", "q1", "q2", "q3", "qpic", "qpic_without", "delta")


def _internodes(ref: flatten.RefTree):
    """(parent, lo, hi, kids, edges) of a reference tree: [lo, hi) = the lookup ids below every node, kids in id order, edges = the
    internodes as (child node, other end) in node order -- under a degree-2 root the edge through the root once, at the child that
    holds lookup id 0, with the root's other child as its other end"""
    parent = np.asarray(ref.parent, dtype=np.int64)
    N, n = len(parent), ref.n_taxa
    lo, hi = np.full(N, n, dtype=np.int64), np.zeros(N, dtype=np.int64)
    for i in range(n):
        v = int(ref.leaf_node[i])
        while v >= 0:
            lo[v], hi[v] = min(lo[v], i), max(hi[v], i + 1)
            v = int(parent[v])
    kids = [sorted(np.nonzero(parent == v)[0].tolist(), key=lambda k: lo[k]) for v in range(N)]
    root = int(np.nonzero(parent < 0)[0][0])
    edges = []
    for v in range(N):
        if v == root or not kids[v]:
            continue
        u = int(parent[v])
        if u == root and len(kids[u]) == 2:
            w = kids[u][1] if kids[u][0] == v else kids[u][0]
            if kids[w] and v == kids[u][0]:
                edges.append((v, w))
        else:
            edges.append((v, u))
    return parent, lo, hi, kids, edges


def drop_one_columns(ref: flatten.RefTree, taxa, rows, totals) -> dict:
    """The columns of QuartetScores --drop-one from Context.branch_taxon_support: rows (len(taxa), n_nodes, 4) and totals (n_nodes, 4)
    int64 in BRANCH_TAXON_FIELDS order, taxa = the lookup ids of the rows (None = all, in id order) -> dict in DROP_ONE_COLUMNS order
    with one entry per row's taxon (in the order of taxa) and internode (in node order; under a degree-2 root the edge through the root
    once, at the child that holds lookup id 0): int64 arrays taxon, node = the edge's child node, [lo, hi) = the lookup ids below it,
    group = the number of taxa in the taxon's link at its end of the edge, quartets q1 q2 q3 = the row's words, the list name and the
    float64 arrays qpic = log_score(totals), qpic_without = log_score(totals - row), nan where no 4-set around the edge is left
    without the taxon (it is alone in its link at an end of degree 3: the edge dissolves), and delta = qpic_without - qpic."""
    parent, lo, hi, kids, edges = _internodes(ref)
    N, n = len(parent), ref.n_taxa
    ids = np.arange(n, dtype=np.int64) if taxa is None else np.asarray(taxa, dtype=np.int64).reshape(-1)
    rows = np.asarray(rows, dtype=np.int64).reshape(len(ids), N, 4)
    totals = np.asarray(totals, dtype=np.int64).reshape(N, 4)

    def link_size(end, x, away):
        """taxa in x's link at the node `end`, whose link towards `away` is the edge itself"""
        for k in kids[end]:
            if k != away and lo[k] <= x < hi[k]:
                return int(hi[k] - lo[k])
        return int(n - (hi[end] - lo[end]))          # the parent's side

    out = {name: [] for name in DROP_ONE_COLUMNS}
    for k, x in enumerate(ids.tolist()):
        for v, w in edges:
            r, t = rows[k, v], totals[v]
            below = lo[v] <= x < hi[v]
            if below:
                group = link_size(v, x, None)
            elif int(parent[v]) == w:
                group = link_size(w, x, v)
            else:                                    # the other child of a degree-2 root
                group = link_size(w, x, None)
            left = [int(t[i] - r[i]) for i in range(4)]
            qpic = log_score(int(t[1]), int(t[2]), int(t[3]))
            without = log_score(left[1], left[2], left[3]) if left[0] > 0 else math.nan
            for name, val in zip(DROP_ONE_COLUMNS, (x, ref.names[x], v, int(lo[v]), int(hi[v]), group, int(r[0]), int(r[1]), int(r[2]), int(r[3]),
                                                    qpic, without, without - qpic)):
                out[name].append(val)
    for name in DROP_ONE_COLUMNS:
        if name != "name":
            out[name] = np.asarray(out[name], dtype=np.float64 if name in ("qpic", "qpic_without", "delta") else np.int64)
    return out


TREE_BRANCH_FIELDS = ("present", "q1", "q2", "q3")
TREE_BRANCH_COLUMNS = ("tree", "node", "lo", "hi", "present", "q1", "q2", "q3", "concordance")
BOOTSTRAP_COLUMNS = ("node", "lo", "hi", "qpic", "mean", "sd", "lo95", "hi95", "reps")


def tree_branch_columns(ref: flatten.RefTree, rows, first_tree=0) -> dict:
    """The columns of QuartetScores --branch-trees from Context.tree_branch_support: rows (m, n_nodes, 4) int64 in TREE_BRANCH_FIELDS
    order, first_tree = the index of rows[0] among all evaluation trees -> dict in TREE_BRANCH_COLUMNS order with one entry per tree
    and internode (in node order; the edge through a degree-2 root once, as in drop_one_columns) that has present > 0: int64 arrays
    tree, node = the edge's child node, [lo, hi) = the lookup ids below it, present q1 q2 q3 = the row's words, and the float64 array
    concordance = q1 / (q1 + q2 + q3), nan where all three are 0."""
    parent, lo, hi, _, edges = _internodes(ref)
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, len(parent), 4)
    out = {name: [] for name in TREE_BRANCH_COLUMNS}
    for t in range(len(rows)):
        for v, _ in edges:
            present, q1, q2, q3 = (int(z) for z in rows[t, v])
            if present == 0:
                continue
            s = q1 + q2 + q3
            for name, val in zip(TREE_BRANCH_COLUMNS, (first_tree + t, v, int(lo[v]), int(hi[v]), present, q1, q2, q3, q1 / s if s else math.nan)):
                out[name].append(val)
    return {name: np.asarray(col, dtype=np.float64 if name == "concordance" else np.int64) for name, col in out.items()}


def bootstrap_columns(ref: flatten.RefTree, sums, replicates) -> dict:
    """The columns of QuartetScores --bootstrap: sums (n_nodes, 4) = Context.tree_branch_support(...).sum(0) over all evaluation trees,
    replicates (B, n_nodes, 4) = Context.branch_resample of the same rows with every replicate's multiplicities -> dict in
    BOOTSTRAP_COLUMNS order with one entry per internode (as in drop_one_columns): int64 arrays node, lo, hi, reps = B and the float64
    arrays qpic = log_score(sums[1:4]) and, over the B values log_score(replicates[r][1:4]), mean, sd (of the population),
    lo95 = the sorted value at index floor(0.025 (B - 1)) and hi95 = the one at ceil(0.975 (B - 1))."""
    parent, lo, hi, _, edges = _internodes(ref)
    N = len(parent)
    sums = np.asarray(sums, dtype=np.int64).reshape(N, 4)
    reps = np.asarray(replicates, dtype=np.int64).reshape(-1, N, 4)
    B = len(reps)
    out = {name: [] for name in BOOTSTRAP_COLUMNS}
    for v, _ in edges:
        vals = [log_score(int(r[v, 1]), int(r[v, 2]), int(r[v, 3])) for r in reps]
        total = dev = 0.0                            # plain double sums in replicate order, as the CLI adds them
        for x in vals:
            total += x
        mean = total / B if B else math.nan
        for x in vals:
            dev += (x - mean) * (x - mean)
        sd = math.sqrt(dev / B) if B else math.nan
        vals.sort()
        lo95 = vals[int(math.floor(0.025 * (B - 1)))] if B else math.nan
        hi95 = vals[int(math.ceil(0.975 * (B - 1)))] if B else math.nan
        for name, val in zip(BOOTSTRAP_COLUMNS, (v, int(lo[v]), int(hi[v]), log_score(int(sums[v, 1]), int(sums[v, 2]), int(sums[v, 3])),
                                                 mean, sd, lo95, hi95, B)):
            out[name].append(val)
    return {name: np.asarray(col, dtype=np.int64 if name in ("node", "lo", "hi", "reps") else np.float64) for name, col in out.items()}


BRANCH_FREQUENCY_FIELDS = ("en", "Z1", "Z2", "Z3")
FREQUENCY_ONE = 1 << 40                              # the fixed-point unit of Z1, Z2, Z3
LOCAL_PP_COLUMNS = ("node", "lo", "hi", "en", "f1", "f2", "f3", "pp1", "pp2", "pp3", "length", "polytomy_p")


def _beta_continued_fraction(p: float, q: float, x: float) -> float:
    """the continued fraction of I_x(p, q) without its front factor x^p (1-x)^q / (p B(p, q)) (modified Lentz), for
    x < (p + 1) / (p + q + 2); csrc/host/local_pp.hpp step for step"""
    tiny, eps = 1e-300, 1e-16
    qab, qap, qam = p + q, p + 1.0, p - 1.0
    c, d = 1.0, 1.0 - qab * x / qap
    if abs(d) < tiny:
        d = tiny
    d = 1.0 / d
    h = d
    for m in range(1, 100001):
        m2 = 2.0 * m
        for aa in (m * (q - m) * x / ((qam + m2) * (p + m2)), -(p + m) * (qab + m) * x / ((p + m2) * (qap + m2))):
            d = 1.0 + aa * d
            if abs(d) < tiny:
                d = tiny
            c = 1.0 + aa / c
            if abs(c) < tiny:
                c = tiny
            d = 1.0 / d
            h *= d * c
        if abs(d * c - 1.0) < eps:
            break
    return h


def _log_beta_upper_third(a: float, b: float) -> float:
    """ln(B(a, b) (1 - I_{1/3}(a, b))): the continued fraction on whichever of I_{2/3}(b, a) and I_{1/3}(a, b) converges"""
    l13, l23 = math.log(1.0 / 3.0), math.log(2.0 / 3.0)
    if 2.0 / 3.0 < (b + 1.0) / (a + b + 2.0):
        return b * l23 + a * l13 - math.log(b) + math.log(_beta_continued_fraction(b, a, 2.0 / 3.0))
    log_beta = math.lgamma(a) + math.lgamma(b) - math.lgamma(a + b)
    log_lower = a * l13 + b * l23 - log_beta - math.log(a) + math.log(_beta_continued_fraction(a, b, 1.0 / 3.0))
    return log_beta + math.log1p(-math.exp(log_lower))


def local_pp(en: int, z, lam: float = 0.5) -> Tuple[float, float, float, float, float]:
    """The local posterior of a branch (Sayyari & Mirarab 2016) from en = the trees that resolve a 4-set around it and
    z = (z1, z2, z3) = the sums of their normalised frequencies (Context.branch_frequencies' Z_i / 2^40), lam = the prior's rate ->
    (pp1, pp2, pp3, length, polytomy_p): the posterior of the branch and of its two alternatives (in the order of q2, q3), the
    branch's length in coalescent units (0 where z1 / (en + 2 lam - 1) <= 1/3, inf where it is >= 1) and the p-value of the polytomy
    test (chi-square, 2 degrees of freedom). All nan where en = 0. Log space throughout; the arithmetic of csrc/host/local_pp.hpp."""
    if lam <= 0:
        raise ValueError("local_pp: lam must be positive")
    if en <= 0:
        return (math.nan,) * 5
    n = float(en)
    z = [float(x) for x in z]
    w = [x * math.log(2.0) + _log_beta_upper_third(x + 1.0, n - x + 2.0 * lam) for x in z]
    top = max(w)
    total = math.exp(w[0] - top) + math.exp(w[1] - top) + math.exp(w[2] - top)
    pp = [math.exp(x - top) / total for x in w]
    theta = z[0] / (n + 2.0 * lam - 1.0)
    if not math.isfinite(theta) or theta <= 1.0 / 3.0:
        length = 0.0
    elif theta >= 1.0:
        length = math.inf
    else:
        length = -math.log(1.5 * (1.0 - theta))
    chi2 = 0.0
    for x in z:
        chi2 += (x - n / 3.0) * (x - n / 3.0) / (n / 3.0)
    return pp[0], pp[1], pp[2], length, math.exp(-chi2 / 2.0)


def local_pp_columns(ref: flatten.RefTree, freq, lam: float = 0.5) -> dict:
    """The columns of QuartetScores --local-pp: freq (n_nodes, 4) int64 in BRANCH_FREQUENCY_FIELDS order = Context.branch_frequencies
    over all evaluation trees -> dict in LOCAL_PP_COLUMNS order with one entry per internode (as in bootstrap_columns): int64 arrays
    node, lo, hi, en and the float64 arrays f_i = Z_i / 2^40 and local_pp(en, (f1, f2, f3), lam)'s five. The floats other than f_i
    are nan where en = 0, and where the branch does not leave two taxa of the tree's n on either side (no 4-set lies around it)."""
    parent, lo, hi, _, edges = _internodes(ref)
    N, n = len(parent), ref.n_taxa
    freq = np.asarray(freq, dtype=np.int64).reshape(N, 4)
    out = {name: [] for name in LOCAL_PP_COLUMNS}
    for v, _ in edges:
        en = int(freq[v, 0])
        f = [int(freq[v, i]) / FREQUENCY_ONE for i in (1, 2, 3)]
        below = int(hi[v] - lo[v])
        splits = n - 1 > 0 and below >= 2 and n - below >= 2
        for name, val in zip(LOCAL_PP_COLUMNS, (v, int(lo[v]), int(hi[v]), en, *f, *(local_pp(en if splits else 0, f, lam)))):
            out[name].append(val)
    return {name: np.asarray(col, dtype=np.int64 if name in ("node", "lo", "hi", "en") else np.float64) for name, col in out.items()}


GROUP_FIELDS = ("quartets", "q1", "q2", "q3", "outvoted", "uninformed")
GROUP_KINDS = ("quad", "split")


def _group_labels(n_taxa, labels) -> np.ndarray:
    a = np.asarray(labels)
    if a.ndim == 1:
        a = a[None, :]
    if a.ndim != 2 or a.shape[1] != n_taxa:
        raise ValueError(f"group labels need the shape (n_hyp, {n_taxa}), got {a.shape}")
    if a.size and (a.min() < 0 or a.max() > 255):
        raise QSError(_lib.QS_ERR_ARG, "group labels are 0..4")
    return np.ascontiguousarray(a, dtype=np.uint8)


TREE_TAXA_PLAN_FIELDS = ("W", "cap", "nb", "flight", "diff_bytes", "lds_bytes", "max_taxa")


def tree_taxa_plan(n_taxa: int) -> dict:
    """qs_tree_taxa_plan (host-only, no device): the LDS plan of qs_tree_taxon_agreement for n_taxa as a dict of TREE_TAXA_PLAN_FIELDS
    and "supported" (False above max_taxa, where cap and lds_bytes are 0)."""
    L = _lib.load()
    out = np.zeros(7, dtype=np.uint32)
    rc = L.qs_tree_taxa_plan(n_taxa, out.ctypes.data_as(C.c_void_p))
    if rc not in (0, _lib.QS_ERR_UNSUPPORTED):
        raise QSError(rc, L.qs_last_error(None).decode())
    return {**{k: int(v) for k, v in zip(TREE_TAXA_PLAN_FIELDS, out)}, "supported": rc == 0}


def group_check(n_taxa: int, labels) -> Tuple[np.ndarray, np.ndarray]:
    """qs_group_check (host-only, no device): labels (n_hyp, n_taxa) in 0..4 -> (kind uint8 (n_hyp,): 0 quad, 1 split -- GROUP_KINDS --,
    quartets uint64 (n_hyp,): the whole-table number of counted 4-sets). QSError(QS_ERR_ARG) names the first hypothesis that is
    neither a quad nor a split and what it lacks."""
    L = _lib.load()
    a = _group_labels(n_taxa, labels)
    kind, quartets = np.zeros(len(a), dtype=np.uint8), np.zeros(len(a), dtype=np.uint64)
    rc = L.qs_group_check(n_taxa, a.ctypes.data_as(C.c_void_p), len(a), kind.ctypes.data_as(C.c_void_p), quartets.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise QSError(rc, L.qs_last_error(None).decode())
    return kind, quartets


def parse_group_spec(text: str, name_to_id) -> Tuple[List[str], np.ndarray]:
    """The SPEC file of QuartetScores --test-groups -> (names, labels uint8 (n_hyp, n_taxa)) for Context.group_support. One
    hypothesis per non-empty line that does not start with '#': NAME<TAB>G1<TAB>G2 (split S1 | S2) or NAME<TAB>G1<TAB>G2<TAB>G3<TAB>G4
    (quad S1 S2 | S3 S4); a group is a comma-separated list of taxon names, and one group of a split may be '*' = every taxon the
    other group does not name. ValueError names the line (from 1) of an unknown name, a name in two groups, an empty group, a
    split group with one taxon, or a line with three or more than four groups."""
    n = len(name_to_id)
    names, rows = [], []
    for ln, line in enumerate(text.splitlines(), 1):
        line = line.rstrip("\r")
        if not line.strip() or line.lstrip().startswith("#"):
            continue
        cols = line.split("\t")
        if len(cols) not in (3, 5):
            raise ValueError(f"line {ln}: a hypothesis needs a name and two or four groups, found {len(cols) - 1} group(s)")
        row = np.zeros(n, dtype=np.uint8)
        stars = [k for k, g in enumerate(cols[1:], 1) if g.strip() == "*"]
        if stars and (len(cols) != 3 or len(stars) > 1):
            raise ValueError(f"line {ln}: '*' may stand for one group of a split only")
        for k, g in enumerate(cols[1:], 1):
            if k in stars:
                continue
            members = [x.strip() for x in g.split(",")]
            if members == [""]:
                raise ValueError(f"line {ln}: group {k} is empty")
            for x in members:
                if x not in name_to_id:
                    raise ValueError(f"line {ln}: unknown taxon '{x}' in group {k}")
                if row[name_to_id[x]]:
                    raise ValueError(f"line {ln}: taxon '{x}' is in two groups (or twice in one)")
                row[name_to_id[x]] = k
        if stars:
            row[row == 0] = stars[0]
        if len(cols) == 3:
            for k in (1, 2):
                if (row == k).sum() < 2:
                    raise ValueError(f"line {ln}: group {k} of a split needs at least two taxa" if (row == k).sum() else f"line {ln}: group {k} is empty")
        names.append(cols[0])
        rows.append(row)
    return names, (np.stack(rows) if rows else np.zeros((0, n), dtype=np.uint8))


def group_columns(kind, counts) -> dict:
    """The columns of QuartetScores --test-groups from Context.group_support's (n_hyp, 6) words and group_check's kinds: the six
    GROUP_FIELDS as int64 arrays, support = q1 / (q1 + q2 + q3) (nan where that is 0) and qpic = log_score(q1, q2, q3) for quad
    hypotheses (nan for splits, whose q2 / q3 division means nothing)."""
    a = np.asarray(counts, dtype=np.int64).reshape(-1, 6)
    out = {name: a[:, k] for k, name in enumerate(GROUP_FIELDS)}
    tot = a[:, 1] + a[:, 2] + a[:, 3]
    with np.errstate(invalid="ignore", divide="ignore"):
        out["support"] = np.where(tot > 0, a[:, 1] / np.maximum(tot, 1), np.nan)
    out["qpic"] = np.array([log_score(int(r[1]), int(r[2]), int(r[3])) if k == 0 else math.nan for k, r in zip(np.asarray(kind).reshape(-1), a)], dtype=np.float64)
    return out


PLACEMENT_COLUMNS = ("taxon", "name", "current", "best", "gain", "n_best", "best_node", "best_lo", "best_hi", "distance")


def placement_scores(ref: flatten.RefTree, links) -> np.ndarray:
    """qs_placement_scores (host-only, no device): rows of link sums (n_list, 2 * n_nodes) of Context.taxon_placement -> int64
    (n_list, n_nodes), the placement score of the edge above every node; the root's entry is 0."""
    L = _lib.load()
    W = np.ascontiguousarray(links, dtype=np.int64).reshape(-1, 2 * ref.n_nodes)
    out = np.zeros((len(W), ref.n_nodes), dtype=np.int64)
    s, keep = Context._ref_struct(ref)
    for row, dst in zip(W, out):
        rc = L.qs_placement_scores(C.byref(s), row.ctypes.data_as(C.c_void_p), dst.ctypes.data_as(C.c_void_p))
        if rc != 0:
            raise QSError(rc, L.qs_last_error(None).decode())
    del keep
    return out


def _tree_arrays(ref: flatten.RefTree):
    """parent, depth, leaf interval [lo, hi) and links (children + parent edge) of every node; the root's index"""
    parent = np.asarray(ref.parent, dtype=np.int64)
    N, n = len(parent), ref.n_taxa
    root = int(np.nonzero(parent < 0)[0][0])
    order = newick.preorder(ref.root)
    depth = np.zeros(N, dtype=np.int64)
    for x in order[1:]:
        depth[x.index] = depth[x.parent.index] + 1
    lo, hi = np.full(N, n, dtype=np.int64), np.zeros(N, dtype=np.int64)
    leaf_node = np.asarray(ref.leaf_node, dtype=np.int64)
    lo[leaf_node], hi[leaf_node] = np.arange(n), np.arange(n) + 1
    for x in reversed(order[1:]):                      # children before parents
        p = x.parent.index
        lo[p], hi[p] = min(lo[p], lo[x.index]), max(hi[p], hi[x.index])
    links = np.bincount(parent[parent >= 0], minlength=N) + (parent >= 0)
    return parent, depth, lo, hi, links, root


def placement_columns(ref: flatten.RefTree, taxa, scores) -> dict:
    """The columns of QuartetScores --place-taxa (PLACEMENT_COLUMNS) for the listed taxa (lookup ids) and their rows of
    placement_scores. A position = the edges that induce the same bipartition of the OTHER taxa (the taxon's own pendant edge
    belongs to the position of the two other edges at a parent with three links). current = the score at the taxon's own edge,
    best = the largest score, n_best = positions that attain it; the reported position is the current one if it attains best,
    else the one that holds the smallest node index; best_node = its smallest node index, [best_lo, best_hi) the lookup ids
    below that node; distance = 0 for the current position, else the nodes on the path from the taxon's parent to the nearer end
    of the edge above best_node that keep three links without the taxon (1 = an NNI neighbour)."""
    parent, depth, lo, hi, links, root = _tree_arrays(ref)
    N, n = len(parent), ref.n_taxa
    leaf_node = np.asarray(ref.leaf_node, dtype=np.int64)
    edges = np.arange(N) != root
    sc = np.asarray(scores, dtype=np.int64).reshape(len(taxa), N)

    def walk(a, b):
        left, right = [a], [b]
        while left[-1] != right[-1]:
            if depth[left[-1]] >= depth[right[-1]]:
                left.append(int(parent[left[-1]]))
            else:
                right.append(int(parent[right[-1]]))
        return left + right[-2::-1]

    out = {name: [] for name in PLACEMENT_COLUMNS}
    for row, x in zip(sc, taxa):
        x = int(x)
        a, b = lo - (lo > x), hi - (hi > x)            # the interval below every node in the others' numbering
        flip = (a == 0) & (b > 0)
        a, b = np.where(flip, b, a), np.where(flip, n - 1, b)
        key = np.where(b > a, a * n + b, 0)            # the side without the smallest other taxon; 0 = all others on one side
        own = int(leaf_node[x])
        u = int(parent[own])
        if links[u] == 3:
            key[own] = key[[w for w in np.nonzero(parent == u)[0] if w != own][0]]
        current, best = int(row[own]), int(row[edges].max())
        top = edges & (row == best)
        pick = key[own] if current == best else key[np.nonzero(top)[0][0]]
        node = int(np.nonzero(edges & (key == pick))[0][0])
        dist = 0
        if pick != key[own]:
            near = min((walk(u, node), walk(u, int(parent[node]))), key=len)
            dist = sum(1 for w in near if links[w] - (w == u) >= 3)
        vals = (x, ref.names[x], current, best, best - current, len(np.unique(key[top])), node, int(lo[node]), int(hi[node]), dist)
        for name, val in zip(PLACEMENT_COLUMNS, vals):
            out[name].append(val)
    return {k: (v if k == "name" else np.array(v, dtype=np.int64)) for k, v in out.items()}


CLADE_PLACEMENT_COLUMNS = ("clade", "node", "lo", "hi", "size", "current", "best", "gain", "n_best", "best_node", "best_lo", "best_hi", "distance")


def eligible_clades(ref: flatten.RefTree) -> np.ndarray:
    """The default list of Context.clade_placement and --place-clades: the inner non-root nodes of `ref` with at least three
    taxa outside them, in node order."""
    parent, _, lo, hi, links, root = _tree_arrays(ref)
    inner = np.bincount(parent[parent >= 0], minlength=len(parent)) > 0
    return np.nonzero(inner & (np.arange(len(parent)) != root) & (ref.n_taxa - (hi - lo) >= 3))[0].astype(np.int64)


def clade_placement_columns(ref: flatten.RefTree, nodes, scores) -> dict:
    """The columns of QuartetScores --place-clades (CLADE_PLACEMENT_COLUMNS) for the listed nodes and their rows of
    placement_scores over Context.clade_placement. clade = the list index, [lo, hi) the clade's lookup ids. A position = the
    edges OUTSIDE the clade that induce the same bipartition of the taxa outside it; the clade's own edge belongs to the position
    of the two other edges at a parent with three links (under a multifurcation it is a position of its own: the score at the
    node). The remaining columns as placement_columns defines them with the clade in the taxon's place: distance = 0 for the
    current position, else the nodes on the path from the clade's parent to the nearer end of the edge above best_node that keep
    three links without the clade (1 = an NNI of the clade)."""
    parent, depth, lo, hi, links, root = _tree_arrays(ref)
    N, n = len(parent), ref.n_taxa
    sc = np.asarray(scores, dtype=np.int64).reshape(len(nodes), N)

    def walk(a, b):
        left, right = [a], [b]
        while left[-1] != right[-1]:
            if depth[left[-1]] >= depth[right[-1]]:
                left.append(int(parent[left[-1]]))
            else:
                right.append(int(parent[right[-1]]))
        return left + right[-2::-1]

    out = {name: [] for name in CLADE_PLACEMENT_COLUMNS}
    for k, (row, c) in enumerate(zip(sc, nodes)):
        c = int(c)
        cl, ch = int(lo[c]), int(hi[c])
        size = ch - cl
        edges = (np.arange(N) != root) & ~((lo >= cl) & (hi <= ch) & (np.arange(N) != c))   # outside the clade, and its own edge
        a, b = lo - np.where(lo >= ch, size, 0), hi - np.where(hi >= ch, size, 0)            # in the numbering of the taxa outside
        flip = (a == 0) & (b > 0)
        a, b = np.where(flip, b, a), np.where(flip, n - size, b)
        key = np.where(b > a, a * n + b, 0)            # the side without the smallest outside taxon; 0 = all of them on one side
        u = int(parent[c])                             # (the clade's own edge has key 0 so far: nothing outside below it)
        if links[u] == 3:
            key[c] = key[[w for w in np.nonzero(parent == u)[0] if w != c][0]]
        current, best = int(row[c]), int(row[edges].max())
        top = edges & (row == best)
        pick = key[c] if current == best else key[np.nonzero(top)[0][0]]
        node = int(np.nonzero(edges & (key == pick))[0][0])
        dist = 0
        if pick != key[c]:
            near = min((walk(u, node), walk(u, int(parent[node]))), key=len)
            dist = sum(1 for w in near if links[w] - (w == u) >= 3)
        vals = (k, c, cl, ch, size, current, best, best - current, len(np.unique(key[top])), node, int(lo[node]), int(hi[node]), dist)
        for name, val in zip(CLADE_PLACEMENT_COLUMNS, vals):
            out[name].append(val)
    return {k: np.array(v, dtype=np.int64) for k, v in out.items()}


class Context:
    """Thin RAII wrapper of qs_ctx."""

    def __init__(self, n_taxa: int, count_bits: int = 32, device: int = 0, stream: int = 0, d_lo: int = 0, d_hi: int = 0):
        self.L = _lib.load()
        h = C.c_void_p()
        rc = self.L.qs_create(C.byref(h), n_taxa, count_bits, 0, device, C.c_void_p(stream or None), d_lo, d_hi or n_taxa)
        if rc != 0:
            raise QSError(rc, self.L.qs_last_error(None).decode())
        self.h = h
        self.n = n_taxa
        self.count_bits = count_bits
        self.device = device
        self.d_lo, self.d_hi = d_lo, d_hi or n_taxa
        self._batch_trees = {}  # uploaded batch handle -> its number of trees (tree_agreement)
        self._attached = None  # keeps an attached torch tensor alive
        for key, value in DEFAULT_TUNING.items():
            self.set_tuning(key, value)

    def close(self):
        if getattr(self, "h", None):
            self.L.qs_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise QSError(rc, self.L.qs_last_error(self.h).decode())

    # table
    @property
    def table_tuples(self) -> int:
        return int(self.L.qs_table_tuples(self.h))

    @property
    def table_bytes(self) -> int:
        return int(self.L.qs_table_bytes(self.h))

    def table_alloc(self):
        self._chk(self.L.qs_table_alloc(self.h))

    def table_attach(self, tensor):
        """tensor: a torch CUDA tensor with >= table_bytes bytes (kept alive by this object); None detaches the
        caller-owned table (waits for the context's stream first)."""
        if tensor is None:
            self._chk(self.L.qs_table_attach(self.h, None, 0))
            self._attached = None
            return
        nbytes = tensor.numel() * tensor.element_size()
        self._chk(self.L.qs_table_attach(self.h, C.c_void_p(tensor.data_ptr()), nbytes))
        self._attached = tensor

    def issue_probe(self, iterations: int = 100000) -> float:
        """qs_issue_probe: ns per wave instruction and SIMD of the count kernel's bare instruction slot on this device."""
        out = C.c_float(0)
        self._chk(self.L.qs_issue_probe(self.h, iterations, C.byref(out)))
        return float(out.value)

    def sum_words(self, dst, sources):
        """qs_sum_words: dst += sum of the source tensors, as 32-bit words (torch CUDA tensors of equal size; the sources may
        live on peer devices this process has enabled access to); asynchronous."""
        n = dst.numel() * dst.element_size() // 4
        arr = (C.c_void_p * len(sources))(*[s_.data_ptr() for s_ in sources])
        self._chk(self.L.qs_sum_words(self.h, C.c_void_p(dst.data_ptr()), arr, len(sources), n))

    def table_pack16(self, tensor):
        """u32 table -> u16 table in `tensor` (torch CUDA tensor, >= ceil(cells/2)*4 bytes); asynchronous."""
        self._chk(self.L.qs_table_pack16(self.h, C.c_void_p(tensor.data_ptr()), tensor.numel() * tensor.element_size()))

    def wire_attach(self, tensor):
        """Destination of count_batch(..., QS_COUNT_WIRE16X2): table_tuples int32 words (torch CUDA tensor; None detaches)."""
        if tensor is None:
            self._chk(self.L.qs_wire_attach(self.h, None, 0))
        else:
            self._chk(self.L.qs_wire_attach(self.h, C.c_void_p(tensor.data_ptr()), tensor.numel() * tensor.element_size()))
        self._wire = tensor

    def table_pack16x2(self, tensor):
        """u32 table -> one word n0 | n1 << 16 per tuple (batches of binary trees holding all taxa); asynchronous."""
        self._chk(self.L.qs_table_pack16x2(self.h, C.c_void_p(tensor.data_ptr()), tensor.numel() * tensor.element_size()))

    def table_pack32x2(self, tensor):
        """qs_table_pack32x2: (n0, n1) per tuple as two u32 words into `tensor` (int32, >= 2 * table_tuples elements)."""
        self._chk(self.L.qs_table_pack32x2(self.h, C.c_void_p(tensor.data_ptr()), tensor.numel() * tensor.element_size()))

    def unpack32x2(self, src, n_tuples: int, total_trees: int, dst):
        """qs_unpack32x2: n_tuples (n0, n1) pairs of `src` -> [rank][3] u32 tuples in `dst` (n2 = total_trees - n0 - n1)."""
        if src.numel() < 2 * n_tuples or dst.numel() * dst.element_size() < n_tuples * 12:
            raise ValueError("unpack32x2: buffer too small")
        self._chk(self.L.qs_unpack32x2(self.h, C.c_void_p(src.data_ptr()), n_tuples, total_trees, C.c_void_p(dst.data_ptr())))

    def unpack16x2(self, src, n_tuples: int, total_trees: int, dst):
        """n_tuples reduced words -> [tuple][3] u16 cells in `dst` (n2 = total_trees - n0 - n1); asynchronous."""
        if src.numel() * src.element_size() < n_tuples * 4 or dst.numel() * dst.element_size() < n_tuples * 6:
            raise ValueError("unpack16x2: buffer too small")
        self._chk(self.L.qs_unpack16x2(self.h, C.c_void_p(src.data_ptr()), n_tuples, total_trees, C.c_void_p(dst.data_ptr())))

    def table_remap(self, src: "Context", src_id_of):
        """qs_table_remap: this context's table := `src`'s table in another lookup-id order. src_id_of[i] = id in src's order
        of the taxon whose id here is i (flatten.taxon_permutation(ref_here, ref_src)). Asynchronous on this context's stream."""
        perm = np.ascontiguousarray(src_id_of, dtype=np.uint16)
        if perm.shape != (self.n,):
            raise ValueError(f"table_remap: src_id_of needs {self.n} entries, got {perm.shape}")
        self._chk(self.L.qs_table_remap(self.h, src.h, perm.ctypes.data_as(C.c_void_p)))

    def table_restrict(self, src: "Context", src_id_of):
        """qs_table_restrict: this context's table := `src`'s table over a subset of its taxa. src_id_of[i] = id in src's order
        of the taxon whose id here is i (flatten.taxon_restriction(ref_here, ref_src)); any injective map, strictly increasing
        for a pruned reference tree. Asynchronous on this context's stream."""
        ids = np.ascontiguousarray(src_id_of, dtype=np.uint16)
        if ids.shape != (self.n,):
            raise ValueError(f"table_restrict: src_id_of needs {self.n} entries, got {ids.shape}")
        self._chk(self.L.qs_table_restrict(self.h, src.h, ids.ctypes.data_as(C.c_void_p)))

    def table_collapse(self, src: "Context", first_id):
        """qs_table_collapse: this context's table (species) := the sums of `src`'s table (individuals) over one individual per
        species. Species i owns src's ids [first_id[i], first_id[i + 1]) (flatten.species_layout); n_taxa + 1 entries from 0 to
        src's n_taxa, strictly increasing. A sum beyond this context's cell width raises QS_ERR_OVERFLOW at the next sync().
        Asynchronous on this context's stream."""
        ids = np.ascontiguousarray(first_id, dtype=np.uint16)
        if ids.shape != (self.n + 1,) or (np.asarray(first_id).astype(np.int64) != ids).any():
            raise ValueError(f"table_collapse: first_id needs {self.n + 1} entries in [0, 65535], got {np.shape(first_id)}")
        self._chk(self.L.qs_table_collapse(self.h, src.h, ids.ctypes.data_as(C.c_void_p)))

    def tree_agreement(self, ref: flatten.RefTree, hb) -> np.ndarray:
        """qs_tree_agreement: per tree of the uploaded batch `hb` (uploaded with its node ranges) its quartet agreement with `ref`
        -> uint64 (n_trees, 4) in AGREEMENT_FIELDS order (agreement_columns derives the rest). Allocates the device buffer,
        waits for the result and downloads it."""
        import torch
        n_trees = self._batch_trees[hb.value]
        buf = torch.empty(max(1, 4 * n_trees), dtype=torch.int64, device=f"cuda:{self.device}")
        s, keep = self._ref_struct(ref)
        self._chk(self.L.qs_tree_agreement(self.h, C.byref(s), hb, C.c_void_p(buf.data_ptr())))
        self.sync()
        del keep
        return buf[: 4 * n_trees].cpu().numpy().view(np.uint64).reshape(n_trees, 4)

    def tree_branch_support(self, ref: flatten.RefTree, hb) -> np.ndarray:
        """qs_tree_branch_support: per tree of the uploaded batch `hb` (uploaded with its node ranges) and node v of `ref` the four
        words of TREE_BRANCH_FIELDS over the 4-sets around the internode above v that lie inside the tree's taxa -> int64
        (n_trees, n_nodes, 4); tree_branch_columns turns them into the CLI's columns. Allocates the device buffer, waits for the
        result and downloads it."""
        n_trees = self._batch_trees[hb.value]
        words = n_trees * ref.n_nodes * 4
        return self._query(ref, words, lambda s, p: self.L.qs_tree_branch_support(self.h, s, hb, C.c_void_p(p))).reshape(n_trees, ref.n_nodes, 4)

    def tree_taxon_agreement(self, ref: flatten.RefTree, hb) -> np.ndarray:
        """qs_tree_taxon_agreement: per tree of the uploaded batch `hb` (uploaded with its node ranges) and taxon (lookup id) the four
        words of AGREEMENT_FIELDS over the 4-sets of the tree's taxa that hold the taxon -> int64 (n_trees, n_taxa, 4); taxa the tree
        lacks give zeros; tree_taxon_columns turns them into the CLI's columns. Allocates the device buffer, waits for the result
        and downloads it."""
        n_trees = self._batch_trees[hb.value]
        words = n_trees * self.n * 4
        return self._query(ref, words, lambda s, p: self.L.qs_tree_taxon_agreement(self.h, s, hb, C.c_void_p(p))).reshape(n_trees, self.n, 4)

    def branch_resample(self, rows, weights, out=None) -> np.ndarray:
        """qs_branch_resample: rows int64 (m, n_nodes, 4) as tree_branch_support returns them, weights (B, m) unsigned 32-bit ->
        int64 (B, n_nodes, 4), entry [r] = sum over t of weights[r][t] * rows[t]; added to `out` (same shape) if given, so that
        batches of trees stream through with their slice of the weights. Uploads the rows, waits for the result and downloads it."""
        import torch
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        if rows.ndim != 3 or rows.shape[2] != 4:
            raise ValueError("branch_resample: rows must be (m, n_nodes, 4)")
        m, n_nodes = rows.shape[:2]
        wide = np.asarray(weights, dtype=np.int64)
        if wide.ndim != 2 or wide.shape[1] != m:
            raise ValueError(f"branch_resample: weights must be (B, {m})")
        if ((wide < 0) | (wide > 0xFFFFFFFF)).any():
            raise QSError(_lib.QS_ERR_ARG, "branch_resample: weight out of range")
        w = np.ascontiguousarray(wide, dtype=np.uint32)
        B = len(w)
        dev = f"cuda:{self.device}"
        d_rows = torch.from_numpy(rows.reshape(-1)).to(dev) if rows.size else torch.zeros(1, dtype=torch.int64, device=dev)
        start = np.zeros((B, n_nodes, 4), dtype=np.int64) if out is None else np.ascontiguousarray(out, dtype=np.int64).reshape(B, n_nodes, 4)
        d_out = torch.from_numpy(start.reshape(-1)).to(dev) if start.size else torch.zeros(1, dtype=torch.int64, device=dev)
        self._chk(self.L.qs_branch_resample(self.h, C.c_void_p(d_rows.data_ptr()), m, n_nodes, w.ctypes.data_as(C.c_void_p), B,
                                            C.c_void_p(d_out.data_ptr())))
        self.sync()
        return d_out[: start.size].cpu().numpy().reshape(B, n_nodes, 4)

    def branch_frequencies(self, rows, out=None) -> np.ndarray:
        """qs_branch_frequencies: rows int64 (m, n_nodes, 4) as tree_branch_support returns them (a host array, or a torch tensor
        on this context's device, which is read in place) -> int64 (n_nodes, 4) in BRANCH_FREQUENCY_FIELDS order: per node the number
        of trees with q1 + q2 + q3 > 0 and the sums over them of floor(q_i * 2^40 / (q1 + q2 + q3)); added to `out` (same shape) if
        given, so that batches of trees stream through. local_pp / local_pp_columns turn them into the posterior. Waits for the
        result and downloads it."""
        import torch
        dev = f"cuda:{self.device}"
        if isinstance(rows, torch.Tensor):
            if rows.dtype != torch.int64 or not rows.is_contiguous() or str(rows.device) != dev:
                raise ValueError(f"branch_frequencies: a tensor of rows must be contiguous int64 on {dev}")
            d_rows = rows
        else:
            d_rows = np.ascontiguousarray(rows, dtype=np.int64)
        if d_rows.ndim != 3 or d_rows.shape[2] != 4:
            raise ValueError("branch_frequencies: rows must be (m, n_nodes, 4)")
        m, n_nodes = int(d_rows.shape[0]), int(d_rows.shape[1])
        if not isinstance(rows, torch.Tensor):
            d_rows = torch.from_numpy(d_rows.reshape(-1)).to(dev)
        if m * n_nodes == 0:
            d_rows = torch.zeros(1, dtype=torch.int64, device=dev)
        start = np.zeros((n_nodes, 4), dtype=np.int64) if out is None else np.ascontiguousarray(out, dtype=np.int64).reshape(n_nodes, 4)
        d_out = torch.from_numpy(start.reshape(-1)).to(dev) if start.size else torch.zeros(1, dtype=torch.int64, device=dev)
        self._chk(self.L.qs_branch_frequencies(self.h, C.c_void_p(d_rows.data_ptr()), m, n_nodes, C.c_void_p(d_out.data_ptr())))
        self.sync()
        return d_out[: start.size].cpu().numpy().reshape(n_nodes, 4)

    def tree_pair_agreement(self, hb_rows, hb_cols=None, rows=None, cols=None, upper=False) -> np.ndarray:
        """qs_tree_pair_agreement: the quartet agreement of the trees rows = (r0, r1) of the uploaded batch `hb_rows` with the trees
        cols = (c0, c1) of `hb_cols` (None = the same batch; None ranges = all trees; both batches uploaded with their node ranges)
        -> uint64 (r1 - r0, c1 - c0, 5) in PAIR_FIELDS order (pair_columns derives the rest). upper: same batch only; the pairs with
        column index <= row index are skipped and give zeros. Allocates the device buffer, waits for the result and downloads it."""
        import torch
        if hb_cols is None:
            hb_cols = hb_rows
        r0, r1 = rows if rows is not None else (0, self._batch_trees[hb_rows.value])
        c0, c1 = cols if cols is not None else (0, self._batch_trees[hb_cols.value])
        n_r, n_c = max(0, r1 - r0), max(0, c1 - c0)
        buf = torch.empty(max(1, 5 * n_r * n_c), dtype=torch.int64, device=f"cuda:{self.device}")
        self._chk(self.L.qs_tree_pair_agreement(self.h, hb_rows, r0, r1, hb_cols, c0, c1, _lib.QS_PAIRS_UPPER if upper else 0,
                                                C.c_void_p(buf.data_ptr())))
        self.sync()
        return buf[: 5 * n_r * n_c].cpu().numpy().view(np.uint64).reshape(n_r, n_c, 5)

    def _id_list(self, who, ids, limit, dtype=np.uint16):
        """ids (None stays None) -> the contiguous array of unsigned ids the ABI takes, refused before the cast would wrap."""
        if ids is None:
            return None
        wide = np.asarray(ids, dtype=np.int64).reshape(-1)
        if ((wide < 0) | (wide >= limit)).any():
            raise QSError(_lib.QS_ERR_ARG, who + " out of range")
        return np.ascontiguousarray(wide, dtype=dtype)

    def _query(self, ref, words, call) -> np.ndarray:
        """Allocates `words` int64 on the device, runs call(reference struct or None, device address), waits for the result and
        downloads it."""
        import torch
        buf = torch.empty(max(1, words), dtype=torch.int64, device=f"cuda:{self.device}")
        s, keep = self._ref_struct(ref) if ref is not None else (None, None)
        self._chk(call(None if s is None else C.byref(s), buf.data_ptr()))
        self.sync()
        del keep
        return buf[:words].cpu().numpy()

    def _list_query(self, fn, who, ref, taxa, width, extra=0):
        """One of the calls over a list of taxa (None = all, in id order): `width` words per listed taxon and `extra` words behind
        them (their device address is the call's last argument) -> (n_list, the words)."""
        ids = self._id_list(who + ": taxon id", taxa, self.n)
        n_list = self.n if ids is None else len(ids)
        ptr = None if ids is None else ids.ctypes.data_as(C.c_void_p)

        def call(s, p):
            args = (self.h, s, ptr, n_list, C.c_void_p(p))
            return fn(*args, C.c_void_p(p + n_list * width * 8)) if extra else fn(*args)
        return n_list, self._query(ref, n_list * width + extra, call)

    def taxon_support(self, ref: flatten.RefTree) -> np.ndarray:
        """qs_taxon_support: per taxon (lookup id) the six sums of TAXON_FIELDS over the 4-sets of this context's table (whole
        table or shard: add the shards) that hold it -> int64 (n, 6); taxon_columns names and derives the rest. Allocates the
        device buffer, waits for the result and downloads it."""
        return self._query(ref, 6 * self.n, lambda s, p: self.L.qs_taxon_support(self.h, s, C.c_void_p(p))).reshape(self.n, 6)

    def group_support(self, labels) -> np.ndarray:
        """qs_group_support: per hypothesis (labels (n_hyp, n_taxa) in 0..4; parse_group_spec builds them) the six words of
        GROUP_FIELDS over the 4-sets of this context's table (whole table or shard: add the shards) -> int64 (n_hyp, 6);
        group_columns derives the ratios. Needs no reference tree. Allocates the device buffer, waits for the result and
        downloads it."""
        a = _group_labels(self.n, labels)
        return self._query(None, 6 * len(a), lambda s, p: self.L.qs_group_support(self.h, a.ctypes.data_as(C.c_void_p), len(a),
                                                                                    C.c_void_p(p))).reshape(len(a), 6)

    def taxon_placement(self, ref: flatten.RefTree, taxa=None) -> np.ndarray:
        """qs_taxon_placement: per listed taxon (lookup ids; None = all, in id order) the 2 * n_nodes link sums W_x of its
        quartet placement on `ref` from this context's whole table -> int64 (n_list, 2 * n_nodes); placement_scores turns them
        into the score of every edge, placement_columns into the CLI's columns. Allocates the device buffer, waits for the
        result and downloads it."""
        n_list, host = self._list_query(self.L.qs_taxon_placement, "taxon_placement", ref, taxa, 2 * ref.n_nodes)
        return host.reshape(n_list, 2 * ref.n_nodes)

    def taxon_pair_support(self, ref: flatten.RefTree, taxa=None) -> np.ndarray:
        """qs_taxon_pair_support: per listed taxon x (lookup ids; None = all, in id order) and every taxon j the eight words of
        TAXON_PAIR_FIELDS over the 4-sets of this context's whole table that hold both, split by what `ref` shows for the 4-set
        -> int64 (n_list, n, 8); taxon_pair_columns turns them into the CLI's columns. Allocates the device buffer, waits for the
        result and downloads it."""
        n_list, host = self._list_query(self.L.qs_taxon_pair_support, "taxon_pair_support", ref, taxa, 8 * self.n)
        return host.reshape(n_list, self.n, 8)

    def branch_taxon_support(self, ref: flatten.RefTree, taxa=None):
        """qs_branch_taxon_support: per listed taxon x (lookup ids; None = all, in id order) and node v of `ref` the four words of
        BRANCH_TAXON_FIELDS over the 4-sets around the internode above v that hold x, and the same words over all 4-sets around it
        -> (rows int64 (n_list, n_nodes, 4), totals int64 (n_nodes, 4)); QP-IC of the internode without x is log_score of
        (totals - rows[x])[1:4], and drop_one_columns turns both into the CLI's columns. Allocates the device buffers, waits for the
        result and downloads it."""
        width = 4 * ref.n_nodes
        n_list, host = self._list_query(self.L.qs_branch_taxon_support, "branch_taxon_support", ref, taxa, width, extra=width)
        return host[: n_list * width].reshape(n_list, ref.n_nodes, 4), host[n_list * width:].reshape(ref.n_nodes, 4)

    def clade_placement(self, ref: flatten.RefTree, nodes=None) -> np.ndarray:
        """qs_clade_placement: per listed non-root node of `ref` (None = eligible_clades(ref)) the 2 * n_nodes link sums W_C of the
        quartet placement of the clade below it, pruned and regrafted unchanged inside, from this context's whole table -> int64
        (n_list, 2 * n_nodes); placement_scores turns a row into the score of every edge outside the clade (the entries of the
        nodes strictly inside it are not positions, the node's own entry is the current position's score),
        clade_placement_columns into the CLI's columns. Allocates the device buffer, waits for the result and downloads it."""
        ids = self._id_list("clade_placement: node index", eligible_clades(ref) if nodes is None else nodes, ref.n_nodes, np.uint32)
        width = 2 * ref.n_nodes
        return self._query(ref, len(ids) * width, lambda s, p: self.L.qs_clade_placement(
            self.h, s, ids.ctypes.data_as(C.c_void_p) if len(ids) else None, len(ids), C.c_void_p(p))).reshape(len(ids), width)

    def table_clear(self):
        self._chk(self.L.qs_table_clear(self.h))

    def table_download(self) -> np.ndarray:
        dt = np.uint32 if self.count_bits == 32 else np.uint16
        out = np.zeros((max(self.table_tuples, 1), 3), dtype=dt)
        self._chk(self.L.qs_table_download(self.h, out.ctypes.data_as(C.c_void_p), self.table_bytes))
        return out[: self.table_tuples]

    def table_upload(self, arr: np.ndarray):
        arr = np.ascontiguousarray(arr)
        self._chk(self.L.qs_table_upload(self.h, arr.ctypes.data_as(C.c_void_p), arr.nbytes))

    # batches
    @staticmethod
    def _batch_struct(b: flatten.TreeBatch, with_nodes=True):
        s = _lib.TreeBatchC()
        s.n_trees = b.n_trees
        keep = [np.ascontiguousarray(x) for x in (b.leaf_off, b.leaf_ids, b.adj_depth, b.node_off, b.rng_off, b.ranges)]
        s.leaf_off, s.leaf_ids, s.adj_depth = (k.ctypes.data for k in keep[:3])
        if with_nodes:
            s.node_off, s.rng_off, s.ranges = (k.ctypes.data for k in keep[3:])
        return s, keep

    def batch_upload(self, b: flatten.TreeBatch, with_nodes=True):
        s, keep = self._batch_struct(b, with_nodes)
        h = C.c_void_p()
        self._chk(self.L.qs_batch_upload(self.h, C.byref(s), C.byref(h)))
        del keep
        self._batch_trees[h.value] = b.n_trees
        return h

    def batch_flags(self, hb) -> int:
        """_lib.QS_BATCH_ALL_TAXA | _lib.QS_BATCH_BINARY as found by the upload's validation."""
        return int(self.L.qs_batch_flags(hb))

    def batch_free(self, hb):
        self._batch_trees.pop(hb.value, None)
        self.L.qs_batch_free(self.h, hb)

    def count_batch(self, hb, algo=QS_ALGO_AUTO):
        self._chk(self.L.qs_count_batch(self.h, hb, algo))

    def count_trees(self, b: flatten.TreeBatch, algo=QS_ALGO_AUTO):
        s, keep = self._batch_struct(b, True)
        self._chk(self.L.qs_count_trees(self.h, C.byref(s), algo))
        del keep

    def sync(self):
        self._chk(self.L.qs_sync(self.h))

    @property
    def trees_counted(self) -> int:
        return int(self.L.qs_trees_counted(self.h))

    def last_count_ms(self) -> Tuple[float, float, float]:
        out = (C.c_float * 3)()
        self._chk(self.L.qs_last_count_ms(self.h, C.byref(out)))
        return tuple(float(x) for x in out)

    def last_score_ms(self) -> dict:
        """qs_last_score_ms: phases of the most recent score() in ms."""
        out = (C.c_float * 6)()
        self._chk(self.L.qs_last_score_ms(self.h, C.byref(out)))
        keys = ("total", "setup", "pass1", "pass2", "wait_overflow_d2h", "host_finish")
        return {k: float(v) for k, v in zip(keys, out)}

    def last_score_log(self) -> int:
        """Records the last score() logged in single-read mode; 0 = the table was read twice."""
        return int(self.L.qs_last_score_log(self.h))

    def last_score_estimate(self) -> int:
        """Automatic scoring mode: the log size the last score() predicted from its sample; 0 = no estimate ran."""
        return int(self.L.qs_last_score_estimate(self.h))

    def last_count_launches(self) -> int:
        return int(self.L.qs_last_count_launches(self.h))

    def last_count_fix_ms(self) -> float:
        """Share of last_count_ms()[1] spent in the depth-clamp correction kernels (QS_TUNE_DEPTH_CLAMP)."""
        return float(self.L.qs_last_count_fix_ms(self.h))

    def last_count_events(self):
        """[(kind, ms)] of every kernel of the last timed count_batch in launch order; kind: "panel" | "count" | "fix"."""
        ms = (C.c_float * 256)()
        kind = (C.c_uint8 * 256)()
        k = int(self.L.qs_last_count_events(self.h, ms, kind, 256))
        return [(("panel", "count", "fix")[min(int(kind[i]), 2)], float(ms[i])) for i in range(k)]

    def last_count_split(self) -> Tuple[int, int]:
        """(d_mid, slices split there) of the last count_batch (QS_TUNE_FIX_OVERLAP); (0, 0) = every slice was one count launch."""
        k = C.c_uint32(0)
        return int(self.L.qs_last_count_split(self.h, C.byref(k))), int(k.value)

    def batch_clamp_info(self, hb) -> Tuple[int, int, int]:
        """(trees counted in a class below their own depth bits, their (tree, quartet) corrections, correction workgroups)."""
        out = (C.c_uint64 * 3)()
        self._chk(self.L.qs_batch_clamp_info(hb, C.byref(out)))
        return tuple(int(x) for x in out)

    def set_tuning(self, key: int, value: int):
        """qs_set_tuning: _lib.QS_TUNE_PANEL_SLICE_BYTES / QS_TUNE_GATHER_IMPL / QS_TUNE_PANEL_KERNEL (A/B runs, tests)."""
        self._chk(self.L.qs_set_tuning(self.h, key, value))

    def last_count_variant(self) -> str:
        return self.L.qs_last_count_variant(self.h).decode()

    def lookup(self, abcd: np.ndarray) -> np.ndarray:
        q = np.ascontiguousarray(abcd, dtype=np.uint16).reshape(-1, 4)
        out = np.zeros((len(q), 3), dtype=np.uint64)
        self._chk(self.L.qs_lookup(self.h, len(q), q.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)))
        return out

    # scoring
    @staticmethod
    def _ref_struct(ref: flatten.RefTree):
        s = _lib.RefTreeC()
        par = np.ascontiguousarray(ref.parent, dtype=np.int32)
        ln = np.ascontiguousarray(ref.leaf_node, dtype=np.uint32)
        s.n_nodes, s.n_taxa, s.parent, s.leaf_node = ref.n_nodes, ref.n_taxa, par.ctypes.data, ln.ctypes.data
        return s, (par, ln)

    def score(self, ref: flatten.RefTree, flags=QS_SCORE_QP_WRAP32):
        s, keep = self._ref_struct(ref)
        lq = np.zeros(ref.n_nodes); qp = np.zeros(ref.n_nodes); eqp = np.zeros(ref.n_nodes)
        bif = C.c_int(0)
        self._chk(self.L.qs_score(self.h, C.byref(s), flags, lq.ctypes.data_as(C.c_void_p), qp.ctypes.data_as(C.c_void_p),
                                  eqp.ctypes.data_as(C.c_void_p), C.byref(bif)))
        del keep
        return lq, qp, eqp, bool(bif.value)

    def score_prepare(self, ref: flatten.RefTree, n_trees_total: int = 0):
        """qs_score_prepare: the set-up of a first score() ahead of time (allowed while count kernels are in flight)."""
        s, keep = self._ref_struct(ref)
        self._chk(self.L.qs_score_prepare(self.h, C.byref(s), int(n_trees_total)))
        del keep

    # scoring in steps (table shards / multi-GPU); buffers are torch int64 CUDA tensors owned by the caller
    def score_pair_slots(self, ref: flatten.RefTree) -> int:
        s, keep = self._ref_struct(ref)
        return int(self.L.qs_score_pair_slots(C.byref(s)))

    def score_set_view(self, tensor, count_bits: int, rank_lo: int, n_tuples: int):
        """score_pass1/2 read tuples [rank_lo, rank_lo + n_tuples) from `tensor` (torch CUDA tensor; None = own table)."""
        if tensor is None:
            self._chk(self.L.qs_score_set_view(self.h, None, 0, 0, 0))
            self._view = None
            return
        need = n_tuples * 3 * (count_bits // 8)
        if tensor.numel() * tensor.element_size() < need:
            raise ValueError("view tensor smaller than the tuple range")
        self._chk(self.L.qs_score_set_view(self.h, C.c_void_p(tensor.data_ptr()), count_bits, rank_lo, n_tuples))
        self._view = tensor

    def score_pass1(self, ref: flatten.RefTree, sums, mins):
        s, keep = self._ref_struct(ref)
        self._chk(self.L.qs_score_pass1(self.h, C.byref(s), C.c_void_p(sums.data_ptr()), C.c_void_p(mins.data_ptr())))

    def score_pass2(self, ref: flatten.RefTree, mins, cand):
        s, keep = self._ref_struct(ref)
        self._chk(self.L.qs_score_pass2(self.h, C.byref(s), C.c_void_p(mins.data_ptr()), C.c_void_p(cand.data_ptr())))

    def score_overflow(self, ref: flatten.RefTree, mins, cand) -> np.ndarray:
        """qs_score_overflow: (k, 4) int64 rows (key, q1, q2, q3) = every near-minimal quartet of the node pairs whose
        candidate slots did not suffice in score_pass2 (k = 0 almost always)."""
        s, keep = self._ref_struct(ref)
        p = C.c_void_p()
        k = C.c_uint64(0)
        self._chk(self.L.qs_score_overflow(self.h, C.byref(s), C.c_void_p(mins.data_ptr()), C.c_void_p(cand.data_ptr()), C.byref(p), C.byref(k)))
        if not k.value:
            return np.zeros((0, 4), dtype=np.int64)
        try:
            buf = (C.c_int64 * (4 * k.value)).from_address(p.value)
            return np.frombuffer(buf, dtype=np.int64).reshape(-1, 4).copy()
        finally:
            self.L.qs_free_host(p)

    def score_finish(self, ref: flatten.RefTree, sums_host: np.ndarray, cand_host: np.ndarray, flags=QS_SCORE_QP_WRAP32, extra=None):
        """sums_host: int64[3P]; cand_host: int64[parts, 8P] (gathered over the shards); extra: (k, 4) rows of
        score_overflow (concatenated over the shards) or None."""
        return score_finish_host(ref, sums_host, cand_host, flags, extra=extra, _ctx=self)

    def raw_qic(self, ref: flatten.RefTree, r0: int, nq: int, lex: bool = False):
        """topology + count triple of nq quartets from rank r0 on (lex=False) or from the r0-th 4-subset in lexicographic
        order of the sorted ids on (lex=True: the reference's -q line order)."""
        s, keep = self._ref_struct(ref)
        topo = np.zeros(nq, dtype=np.uint8)
        q = np.zeros((nq, 3), dtype=np.uint64)
        f = self.L.qs_raw_qic_lex if lex else self.L.qs_raw_qic
        self._chk(f(self.h, C.byref(s), r0, nq, topo.ctypes.data_as(C.c_void_p), q.ctypes.data_as(C.c_void_p)))
        del keep
        return topo, q


def score_finish_host(ref: flatten.RefTree, sums_host: np.ndarray, cand_host: np.ndarray, flags=QS_SCORE_QP_WRAP32, extra=None, _ctx=None):
    """qs_score_finish: pure host arithmetic on the reduced per-node-pair sums and the gathered candidates (no device
    needed; `_ctx` only lends its cached reference tree). sums_host: int64[3P]; cand_host: int64[parts, 8P]."""
    L = _lib.load()
    s, keep = Context._ref_struct(ref)
    sums_host = np.ascontiguousarray(sums_host, dtype=np.int64)
    cand_host = np.ascontiguousarray(cand_host, dtype=np.int64)
    parts = cand_host.size // (_lib.QS_SCORE_CAND_SLOTS * (sums_host.size // 3))
    lq = np.zeros(ref.n_nodes); qp = np.zeros(ref.n_nodes); eqp = np.zeros(ref.n_nodes)
    bif = C.c_int(0)
    h = _ctx.h if _ctx is not None else None
    ex = np.ascontiguousarray(extra, dtype=np.int64).reshape(-1, 4) if extra is not None and len(extra) else None
    rc = L.qs_score_finish(h, C.byref(s), flags, sums_host.ctypes.data_as(C.c_void_p), cand_host.ctypes.data_as(C.c_void_p), parts,
                           ex.ctypes.data_as(C.c_void_p) if ex is not None else None, len(ex) if ex is not None else 0,
                           lq.ctypes.data_as(C.c_void_p), qp.ctypes.data_as(C.c_void_p), eqp.ctypes.data_as(C.c_void_p), C.byref(bif))
    if rc != 0:
        raise QSError(rc, L.qs_last_error(h).decode())
    del keep
    return lq, qp, eqp, bool(bif.value)


def _read_eval(eval_trees) -> List[str]:
    """evalTreesPath of the reference: a file of ';'-terminated Newick trees. A list of
    Newick strings is accepted as well (tests)."""
    if isinstance(eval_trees, (str, os.PathLike)) and os.path.exists(str(eval_trees)):
        with open(eval_trees) as f:
            return [f.read()]
    if isinstance(eval_trees, str):
        return [eval_trees]
    return list(eval_trees)


class QuartetCounterLookup:
    """QuartetCounterLookup<CINT>(refTree, evalTreesPath, m, savemem) -- counting happens in the
    constructor (QuartetCounterLookup.hpp:245-273). `savemem` is accepted and ignored: the GPU
    table is always the compact C(n,4)x3 layout and holds semantic (1x) counts."""

    def __init__(self, refTree: Union[str, flatten.RefTree], evalTreesPath, m: Optional[int] = None, savemem: bool = False,
                 *, count_bits: Optional[int] = None, device: int = 0, stream: int = 0, algo: int = QS_ALGO_AUTO,
                 batch_trees: int = 4096, table_tensor=None, species_map=None):
        self.ref = refTree if isinstance(refTree, flatten.RefTree) else flatten.flatten_reference(refTree)
        texts = _read_eval(evalTreesPath)
        # species_map ({species: [individuals]} or the text of a map file): the evaluation trees' leaves are individuals; count
        # under their ids, then collapse into the species' table (qs_table_collapse) and let the individuals' table go
        layout = None
        if species_map is not None and table_tensor is not None:
            raise ValueError("table_tensor and species_map do not go together: the tensor would hold the individuals' table, and the species' "
                             "table that takes its place is the context's own")
        if species_map is not None:
            layout = flatten.species_layout(self.ref, flatten.parse_species_map(species_map) if isinstance(species_map, str) else species_map)
        name_to_id = layout.name_to_id if layout else self.ref.name_to_id
        batch = flatten.flatten_eval_trees(texts, name_to_id)  # raises UnknownTaxonError like QCL:218
        self.m = batch.n_trees if m is None else m
        self.savemem = savemem
        bits = count_bits or count_bits_for(self.m)
        self.ctx = Context(len(name_to_id), bits, device, stream)
        if table_tensor is not None:
            self.ctx.table_attach(table_tensor)
            self.ctx.table_clear()
        else:
            self.ctx.table_alloc()
        for lo in range(0, batch.n_trees, batch_trees):
            hi = min(batch.n_trees, lo + batch_trees)
            self.ctx.count_trees(batch.slice(lo, hi) if (lo, hi) != (0, batch.n_trees) else batch, algo)
        if layout:
            sizes = np.sort(np.diff(layout.first_id.astype(np.int64)))[-4:]
            species = Context(self.ref.n_taxa, 16 if bits == 16 and self.m * int(np.prod(sizes)) < 65536 else 32, device, stream)
            species.table_alloc()
            species.table_collapse(self.ctx, layout.first_id)
            species.sync()   # (a sum beyond 32 bits raises here)
            self.ctx.close()
            self.ctx = species
        # "lookup table size in bytes: ..." (QuartetCounterLookup.hpp:268-272)
        self.lookup_table_bytes = self.ctx.table_bytes
        self._node_to_lookup = {int(v): i for i, v in enumerate(self.ref.leaf_node)}

    def countQuartetOccurrences(self, aIdx: int, bIdx: int, cIdx: int, dIdx: int) -> Tuple[int, int, int]:
        """Arguments are reference-tree NODE indices (QuartetCounterLookup.hpp:299-318)."""
        ids = [self._node_to_lookup[x] for x in (aIdx, bIdx, cIdx, dIdx)]
        r = self.ctx.lookup(np.array(ids, dtype=np.uint16))[0]
        return int(r[0]), int(r[1]), int(r[2])

    def table(self) -> np.ndarray:
        return self.ctx.table_download()


def score_check(ref: flatten.RefTree, flags: int) -> None:
    """qs_score_check without a context (host-only): raises the QSError qs_score would end with for reasons of the reference tree
    alone -- QS_ERR_REFERENCE_THROWS for QS_SCORE_SAVEMEM_LOOKUPS with a rooted reference tree."""
    L = _lib.load()
    parent = np.ascontiguousarray(ref.parent, dtype=np.int32)
    leaf_node = np.ascontiguousarray(ref.leaf_node, dtype=np.uint32)
    s = _lib.RefTreeC(ref.n_nodes, ref.n_taxa, parent.ctypes.data, leaf_node.ctypes.data)
    rc = L.qs_score_check(None, C.byref(s), flags)
    if rc != 0:
        raise QSError(rc, L.qs_last_error(None).decode())


class QuartetScoreComputer:
    """QuartetScoreComputer<CINT>(refTree, evalTreesPath, m, verboseOutput, enforceSmallMem): does
    all the work in its constructor (QuartetScoreComputer.hpp:698-785). Scores are indexed by
    edge; edge e is the edge above node e+1 of the reference tree in preorder."""

    def __init__(self, refTree: Union[str, flatten.RefTree], evalTreesPath, m: Optional[int] = None, verboseOutput: bool = False,
                 enforceSmallMem: bool = False, *, qp_exact64: bool = False, root_as_edge: bool = False, fail_fast: bool = False, log=None, **kw):
        self.ref = refTree if isinstance(refTree, flatten.RefTree) else flatten.flatten_reference(refTree)
        say = log or (lambda s: None)
        n = self.ref.n_taxa
        score_flags = ((QS_SCORE_QP_EXACT64 if qp_exact64 else QS_SCORE_QP_WRAP32) | (QS_SCORE_ROOT_AS_EDGE if root_as_edge else 0) |
                       (QS_SCORE_SAVEMEM_LOOKUPS if enforceSmallMem else 0))
        # what the scoring would refuse because of the reference tree alone (`-s` + a rooted reference: the reference program
        # throws there, after it has counted) is known now. Like the CLI (QuartetScores.cpp: a note, then the reference's order of
        # events): say so, count, and let the scoring raise; fail_fast=True (the CLI's --fail-fast) raises before the counting
        try:
            score_check(self.ref, score_flags)
        except QSError as e:
            if fail_fast or e.code != _lib.QS_ERR_REFERENCE_THROWS:
                raise
            say("note: the scoring of this reference tree will end with the reference's exception (-s with a rooted reference tree); counting first, like the reference")
        self.quartetCounterLookup = QuartetCounterLookup(self.ref, evalTreesPath, m, enforceSmallMem, **kw)
        say(f"There are {self.quartetCounterLookup.m} evaluation trees.")
        say(f"The reference tree has {n} taxa.")
        say(f"lookup table size in bytes: {self.quartetCounterLookup.lookup_table_bytes}")
        say("Finished counting quartets.")
        ctx = self.quartetCounterLookup.ctx
        # root_as_edge: a degree-2 root as a subdivision of one edge instead of the reference's handling (quirk Q5)
        # enforceSmallMem (`-s`): the reference's compact table behind the lookups of a degree-2 root's node pairs -- it throws
        # there (quartet_lookup_table.hpp:79-85), and so does this constructor (QSError, code QS_ERR_REFERENCE_THROWS)
        lq, qp, eqp, bif = ctx.score(self.ref, score_flags)
        self.bifurcating = bif
        say("The reference tree is bifurcating." if bif else "The reference tree is multifurcating.")
        self._lq, self._qp, self._eqp = lq[1:], (qp[1:] if bif else None), (eqp[1:] if bif else None)
        say("Finished computing scores.")

    def getLQICScores(self) -> List[float]:
        return list(self._lq)

    def getQPICScores(self) -> List[float]:
        return [] if self._qp is None else list(self._qp)

    def getEQPICScores(self) -> List[float]:
        return [] if self._eqp is None else list(self._eqp)

    def edge_leafset(self, e: int) -> frozenset:
        """Taxon names below edge e (the child side)."""
        node = self.ref.nodes[e + 1]
        return frozenset(x.name for x in newick.preorder(node) if x.is_leaf)

    def scores_by_bipartition(self):
        """{canonical side: (lq, qp, eqp)} for internal edges, keyed like tests/oracle_api.py."""
        names = self.ref.names
        out = {}
        for e in range(self.ref.n_nodes - 1):
            below = self.edge_leafset(e)
            if len(below) <= 1 or len(below) >= len(names) - 1:
                continue
            other = frozenset(names) - below
            key = below if (len(below) < len(other) or (len(below) == len(other) and min(names) not in below)) else other
            val = (self._lq[e], None if self._qp is None else self._qp[e], None if self._eqp is None else self._eqp[e])
            while key in out:
                key = frozenset(list(key) + ["#dup"])
            out[key] = val
        return out

    def printRawQICScores(self, rawPath: str, chunk: int = 1 << 20):
        """-q file: "(a,b|c,d): qic" per quartet resolved in the reference, in the reference's own line order: four
        nested loops over its Euler-tour leaves = lexicographic in the sorted lookup ids
        (QuartetScoreComputer.hpp:626-690). QIC via the host libm; %g like operator<<(double)."""
        import itertools
        ctx = self.quartetCounterLookup.ctx
        names = self.ref.names
        total = ctx.table_tuples
        combos = itertools.combinations(range(len(names)), 4)     # lexicographic
        with open(rawPath, "w") as f:
            for r0 in range(0, total, chunk):
                nq = min(chunk, total - r0)
                topo, q = ctx.raw_qic(self.ref, r0, nq, lex=True)
                for i in range(nq):
                    a, b, c, d = next(combos)
                    t = topo[i]
                    if t == 255:
                        continue
                    if t == 0:
                        lab = (names[a], names[b], names[c], names[d])
                    else:
                        lab = (names[a], names[d], names[b], names[c])
                    f.write("(%s,%s|%s,%s): %g\n" % (lab + (log_score(int(q[i, 0]), int(q[i, 1]), int(q[i, 2])),)))


def log_score(q1: int, q2: int, q3: int) -> float:
    """QuartetScoreComputer.hpp:135-159 with the host libm (C doubles via math.log)."""
    if q1 == 0 and q2 == 0 and q3 == 0:
        return 0.0
    s = q1 + q2 + q3
    p1, p2, p3 = q1 / s, q2 / s, q3 / s
    qic = 1.0
    if p1 != 0:
        qic += p1 * math.log(p1) / math.log(3)
    if p2 != 0:
        qic += p2 * math.log(p2) / math.log(3)
    if p3 != 0:
        qic += p3 * math.log(p3) / math.log(3)
    return qic * -1 if (q1 < q2 or q1 < q3) else qic
