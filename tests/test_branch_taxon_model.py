"""Per-branch quartet sums through every taxon without a GPU: the numpy model of qs_branch_taxa.hip (tests/branch_taxon_model.py)
against an independent statement in taxon groups (tests/group_model.py), the closed form of the number of 4-sets, and the lines.

The statement: the 4-sets around an internode take one taxon behind each of two different links at either end, so for two links
A, B at one end and C, D at the other the quad hypothesis A B | C D of group_model counts exactly the 4-sets around the internode
through that link pair, and with x's label set to 0 those among them that do not hold x. Summed over the link pairs that is
totals - row(x). The labels 1..4 follow the cyclic order of the lookup ids, the frame in which qs_score puts the crossing pairing
into q2 under a bifurcating reference; under a multifurcating one its argument order (frame 1) exchanges the two discordant
counts depending on where a 4-set wraps around the id order, so only their sum is a statement about groups there."""
import itertools

import numpy as np

import branch_taxon_model as M
import bruteforce
import group_model
from helpers import binom
from quartetscores_amd import flatten, synth
from test_taxon_pair_model import random_cases


def test_model_against_group_hypotheses_and_the_closed_form():
    cases = binary = multi = rooted = dissolved = 0
    for n, ref_nw, trees in random_cases(36, 41):
        ref = flatten.flatten_reference(ref_nw)
        table = bruteforce.count_table(ref.names, trees)
        rows, totals = M.model(table, ref)
        assert rows.dtype == np.int64 and rows.shape == (n, ref.n_nodes, 4) and totals.shape == (ref.n_nodes, 4)
        edges = M.internodes(ref)
        on = np.zeros(ref.n_nodes, dtype=bool)
        on[[v for v, _ in edges]] = True
        assert not totals[~on].any() and not rows[:, ~on].any()
        assert (totals[:, 0] == M.closed_form_quartets(ref)).all()
        assert (rows.sum(axis=0) == 4 * totals).all()          # every 4-set holds four taxa
        bif = M.is_bifurcating(ref)
        for v, w in edges:
            ends = [M.links_at(ref, v, w), M.links_at(ref, w, v)]
            assert all(len(e) >= 2 for e in ends)
            for x in range(n):
                want = np.zeros(4, dtype=object)
                for (a, b), (c, d) in itertools.product(itertools.combinations(ends[0], 2), itertools.combinations(ends[1], 2)):
                    row = M.cyclic_labels(n, ((a, b), (c, d)))
                    row[x] = 0
                    if group_model.kind_of(row) != 0:
                        continue                                # x was alone in its link: no 4-set of this link pair is left
                    want += group_model.model_counts(table, row[None, :], n)[0][:4]
                got = totals[v] - rows[x, v]
                if bif:
                    assert [int(z) for z in got] == [int(z) for z in want], (ref_nw, v, x)
                else:
                    assert (int(got[0]), int(got[1]), int(got[2] + got[3])) == (int(want[0]), int(want[1]), int(want[2] + want[3])), (ref_nw, v, x)
                dissolved += int(got[0] == 0)
        cases += 1
        rooted += int(bool(edges) and any(ref.parent[v] != w for v, w in edges))
        binary += int(bif and bool(edges))
        multi += int(not bif and bool(edges))
    assert cases >= 30 and binary and multi and rooted and dissolved


def test_words_by_hand():
    # five taxa, ((a,b),c,(d,e)): two internodes; the 4-sets in rank order are abcd abce abde acde bcde
    ref = flatten.flatten_reference("((a,b),c,(d,e));")
    assert ref.names == ["a", "b", "c", "d", "e"]
    table = np.array([[5, 1, 0], [4, 0, 2], [7, 0, 0], [1, 1, 6], [0, 3, 3]])
    rows, totals = M.model(table, ref)
    (v_ab, _), (v_de, _) = M.internodes(ref)
    assert (ref.leaf_node[:2] != v_ab).all() and ref.parent[ref.leaf_node[0]] == v_ab
    # around the edge above (a,b): abcd and abce, both ab|..: the cells as they stand; abde has its junctions two edges apart and
    # counts for neither; around the edge above (d,e): acde and bcde
    assert totals[v_ab].tolist() == [2, 9, 1, 2] and totals[v_de].tolist() == [2, 1, 4, 9]
    assert rows[2, v_ab].tolist() == [2, 9, 1, 2] and rows[0, v_ab].tolist() == [2, 9, 1, 2] and rows[3, v_ab].tolist() == [1, 5, 1, 0]
    assert rows[3, v_de].tolist() == [2, 1, 4, 9] and rows[0, v_de].tolist() == [1, 1, 1, 6]
    assert (M.closed_form_quartets(ref) == totals[:, 0]).all()
    lines = M.columns(ref, [3, 0], rows[[3, 0]], totals)
    assert len(lines) == 4 and lines[0][:10] == (3, "d", v_ab, 0, 2, 2, 1, 5, 1, 0)
    assert lines[0][10] == "%.6f" % M.log_score(9, 1, 2) and lines[0][11] == "%.6f" % M.log_score(4, 0, 2)
    assert lines[0][12] == "%.6f" % (M.log_score(4, 0, 2) - M.log_score(9, 1, 2))
    assert lines[2][:6] == (0, "a", v_ab, 0, 2, 1) and lines[2][11:] == ("nan", "nan")     # a alone in its link: the edge dissolves
    assert lines[3][:6] == (0, "a", v_de, 3, 5, 2) and lines[3][11] == "%.6f" % M.log_score(0, 3, 3)


def test_the_plan_counts_every_resolved_adjacent_4_set_once():
    rng = np.random.default_rng(8)
    ref = flatten.flatten_reference(synth.random_tree(12, rng))
    quads, ranks, child, second, cols = M.plan(ref)
    assert len(ranks) == len(set(ranks.tolist())) and (second < 0).all() and int(binom(12, 4)) > len(ranks) > 0
    assert sorted(set(child.tolist())) == sorted(v for v, _ in M.internodes(ref))
