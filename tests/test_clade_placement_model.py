"""Quartet placement of clades without a GPU: the numpy model (tests/clade_placement_model.py) against a brute force that prunes the
clade and re-inserts its subtree on every edge of the pruned reference tree, the closed form for a constant table, the derived
columns on a planted clade, and engine.eligible_clades / engine.clade_placement_columns against the model."""
import numpy as np
import pytest

import bruteforce
import clade_placement_model as CM
import placement_model as P
from quartetscores_amd import engine, flatten, synth
from test_placement_model import random_cases


@pytest.fixture(scope="module")
def cases():
    """(reference, table, nodes, link sums, scores) of the random cases, computed once: every non-root node with at least three
    taxa outside it, leaves included"""
    out = []
    for n, ref_nw, trees in random_cases(80, 53):
        ref = flatten.flatten_reference(ref_nw)
        table = bruteforce.count_table(ref.names, trees).astype(np.int64)
        S = P.Shape(ref)
        nodes = [v for v in range(S.N) if v != S.root and n - (S.hi[v] - S.lo[v]) >= 3]
        links = CM.link_sums(table, ref, nodes)
        out.append((ref_nw, ref, table, nodes, links, P.scores(ref, links)))
    return out


def test_model_matches_the_brute_force_regrafting(cases):
    checked = inner = moved = multi = 0
    for ref_nw, ref, table, nodes, links, sc in cases:
        S = P.Shape(ref)
        multi += int((S.links > 3).any())
        every_taxon = P.link_sums(table, ref)
        for row, c in enumerate(nodes):
            lo, hi = int(S.lo[c]), int(S.hi[c])
            want, _rest = CM.brute_scores(ref, table, c)       # (asserts that the rest of the score is the same at every position)
            keys = CM.position_keys(S, c)
            seen = set()
            for v in range(S.N):
                if keys[v] is None or keys[v] == (0, 0):
                    continue
                assert int(sc[row, v]) == want[keys[v]], (ref_nw, c, v)
                seen.add(keys[v])
            assert seen == set(want), (ref_nw, c)               # every edge of the pruned tree is a position outside the clade
            checked += len(seen)
            # all links into and out of the clade's own nodes are 0 (its own edge is a link of its parent)
            own = [v for v in range(S.N) if S.lo[v] >= lo and S.hi[v] <= hi]
            assert not links[row, [S.N + v for v in own]].any() and not links[row, [v for v in own if v != c]].any(), (ref_nw, c)
            if hi - lo == 1:
                assert (links[row] == every_taxon[lo]).all(), (ref_nw, c)   # a one-leaf clade: the taxon's row
            else:
                inner += 1
                moved += int(sc[row][[v for v in range(S.N) if keys[v] is not None]].max() > sc[row, c])
    assert len(cases) >= 40 and checked > 5000 and inner > 150 and moved and multi >= 6


def test_edges_with_the_same_bipartition_score_equal(cases):
    for ref_nw, ref, table, nodes, links, sc in cases:
        S = P.Shape(ref)
        for row, c in enumerate(nodes):
            by_key = {}
            for v, k in enumerate(CM.position_keys(S, c)):
                if k is not None:
                    by_key.setdefault(k, set()).add(int(sc[row, v]))
            assert all(len(vals) == 1 for vals in by_key.values()), (ref_nw, c)


@pytest.mark.parametrize("kw", [{}, {"collapse": 0.4}, {"rooted": True}, {"collapse": 1.0}])
def test_constant_table_closed_form(kw):
    n = 11
    ref = flatten.flatten_reference(synth.random_tree(n, np.random.default_rng(7), **kw))
    table = np.full((len(bruteforce.rank_order_quads(n)), 3), 5, dtype=np.int64)
    S = P.Shape(ref)
    nodes = [v for v in range(S.N) if v != S.root and n - (S.hi[v] - S.lo[v]) >= 3]
    assert len(nodes) >= n
    for c in nodes:
        assert (CM.constant_links(ref, c, 5) == CM.clade_link_sums(table, ref, c)).all(), c


def test_eligible_clades_and_columns_of_engine_equal_the_model(cases):
    assert engine.CLADE_PLACEMENT_COLUMNS == CM.COLUMNS
    for ref_nw, ref, table, nodes, links, sc in cases:
        assert list(engine.eligible_clades(ref)) == CM.eligible(ref), ref_nw
        assert set(CM.eligible(ref)) <= set(nodes)
        got, want = engine.clade_placement_columns(ref, nodes, sc), CM.columns(ref, nodes, sc)
        assert list(got) == list(CM.COLUMNS)
        for k in CM.COLUMNS:
            assert list(got[k]) == list(want[k]), (ref_nw, k)
        assert (got["gain"] >= 0).all() and ((got["distance"] == 0) | (got["gain"] > 0)).all()   # only a better position is away


def test_planted_clade():
    ref_nw, trees, true_side, moved = CM.planted()
    assert moved >= 3
    ref = flatten.flatten_reference(ref_nw)
    table = bruteforce.count_table(ref.names, trees)
    S = P.Shape(ref)
    ids = sorted(ref.name_to_id[x] for x in ("ca", "cb", "cc"))
    c = next(v for v in range(S.N) if (S.lo[v], S.hi[v]) == (ids[0], ids[-1] + 1))
    right = [ref.name_to_id[x] for x in ("o8", "o9", "o10")]
    ok = next(v for v in range(S.N) if (S.lo[v], S.hi[v]) == (min(right), max(right) + 1))   # a clade that every tree has where the reference has it
    nodes = [c, ok]
    cols = CM.columns(ref, nodes, P.scores(ref, CM.link_sums(table, ref, nodes)))
    assert cols["size"][0] == 3 and cols["n_best"][0] == 1 and cols["gain"][0] > 0 and cols["distance"][0] == moved
    assert cols["best"][0] == 7 * 3 * (11 * 10 * 9 // 6)          # every quartet with one taxon of the clade, in every tree
    below = {ref.names[i] for i in range(cols["best_lo"][0], cols["best_hi"][0])} - {"ca", "cb", "cc"}
    assert below == true_side                                      # the true bipartition
    assert cols["gain"][1] == 0 and cols["distance"][1] == 0 and cols["best_node"][1] == S.parent[ok]   # the three edges at its parent are one position
    got = engine.clade_placement_columns(ref, nodes, P.scores(ref, CM.link_sums(table, ref, nodes)))
    assert all(list(got[k]) == list(cols[k]) for k in CM.COLUMNS)
