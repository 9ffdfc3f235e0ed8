"""tests/tree_branch_model.py (the closed forms of qs_tree_branch_support over node pairs) against the per-4-set brute force:
bruteforce.count_table of one tree alone through branch_taxon_model.model(...)[1], word 0 restricted to the tree's taxa."""
import numpy as np
import pytest

import branch_taxon_model as BM
import bruteforce
import tree_branch_model as TB
from quartetscores_amd import flatten, synth
from tree_branch_model import REF_KINDS, mixed_trees


def brute(ref, tree, the_plan):
    """branch_taxon_model.model of the tree's own table; word 0 (all 4-sets around the internode) cut down to those inside P_t"""
    table = bruteforce.count_table(ref.names, [tree])
    want = BM.model(table, ref, the_plan)[1]
    masked = TB.brute_rows(ref, tree, the_plan, table)
    assert (masked[:, 1:] == want[:, 1:]).all() and (masked[:, 0] <= want[:, 0]).all()
    return masked


@pytest.mark.parametrize("ref_kind", sorted(REF_KINDS))
@pytest.mark.parametrize("n", [5, 6, 9, 17, 30])
def test_model_matches_brute_force(ref_kind, n):
    rng = np.random.default_rng(1000 * n + sorted(REF_KINDS).index(ref_kind))
    ref = flatten.flatten_reference(synth.random_tree(n, rng, **REF_KINDS[ref_kind]))
    if ref_kind in ("binary", "rooted") or n >= 9:       # both frames are covered (a collapsed small tree may stay binary)
        assert BM.is_bifurcating(ref) == (ref_kind in ("binary", "rooted"))
    the_plan, the_items = BM.plan(ref), TB.items(ref)
    for t in mixed_trees(n, rng, 12 if n < 30 else 6):
        got = TB.model_tree(ref, t, the_items=the_items)
        want = brute(ref, t, the_plan)
        assert (got == want).all(), (ref_kind, n, t, np.nonzero((got != want).any(1))[0])
        if ref_kind == "star":
            assert not got.any()
        assert (TB.model_tree(ref, t, recentre=False, the_items=the_items) == got).all()


def test_full_tree_present_is_closed_form():
    rng = np.random.default_rng(5)
    ref_nw = synth.random_tree(14, rng, collapse=0.3)
    ref = flatten.flatten_reference(ref_nw)
    got = TB.model_tree(ref, ref_nw)
    assert (got[:, 0] == BM.closed_form_quartets(ref)).all()
    assert (got[:, 1] == got[:, 0]).all() and not got[:, 2:].any()   # the reference agrees with itself around every internode


def test_engine_columns():
    """engine.tree_branch_columns and engine.bootstrap_columns on the model's rows: the lines left out, the root edge once, the
    percentile indices"""
    from quartetscores_amd import engine
    rng = np.random.default_rng(8)
    for kw in ({"rooted": True}, {"collapse": 0.3}):
        ref = flatten.flatten_reference(synth.random_tree(12, rng, **kw))
        trees = mixed_trees(12, rng, 12)
        rows = np.array([TB.model_tree(ref, t) for t in trees])
        edges = [v for v, w in BM.internodes(ref) if not (ref.parent[v] != w and ref.parent[w] == ref.parent[v] and v > w)]
        cols = engine.tree_branch_columns(ref, rows, first_tree=100)
        assert list(cols) == list(engine.TREE_BRANCH_COLUMNS)
        want = [(100 + t, v) for t in range(len(trees)) for v in edges if rows[t, v, 0] > 0]
        assert list(zip(cols["tree"].tolist(), cols["node"].tolist())) == want and 0 < len(want) < len(trees) * len(edges)
        for i, (t, v) in enumerate(want):
            p, q1, q2, q3 = rows[t - 100, v].tolist()
            assert (cols["present"][i], cols["q1"][i], cols["q2"][i], cols["q3"][i]) == (p, q1, q2, q3)
            assert (np.isnan(cols["concordance"][i]) and q1 + q2 + q3 == 0) or cols["concordance"][i] == q1 / (q1 + q2 + q3)
        # B = 41 replicates with distinct scores: replicate r holds (41 + r, 41 - r, 0) at every internode
        B = 41
        reps = np.zeros((B, ref.n_nodes, 4), dtype=np.int64)
        for r in range(B):
            reps[r, :, 1], reps[r, :, 2] = 41 + r, 41 - r
        boot = engine.bootstrap_columns(ref, rows.sum(0), reps)
        assert list(boot) == list(engine.BOOTSTRAP_COLUMNS) and boot["node"].tolist() == edges and (boot["reps"] == B).all()
        vals = sorted(BM.log_score(41 + r, 41 - r, 0) for r in range(B))
        assert (boot["lo95"] == vals[1]).all() and (boot["hi95"] == vals[39]).all()          # floor(0.025 x 40), ceil(0.975 x 40)
        assert np.allclose(boot["mean"], np.mean(vals), rtol=0, atol=1e-12) and np.allclose(boot["sd"], np.std(vals), rtol=0, atol=1e-12)
        total = rows.sum(0)
        assert boot["qpic"].tolist() == [BM.log_score(*total[v, 1:].tolist()) for v in edges]
        same = engine.bootstrap_columns(ref, total, np.repeat(total[None], 7, axis=0))
        assert np.allclose(same["mean"], same["qpic"], rtol=0, atol=1e-15) and (same["sd"] < 1e-15).all()
