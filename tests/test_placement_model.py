"""Quartet placement without a GPU: the numpy model (tests/placement_model.py) against a brute force that re-inserts the taxon
on every edge of the pruned reference tree, the two identities with the per-taxon support, the host-only qs_placement_scores,
the derived columns on a planted misplacement, and the refusals of QuartetScores --place-taxa."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bruteforce
import placement_model as P
import taxon_model as M
from quartetscores_amd import _lib, engine, flatten, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "quartetscores_amd", "bin", "QuartetScores")


def random_cases(count, seed):
    """5-10 taxa; binary, collapsed (up to a star) and rooted references; evaluation trees with dropout and collapsed edges"""
    rng = np.random.default_rng(seed)
    for i in range(count):
        n = int(rng.integers(5, 11))
        ref_kw = [{}, {"collapse": 0.3}, {"rooted": True}, {"collapse": 1.0}, {"rooted": True, "collapse": 0.5}, {"collapse": 0.7}][i % 6]
        ref_nw = synth.random_tree(n, rng, **ref_kw)
        trees = []
        for k in range(int(rng.integers(2, 8))):
            ev_kw = [{}, {"collapse": float(rng.uniform(0.1, 0.9))}, {"dropout": float(rng.uniform(0.1, 0.5)), "min_taxa": 4},
                     {"rooted": True}, {"rooted": True, "collapse": 0.3, "dropout": 0.3}][(i + k) % 5]
            trees.append(synth.random_tree(n, rng, **ev_kw))
        yield n, ref_nw, trees


@pytest.fixture(scope="module")
def cases():
    """(reference, table, link sums, scores) of the random cases, computed once"""
    out = []
    for n, ref_nw, trees in random_cases(42, 31):
        ref = flatten.flatten_reference(ref_nw)
        table = bruteforce.count_table(ref.names, trees).astype(np.int64)
        links = P.link_sums(table, ref)
        out.append((ref_nw, ref, table, links, P.scores(ref, links)))
    return out


def test_model_matches_the_brute_force_reinsertion(cases):
    checked = moved = multi = 0
    for ref_nw, ref, table, links, sc in cases:
        S = P.Shape(ref)
        multi += int((S.links > 3).any())
        for x in range(ref.n_taxa):
            want = P.brute_scores(ref_nw, ref.names, table, x)
            keys = P.position_keys(S, x)
            seen = set()
            for v in range(S.N):
                if v == S.root or keys[v] == (0, 0):
                    continue
                assert int(sc[x, v]) == want[keys[v]], (ref_nw, x, v)
                seen.add(keys[v])
            assert seen == set(want), (ref_nw, x)              # every edge of the pruned tree is a position of the full tree
            checked += len(seen)
            moved += int(sc[x].max() > sc[x, ref.leaf_node[x]])
    assert len(cases) >= 36 and checked > 1000 and moved and multi >= 6


def test_identities_with_the_per_taxon_support(cases):
    for ref_nw, ref, table, links, sc in cases:
        support = M.model_counts(table, ref)
        own = sc[np.arange(ref.n_taxa), ref.leaf_node.astype(np.int64)]
        assert (own == support[:, 1]).all(), ref_nw                                   # current = concordant
        assert (links.sum(axis=1) == support[:, 1:4].sum(axis=1)).all(), ref_nw       # every triple has a median
        assert (links >= 0).all() and (sc >= 0).all()


def test_edges_with_the_same_bipartition_score_equal(cases):
    shared = 0
    for ref_nw, ref, table, links, sc in cases:
        S = P.Shape(ref)
        for x in range(ref.n_taxa):
            by_key = {}
            for v, k in enumerate(P.position_keys(S, x)):
                if k is not None:
                    by_key.setdefault(k, set()).add(int(sc[x, v]))
                    shared += 1
            assert all(len(vals) == 1 for vals in by_key.values()), (ref_nw, x)
            shared -= len(by_key)
    assert shared > 100                                                                # edges beyond the first of their position


def ref_struct(ref, parent=None):
    s = _lib.RefTreeC()
    par = np.ascontiguousarray(ref.parent if parent is None else parent, dtype=np.int32)
    ln = np.ascontiguousarray(ref.leaf_node, dtype=np.uint32)
    s.n_nodes, s.n_taxa, s.parent, s.leaf_node = len(par), ref.n_taxa, par.ctypes.data, ln.ctypes.data
    return s, (par, ln)


def test_host_entry_point_equals_the_model_and_refuses_a_malformed_tree(cases):
    L = _lib.load()          # host-only: no device is touched
    for ref_nw, ref, table, links, sc in cases:
        assert (engine.placement_scores(ref, links) == sc).all(), ref_nw
    ref_nw, ref, table, links, sc = cases[0]
    # a numbering in which parents come after their children gives the same scores per node
    N = ref.n_nodes
    back = np.arange(N)[::-1]
    flipped = flatten.RefTree(ref.root, ref.nodes[::-1], np.where(ref.parent[::-1] >= 0, N - 1 - ref.parent[::-1], -1).astype(np.int32),
                              (N - 1 - ref.leaf_node).astype(np.uint32), ref.names, ref.name_to_id)
    W = np.concatenate([links[:, :N][:, back], links[:, N:][:, back]], axis=1)
    assert (engine.placement_scores(flipped, W) == sc[:, back]).all()
    out = np.zeros(N, dtype=np.int64)
    row = np.ascontiguousarray(links[0])
    for bad in (np.full(N, -1), np.where(np.arange(N) == 1, 1, ref.parent), np.zeros(N)):   # two roots, its own parent, no root
        s, keep = ref_struct(ref, bad)
        assert L.qs_placement_scores(C.byref(s), row.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)) == _lib.QS_ERR_ARG
        assert b"reference tree" in L.qs_last_error(None)
    s, keep = ref_struct(ref)
    assert L.qs_placement_scores(C.byref(s), None, out.ctypes.data_as(C.c_void_p)) == _lib.QS_ERR_ARG
    assert L.qs_placement_scores(C.byref(s), row.ctypes.data_as(C.c_void_p), None) == _lib.QS_ERR_ARG
    with pytest.raises(engine.QSError):
        engine.placement_scores(flatten.RefTree(ref.root, ref.nodes, np.full(N, -1, dtype=np.int32), ref.leaf_node, ref.names, ref.name_to_id), links)


def test_columns_of_engine_equal_the_model(cases):
    assert engine.PLACEMENT_COLUMNS == P.COLUMNS
    for ref_nw, ref, table, links, sc in cases:
        taxa = list(range(ref.n_taxa))
        got, want = engine.placement_columns(ref, taxa, sc), P.columns(ref, taxa, sc)
        assert list(got) == list(P.COLUMNS)
        for k in P.COLUMNS:
            assert list(got[k]) == list(want[k]), (ref_nw, k)
        assert (got["gain"] >= 0).all() and ((got["distance"] == 0) | (got["gain"] > 0)).all()   # only a better position is away


def test_planted_misplacement():
    ref_nw, trees, true_side, moved = P.planted()
    assert moved >= 3
    ref = flatten.flatten_reference(ref_nw)
    table = bruteforce.count_table(ref.names, trees)
    sc = P.scores(ref, P.link_sums(table, ref))
    x = ref.name_to_id["tx"]
    cols = P.columns(ref, list(range(ref.n_taxa)), sc)
    assert cols["n_best"][x] == 1 and cols["gain"][x] > 0 and cols["distance"][x] == moved
    assert cols["best"][x] == 7 * 11 * 10 * 9 // 6               # every quartet of tx in every tree
    below = {ref.names[i] for i in range(cols["best_lo"][x], cols["best_hi"][x])} - {"tx"}
    assert below == true_side                                     # the true bipartition
    rest = np.delete(np.arange(ref.n_taxa), x)
    assert (cols["gain"][rest] < cols["gain"][x]).all()           # the planted taxon gains most
    got = engine.placement_columns(ref, [x], sc[x:x + 1])
    assert all(list(got[k]) == [cols[k][x]] for k in P.COLUMNS)


# ---- QuartetScores --place-taxa: refusals before the device is touched ---------------------------------------------------

def run(*args):
    return subprocess.run([BIN, *map(str, args)], capture_output=True, text=True, timeout=600)


@pytest.fixture()
def files(tmp_path):
    n = 12
    (tmp_path / "r.nwk").write_text(synth.reference_tree(n, 1) + "\n")
    (tmp_path / "e.nwk").write_text("\n".join(synth.tree_set(n, 6, 2)) + "\n")
    return tmp_path


def base(files):
    return ["-r", files / "r.nwk", "-e", files / "e.nwk", "-o", files / "o.nwk"]


def test_missing_value(files):
    p = run(*base(files), "--place-taxa")
    assert p.returncode == 1 and "Missing a value for this argument! for arg --place-taxa" in p.stderr, p.stderr
    p = run(*base(files), "--place-taxa", files / "p.tsv", "--place-only")
    assert p.returncode == 1 and "Missing a value for this argument! for arg --place-only" in p.stderr, p.stderr


def test_place_only_needs_place_taxa(files):
    (files / "names.txt").write_text("t1\n")
    p = run(*base(files), "--place-only", files / "names.txt")
    assert p.returncode == 1 and "--place-only needs --place-taxa" in p.stderr, p.stderr


def test_unknown_label(files):
    (files / "names.txt").write_text("t1\n\n  nobody \nt2\n")
    p = run(*base(files), "--place-taxa", files / "p.tsv", "--place-only", files / "names.txt")
    assert p.returncode == 1 and "the taxon nobody is not in the reference tree" in p.stderr, p.stderr
    assert not (files / "p.tsv").exists() and not (files / "o.nwk").exists()
    (files / "names.txt").write_text("\n \n")
    p = run(*base(files), "--place-taxa", files / "p.tsv", "--place-only", files / "names.txt")
    assert p.returncode == 1 and "the list of taxa is empty" in p.stderr, p.stderr


@pytest.mark.parametrize("extra", [["--gpus", "2"], ["--table-shards", "2"]])
def test_refused_without_the_whole_table_on_one_gpu(files, extra):
    p = run(*base(files), "--place-taxa", files / "p.tsv", *extra)
    assert p.returncode == 1 and "--place-taxa needs the whole count table on one GPU" in p.stderr, p.stderr
    assert not (files / "p.tsv").exists() and not (files / "o.nwk").exists()


def test_refused_existing_file(files):
    (files / "p.tsv").write_text("keep\n")
    p = run(*base(files), "--place-taxa", files / "p.tsv")
    assert p.returncode == 1 and "already exists" in p.stderr, p.stderr
    assert (files / "p.tsv").read_text() == "keep\n" and not (files / "o.nwk").exists()


@pytest.mark.parametrize("other", ["-o", "-q", "--per-tree", "--per-taxon", "--without-taxa"])
def test_refused_file_that_is_another_output(files, other):
    shared = files / "shared.out"
    (files / "drop.txt").write_text("t3\n")
    args = ["-r", files / "r.nwk", "-e", files / "e.nwk", "--place-taxa", shared]
    if other == "-o":
        args += ["-o", shared]
    elif other == "--without-taxa":
        args += ["-o", files / "o.nwk", other, files / "drop.txt", shared]
    else:
        args += ["-o", files / "o.nwk", other, shared]
    p = run(*args)
    assert p.returncode == 1 and ("is also another output file" in p.stderr or "is given twice" in p.stderr), p.stderr
    assert not shared.exists() and not (files / "o.nwk").exists()


def test_usage_names_the_flags():
    p = run("--help")
    assert "--place-taxa" in p.stdout + p.stderr and "--place-only" in p.stdout + p.stderr
