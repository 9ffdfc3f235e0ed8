"""Per-taxon quartet support without a GPU: the numpy model of qs_taxon.hip (tests/taxon_model.py) against a brute force from
bipartitions, the closed identities of the six sums, the derived columns, and the refusals of QuartetScores --per-taxon."""
import os
import subprocess

import numpy as np
import pytest

import bruteforce
import taxon_model as M
from helpers import binom
from quartetscores_amd import engine, flatten, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "quartetscores_amd", "bin", "QuartetScores")


def random_cases(count, seed):
    rng = np.random.default_rng(seed)
    for i in range(count):
        n = int(rng.integers(5, 25))
        ref_kw = [{}, {"collapse": 0.3}, {"rooted": True}, {"collapse": 1.0}, {"rooted": True, "collapse": 0.5}, {"collapse": 0.7}][i % 6]
        ref_nw = synth.random_tree(n, rng, **ref_kw)
        trees = []
        for k in range(int(rng.integers(1, 8))):
            ev_kw = [{}, {"collapse": float(rng.uniform(0.1, 1.0))}, {"dropout": float(rng.uniform(0.1, 0.8)), "min_taxa": int(rng.integers(1, 5))},
                     {"rooted": True}, {"rooted": True, "collapse": 0.3, "dropout": 0.3}][(i + k) % 5]
            trees.append(synth.random_tree(n, rng, **ev_kw))
        yield n, ref_nw, trees


def test_model_matches_brute_force():
    cases = unresolved = outvoted = uninformed = 0
    for n, ref_nw, trees in random_cases(72, 23):
        ref = flatten.flatten_reference(ref_nw)
        table = bruteforce.count_table(ref.names, trees)
        got, want = M.model_counts(table, ref), M.brute_counts(ref_nw, ref.names, trees)
        assert got.shape == (n, 6) and (got == want).all(), (ref_nw, trees)
        cases += 1
        unresolved += int(want[:, 3].sum() > 0)
        outvoted += int(want[:, 4].sum() > 0)
        uninformed += int(want[:, 5].sum() > 0)
    assert cases >= 60 and unresolved and outvoted and uninformed


def test_closed_identities():
    for n, ref_nw, trees in random_cases(30, 29):
        ref = flatten.flatten_reference(ref_nw)
        table = bruteforce.count_table(ref.names, trees).astype(np.int64)
        got = M.model_counts(table, ref)
        topo = M.model_topology(ref, M.quads_in_rank_order(n))
        res = topo != 255
        assert int(got[:, 0].sum()) == 4 * int(res.sum()) == 4 * M.resolved_quartets(ref)
        assert int((got[:, 1] + got[:, 2]).sum()) == 4 * int(table[res].sum())
        assert int(got[:, 3].sum()) == 4 * int(table[~res].sum())
        assert (got[:, 4] + got[:, 5] <= got[:, 0]).all()          # an outvoted quartet has a count, an uninformed one has none
        assert (got[:, 0] <= int(binom(n - 1, 3))).all()
        # shards add: the table cut at two ranks
        cuts = [0, len(table) // 3, len(table) // 3 + 1, len(table)]
        parts = sum(M.model_counts(table[lo:hi], ref, rank_lo=lo) for lo, hi in zip(cuts, cuts[1:]))
        assert (parts == got).all()


def test_a_rogue_taxon_stands_out():
    # eleven taxa in a caterpillar; in every evaluation tree t5 sits somewhere else, the ten others keep their places
    names = [f"t{i}" for i in range(11)]
    cat = lambda xs: xs[0] if len(xs) == 1 else "(" + xs[0] + "," + cat(xs[1:]) + ")"
    ref_nw = cat(names) + ";"
    others = [x for x in names if x != "t5"]
    trees = [cat(others[:k] + ["t5"] + others[k:]) + ";" for k in range(10)]
    ref = flatten.flatten_reference(ref_nw)
    cols = engine.taxon_columns(M.model_counts(bruteforce.count_table(ref.names, trees), ref))
    rogue = ref.name_to_id["t5"]
    assert cols["concordance_without"][rogue] == 1.0                # without t5 the trees agree with the reference completely
    assert (np.delete(cols["concordance_without"], rogue) < 1.0).all()
    assert cols["concordance"].argmin() == rogue


def test_named_and_derived_columns():
    # five taxa, five quartets; quartet j leaves taxon j out and holds (q1, q2 + q3) = (q1[j], alt[j])
    q1, alt = np.array([10, 0, 30, 5, 0]), np.array([0, 10, 10, 5, 0])
    counts = np.zeros((5, 6), dtype=np.int64)
    counts[:, 0], counts[:, 1], counts[:, 2] = 4, q1.sum() - q1, alt.sum() - alt
    cols = engine.taxon_columns(counts)
    assert list(cols) == ["quartets", *engine.TAXON_FIELDS, "concordance", "concordance_without"]
    assert engine.TAXON_FIELDS == M.FIELDS
    assert cols["quartets"].tolist() == [4] * 5                      # C(4,3)
    assert cols["concordant"].tolist() == [35, 45, 15, 40, 45] and cols["discordant"].tolist() == [25, 15, 15, 20, 25]
    assert cols["concordance"].tolist() == [35 / 60, 45 / 60, 15 / 30, 40 / 60, 45 / 70]
    without = cols["concordance_without"]                            # = the quartet that leaves the taxon out
    assert without[:4].tolist() == [1.0, 0.0, 0.75, 0.5] and np.isnan(without[4])
    zero = engine.taxon_columns(np.zeros((4, 6), dtype=np.int64))
    assert zero["quartets"].tolist() == [1] * 4
    assert np.isnan(zero["concordance"]).all() and np.isnan(zero["concordance_without"]).all()


# ---- QuartetScores --per-taxon: refusals before the device is touched ----------------------------------------------------

def run(*args):
    return subprocess.run([BIN, *map(str, args)], capture_output=True, text=True, timeout=600)


@pytest.fixture()
def files(tmp_path):
    n = 12
    (tmp_path / "r.nwk").write_text(synth.reference_tree(n, 1) + "\n")
    (tmp_path / "e.nwk").write_text("\n".join(synth.tree_set(n, 6, 2)) + "\n")
    return tmp_path


def test_missing_value(files):
    p = run("-r", files / "r.nwk", "-e", files / "e.nwk", "-o", files / "o.nwk", "--per-taxon")
    assert p.returncode == 1 and "Missing a value for this argument! for arg --per-taxon" in p.stderr, p.stderr


@pytest.mark.parametrize("extra", [["--gpus", "2"], ["--table-shards", "2"]])
def test_refused_without_the_whole_table_on_one_gpu(files, extra):
    p = run("-r", files / "r.nwk", "-e", files / "e.nwk", "-o", files / "o.nwk", "--per-taxon", files / "p.tsv", *extra)
    assert p.returncode == 1 and "--per-taxon needs the whole count table on one GPU" in p.stderr, p.stderr
    assert not (files / "p.tsv").exists() and not (files / "o.nwk").exists()


def test_refused_existing_file(files):
    (files / "p.tsv").write_text("keep\n")
    p = run("-r", files / "r.nwk", "-e", files / "e.nwk", "-o", files / "o.nwk", "--per-taxon", files / "p.tsv")
    assert p.returncode == 1 and "already exists" in p.stderr, p.stderr
    assert (files / "p.tsv").read_text() == "keep\n" and not (files / "o.nwk").exists()


@pytest.mark.parametrize("other", ["-o", "-q", "--per-tree"])
def test_refused_file_that_is_another_output(files, other):
    shared = files / "shared.out"
    args = ["-r", files / "r.nwk", "-e", files / "e.nwk", "--per-taxon", shared]
    args += ["-o", shared] if other == "-o" else ["-o", files / "o.nwk", other, shared]
    p = run(*args)
    assert p.returncode == 1 and "is also another output file" in p.stderr, p.stderr
    assert not shared.exists() and not (files / "o.nwk").exists()


def test_usage_names_the_flag():
    p = run("--help")
    assert "--per-taxon" in p.stdout + p.stderr
