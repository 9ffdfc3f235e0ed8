"""Per-tree quartet agreement without a GPU: the node-pair formulas of tests/agreement_model.py (the model of qs_agree.hip)
against a per-quartet brute force, the derived columns, and the refusals of QuartetScores --per-tree."""
import os
import subprocess

import numpy as np
import pytest

import agreement_model as M
from quartetscores_amd import engine, flatten, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "quartetscores_amd", "bin", "QuartetScores")


def random_pairs(count, seed):
    rng = np.random.default_rng(seed)
    for i in range(count):
        n = int(rng.integers(5, 31)) if i % 4 else int(rng.integers(5, 12))
        ref_kw = [{}, {"rooted": True}, {"collapse": 0.3}, {"collapse": 1.0}, {"rooted": True, "collapse": 0.5}][i % 5]
        ev_kw = [{}, {"collapse": float(rng.uniform(0.1, 1.0))}, {"dropout": float(rng.uniform(0.1, 0.9)), "min_taxa": int(rng.integers(1, 5))},
                 {"rooted": True}, {"rooted": True, "collapse": 0.3, "dropout": 0.3}, {"collapse": 1.0}][i % 6]
        yield synth.random_tree(n, rng, **ref_kw), synth.random_tree(n, rng, **ev_kw)


def test_model_matches_brute_force():
    seen_small = seen_star = 0
    for ref_nw, ev_nw in random_pairs(120, 17):
        ref = flatten.flatten_reference(ref_nw)
        want = M.brute_counts(ref_nw, ref.names, ev_nw)
        assert M.model_tree(ref, ev_nw) == want, (ref_nw, ev_nw)
        assert M.model_tree(ref, ev_nw, recentre=False) == want
        seen_small += want == (0, 0, 0, 0)
        seen_star += want[2] == 0
    assert seen_small and seen_star


def test_closed_form_nni():
    # one NNI across the edge with subtrees A, B | C, D: exactly |A| |B| |C| |D| quartets change their topology
    A, B, C, D = ["a0", "a1"], ["b0", "b1", "b2"], ["c0"], ["d0", "d1", "d2", "d3"]
    cat = lambda xs: xs[0] if len(xs) == 1 else "(" + xs[0] + "," + cat(xs[1:]) + ")"
    ref_nw = f"({cat(A)},{cat(B)},({cat(C)},{cat(D)}));"
    ev_nw = f"({cat(A)},{cat(C)},({cat(B)},{cat(D)}));"
    ref = flatten.flatten_reference(ref_nw)
    full = 10 * 9 * 8 * 7 // 24
    assert M.model_tree(ref, ev_nw) == (full - 24, 24, full, full)


def test_derived_columns():
    cols = engine.agreement_columns(np.array([[3, 1, 4, 5], [0, 0, 0, 0], [0, 0, 0, 1]], dtype=np.uint64), [5, 3, 4])
    assert cols["quartets"].tolist() == [5, 0, 1]
    assert cols["eval_only"].tolist() == [0, 0, 0]
    assert cols["ref_only"].tolist() == [1, 0, 1]
    assert cols["unresolved"].tolist() == [0, 0, 0]
    assert cols["concordance"][0] == 0.75 and np.isnan(cols["concordance"][1])


# ---- QuartetScores --per-tree: refusals before the device is touched -----------------------------------------------------

def run(*args):
    return subprocess.run([BIN, *map(str, args)], capture_output=True, text=True, timeout=600)


@pytest.fixture()
def files(tmp_path):
    n = 12
    (tmp_path / "r.nwk").write_text(synth.reference_tree(n, 1) + "\n")
    (tmp_path / "e.nwk").write_text("\n".join(synth.tree_set(n, 6, 2)) + "\n")
    return tmp_path


def test_missing_value(files):
    p = run("-r", files / "r.nwk", "-e", files / "e.nwk", "-o", files / "o.nwk", "--per-tree")
    assert p.returncode == 1 and "Missing a value for this argument! for arg --per-tree" in p.stderr, p.stderr


@pytest.mark.parametrize("extra", [["--gpus", "2"], ["--table-shards", "2"], ["--load-table", "t.bin"]])
def test_refused_without_counting_on_one_gpu(files, extra):
    p = run("-r", files / "r.nwk", "-e", files / "e.nwk", "-o", files / "o.nwk", "--per-tree", files / "p.tsv", *extra)
    assert p.returncode == 1 and "--per-tree needs the evaluation trees counted on one GPU" in p.stderr, p.stderr
    assert not (files / "p.tsv").exists() and not (files / "o.nwk").exists()


def test_refused_existing_or_shared_file(files):
    (files / "p.tsv").write_text("keep\n")
    p = run("-r", files / "r.nwk", "-e", files / "e.nwk", "-o", files / "o.nwk", "--per-tree", files / "p.tsv")
    assert p.returncode == 1 and "already exists" in p.stderr, p.stderr
    assert (files / "p.tsv").read_text() == "keep\n"
    p = run("-r", files / "r.nwk", "-e", files / "e.nwk", "-o", files / "o.nwk", "--per-tree", files / "o.nwk")
    assert p.returncode == 1 and "is also another output file" in p.stderr, p.stderr
