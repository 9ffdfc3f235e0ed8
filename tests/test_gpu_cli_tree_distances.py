"""QuartetScores --tree-distances FILE on the device: one line per pair of evaluation trees with the counts of
Context.tree_pair_agreement, together with --per-tree, the other outputs byte-identical with and without the flag, and the refusal
with --load-table."""
import os
import subprocess

import numpy as np
import pytest

from quartetscores_amd import flatten, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "quartetscores_amd", "bin", "QuartetScores")
HEADER = ["a", "b", "taxa", "quartets", "concordant", "discordant", "a_only", "b_only", "unresolved", "concordance", "distance"]


def run(*args):
    return subprocess.run([BIN, *map(str, args)], capture_output=True, text=True, timeout=600)


def test_tree_distances_file(tmp_path):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    from quartetscores_amd import engine
    n = 30
    rng = np.random.default_rng(3)
    ref_nw = synth.random_tree(n, rng)
    trees = (synth.tree_set(n, 12, 4) + synth.tree_set(n, 12, 5, collapse=0.3) + synth.tree_set(n, 8, 6, dropout=0.4, min_taxa=2)
             + synth.tree_set(n, 2, 8, dropout=0.93, min_taxa=2) + synth.tree_set(n, 6, 7, rooted=True))   # (two trees of a few taxa: nan)
    m = len(trees)
    assert m == 40
    (tmp_path / "r.nwk").write_text(ref_nw + "\n")
    (tmp_path / "e.nwk").write_text("\n".join(trees) + "\n")
    common = ("-r", tmp_path / "r.nwk", "-e", tmp_path / "e.nwk")
    p = run(*common, "-o", tmp_path / "a.nwk", "-q", tmp_path / "a.q", "--per-tree", tmp_path / "a.tsv")
    assert p.returncode == 0, p.stderr
    p = run(*common, "-o", tmp_path / "b.nwk", "-q", tmp_path / "b.q", "--tree-distances", tmp_path / "b.dist")
    assert p.returncode == 0, p.stderr
    p = run(*common, "-o", tmp_path / "c.nwk", "-q", tmp_path / "c.q", "--per-tree", tmp_path / "c.tsv", "--tree-distances", tmp_path / "c.dist")
    assert p.returncode == 0, p.stderr
    for name in ("b", "c"):
        assert (tmp_path / "a.nwk").read_bytes() == (tmp_path / f"{name}.nwk").read_bytes()
        assert (tmp_path / "a.q").read_bytes() == (tmp_path / f"{name}.q").read_bytes()
    assert (tmp_path / "a.tsv").read_bytes() == (tmp_path / "c.tsv").read_bytes()
    assert (tmp_path / "b.dist").read_bytes() == (tmp_path / "c.dist").read_bytes()

    lines = (tmp_path / "b.dist").read_text().splitlines()
    assert lines[0].split("\t") == HEADER
    rows = [ln.split("\t") for ln in lines[1:]]
    assert len(rows) == m * (m - 1) // 2 == 780

    ref = flatten.flatten_reference(ref_nw)
    ctx = engine.Context(n)
    hb = ctx.batch_upload(flatten.flatten_eval_trees(trees, ref.name_to_id))
    cols = engine.pair_columns(ctx.tree_pair_agreement(hb))
    ctx.batch_free(hb)
    pairs = [(a, b) for a in range(m) for b in range(a + 1, m)]
    for (a, b), r in zip(pairs, rows):
        assert (int(r[0]), int(r[1])) == (a, b)
        for k, name in enumerate(["shared", "quartets", "concordant", "discordant", "row_only", "col_only", "unresolved"]):
            assert int(r[2 + k]) == int(cols[name][a, b]), (a, b, name)
        for k, name in ((9, "concordance"), (10, "distance")):
            x = cols[name][a, b]
            assert r[k] == ("nan" if np.isnan(x) else f"{x:.6f}"), (a, b, name)
    assert any(r[10] == "nan" for r in rows) and any(r[10] != "nan" and float(r[10]) > 0 for r in rows)


def test_refused_with_load_table(tmp_path):
    n = 12
    (tmp_path / "r.nwk").write_text(synth.reference_tree(n, 1) + "\n")
    (tmp_path / "e.nwk").write_text("\n".join(synth.tree_set(n, 6, 2)) + "\n")
    (tmp_path / "t.bin").write_bytes(b"\0" * 16)
    p = run("-r", tmp_path / "r.nwk", "-e", tmp_path / "e.nwk", "-o", tmp_path / "o.nwk", "--load-table", tmp_path / "t.bin",
            "--tree-distances", tmp_path / "d.tsv")
    assert p.returncode != 0
    assert "--tree-distances" in p.stderr
    assert not (tmp_path / "o.nwk").exists() and not (tmp_path / "d.tsv").exists()
