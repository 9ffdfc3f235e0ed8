"""QuartetScores --per-taxon FILE on the device: one line per taxon with the columns of Context.taxon_support, the other
outputs byte-identical with and without the flag, and the same file from --load-table of the saved table."""
import os
import subprocess

import numpy as np
import pytest

from quartetscores_amd import flatten, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "quartetscores_amd", "bin", "QuartetScores")
HEADER = ["taxon", "name", "quartets", "ref_resolved", "concordant", "discordant", "eval_only", "outvoted", "uninformed", "concordance",
          "concordance_without"]


def run(*args):
    return subprocess.run([BIN, *map(str, args)], capture_output=True, text=True, timeout=600)


def test_per_taxon_file(tmp_path, m=62):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    from quartetscores_amd import engine
    n = 30
    rng = np.random.default_rng(3)
    ref_nw = synth.random_tree(n, rng, collapse=0.2)
    k = m // 4
    trees = (synth.tree_set(n, k, 4) + synth.tree_set(n, k, 5, collapse=0.3) + synth.tree_set(n, k, 6, dropout=0.4, min_taxa=2)
             + synth.tree_set(n, m - 3 * k, 7, rooted=True))
    (tmp_path / "r.nwk").write_text(ref_nw + "\n")
    (tmp_path / "e.nwk").write_text("\n".join(trees) + "\n")
    common = ("-r", tmp_path / "r.nwk", "-e", tmp_path / "e.nwk")
    p = run(*common, "-o", tmp_path / "a.nwk", "-q", tmp_path / "a.q")
    assert p.returncode == 0, p.stderr
    p = run(*common, "-o", tmp_path / "b.nwk", "-q", tmp_path / "b.q", "--per-taxon", tmp_path / "p.tsv", "--per-tree", tmp_path / "t.tsv",
            "--save-table", tmp_path / "table.bin")
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "a.nwk").read_bytes() == (tmp_path / "b.nwk").read_bytes()
    assert (tmp_path / "a.q").read_bytes() == (tmp_path / "b.q").read_bytes()
    assert (tmp_path / "t.tsv").exists()

    lines = (tmp_path / "p.tsv").read_text().splitlines()
    assert lines[0].split("\t") == HEADER
    rows = [ln.split("\t") for ln in lines[1:]]
    assert len(rows) == n

    ref = flatten.flatten_reference(ref_nw)
    ctx = engine.Context(n, 16)
    ctx.table_alloc()
    ctx.count_trees(flatten.flatten_eval_trees(trees, ref.name_to_id))
    cols = engine.taxon_columns(ctx.taxon_support(ref))
    assert cols["discordant"].sum() > 0 and cols["eval_only"].sum() > 0
    for x, r in enumerate(rows):
        assert int(r[0]) == x and r[1] == ref.names[x]
        for j, name in enumerate(HEADER[2:9]):
            assert int(r[2 + j]) == int(cols[name][x]), (x, name)
        for j, name in enumerate(HEADER[9:]):
            v = cols[name][x]
            assert r[9 + j] == ("nan" if np.isnan(v) else f"{v:.6f}"), (x, name)

    # the saved table, loaded: no trees are counted, the same file
    p = run(*common, "-o", tmp_path / "c.nwk", "--load-table", tmp_path / "table.bin", "--per-taxon", tmp_path / "p2.tsv")
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "p2.tsv").read_bytes() == (tmp_path / "p.tsv").read_bytes()
    assert (tmp_path / "c.nwk").read_bytes() == (tmp_path / "a.nwk").read_bytes()
