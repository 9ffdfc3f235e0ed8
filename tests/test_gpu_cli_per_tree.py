"""QuartetScores --per-tree FILE on the device: one line per evaluation tree with the counts of Context.tree_agreement, and the
other outputs byte-identical with and without the flag."""
import os
import subprocess

import numpy as np
import pytest

from quartetscores_amd import flatten, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "quartetscores_amd", "bin", "QuartetScores")


def run(*args):
    return subprocess.run([BIN, *map(str, args)], capture_output=True, text=True, timeout=600)


def test_per_tree_file(tmp_path):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    from quartetscores_amd import engine
    n = 30
    rng = np.random.default_rng(3)
    ref_nw = synth.random_tree(n, rng)
    trees = (synth.tree_set(n, 20, 4) + synth.tree_set(n, 20, 5, collapse=0.3) + synth.tree_set(n, 20, 6, dropout=0.4, min_taxa=2)
             + synth.tree_set(n, 10, 7, rooted=True))
    (tmp_path / "r.nwk").write_text(ref_nw + "\n")
    (tmp_path / "e.nwk").write_text("\n".join(trees) + "\n")
    common = ("-r", tmp_path / "r.nwk", "-e", tmp_path / "e.nwk")
    p = run(*common, "-o", tmp_path / "a.nwk", "-q", tmp_path / "a.q")
    assert p.returncode == 0, p.stderr
    p = run(*common, "-o", tmp_path / "b.nwk", "-q", tmp_path / "b.q", "--per-tree", tmp_path / "p.tsv")
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "a.nwk").read_bytes() == (tmp_path / "b.nwk").read_bytes()
    assert (tmp_path / "a.q").read_bytes() == (tmp_path / "b.q").read_bytes()

    lines = (tmp_path / "p.tsv").read_text().splitlines()
    assert lines[0].split("\t") == ["tree", "taxa", "quartets", "concordant", "discordant", "eval_only", "ref_only", "unresolved", "concordance"]
    rows = [ln.split("\t") for ln in lines[1:]]
    assert len(rows) == len(trees)

    ref = flatten.flatten_reference(ref_nw)
    ctx = engine.Context(n)
    b = flatten.flatten_eval_trees(trees, ref.name_to_id)
    hb = ctx.batch_upload(b)
    want = ctx.tree_agreement(ref, hb)
    ctx.batch_free(hb)
    cols = engine.agreement_columns(want, np.diff(b.leaf_off.astype(np.int64)))
    for t, r in enumerate(rows):
        assert int(r[0]) == t and int(r[1]) == int(b.leaf_off[t + 1] - b.leaf_off[t])
        for k, name in enumerate(["quartets", "concordant", "discordant", "eval_only", "ref_only", "unresolved"]):
            assert int(r[2 + k]) == int(cols[name][t]), (t, name)
        c = cols["concordance"][t]
        assert r[8] == ("nan" if np.isnan(c) else f"{c:.6f}")
