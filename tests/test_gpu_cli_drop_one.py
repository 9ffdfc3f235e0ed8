"""QuartetScores --drop-one FILE [--drop-one-only NAMES] on the device: one line per taxon and internode with the columns the numpy
model (tests/branch_taxon_model.py) defines, the annotated tree byte-identical with and without the flag, the same file from
--load-table of the saved table, and exactly the listed taxa with --drop-one-only."""
import os
import subprocess

import numpy as np
import pytest

import branch_taxon_model as M
import bruteforce
from quartetscores_amd import engine, flatten, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "quartetscores_amd", "bin", "QuartetScores")


def run(*args):
    return subprocess.run([BIN, *map(str, args)], capture_output=True, text=True, timeout=600)


def read_tsv(path):
    lines = path.read_text().splitlines()
    assert lines[0].split("\t") == list(engine.DROP_ONE_COLUMNS)
    return [ln.split("\t") for ln in lines[1:]]


@pytest.mark.parametrize("kind", ["binary", "rooted", "multifurcating"])
def test_drop_one_file(tmp_path, kind):
    n, m = 12, 30
    rng = np.random.default_rng(3)
    ref_nw = synth.random_tree(n, rng, **{"binary": {}, "rooted": {"rooted": True}, "multifurcating": {"collapse": 0.3}}[kind])
    trees = synth.tree_set(n, 10, 4) + synth.tree_set(n, 10, 5, collapse=0.3) + synth.tree_set(n, 10, 6, dropout=0.4, min_taxa=2)
    assert len(trees) == m
    (tmp_path / "r.nwk").write_text(ref_nw + "\n")
    (tmp_path / "e.nwk").write_text("\n".join(trees) + "\n")
    common = ("-r", tmp_path / "r.nwk", "-e", tmp_path / "e.nwk")
    p = run(*common, "-o", tmp_path / "a.nwk", "--per-taxon", tmp_path / "a.x.tsv")
    assert p.returncode == 0, p.stderr
    p = run(*common, "-o", tmp_path / "b.nwk", "--per-taxon", tmp_path / "b.x.tsv", "--drop-one", tmp_path / "drop.tsv", "--save-table", tmp_path / "table.bin")
    assert p.returncode == 0, p.stderr
    for name in ("nwk", "x.tsv"):
        assert (tmp_path / f"a.{name}").read_bytes() == (tmp_path / f"b.{name}").read_bytes(), name

    ref = flatten.flatten_reference(ref_nw)
    every, totals = M.model(bruteforce.count_table(ref.names, trees), ref)
    want = [[str(z) for z in line] for line in M.columns(ref, list(range(n)), every, totals)]
    rows = read_tsv(tmp_path / "drop.tsv")
    assert rows == want and len(rows) > n
    assert any(r[11] == "nan" for r in rows) and any(r[12] not in ("nan", "0.000000", "-0.000000") for r in rows)

    # a list: unsorted in the file, blank lines, a repeated label -- exactly the listed taxa, in id order
    listed = [7, 3, 11, 0, 3]
    (tmp_path / "names.txt").write_text("\n".join(ref.names[i] for i in listed) + "\n\n")
    p = run(*common, "-o", tmp_path / "d.nwk", "--drop-one", tmp_path / "drop1.tsv", "--drop-one-only", tmp_path / "names.txt")
    assert p.returncode == 0, p.stderr
    keep = {str(i) for i in listed}
    assert read_tsv(tmp_path / "drop1.tsv") == [r for r in rows if r[0] in keep]
    assert (tmp_path / "d.nwk").read_bytes() == (tmp_path / "a.nwk").read_bytes()

    # the saved table, loaded: no trees are counted, the same file
    p = run(*common, "-o", tmp_path / "e2.nwk", "--load-table", tmp_path / "table.bin", "--drop-one", tmp_path / "drop2.tsv")
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "drop2.tsv").read_bytes() == (tmp_path / "drop.tsv").read_bytes()
    assert (tmp_path / "e2.nwk").read_bytes() == (tmp_path / "a.nwk").read_bytes()
