"""QuartetScores --taxon-pairs FILE [--taxon-pairs-only NAMES] on the device: one line per pair of taxa with the columns the numpy
model (tests/taxon_pair_model.py) defines, the other outputs byte-identical with and without the flag, the same file from
--load-table of the saved table, and a planted attraction found through the CLI."""
import os
import subprocess

import numpy as np
import pytest

import bruteforce
import taxon_pair_model as M
from quartetscores_amd import flatten, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "quartetscores_amd", "bin", "QuartetScores")


def run(*args):
    return subprocess.run([BIN, *map(str, args)], capture_output=True, text=True, timeout=600)


def text_of(value):
    if isinstance(value, (float, np.floating)):
        return "nan" if np.isnan(value) else "%.6f" % value      # as --per-taxon's concordance
    return str(value)


def model_rows(ref, trees, taxa=None):
    table = bruteforce.count_table(ref.names, trees)
    cols = M.columns(M.pair_counts(table, ref, taxa), ref.names, taxa)
    return [[text_of(cols[name][i]) for name in M.COLUMNS] for i in range(len(cols["a"]))]


def read_tsv(path):
    lines = path.read_text().splitlines()
    assert lines[0].split("\t") == list(M.COLUMNS)
    return [ln.split("\t") for ln in lines[1:]]


def test_taxon_pairs_file(tmp_path, m=42):
    n = 24
    rng = np.random.default_rng(3)
    ref_nw = synth.random_tree(n, rng, collapse=0.2)
    k = m // 4
    trees = (synth.tree_set(n, k, 4) + synth.tree_set(n, k, 5, collapse=0.3) + synth.tree_set(n, k, 6, dropout=0.4, min_taxa=2)
             + synth.tree_set(n, m - 3 * k, 7, rooted=True))
    (tmp_path / "r.nwk").write_text(ref_nw + "\n")
    (tmp_path / "e.nwk").write_text("\n".join(trees) + "\n")
    common = ("-r", tmp_path / "r.nwk", "-e", tmp_path / "e.nwk")
    others = lambda tag: ("--per-taxon", tmp_path / f"{tag}.x.tsv", "--per-tree", tmp_path / f"{tag}.t.tsv", "--place-taxa", tmp_path / f"{tag}.p.tsv")
    p = run(*common, "-o", tmp_path / "a.nwk", "-q", tmp_path / "a.q", *others("a"))
    assert p.returncode == 0, p.stderr
    p = run(*common, "-o", tmp_path / "b.nwk", "-q", tmp_path / "b.q", *others("b"), "--taxon-pairs", tmp_path / "pairs.tsv", "--save-table", tmp_path / "table.bin")
    assert p.returncode == 0, p.stderr
    for name in ("nwk", "q", "x.tsv", "t.tsv", "p.tsv"):
        assert (tmp_path / f"a.{name}").read_bytes() == (tmp_path / f"b.{name}").read_bytes(), name

    ref = flatten.flatten_reference(ref_nw)
    rows = read_tsv(tmp_path / "pairs.tsv")
    want = model_rows(ref, trees)
    assert len(rows) == n * (n - 1) // 2 and rows == want
    # the two sisters of a cherry of the reference are never resolved apart: joined is nan there, a ratio elsewhere
    assert any(r[11] == "nan" for r in rows) and any(r[11] not in ("nan", "0.000000") for r in rows)

    # alone beside -o: the same files
    p = run(*common, "-o", tmp_path / "c.nwk", "-q", tmp_path / "c.q", "--taxon-pairs", tmp_path / "pairs0.tsv")
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "c.nwk").read_bytes() == (tmp_path / "a.nwk").read_bytes() and (tmp_path / "c.q").read_bytes() == (tmp_path / "a.q").read_bytes()
    assert (tmp_path / "pairs0.tsv").read_bytes() == (tmp_path / "pairs.tsv").read_bytes()

    # a list: unsorted in the file, blank lines, a repeated label -- exactly the lines with a listed taxon, in order
    listed = [17, 3, 23, 0, 3]
    (tmp_path / "names.txt").write_text("\n".join(ref.names[i] for i in listed) + "\n\n")
    p = run(*common, "-o", tmp_path / "d.nwk", "--taxon-pairs", tmp_path / "pairs1.tsv", "--taxon-pairs-only", tmp_path / "names.txt")
    assert p.returncode == 0, p.stderr
    keep = {str(i) for i in listed}
    assert read_tsv(tmp_path / "pairs1.tsv") == [r for r in rows if r[0] in keep or r[1] in keep]
    assert read_tsv(tmp_path / "pairs1.tsv") == model_rows(ref, trees, sorted(set(listed)))
    assert (tmp_path / "d.nwk").read_bytes() == (tmp_path / "a.nwk").read_bytes()

    # the saved table, loaded: no trees are counted, the same file
    p = run(*common, "-o", tmp_path / "e2.nwk", "--load-table", tmp_path / "table.bin", "--taxon-pairs", tmp_path / "pairs2.tsv")
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "pairs2.tsv").read_bytes() == (tmp_path / "pairs.tsv").read_bytes()
    assert (tmp_path / "e2.nwk").read_bytes() == (tmp_path / "a.nwk").read_bytes()


MARGIN = 0.05    # tests/taxon_pair_model.planted(): the numpy model gives 0.727 for (u, v) and 0.635 for u with v's neighbour


def test_planted_attraction_through_the_cli(tmp_path):
    ref_nw, trees, u, v = M.planted()
    (tmp_path / "r.nwk").write_text(ref_nw + "\n")
    (tmp_path / "e.nwk").write_text("\n".join(trees) + "\n")
    p = run("-r", tmp_path / "r.nwk", "-e", tmp_path / "e.nwk", "-o", tmp_path / "o.nwk", "--taxon-pairs", tmp_path / "pairs.tsv")
    assert p.returncode == 0, p.stderr
    ref = flatten.flatten_reference(ref_nw)
    rows = read_tsv(tmp_path / "pairs.tsv")
    assert rows == model_rows(ref, trees)
    apart = sorted(((float(r[11]), r[2], r[3]) for r in rows if int(r[6]) > 0), reverse=True)
    assert {apart[0][1], apart[0][2]} == {u, v}
    assert apart[0][0] >= apart[1][0] + MARGIN and apart[0][0] > 0.7
