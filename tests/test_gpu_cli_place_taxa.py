"""QuartetScores --place-taxa FILE [--place-only NAMES] on the device: one line per placed taxon with the columns the numpy model
(tests/placement_model.py) defines, the other outputs byte-identical with and without the flag, the same file from --load-table of
the saved table, and the planted misplacement found through the CLI."""
import os
import subprocess

import numpy as np
import pytest

import bruteforce
import placement_model as P
from quartetscores_amd import flatten, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "quartetscores_amd", "bin", "QuartetScores")


def run(*args):
    return subprocess.run([BIN, *map(str, args)], capture_output=True, text=True, timeout=600)


def model_rows(ref, trees, taxa):
    table = bruteforce.count_table(ref.names, trees)
    cols = P.columns(ref, taxa, P.scores(ref, P.link_sums(table, ref, taxa)))
    return [[str(cols[name][i]) for name in P.COLUMNS] for i in range(len(taxa))]


def read_tsv(path):
    lines = path.read_text().splitlines()
    assert lines[0].split("\t") == list(P.COLUMNS)
    return [ln.split("\t") for ln in lines[1:]]


def test_place_taxa_file(tmp_path, m=42):
    n = 24
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
    p = run(*common, "-o", tmp_path / "b.nwk", "-q", tmp_path / "b.q", "--place-taxa", tmp_path / "p.tsv", "--per-taxon", tmp_path / "x.tsv",
            "--per-tree", tmp_path / "t.tsv", "--save-table", tmp_path / "table.bin")
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "a.nwk").read_bytes() == (tmp_path / "b.nwk").read_bytes()
    assert (tmp_path / "a.q").read_bytes() == (tmp_path / "b.q").read_bytes()
    assert (tmp_path / "t.tsv").exists() and (tmp_path / "x.tsv").exists()

    ref = flatten.flatten_reference(ref_nw)
    rows = read_tsv(tmp_path / "p.tsv")
    want = model_rows(ref, trees, list(range(n)))
    assert rows == want
    assert any(int(r[4]) > 0 for r in rows)   # random trees against a random reference: taxa would move
    # current = the concordant column of --per-taxon
    support = [ln.split("\t") for ln in (tmp_path / "x.tsv").read_text().splitlines()[1:]]
    assert [r[2] for r in rows] == [s[4] for s in support]

    # a list: unsorted in the file, blank lines, a repeated label -- the lines of the listed taxa, in lookup-id order
    listed = [17, 3, 23, 0, 3]
    (tmp_path / "names.txt").write_text("\n".join(ref.names[i] for i in listed) + "\n\n")
    p = run(*common, "-o", tmp_path / "c.nwk", "--place-taxa", tmp_path / "p1.tsv", "--place-only", tmp_path / "names.txt")
    assert p.returncode == 0, p.stderr
    assert read_tsv(tmp_path / "p1.tsv") == [rows[i] for i in sorted(set(listed))]
    assert (tmp_path / "c.nwk").read_bytes() == (tmp_path / "a.nwk").read_bytes()

    # the saved table, loaded: no trees are counted, the same file; beside --also-ref and --without-taxa
    (tmp_path / "drop.txt").write_text(ref.names[5] + "\n")
    p = run(*common, "-o", tmp_path / "d.nwk", "--load-table", tmp_path / "table.bin", "--place-taxa", tmp_path / "p2.tsv",
            "--also-ref", tmp_path / "r.nwk", tmp_path / "also.nwk", "--without-taxa", tmp_path / "drop.txt", tmp_path / "w.nwk")
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "p2.tsv").read_bytes() == (tmp_path / "p.tsv").read_bytes()
    assert (tmp_path / "d.nwk").read_bytes() == (tmp_path / "a.nwk").read_bytes()
    assert (tmp_path / "also.nwk").exists() and (tmp_path / "w.nwk").exists()


def star_with_clades(n):
    """a root of many children: single leaves and small clades, so that positions tie and parents of more than three links occur"""
    names = [f"t{i}" for i in np.random.default_rng(8).permutation(n)]
    return "(" + ",".join(names[:6] + ["(" + names[6] + "," + names[7] + ")", "(" + ",".join(names[8:12]) + ")", "((" + names[12] + "," +
                          names[13] + ")," + names[14] + ")"] + names[15:]) + ");"


REFERENCES = {
    "rooted": lambda n: synth.random_tree(n, np.random.default_rng(41), rooted=True),
    "rooted_collapsed": lambda n: synth.random_tree(n, np.random.default_rng(42), rooted=True, collapse=0.5),
    "strongly_collapsed": lambda n: synth.random_tree(n, np.random.default_rng(43), collapse=0.8),
    "star": lambda n: "(" + ",".join(f"t{i}" for i in range(n)) + ");",
    "star_with_clades": star_with_clades,
}


@pytest.mark.parametrize("kind", sorted(REFERENCES))
def test_columns_on_rooted_and_collapsed_references(tmp_path, kind):
    # the CLI's own column code where positions tie: a degree-2 root, parents of more than three links, a star
    n = 18
    ref_nw = REFERENCES[kind](n)
    trees = synth.tree_set(n, 9, 50) + synth.tree_set(n, 9, 51, collapse=0.4) + synth.tree_set(n, 6, 52, rooted=True, dropout=0.2)
    (tmp_path / "r.nwk").write_text(ref_nw + "\n")
    (tmp_path / "e.nwk").write_text("\n".join(trees) + "\n")
    p = run("-r", tmp_path / "r.nwk", "-e", tmp_path / "e.nwk", "-o", tmp_path / "o.nwk", "--place-taxa", tmp_path / "p.tsv")
    assert p.returncode == 0, p.stderr
    ref = flatten.flatten_reference(ref_nw)
    rows = read_tsv(tmp_path / "p.tsv")
    assert rows == model_rows(ref, trees, list(range(n)))
    if kind == "star":
        assert all(r[2] == "0" for r in rows)            # a star resolves no quartet: nothing is concordant where the taxa stand


def test_planted_misplacement_through_the_cli(tmp_path):
    ref_nw, trees, true_side, moved = P.planted()
    (tmp_path / "r.nwk").write_text(ref_nw + "\n")
    (tmp_path / "e.nwk").write_text("\n".join(trees) + "\n")
    (tmp_path / "names.txt").write_text("tx\n")
    p = run("-r", tmp_path / "r.nwk", "-e", tmp_path / "e.nwk", "-o", tmp_path / "o.nwk", "--place-taxa", tmp_path / "p.tsv",
            "--place-only", tmp_path / "names.txt")
    assert p.returncode == 0, p.stderr
    ref = flatten.flatten_reference(ref_nw)
    (row,) = read_tsv(tmp_path / "p.tsv")
    col = dict(zip(P.COLUMNS, row))
    assert col["name"] == "tx" and int(col["taxon"]) == ref.name_to_id["tx"]
    assert int(col["n_best"]) == 1 and int(col["gain"]) > 0 and int(col["distance"]) == moved
    assert {ref.names[i] for i in range(int(col["best_lo"]), int(col["best_hi"]))} - {"tx"} == true_side
    assert row == model_rows(ref, trees, [ref.name_to_id["tx"]])[0]
