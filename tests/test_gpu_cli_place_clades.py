"""QuartetScores --place-clades FILE [--place-clades-only SPEC]: one line per placed clade with the columns the numpy model
(tests/clade_placement_model.py) defines, for the default list and for SPEC lists, the other outputs byte-identical with and
without the flag, the same file from --load-table of the saved table, the planted clade found through the CLI (on the device),
and every refusal before the device is touched (no GPU needed), with no output file left behind."""
import os
import subprocess

import numpy as np
import pytest

import bruteforce
import clade_placement_model as CM
import placement_model as P
from quartetscores_amd import flatten, synth

gpu = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "quartetscores_amd", "bin", "QuartetScores")


def run(*args):
    return subprocess.run([BIN, *map(str, args)], capture_output=True, text=True, timeout=600)


def model_rows(ref, trees, nodes):
    table = bruteforce.count_table(ref.names, trees)
    cols = CM.columns(ref, nodes, P.scores(ref, CM.link_sums(table, ref, nodes)))
    return [[str(cols[name][i]) for name in CM.COLUMNS] for i in range(len(nodes))]


def read_tsv(path):
    lines = path.read_text().splitlines()
    assert lines[0].split("\t") == list(CM.COLUMNS)
    return [ln.split("\t") for ln in lines[1:]]


def spec_line(ref, S, v):
    """a SPEC line for node v: its first and last label (their smallest common subtree is v), tab-separated"""
    a, b = ref.names[int(S.lo[v])], ref.names[int(S.hi[v]) - 1]
    return a if a == b else a + "\t" + b


@gpu
def test_place_clades_file(tmp_path, m=42):
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
    p = run(*common, "-o", tmp_path / "b.nwk", "-q", tmp_path / "b.q", "--place-clades", tmp_path / "c.tsv", "--place-taxa", tmp_path / "p.tsv",
            "--per-taxon", tmp_path / "x.tsv", "--save-table", tmp_path / "table.bin")
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "a.nwk").read_bytes() == (tmp_path / "b.nwk").read_bytes()
    assert (tmp_path / "a.q").read_bytes() == (tmp_path / "b.q").read_bytes()
    assert (tmp_path / "p.tsv").exists() and (tmp_path / "x.tsv").exists()

    ref = flatten.flatten_reference(ref_nw)
    S = P.Shape(ref)
    nodes = CM.eligible(ref)
    rows = read_tsv(tmp_path / "c.tsv")
    assert rows == model_rows(ref, trees, nodes)
    gain = CM.COLUMNS.index("gain")
    assert len(rows) >= 10 and any(int(r[gain]) > 0 for r in rows)   # random trees against a random reference: clades would move

    # a SPEC: its own order, a blank line, a leaf, three labels for one clade -- the lines of the listed clades, renumbered
    listed = [nodes[7], nodes[0], int(ref.leaf_node[5]), nodes[-1]]
    big = max(nodes, key=lambda v: S.hi[v] - S.lo[v])
    if big not in listed:
        listed.append(big)
    text = [spec_line(ref, S, v) for v in listed]
    lo, hi = int(S.lo[big]), int(S.hi[big])
    text[listed.index(big)] = "\t".join([ref.names[hi - 1], " " + ref.names[lo + 1] + " ", ref.names[lo]])
    (tmp_path / "spec.txt").write_text(text[0] + "\n\n" + "\n".join(text[1:]) + "\n")
    p = run(*common, "-o", tmp_path / "c.nwk", "--place-clades", tmp_path / "c1.tsv", "--place-clades-only", tmp_path / "spec.txt")
    assert p.returncode == 0, p.stderr
    assert read_tsv(tmp_path / "c1.tsv") == model_rows(ref, trees, listed)
    by_node = {r[1]: r[2:] for r in rows}
    assert all(r[2:] == by_node[r[1]] for r in read_tsv(tmp_path / "c1.tsv") if r[1] in by_node)
    assert (tmp_path / "c.nwk").read_bytes() == (tmp_path / "a.nwk").read_bytes()

    # the saved table, loaded: no trees are counted, the same file; beside --also-ref and --without-taxa
    (tmp_path / "drop.txt").write_text(ref.names[5] + "\n")
    p = run(*common, "-o", tmp_path / "d.nwk", "--load-table", tmp_path / "table.bin", "--place-clades", tmp_path / "c2.tsv",
            "--also-ref", tmp_path / "r.nwk", tmp_path / "also.nwk", "--without-taxa", tmp_path / "drop.txt", tmp_path / "w.nwk")
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "c2.tsv").read_bytes() == (tmp_path / "c.tsv").read_bytes()
    assert (tmp_path / "d.nwk").read_bytes() == (tmp_path / "a.nwk").read_bytes()
    assert (tmp_path / "also.nwk").exists() and (tmp_path / "w.nwk").exists()


REFERENCES = {
    "rooted": lambda n: synth.random_tree(n, np.random.default_rng(41), rooted=True),
    "rooted_collapsed": lambda n: synth.random_tree(n, np.random.default_rng(42), rooted=True, collapse=0.5),
    "collapsed": lambda n: synth.random_tree(n, np.random.default_rng(43), collapse=0.5),
}


@gpu
@pytest.mark.parametrize("kind", sorted(REFERENCES))
def test_columns_on_rooted_and_collapsed_references(tmp_path, kind):
    # the CLI's own column code where positions tie: a degree-2 root, clades below parents of more than three links
    n = 18
    ref_nw = REFERENCES[kind](n)
    trees = synth.tree_set(n, 9, 50) + synth.tree_set(n, 9, 51, collapse=0.4) + synth.tree_set(n, 6, 52, rooted=True, dropout=0.2)
    (tmp_path / "r.nwk").write_text(ref_nw + "\n")
    (tmp_path / "e.nwk").write_text("\n".join(trees) + "\n")
    p = run("-r", tmp_path / "r.nwk", "-e", tmp_path / "e.nwk", "-o", tmp_path / "o.nwk", "--place-clades", tmp_path / "c.tsv")
    assert p.returncode == 0, p.stderr
    ref = flatten.flatten_reference(ref_nw)
    rows = read_tsv(tmp_path / "c.tsv")
    assert rows and rows == model_rows(ref, trees, CM.eligible(ref))


@gpu
def test_planted_clade_through_the_cli(tmp_path):
    ref_nw, trees, true_side, moved = CM.planted()
    (tmp_path / "r.nwk").write_text(ref_nw + "\n")
    (tmp_path / "e.nwk").write_text("\n".join(trees) + "\n")
    (tmp_path / "spec.txt").write_text("cc\tca\n")
    p = run("-r", tmp_path / "r.nwk", "-e", tmp_path / "e.nwk", "-o", tmp_path / "o.nwk", "--place-clades", tmp_path / "c.tsv",
            "--place-clades-only", tmp_path / "spec.txt")
    assert p.returncode == 0, p.stderr
    ref = flatten.flatten_reference(ref_nw)
    (row,) = read_tsv(tmp_path / "c.tsv")
    col = {k: int(v) for k, v in zip(CM.COLUMNS, row)}
    assert {ref.names[i] for i in range(col["lo"], col["hi"])} == {"ca", "cb", "cc"} and col["size"] == 3 and col["clade"] == 0
    assert col["n_best"] == 1 and col["gain"] > 0 and col["distance"] == moved
    assert {ref.names[i] for i in range(col["best_lo"], col["best_hi"])} - {"ca", "cb", "cc"} == true_side
    assert row == model_rows(ref, trees, [col["node"]])[0]


# ---- refusals before the device is touched: no GPU needed ------------------------------------------------------------------

@pytest.fixture()
def files(tmp_path):
    (tmp_path / "r.nwk").write_text("((a,b),((c,d),(e,(f,(g,(h,i))))));\n")
    (tmp_path / "e.nwk").write_text("\n".join(synth.tree_set(9, 4, 2)) + "\n")
    return tmp_path


def base(files):
    return ["-r", files / "r.nwk", "-e", files / "e.nwk", "-o", files / "o.nwk"]


def refused(files, message, *args):
    p = run(*base(files), *args)
    assert p.returncode == 1 and message in p.stderr, p.stderr
    assert not (files / "c.tsv").exists() and not (files / "o.nwk").exists()


def test_missing_value(files):
    p = run(*base(files), "--place-clades")
    assert p.returncode == 1 and "Missing a value for this argument! for arg --place-clades" in p.stderr, p.stderr
    p = run(*base(files), "--place-clades", files / "c.tsv", "--place-clades-only")
    assert p.returncode == 1 and "Missing a value for this argument! for arg --place-clades-only" in p.stderr, p.stderr


def test_place_clades_only_needs_place_clades(files):
    (files / "spec.txt").write_text("a\tb\n")
    refused(files, "--place-clades-only needs --place-clades", "--place-clades-only", files / "spec.txt")


@pytest.mark.parametrize("text, message", [
    ("a\tb\n\nc\tnobody\n", "spec.txt line 3: the taxon nobody is not in the reference tree"),
    ("a\tb\na\tc\n", "spec.txt line 2: the smallest subtree that holds these labels is the whole reference tree"),
    ("c\td\ni\td\n", "spec.txt line 2: the clade leaves fewer than three taxa outside it (2)"),
    ("e\tg\n\nh\ti\nf\te\n", "spec.txt line 4: the same clade as line 1"),
    ("a\n a \n", "spec.txt line 2: the same clade as line 1"),
    ("\n \n", "the list of clades is empty"),
])
def test_refused_spec(files, text, message):
    (files / "spec.txt").write_text(text)
    refused(files, message, "--place-clades", files / "c.tsv", "--place-clades-only", files / "spec.txt")


@pytest.mark.parametrize("extra", [["--gpus", "2"], ["--table-shards", "2"]])
def test_refused_without_the_whole_table_on_one_gpu(files, extra):
    refused(files, "--place-clades needs the whole count table on one GPU", "--place-clades", files / "c.tsv", *extra)


def test_refused_existing_file(files):
    (files / "keep.tsv").write_text("keep\n")
    refused(files, "already exists", "--place-clades", files / "keep.tsv")
    assert (files / "keep.tsv").read_text() == "keep\n"


@pytest.mark.parametrize("other", ["-o", "-q", "--per-tree", "--per-taxon", "--place-taxa", "--without-taxa"])
def test_refused_file_that_is_another_output(files, other):
    shared = files / "shared.out"
    (files / "drop.txt").write_text("c\n")
    args = ["-r", files / "r.nwk", "-e", files / "e.nwk", "--place-clades", shared]
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
    assert "--place-clades F" in p.stdout + p.stderr and "--place-clades-only SPEC" in p.stdout + p.stderr
