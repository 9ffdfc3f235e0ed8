"""QuartetScores --species-map FILE without a GPU: every argument error, map-file error and refused combination comes before the
device is touched, with a non-zero exit, a message that names the flag or the label, and no output file."""
import os
import subprocess

import pytest

from quartetscores_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "quartetscores_amd", "bin", "QuartetScores")
REF = "((A,B),(C,(D,E)),F);"
TREES = ["((a1,a2),(B,c1),(D,(E,F)));", "((a1,B),(c1,a2),((D,E),F));"]


def run(*args):
    return subprocess.run([BIN, *map(str, args)], capture_output=True, text=True, timeout=600)


@pytest.fixture()
def files(tmp_path):
    (tmp_path / "r.nwk").write_text(REF + "\n")
    (tmp_path / "e.nwk").write_text("\n".join(TREES) + "\n")
    (tmp_path / "map.txt").write_text("# two individuals of A\nA: a1, a2\nC:c1\n")
    return tmp_path


def base(files):
    return ["-r", files / "r.nwk", "-e", files / "e.nwk", "-o", files / "o.nwk"]


def refused(files, args, *words):
    p = run(*base(files), *args, "--trace")
    assert p.returncode == 1, (p.stdout, p.stderr)
    for w in words:
        assert w in p.stderr, p.stderr
    assert "[trace]" not in p.stderr and "no HIP device" not in p.stderr      # before the device is touched
    assert not (files / "o.nwk").exists() and not (files / "x.out").exists()


def test_missing_value(files):
    p = run(*base(files), "--species-map")
    assert p.returncode == 1 and "Missing a value for this argument! for arg --species-map" in p.stderr, p.stderr
    assert not (files / "o.nwk").exists()


def test_missing_file(files):
    refused(files, ["--species-map", files / "nothing.txt"], "nothing.txt")


@pytest.mark.parametrize("text,words", [
    ("X:x1,x2\n", ["line 1", "'X'", "not a leaf of the reference tree"]),
    ("A:a1,a2\n\n#c\nC:c1,a1\n", ["line 4", "'a1'", "listed twice", "'A'", "'C'"]),
    ("A:a1,a2,a1\n", ["line 1", "'a1'", "listed twice"]),
    ("A:a1,B\n", ["'B'", "unlisted species"]),
    ("A:\n", ["line 1", "'A'", "empty individual list"]),
    ("A:a1,,a2\n", ["line 1", "'A'", "empty individual name"]),
    ("A:a1\nA:a2\n", ["line 2", "'A'", "two lines"]),
    ("A a1 a2\n", ["line 1", "no ':'", "'A a1 a2'"]),
    ("A:" + ",".join(f"a{i}" for i in range(4092)) + "\n", ["more than 4096 individuals", "'F'"]),   # (4097 with the other five: F is where the count passes 4096)
], ids=["unknown-species", "twice-two-species", "twice-one-species", "unlisted-species-name", "empty-list", "empty-name", "two-lines", "no-colon", "too-many"])
def test_map_file_errors_name_the_label(files, text, words):
    (files / "bad.txt").write_text(text)
    refused(files, ["--species-map", files / "bad.txt"], "--species-map", "bad.txt", *words)


def test_an_individual_may_carry_the_name_of_a_listed_species(files):
    # (A is listed, so the label A is free for one of its individuals: no error of the map; the run then needs the device)
    (files / "ok.txt").write_text("A:A,a2\n")
    p = run(*base(files), "--species-map", files / "ok.txt", "--gpus", 2)
    assert p.returncode == 1 and "--gpus" in p.stderr and "ok.txt" not in p.stderr


def test_fewer_than_four_species(files):
    (files / "r.nwk").write_text("(A,B,C);\n")
    refused(files, ["--species-map", files / "map.txt"], "--species-map", "fewer than 4 species")


@pytest.mark.parametrize("extra,words", [
    (["--load-table", "x.out"], ["--species-map", "--load-table"]),
    (["--gpus", "2"], ["--species-map", "--gpus"]),
    (["--table-shards", "2"], ["--species-map", "--table-shards"]),
])
def test_refused_routes(files, extra, words):
    refused(files, ["--species-map", files / "map.txt", *[files / x if x.endswith(".out") else x for x in extra]], *words)


@pytest.mark.parametrize("flag", ["--per-tree", "--tree-distances", "--branch-trees", "--bootstrap", "--local-pp", "--tree-taxa"])
def test_refused_with_the_outputs_computed_from_the_trees(files, flag):
    refused(files, ["--species-map", files / "map.txt", flag, files / "x.out"], flag, "--species-map", "individuals")


def test_usage_names_the_flag():
    text = run("-h").stdout
    assert "--species-map FILE" in text and "species:ind1,ind2" in text


def test_the_binding_declares_the_call():
    assert "qs_table_collapse" in _lib.EXPORTS
    L = _lib.load()
    assert len(L.qs_table_collapse.argtypes) == 3 and L.qs_table_collapse.restype is not None
