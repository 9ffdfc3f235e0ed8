"""QuartetScores --taxon-pairs FILE [--taxon-pairs-only NAMES] without a GPU: every refusal comes before the device is touched, with
a non-zero exit, its message and no output file; the binding declares qs_taxon_pair_support; engine.taxon_pair_columns equals the
columns tests/taxon_pair_model.py defines."""
import os
import subprocess

import numpy as np
import pytest

import bruteforce
import taxon_pair_model as M
from quartetscores_amd import _lib, engine, flatten, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "quartetscores_amd", "bin", "QuartetScores")
N = 12


def run(*args):
    return subprocess.run([BIN, *map(str, args)], capture_output=True, text=True, timeout=600)


@pytest.fixture()
def files(tmp_path):
    (tmp_path / "r.nwk").write_text(synth.reference_tree(N, 1) + "\n")
    (tmp_path / "e.nwk").write_text("\n".join(synth.tree_set(N, 6, 2)) + "\n")
    (tmp_path / "names.txt").write_text("\nt3\nt7 \n\nt3\n")
    (tmp_path / "unknown.txt").write_text("t3\nt99\n")
    return tmp_path


def base(files):
    return ["-r", files / "r.nwk", "-e", files / "e.nwk", "-o", files / "o.nwk"]


def nothing_written(files):
    return not (files / "p.tsv").exists() and not (files / "o.nwk").exists()


def test_missing_value(files):
    for flag in ("--taxon-pairs", "--taxon-pairs-only"):
        p = run(*base(files), flag)
        assert p.returncode == 1 and "Missing a value for this argument! for arg " + flag in p.stderr, p.stderr
    assert nothing_written(files)


@pytest.mark.parametrize("extra", [["--gpus", "2"], ["--table-shards", "2"]])
def test_refused_without_the_whole_table_on_one_gpu(files, extra):
    p = run(*base(files), "--taxon-pairs", files / "p.tsv", *extra, "--trace")
    assert p.returncode == 1 and "--taxon-pairs needs the whole count table on one GPU" in p.stderr, p.stderr
    assert "[trace]" not in p.stderr and nothing_written(files)


def test_refused_existing_file(files):
    (files / "p.tsv").write_text("keep\n")
    p = run(*base(files), "--taxon-pairs", files / "p.tsv", "--trace")
    assert p.returncode == 1 and "--taxon-pairs: the output file" in p.stderr and "already exists" in p.stderr, p.stderr
    assert "[trace]" not in p.stderr
    assert (files / "p.tsv").read_text() == "keep\n" and not (files / "o.nwk").exists()


@pytest.mark.parametrize("other", ["-o", "-q", "--per-tree", "--per-taxon", "--place-taxa", "--place-clades", "--tree-distances", "--save-table"])
def test_refused_file_that_is_another_output(files, other):
    shared = files / "shared.out"
    args = ["-r", files / "r.nwk", "-e", files / "e.nwk", "--taxon-pairs", shared]
    args += ["-o", shared] if other == "-o" else ["-o", files / "o.nwk", other, shared]
    p = run(*args, "--trace")
    assert p.returncode == 1 and "is also another output file" in p.stderr, p.stderr
    assert "[trace]" not in p.stderr and not shared.exists() and not (files / "o.nwk").exists()


def test_only_needs_the_flag(files):
    p = run(*base(files), "--taxon-pairs-only", files / "names.txt", "--trace")
    assert p.returncode == 1 and "--taxon-pairs-only needs --taxon-pairs FILE" in p.stderr, p.stderr
    assert "[trace]" not in p.stderr and nothing_written(files)


def test_unknown_name_is_named_before_the_device(files):
    p = run(*base(files), "--taxon-pairs", files / "p.tsv", "--taxon-pairs-only", files / "unknown.txt", "--trace")
    assert p.returncode == 1 and "--taxon-pairs-only" in p.stderr and "t99" in p.stderr and "not in the reference tree" in p.stderr, p.stderr
    assert "[trace]" not in p.stderr and "no HIP device" not in p.stderr and nothing_written(files)


def test_usage_names_the_flags():
    text = run("-h").stdout
    assert "--taxon-pairs F" in text and "--taxon-pairs-only NAMES" in text


def test_the_binding_declares_the_call():
    assert "qs_taxon_pair_support" in _lib.EXPORTS
    L = _lib.load()
    assert len(L.qs_taxon_pair_support.argtypes) == 5 and L.qs_taxon_pair_support.restype is not None


def test_engine_columns_equal_the_models():
    rng = np.random.default_rng(3)
    for kw in ({}, {"collapse": 0.5}, {"collapse": 1.0}):
        ref_nw = synth.random_tree(9, rng, **kw)
        ref = flatten.flatten_reference(ref_nw)
        table = bruteforce.count_table(ref.names, synth.tree_set(9, 5, 4, dropout=0.3) + synth.tree_set(9, 3, 5, collapse=0.5))
        for taxa in (None, [4], [8, 0, 3]):
            counts = M.pair_counts(table, ref, taxa)
            got, want = engine.taxon_pair_columns(counts, ref.names, taxa), M.columns(counts, ref.names, taxa)
            assert list(got) == list(want) == list(M.COLUMNS) == list(engine.TAXON_PAIR_COLUMNS)
            for name in M.COLUMNS:
                if name.startswith("name_"):
                    assert list(got[name]) == list(want[name])
                else:
                    assert got[name].dtype == want[name].dtype and np.array_equal(got[name], want[name], equal_nan=want[name].dtype == np.float64), name
            assert len(got["a"]) == (36 if taxa is None else sum(8 - k for k in range(len(taxa))))
    assert engine.TAXON_PAIR_FIELDS == M.FIELDS
