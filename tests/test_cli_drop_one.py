"""QuartetScores --drop-one FILE [--drop-one-only NAMES] without a GPU: every refusal comes before the device is touched, with a
non-zero exit, its message and no output file; the binding declares qs_branch_taxon_support; engine.drop_one_columns equals the
lines tests/branch_taxon_model.py defines."""
import math
import os
import subprocess

import numpy as np
import pytest

import branch_taxon_model as M
import bruteforce
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
    return not (files / "d.tsv").exists() and not (files / "o.nwk").exists()


def test_missing_value(files):
    for flag in ("--drop-one", "--drop-one-only"):
        p = run(*base(files), flag)
        assert p.returncode == 1 and "Missing a value for this argument! for arg " + flag in p.stderr, p.stderr
    assert nothing_written(files)


@pytest.mark.parametrize("extra", [["--gpus", "2"], ["--table-shards", "2"]])
def test_refused_without_the_whole_table_on_one_gpu(files, extra):
    p = run(*base(files), "--drop-one", files / "d.tsv", *extra, "--trace")
    assert p.returncode == 1 and "--drop-one needs the whole count table on one GPU" in p.stderr, p.stderr
    assert "[trace]" not in p.stderr and nothing_written(files)


def test_refused_existing_file(files):
    (files / "d.tsv").write_text("keep\n")
    p = run(*base(files), "--drop-one", files / "d.tsv", "--trace")
    assert p.returncode == 1 and "--drop-one: the output file" in p.stderr and "already exists" in p.stderr, p.stderr
    assert "[trace]" not in p.stderr
    assert (files / "d.tsv").read_text() == "keep\n" and not (files / "o.nwk").exists()


@pytest.mark.parametrize("other", ["-o", "-q", "--per-taxon", "--place-taxa", "--taxon-pairs", "--save-table"])
def test_refused_file_that_is_another_output(files, other):
    shared = files / "shared.out"
    args = ["-r", files / "r.nwk", "-e", files / "e.nwk", "--drop-one", shared]
    args += ["-o", shared] if other == "-o" else ["-o", files / "o.nwk", other, shared]
    p = run(*args, "--trace")
    assert p.returncode == 1 and "is also another output file" in p.stderr, p.stderr
    assert "[trace]" not in p.stderr and not shared.exists() and not (files / "o.nwk").exists()


def test_only_needs_the_flag(files):
    p = run(*base(files), "--drop-one-only", files / "names.txt", "--trace")
    assert p.returncode == 1 and "--drop-one-only needs --drop-one FILE" in p.stderr, p.stderr
    assert "[trace]" not in p.stderr and nothing_written(files)


def test_unknown_name_is_named_before_the_device(files):
    p = run(*base(files), "--drop-one", files / "d.tsv", "--drop-one-only", files / "unknown.txt", "--trace")
    assert p.returncode == 1 and "--drop-one-only" in p.stderr and "t99" in p.stderr and "not in the reference tree" in p.stderr, p.stderr
    assert "[trace]" not in p.stderr and "no HIP device" not in p.stderr and nothing_written(files)


def test_usage_names_the_flags():
    text = run("-h").stdout
    assert "--drop-one F" in text and "--drop-one-only NAMES" in text


def test_the_binding_declares_the_call():
    assert "qs_branch_taxon_support" in _lib.EXPORTS
    L = _lib.load()
    assert len(L.qs_branch_taxon_support.argtypes) == 6 and L.qs_branch_taxon_support.restype is not None


def test_engine_columns_equal_the_models():
    rng = np.random.default_rng(3)
    nans = numbers = through_root = 0
    for kw in ({}, {"collapse": 0.4}, {"rooted": True}, {"collapse": 1.0}):
        ref_nw = synth.random_tree(9, rng, **kw)
        ref = flatten.flatten_reference(ref_nw)
        table = bruteforce.count_table(ref.names, synth.tree_set(9, 5, 4, dropout=0.3) + synth.tree_set(9, 3, 5, collapse=0.5))
        every, totals = M.model(table, ref)
        edges = M.internodes(ref)
        merged = [v for v, w in edges if ref.parent[v] != w]
        through_root += int(bool(merged))
        for taxa in (None, [4], [8, 0, 3]):
            ids = list(range(9)) if taxa is None else taxa
            got = engine.drop_one_columns(ref, taxa, every[ids], totals)
            want = M.columns(ref, ids, every[ids], totals)
            assert list(got) == list(engine.DROP_ONE_COLUMNS)
            assert len(want) == len(ids) * (len(edges) - len(merged) // 2) == len(got["taxon"])
            for i, line in enumerate(want):
                for name, val in zip(engine.DROP_ONE_COLUMNS, line):
                    g = got[name][i]
                    if name in ("qpic", "qpic_without", "delta"):
                        assert ("nan" if math.isnan(g) else "%.6f" % g) == val, (name, i)
                    else:
                        assert g == val and (name == "name" or got[name].dtype == np.int64), (name, i)
                # nan exactly where the taxon is alone in its link at an end of degree 3
                x, v, group = line[0], line[2], line[5]
                w = dict(edges)[v]
                end = v if line[3] <= x < line[4] else w
                degree3 = len(M.links_at(ref, end, w if end == v else v)) == 2
                assert (line[11] == "nan") == (group == 1 and degree3) == (line[12] == "nan"), line
                nans += int(line[11] == "nan")
                numbers += int(line[11] != "nan")
    assert engine.BRANCH_TAXON_FIELDS == M.FIELDS
    assert nans and numbers and through_root
