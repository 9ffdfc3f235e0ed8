"""QuartetScores --also-ref REF OUT: further reference trees scored from the count table of -r (qs_table_remap), and
flatten.taxon_permutation, the id map behind it."""
import os
import subprocess

import numpy as np
import pytest

from quartetscores_amd import flatten, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "quartetscores_amd", "bin", "QuartetScores")


def run(*args):
    return subprocess.run([BIN, *map(str, args)], capture_output=True, text=True, timeout=600)


@pytest.fixture()
def files(tmp_path):
    n = 20
    rng = np.random.default_rng(5)
    trees = {"a": synth.reference_tree(n, 1), "b": synth.reference_tree(n, 2), "m": synth.random_tree(n, rng, collapse=0.4),
             "x": synth.reference_tree(n + 1, 3)}
    paths = {}
    for k, nw in trees.items():
        paths[k] = tmp_path / f"{k}.nwk"
        paths[k].write_text(nw + "\n")
    ev = synth.tree_set(n, 25, 6, dropout=0.2) + synth.tree_set(n, 25, 7, collapse=0.3) + synth.tree_set(n, 10, 8, rooted=True)
    paths["e"] = tmp_path / "eval.nwk"
    paths["e"].write_text("\n".join(ev) + "\n")
    return paths


# ---- without a GPU --------------------------------------------------------------------------------------------------

def test_missing_second_value(files, tmp_path):
    for tail in ([files["b"]], [files["b"], "-v"]):
        p = run("-r", files["a"], "-e", files["e"], "-o", tmp_path / "o.nwk", "--also-ref", *tail)
        assert p.returncode == 1 and "--also-ref" in p.stderr, p.stderr
    assert not (tmp_path / "o.nwk").exists()


def test_existing_or_repeated_output_is_refused(files, tmp_path):
    (tmp_path / "taken.nwk").write_text("x\n")
    p = run("-r", files["a"], "-e", files["e"], "-o", tmp_path / "o.nwk", "--also-ref", files["b"], tmp_path / "taken.nwk")
    assert p.returncode == 1 and "taken.nwk" in p.stderr and "already exists" in p.stderr, p.stderr
    for out in (tmp_path / "o.nwk", tmp_path / "b.out"):   # the -o file, another --also-ref output
        p = run("-r", files["a"], "-e", files["e"], "-o", tmp_path / "o.nwk", "--also-ref", files["b"], tmp_path / "b.out",
                "--also-ref", files["m"], out)
        assert p.returncode == 1 and "given twice" in p.stderr, p.stderr
    assert (tmp_path / "taken.nwk").read_text() == "x\n"


def test_different_taxon_set_is_refused_before_the_device(files, tmp_path):
    p = run("-r", files["a"], "-e", files["e"], "-o", tmp_path / "o.nwk", "--also-ref", files["x"], tmp_path / "x.out", "--trace")
    assert p.returncode == 1, p.stderr
    assert "taxa differ" in p.stderr and "extra: t20" in p.stderr, p.stderr
    assert "[trace]" not in p.stderr                  # ended before the run's first step (the HIP start-up follows it)
    assert "no HIP device" not in p.stderr
    assert not (tmp_path / "o.nwk").exists() and not (tmp_path / "x.out").exists()


@pytest.mark.parametrize("flag", [["--gpus", "2"], ["--table-shards", "2"]])
def test_multi_gpu_and_table_shards_are_refused(files, tmp_path, flag):
    p = run("-r", files["a"], "-e", files["e"], "-o", tmp_path / "o.nwk", "--also-ref", files["b"], tmp_path / "b.out", *flag)
    assert p.returncode == 1 and "--also-ref works on one GPU" in p.stderr, p.stderr
    assert not (tmp_path / "o.nwk").exists()


def test_taxon_permutation():
    a = flatten.flatten_reference("((t0,t1),(t2,t3),(t4,t5));")
    b = flatten.flatten_reference("((t5,t2),(t0,t4),(t3,t1));")
    perm = flatten.taxon_permutation(b, a)
    assert perm.dtype == np.uint16
    assert [a.names[i] for i in perm] == b.names
    assert list(flatten.taxon_permutation(a, a)) == list(range(6))
    assert list(flatten.taxon_permutation(a, b)[perm]) == list(range(6))      # the inverse


def test_taxon_permutation_names_missing_and_extra_taxa():
    a = flatten.flatten_reference("((t0,t1),(t2,t3),(t4,t5));")
    b = flatten.flatten_reference("((t0,t1),(t2,t3),(t4,t9));")
    with pytest.raises(ValueError, match=r"missing t5; extra t9"):
        flatten.taxon_permutation(b, a)


# ---- on the GPU -----------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("flags", [[], ["--exact-qp", "--root-as-edge"]])
def test_also_ref_outputs_equal_separate_runs(files, tmp_path, flags):
    d = tmp_path
    one = run("-r", files["a"], "-e", files["e"], "-o", d / "a_alone.nwk", *flags)
    assert one.returncode == 0, one.stderr
    sep = {}
    for k in ("b", "m"):
        p = run("-r", files[k], "-e", files["e"], "-o", d / f"{k}_alone.nwk", *flags)
        assert p.returncode == 0, p.stderr
        sep[k] = (d / f"{k}_alone.nwk").read_bytes()
    p = run("-r", files["a"], "-e", files["e"], "-o", d / "a_out.nwk", "--also-ref", files["b"], d / "b_out.nwk",
            "--also-ref", files["m"], d / "m_out.nwk", "--save-table", d / "table.bin", *flags)
    assert p.returncode == 0, p.stderr
    assert (d / "a_out.nwk").read_bytes() == (d / "a_alone.nwk").read_bytes()
    assert (d / "b_out.nwk").read_bytes() == sep["b"] and (d / "m_out.nwk").read_bytes() == sep["m"]
    # stdout: the primary block as without --also-ref, then one block per further tree
    assert p.stdout.count("Finished computing scores.") == 3
    assert "Scoring the reference tree %s from the same count table." % files["m"] in p.stdout
    assert "Remapped the count table in " in p.stdout and "The reference tree is multifurcating." in p.stdout
    # a saved table scores further trees later
    p = run("-r", files["a"], "-e", files["e"], "-o", d / "a2.nwk", "--load-table", d / "table.bin",
            "--also-ref", files["m"], d / "m2.nwk", "--also-ref", files["b"], d / "b2.nwk", *flags)
    assert p.returncode == 0, p.stderr
    assert (d / "a2.nwk").read_bytes() == (d / "a_alone.nwk").read_bytes()
    assert (d / "b2.nwk").read_bytes() == sep["b"] and (d / "m2.nwk").read_bytes() == sep["m"]
