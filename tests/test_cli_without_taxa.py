"""QuartetScores --without-taxa NAMES OUT: the -r tree scored without the listed taxa from the count table of the full
run (pruning + qs_table_restrict), against separate runs on pruned input files."""
import os
import subprocess

import numpy as np
import pytest

from quartetscores_amd import newick, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "quartetscores_amd", "bin", "QuartetScores")
N = 20


def run(*args):
    return subprocess.run([BIN, *map(str, args)], capture_output=True, text=True, timeout=600)


def pruned_text(nw, drop):
    root = newick.prune(newick.parse_tree(nw), drop)
    if root is None or sum(x.is_leaf for x in newick.preorder(root)) < 4:
        return None
    return newick.write(root)


@pytest.fixture()
def files(tmp_path):
    rng = np.random.default_rng(15)
    ref = synth.reference_tree(N, 11)
    leaves = [x.name for x in newick.preorder(newick.parse_tree(ref)) if x.is_leaf]
    first = newick.parse_tree(ref).children[0]
    drops = {"one": ["t3"], "some": [f"t{i}" for i in rng.choice(N, size=6, replace=False)],
             "subtree": [x.name for x in newick.preorder(first) if x.is_leaf],      # a whole root subtree (rule 4 of the pruner)
             "many": leaves[:N - 3], "unknown": ["t3", "t99"]}
    assert 2 <= len(drops["subtree"]) <= N - 4
    paths = {"r": tmp_path / "ref.nwk", "m": tmp_path / "multi.nwk", "b": tmp_path / "other.nwk", "e": tmp_path / "eval.nwk"}
    paths["r"].write_text(ref + "\n")
    paths["m"].write_text(synth.random_tree(N, rng, collapse=0.4) + "\n")
    paths["b"].write_text(synth.reference_tree(N, 12) + "\n")
    ev = synth.tree_set(N, 25, 16, dropout=0.2) + synth.tree_set(N, 25, 17, collapse=0.3) + synth.tree_set(N, 10, 18, rooted=True)
    paths["e"].write_text("\n".join(ev) + "\n")
    for k, names in drops.items():
        paths[k] = tmp_path / f"{k}.txt"
        # blank lines, a repeated name and trailing blanks do not matter
        paths[k].write_text("\n" + "\n".join(names) + "\n\n" + names[0] + " \n")
    paths["empty"] = tmp_path / "empty.txt"
    paths["empty"].write_text("\n \n")
    return paths, drops, ev


def base(paths, tmp_path, ref="r"):
    return ["-r", paths[ref], "-e", paths["e"], "-o", tmp_path / "o.nwk"]


# ---- without a GPU --------------------------------------------------------------------------------------------------

def test_missing_second_value(files, tmp_path):
    paths = files[0]
    for tail in ([paths["one"]], [paths["one"], "-v"]):
        p = run(*base(paths, tmp_path), "--without-taxa", *tail)
        assert p.returncode == 1 and "--without-taxa" in p.stderr and "NAMES OUT" in p.stderr, p.stderr
    assert not (tmp_path / "o.nwk").exists()


def test_unknown_name_is_named_before_the_device(files, tmp_path):
    paths = files[0]
    p = run(*base(paths, tmp_path), "--without-taxa", paths["unknown"], tmp_path / "x.out", "--trace")
    assert p.returncode == 1 and "t99" in p.stderr and "not in the reference tree" in p.stderr, p.stderr
    assert "[trace]" not in p.stderr and "no HIP device" not in p.stderr
    assert not (tmp_path / "o.nwk").exists() and not (tmp_path / "x.out").exists()


def test_empty_list_is_refused(files, tmp_path):
    paths = files[0]
    p = run(*base(paths, tmp_path), "--without-taxa", paths["empty"], tmp_path / "x.out", "--trace")
    assert p.returncode == 1 and "empty" in p.stderr and "[trace]" not in p.stderr, p.stderr


def test_fewer_than_four_taxa_left_is_refused(files, tmp_path):
    paths = files[0]
    p = run(*base(paths, tmp_path), "--without-taxa", paths["many"], tmp_path / "x.out", "--trace")
    assert p.returncode == 1 and "fewer than four taxa" in p.stderr and "[trace]" not in p.stderr, p.stderr
    assert not (tmp_path / "x.out").exists()


def test_existing_or_repeated_output_is_refused(files, tmp_path):
    paths = files[0]
    (tmp_path / "taken.nwk").write_text("x\n")
    p = run(*base(paths, tmp_path), "--without-taxa", paths["one"], tmp_path / "taken.nwk")
    assert p.returncode == 1 and "taken.nwk" in p.stderr and "already exists" in p.stderr, p.stderr
    for out in (tmp_path / "o.nwk", tmp_path / "a.out"):     # the -o file, another --without-taxa output
        p = run(*base(paths, tmp_path), "--without-taxa", paths["one"], tmp_path / "a.out", "--without-taxa", paths["some"], out)
        assert p.returncode == 1 and "given twice" in p.stderr, p.stderr
    extra = {"--also-ref": [paths["b"], tmp_path / "same.out"], "--per-taxon": [tmp_path / "same.out"], "-q": [tmp_path / "same.out"]}
    for flag, vals in extra.items():                          # ... and any other output of the run
        p = run(*base(paths, tmp_path), flag, *vals, "--without-taxa", paths["one"], tmp_path / "same.out")
        assert p.returncode == 1 and ("given twice" in p.stderr or "also another output" in p.stderr), (flag, p.stderr)
    assert (tmp_path / "taken.nwk").read_text() == "x\n" and not (tmp_path / "o.nwk").exists()


@pytest.mark.parametrize("flag", [["--gpus", "2"], ["--table-shards", "2"]])
def test_multi_gpu_and_table_shards_are_refused(files, tmp_path, flag):
    paths = files[0]
    p = run(*base(paths, tmp_path), "--without-taxa", paths["one"], tmp_path / "a.out", *flag)
    assert p.returncode == 1 and "--without-taxa works on one GPU" in p.stderr, p.stderr
    assert not (tmp_path / "o.nwk").exists()


def test_usage_names_the_flag():
    assert "--without-taxa NAMES OUT" in run("-h").stdout


# ---- on the GPU -----------------------------------------------------------------------------------------------------

def comments_in_post_order(text):
    """the [comment] ("" = none) of every node of an annotated tree, in the order the nodes end in the text = post-order"""
    out, pending, i = [], "", 0
    while i < len(text):
        ch = text[i]
        if ch == "'":                                          # a quoted label
            i = text.index("'", i + 1) + 1
            continue
        if ch == "[":
            j = text.index("]", i)
            pending = text[i + 1:j]
            i = j + 1
            continue
        if ch in ",);":                                        # every node ends at exactly one of these
            out.append(pending)
            pending = ""
        i += 1
    return out


def annotations(text):
    """{leaf set below an edge: its annotation string}: the tree parsed by newick.py (which skips comments), the comments
    taken from the text node by node"""
    post = []

    def rec(x):
        for c in x.children:
            rec(c)
        post.append(x)
    rec(newick.parse_tree(text))
    notes = comments_in_post_order(text)
    assert len(notes) == len(post)
    out = {}
    for x, note in zip(post, notes):
        key = frozenset(y.name for y in newick.preorder(x) if y.is_leaf)
        assert key not in out
        out[key] = note
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [[], ["--exact-qp", "--root-as-edge"]])
def test_without_taxa_outputs_equal_separate_runs_on_pruned_files(files, tmp_path, flags):
    paths, drops, ev = files
    d = tmp_path
    plain = run("-r", paths["r"], "-e", paths["e"], "-o", d / "plain.nwk", "-q", d / "plain.q", *flags)
    assert plain.returncode == 0, plain.stderr
    p = run("-r", paths["r"], "-e", paths["e"], "-o", d / "full.nwk", "-q", d / "full.q", "--save-table", d / "table.bin",
            "--without-taxa", paths["some"], d / "some.out", "--without-taxa", paths["subtree"], d / "subtree.out", *flags)
    assert p.returncode == 0, p.stderr
    # the primary tree's outputs and stdout block as without the flag
    assert (d / "full.nwk").read_bytes() == (d / "plain.nwk").read_bytes()
    assert (d / "full.q").read_bytes() == (d / "plain.q").read_bytes()
    head = plain.stdout[:plain.stdout.index("Finished computing scores.") + len("Finished computing scores.\n")]
    timeless = lambda s: "\n".join(ln for ln in s.splitlines() if "microseconds" not in ln)   # noqa: E731
    assert timeless(p.stdout).startswith(timeless(head))
    assert p.stdout.count("Finished computing scores.") == 3
    assert "Scoring the reference tree without 6 taxa (%s) from the same count table." % paths["some"] in p.stdout
    assert "Restricted the count table in " in p.stdout
    want = {}
    for k in ("some", "subtree"):
        (d / f"{k}_ref.nwk").write_text(pruned_text(paths["r"].read_text(), drops[k]) + "\n")
        (d / f"{k}_eval.nwk").write_text("\n".join(t for t in (pruned_text(nw, drops[k]) for nw in ev) if t) + "\n")
        q = run("-r", d / f"{k}_ref.nwk", "-e", d / f"{k}_eval.nwk", "-o", d / f"{k}_alone.nwk", *flags)
        assert q.returncode == 0, q.stderr
        want[k] = annotations((d / f"{k}_alone.nwk").read_text().strip())
        got = annotations((d / f"{k}.out").read_text().strip())
        assert got == want[k], k
        assert sum(bool(v) for v in got.values()) >= 3
    # after --load-table: the evaluation trees are not read again
    p = run("-r", paths["r"], "-e", paths["e"], "-o", d / "full2.nwk", "--load-table", d / "table.bin",
            "--without-taxa", paths["subtree"], d / "subtree2.out", "--without-taxa", paths["some"], d / "some2.out", *flags)
    assert p.returncode == 0, p.stderr
    assert (d / "full2.nwk").read_bytes() == (d / "plain.nwk").read_bytes()
    for k in ("some", "subtree"):
        assert annotations((d / f"{k}2.out").read_text().strip()) == want[k], k


@pytest.mark.gpu
def test_beside_also_ref_per_taxon_and_a_multifurcating_reference(files, tmp_path):
    paths, drops, ev = files
    d = tmp_path
    alone = run("-r", paths["m"], "-e", paths["e"], "-o", d / "alone.nwk", "--also-ref", paths["b"], d / "alone_b.nwk",
                "--per-taxon", d / "alone.tsv", "--per-tree", d / "alone_tree.tsv")
    assert alone.returncode == 0, alone.stderr
    p = run("-r", paths["m"], "-e", paths["e"], "-o", d / "o.nwk", "--also-ref", paths["b"], d / "b.nwk", "--per-taxon", d / "o.tsv",
            "--per-tree", d / "tree.tsv", "--without-taxa", paths["some"], d / "some.out", "--trace")
    assert p.returncode == 0, p.stderr
    for x, y in (("o.nwk", "alone.nwk"), ("b.nwk", "alone_b.nwk"), ("o.tsv", "alone.tsv"), ("tree.tsv", "alone_tree.tsv")):
        assert (d / x).read_bytes() == (d / y).read_bytes(), x
    assert "[trace] qs_table_restrict for %s" % paths["some"] in p.stderr
    assert "--without-taxa table allocated" in p.stderr
    assert p.stderr.index("--without-taxa table allocated") < p.stderr.index("qs_table_restrict")
    (d / "ref.nwk").write_text(pruned_text(paths["m"].read_text(), drops["some"]) + "\n")
    (d / "eval.nwk").write_text("\n".join(t for t in (pruned_text(nw, drops["some"]) for nw in ev) if t) + "\n")
    q = run("-r", d / "ref.nwk", "-e", d / "eval.nwk", "-o", d / "sep.nwk")
    assert q.returncode == 0, q.stderr
    assert annotations((d / "some.out").read_text().strip()) == annotations((d / "sep.nwk").read_text().strip())
