"""QuartetScores --test-groups SPEC FILE on the device: one line per hypothesis whose integer columns are Context.group_support's on
the same inputs and whose ratios are the Python host's, the other outputs byte-identical with and without the flag, the same file
from --load-table of the saved table, and the refusals before anything is written."""
import math
import os
import subprocess

import numpy as np
import pytest

from quartetscores_amd import flatten, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "quartetscores_amd", "bin", "QuartetScores")
HEADER = ["name", "kind", "quartets", "q1", "q2", "q3", "outvoted", "uninformed", "support", "qpic"]


def run(*args):
    return subprocess.run([BIN, *map(str, args)], capture_output=True, text=True, timeout=600)


def inputs(tmp_path, n=33, m=42):
    rng = np.random.default_rng(3)
    ref_nw = synth.random_tree(n, rng)
    k = m // 4
    trees = (synth.tree_set(n, k, 4) + synth.tree_set(n, k, 5, collapse=0.3) + synth.tree_set(n, k, 6, dropout=0.4, min_taxa=2)
             + synth.tree_set(n, m - 3 * k, 7, rooted=True))
    (tmp_path / "r.nwk").write_text(ref_nw + "\n")
    (tmp_path / "e.nwk").write_text("\n".join(trees) + "\n")
    return flatten.flatten_reference(ref_nw), trees, ("-r", tmp_path / "r.nwk", "-e", tmp_path / "e.nwk")


def spec_text(ref):
    nm = ref.names
    pick = np.random.default_rng(9).permutation(len(nm))
    g = lambda ids: ",".join(nm[i] for i in ids)
    lines = ["# hypotheses around contested branches", "",
             "edge\t" + "\t".join((g(range(0, 5)), g(range(5, 9)), g(range(9, 20)), g(range(20, 33)))),
             "scattered\t" + "\t".join((g(pick[:3]), g(pick[3:4]), g(pick[4:11]), g(pick[11:13]))),
             "mono\t" + g(range(4, 11)) + "\t*",
             "  # an indented comment",
             "rest\t*\t" + g(pick[:2]),
             "two_sets\t" + g(pick[5:9]) + "\t" + g(pick[20:31])]
    lines += [f"h{i}\t{nm[pick[i]]}\t{nm[pick[i + 1]]}\t{nm[pick[i + 2]]}\t{g(pick[i + 3:i + 6])}" for i in range(6)]   # more than one pass
    return "\n".join(lines) + "\n"


def fmt(x):
    return "nan" if math.isnan(x) else "%.6f" % x


def test_test_groups_file(tmp_path):
    from quartetscores_amd import engine
    ref, trees, common = inputs(tmp_path)
    text = spec_text(ref)
    (tmp_path / "spec.tsv").write_text(text)
    p = run(*common, "-o", tmp_path / "a.nwk", "-q", tmp_path / "a.q")
    assert p.returncode == 0, p.stderr
    p = run(*common, "-o", tmp_path / "b.nwk", "-q", tmp_path / "b.q", "--test-groups", tmp_path / "spec.tsv", tmp_path / "g.tsv",
            "--per-taxon", tmp_path / "x.tsv", "--save-table", tmp_path / "table.bin")
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "a.nwk").read_bytes() == (tmp_path / "b.nwk").read_bytes()
    assert (tmp_path / "a.q").read_bytes() == (tmp_path / "b.q").read_bytes()
    assert (tmp_path / "x.tsv").exists()

    names, labels = engine.parse_group_spec(text, ref.name_to_id)
    assert len(names) == 11
    kind, _ = engine.group_check(ref.n_taxa, labels)
    ctx = engine.Context(ref.n_taxa, 16)
    ctx.table_alloc()
    ctx.count_trees(flatten.flatten_eval_trees(trees, ref.name_to_id))
    words = ctx.group_support(labels)
    cols = engine.group_columns(kind, words)
    want = [[names[h], engine.GROUP_KINDS[kind[h]]] + [str(int(x)) for x in words[h]] + [fmt(cols["support"][h]), fmt(cols["qpic"][h])]
            for h in range(len(names))]
    lines = (tmp_path / "g.tsv").read_text().splitlines()
    assert lines[0].split("\t") == HEADER
    assert [ln.split("\t") for ln in lines[1:]] == want
    assert {row[1] for row in want} == {"quad", "split"} and all(row[9] == "nan" for row in want if row[1] == "split")
    assert all(row[9] != "nan" for row in want if row[1] == "quad") and any(int(row[3]) > 0 for row in want)

    # the saved table, loaded: no trees are counted, the same file, the other outputs as before
    p = run(*common, "-o", tmp_path / "c.nwk", "-q", tmp_path / "c.q", "--load-table", tmp_path / "table.bin",
            "--test-groups", tmp_path / "spec.tsv", tmp_path / "g2.tsv")
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "g2.tsv").read_bytes() == (tmp_path / "g.tsv").read_bytes()
    assert (tmp_path / "c.nwk").read_bytes() == (tmp_path / "a.nwk").read_bytes()
    assert (tmp_path / "c.q").read_bytes() == (tmp_path / "a.q").read_bytes()


def test_refusals_before_anything_is_written(tmp_path):
    ref, trees, common = inputs(tmp_path, n=12, m=8)
    nm = ref.names
    good = f"ok\t{nm[0]},{nm[1]}\t{nm[2]},{nm[3]}\n"
    (tmp_path / "spec.tsv").write_text(good)
    out = tmp_path / "o.nwk"

    def refused(args, *words, spec=None):
        if spec is not None:
            (tmp_path / "bad.tsv").write_text(good + spec)
        p = run(*common, "-o", out, *args)
        assert p.returncode == 1
        for w in words:
            assert w in p.stderr, p.stderr
        assert not out.exists() and not (tmp_path / "g.tsv").exists()

    tg = ("--test-groups", tmp_path / "spec.tsv", tmp_path / "g.tsv")
    refused(tg + ("--gpus", 2), "--test-groups needs the whole count table on one GPU")
    refused(tg + ("--table-shards", 2), "--test-groups needs the whole count table on one GPU")
    refused(("--test-groups", tmp_path / "spec.tsv", out), "is also another output file")
    refused(("--test-groups", tmp_path / "spec.tsv", tmp_path / "q.txt", "-q", tmp_path / "q.txt"), "is also another output file")
    (tmp_path / "there.tsv").write_text("x\n")
    refused(("--test-groups", tmp_path / "spec.tsv", tmp_path / "there.tsv"), "there.tsv already exists")
    bad = ("--test-groups", tmp_path / "bad.tsv", tmp_path / "g.tsv")
    refused(bad, "bad.tsv line 2", "unknown taxon 'nobody'", spec=f"x\t{nm[0]},nobody\t{nm[2]},{nm[3]}\n")
    refused(bad, "bad.tsv line 3", f"'{nm[2]}'", "two groups", spec=f"\nx\t{nm[0]},{nm[2]}\t{nm[2]},{nm[3]}\n")
    refused(bad, "bad.tsv line 2", "group 2 is empty", spec=f"x\t{nm[0]},{nm[1]}\t\n")
    refused(bad, "bad.tsv line 2", "group 1", "at least two taxa", spec=f"x\t{nm[0]}\t{nm[2]},{nm[3]}\n")
    refused(bad, "bad.tsv line 2", "found 3 group(s)", spec=f"x\t{nm[0]}\t{nm[1]}\t{nm[2]}\n")
    refused(bad, "bad.tsv line 2", "found 5 group(s)", spec=f"x\t{nm[0]}\t{nm[1]}\t{nm[2]}\t{nm[3]}\t{nm[4]}\n")
    refused(bad, "bad.tsv line 2", "'*'", spec=f"x\t*\t{nm[1]}\t{nm[2]}\t{nm[3]}\n")
    p = run(*common, "-o", out, "--test-groups", tmp_path / "spec.tsv")
    assert p.returncode == 1 and "--test-groups" in p.stderr and not out.exists()
