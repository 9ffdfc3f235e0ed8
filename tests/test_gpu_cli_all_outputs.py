"""QuartetScores with every output option at once against the same outputs in three runs of a disjoint third each: every file equal
byte for byte, the annotated tree equal in all four. The outputs share the hooks behind every batch's count and behind the final
sync and promise to work beside every other output; the per-flag tests compare each with its numpy model."""
import os
import subprocess

import numpy as np
import pytest

from quartetscores_amd import flatten, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "quartetscores_amd", "bin", "QuartetScores")


@pytest.mark.parametrize("kind", ["rooted", "multifurcating"])
def test_all_outputs_at_once_equal_the_outputs_in_parts(tmp_path, kind):
    n, m = 12, 30
    rng = np.random.default_rng(3)
    ref_nw = synth.random_tree(n, rng, **{"rooted": {"rooted": True}, "multifurcating": {"collapse": 0.3}}[kind])
    trees = synth.tree_set(n, 10, 4) + synth.tree_set(n, 10, 5, collapse=0.3) + synth.tree_set(n, 10, 6, dropout=0.4, min_taxa=2)
    assert len(trees) == m
    names = flatten.flatten_reference(ref_nw).names
    (tmp_path / "r.nwk").write_text(ref_nw + "\n")
    (tmp_path / "e.nwk").write_text("\n".join(trees) + "\n")
    (tmp_path / "r2.nwk").write_text(synth.random_tree(n, np.random.default_rng(9)) + "\n")
    (tmp_path / "drop.txt").write_text(f"{names[2]}\n{names[9]}\n")
    (tmp_path / "groups.txt").write_text(f"quad\t{names[0]},{names[1]}\t{names[4]}\t{names[7]}\t{names[10]},{names[11]}\n"
                                         f"split\t{names[3]},{names[4]},{names[5]}\t*\n")

    def outputs(tag):
        d = tmp_path / tag
        d.mkdir()
        return [["-q", d / "raw.txt"], ["--qic-binary", d / "raw.bin"], ["--save-table", d / "table.bin"], ["--per-tree", d / "per_tree.tsv"],
                ["--tree-distances", d / "distances.tsv"], ["--per-taxon", d / "per_taxon.tsv"],
                ["--place-taxa", d / "place_taxa.tsv"], ["--place-clades", d / "place_clades.tsv"], ["--test-groups", tmp_path / "groups.txt", d / "groups.tsv"],
                ["--taxon-pairs", d / "pairs.tsv"], ["--drop-one", d / "drop_one.tsv"], ["--also-ref", tmp_path / "r2.nwk", d / "also.nwk"],
                ["--branch-trees", d / "branch_trees.tsv"], ["--bootstrap", d / "bootstrap.tsv", "--bootstrap-reps", 20], ["--local-pp", d / "local_pp.tsv"],
                ["--without-taxa", tmp_path / "drop.txt", d / "without.nwk"]]

    def run(tag, chosen):
        args = ["-r", tmp_path / "r.nwk", "-e", tmp_path / "e.nwk", "-o", tmp_path / tag / "o.nwk"] + [x for option in chosen for x in option]
        p = subprocess.run([BIN, *map(str, args)], capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, (tag, p.stderr)
        return sorted(os.listdir(tmp_path / tag))

    whole = run("a", outputs("a"))
    assert len(whole) == 17
    parts = []
    for tag, third in (("b1", slice(0, 6)), ("b2", slice(6, 12)), ("b3", slice(12, 16))):
        written = run(tag, outputs(tag)[third])
        for name in written:
            assert (tmp_path / tag / name).read_bytes() == (tmp_path / "a" / name).read_bytes(), (tag, name)
        assert (tmp_path / tag / "o.nwk").stat().st_size > 0
        parts += [name for name in written if name != "o.nwk"]
    assert sorted(parts + ["o.nwk"]) == whole   # the thirds are disjoint and cover every output
    for name in whole:
        assert (tmp_path / "a" / name).stat().st_size > 0, name
