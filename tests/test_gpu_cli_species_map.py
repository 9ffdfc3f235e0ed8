"""QuartetScores --species-map FILE on the device: the saved table is the model's collapse of the table the Python engine counts over
the individuals, the annotated tree carries QuartetScoreComputer(species_map=...)'s scores, a --load-table run without the map resumes
on the saved table, a map that only renames changes nothing, and a run without the flag writes what the commit before it wrote."""
import importlib.util
import json
import os
import re
import subprocess

import numpy as np
import pytest

from species_model import collapse_table, individuals_of
from quartetscores_amd import flatten, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "quartetscores_amd", "bin", "QuartetScores")
GOLDEN = os.path.join(ROOT, "tests", "golden")
SIZES = (3, 2, 4, 1, 2, 3, 1, 4)      # 20 individuals in 8 species


def run(*args):
    return subprocess.run([BIN, *map(str, args)], capture_output=True, text=True, timeout=600)


def fixture_module():
    spec = importlib.util.spec_from_file_location("make_species_map_fixture", os.path.join(GOLDEN, "make_species_map_fixture.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """the species tree, 60 mixed gene trees over the 20 individuals, the map file, and one --species-map run with --save-table"""
    tmp = tmp_path_factory.mktemp("species_map")
    ref_nw = synth.reference_tree(len(SIZES), 201)
    ref = flatten.flatten_reference(ref_nw)
    mapping = {s: individuals_of(s, k) for s, k in zip(sorted(ref.names), SIZES) if k > 1}     # (singletons keep their species' name)
    inds = [x for s in sorted(ref.names) for x in mapping.get(s, [s])]
    n = len(inds)
    assert n == 20
    trees = (synth.tree_set(n, 15, 202, names=inds, dropout=0.2) + synth.tree_set(n, 15, 203, names=inds, collapse=0.3) +
             synth.tree_set(n, 15, 204, names=inds, rooted=True) + synth.tree_set(n, 15, 205, names=inds))
    (tmp / "r.nwk").write_text(ref_nw + "\n")
    (tmp / "e.nwk").write_text("\n".join(trees) + "\n")
    (tmp / "map.txt").write_text("# individuals per species\n\n" + "".join(f" {s} : {' , '.join(v)}\n" for s, v in mapping.items()))
    common = ("-r", tmp / "r.nwk", "-e", tmp / "e.nwk")
    p = run(*common, "--species-map", tmp / "map.txt", "-o", tmp / "a.nwk", "--save-table", tmp / "table.bin", "--per-taxon", tmp / "a.taxon",
            "--place-taxa", tmp / "a.place", "--test-groups", spec_file(tmp, ref), tmp / "a.groups", "--drop-one", tmp / "a.drop", "--trace")
    assert p.returncode == 0, p.stderr
    return dict(tmp=tmp, ref_nw=ref_nw, ref=ref, mapping=mapping, trees=trees, common=common, first=p)


def spec_file(tmp, ref):
    nm = ref.names
    (tmp / "spec.tsv").write_text(f"quad\t{nm[0]}\t{nm[1]},{nm[2]}\t{nm[3]}\t{nm[4]},{nm[5]}\nsplit\t{nm[0]},{nm[1]},{nm[2]}\t*\n")
    return tmp / "spec.tsv"


def edge_scores(newick_text):
    """the annotated tree's scores, sorted (the writer's order of the edges is the Newick text's, not the score arrays')"""
    return sorted(re.findall(r"(qp-ic|lq-ic|eqp-ic):(-?[0-9.]+|-?inf|-?nan)", newick_text))


def test_saved_table_is_the_collapse_of_the_individuals_table(data):
    from quartetscores_amd import engine
    lay = flatten.species_layout(data["ref"], data["mapping"])
    ctx = engine.Context(len(lay.names), 16)
    ctx.table_alloc()
    ctx.count_trees(flatten.flatten_eval_trees(data["trees"], lay.name_to_id))
    want = collapse_table(ctx.table_download(), len(lay.names), lay.first_id)
    raw = (data["tmp"] / "table.bin").read_bytes()
    # 60 trees x (4 x 4 x 3 x 3, the four largest groups) = 8640 < 65536: 16-bit cells
    assert len(raw) == want.size * 2
    got = np.frombuffer(raw, dtype=np.uint16).reshape(-1, 3)
    assert (got == want).all() and want.max() > 60


def test_annotated_tree_carries_the_python_engines_scores(data):
    from quartetscores_amd import engine
    qsc = engine.QuartetScoreComputer(data["ref_nw"], data["trees"], species_map=data["mapping"])
    got = edge_scores((data["tmp"] / "a.nwk").read_text())
    want = []
    for e in range(data["ref"].n_nodes - 1):      # per edge: qp-ic, lq-ic, eqp-ic, parts omitted when +inf (the writer's rule)
        lq, qp, eqp = qsc.getLQICScores()[e], qsc.getQPICScores()[e], qsc.getEQPICScores()[e]
        if lq != np.inf:
            want += [("qp-ic", "%.6f" % qp), ("lq-ic", "%.6f" % lq)]
        if eqp != np.inf:
            want.append(("eqp-ic", "%.6f" % eqp))
    assert qsc.bifurcating and got == sorted(want) and len(got) > 0
    # and the same object from the text of the map file
    again = engine.QuartetScoreComputer(data["ref_nw"], data["trees"], species_map=(data["tmp"] / "map.txt").read_text())
    assert again.getLQICScores() == qsc.getLQICScores()
    assert again.quartetCounterLookup.ctx.n == len(SIZES)


def test_load_table_without_the_map_resumes_on_the_species_table(data):
    tmp = data["tmp"]
    p = run(*data["common"], "--load-table", tmp / "table.bin", "-o", tmp / "b.nwk", "--per-taxon", tmp / "b.taxon",
            "--place-taxa", tmp / "b.place", "--test-groups", tmp / "spec.tsv", tmp / "b.groups", "--drop-one", tmp / "b.drop")
    assert p.returncode == 0, p.stderr
    assert "Collapsed the count table" not in p.stdout
    for name in ("nwk", "taxon", "place", "groups", "drop"):
        a, b = (tmp / f"a.{name}").read_bytes(), (tmp / f"b.{name}").read_bytes()
        assert a == b and len(a) > 0, name


def test_a_map_that_only_renames_changes_nothing(data, tmp_path):
    ref_nw, trees = fixture_module().plain_inputs()
    ref = flatten.flatten_reference(ref_nw)
    renamed = [re.sub(r"t(\d+)", r"ind\1", nw) for nw in trees]
    (tmp_path / "r.nwk").write_text(ref_nw + "\n")
    (tmp_path / "plain.nwk").write_text("\n".join(trees) + "\n")
    (tmp_path / "renamed.nwk").write_text("\n".join(renamed) + "\n")
    (tmp_path / "map.txt").write_text("".join(f"{s}:{s.replace('t', 'ind')}\n" for s in ref.names))
    p = run("-r", tmp_path / "r.nwk", "-e", tmp_path / "plain.nwk", "-o", tmp_path / "plain.out")
    assert p.returncode == 0, p.stderr
    q = run("-r", tmp_path / "r.nwk", "-e", tmp_path / "renamed.nwk", "-o", tmp_path / "renamed.out", "--species-map", tmp_path / "map.txt")
    assert q.returncode == 0, q.stderr
    assert (tmp_path / "plain.out").read_bytes() == (tmp_path / "renamed.out").read_bytes()
    # (the evaluation trees' own names without the map: unknown to the reference tree)
    r = run("-r", tmp_path / "r.nwk", "-e", tmp_path / "renamed.nwk", "-o", tmp_path / "none.out")
    assert r.returncode != 0 and not (tmp_path / "none.out").exists()


def test_a_run_without_the_flag_writes_what_the_parent_commit_wrote(tmp_path):
    mod = fixture_module()
    with open(os.path.join(GOLDEN, "species_map_plain.json")) as f:
        want = json.load(f)
    got = mod.run_plain(BIN, str(tmp_path))
    assert set(got) == set(want) == set(mod.PLAIN_OUTPUTS)
    for flag in want:
        assert got[flag] == want[flag], flag


# ---- few trees, large groups: the species' table needs 32-bit cells although the number of trees asks for 16 ---------------------

WIDE_SIZES = (4, 1, 4, 1, 4, 1, 4, 1)      # 300 trees x 4^4 = 76 800 >= 65 536


def annotation(ref, scores):
    """the sorted score parts write_annotated gives the tree for (lq, qp, eqp, bifurcating) of Context.score"""
    lq, qp, eqp, bif = scores
    want = []
    for e in range(1, ref.n_nodes):
        if lq[e] != np.inf:
            want += ([("qp-ic", "%.6f" % qp[e])] if bif else []) + [("lq-ic", "%.6f" % lq[e])]
        if bif and eqp[e] != np.inf:
            want.append(("eqp-ic", "%.6f" % eqp[e]))
    return sorted(want)


@pytest.fixture(scope="module")
def wide(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("species_map_wide")
    rng = np.random.default_rng(221)
    ref_nw, other_nw = synth.random_tree(len(WIDE_SIZES), rng), synth.random_tree(len(WIDE_SIZES), rng)
    ref = flatten.flatten_reference(ref_nw)
    mapping = {s: individuals_of(s, k) for s, k in zip(ref.names, WIDE_SIZES) if k > 1}
    inds = [x for s in ref.names for x in mapping.get(s, [s])]
    n = len(inds)
    trees = synth.tree_set(n, 150, 222, names=inds) + synth.tree_set(n, 100, 223, names=inds, dropout=0.2) + synth.tree_set(n, 50, 224, names=inds, collapse=0.3)
    (tmp / "r.nwk").write_text(ref_nw + "\n")
    (tmp / "other.nwk").write_text(other_nw + "\n")
    (tmp / "e.nwk").write_text("\n".join(trees) + "\n")
    (tmp / "map.txt").write_text("".join(f"{s}:{','.join(v)}\n" for s, v in mapping.items()))
    drop = [ref.names[1], ref.names[6]]
    (tmp / "drop.txt").write_text("\n".join(drop) + "\n")
    common = ("-r", tmp / "r.nwk", "-e", tmp / "e.nwk")
    p = run(*common, "--species-map", tmp / "map.txt", "-o", tmp / "a.nwk", "--save-table", tmp / "table.bin", "--per-taxon", tmp / "a.taxon",
            "--also-ref", tmp / "other.nwk", tmp / "a.other", "--without-taxa", tmp / "drop.txt", tmp / "a.without", "--trace")
    assert p.returncode == 0, p.stderr
    return dict(tmp=tmp, ref_nw=ref_nw, other_nw=other_nw, ref=ref, mapping=mapping, trees=trees, drop=drop, common=common, first=p)


def test_wide_species_table_serves_also_ref_and_without_taxa(wide):
    from quartetscores_amd import engine, newick
    tmp, ref = wide["tmp"], wide["ref"]
    assert "-> 8 species, 32-bit cells" in wide["first"].stderr and len(wide["trees"]) < 65536
    qsc = engine.QuartetScoreComputer(wide["ref_nw"], wide["trees"], species_map=wide["mapping"])
    src = qsc.quartetCounterLookup.ctx
    assert src.count_bits == 32 and src.n == len(WIDE_SIZES) and int(src.table_download().max()) > len(wide["trees"])
    assert edge_scores((tmp / "a.nwk").read_text()) == annotation(ref, src.score(ref))
    other = flatten.flatten_reference(wide["other_nw"])
    remapped = engine.Context(other.n_taxa, 32)
    remapped.table_alloc()
    remapped.table_remap(src, flatten.taxon_permutation(other, ref))
    want = annotation(other, remapped.score(other))
    assert edge_scores((tmp / "a.other").read_text()) == want and len(want) > 0
    small = flatten.flatten_reference(newick.write(newick.prune(newick.parse_tree(wide["ref_nw"]), wide["drop"])))
    cut = engine.Context(small.n_taxa, 32)
    cut.table_alloc()
    cut.table_restrict(src, flatten.taxon_restriction(small, ref))
    want = annotation(small, cut.score(small))
    assert edge_scores((tmp / "a.without").read_text()) == want and len(want) > 0


def test_wide_saved_table_loads_without_the_map(wide):
    tmp = wide["tmp"]
    assert (tmp / "table.bin").stat().st_size == 70 * 3 * 4          # C(8,4) tuples of 32-bit cells, though 300 trees ask for 16
    p = run(*wide["common"], "--load-table", tmp / "table.bin", "-o", tmp / "b.nwk", "--per-taxon", tmp / "b.taxon",
            "--also-ref", tmp / "other.nwk", tmp / "b.other", "--without-taxa", tmp / "drop.txt", tmp / "b.without")
    assert p.returncode == 0, p.stderr
    for name in ("nwk", "taxon", "other", "without"):
        a, b = (tmp / f"a.{name}").read_bytes(), (tmp / f"b.{name}").read_bytes()
        assert a == b and len(a) > 0, name
    (tmp / "short.bin").write_bytes((tmp / "table.bin").read_bytes()[:-4])
    q = run(*wide["common"], "--load-table", tmp / "short.bin", "-o", tmp / "c.nwk")
    assert q.returncode == 1 and "--load-table: size does not match" in q.stderr and not (tmp / "c.nwk").exists()


def test_stdout_carries_the_collapsed_line(data):
    p = data["first"]
    assert re.search(r"^Collapsed the count table in \d+ microseconds\.$", p.stdout, flags=re.M), p.stdout
    assert "[trace] qs_table_collapse: 20 individuals -> 8 species, 16-bit cells" in p.stderr
    assert p.stdout.index("Collapsed the count table") < p.stdout.index("Finished counting quartets.")
