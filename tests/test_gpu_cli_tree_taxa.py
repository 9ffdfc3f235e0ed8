"""QuartetScores --tree-taxa FILE [--tree-taxa-only NAMES] [--tree-taxa-min-gain G] against the Python route
(engine.Context.tree_taxon_agreement, engine.tree_taxon_columns), the rogue-leaf list on an input whose rogue leaves are known, the
outputs it must leave alone, and the refusals that come before the device is touched."""
import math
import os
import subprocess

import numpy as np
import pytest

import tree_taxon_model as M
from quartetscores_amd import flatten, synth
from tree_branch_model import mixed_trees

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "quartetscores_amd", "bin", "QuartetScores")
N, TREES = 24, 40

pytestmark = pytest.mark.gpu


def run(*args):
    return subprocess.run([BIN, *map(str, args)], capture_output=True, text=True, timeout=600)


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    from quartetscores_amd import engine
    return engine


def fmt(z):
    return "nan" if math.isnan(z) else "%.6f" % z


def text_of(eng, cols):
    lines = ["\t".join(eng.TREE_TAXA_COLUMNS)]
    for i in range(len(cols["tree"])):
        lines.append("\t".join(fmt(cols[k][i]) if k in eng.TREE_TAXA_FLOATS else str(cols[k][i]) for k in eng.TREE_TAXA_COLUMNS))
    return "".join(line + "\n" for line in lines)


def python_route(eng, ref, trees):
    ctx = eng.Context(ref.n_taxa)
    b = flatten.flatten_eval_trees(trees, ref.name_to_id)
    hb = ctx.batch_upload(b)
    words = ctx.tree_taxon_agreement(ref, hb)
    ctx.batch_free(hb)
    return words, b


@pytest.fixture(scope="module", params=["unrooted", "rooted"])
def case(request, tmp_path_factory, eng):
    d = tmp_path_factory.mktemp(request.param)
    rng = np.random.default_rng(3 if request.param == "rooted" else 4)
    ref_nw = synth.random_tree(N, rng, rooted=request.param == "rooted", collapse=0.0 if request.param == "rooted" else 0.2)
    trees = mixed_trees(N, rng, TREES - 1) + [M.star([f"t{i}" for i in range(N)])]      # (the star resolves nothing: its ratios are nan)
    (d / "r.nwk").write_text(ref_nw + "\n")
    (d / "e.nwk").write_text("\n".join(trees) + "\n")
    ref = flatten.flatten_reference(ref_nw)
    words, b = python_route(eng, ref, trees)
    return d, ref, words, b


def test_file_equals_the_python_route(eng, case):
    d, ref, words, b = case
    base = ["-r", d / "r.nwk", "-e", d / "e.nwk"]
    p = run(*base, "-o", d / "o.nwk", "--tree-taxa", d / "t.tsv", "--per-tree", d / "p.tsv")
    assert p.returncode == 0, p.stderr
    cols = eng.tree_taxon_columns(ref.names, words, b)
    assert (d / "t.tsv").read_text() == text_of(eng, cols)
    small = sum(int(b.leaf_off[t + 1] - b.leaf_off[t]) < 4 for t in range(TREES))
    assert small and len(set(cols["tree"].tolist())) == TREES - small and len(cols["tree"]) < TREES * N      # dropout trees hold fewer taxa
    assert np.isnan(cols["gain"]).any() and (cols["gain"] > 0).any() and (cols["gain"] < 0).any()
    # tree_concordance is --per-tree's figure
    per_tree = {f[0]: f[8] for f in (line.split("\t") for line in (d / "p.tsv").read_text().split("\n")[1:-1])}
    for line in (d / "t.tsv").read_text().split("\n")[1:-1]:
        f = line.split("\t")
        assert f[10] == per_tree[f[0]]
    # --tree-taxa-only
    some = [ref.names[i] for i in (5, 0, 17)]
    (d / "names.txt").write_text("\n".join(some + [some[0]]) + "\n\n")
    p = run(*base, "-o", d / "o2.nwk", "--tree-taxa", d / "t2.tsv", "--tree-taxa-only", d / "names.txt")
    assert p.returncode == 0, p.stderr
    only = eng.tree_taxon_columns(ref.names, words, b, only=[0, 5, 17])
    assert 0 < len(only["tree"]) < len(cols["tree"]) and (d / "t2.tsv").read_text() == text_of(eng, only)
    # ... with --tree-taxa-min-gain, beside the other outputs that work behind the count
    p = run(*base, "-o", d / "o3.nwk", "--tree-taxa", d / "t3.tsv", "--tree-taxa-only", d / "names.txt", "--tree-taxa-min-gain", "-0.01",
            "--per-tree", d / "p3.tsv", "--branch-trees", d / "b3.tsv", "--bootstrap", d / "boot3.tsv", "--bootstrap-reps", 5, "--local-pp", d / "l3.tsv")
    assert p.returncode == 0, p.stderr
    both = eng.tree_taxon_columns(ref.names, words, b, only=[0, 5, 17], min_gain=-0.01)
    assert 0 < len(both["tree"]) < len(only["tree"]) and (d / "t3.tsv").read_text() == text_of(eng, both)
    # with and without the flag: the annotated tree, --per-tree and the other outputs are the same
    p = run(*base, "-o", d / "o4.nwk", "--per-tree", d / "p4.tsv", "--branch-trees", d / "b4.tsv", "--bootstrap", d / "boot4.tsv", "--bootstrap-reps", 5,
            "--local-pp", d / "l4.tsv")
    assert p.returncode == 0, p.stderr
    assert (d / "o.nwk").read_bytes() == (d / "o2.nwk").read_bytes() == (d / "o3.nwk").read_bytes() == (d / "o4.nwk").read_bytes()
    assert (d / "p.tsv").read_bytes() == (d / "p3.tsv").read_bytes() == (d / "p4.tsv").read_bytes()
    for name in ("b", "boot", "l"):
        assert (d / f"{name}3.tsv").read_bytes() == (d / f"{name}4.tsv").read_bytes()


def test_min_gain_lists_the_regrafted_leaves(eng, tmp_path):
    """every tree is the reference except three, in each of which one leaf is regrafted far away: the rogue-leaf list is those three
    lines. What is expected comes from the model, not from the code under test."""
    rng = np.random.default_rng(31)
    ref_nw = synth.random_tree(N, rng)
    ref = flatten.flatten_reference(ref_nw)
    moved = {2: "t7", 5: "t19", 9: "t0"}
    trees = [M.regraft_far(ref_nw, moved[t], rng) if t in moved else ref_nw for t in range(12)]
    gain = [M.gains(M.model_tree(ref, t), range(N)) for t in trees]
    rogue = {(t, ref.name_to_id[nm]) for t, nm in moved.items()}
    for t, x in rogue:
        assert gain[t][x] == max(gain[t].values()) and sum(g == gain[t][x] for g in gain[t].values()) == 1
    lowest_rogue = min(gain[t][x] for t, x in rogue)
    highest_other = max(g for t in range(12) for x, g in gain[t].items() if (t, x) not in rogue)
    assert 0 <= highest_other < lowest_rogue
    G = (highest_other + lowest_rogue) / 2
    (tmp_path / "r.nwk").write_text(ref_nw + "\n")
    (tmp_path / "e.nwk").write_text("\n".join(trees) + "\n")
    p = run("-r", tmp_path / "r.nwk", "-e", tmp_path / "e.nwk", "-o", tmp_path / "o.nwk", "--tree-taxa", tmp_path / "t.tsv", "--tree-taxa-min-gain", repr(G))
    assert p.returncode == 0, p.stderr
    got = [line.split("\t") for line in (tmp_path / "t.tsv").read_text().split("\n")[1:-1]]
    assert {(int(f[0]), int(f[1])) for f in got} == rogue and len(got) == 3
    for f in got:
        assert f[2] == moved[int(f[0])] and f[11] == "1.000000" and float(f[12]) == pytest.approx(gain[int(f[0])][int(f[1])], abs=1e-6)
    # the full file: every line of every other tree is below G, and the rogue lines carry the largest gain of their tree
    p = run("-r", tmp_path / "r.nwk", "-e", tmp_path / "e.nwk", "-o", tmp_path / "o2.nwk", "--tree-taxa", tmp_path / "all.tsv")
    assert p.returncode == 0, p.stderr
    full = [line.split("\t") for line in (tmp_path / "all.tsv").read_text().split("\n")[1:-1]]
    assert len(full) == 12 * N
    for t in range(12):
        mine = {int(f[1]): float(f[12]) for f in full if int(f[0]) == t}
        assert len(mine) == N and any(g < G for g in mine.values())
        if t in moved:
            assert max(mine, key=mine.get) == ref.name_to_id[moved[t]]
        else:
            assert all(g == 0.0 for g in mine.values())


def test_two_batches_stream_through(eng, tmp_path):
    """4100 trees reach the device in two batches: the lines carry on with the right tree numbers"""
    rng = np.random.default_rng(22)
    n = 17
    ref_nw = synth.random_tree(n, rng, collapse=0.1)
    some = mixed_trees(n, rng, 64)
    pick = [(7 * i) % 64 for i in range(4100)]
    (tmp_path / "r.nwk").write_text(ref_nw + "\n")
    (tmp_path / "e.nwk").write_text("\n".join(some[i] for i in pick) + "\n")
    p = run("-r", tmp_path / "r.nwk", "-e", tmp_path / "e.nwk", "-o", tmp_path / "o.nwk", "--tree-taxa", tmp_path / "t.tsv", "--tree-taxa-min-gain", "0.05")
    assert p.returncode == 0, p.stderr
    ref = flatten.flatten_reference(ref_nw)
    words, _ = python_route(eng, ref, some)
    b = flatten.flatten_eval_trees([some[i] for i in pick], ref.name_to_id)
    cols = eng.tree_taxon_columns(ref.names, words[pick], b, min_gain=0.05)
    assert cols["tree"].max() > 2048 and (tmp_path / "t.tsv").read_text() == text_of(eng, cols)


def base(d):
    (d / "r.nwk").write_text(synth.reference_tree(N, 1) + "\n")
    (d / "e.nwk").write_text("\n".join(synth.tree_set(N, 6, 2)) + "\n")
    return ["-r", d / "r.nwk", "-e", d / "e.nwk", "-o", d / "o.nwk"]


@pytest.mark.parametrize("extra", [["--load-table", "t.bin"], ["--table-shards", "2"], ["--gpus", "2"]])
def test_refused_where_no_trees_are_counted_on_one_gpu(tmp_path, extra):
    p = run(*base(tmp_path), "--tree-taxa", tmp_path / "x.tsv", *extra, "--trace")
    assert p.returncode == 1 and "--tree-taxa needs the evaluation trees counted on one GPU" in p.stderr, p.stderr
    assert "[trace]" not in p.stderr and not (tmp_path / "x.tsv").exists() and not (tmp_path / "o.nwk").exists()


def test_refused_files_and_stray_options(tmp_path):
    args = base(tmp_path)
    (tmp_path / "keep.tsv").write_text("keep\n")
    (tmp_path / "names.txt").write_text("t1\nt2\n")
    p = run(*args, "--tree-taxa", tmp_path / "keep.tsv", "--trace")
    assert p.returncode == 1 and "--tree-taxa: the output file" in p.stderr and "already exists" in p.stderr, p.stderr
    assert "[trace]" not in p.stderr and (tmp_path / "keep.tsv").read_text() == "keep\n"
    p = run(*args, "--tree-taxa", tmp_path / "same.tsv", "--per-tree", tmp_path / "same.tsv", "--trace")
    assert p.returncode == 1 and "is also another output file" in p.stderr and "[trace]" not in p.stderr, p.stderr
    p = run(*args, "--tree-taxa-only", tmp_path / "names.txt", "--trace")
    assert p.returncode == 1 and "--tree-taxa-only needs --tree-taxa FILE" in p.stderr and "[trace]" not in p.stderr, p.stderr
    p = run(*args, "--tree-taxa-min-gain", "0.1", "--trace")
    assert p.returncode == 1 and "--tree-taxa-min-gain needs --tree-taxa FILE" in p.stderr and "[trace]" not in p.stderr, p.stderr
    p = run(*args, "--tree-taxa", tmp_path / "t.tsv", "--tree-taxa-min-gain", "much", "--trace")
    assert p.returncode == 1 and "Couldn't read argument value from string 'much' for arg --tree-taxa-min-gain" in p.stderr, p.stderr
    p = run(*args, "--tree-taxa", tmp_path / "t.tsv", "--tree-taxa-min-gain")
    assert p.returncode == 1 and "Missing a value for this argument! for arg --tree-taxa-min-gain" in p.stderr, p.stderr
    (tmp_path / "bad.txt").write_text("t1\nnobody\n")
    p = run(*args, "--tree-taxa", tmp_path / "t.tsv", "--tree-taxa-only", tmp_path / "bad.txt", "--trace")
    assert p.returncode == 1 and "the taxon nobody is not in the reference tree" in p.stderr and "[trace]" not in p.stderr, p.stderr
    (tmp_path / "empty.txt").write_text("\n")
    p = run(*args, "--tree-taxa", tmp_path / "t.tsv", "--tree-taxa-only", tmp_path / "empty.txt")
    assert p.returncode == 1 and "the list of taxa is empty" in p.stderr, p.stderr
    assert not (tmp_path / "o.nwk").exists() and not (tmp_path / "same.tsv").exists() and not (tmp_path / "t.tsv").exists()
    # one taxon more than the device plan supports
    n = M.max_taxa() + 1
    (tmp_path / "big.nwk").write_text(M.ladder(M.names_of(n)) + "\n")
    p = run("-r", tmp_path / "big.nwk", "-e", tmp_path / "big.nwk", "-o", tmp_path / "o.nwk", "--tree-taxa", tmp_path / "t.tsv", "--trace")
    assert p.returncode == 1 and f"has {n} taxa, the device plan supports at most {n - 1}" in p.stderr and "[trace]" not in p.stderr, p.stderr
    assert not (tmp_path / "o.nwk").exists() and not (tmp_path / "t.tsv").exists()
    text = run("-h").stdout
    assert "--tree-taxa F" in text and "--tree-taxa-only NAMES" in text and "--tree-taxa-min-gain G" in text and "(trees x taxa) lines" in text
