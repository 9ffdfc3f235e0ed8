"""QuartetScores --local-pp FILE [--local-pp-lambda L] against the Python route (engine.Context.tree_branch_support /
branch_frequencies, engine.local_pp_columns): integers and f_i byte for byte, the posterior's floats as text or within 1e-6 where the
last printed digit differs; beside --branch-trees / --bootstrap, whose files do not change; -o and -q unchanged by the flag."""
import math
import os
import subprocess

import numpy as np
import pytest

from quartetscores_amd import flatten, synth
from tree_branch_model import mixed_trees

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "quartetscores_amd", "bin", "QuartetScores")
N, M = 24, 40

pytestmark = pytest.mark.gpu


def run(*args):
    return subprocess.run([BIN, *map(str, args)], capture_output=True, text=True, timeout=600)


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    from quartetscores_amd import engine
    return engine


@pytest.fixture(scope="module", params=["unrooted", "rooted"])
def case(request, tmp_path_factory, eng):
    """reference and trees on disk, and the Python route's sums"""
    d = tmp_path_factory.mktemp(request.param)
    rng = np.random.default_rng(15 if request.param == "rooted" else 16)
    ref_nw = synth.random_tree(N, rng, rooted=request.param == "rooted", collapse=0.0 if request.param == "rooted" else 0.2)
    trees = mixed_trees(N, rng, M)
    (d / "r.nwk").write_text(ref_nw + "\n")
    (d / "e.nwk").write_text("\n".join(trees) + "\n")
    ref = flatten.flatten_reference(ref_nw)
    ctx = eng.Context(N)
    hb = ctx.batch_upload(flatten.flatten_eval_trees(trees, ref.name_to_id))
    freq = ctx.branch_frequencies(ctx.tree_branch_support(ref, hb))
    ctx.batch_free(hb)
    return d, ref, freq


def fmt(z):
    return "nan" if math.isnan(z) else "inf" if math.isinf(z) else "%.6f" % z


def same_lines(eng, path, cols):
    """the file's lines against the columns: header, integers and f_i as text, the other floats as text or within 1e-6"""
    got = path.read_text().split("\n")
    assert got[0] == "\t".join(eng.LOCAL_PP_COLUMNS) and got[-1] == "" and len(got) - 2 == len(cols["node"]) > 0
    for i, line in enumerate(got[1:-1]):
        f = line.split("\t")
        assert len(f) == len(eng.LOCAL_PP_COLUMNS)
        for k, name in enumerate(eng.LOCAL_PP_COLUMNS):
            if name in ("node", "lo", "hi", "en"):
                assert f[k] == str(int(cols[name][i])), (i, name, line)
            elif name in ("f1", "f2", "f3") or f[k] == fmt(cols[name][i]):
                assert f[k] == fmt(cols[name][i]), (i, name, line)
            else:
                assert abs(float(f[k]) - cols[name][i]) <= 1e-6, (i, name, line, cols[name][i])


def test_file_equals_the_python_route(eng, case):
    d, ref, freq = case
    p = run("-r", d / "r.nwk", "-e", d / "e.nwk", "-o", d / "o.nwk", "-q", d / "q.txt", "--local-pp", d / "pp.tsv")
    assert p.returncode == 0, p.stderr
    cols = eng.local_pp_columns(ref, freq)
    same_lines(eng, d / "pp.tsv", cols)
    assert (cols["en"] > 0).all() and (cols["en"] < M).any()           # trees with dropped taxa or stars leave branches out
    assert np.allclose(cols["pp1"] + cols["pp2"] + cols["pp3"], 1.0, rtol=0, atol=1e-8)
    assert (cols["pp1"] > 0.5).any() and ((cols["polytomy_p"] >= 0) & (cols["polytomy_p"] <= 1)).all() and (cols["length"] >= 0).all()
    # lambda = 1: another file, the same sums
    p = run("-r", d / "r.nwk", "-e", d / "e.nwk", "-o", d / "o1.nwk", "--local-pp", d / "pp1.tsv", "--local-pp-lambda", 1)
    assert p.returncode == 0, p.stderr
    other = eng.local_pp_columns(ref, freq, 1.0)
    same_lines(eng, d / "pp1.tsv", other)
    assert (d / "pp1.tsv").read_bytes() != (d / "pp.tsv").read_bytes() and not (other["length"] == cols["length"]).all()
    # without the flag -o and -q are the same bytes
    p = run("-r", d / "r.nwk", "-e", d / "e.nwk", "-o", d / "o2.nwk", "-q", d / "q2.txt")
    assert p.returncode == 0, p.stderr
    assert (d / "o2.nwk").read_bytes() == (d / "o.nwk").read_bytes() == (d / "o1.nwk").read_bytes()
    assert (d / "q2.txt").read_bytes() == (d / "q.txt").read_bytes()


def test_beside_branch_trees_and_bootstrap(eng, case):
    d, ref, freq = case
    flags = ["--branch-trees", "b.tsv", "--bootstrap", "boot.tsv", "--bootstrap-reps", 20, "--bootstrap-seed", 3]
    outs = {}
    for sub, extra in (("with", ["--local-pp", "pp.tsv"]), ("without", [])):
        w = d / sub
        w.mkdir()
        args = [w / a if isinstance(a, str) and a.endswith(".tsv") else a for a in flags + extra]
        p = run("-r", d / "r.nwk", "-e", d / "e.nwk", "-o", w / "o.nwk", *args)
        assert p.returncode == 0, p.stderr
        outs[sub] = w
    for name in ("b.tsv", "boot.tsv", "o.nwk"):
        assert (outs["with"] / name).read_bytes() == (outs["without"] / name).read_bytes(), name
    assert len((outs["with"] / "b.tsv").read_text().split("\n")) > 3
    same_lines(eng, outs["with"] / "pp.tsv", eng.local_pp_columns(ref, freq))


def test_root_edge_once(eng, case):
    d, ref, freq = case
    cols = eng.local_pp_columns(ref, freq)
    root = int(np.nonzero(np.asarray(ref.parent) < 0)[0][0])
    kids = np.nonzero(np.asarray(ref.parent) == root)[0]
    if len(kids) == 2:   # (the rooted case) both children are inner nodes of this tree: one line for the two
        assert freq[kids[0], 0] > 0 and (freq[kids[0]] == freq[kids[1]]).all()
        assert sum(int(v) in kids.tolist() for v in cols["node"]) == 1
