"""The local posterior without a GPU: engine.local_pp (pure math) and the C++ host's qsh_local_pp (csrc/host/local_pp.hpp, through
native_ingest.local_pp) against tests/local_pp_model.py (big integers and mpmath at 50 digits) on rows of the per-tree model and on
the stated cases; engine.local_pp_columns; the refusals of QuartetScores --local-pp, which come before the device is touched.

Tolerance: 1e-8 absolute on the posteriors and the p-value, 1e-8 relative on the length. At en = 10^4 the log terms are below 7e4 in
magnitude and carry about 1e-11 each in double; tens of them stay below 1e-9, and the bound leaves a factor of ten over that."""
import math
import os
import subprocess

import mpmath
import numpy as np
import pytest

import branch_taxon_model as BM
import local_pp_model as LM
import tree_branch_model as TB
from quartetscores_amd import _lib, engine, flatten, native_ingest, synth
from tree_branch_model import mixed_trees

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "quartetscores_amd", "bin", "QuartetScores")
ONE = LM.ONE
TOL = 1e-8


def close(got, want):
    """the five figures of one branch within the bound; the three posteriors add up to 1 within it"""
    assert len(got) == len(want) == 5
    if any(math.isnan(x) for x in want):
        assert all(math.isnan(x) for x in want) and all(math.isnan(x) for x in got), (got, want)
        return
    for i in (0, 1, 2, 4):
        assert abs(got[i] - want[i]) <= TOL, (i, got, want)
    assert abs(got[0] + got[1] + got[2] - 1.0) <= TOL, got
    if math.isinf(want[3]) or want[3] == 0.0:
        assert got[3] == want[3], (got, want)
    else:
        assert abs(got[3] - want[3]) <= TOL * abs(want[3]), (got, want)


def both(en, Z, lam):
    """(engine.local_pp, qsh_local_pp) of the fixed-point sums Z"""
    return engine.local_pp(en, [x / ONE for x in Z], lam), native_ingest.local_pp(en, Z, lam)


def want_of(en, Z, lam):
    with mpmath.workdps(50):
        return LM.posterior(en, [mpmath.mpf(x) / ONE for x in Z], lam)


def test_model_tails_add_up_to_beta():
    """the model's series on both sides of 1/3: the two tails are B(a, b), also where one of them is 10^-600 of it"""
    with mpmath.workdps(50):
        for a, b in ((4, 1), (1.3, 0.7), (35, 67), (21, 81), (8001, 2001), (3401, 6601), (1001, 9001), (10001, 1)):
            upper, lower = LM.beta_tail(b, a, mpmath.mpf(2) / 3), LM.beta_tail(a, b, mpmath.mpf(1) / 3)
            assert abs((upper + lower) / mpmath.beta(a, b) - 1) < mpmath.mpf(10) ** -40, (a, b)
        assert abs(LM.beta_tail(1, 10001, mpmath.mpf(2) / 3) - (1 - mpmath.power(mpmath.mpf(1) / 3, 10001)) / 10001) < mpmath.mpf(10) ** -50


def test_frequency_model():
    rows = [[[9, 1, 1, 1], [5, 0, 0, 0], [0, 0, 0, 0]], [[9, 3, 0, 0], [5, 2, 1, 0], [7, 0, 0, 0]]]
    third = ONE // 3
    assert LM.frequencies(rows) == [[2, third + ONE, third, third], [1, 2 * ONE // 3, third, 0], [0, 0, 0, 0]]
    S = math.comb(4096, 4)
    assert LM.frequencies([[[S, S - 1, 1, 0]]]) == [[1, (S - 1) * ONE // S, ONE // S, 0]]


@pytest.mark.parametrize("lam", [0.25, 0.5, 1.0])
def test_spot_values_and_edges(lam):
    cases = [(3, (3, 0, 0)), (3, (1, 1, 1)), (100, (34, 33, 33)), (100, (40, 30, 30)), (100, (20, 60, 20)),
             (10000, (8000, 1000, 1000)), (10000, (3400, 3300, 3300)),
             (1, (1, 0, 0)), (1, (0, 1, 0)), (1, (0.25, 0.5, 0.25)),                 # en = 1
             (7, (7, 0, 0)), (50, (50, 0, 0)),                                       # z_1 = en
             (9, (3, 3, 3)), (9, (2, 5, 2)), (40, (13.25, 13.5, 13.25)),             # theta <= 1/3
             (12, (7.5, 2.25, 2.25)), (600, (333.125, 140.5, 126.375))]
    for en, z in cases:
        Z = [int(x * ONE) for x in z]
        want = want_of(en, Z, lam)
        for got in both(en, Z, lam):
            close(got, want)
    if lam == 0.5:
        for (en, z), pp1 in zip(cases[:5], (0.952381, 1 / 3, 0.372599, 0.799089, 4.55e-8)):
            got = engine.local_pp(en, z, lam)[0]
            assert abs(got - pp1) < (1e-10 if pp1 < 1e-6 else 1e-6), (z, got)
    # z_1 = en: the length is infinite where 2 lam = 1 and finite above; theta <= 1/3: 0
    for got in both(50, [50 * ONE, 0, 0], lam):
        assert (math.isinf(got[3]) and lam <= 0.5) or (lam > 0.5 and got[3] == -math.log(1.5 * (1 - 50 / (49 + 2 * lam))))
    for got in both(9, [2 * ONE, 5 * ONE, 2 * ONE], lam):
        assert got[3] == 0.0
    for got in both(9, [3 * ONE] * 3, lam):
        assert got[4] == 1.0 and got[0] == got[1] == got[2]
    for got in both(0, [0, 0, 0], lam):
        assert all(math.isnan(x) for x in got)
    # the benchmark's size: B(8001, 2001) is 10^-2176
    for got in both(10000, [8000 * ONE, 1000 * ONE, 1000 * ONE], lam):
        assert got[0] == 1.0 and got[1] == got[2] == 0.0 and got[4] == 0.0


def test_bad_arguments():
    with pytest.raises(ValueError):
        engine.local_pp(3, (1, 1, 1), 0.0)
    with pytest.raises(native_ingest.IngestError):
        native_ingest.local_pp(3, [ONE, ONE, ONE], 0.0)


def star(n):
    return "(" + ",".join(f"t{i}" for i in range(n)) + ");"


@pytest.fixture(scope="module")
def cases():
    """(ref, rows (m, n_nodes, 4)) at 5..16 taxa: mixed trees (dropped taxa, collapsed edges), a star and a tree of four taxa"""
    rng = np.random.default_rng(19)
    out = []
    for n, kw in ((5, {}), (9, {"collapse": 0.3}), (12, {"rooted": True}), (16, {})):
        ref = flatten.flatten_reference(synth.random_tree(n, rng, **kw))
        trees = mixed_trees(n, rng, 12) + [star(n), "((t0,t1),(t2,t3));"]
        the_items = TB.items(ref)
        out.append((ref, np.array([TB.model_tree(ref, t, the_items=the_items) for t in trees])))
    return out


def test_rows_of_the_tree_model(cases):
    seen_star = seen_absent = seen_resolved = False
    for ref, rows in cases:
        freq = LM.frequencies(rows.tolist())
        edges = [v for v, _ in BM.internodes(ref)]
        assert edges
        star_row, four_taxa = rows[-2], rows[-1]
        assert not star_row[:, 1:].any()
        for v in edges:
            en, Z = freq[v][0], freq[v][1:]
            assert en == int((rows[:, v, 1:].sum(1) > 0).sum()) <= len(rows)
            seen_star |= star_row[v, 0] > 0                       # present > 0, S = 0: the tree does not count
            seen_absent |= four_taxa[v, 0] == 0                   # the tree lacks the branch's taxa
            seen_resolved |= en > 0
            assert en * ONE - 3 * en <= sum(Z) <= en * ONE
            for lam in (0.25, 0.5, 1.0):
                want = want_of(en, Z, lam)
                for got in both(en, Z, lam):
                    close(got, want)
    assert seen_star and seen_absent and seen_resolved


def test_local_pp_columns(cases):
    for ref, rows in cases:
        freq = np.array(LM.frequencies(rows.tolist()), dtype=np.int64)
        # the edge through a degree-2 root stands at both its inner children and is written once, at the child that holds id 0
        edges = [v for v, w in BM.internodes(ref) if not (ref.parent[v] != w and ref.parent[w] == ref.parent[v] and v > w)]
        for lam in (0.5, 1.0):
            cols = engine.local_pp_columns(ref, freq, lam)
            assert list(cols) == list(engine.LOCAL_PP_COLUMNS) == ["node", "lo", "hi", "en", "f1", "f2", "f3", "pp1", "pp2", "pp3", "length", "polytomy_p"]
            assert cols["node"].tolist() == edges
            boot = engine.bootstrap_columns(ref, rows.sum(0), rows[:1])
            assert cols["node"].tolist() == boot["node"].tolist() and cols["lo"].tolist() == boot["lo"].tolist() and cols["hi"].tolist() == boot["hi"].tolist()
            for name in engine.LOCAL_PP_COLUMNS:
                assert cols[name].dtype == (np.int64 if name in ("node", "lo", "hi", "en") else np.float64), name
            for i, v in enumerate(edges):
                assert cols["en"][i] == freq[v, 0]
                assert [cols["f1"][i], cols["f2"][i], cols["f3"][i]] == [int(freq[v, k]) / ONE for k in (1, 2, 3)]
                want = engine.local_pp(int(freq[v, 0]), [int(freq[v, k]) / ONE for k in (1, 2, 3)], lam)
                got = tuple(float(cols[k][i]) for k in ("pp1", "pp2", "pp3", "length", "polytomy_p"))
                assert got == want or (all(math.isnan(x) for x in got) and freq[v, 0] == 0)
    ref, rows = cases[2]
    assert len([v for v, w in BM.internodes(ref) if ref.parent[v] != w]) == 2        # the rooted case has the merged edge
    empty = engine.local_pp_columns(ref, np.zeros((ref.n_nodes, 4), dtype=np.int64))
    assert np.isnan(empty["pp1"]).all() and np.isnan(empty["length"]).all() and not empty["f1"].any()


def test_binding_declares_the_call():
    assert "qs_branch_frequencies" in _lib.EXPORTS


def run(*args):
    return subprocess.run([BIN, *map(str, args)], capture_output=True, text=True, timeout=600)


@pytest.fixture()
def files(tmp_path):
    (tmp_path / "r.nwk").write_text(synth.reference_tree(12, 1) + "\n")
    (tmp_path / "e.nwk").write_text("\n".join(synth.tree_set(12, 6, 2)) + "\n")
    return tmp_path


def base(files):
    return ["-r", files / "r.nwk", "-e", files / "e.nwk", "-o", files / "o.nwk"]


@pytest.mark.parametrize("extra", [["--load-table", "t.bin"], ["--table-shards", "2"], ["--gpus", "2"]])
def test_cli_refused_where_no_trees_are_counted_on_one_gpu(files, extra):
    p = run(*base(files), "--local-pp", files / "x.tsv", *extra, "--trace")
    assert p.returncode == 1 and "--local-pp needs the evaluation trees counted on one GPU" in p.stderr, p.stderr
    assert "[trace]" not in p.stderr and not (files / "x.tsv").exists() and not (files / "o.nwk").exists()


def test_cli_refused_files_and_stray_options(files):
    args = base(files)
    (files / "keep.tsv").write_text("keep\n")
    p = run(*args, "--local-pp", files / "keep.tsv", "--trace")
    assert p.returncode == 1 and "--local-pp: the output file" in p.stderr and "already exists" in p.stderr, p.stderr
    assert "[trace]" not in p.stderr and (files / "keep.tsv").read_text() == "keep\n"
    for other in ("--bootstrap", "--branch-trees", "-q"):
        p = run(*args, "--local-pp", files / "same.tsv", other, files / "same.tsv", "--trace")
        assert p.returncode == 1 and "is also another output file" in p.stderr and "[trace]" not in p.stderr, p.stderr
    p = run(*args, "--local-pp-lambda", "1", "--trace")
    assert p.returncode == 1 and "--local-pp-lambda needs --local-pp FILE" in p.stderr and "[trace]" not in p.stderr, p.stderr
    for bad in ("0", "-1", "x", "nan", "inf", "1e999"):
        p = run(*args, "--local-pp", files / "x.tsv", "--local-pp-lambda", bad, "--trace")
        assert p.returncode == 1 and "for arg --local-pp-lambda" in p.stderr and "[trace]" not in p.stderr, (bad, p.stderr)
    for flag in ("--local-pp", "--local-pp-lambda"):
        p = run(*args, flag)
        assert p.returncode == 1 and "Missing a value for this argument! for arg " + flag in p.stderr, p.stderr
    assert not (files / "o.nwk").exists() and not (files / "same.tsv").exists() and not (files / "x.tsv").exists()
    text = run("-h").stdout
    assert "--local-pp F" in text and "--local-pp-lambda L" in text and "assumes a binary" in text
