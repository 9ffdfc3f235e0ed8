"""Quartet support of taxon groups without a GPU: the numpy model of qs_group_support (tests/group_model.py) against a direct
count over the trees, the host-only qs_group_check, and the SPEC parser of --test-groups."""
import numpy as np
import pytest

import bruteforce
import group_model as M
from helpers import binom
from quartetscores_amd import _lib, engine, flatten, synth


def cases(seed):
    rng = np.random.default_rng(seed)
    for n in (5, 6, 7, 8, 9):
        ref_nw = synth.random_tree(n, rng)
        trees = []
        for k in range(6):   # (no tree both complete and resolved: some 4-sets stay without any count)
            kw = [{"dropout": 0.3, "min_taxa": 4}, {"collapse": 0.5}, {"dropout": 0.4, "min_taxa": 4}, {"rooted": True, "dropout": 0.3, "min_taxa": 4},
                  {"rooted": True, "collapse": 0.3, "dropout": 0.2}, {"collapse": 1.0}][k]
            trees.append(synth.random_tree(n, rng, **kw))
        yield n, ref_nw, trees


def test_model_equals_a_direct_count_over_the_trees():
    seen_outvoted = seen_uninformed = 0
    for n, ref_nw, trees in cases(41):
        ref = flatten.flatten_reference(ref_nw)
        table = bruteforce.count_table(ref.names, trees)
        labels = M.hypotheses(n, 10, 100 + n)
        got, want = M.model_counts(table, labels, n), M.brute_counts(ref.names, trees, labels)
        assert (got == want).all(), (n, trees, labels, got, want)
        assert [int(x) for x in got[:, 0]] == [M.whole_table_quartets(row) for row in labels]
        # shards add: the table cut at two ranks
        cuts = [0, len(table) // 3, len(table) // 3 + 1, len(table)]
        parts = sum(M.model_counts(table[lo:hi], labels, n, rank_lo=lo) for lo, hi in zip(cuts, cuts[1:]))
        assert (parts == got).all()
        seen_outvoted += int(sum(got[:, 4]))
        seen_uninformed += int(sum(got[:, 5]))
    assert seen_outvoted and seen_uninformed


def test_a_planted_branch_is_supported():
    # every tree holds ((a,b),(c,d)) around its central branch: the quad hypothesis a b | c d gets all counts in q1
    names = list("abcdefgh")
    trees = ["((a,e),(b,f),((c,g),(d,h)));", "(((a,b),e,f),((c,g),d),h);", "((a,(b,e)),f,(g,(h,(c,d))));"]
    ids = {x: i for i, x in enumerate(names)}
    table = bruteforce.count_table(names, trees)
    _, labels = engine.parse_group_spec("H\ta\tb\tc\td\nS\ta,b\t*\n", ids)
    got = M.model_counts(table, labels, len(names))
    assert list(got[0]) == [1, 3, 0, 0, 0, 0]
    assert got[1][0] == binom(6, 2) and got[1][1] > got[1][2] + got[1][3]


def test_group_check_kinds_quartets_and_refusals():
    n = 12
    labels = M.hypotheses(n, 12, 5)
    kind, quartets = engine.group_check(n, labels)
    assert kind.dtype == np.uint8 and quartets.dtype == np.uint64
    assert list(kind) == [M.kind_of(row) for row in labels]
    assert [int(x) for x in quartets] == [M.whole_table_quartets(row) for row in labels]
    assert 0 in kind and 1 in kind
    big = np.zeros((1, 65535), dtype=np.uint8)
    big[0, :32768], big[0, 32768:] = 1, 2
    assert int(engine.group_check(65535, big)[1][0]) == int(binom(32768, 2)) * int(binom(32767, 2))

    def refused(row, *words):
        bad = labels.copy()
        bad[7] = row
        with pytest.raises(engine.QSError) as ei:
            engine.group_check(n, bad)
        assert ei.value.code == _lib.QS_ERR_ARG
        for w in ("hypothesis 7",) + words:
            assert w in str(ei.value), str(ei.value)

    z = np.zeros(n, dtype=np.uint8)
    refused(z, "no taxon carries label 1")
    refused(np.r_[1, 1, 2, z[3:]], "only one taxon carries label 2", "split")
    refused(np.r_[1, 2, 2, z[3:]], "only one taxon carries label 1")
    refused(np.r_[1, 1, z[2:]], "no taxon carries label 2")
    refused(np.r_[1, 2, 3, z[3:]], "no taxon carries label 4", "quad")
    refused(np.r_[1, 2, 4, 4, z[4:]], "no taxon carries label 3")
    refused(np.r_[3, 4, 4, z[3:]], "no taxon carries label 1")
    refused(np.r_[1, 2, 3, 4, 5, z[5:]], "taxon 4", "label 5")
    L = _lib.load()
    assert L.qs_group_check(n, None, 1, None, None) == _lib.QS_ERR_ARG
    ok = np.ascontiguousarray(labels)
    assert L.qs_group_check(n, ok.ctypes.data, 0, None, None) == _lib.QS_ERR_ARG
    assert L.qs_group_check(n, ok.ctypes.data, len(ok), None, None) == _lib.QS_OK      # both outputs are optional


def test_parse_group_spec():
    names = ["t%d" % i for i in range(8)]
    ids = {x: i for i, x in enumerate(names)}
    text = ("# a comment\n"
            "\n"
            "mono\tt1,t2, t3\t*\n"
            "rest\t*\tt0,t7\r\n"
            "   \n"
            "quad\tt0\tt1,t2\tt5\tt7,t6\n"
            "  # indented comment\n"
            "two\tt0,t1\tt4,t5")
    got_names, labels = engine.parse_group_spec(text, ids)
    assert got_names == ["mono", "rest", "quad", "two"]
    assert labels.dtype == np.uint8 and labels.tolist() == [[2, 1, 1, 1, 2, 2, 2, 2], [2, 1, 1, 1, 1, 1, 1, 2], [1, 2, 2, 0, 0, 3, 4, 4],
                                                            [1, 1, 0, 0, 2, 2, 0, 0]]
    assert list(engine.group_check(8, labels)[0]) == [1, 1, 0, 1]
    empty_names, empty = engine.parse_group_spec("# nothing\n\n", ids)
    assert empty_names == [] and empty.shape == (0, 8)

    def refused(body, line, *words):
        with pytest.raises(ValueError) as ei:
            engine.parse_group_spec("# head\nfine\tt0,t1\tt2,t3\n" + body, ids)
        for w in (f"line {line}",) + words:
            assert w in str(ei.value), str(ei.value)

    refused("x\tt0,t9\tt1,t2\n", 3, "unknown taxon 't9'")
    refused("\nx\tt0,t1\tt1,t2\n", 4, "'t1'", "two groups")
    refused("x\tt0,t1\t\n", 3, "group 2 is empty")
    refused("x\tt0\tt1\t\tt3\n", 3, "group 3 is empty")
    refused("x\tt0\tt1,t2\n", 3, "group 1", "at least two taxa")
    refused("x\tt0,t1\tt2,t3\tt4\n", 3, "found 3 group(s)")
    refused("x\tt0\tt1\tt2\tt3\tt4\n", 3, "found 5 group(s)")
    refused("x\tt0,t1\n", 3, "found 1 group(s)")
    refused("x\t*\t*\n", 3, "'*'")
    refused("x\tt0\t*\tt2\tt3\n", 3, "'*'")
    refused("x\t*\tt0,t1,t2,t3,t4,t5,t6\n", 3, "group 1", "at least two taxa")
