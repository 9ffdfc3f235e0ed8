"""Pruning a reference tree: the C++ host's rule (csrc/host/newick.hpp prune, through qsh_prune_newick) against
quartetscores_amd.newick.prune, hand cases for every step of the rule, and flatten.taxon_restriction, the id map of
qs_table_restrict that follows from it."""
import numpy as np
import pytest

from quartetscores_amd import flatten, native_ingest, newick, synth


def with_lengths(nw, rng, share):
    """the generator's Newick with a branch length on about `share` of its nodes (it writes none)"""
    out = []
    for i, ch in enumerate(nw):
        if ch in ",);" and i and nw[i - 1] not in "(," and not (ch == ";") and rng.random() < share:
            out.append(":%s" % rng.choice(["0.1", "0.25", "1e-3", "2", "0.30000000000000004", "7.5"]))
        out.append(ch)
    return "".join(out)


def shape(root):
    """{leaf set of a node: (leaf sets of its children in order, branch length as a double or None)} and the root's key"""
    out = {}

    def rec(x):
        if x.is_leaf:
            key = frozenset([x.name])
            kids = ()
        else:
            sets = [rec(c) for c in x.children]
            key = frozenset().union(*sets)
            kids = tuple(sets)
        assert key not in out, "a node with one child is left"
        out[key] = (kids, None if x.length is None else float(x.length))
        return key
    return out, rec(root)


def test_cpp_and_python_pruners_agree_on_random_trees():
    rng = np.random.default_rng(2024)
    nothing_left = splices = 0
    for it in range(400):
        n = int(rng.integers(4, 16))
        nw = synth.random_tree(n, rng, collapse=float(rng.choice([0.0, 0.3])), rooted=bool(it % 3 == 0))
        nw = with_lengths(nw, rng, float(rng.choice([0.0, 0.6, 1.0])))
        drop = [f"t{i}" for i in range(n) if rng.random() < rng.choice([0.1, 0.4, 0.9])] + ["not_there"]
        got = native_ingest.prune_newick(nw, drop)
        py = newick.prune(newick.parse_tree(nw), drop)
        if py is None:
            assert got == ""
            nothing_left += 1
            continue
        assert shape(newick.parse_tree(got)) == shape(py), (nw, drop, got, newick.write(py))
        assert got == newick.write(py)                        # and the same text (labels, the text of the lengths)
        # the kept leaves keep their relative depth-first order
        kept = [x.name for x in newick.preorder(newick.parse_tree(nw)) if x.is_leaf and x.name not in set(drop)]
        assert [x.name for x in newick.preorder(py) if x.is_leaf] == kept
        root = newick.parse_tree(nw)
        if len(root.children) >= 3 and len(kept) >= 3:
            assert len(py.children) >= 3                      # an unrooted tree stays unrooted
        splices += got.count(":") < nw.count(":")
    assert nothing_left and splices


HAND = [
    # a whole root subtree dropped from an unrooted tree (step 4): the first inner child dissolves, its length goes to the other
    ("((a:1,b:2)x:3,(c:1,d:1)y:0.5,(e:1,(f:1,g:1):0.1)z:0.25);", "e f g", "(a:1,b:2,(c:1,d:1)y:3.5);"),
    ("(a:1,(c:1,d:1)y:0.5,(e:1,f:1)z:0.25);", "e f", "(a:1.5,c:1,d:1);"),
    ("((a,b),(c,d),(e,f));", "a b", "(c,d,(e,f));"),
    # the same from a rooted tree: the root keeps its two children
    ("((a:1,b:2)x:3,((c:1,d:1)y:0.5,(e:1,(f:1,g:1):0.1)z:0.25)w:0.2);", "e f g", "((a:1,b:2)x:3,(c:1,d:1)y:0.7);"),
    ("((a,b),((c,d),(e,f)));", "a", "(b,((c,d),(e,f)));"),
    # a cherry reduced to one leaf (step 2): the lengths are summed, a missing one counts as absent, the label goes
    ("((a:1,b:2)x:3,c,d,e);", "b", "(a:4,c,d,e);"),
    ("((a,b:2)x:3,c,d,e);", "b", "(a:3,c,d,e);"),
    ("((a:1,b:2)x,c,d,e);", "b", "(a:1,c,d,e);"),
    ("((a,b)x,c,d,e);", "a", "(b,c,d,e);"),
    # a chain of splices
    ("((((a:0.1,b:0.2):0.3,c):0.4,d:1):0.5,e,f,g);", "b c d", "(a:1.3,e,f,g);"),
    # a root with one child left (step 3): the child becomes the root and loses its length
    ("((a,b,(c,d))x:5,e,f);", "e f", "(a,b,(c,d))x;"),
    ("(((a,b,(c,d))x:5)y:1,e);", "e", "(a,b,(c,d))x;"),
    # ... and step 4 holds for the node that replaced an unrooted tree's root as well; a rooted tree's stays at two children
    ("(((a,b),(c,d)),e,f);", "e f", "(a,b,(c,d));"),
    ("(((a:1,b:1):0.5,(c:1,d:1):0.25):2,e,f);", "e f", "(a:1,b:1,(c:1,d:1):0.75);"),
    ("(((a,b),(c,d)),e);", "e", "((a,b),(c,d));"),
    # inner nodes left without children go, repeatedly
    ("(((a,b),(c,d)),e,f,g,h);", "a b c d", "(e,f,g,h);"),
    # quoted labels: matched as parsed, written quoted again
    ("(('a b':1,'it''s':2),c,d,'e(1)');", ["a b"], "('it''s':2,c,d,'e(1)');"),
    ("(('a b':1,'it''s':2),c,d,'e(1)');", ["it's", "e(1)"], "('a b':1,c,d);"),
    # nothing left
    ("((a,b),c);", "a b c", ""),
]


@pytest.mark.parametrize("nw,drop,want", HAND)
def test_hand_cases(nw, drop, want):
    names = drop.split() if isinstance(drop, str) else drop
    assert native_ingest.prune_newick(nw, names) == want
    py = newick.prune(newick.parse_tree(nw), names)
    assert (newick.write(py) if py is not None else "") == want


def test_prune_leaves_its_argument_alone():
    nw = "((a:1,b:2)x:3,(c:1,d:1)y:0.5,(e:1,f:1)z:0.25);"
    root = newick.parse_tree(nw)
    newick.prune(root, ["e", "f", "b"])
    assert newick.write(root) == nw


def test_taxon_restriction_is_increasing_for_a_pruned_tree():
    rng = np.random.default_rng(7)
    for n in (8, 21):
        nw = synth.random_tree(n, rng, collapse=0.2)
        src = flatten.flatten_reference(nw)
        drop = [src.names[i] for i in rng.choice(n, size=n // 3, replace=False)]
        dst = flatten.flatten_reference(newick.prune(newick.parse_tree(nw), drop))
        ids = flatten.taxon_restriction(dst, src)
        assert ids.dtype == np.uint16 and len(ids) == n - len(drop)
        assert (np.diff(ids.astype(np.int64)) > 0).all()
        assert [src.names[i] for i in ids] == dst.names
        assert sorted(set(range(n)) - set(ids.tolist())) == sorted(src.name_to_id[nm] for nm in drop)
    a = flatten.flatten_reference("((t0,t1),(t2,t3),(t4,t5));")
    b = flatten.flatten_reference("((t5,t2),t0,t3);")
    assert list(flatten.taxon_restriction(b, a)) == [5, 2, 0, 3]           # any order: a subset of another tree
    assert list(flatten.taxon_restriction(a, a)) == list(flatten.taxon_permutation(a, a))


def test_taxon_restriction_names_the_taxa_the_source_lacks():
    a = flatten.flatten_reference("((t0,t1),(t2,t3),(t4,t5));")
    b = flatten.flatten_reference("((t0,t9),t2,(t7,t3));")
    with pytest.raises(ValueError, match=r"missing none; extra t7, t9"):
        flatten.taxon_restriction(b, a)
