"""tests/agree_rounds.py against the source it restates, and the shapes of tests/test_gpu_tree_rounds.py against the rounds they are
named for: a shape that no longer holds its path would let the device test pass without testing it. No GPU."""
import os
import re

import numpy as np
import pytest

import agree_rounds as AR
from quartetscores_amd import flatten, newick

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "quartetscores_amd", "csrc")


@pytest.mark.parametrize("n,want", [(40, (2, 256, 64)), (340, (11, 256, 64)), (600, (19, 256, 64)), (991, (31, 256, 64)),
                                    (992, (32, 252, 63)), (1100, (35, 232, 58)), (2259, (71, 112, 28))])
def test_plan_values(n, want):
    assert AR.plan(n) == want


def test_plan_is_the_one_in_the_source():
    """the LDS budget, the three assignments of agree_plan, the LDS size of the launches and the walk of the three kernels, as text"""
    squeeze = lambda s: re.sub(r"\s+", "", s)
    with open(os.path.join(CSRC, "qs_agree.hip")) as f:
        src = f.read()
    assert re.search(r"constexpr\s+uint32_t\s+kAgreeLdsBytes\s*=\s*(\d+)\s*;", src).group(1) == str(AR.LDS_BYTES)
    body = re.search(r"void agree_plan\(uint32_t n, uint32_t &W, uint32_t &cap, uint32_t &nb\) \{(.*?)\n\}", src, re.S).group(1)
    assert [squeeze(s) for s in body.strip().split("\n")] == [
        "W=n/32+1;",
        "constuint32_tcap_max=(kAgreeLdsBytes/8-W)/W;",
        "nb=std::max(1u,std::min(64u,cap_max/4));",
        "cap=std::min(cap_max,4*nb);",
    ]
    for name, arrays in (("qs_agree.hip", "a."), ("qs_agree_pairs.hip", "a.t."), ("qs_tree_branch.hip", "a.")):
        with open(os.path.join(CSRC, name)) as f:
            text = squeeze(f.read())
        assert "agree_plan(n,a.W,a.cap,a.nb);" in text, name
        assert "constsize_tlds=(size_t)(a.W+a.cap*a.W)*sizeof(uint2);" in text, name
        r = arrays + "rng_off"
        assert f"constuint32_tk_base={r}[v0];uint32_tv1=v0;while(v1<v_hi&&{r}[v1+1]-k_base<=a.cap)++v1;" \
               f"constboolstored=v1>v0;if(!stored)v1=v0+1;" in text, name
        assert "blockIdx.y*a.nb" in text and "min(v_lo+a.nb,v_all)" in text, name


def blocks_of(n, text, recentre=True):
    b = flatten.flatten_eval_trees([text], {nm: i for i, nm in enumerate(AR.names_of(n))}, recentre)
    return b, AR.rounds(b, n)[0]


@pytest.fixture(scope="module")
def shapes_340():
    return AR.SHAPES_340(AR.names_of(340))


@pytest.mark.parametrize("recentre", [True, False])
def test_hub_shapes_340(shapes_340, recentre):
    assert AR.plan(340) == (11, 256, 64)
    get = lambda k: blocks_of(340, shapes_340[k], recentre)

    b, bl = get("hub257_mid")                       # stored, unstored, stored in block 1
    assert AR.max_links(b) == [257] and AR.kinds(bl[0]) == "S" and bl[0][0] == ("S", 64)
    assert AR.kinds(bl[1]) == "SUS" and len(bl) == 2

    b, bl = get("hub256")                           # as many links as the budget: stored, alone in its round
    assert AR.max_links(b) == [256] and bl[0] == [("S", 64)]
    assert AR.kinds(bl[1]) == "SSS" and bl[1][1] == ("S", 1)
    links = np.diff(b.rng_off.astype(np.int64))
    assert links[64 + bl[1][0][1]] == 256

    b, bl = get("hub_first")                        # the root of the text: no parent link, the first node of block 0
    assert np.diff(b.rng_off.astype(np.int64))[0] == 257 and AR.kinds(bl[0]).startswith("US")

    b, bl = get("hub_last")                         # the last inner node of the tree; all its children are leaves
    links = np.diff(b.rng_off.astype(np.int64))
    assert links[-1] == 257 and AR.kinds(bl[-1]).endswith("SU") and len(bl) == 2
    k0 = int(b.rng_off[-2])
    lens = [(int(b.ranges[2 * k + 1]) + 340 - int(b.ranges[2 * k])) % 340 for k in range(k0, k0 + 257)]
    assert sorted(lens) == [1] * 256 + [340 - 256]

    b, bl = get("hub_dropout")                      # lacks 8 - 10 % of the taxa; stored nodes on both sides of the hub
    L = int(b.leaf_off[1])
    assert 0.90 * 340 <= L <= 0.92 * 340 and AR.max_links(b)[0] >= 257 and "SUS" in AR.kinds(bl[0])
    assert len(newick.parse_tree(shapes_340["hub_dropout"]).children) == 2   # written rooted

    for k in ("hub257_mid", "hub_first", "hub_last", "hub_dropout"):   # one unstored node each, and it is the hub
        assert sum(AR.kinds(x).count("U") for x in get(k)[1]) == 1, k


@pytest.mark.parametrize("name", ["fans7", "fans5"])
def test_fan_shapes_340(shapes_340, name):
    b, bl = blocks_of(340, shapes_340[name])
    assert int(b.leaf_off[1]) == 340 and AR.max_links(b)[0] == int(name[-1])
    assert all("U" not in AR.kinds(x) for x in bl)
    assert any(AR.kinds(x).count("S") >= 2 for x in bl)
    assert sum(r[1] for x in bl for r in x) == int(b.node_off[1])   # the rounds take every node once


def test_two_hubs():
    n = 550
    assert 530 <= n <= 560 and AR.plan(n)[1:] == (256, 64)
    for recentre in (True, False):
        b, bl = blocks_of(n, AR.two_hubs(AR.names_of(n)), recentre)
        links = np.diff(b.rng_off.astype(np.int64))
        big = np.nonzero(links >= 257)[0]
        assert len(big) == 2 and big[1] == big[0] + 1 and big[1] < 64      # next to each other, in one block
        assert "SUUS" in AR.kinds(bl[0])


@pytest.mark.parametrize("n", [1100, 2259])
def test_sparse_shapes_of_the_large_plans(n):
    W, cap, nb = AR.plan(n)
    assert (W, cap, nb) == {1100: (35, 232, 58), 2259: (71, 112, 28)}[n]
    shapes = AR.sparse_shapes(AR.names_of(n))
    for name, text in shapes.items():
        b, bl = blocks_of(n, text)
        assert 300 <= int(b.leaf_off[1]) <= 340
        assert len(set((b.leaf_ids >> 5).tolist())) == W, name           # every word of the bitmaps is in use
        if name == "hub":
            assert AR.max_links(b) == [cap + 1]
            assert [AR.kinds(x) for x in bl].count("SUS") == 1 and sum(AR.kinds(x).count("U") for x in bl) == 1
            assert AR.kinds(bl[0]) == "S"                                # the hub is not in the first block
        else:
            assert all("U" not in AR.kinds(x) for x in bl) and sum(AR.kinds(x).count("S") >= 2 for x in bl) >= 1
            assert max(r[1] for x in bl for r in x) < nb                 # no round holds a whole block


def test_rounds_of_small_and_ordinary_trees():
    ids = {nm: i for i, nm in enumerate(AR.names_of(12))}
    b = flatten.flatten_eval_trees(["(t0,t1,t2);", "((t0,t1),(t2,t3),(t4,t5));", "(t0,t1,t2,t3,t4,t5,t6,t7,t8,t9,t10,t11);"], ids)
    assert AR.rounds(b, 12) == [[], [[("S", 4)]], [[("S", 1)]]]
    assert AR.max_links(b) == [3, 3, 12]


def test_generators_give_the_trees_they_describe():
    rng = np.random.default_rng(0)
    names = AR.names_of(60)
    for text in (AR.hub_tree(names, 10, 30, 5, rng), AR.hub_tree(names, 0, 30, 5, rng), AR.hub_tree(names, 30, 30, 0, rng),
                 AR.hub_tree(names[:50], 5, 20, 3, rng, rooted=True), AR.fan_tree(names, 6, rng), AR.two_hub_tree(names, 5, 20, rng)):
        assert sorted(re.findall(r"t\d+", text), key=lambda s: int(s[1:])) in (names, names[:50])
    b, _ = blocks_of(60, AR.hub_tree(names, 10, 30, 5, rng))
    links = np.diff(b.rng_off.astype(np.int64)).tolist()
    assert links[10] == 31 and links.count(31) == 1 and set(links) == {3, 31}
    assert len(links) == 10 + 1 + 5 + (60 - 10 - 30 - 5 - 1)   # top and first subtree, hub, cherries, the rest
    b, _ = blocks_of(60, AR.hub_tree(names, 0, 30, 5, rng))
    assert np.diff(b.rng_off.astype(np.int64)).tolist()[0] == 30
    b, _ = blocks_of(60, AR.fan_tree(names, 6, rng))
    links = np.diff(b.rng_off.astype(np.int64)).tolist()
    assert set(links[1:]) == {6} and 3 <= links[0] <= 6
    assert AR.relabel_in_order("((t5,t3),t9,(t0,t1));") == "((t0,t1),t2,(t3,t4));"
    spread = AR.spread_names(AR.names_of(2259), 320, rng)
    assert len(set(spread)) == 320 and len({int(s[1:]) >> 5 for s in spread}) == 71
