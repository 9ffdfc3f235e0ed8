"""qs_table_collapse: a count table over individuals summed into the table of their species equals the specification
(tests/species_model.py) cell for cell, agrees with qs_group_support's quad sums, and scores like the table it stands for --
with cells above trees-counted."""
import functools

import numpy as np
import pytest

import helpers
from oracle_api import Oracle
from species_model import collapse_table, individuals_of, with_clades
from quartetscores_amd import _lib, flatten, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    from quartetscores_amd import engine
    return engine


def rank4(a, b, c, d):
    return int(helpers.binom(d, 4) + helpers.binom(c, 3) + helpers.binom(b, 2) + a)


# ---- addressing: every cell of a table that names its own (rank, slot), small enough for no sum to overflow ---------------

@functools.lru_cache(maxsize=None)
def hashed_table(n, bits):
    """(C(n,4), 3): cell (rank, slot) = a hash of (rank, slot) reduced to 0..250, so that a tuple or a slot taken from the
    wrong place shows and the largest sum of the cases below (66 x 2 x 250) fits 16 bits"""
    cell = np.arange(3 * int(helpers.binom(n, 4)), dtype=np.uint64)
    h = (cell + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
    h ^= h >> np.uint64(29)
    t = ((h >> np.uint64(13)) % np.uint64(251)).astype(np.uint32 if bits == 32 else np.uint16).reshape(-1, 3)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def uploaded(eng, n, bits):
    ctx = eng.Context(n, bits)
    ctx.table_alloc()
    ctx.table_upload(hashed_table(n, bits))
    return ctx


def random_sizes(n_src, n_dst, largest):
    """n_dst group sizes in 1..largest that add up to n_src, seeded by the shape. The four largest multiply to at most 400: a
    destination cell is the sum of that many hashed cells of 125 on average (50 000, and 65 535 is ten standard deviations
    away), so that the 16-bit destinations hold every sum -- the test asserts that of the model's table."""
    rng = np.random.default_rng(1000 * n_src + n_dst)
    sizes = np.ones(n_dst, dtype=np.int64)
    for _ in range(100000):
        if sizes.sum() == n_src:
            return tuple(int(x) for x in sizes)
        i = int(rng.integers(n_dst))
        sizes[i] += 1
        if sizes[i] > largest or np.prod(np.sort(sizes)[-4:]) > 400:
            sizes[i] -= 1
    raise AssertionError("no such sizes")


CASES = {
    "4-singletons": (1, 1, 1, 1),                       # one tuple
    "5-pair-at-0": (2, 1, 1, 1), "5-pair-at-1": (1, 2, 1, 1), "5-pair-at-2": (1, 1, 2, 1), "5-pair-at-3": (1, 1, 1, 2),
    "9-to-4": (2, 2, 2, 3),                             # one destination tuple, the sum of 24
    "33-singletons": (1,) * 33,                         # a copy
    "70-to-23": random_sizes(70, 23, 6),                # row prefixes longer than a wave
    "70-to-4-long-first": (66, 1, 2, 1),                # a group longer than a wave, at either end
    "70-to-4-long-last": (1, 2, 1, 66),
    "131-to-40": random_sizes(131, 40, 8),              # 1.1e7 source tuples, C(39,3) = 9139 destination rows: 572 workgroups
}
CELLS = [(32, 32), (16, 16), (16, 32)]


def first_of(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint16)


@functools.lru_cache(maxsize=None)
def model(sizes, src_bits):
    want = collapse_table(hashed_table(sum(sizes), src_bits), sum(sizes), first_of(sizes))
    want.setflags(write=False)
    return want


def collapsed(eng, src, first, bits=None):
    dst = eng.Context(len(first) - 1, bits or src.count_bits)
    dst.table_alloc()
    dst.table_collapse(src, first)
    dst.sync()
    return dst


def test_the_case_list_is_what_it_says():
    assert {k: sum(v) for k, v in CASES.items() if k[0] in "79"} == {"9-to-4": 9, "70-to-23": 70, "70-to-4-long-first": 70, "70-to-4-long-last": 70}
    assert sum(CASES["131-to-40"]) == 131 and len(CASES["131-to-40"]) == 40 and len(CASES["70-to-23"]) == 23
    assert max(CASES["70-to-23"]) <= 6 and np.cumsum(CASES["70-to-23"])[-2] > 64


@pytest.mark.parametrize("cells", CELLS, ids=lambda c: f"{c[0]}to{c[1]}")
@pytest.mark.parametrize("case", list(CASES))
def test_every_cell_is_the_sum_of_the_right_cells(eng, case, cells):
    sizes = CASES[case]
    src = uploaded(eng, sum(sizes), cells[0])
    got = collapsed(eng, src, first_of(sizes), cells[1]).table_download()
    want = model(sizes, cells[0])
    assert got.dtype == (np.uint32 if cells[1] == 32 else np.uint16) and got.shape == want.shape
    assert int(want.max()) <= 65535
    assert (got == want).all()
    if set(sizes) == {1}:
        assert (got == hashed_table(len(sizes), cells[0])).all()       # singletons: a copy


# ---- cell limits ----------------------------------------------------------------------------------------------------------

def filled(eng, n, bits, value):
    ctx = eng.Context(n, bits)
    ctx.table_alloc()
    ctx.table_upload(np.full((int(helpers.binom(n, 4)), 3), value, dtype=np.uint32 if bits == 32 else np.uint16))
    return ctx


def test_sums_of_exactly_65535_fit_16_bits(eng):
    got = collapsed(eng, filled(eng, 6, 16, 21845), first_of((3, 1, 1, 1)), 16).table_download()
    assert got.shape == (1, 3) and (got == 65535).all()


def test_a_sum_of_65536_overflows_16_bits_and_fits_32(eng):
    src = filled(eng, 5, 16, 32768)
    first = first_of((2, 1, 1, 1))
    dst = eng.Context(4, 16)
    dst.table_alloc()
    dst.table_collapse(src, first)
    with pytest.raises(eng.QSError) as ei:
        dst.sync()
    assert ei.value.code == _lib.QS_ERR_OVERFLOW
    assert (collapsed(eng, src, first, 32).table_download() == 65536).all()


def test_a_sum_of_2_to_the_32_overflows(eng):
    dst = eng.Context(4, 32)
    dst.table_alloc()
    dst.table_collapse(filled(eng, 5, 32, 1 << 31), first_of((2, 1, 1, 1)))
    with pytest.raises(eng.QSError) as ei:
        dst.sync()
    assert ei.value.code == _lib.QS_ERR_OVERFLOW


# ---- real trees -------------------------------------------------------------------------------------------------------------

def mixed_trees(n, seed):
    """dropout, collapsed edges and rooted trees in one batch"""
    return (synth.tree_set(n, 12, seed, dropout=0.2) + synth.tree_set(n, 12, seed + 1, collapse=0.3) +
            synth.tree_set(n, 12, seed + 2, rooted=True) + synth.tree_set(n, 6, seed + 3))


def counted(eng, name_to_id, trees, bits=16):
    ctx = eng.Context(len(name_to_id), bits)
    ctx.table_alloc()
    ctx.count_trees(flatten.flatten_eval_trees(trees, name_to_id))
    return ctx


REAL_SIZES = (3, 1, 4, 2, 2, 5, 1, 3, 3)      # 24 individuals in 9 species


@pytest.fixture(scope="module")
def real(eng):
    n = sum(REAL_SIZES)
    names = [f"t{i}" for i in range(n)]
    trees = mixed_trees(n, 51)
    src = counted(eng, {nm: i for i, nm in enumerate(names)}, trees)
    first = first_of(REAL_SIZES)
    want = collapse_table(src.table_download(), n, first)
    return src, first, want, len(trees)


def test_collapse_of_a_counted_table_equals_the_model(eng, real):
    src, first, want, m = real
    for bits in (16, 32):
        dst = collapsed(eng, src, first, bits)
        assert (dst.table_download() == want).all()
        assert dst.trees_counted == src.trees_counted == m
    assert want.max() > m                                           # cells above trees-counted


def test_collapsed_tuples_equal_the_quad_sums_of_group_support(eng, real):
    src, first, want, _ = real
    got = collapsed(eng, src, first).table_download()
    W, X, Y, Z = 0, 2, 5, 8
    tuple_ = got[rank4(W, X, Y, Z)].astype(np.int64)
    # the three label orders of the four species: S1 S2 | S3 S4 puts (F1, F2, F3) at these slots of the sorted tuple
    for order, slots in (((W, X, Y, Z), (0, 1, 2)), ((W, Y, X, Z), (1, 0, 2)), ((W, Z, X, Y), (2, 0, 1))):
        labels = np.zeros(sum(REAL_SIZES), dtype=np.uint8)
        for k, s in enumerate(order, 1):
            labels[first[s]:first[s + 1]] = k
        words = np.asarray(src.group_support(labels), dtype=np.int64).reshape(-1, 6)[0]
        assert words[0] == np.prod([REAL_SIZES[s] for s in order])
        assert words[1:4].tolist() == [int(tuple_[k]) for k in slots], order
    assert tuple_.sum() > 0


# ---- scores with cells above trees-counted --------------------------------------------------------------------------------

def by_bipartition(eng, ref, lq, qp, eqp, bif):
    q = eng.QuartetScoreComputer.__new__(eng.QuartetScoreComputer)
    q.ref, q._lq, q._qp, q._eqp = ref, lq[1:], (qp[1:] if bif else None), (eqp[1:] if bif else None)
    return q.scores_by_bipartition()


def assert_scores_equal(eng, ref, got, want, what):
    got = by_bipartition(eng, ref, *got)
    assert set(got) == set(want)
    for k in want:
        for g, w in zip(got[k], want[k]):
            assert (g is None and w is None) or int(helpers.ulp_diff(g, w)) == 0, (what, sorted(k), got[k], want[k])


@pytest.mark.parametrize("kind", ["bifurcating", "multifurcating", "rooted"])
def test_clades_of_two_score_like_sixteen_copies_of_the_species_trees(eng, kind):
    n, k = 12, 2
    rng = np.random.default_rng(61)
    ref_nw = {"bifurcating": synth.random_tree(n, rng), "multifurcating": synth.random_tree(n, rng, collapse=0.4),
              "rooted": synth.random_tree(n, rng, rooted=True)}[kind]
    ref = flatten.flatten_reference(ref_nw)
    species_trees = (synth.tree_set(n, 10, 62) + synth.tree_set(n, 10, 63, collapse=0.3) + synth.tree_set(n, 10, 64, dropout=0.2))
    gene_trees = [with_clades(nw, k, rng) for nw in species_trees]
    lay = flatten.species_layout(ref, {s: individuals_of(s, k) for s in ref.names})
    assert lay.first_id.tolist() == list(range(0, 2 * n + 1, 2))
    dst = collapsed(eng, counted(eng, lay.name_to_id, gene_trees), lay.first_id)
    o = Oracle(ref_nw)
    o.count("\n".join(species_trees), mult=[k ** 4] * len(species_trees))
    assert o.names == ref.names
    got = dst.table_download()
    assert (got.astype(np.uint64) == o.counts()).all()
    assert got.max() > dst.trees_counted == len(species_trees)
    o.score(qp_exact64=False)
    scores = dst.score(ref, eng.QS_SCORE_QP_WRAP32)
    assert scores[3] == o.bifurcating == (kind != "multifurcating")
    assert_scores_equal(eng, ref, scores, o.scores_by_bipartition(), "wrap32")
    o.score(qp_exact64=True)
    assert_scores_equal(eng, ref, dst.score(ref, eng.QS_SCORE_QP_EXACT64), o.scores_by_bipartition(), "exact64")


def test_cells_beyond_the_log_tables_floor_score_and_sum_like_the_oracle(eng):
    """clades of six: cells of 1296 x (up to 80 trees) pass 65 536, the size the score's log table has for at most that many trees, so
    the bound qs_table_collapse records is what sizes it; the same holds for a table re-indexed out of the collapsed one and for the
    per-taxon sums over it"""
    import taxon_model
    n, k = 12, 6
    rng = np.random.default_rng(65)
    ref_nw = synth.random_tree(n, rng)
    ref = flatten.flatten_reference(ref_nw)
    species_trees = [ref_nw] * 60 + synth.tree_set(n, 20, 66)
    gene_trees = [with_clades(nw, k, rng) for nw in species_trees]
    lay = flatten.species_layout(ref, {s: individuals_of(s, k) for s in ref.names})
    dst = collapsed(eng, counted(eng, lay.name_to_id, gene_trees), lay.first_id, 32)
    o = Oracle(ref_nw)
    o.count("\n".join(species_trees), mult=[k ** 4] * len(species_trees))
    got = dst.table_download()
    assert (got.astype(np.uint64) == o.counts()).all()
    assert got.max() >= 60 * 1296 > 65536 > dst.trees_counted == 80
    again = eng.Context(n, 32)
    again.table_alloc()
    again.table_remap(dst, np.arange(n))
    for qp_exact64, flags in ((False, eng.QS_SCORE_QP_WRAP32), (True, eng.QS_SCORE_QP_EXACT64)):
        o.score(qp_exact64=qp_exact64)
        for ctx in (dst, again):
            assert_scores_equal(eng, ref, ctx.score(ref, flags), o.scores_by_bipartition(), flags)
    want = taxon_model.model_counts(got, ref)
    for ctx in (dst, again):
        assert (np.asarray(ctx.taxon_support(ref)).astype(np.int64).reshape(n, 6) == want).all()


def test_scores_equal_those_of_the_uploaded_model_table(eng, real):
    src, first, want, _ = real
    ref = flatten.flatten_reference(synth.reference_tree(len(REAL_SIZES), 71))
    dst = collapsed(eng, src, first, 32)
    fresh = eng.Context(len(REAL_SIZES), 32)
    fresh.table_alloc()
    fresh.table_upload(want.astype(np.uint32))
    for flags in (eng.QS_SCORE_QP_WRAP32, eng.QS_SCORE_QP_EXACT64, eng.QS_SCORE_QP_EXACT64 | eng.QS_SCORE_ROOT_AS_EDGE):
        a, b = dst.score(ref, flags), fresh.score(ref, flags)
        assert a[3] == b[3]
        for x, y in zip(a[:3], b[:3]):
            assert (x.view(np.int64) == y.view(np.int64)).all()


# ---- re-use of a destination ------------------------------------------------------------------------------------------------

def test_second_collapse_and_score_leave_nothing_of_the_first(eng, real):
    src, _, _, _ = real
    n = sum(REAL_SIZES)
    ref = flatten.flatten_reference(synth.reference_tree(len(REAL_SIZES), 72))
    dst = eng.Context(len(REAL_SIZES), 32)
    dst.table_alloc()
    layouts = [REAL_SIZES, REAL_SIZES[::-1]]
    assert layouts[0] != layouts[1]
    for sizes in layouts:
        first = first_of(sizes)
        dst.table_collapse(src, first)
        dst.sync()
        want = collapse_table(src.table_download(), n, first)
        assert (dst.table_download() == want).all()
        fresh = eng.Context(len(sizes), 32)
        fresh.table_alloc()
        fresh.table_upload(want.astype(np.uint32))
        for x, y in zip(dst.score(ref)[:3], fresh.score(ref)[:3]):    # (not the log of the earlier score)
            assert (x.view(np.int64) == y.view(np.int64)).all()


# ---- refusals ---------------------------------------------------------------------------------------------------------------

def test_error_codes(eng):
    n, sizes = 12, (2, 1, 1, 3, 1, 1, 2, 1)
    src = uploaded(eng, n, 32)
    first = first_of(sizes)

    def code(dst, first=first, source=src):
        with pytest.raises(eng.QSError) as ei:
            dst.table_collapse(source, first)
        return ei.value.code

    dst = eng.Context(len(sizes), 32)
    dst.table_alloc()
    mark = np.full((int(helpers.binom(len(sizes), 4)), 3), 7, dtype=np.uint32)
    dst.table_upload(mark)
    bad = first.copy(); bad[3], bad[4] = first[4], first[3]
    assert code(dst, bad) == _lib.QS_ERR_ARG                            # not increasing
    bad = first.copy(); bad[2] = bad[1]
    assert code(dst, bad) == _lib.QS_ERR_ARG                            # an empty group
    bad = first.copy(); bad[0] = 1
    assert code(dst, bad) == _lib.QS_ERR_ARG                            # does not begin at 0
    bad = first.copy(); bad[-1] = n - 1
    assert code(dst, bad) == _lib.QS_ERR_ARG                            # does not end at n_src
    larger = eng.Context(n + 1, 32)
    larger.table_alloc()
    assert code(larger, np.arange(n + 2)) == _lib.QS_ERR_ARG            # n_dst > n_src
    narrow = eng.Context(len(sizes), 16)
    narrow.table_alloc()
    assert code(narrow) == _lib.QS_ERR_ARG                              # 32 -> 16 bits
    shard = eng.Context(len(sizes), 32, d_lo=0, d_hi=len(sizes) - 2)
    shard.table_alloc()
    assert code(shard) == _lib.QS_ERR_UNSUPPORTED                       # a table shard as destination
    src_shard = eng.Context(n, 32, d_lo=0, d_hi=n - 2)
    src_shard.table_alloc()
    assert code(dst, source=src_shard) == _lib.QS_ERR_UNSUPPORTED       # ... and as source
    assert code(eng.Context(len(sizes), 32)) == _lib.QS_ERR_STATE       # a destination without a table
    assert code(dst, source=eng.Context(n, 32)) == _lib.QS_ERR_STATE    # a source without one
    dst.sync()
    assert (dst.table_download() == mark).all() and dst.trees_counted == 0   # unchanged by the refused calls
    dst.table_collapse(src, first)                                      # and the context still works
    dst.sync()
    assert (dst.table_download() == model(sizes, 32)).all()
