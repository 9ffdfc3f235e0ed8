"""qs_taxon_support / Context.taxon_support: the six per-taxon sums over the count table, bit for bit against the numpy model
(tests/taxon_model.py) and an accumulation of Context.raw_qic, consistent with the per-tree agreement kernel (which never sees
the table) also at 512 taxa, additive over table shards, repeatable, and without side effects on the table or a pending score."""
import ctypes as C
import functools

import numpy as np
import pytest

import taxon_model as M
from helpers import binom
from quartetscores_amd import _lib, distributed, flatten, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    from quartetscores_amd import engine
    return engine


def mixed_trees(n, seed):
    """dropout, collapsed edges and rooted trees in one batch (as tests/test_gpu_table_remap.py)"""
    return (synth.tree_set(n, 12, seed, dropout=0.2) + synth.tree_set(n, 12, seed + 1, collapse=0.3) +
            synth.tree_set(n, 12, seed + 2, rooted=True) + synth.tree_set(n, 6, seed + 3))


def reference(n, kind, seed):
    rng = np.random.default_rng(seed)
    kw = {"binary": {}, "multifurcating": {"collapse": 0.4}, "rooted": {"rooted": True}}[kind]
    return flatten.flatten_reference(synth.random_tree(n, rng, **kw))


def counted(eng, ref, trees, bits):
    ctx = eng.Context(ref.n_taxa, bits)
    ctx.table_alloc()
    ctx.count_trees(flatten.flatten_eval_trees(trees, ref.name_to_id))
    return ctx


@functools.lru_cache(maxsize=2)
def quads(n):
    return M.quads_in_rank_order(n)


def model(table, ref):
    n = ref.n_taxa
    return M._accumulate(n, quads(n), M._terms(table, M.model_topology(ref, quads(n))))


@pytest.mark.parametrize("kind", ["binary", "multifurcating", "rooted"])
@pytest.mark.parametrize("bits", [16, 32])
@pytest.mark.parametrize("n", [4, 5, 7, 9, 17, 33, 64, 130])
def test_equals_model_of_the_downloaded_table(eng, n, bits, kind):
    ref = reference(n, kind, 1000 + n)
    ctx = counted(eng, ref, mixed_trees(n, 300 + n), bits)
    got = ctx.taxon_support(ref)
    table = ctx.table_download()
    assert got.dtype == np.int64 and got.shape == (n, 6)
    assert (got == model(table, ref)).all()
    if n <= 33:   # an independent device path: every rank's topology and counts from raw_qic
        topo, q = ctx.raw_qic(ref, 0, len(table))
        q = q.astype(np.int64)
        res = topo != 255
        z = np.zeros(len(table), dtype=np.int64)
        terms = np.stack([res.astype(np.int64), q[:, 0], q[:, 1] + q[:, 2], np.where(res, z, table.astype(np.int64).sum(1)),
                          (res & (np.maximum(q[:, 1], q[:, 2]) > q[:, 0])).astype(np.int64),
                          (res & (q.sum(1) == 0)).astype(np.int64)], axis=1)
        assert (got == M._accumulate(n, quads(n), terms)).all()


def agreement_sums(eng, ctx, ref, trees):
    """(concordant, discordant, eval_only) summed over the trees, from qs_tree_agreement"""
    hb = ctx.batch_upload(flatten.flatten_eval_trees(trees, ref.name_to_id))
    try:
        a = ctx.tree_agreement(ref, hb).astype(np.int64)
    finally:
        ctx.batch_free(hb)
    return int(a[:, 0].sum()), int(a[:, 1].sum()), int((a[:, 2] - a[:, 0] - a[:, 1]).sum())


@pytest.mark.parametrize("n,bits", [(40, 32), (96, 16), (512, 16)])
def test_identities_against_the_per_tree_agreement(eng, n, bits):
    ref = reference(n, "multifurcating" if n != 96 else "rooted", 2000 + n)
    trees = mixed_trees(n, 400 + n)
    ctx = counted(eng, ref, trees, bits)
    got = ctx.taxon_support(ref)
    conc, disc, eval_only = agreement_sums(eng, ctx, ref, trees)
    assert int(got[:, 1].sum()) == 4 * conc
    assert int(got[:, 2].sum()) == 4 * disc
    assert int(got[:, 3].sum()) == 4 * eval_only
    assert int(got[:, 0].sum()) == 4 * M.resolved_quartets(ref)
    assert (got[:, 4] + got[:, 5] <= got[:, 0]).all() and (got >= 0).all()
    assert (got[:, 0] <= int(binom(n - 1, 3))).all()
    assert conc > 0 and disc > 0 and (eval_only > 0 or n == 96)


@pytest.mark.parametrize("by", ["c4", "cost"])
@pytest.mark.parametrize("n,bits", [(9, 32), (41, 16), (70, 32)])
def test_shards_add_up(eng, n, bits, by):
    ref = reference(n, "multifurcating", 3000 + n)
    whole = counted(eng, ref, mixed_trees(n, 500 + n), bits)
    want = whole.taxon_support(ref)
    table = whole.table_download()
    bounds = distributed.shard_bounds(n, 3, by)
    total = np.zeros_like(want)
    for lo, hi in zip(bounds, bounds[1:]):
        if lo == hi:      # (more shards than largest ids to hand out: qs_create knows no such context)
            continue
        shard = eng.Context(n, bits, d_lo=lo, d_hi=hi)
        r0, r1 = int(binom(lo, 4)), int(binom(hi, 4))
        shard.table_alloc()
        assert shard.table_tuples == r1 - r0
        if r1 > r0:
            shard.table_upload(table[r0:r1])
        part = shard.taxon_support(ref)
        assert (part == M.model_counts(table[r0:r1], ref, rank_lo=r0)).all()
        total += part
    assert (total == want).all()


def test_empty_shard_gives_zeros(eng):
    n = 20
    ref = reference(n, "binary", 7)
    shard = eng.Context(n, 32, d_lo=0, d_hi=3)
    shard.table_alloc()
    assert shard.table_tuples == 0
    assert (shard.taxon_support(ref) == 0).all()


def test_many_taxa_in_a_shard(eng):
    # 3000 taxa: 141 KB of accumulators in LDS; a shard with the largest ids 4..7 (69 tuples)
    n = 3000
    ref = reference(n, "multifurcating", 8)
    shard = eng.Context(n, 16, d_lo=4, d_hi=8)
    shard.table_alloc()
    r0, r1 = int(binom(4, 4)), int(binom(8, 4))
    table = np.random.default_rng(9).integers(0, 60000, size=(r1 - r0, 3)).astype(np.uint16)
    table[::5] = 0
    shard.table_upload(table)
    assert (shard.taxon_support(ref) == M.model_counts(table, ref, rank_lo=r0)).all()


def test_large_counts_take_the_wide_sums(eng):
    # counts close to 2^32 behind an uploaded 32-bit table (trees unknown): 64-bit partial sums
    n = 70
    ref = reference(n, "multifurcating", 10)
    ctx = eng.Context(n, 32)
    ctx.table_alloc()
    rng = np.random.default_rng(11)
    table = rng.integers(0, 1 << 32, size=(int(binom(n, 4)), 3), dtype=np.uint64).astype(np.uint32)
    table[rng.random(len(table)) < 0.2] = 0
    ctx.table_upload(table)
    got = ctx.taxon_support(ref)
    want = np.zeros((n, 6), dtype=object)   # exact: the weights of the model's bincount would leave float64's integers
    terms = M._terms(table, M.model_topology(ref, quads(n))).astype(object)
    for x in range(4):
        for k in range(6):
            np.add.at(want[:, k], quads(n)[:, x], terms[:, k])
    assert (got.astype(object) == want).all()
    # the same table, said to hold few trees (a wrong hint would be the caller's error; here every count is masked below it)
    small = (table & 0xFFF).astype(np.uint32)
    ctx.table_upload(small)
    ctx.set_tuning(_lib.QS_TUNE_TABLE_TREES, 0xFFF)
    assert (ctx.taxon_support(ref) == model(small, ref)).all()


def test_repeatable_and_without_side_effects(eng):
    import torch
    n = 48
    ref = reference(n, "binary", 12)
    trees = mixed_trees(n, 13)
    ctx = counted(eng, ref, trees, 32)
    before = ctx.table_download()
    first = ctx.taxon_support(ref)
    assert (ctx.taxon_support(ref) == first).all()
    assert (ctx.table_download() == before).all() and ctx.trees_counted == len(trees)

    def scores(between):
        c = counted(eng, ref, trees, 32)
        c.set_tuning(_lib.QS_TUNE_SCORE_PASSES, 2)   # single-read scoring: pass 2 filters the log pass 1 left
        P = c.score_pair_slots(ref)
        sums = torch.empty(3 * P, dtype=torch.int64, device="cuda"); mins = torch.empty(P, dtype=torch.int64, device="cuda")
        cand = torch.empty(8 * P, dtype=torch.int64, device="cuda")
        c.score_pass1(ref, sums, mins)
        if between:
            assert (c.taxon_support(ref) == first).all()
        c.score_pass2(ref, mins, cand)
        logged = c.last_score_log()
        extra = c.score_overflow(ref, mins, cand)
        out = c.score_finish(ref, sums.cpu().numpy(), cand.cpu().numpy()[None, :], extra=extra)
        return logged, [np.asarray(x, dtype=np.float64).view(np.int64) for x in out[:3]]

    (log_a, plain), (log_b, mixed) = scores(False), scores(True)
    # pass 2 filtered pass 1's log both times (0 = it had to read the table); how many records a pass logs depends on the order in
    # which its waves lower the minima, the scores do not
    assert log_a > 0 and log_b > 0
    for x, y in zip(plain, mixed):
        assert (x == y).all()


def test_error_codes(eng):
    import torch
    n = 12
    ref = reference(n, "binary", 14)
    ctx = counted(eng, ref, mixed_trees(n, 15), 32)
    want = ctx.taxon_support(ref)

    def code(f):
        with pytest.raises(eng.QSError) as ei:
            f()
        return ei.value.code

    assert code(lambda: eng.Context(n, 32).taxon_support(ref)) == _lib.QS_ERR_STATE          # no table
    assert code(lambda: ctx.taxon_support(reference(n + 1, "binary", 14))) == _lib.QS_ERR_ARG  # n_taxa differs
    bad = reference(n, "binary", 14)
    bad.leaf_node = bad.leaf_node.copy()
    bad.leaf_node[[0, n - 1]] = bad.leaf_node[[n - 1, 0]]   # ids 0 and n-1 swapped: not depth-first any more
    assert code(lambda: ctx.taxon_support(bad)) == _lib.QS_ERR_ARG
    buf = torch.zeros(6 * n + 1, dtype=torch.int64, device="cuda")
    s, keep = ctx._ref_struct(ref)
    assert ctx.L.qs_taxon_support(ctx.h, C.byref(s), C.c_void_p(buf.data_ptr() + 4)) == _lib.QS_ERR_ARG   # misaligned
    assert ctx.L.qs_taxon_support(ctx.h, C.byref(s), None) == _lib.QS_ERR_ARG
    # C(2999,3) x (2^32 - 1) does not fit 63 bits; with the trees known it does
    big_ref = reference(3000, "binary", 16)
    big = eng.Context(3000, 32, d_lo=4, d_hi=6)
    big.table_alloc()
    assert code(lambda: big.taxon_support(big_ref)) == _lib.QS_ERR_OVERFLOW
    big.set_tuning(_lib.QS_TUNE_TABLE_TREES, 1000)
    assert (big.taxon_support(big_ref)[:, 1:5] == 0).all()
    wide = eng.Context(3500, 16, d_lo=4, d_hi=6)
    wide.table_alloc()
    assert code(lambda: wide.taxon_support(reference(3500, "binary", 17))) == _lib.QS_ERR_UNSUPPORTED
    assert (ctx.taxon_support(ref) == want).all()            # and the context still works after the refusals
