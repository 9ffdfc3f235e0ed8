"""The score passes of qs_score.hip per node pair against tests/score_model.py: what every rank of a multi-GPU run hands to
the collectives -- sums_dev[3P], min_dev[P], cand_dev[8P], the qs_score_overflow list, the swap flags of a degree-2 root --
compared with an independent numpy computation of the same thing, for every kernel route, table shape and rank range.

Final scores hide most of this (LQ-IC and EQP-IC are minima over many node pairs, QP-IC reads adjacent pairs only), and the
bundle and scan kernels share their classification, so neither the oracle tests nor kernel-against-kernel tests see a quartet
filed under the wrong node pair, a wrong q2 / q3 order in a non-adjacent pair or a candidate set with garbage beside the winner.

Asserted per case (check()): all sums exactly; every minimum within 5e-13 of the exact one and the "no quartet" sentinel
exactly where the model has it; must <= device candidates <= may per node pair, swap flags included; qs_score_finish on the
device's outputs bit-identical to the host-only finish of the model's sums and exact minimisers. The two margins are derived
in score_model.py's docstring from the tolerance of pass 2; nothing is tuned against the kernel's output.

Every tuple's sum stays below 2^32: beyond that scan_qic clamps the sum and only promises an ordering (not covered here).
tests/test_score_model.py asserts that these inputs contain the ties, overflows, flagged minimisers and cut node pairs that
the cases below rely on.
Run on the GPU box: python -m pytest tests/test_gpu_score_passes.py -m gpu
"""
import functools

import numpy as np
import pytest

import score_model as sm
from quartetscores_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    from quartetscores_amd import engine
    return engine


table = functools.lru_cache(maxsize=None)(sm.table)


@functools.lru_cache(maxsize=None)
def model(refname, kind, r_lo=0, cnt=None, tol_exp=12):
    """the model's passes over ranks [r_lo, r_lo + cnt) of a named table under a named reference: computed once, never changed"""
    _, M = sm.ref_case(refname)
    T, _ = table(kind, M.n)
    cnt = len(T) - r_lo if cnt is None else cnt
    return M.passes(T[r_lo:r_lo + cnt], r_lo, margins=(sm.may_margin(tol_exp),))


def cells(T, bits):
    return np.ascontiguousarray(T.astype(np.uint16 if bits == 16 else np.uint32))


def context(eng, refname, kind, tuning=(), bits=None, d_lo=0, d_hi=0):
    """a context that holds the named table (or its shard of largest ids [d_lo, d_hi))"""
    _, M = sm.ref_case(refname)
    T, tbits = table(kind, M.n)
    bits = bits or tbits
    ctx = eng.Context(M.n, bits, d_lo=d_lo, d_hi=d_hi)
    for k, v in tuning:
        ctx.set_tuning(k, v)
    ctx.table_alloc()
    r0, r1 = (sm.n_quartets(d_lo), sm.n_quartets(d_hi)) if d_hi else (0, len(T))
    ctx.table_upload(cells(T[r0:r1], bits))
    return ctx


def view_tensor(T, bits, r_lo, cnt):
    """tuples [r_lo, r_lo + cnt) as a device tensor of 32-bit words (padded to whole words)"""
    import torch
    raw = cells(T[r_lo:r_lo + cnt], bits).reshape(-1).view(np.uint8)
    buf = np.zeros(len(raw) + (-len(raw)) % 4, dtype=np.uint8)
    buf[:len(raw)] = raw
    return torch.from_numpy(buf).cuda().view(torch.int32)


class Dev:
    pass


def pass1(ctx, ref, P):
    import torch
    sums = torch.empty(3 * P, dtype=torch.int64, device="cuda")
    mins = torch.empty(P, dtype=torch.int64, device="cuda")
    ctx.score_pass1(ref, sums, mins)
    return sums, mins


def pass2(ctx, ref, P, mins):
    """-> (cand int64[8P], overflow list (k, 4), last_score_log())"""
    import torch
    cand = torch.empty(8 * P, dtype=torch.int64, device="cuda")
    ctx.score_pass2(ref, mins, cand)
    logged = ctx.last_score_log()
    extra = ctx.score_overflow(ref, mins, cand)
    return cand.cpu().numpy(), extra, logged


def run(ctx, ref, P):
    d = Dev()
    sums, mins = pass1(ctx, ref, P)
    d.cand, d.extra, d.logged = pass2(ctx, ref, P, mins)
    d.sums, d.mins = sums.cpu().numpy(), mins.cpu().numpy()
    return d


def check_sums_and_minima(d, want, what):
    assert np.array_equal(d.sums, want.sums), (what, "sums", np.flatnonzero(d.sums != want.sums)[:8])
    empty = want.mins == sm.KSORT_MAX
    assert np.array_equal(d.mins == sm.KSORT_MAX, empty), (what, "sentinel")
    err = np.abs(sm.sortable_to_f64(d.mins[~empty]) - want.exact_min[~empty])
    print(what, "max |device minimum - exact minimum| = %.3g over %d node pairs" % (err.max() if len(err) else 0.0, len(err)))
    assert (err <= sm.MIN_MARGIN).all(), (what, "minima", float(err.max()))


def check_candidates(got, marked, listed, want, margin, what):
    must, may = want.must, want.sets(margin)
    assert listed <= marked, (what, "list rows of unmarked node pairs", sorted(listed - marked)[:8])
    assert set(must) <= set(got) <= set(may), (what, "node pairs with candidates")
    for key in got:
        assert must[key] <= got[key], (what, key, "misses", sorted(must[key] - got[key])[:4])
        assert got[key] <= may[key], (what, key, "beyond the tolerance", sorted(got[key] - may[key])[:4])


def check(eng, ctx, ref, d, want, what, tol_exp=12):
    check_sums_and_minima(d, want, what)
    got, marked = sm.decode_candidates(d.cand, d.extra, want.P)
    listed = set((np.asarray(d.extra, dtype=np.int64).reshape(-1, 4)[:, 0] & 0xFFFFFFFF).tolist())
    check_candidates(got, marked, listed, want, sm.may_margin(tol_exp), what)
    mine = ctx.score_finish(ref, d.sums, d.cand[None, :], extra=d.extra)
    cand, extra = sm.encode_candidates(want.must, want.P)
    theirs = eng.score_finish_host(ref, want.sums, cand, extra=extra)
    assert mine[3] == theirs[3]
    for name, u, v in zip(("LQ-IC", "QP-IC", "EQP-IC"), mine[:3], theirs[:3]):
        assert np.array_equal(u.view(np.int64), v.view(np.int64)), (what, name)
    return got, marked


# ---- reference trees ----

@pytest.mark.parametrize("refname", sorted(sm.REFERENCES))
def test_every_reference_shape(eng, refname):
    """Random, caterpillar (lca(a,b) changes with every a), balanced (long runs), multifurcating (frame 1, with and without a
    large polytomy), rooted with 1, n/2 and n-1 taxa under the root's first child (both ends of root_split), 70 taxa (35 full
    bundles of 64 rows plus a partial one for the second id 1, more than 8192 ranks per workgroup round) and 9 taxa (less than
    one bundle, less than one scan chunk): random and tie-heavy 16-bit tables through both kernels."""
    ref, M = sm.ref_case(refname)
    for kind in ("multi", "ties"):
        for kernel in (0, 1):
            ctx = context(eng, refname, kind, tuning=((_lib.QS_TUNE_SCORE_KERNEL, kernel),))
            check(eng, ctx, ref, run(ctx, ref, M.P), model(refname, kind), (refname, kind, kernel))
            ctx.close()


# ---- tables ----

@pytest.mark.parametrize("refname", ["random24", "rooted12"])
@pytest.mark.parametrize("kind,tuning", [
    pytest.param("lds_edge", (), id="lds_edge"), pytest.param("u16_max", (), id="u16_max"), pytest.param("u32_big", (), id="u32_big"),
    pytest.param("wide", (), id="wide"), pytest.param("zero", (), id="zero"),
    pytest.param("overflow", ((_lib.QS_TUNE_SCORE_CAND_SLOTS, 1),), id="overflow_1slot"),
    pytest.param("overflow", ((_lib.QS_TUNE_SCORE_CAND_SLOTS, 8),), id="overflow_8slots"),
    pytest.param("ties", ((_lib.QS_TUNE_SCORE_CAND_SLOTS, 1),), id="ties_1slot")])
def test_every_table_shape(eng, refname, kind, tuning):
    """Sums on both sides of the LDS copy of the log table, 16-bit cells at 65 535, 32-bit counts of a few 10^8 (libm's log on
    the device), reduced triples beyond 21 bits (finished from the list), more near-minimal triples than candidate slots (1
    and 8 slots), an all-zero table -- through both kernels."""
    ref, M = sm.ref_case(refname)
    for kernel in (0, 1):
        ctx = context(eng, refname, kind, tuning=tuning + ((_lib.QS_TUNE_SCORE_KERNEL, kernel),))
        d = run(ctx, ref, M.P)
        got, marked = check(eng, ctx, ref, d, model(refname, kind), (refname, kind, kernel))
        if kind in ("overflow", "wide"):
            assert marked and len(d.extra) > 0
        if kind == "zero":
            assert not d.sums.any() and not marked
        ctx.close()


@pytest.mark.parametrize("refname", ["random24", "rooted12"])
def test_scores_do_not_depend_on_the_log_table_hint(eng, refname):
    """QS_TUNE_TABLE_TREES sizes the global log table (never below 65 536 entries); the header promises that scores do not
    depend on it: identical sums, minima within the same margin of the exact ones, with the hint at 0 and at 100."""
    ref, M = sm.ref_case(refname)
    seen = []
    for hint in (0, 100):
        ctx = context(eng, refname, "lds_edge", tuning=((_lib.QS_TUNE_TABLE_TREES, hint),))
        d = run(ctx, ref, M.P)
        check(eng, ctx, ref, d, model(refname, "lds_edge"), (refname, "hint", hint))
        seen.append(d)
        ctx.close()
    assert np.array_equal(seen[0].sums, seen[1].sums)


# ---- routes ----

SMALL_LOG = 16      # records: less than the chunk of 64 a wave reserves

ROUTES = {
    "load0": ((_lib.QS_TUNE_SCORE_KERNEL, 0), (_lib.QS_TUNE_SCORE_LOAD, 0)),
    "load1": ((_lib.QS_TUNE_SCORE_KERNEL, 0), (_lib.QS_TUNE_SCORE_LOAD, 1)),
    "load2": ((_lib.QS_TUNE_SCORE_KERNEL, 0), (_lib.QS_TUNE_SCORE_LOAD, 2)),
    "load3": ((_lib.QS_TUNE_SCORE_KERNEL, 0), (_lib.QS_TUNE_SCORE_LOAD, 3)),
    "scan": ((_lib.QS_TUNE_SCORE_KERNEL, 1),),
    "two_passes": ((_lib.QS_TUNE_SCORE_PASSES, 1),),
    "logged": ((_lib.QS_TUNE_SCORE_PASSES, 2),),
    "logged_load1": ((_lib.QS_TUNE_SCORE_PASSES, 2), (_lib.QS_TUNE_SCORE_LOAD, 1)),
    "log_overflows": ((_lib.QS_TUNE_SCORE_PASSES, 2), (_lib.QS_TUNE_SCORE_LOG_CAP, SMALL_LOG)),
    "tol12": ((_lib.QS_TUNE_SCORE_TOL_EXP, 12),),
    "tol2": ((_lib.QS_TUNE_SCORE_TOL_EXP, 2),),
    "tol2_scan": ((_lib.QS_TUNE_SCORE_TOL_EXP, 2), (_lib.QS_TUNE_SCORE_KERNEL, 1)),
    "tol2_logged": ((_lib.QS_TUNE_SCORE_TOL_EXP, 2), (_lib.QS_TUNE_SCORE_PASSES, 2)),
}


@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("refname", ["random24", "rooted12", "random70"])
def test_every_route(eng, refname, route):
    """The bundle kernel with each of its four load modes, the scan kernel, two passes, the single-read pass whose pass 2 filters
    the candidate log (last_score_log() > 0), a log forced to overflow so that pass 2 reads the table after all
    (last_score_log() == 0), and a tolerance of 1e-2 (may widens to 1e-2 + 1e-12, must stays)."""
    ref, M = sm.ref_case(refname)
    tol_exp = 2 if route.startswith("tol2") else 12
    for kind in ("multi", "ties") if M.n < 70 else ("multi",):
        ctx = context(eng, refname, kind, tuning=ROUTES[route])
        d = run(ctx, ref, M.P)
        if route in ("logged", "logged_load1", "tol2_logged"):
            assert d.logged > 0, (refname, kind, route)
        else:
            assert d.logged == 0, (refname, kind, route)
        check(eng, ctx, ref, d, model(refname, kind, 0, None, tol_exp), (refname, kind, route), tol_exp)
        ctx.close()


# ---- rank ranges ----

@pytest.mark.parametrize("shard", ["0-5", "4-5", "5-last", "last"])
@pytest.mark.parametrize("refname", ["random24", "rooted12"])
def test_table_shards(eng, refname, shard):
    """Contexts that own the tuples whose largest id lies in [d_lo, d_hi): five tuples, four tuples that do not start at rank
    0, nearly everything, the last id alone -- each against the model on the same ranks (the sums of a degree-2 root's node
    pairs included: every shard adds its part)."""
    ref, M = sm.ref_case(refname)
    n = M.n
    d_lo, d_hi = {"0-5": (0, 5), "4-5": (4, 5), "5-last": (5, n - 1), "last": (n - 1, n)}[shard]
    r0, r1 = sm.n_quartets(d_lo), sm.n_quartets(d_hi)
    for kind, route in (("multi", "load0"), ("ties", "scan"), ("multi", "logged")):
        ctx = context(eng, refname, kind, tuning=ROUTES[route], d_lo=d_lo, d_hi=d_hi)
        check(eng, ctx, ref, run(ctx, ref, M.P), model(refname, kind, r0, r1 - r0), (refname, shard, kind, route))
        ctx.close()


@pytest.mark.parametrize("refname,bits", [("random24", 16), ("random24", 32), ("rooted12", 16), ("multif41", 16), ("random70", 16),
                                          ("random9", 32)])
def test_ragged_views(eng, refname, bits):
    """Views through qs_score_set_view as the reduce-scattered shards of the tree-sharded multi-GPU path are: starting and
    ending inside a row, inside one row, one tuple at rank 0 and one mid-table, the last five tuples, (7, 8192 + 9) -- the
    bundle kernel's plan (whole rows per second id + partial rows through the scan kernel) and the scan kernel alone."""
    ref, M = sm.ref_case(refname)
    T, _ = table("multi", M.n)
    ctx = context(eng, refname, "multi", bits=bits)
    for r_lo, cnt in sm.ragged_views(M.n, bits):
        view = view_tensor(T, bits, r_lo, cnt)
        ctx.score_set_view(view, bits, r_lo, cnt)
        for kernel in (0, 1):
            ctx.set_tuning(_lib.QS_TUNE_SCORE_KERNEL, kernel)
            check(eng, ctx, ref, run(ctx, ref, M.P), model(refname, "multi", r_lo, cnt), (refname, bits, r_lo, cnt, kernel))
    ctx.score_set_view(None, 0, 0, 0)
    ctx.close()


@pytest.mark.parametrize("refname,kind", [("random24", "multi"), ("random24", "ties"), ("rooted12", "ties"), ("random70", "multi")])
def test_views_that_partition_the_table(eng, refname, kind):
    """What distributed.score_sharded relies on: over views that split the table, the element-wise SUM of the sums and MIN of
    the minima are the whole table's, and the union of the candidates every view finds against the REDUCED minima holds the
    whole table's exact minimisers and nothing beyond its tolerance."""
    import torch
    ref, M = sm.ref_case(refname)
    T, bits = table(kind, M.n)
    whole = model(refname, kind)
    ctx = context(eng, refname, kind)
    views = [(r_lo, cnt, view_tensor(T, bits, r_lo, cnt)) for r_lo, cnt in sm.partition(M.n, bits)]
    sums = mins = None
    for r_lo, cnt, view in views:
        ctx.score_set_view(view, bits, r_lo, cnt)
        s_, m_ = pass1(ctx, ref, M.P)
        part = Dev()
        part.sums, part.mins = s_.cpu().numpy(), m_.cpu().numpy()
        check_sums_and_minima(part, model(refname, kind, r_lo, cnt), (refname, kind, r_lo, cnt))
        sums = s_ if sums is None else sums + s_                    # all_reduce(SUM)
        mins = m_ if mins is None else torch.minimum(mins, m_)      # all_reduce(MIN)
    total = Dev()
    total.sums, total.mins = sums.cpu().numpy(), mins.cpu().numpy()
    check_sums_and_minima(total, whole, (refname, kind, "reduced"))
    union, marked, listed, cands, extras = {}, set(), set(), [], []
    for r_lo, cnt, view in views:
        ctx.score_set_view(view, bits, r_lo, cnt)
        cand, extra, _ = pass2(ctx, ref, M.P, mins)
        got, mk = sm.decode_candidates(cand, extra, M.P)
        for key, members in got.items():
            union.setdefault(key, set()).update(members)
        marked |= mk
        listed |= set((np.asarray(extra, dtype=np.int64).reshape(-1, 4)[:, 0] & 0xFFFFFFFF).tolist())
        cands.append(cand)
        extras.append(np.asarray(extra, dtype=np.int64).reshape(-1, 4))
    check_candidates(union, marked, listed, whole, sm.MAY_MARGIN, (refname, kind, "union"))
    mine = ctx.score_finish(ref, total.sums, np.stack(cands), extra=np.concatenate(extras))     # all_gather
    enc = sm.encode_candidates(whole.must, M.P)
    theirs = eng.score_finish_host(ref, whole.sums, enc[0], extra=enc[1])
    for u, v in zip(mine[:3], theirs[:3]):
        assert np.array_equal(u.view(np.int64), v.view(np.int64))
    ctx.score_set_view(None, 0, 0, 0)
    ctx.close()


# ---- a candidate log that no longer describes the state ----

LOGGED = ((_lib.QS_TUNE_SCORE_PASSES, 2),)
SAME_TUNING = [(_lib.QS_TUNE_SCORE_CAND_SLOTS, 8), (_lib.QS_TUNE_SCORE_TOL_EXP, 12), (_lib.QS_TUNE_SCORE_KERNEL, 0), (_lib.QS_TUNE_TABLE_TREES, 0),
               (_lib.QS_TUNE_SCORE_PASSES, 2), (_lib.QS_TUNE_SCORE_LOG_CAP, 0), (_lib.QS_TUNE_SCORE_DEDUPE, 1), (_lib.QS_TUNE_SCORE_LOAD, 0),
               (_lib.QS_TUNE_PANEL_KERNEL, 0)]


def candidates_of(ctx, ref, M, mins, want, what):
    cand, extra, logged = pass2(ctx, ref, M.P, mins)
    got, marked = sm.decode_candidates(cand, extra, M.P)
    listed = set((np.asarray(extra, dtype=np.int64).reshape(-1, 4)[:, 0] & 0xFFFFFFFF).tolist())
    check_candidates(got, marked, listed, want, sm.MAY_MARGIN, what)
    return logged


@pytest.mark.parametrize("refname", ["random24", "rooted12"])
def test_stale_candidate_log_is_not_used(eng, refname):
    """After a pass 1 that logged its candidates, a new table, another view or any qs_set_tuning between pass 1 and pass 2
    makes pass 2 read the table: last_score_log() == 0, and the candidates are the ones of the state pass 2 runs in (per the
    model, with that state's own minima), not the logged ones."""
    ref, M = sm.ref_case(refname)
    T, bits = table("multi", M.n)
    T2 = table("ties", M.n)[0]
    nq = len(T)
    r_lo, cnt = sm.ragged_views(M.n, bits)[0]
    view = view_tensor(T, bits, r_lo, cnt)
    ctx = context(eng, refname, "multi", tuning=LOGGED)
    # the minima of the two other states, by passes of their own
    ctx.table_upload(cells(T2, bits))
    _, mins_t2 = pass1(ctx, ref, M.P)
    ctx.table_upload(cells(T, bits))
    ctx.score_set_view(view, bits, r_lo, cnt)
    _, mins_view = pass1(ctx, ref, M.P)
    ctx.score_set_view(None, 0, 0, 0)
    # control: nothing in between -> pass 2 filters the log
    _, mins = pass1(ctx, ref, M.P)
    assert candidates_of(ctx, ref, M, mins, model(refname, "multi"), "control") > 0
    # a second pass 2 finds the log spent
    assert candidates_of(ctx, ref, M, mins, model(refname, "multi"), "spent") == 0
    # another table
    keep = pass1(ctx, ref, M.P)
    ctx.table_upload(cells(T2, bits))
    assert candidates_of(ctx, ref, M, mins_t2, model(refname, "ties"), "upload") == 0
    ctx.table_upload(cells(T, bits))
    # another view
    keep = pass1(ctx, ref, M.P)
    ctx.score_set_view(view, bits, r_lo, cnt)
    assert candidates_of(ctx, ref, M, mins_view, model(refname, "multi", r_lo, cnt), "view") == 0
    ctx.score_set_view(None, 0, 0, 0)
    # any tuning call, also one that changes nothing
    for key, value in SAME_TUNING:
        _, mins = pass1(ctx, ref, M.P)
        ctx.set_tuning(key, value)
        assert candidates_of(ctx, ref, M, mins, model(refname, "multi"), ("tuning", key)) == 0
    # ... and the log works again afterwards
    _, mins = pass1(ctx, ref, M.P)
    assert candidates_of(ctx, ref, M, mins, model(refname, "multi"), "again") > 0
    assert nq == ctx.table_tuples and keep is not None
    ctx.close()
