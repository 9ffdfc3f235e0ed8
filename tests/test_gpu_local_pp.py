"""qs_branch_frequencies / Context.branch_frequencies: per node the number of trees that resolve a 4-set around its internode and the
fixed-point sums of their normalised frequencies, equal to the big-integer model (tests/local_pp_model.py) on synthetic rows at every
edge of the kernel's tiling and at the largest S, on real rows of qs_tree_branch_support, and independent of batching and repetition."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import local_pp_model as LM
from quartetscores_amd import _lib, flatten, synth
from tree_branch_model import mixed_trees

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = LM.ONE
S_MAX = math.comb(4096, 4)


def kernel_constant(name):
    with open(os.path.join(ROOT, "quartetscores_amd", "csrc", "qs_tree_branch.hip")) as f:
        return int(re.search(r"\b%s = (\d+)" % name, f.read()).group(1))


CHUNK, BLOCK = kernel_constant("kFreqTrees"), kernel_constant("kFreqNodes")


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    from quartetscores_amd import engine
    return engine


@pytest.fixture(scope="module")
def ctx(eng):
    return eng.Context(24)


def model(rows):
    return np.array(LM.frequencies(rows.tolist()), dtype=np.int64).reshape(rows.shape[1], 4)


def synthetic(rng, m, n_nodes):
    """random words, many rows all zero, some with present > 0 and S = 0, some at the largest S"""
    rows = np.zeros((m, n_nodes, 4), dtype=np.int64)
    kind = rng.integers(0, 6, size=(m, n_nodes))
    small = rng.integers(0, 50, size=(m, n_nodes, 3))
    big = rng.integers(0, S_MAX // 3, size=(m, n_nodes, 3))
    rows[..., 1:] = np.where((kind == 1)[..., None], small, np.where((kind == 2)[..., None], big, 0))
    rows[..., 0] = np.where(kind >= 1, rows[..., 1:].sum(-1) + rng.integers(0, 9, size=(m, n_nodes)), 0)
    return rows


def test_tiling_constants():
    assert BLOCK == 64 and CHUNK >= 2    # the node counts below (63, 65, 300) sit around one block and span several


@pytest.mark.parametrize("n_nodes", [1, 63, 65, 300])
def test_synthetic_rows_equal_the_model(eng, ctx, n_nodes):
    rng = np.random.default_rng(n_nodes)
    for m in (1, CHUNK - 1, CHUNK, CHUNK + 1, 600):
        rows = synthetic(rng, m, n_nodes)
        got = ctx.branch_frequencies(rows)
        assert got.shape == (n_nodes, 4) and got.dtype == np.int64
        want = model(rows)
        assert (got == want).all(), (m, n_nodes, np.nonzero((got != want).any(1))[0][:5])
        assert (got[:, 0] == ((rows[:, :, 1:].sum(2)) > 0).sum(0)).all()


def test_exact_division_at_the_limits(eng, ctx):
    third = S_MAX // 3
    rows = np.array([[[3, 1, 1, 1], [S_MAX, S_MAX - 1, 1, 0], [S_MAX, third, third, S_MAX - 2 * third], [S_MAX, S_MAX, 0, 0], [S_MAX, 0, 0, S_MAX],
                      [5, 0, 0, 0], [1, 0, 1, 0], [S_MAX, 1, S_MAX - 2, 1]]], dtype=np.int64)
    got = ctx.branch_frequencies(rows)
    assert got[0].tolist() == [1] + [ONE // 3] * 3
    assert got[1].tolist() == [1, (S_MAX - 1) * ONE // S_MAX, ONE // S_MAX, 0]
    assert got[2].tolist() == [1, third * ONE // S_MAX, third * ONE // S_MAX, (S_MAX - 2 * third) * ONE // S_MAX]
    assert got[3].tolist() == [1, ONE, 0, 0] and got[4].tolist() == [1, 0, 0, ONE] and got[5].tolist() == [0, 0, 0, 0]
    assert (got == model(rows)).all()
    # quotients that sit on or beside a multiple of S: q x 2^40 = k x S + r with r = 0, 1, S - 1 wherever such q exists
    rng = np.random.default_rng(3)
    cells = []
    for _ in range(3000):
        s = int(rng.integers(1, S_MAX + 1))
        q = (int(rng.integers(0, ONE + 1)) * s >> 40) + int(rng.integers(0, 2))
        q = min(q, s)
        rest = s - q
        other = int(rng.integers(0, rest + 1))
        cells.append([s, q, other, rest - other])
    rows = np.array(cells, dtype=np.int64).reshape(10, 300, 4)
    assert (ctx.branch_frequencies(rows) == model(rows)).all()


def test_streaming_and_repetition(eng, ctx):
    import torch
    rng = np.random.default_rng(8)
    rows = synthetic(rng, 150, 70)
    whole = ctx.branch_frequencies(rows)
    assert whole.any() and (whole == model(rows)).all()
    half = ctx.branch_frequencies(rows[:75])
    assert (ctx.branch_frequencies(rows[75:], out=half) == whole).all()
    assert (ctx.branch_frequencies(rows, out=whole) == 2 * whole).all()
    on_device = torch.from_numpy(rows).to(f"cuda:{ctx.device}")
    assert (ctx.branch_frequencies(on_device) == whole).all()
    assert not ctx.branch_frequencies(np.zeros((0, 70, 4), dtype=np.int64)).any()
    assert ctx.branch_frequencies(np.zeros((3, 0, 4), dtype=np.int64)).shape == (0, 4)
    with pytest.raises(ValueError):
        ctx.branch_frequencies(np.zeros((3, 4), dtype=np.int64))


@pytest.mark.parametrize("n,kind", [(12, "binary"), (12, "mixed"), (24, "binary"), (24, "mixed"), (70, "mixed")])
def test_real_rows(eng, n, kind):
    """rows of qs_tree_branch_support: binary complete trees, and trees with 20 % of the edges collapsed and 10 % of the taxa dropped
    beside the mixed shapes; 70 taxa have more than one block of tree nodes there"""
    rng = np.random.default_rng(n + len(kind))
    ref = flatten.flatten_reference(synth.random_tree(n, rng))
    if kind == "binary":
        trees = [synth.random_tree(n, rng) for _ in range(40)]
    else:
        trees = [synth.random_tree(n, rng, collapse=0.2, dropout=0.1) for _ in range(28)] + mixed_trees(n, rng, 12)
    c = eng.Context(n)
    b = flatten.flatten_eval_trees(trees, ref.name_to_id)
    hb = c.batch_upload(b)
    rows = c.tree_branch_support(ref, hb)
    c.batch_free(hb)
    assert rows[:, :, 1:].any()
    got = c.branch_frequencies(rows)
    assert (got == model(rows)).all()
    en = (rows[:, :, 1:].sum(2) > 0).sum(0)
    assert (got[:, 0] == en).all() and en.max() > 0
    if kind == "binary":
        inner = en > 0
        assert (en[inner] == len(trees)).all()
        total = got[:, 1:].sum(1)
        assert (total[inner] <= en[inner] * ONE).all() and (total[inner] >= en[inner] * ONE - 3 * en[inner]).all()
    # the same trees in two batches of other sizes, each through its own tree_branch_support
    parts = None
    for lo, hi in ((0, 7), (7, len(trees))):
        hb = c.batch_upload(flatten.flatten_eval_trees(trees[lo:hi], ref.name_to_id))
        parts = c.branch_frequencies(c.tree_branch_support(ref, hb), out=parts)
        c.batch_free(hb)
    assert (parts == got).all()


def test_error_codes(eng, ctx):
    import torch
    buf = torch.zeros(5 * 6 * 4 + 1, dtype=torch.int64, device=f"cuda:{ctx.device}")
    dst = torch.zeros(6 * 4 + 1, dtype=torch.int64, device=f"cuda:{ctx.device}")
    call = lambda rows, m, dst_ptr: ctx.L.qs_branch_frequencies(ctx.h, rows, m, 6, dst_ptr)
    rows_p, dst_p = C.c_void_p(buf.data_ptr()), C.c_void_p(dst.data_ptr())
    assert call(None, 5, dst_p) == _lib.QS_ERR_ARG
    assert call(rows_p, 5, None) == _lib.QS_ERR_ARG
    assert call(C.c_void_p(buf.data_ptr() + 4), 5, dst_p) == _lib.QS_ERR_ARG
    assert call(rows_p, 5, C.c_void_p(dst.data_ptr() + 4)) == _lib.QS_ERR_ARG
    assert call(rows_p, 1 << 23, dst_p) == _lib.QS_ERR_OVERFLOW      # (the check comes before anything is read)
    assert b"2^23" in ctx.L.qs_last_error(ctx.h)
    assert ctx.L.qs_branch_frequencies(None, rows_p, 5, 6, dst_p) == _lib.QS_ERR_ARG
    assert call(rows_p, 0, dst_p) == _lib.QS_OK
    assert ctx.L.qs_branch_frequencies(ctx.h, rows_p, 5, 0, dst_p) == _lib.QS_OK
    ctx.sync()
    assert not dst.cpu().numpy().any()           # a refused call wrote nothing
    # rows that are 8-byte but not 16-byte aligned are read as well
    buf[1:1 + 5 * 6 * 4] = torch.arange(5 * 6 * 4, dtype=torch.int64, device=buf.device)
    assert call(C.c_void_p(buf.data_ptr() + 8), 5, dst_p) == _lib.QS_OK
    ctx.sync()
    want = model(np.arange(5 * 6 * 4, dtype=np.int64).reshape(5, 6, 4))
    assert (dst.cpu().numpy()[:24].reshape(6, 4) == want).all()
