"""qs_fix_overlap_plan (host-only, no GPU): where a slice of the count step is split so that the depth-clamp corrections of the upper
d-range run beside the count launch of the lower one (QS_TUNE_FIX_OVERLAP)."""
import ctypes as C
from math import comb

from quartetscores_amd import _lib

CORRECTIONS = [10 ** k for k in range(3, 13)]


def plan(L, n, d_lo, d_hi, bits, corrections, groups=313, mode=0, depth_bits=4, keep=0):
    ms = (C.c_double * 2)()
    r = L.qs_fix_overlap_plan(n, d_lo, d_hi, bits, mode, depth_bits, groups, corrections, keep, ms)
    return r, ms[0], ms[1]


def test_every_size_gets_an_in_range_monotone_split_or_the_single_launch():
    """n = 8 .. 1024, whole tables and the upper half as a shard, both cell widths: no corrections = no split; with corrections the
    answer is 0 (one launch) or a d_mid inside the shard whose d-blocks are aligned to d_hi (16-bit cells: possibly moved up by 4, and
    the upper range then starts at an even cell), whose modelled lower launch covers the upper corrections one and a half times; as
    the corrections grow d_mid never falls, and once the lower launch would be too large the answer stays 0. Small tables (40 taxa
    hold 1 500 tiles, a wave population is 4 096) are never split."""
    L = _lib.load()
    split_some = 0
    for n in range(8, 1025):
        for d_lo, d_hi in ((0, n), (n // 2, n)):
            for bits in (32, 16):
                assert plan(L, n, d_lo, d_hi, bits, 0) == (0, 0.0, 0.0)
                last, ended = 0, False
                for corr in CORRECTIONS:
                    r, lo_ms, fix_ms = plan(L, n, d_lo, d_hi, bits, corr)
                    assert r >= 0
                    if r == 0:
                        ended = ended or last > 0
                        continue
                    assert not ended, (n, d_lo, bits, corr, r)                     # too large a lower launch: larger ones are too
                    assert max(d_lo, 3) < r < d_hi and r >= last, (n, d_lo, bits, corr, r, last)
                    assert (d_hi - r) % 8 == 0 or (bits == 16 and (d_hi - r) % 8 == 4), (n, d_lo, bits, corr, r)
                    if bits == 16:
                        assert (comb(r, 4) - comb(d_lo, 4)) % 2 == 0, (n, d_lo, r)
                    assert lo_ms >= 1.5 * fix_ms > 0.0
                    last = r
                    split_some += 1
                if n <= 40:
                    assert last == 0, n
    assert split_some > 1000


def test_the_headline_shape_and_the_kept_split():
    """512 taxa x 10 000 binary trees in one slice of 313 groups with the 1.41e8 corrections of the record: d_mid lies where the lower
    launch is a few per cent of the count (200 .. 230). Deeper classes and the general modes cost more per tile, so the same
    corrections are covered by a smaller lower range. A d_mid in use is kept while it fits."""
    L = _lib.load()
    r, lo_ms, fix_ms = plan(L, 512, 0, 512, 32, 141_000_000)
    assert 200 <= r <= 230 and (512 - r) % 8 == 0 and 7.0 < fix_ms < 7.6 and 1.5 * fix_ms <= lo_ms < 16.0, (r, lo_ms, fix_ms)
    assert plan(L, 512, 0, 512, 16, 141_000_000)[0] in (r, r + 4)
    assert 0 < plan(L, 512, 0, 512, 32, 141_000_000, depth_bits=7)[0] <= r
    assert 0 < plan(L, 512, 0, 512, 32, 141_000_000, mode=1)[0] <= r
    assert plan(L, 512, 0, 512, 32, 141_000_000, keep=r + 8)[0] == r + 8          # still covers, still a small launch
    assert plan(L, 512, 0, 512, 32, 141_000_000, keep=r - 40)[0] == r            # no longer covers
    assert plan(L, 512, 0, 512, 32, 141_000_000, keep=500)[0] == r               # more than 40 % of the count
    assert plan(L, 512, 500, 512, 32, 141_000_000)[0] == 0                       # a d-range too short to split
    assert plan(L, 512, 0, 512, 24, 1)[0] == _lib.QS_ERR_ARG and plan(L, 512, 0, 600, 32, 1)[0] == _lib.QS_ERR_ARG


def _tile_model(n):
    """The count kernel's tiling restated: (cost units, wave tiles) of the d-range [d_lo, d_hi) -- d-blocks of 8 counted down from
    d_hi, per third id c a tile for every pair of 16-wide a-blocks under an 8-wide b-block plus the diagonal pairs, a tile priced at
    4 + the d slots it serves (those above c)."""
    def tiles_for_c(c):
        t = (c + 7) // 8
        return t * t // 4 + (t + 1) // 2

    def cost(d_lo, d_hi):
        d_lo, tot, cnt, d1 = max(d_lo, 3), 0, 0, d_hi
        while d1 > d_lo:
            d0 = d1 - 8 if d1 > d_lo + 8 else d_lo
            for c in range(2, d1 - 1):
                live = (d1 - d0) if c < d0 else d1 - 1 - c
                tot += tiles_for_c(c) * (4 + live)
                cnt += tiles_for_c(c)
            d1 = d0
        return tot, cnt
    return cost


def test_the_chosen_split_against_a_tile_model_of_its_own():
    """The planner's answer checked with a Python restatement of the tiling instead of its own model_ms: at the chosen d_mid the
    lower launch (rate: 284.8 ms for the whole 512-taxon table x 313 groups at 4 bits) covers 1.5 times the upper corrections (their
    share of the tuples at 1.9e10 per second + 0.05 ms of launch), holds 4096 tiles and stays below 40 % of the count; one d-block
    lower it does not cover them."""
    L = _lib.load()
    unit_ms = 284.8 / (_tile_model(512)(0, 512)[0] * 313)
    for n, d_lo, groups, corr in ((512, 0, 313, 141_000_000), (512, 0, 100, 60_000_000), (300, 0, 64, 4_000_000), (156, 0, 32, 80_000),
                                  (1024, 700, 157, 400_000_000), (204, 0, 16, 80_000)):
        cost = _tile_model(n)
        r, lo_ms, fix_ms = plan(L, n, d_lo, n, 32, corr, groups=groups)
        assert r > 0, (n, groups, corr)

        def fix(d_mid):
            return corr * (comb(n, 4) - comb(d_mid, 4)) / comb(n, 4) / 1.9e7 + 0.05
        units, tiles = cost(d_lo, r)
        assert abs(units * unit_ms * groups - lo_ms) < 1e-6 * lo_ms and abs(fix(r) - fix_ms) < 1e-9
        assert units * unit_ms * groups >= 1.5 * fix(r) and tiles >= 4096 and units <= 0.4 * cost(d_lo, n)[0]
        assert cost(d_lo, r - 8)[0] * unit_ms * groups < 1.5 * fix(r - 8), (n, r)
