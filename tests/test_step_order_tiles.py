"""The shapes tests/test_gpu_step_order.py counts at hold every instance of the count kernel's 32-tree step: the arithmetic of
bs3_decode_tile / bs3_tile_variant (qs_bitslice3.hpp) restated on the host. No GPU."""


def tile_instances(d_lo, d_hi):
    """The step instances (0: both a-columns, all eight d slots live; 1: both a-columns, cut d-block; 2: one a-block; 3: diagonal) the
    tiling of the shard [d_lo, d_hi) holds, and the width of its narrowest d-block. d-blocks are aligned to the top of the shard."""
    seen, narrowest = set(), 8
    d1 = d_hi
    while d1 > d_lo:
        d0 = d1 - 8 if d1 > d_lo + 8 else d_lo
        narrowest = min(narrowest, d1 - d0)
        for c in range(2, d1 - 1):
            jlo, jhi = (c + 1 - d0 if c >= d0 else 0), d1 - d0
            full = jlo == 0 and jhi == 8
            T = (c + 7) // 8                                     # 8-blocks of ids below c (at least one)
            for tl in range((T * T) // 4):                       # off-diagonal tiles: b-block Bk, a-blocks 2j and 2j + 1
                Bk = max(k for k in range(1, T + 1) if (k * k) // 4 <= tl)
                j = tl - (Bk * Bk) // 4
                has_a2 = 2 * j + 1 < Bk
                seen.add((0 if full else 1) if has_a2 else 2)
            seen.add(3)                                          # (T + 1) // 2 >= 1 pairs of diagonal blocks
        d1 = d0
    return seen, narrowest


def test_forty_taxa_hold_every_instance_of_the_step():
    seen, narrowest = tile_instances(0, 40)
    assert seen == {0, 1, 2, 3} and narrowest == 8
    seen, narrowest = tile_instances(13, 38)      # the shard of test_late_through_a_shard_with_a_narrow_d_block
    assert seen == {0, 1, 2, 3} and narrowest < 8


def test_the_in_step_shard_holds_every_instance():
    seen, narrowest = tile_instances(196, 204)    # the shard of test_late_with_the_waves_of_a_workgroup_in_step
    assert seen == {0, 1, 2, 3} and narrowest == 8
