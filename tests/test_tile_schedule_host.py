"""The plain reference of the passes' tile schedule (tests/tile_schedule_reference.py) checked on its own, so that the GPU
comparison (tests/test_gpu_tile_schedule.py) cannot pass against a reference that is wrong: over the shapes and cost maps
of the GPU test and every width of 1..140 tile columns it keeps the invariants a schedule needs for every pixel to be
rendered exactly once, and it reproduces hand-worked cuts and sweeps. No GPU, no library."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import tile_schedule_reference as ref  # noqa: E402


def check_case(costs, tiles_x, tiles_y):
    w, h = ref.extent(tiles_x, tiles_y)
    assert ref.tiles(w, h) == (tiles_x, tiles_y)
    cap = ref.order_cap(w, h)
    lists = ref.order(costs, tiles_x, tiles_y)
    b = ref.check_invariants(lists, cap, tiles_x, tiles_y)
    assert b == ref.bands(costs, tiles_x, tiles_y)
    return b


@pytest.mark.parametrize("tiles_x,tiles_y", ref.SHAPES)
def test_reference_keeps_invariants_at_gpu_test_shapes(tiles_x, tiles_y):
    for name, costs in ref.cost_maps(tiles_x, tiles_y):
        check_case(costs, tiles_x, tiles_y)


@pytest.mark.parametrize("tiles_y", [1, 3, 6])
def test_reference_keeps_invariants_at_every_width(tiles_y):
    for tiles_x in range(1, 141):
        for name, costs in ref.cost_maps(tiles_x, tiles_y):
            check_case(costs, tiles_x, tiles_y)


def test_order_cap_and_cap_cols_by_hand():
    assert [ref.cap_cols(t) for t in (1, 7, 8, 15, 16, 17, 125, 1024)] == [1, 3, 3, 4, 5, 5, 25, 194]
    # (pixels wide, pixels high) -> widest band x tile rows; beyond 1024 columns the equal share is still narrower than the cap
    assert ref.order_cap(1, 1) == 1 and ref.order_cap(8 * 7 - 6, 8 * 3 - 7) == 3 * 3 and ref.order_cap(1000, 9) == 25 * 2
    assert ref.order_cap(130, 17) == 5 * 3 and ref.order_cap(8 * 1025, 16) == 194 * 2
    for tiles_x in range(1, 2000):
        assert ref.order_cap(8 * tiles_x, 8) >= (tiles_x + 7) // 8         # equal-width bands always fit


def test_equal_width_bands_outside_the_balanced_range():
    hot = np.zeros((3, 15), dtype=np.uint32); hot[:, 0] = ref.NONE
    assert ref.bands(hot, 15, 3) == [15 * i // 8 for i in range(9)]           # costs ignored under 16 columns
    hot = np.zeros((2, 1025), dtype=np.uint32); hot[:, 0] = ref.NONE
    assert ref.bands(hot, 1025, 2) == [1025 * i // 8 for i in range(9)]       # ... and beyond 1024
    assert ref.widths(ref.bands(np.zeros(7 * 3), 7, 3)) == [0, 1, 1, 1, 1, 1, 1, 1]


def test_cuts_by_hand():
    """Cuts worked out on paper: everything in one column pushes the bands beside it to one column each (every band gets a
    column) and the others to cap_cols (the bands left must cover the rest)."""
    maps = dict(ref.cost_maps(125, 3))
    assert ref.widths(ref.bands(maps["col0"], 125, 3)) == [1, 1, 1, 22, 25, 25, 25, 25]
    assert ref.widths(ref.bands(maps["colMid"], 125, 3)) == [25, 25, 12, 1, 1, 11, 25, 25]
    assert ref.widths(ref.bands(dict(ref.cost_maps(17, 3))["colLast"], 17, 3)) == [5, 5, 2, 1, 1, 1, 1, 1]
    # an unmeasured image: every column weighs 1, an eighth of 125 is 15 (rounded down before it is multiplied): 7 x 15 + 20
    assert ref.widths(ref.bands(maps["zero"], 125, 3)) == [15] * 7 + [20]
    # two columns of equal weight 10 (+1) at 3 and 12 of 16, nothing else (+1 each): total 36, ideal cuts at multiples of 4
    c = np.zeros((1, 16), dtype=np.uint32); c[0, 3] = c[0, 12] = 10
    # centres: columns 0,1,2 at 0,1,2 (halves round down); column 3 spans 3..14, centre 8; 4..11 at 14..21; 12 spans 22..33,
    # centre 27; 13,14,15 at 33,34,35. Ideal cuts 4, 8, 12, .., 28 -> first column whose centre reaches them: 3, 3, 4, 6, 10, 12, 13;
    # a cut moves on by a column at least: 3, 4, 5, 6, 10, 12, 13
    assert ref.bands(c, 16, 1) == [0, 3, 4, 5, 6, 10, 12, 13, 16]


@pytest.mark.parametrize("tiles_x,tiles_y", ref.CLAMP_SHAPES)
def test_one_column_maps_reach_the_clamps(tiles_x, tiles_y):
    maps = dict(ref.cost_maps(tiles_x, tiles_y))
    for name in ref.CLAMP_MAPS:
        w = ref.widths(ref.bands(maps[name], tiles_x, tiles_y))
        assert max(w) == ref.cap_cols(tiles_x) and min(w) == 1, (name, w)


def rows_of(lists, band, tiles_x, tiles_y):
    lst = lists[band][lists[band] != ref.NONE].astype(np.int64)
    return (lst // tiles_x).reshape(tiles_y, -1)[:, 0].tolist()


def test_sweeps_by_hand():
    tiles_x, tiles_y = 17, 9
    maps = dict(ref.cost_maps(tiles_x, tiles_y))
    # one expensive tile in row 0 of column 8: its band is walked top-down (head > tail), from 4 rows beyond the peak back to
    # the top, then the rest downwards; a band without costs has its peak in row 0 too
    lists = ref.order(maps["tileRow0"], tiles_x, tiles_y)
    for band in range(8):
        assert rows_of(lists, band, tiles_x, tiles_y) == [4, 3, 2, 1, 0, 5, 6, 7, 8]
    # only the last row costs: bottom-up, from 4 rows above the peak to the bottom, then the rest upwards
    lists = ref.order(maps["lastRow"], tiles_x, tiles_y)
    for band in range(8):
        assert rows_of(lists, band, tiles_x, tiles_y) == [4, 5, 6, 7, 8, 3, 2, 1, 0]
    # the single tile in the middle row (4) of the last column: head == tail, top-down, start clamped to the last row
    lists = ref.order(maps["tileRowMid"], tiles_x, tiles_y)
    assert rows_of(lists, 7, tiles_x, tiles_y) == [8, 7, 6, 5, 4, 3, 2, 1, 0]
    assert rows_of(lists, 0, tiles_x, tiles_y) == [4, 3, 2, 1, 0, 5, 6, 7, 8]
    # bottom-up with the peak within 4 rows of the top: start clamped to row 0, one run
    c = np.zeros((9, 17), dtype=np.uint32); c[8, :] = 5; c[2, :] = 6
    assert rows_of(ref.order(c, 17, 9), 3, 17, 9) == list(range(9))
    # taller than 1024 rows: end to end from the expensive end
    maps = dict(ref.cost_maps(17, 1025))
    assert rows_of(ref.order(maps["lastRow"], 17, 1025), 0, 17, 1025) == list(range(1024, -1, -1))
    assert rows_of(ref.order(maps["tileRowMid"], 17, 1025), 7, 17, 1025) == list(range(1025))
    # 1024 rows still start beyond the peak (row 512 of the last band)
    maps = dict(ref.cost_maps(17, 1024))
    assert rows_of(ref.order(maps["tileRowMid"], 17, 1024), 7, 17, 1024) == list(range(516, -1, -1)) + list(range(517, 1024))


def test_monotone_runs():
    assert ref.monotone_runs([]) == 0 and ref.monotone_runs([5]) == 1 and ref.monotone_runs([0, 1, 2]) == 1 and ref.monotone_runs([2, 1, 0]) == 1
    assert ref.monotone_runs([2, 1, 0, 3, 4]) == 2 and ref.monotone_runs([3, 4, 0, 1, 2]) == 2 and ref.monotone_runs([1, 0, 3, 2]) == 2
    assert ref.monotone_runs([0, 2, 1, 3, 5, 4]) == 3 and ref.monotone_runs([1, 0, 2, 4, 3]) == 3


def test_invariant_checker_rejects_broken_schedules():
    """The checker itself: a dropped tile, a tile listed twice, a hole in the padding, a band the launch is not sized for,
    swapped columns and a third sweep are each named."""
    tiles_x, tiles_y = 17, 5
    w, h = ref.extent(tiles_x, tiles_y)
    cap = ref.order_cap(w, h)
    good = ref.order(dict(ref.cost_maps(tiles_x, tiles_y))["random"], tiles_x, tiles_y)
    ref.check_invariants(good, cap, tiles_x, tiles_y)
    n0 = int((good[0] != ref.NONE).sum())

    def broken(edit, what):
        bad = good.copy()
        edit(bad)
        with pytest.raises(AssertionError, match=what):
            ref.check_invariants(bad, cap, tiles_x, tiles_y)

    def drop(a): a[0, n0 - 1] = ref.NONE
    def twice(a): a[0, n0 - 1] = a[0, 0]
    def hole(a): a[0, n0 - 1], a[0, cap - 1] = ref.NONE, a[0, n0 - 1]
    def out_of_range(a): a[0, 0] = tiles_x * tiles_y
    def swap_columns(a): a[0, 0], a[0, 1] = a[0, 1].copy(), a[0, 0].copy()
    broken(drop, "permutation")
    broken(twice, "permutation")
    assert n0 < cap
    broken(hole, "padding")
    broken(out_of_range, "permutation")
    assert n0 // tiles_y >= 2
    broken(swap_columns, "columns")

    def third_sweep(a):
        x = a[0, :n0 // tiles_y].astype(np.int64) % tiles_x
        a[0, :n0] = (np.array([0, 2, 1, 4, 3])[:, None] * tiles_x + x[None, :]).reshape(-1)
    broken(third_sweep, "row sweep")
    # a band wider than the lists hold: tiles fall off the end of a list (what a missing cap_cols clamp does)
    wide = np.full((8, cap), ref.NONE, dtype=np.uint32)
    b = [0, 6, 8, 10, 12, 14, 15, 16, 17]
    for i in range(8):
        lst = (np.arange(tiles_y)[:, None] * tiles_x + np.arange(b[i], b[i + 1])[None, :]).reshape(-1)[:cap]
        wide[i, :len(lst)] = lst
    with pytest.raises(AssertionError, match="permutation"):
        ref.check_invariants(wide, cap, tiles_x, tiles_y)
