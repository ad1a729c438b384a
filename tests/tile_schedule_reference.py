"""Plain reference of the passes' tile schedule (tile_order_kernel, sunray_amd/csrc/kernels.hip; DESIGN.md "XCD-aware
block->tile map with a cost-aware sweep"), in Python integers, plus the invariants every schedule must keep and the shapes
and cost maps the schedule tests run. No GPU, no library.

The schedule of a launch rectangle of tiles_x x tiles_y tiles (8x8 pixels) is eight tile lists, one per XCD:
  * the tile columns are cut into eight bands, list i holds band i;
  * a band is walked in whole tile rows, ascending x inside a row;
  * each list is order_cap entries long (the pass launch starts 8 * order_cap workgroups), NONE after its last tile.
Everything is integer arithmetic, so a device result is compared with this one for equality."""
import bisect

import numpy as np

NONE = 0xFFFFFFFF
TILE = 8
BANDS = 8
MAX_BALANCED_COLS = 1024     # wider rectangles keep equal-width bands
MIN_BALANCED_COLS = 16       # narrower ones too
MAX_PEAK_ROWS = 1024         # taller rectangles are swept end to end
PEAK_LEAD = 4                # the sweep starts this many rows beyond the row of the most expensive tile


def tiles(width, rows):
    return (width + TILE - 1) // TILE, (rows + TILE - 1) // TILE


def cap_cols(tiles_x):
    """Widest band the cost balancing may form: 1.5 x the equal share, and two columns."""
    return min(tiles_x, 3 * tiles_x // 16 + 2)


def order_cap(width, rows):
    """Entries per list: the widest band either way of cutting can form (balanced, or equal widths rounded up), all rows."""
    tiles_x, tiles_y = tiles(width, rows)
    return max(cap_cols(tiles_x), (tiles_x + BANDS - 1) // BANDS) * tiles_y


def _grid(costs, tiles_x, tiles_y):
    c = np.asarray(costs, dtype=np.uint64).reshape(tiles_y, tiles_x)
    return c


def bands(costs, tiles_x, tiles_y):
    """The nine cut positions b[0] = 0 .. b[8] = tiles_x: band i is columns [b[i], b[i+1])."""
    if not (MIN_BALANCED_COLS <= tiles_x <= MAX_BALANCED_COLS):
        return [tiles_x * i // BANDS for i in range(BANDS + 1)]
    c = _grid(costs, tiles_x, tiles_y)
    col = [int(v) + 1 for v in c.sum(axis=0, dtype=np.uint64).tolist()]      # + 1: an unmeasured image still spreads evenly
    before = [0]
    for v in col:
        before.append(before[-1] + v)
    total = before[-1]
    centre = [before[x] + col[x] // 2 for x in range(tiles_x)]              # non-decreasing in x
    cap = cap_cols(tiles_x)
    b = [0]
    for i in range(1, BANDS):
        left = BANDS - i                                                     # bands still to form after this cut
        # a column belongs to the side of the ideal cut (i eighths of the total) its centre lies on; a cut never moves back
        want = max(bisect.bisect_left(centre, total // BANDS * i), b[-1])
        # constraints, the later ones winning: one column at least, cap at most, the bands left can cover the rest at cap
        # columns each, and each of them gets a column
        want = max(want, b[-1] + 1)
        want = min(want, b[-1] + cap)
        want = max(want, tiles_x - left * cap)
        want = min(want, tiles_x - left)
        b.append(want)
    b.append(tiles_x)
    return b


def _band_rows(c, x0, x1, tiles_y):
    """Row order of the band of columns [x0, x1)."""
    quarter = max(tiles_y // 4, 1)
    part = c[:, x0:x1]
    head = int(part[:quarter].sum(dtype=np.uint64))
    tail = int(part[tiles_y - quarter:].sum(dtype=np.uint64))
    bottom_up = tail > head                                                  # walk from the expensive end to the cheap end
    if tiles_y > MAX_PEAK_ROWS:
        return list(range(tiles_y - 1, -1, -1)) if bottom_up else list(range(tiles_y))
    # start PEAK_LEAD rows beyond the (first) row with the most expensive tile, run to the expensive end, then take the rest
    # from there to the cheap end
    peak = int(np.argmax(part.max(axis=1))) if x1 > x0 else 0
    if bottom_up:
        start = max(peak - PEAK_LEAD, 0)
        return list(range(start, tiles_y)) + list(range(start - 1, -1, -1))
    start = min(peak + PEAK_LEAD, tiles_y - 1)
    return list(range(start, -1, -1)) + list(range(start + 1, tiles_y))


def order(costs, tiles_x, tiles_y):
    """-> [8, order_cap] uint32: the eight lists, NONE after a list's last tile."""
    cap = order_cap(tiles_x * TILE, tiles_y * TILE)
    c = _grid(costs, tiles_x, tiles_y)
    b = bands(costs, tiles_x, tiles_y)
    out = np.full((BANDS, cap), NONE, dtype=np.uint32)
    for i in range(BANDS):
        x0, x1 = b[i], b[i + 1]
        if x1 == x0:
            continue
        rows = np.array(_band_rows(c, x0, x1, tiles_y), dtype=np.int64)
        lst = (rows[:, None] * tiles_x + np.arange(x0, x1, dtype=np.int64)[None, :]).reshape(-1)
        out[i, :len(lst)] = lst                                              # a band wider than the cap does not fit: error
    return out


# ---- invariants ---------------------------------------------------------------------------------------------------------
def monotone_runs(seq):
    """Fewest strictly monotone pieces a sequence of distinct numbers splits into (greedy: a piece ends where the direction turns)."""
    runs, i, n = 0, 0, len(seq)
    while i < n:
        runs += 1
        j = i + 1
        if j < n:
            up = seq[j] > seq[i]
            while j < n and (seq[j] > seq[j - 1]) == up:
                j += 1
        i = j
    return runs


def check_invariants(lists, cap, tiles_x, tiles_y):
    """Asserts what every schedule must keep for each pixel to be rendered exactly once, on an [8, cap] array of lists,
    whatever heuristic produced it; each assertion names the invariant. -> the nine cut positions read off the lists."""
    lists = np.asarray(lists)
    assert lists.shape == (BANDS, cap) and lists.dtype == np.uint32, "shape: eight lists of order_cap entries"
    assert cap % tiles_y == 0, "order_cap: whole rows"
    n_tiles = tiles_x * tiles_y
    real = lists != NONE
    # (b) padding: nothing but NONE after a list's last real entry
    counts = real.sum(axis=1)
    for i in range(BANDS):
        assert real[i, :counts[i]].all(), "(b) padding: list %d has a NONE entry before its last tile" % i
    entries = lists[real].astype(np.int64)
    # (b) permutation
    assert entries.size == n_tiles, "(b) permutation: %d entries for %d tiles" % (entries.size, n_tiles)
    assert (entries < n_tiles).all(), "(b) permutation: tile index out of range"
    seen = np.bincount(entries, minlength=n_tiles)
    assert (seen == 1).all(), "(b) permutation: %d tiles missing, %d listed more than once" % (int((seen == 0).sum()), int((seen > 1).sum()))
    b = [0]
    for i in range(BANDS):
        lst = lists[i, :counts[i]].astype(np.int64)
        if lst.size == 0:
            b.append(b[-1])
            continue
        assert lst.size % tiles_y == 0, "(b) whole rows: list %d has %d tiles, %d rows" % (i, lst.size, tiles_y)
        bw = lst.size // tiles_y
        ty, tx = (lst // tiles_x).reshape(tiles_y, bw), (lst % tiles_x).reshape(tiles_y, bw)
        # (b) list i is exactly the columns [b[i], b[i+1]), row by row, ascending x inside a row
        assert (tx == np.arange(b[-1], b[-1] + bw)[None, :]).all(), "(b) columns: list %d is not columns [%d, %d) in ascending x" % (i, b[-1], b[-1] + bw)
        assert (ty == ty[:, :1]).all(), "(b) whole rows: list %d mixes rows" % i
        rows = ty[:, 0]
        assert np.array_equal(np.sort(rows), np.arange(tiles_y)), "(b) whole rows: list %d does not hold every row once" % i
        # (c) one or two monotone runs
        runs = monotone_runs(rows.tolist())
        assert runs <= 2, "(c) row sweep: list %d walks its rows in %d monotone runs" % (i, runs)
        # (a) no band wider than the list can hold
        assert bw <= cap // tiles_y, "(a) band %d is %d columns wide, order_cap holds %d" % (i, bw, cap // tiles_y)
        b.append(b[-1] + bw)
    # (a) cuts
    assert b[0] == 0 and b[BANDS] == tiles_x, "(a) cuts: bands end at column %d of %d" % (b[BANDS], tiles_x)
    assert all(b[i] <= b[i + 1] for i in range(BANDS)), "(a) cuts: decreasing"
    if tiles_x >= BANDS:
        assert all(b[i] < b[i + 1] for i in range(BANDS)), "(a) cuts: an empty band with %d columns" % tiles_x
    return b


# ---- the cases of the schedule tests --------------------------------------------------------------------------------------
# (tiles_x, tiles_y): below the balancing threshold (empty bands under 8 columns); the >= 16 switch (cap_cols 4 -> 5); the
# quarter of the rows 0 -> 1 and the sweep start clamped at both ends; the 1000-pixel case (cap 25); the widest balanced
# rectangle and the first one beyond; the tallest one with a peak row and the first one swept end to end.
SHAPES = [(1, 1), (7, 3), (8, 1), (9, 4), (15, 3), (16, 3), (17, 3), (17, 1), (17, 2), (17, 4), (17, 5), (17, 9), (125, 3),
          (1024, 2), (1025, 2), (17, 1024), (17, 1025)]
# maps that put everything into one column: at these shapes they must drive a band to cap_cols and one to a single column
CLAMP_MAPS = ("col0", "colLast", "colMid")
CLAMP_SHAPES = [(16, 3), (17, 3), (125, 3)]


def extent(tiles_x, tiles_y):
    """Ragged pixel extent (width, rows) of a rectangle of tiles_x x tiles_y tiles."""
    return TILE * tiles_x - 6, TILE * tiles_y - 7


def cost_maps(tiles_x, tiles_y):
    """-> [(name, uint32 [tiles_y * tiles_x])]: the adversarial cost maps, one of each kind."""
    z = lambda: np.zeros((tiles_y, tiles_x), dtype=np.uint32)
    maps = [("zero", z()), ("saturated", np.full((tiles_y, tiles_x), NONE, dtype=np.uint32))]
    rng = np.random.default_rng(20241 + 1031 * tiles_x + tiles_y)
    r = rng.integers(0, 1 << 20, size=(tiles_y, tiles_x)).astype(np.uint32)
    r[rng.random((tiles_y, tiles_x)) < 0.3] = 0
    maps.append(("random", r))
    for name, x in (("col0", 0), ("colLast", tiles_x - 1), ("colMid", tiles_x // 2)):
        m = z(); m[:, x] = NONE
        maps.append((name, m))
    m = z(); m[:, :tiles_x // 2] = 1000
    maps.append(("leftHalf", m))
    m = z(); m[:, tiles_x - tiles_x // 2:] = 1000
    maps.append(("rightHalf", m))
    m = z(); m[tiles_y - 1, :] = 1000
    maps.append(("lastRow", m))
    m = z(); m[0, :] = 1000
    maps.append(("firstRow", m))
    for name, y, x in (("tileRow0", 0, tiles_x // 2), ("tileRowLast", tiles_y - 1, 0), ("tileRowMid", tiles_y // 2, tiles_x - 1)):
        m = z(); m[y, x] = NONE
        maps.append((name, m))
    return [(name, np.ascontiguousarray(m).reshape(-1)) for name, m in maps]


def widths(b):
    return [b[i + 1] - b[i] for i in range(BANDS)]
