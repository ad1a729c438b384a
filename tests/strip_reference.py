"""The round-1/2 Python implementations of the strip geometry and plans (Partition, balanced_bounds, axis_cost_from_tiles,
history_exchange_plan), kept as the reference the C++ port behind the C ABI (csrc/multi_gpu.cpp, sr_partition_* /
sr_balanced_bounds / sr_axis_cost_from_tiles / sr_history_exchange_plan) is checked against (tests/test_host_abi.py), and the
models of the multi-device renderer's strip kernels (csrc/strip_copy.hip): pack / unpack as numpy slice copies, the
history-reach check restated on hand-workable scalars and, operation for operation, in vectorised fp32."""
SPATIAL_HALO = 30


class Partition:
    """`world` contiguous strips of a width x height image along one axis. `bounds` (world + 1 increasing cut positions,
    e.g. from balanced_bounds) replaces the equal split; it must stay the same for a whole frame sequence: a rank owns
    the temporal history of exactly its strip + halo."""

    def __init__(self, width, height, world, axis="cols", bounds=None):
        if axis not in ("cols", "rows"):
            raise ValueError("axis must be 'cols' or 'rows'")
        self.width, self.height, self.world, self.axis = width, height, world, axis
        self.length = width if axis == "cols" else height
        if bounds is None:
            per = (self.length + world - 1) // world
            bounds = [min(r * per, self.length) for r in range(world)] + [self.length]
        bounds = [int(v) for v in bounds]
        if len(bounds) != world + 1 or bounds[0] != 0 or bounds[-1] != self.length or any(b > a for b, a in zip(bounds, bounds[1:])):
            raise ValueError("bounds must be %d increasing cuts from 0 to %d" % (world + 1, self.length))
        self.bounds = bounds

    def span(self, rank):
        """(start, size) of rank's strip along the axis."""
        return self.bounds[rank], self.bounds[rank + 1] - self.bounds[rank]

    def sizes(self):
        return [self.bounds[r + 1] - self.bounds[r] for r in range(self.world)]

    def tile(self, a0, n):
        """The (y0, h, x0, w) launch rectangle of positions [a0, a0 + n) along the axis, full extent across it."""
        return (0, self.height, a0, n) if self.axis == "cols" else (a0, n, 0, self.width)

    def grown(self, rank, grow):
        """(start, size) of rank's strip grown by `grow` on both sides, clipped to the image."""
        a0, n = self.span(rank)
        lo, hi = max(0, a0 - grow), min(self.length, a0 + n + grow)
        return lo, hi - lo

    def view(self, flat, channels=None):
        """[H, W(, C)] view of a per-pixel buffer (torch tensor or numpy array of H*W rows)."""
        return flat.reshape(self.height, self.width, -1) if channels is None else flat.reshape(self.height, self.width, channels)

    def cut(self, img, a0, n):
        """Slice [a0, a0 + n) along the axis of an [H, W, C] view."""
        return img[:, a0:a0 + n] if self.axis == "cols" else img[a0:a0 + n]


def balanced_bounds(cost, world, min_size=8, max_share=2.5):
    """Cuts positions 0 .. len(cost) into `world` contiguous strips of (nearly) equal summed cost: returns world + 1
    increasing cut positions. Strips are cut one after the other, each taking 1/n of the cost that is left for the n ranks
    that are left, with at least `min_size` positions and at most max_share * length / world (the gather pads every strip
    to the largest one, so a very large cheap strip would inflate the collective). Deterministic: every rank that feeds
    the same profile gets the same cut."""
    import numpy as np
    cost = np.maximum(np.asarray(cost, dtype=np.float64), 0.0) + 1e-12
    length = len(cost)
    min_size = max(1, min(min_size, length // max(world, 1)))
    max_size = max(int(np.ceil(max_share * length / max(world, 1))), min_size)
    cum = np.concatenate([[0.0], np.cumsum(cost)])
    bounds = [0]
    for k in range(world - 1):
        y, n = bounds[-1], world - k
        target = cum[y] + (cum[-1] - cum[y]) / n
        cut = int(np.searchsorted(cum, target, side="left"))
        cut = min(max(cut, y + min_size), y + max_size)          # this strip: [min_size, max_size]
        cut = max(cut, length - (n - 1) * max_size)              # the ranks that are left can still cover the rest ...
        cut = min(cut, length - (n - 1) * min_size)              # ... and each gets its minimum
        bounds.append(max(cut, y))
    bounds.append(length)
    return [int(v) for v in bounds]


def axis_cost_from_tiles(tile_costs, tiles_x, axis, length, tile=8):
    """Per-pixel-column (or per-pixel-row) cost from the per-tile cycle counts the library records for its own tile
    schedule (sr_scene_read_tile_costs, row-major ty * tiles_x + tx): what balanced_bounds cuts."""
    import numpy as np
    t = np.asarray(tile_costs, dtype=np.float64).reshape(-1, tiles_x)
    per_tile = t.sum(axis=0) if axis == "cols" else t.sum(axis=1)
    return np.repeat(per_tile / float(tile), tile)[:length]


def history_exchange_plan(part, motion_halo):
    """Who sends which reservoir band to whom after a RIS pass: rank r needs the pixels within SPATIAL_HALO + motion_halo
    of its strip that lie outside strip + SPATIAL_HALO (those it traced itself); every such pixel is owned — and was
    traced with exact history — by exactly one other rank. Returns a list of (src, dst, start, size) along the axis, in
    a deterministic order every rank derives alike."""
    plan = []
    if motion_halo <= 0 or part.world <= 1:
        return plan
    for dst in range(part.world):
        a0, n = part.span(dst)
        if n <= 0:
            continue
        g0, gn = part.grown(dst, SPATIAL_HALO)
        h0, hn = part.grown(dst, SPATIAL_HALO + motion_halo)
        for lo, hi in ((h0, g0), (g0 + gn, h0 + hn)):         # the band before and the band after the traced region
            for src in range(part.world):
                if src == dst:
                    continue
                s0, sn = part.span(src)
                x0, x1 = max(lo, s0), min(hi, s0 + sn)
                if x1 > x0:
                    plan.append((src, dst, x0, x1 - x0))
    return plan


# ---- strip_pack_kernel / strip_unpack_kernel (csrc/strip_copy.hip) as a byte model ---------------------------------------------
def access_unit(W, x0, w, bpp):
    """Widest access (16, 8, 4 or 2 bytes) every row segment of a plane is aligned to: from x0 * bpp, W * bpp and w * bpp."""
    for u in (16, 8, 4):
        if (x0 * bpp) % u == 0 and (W * bpp) % u == 0 and (w * bpp) % u == 0:
            return u
    return 2


def packed_layout(bpps, w, h):
    """(byte offset of every plane's block, total size): plane after plane, every block padded to 16 bytes."""
    offs, off = [], 0
    for bpp in bpps:
        offs.append(off)
        off += (w * h * bpp + 15) & ~15
    return offs, off


def pack_model(images, bpps, rect, packed_before):
    """The packed buffer after packing rectangle (x0, w, y0, h) of `images` ([H, W * bpp] uint8 arrays) over `packed_before`:
    rows in order within a plane; the padding between blocks and everything behind the last block keep their bytes."""
    import numpy as np
    x0, w, y0, h = rect
    offs, total = packed_layout(bpps, w, h)
    out = np.array(packed_before, dtype=np.uint8, copy=True)
    assert out.size >= total
    for img, bpp, off in zip(images, bpps, offs):
        out[off:off + w * h * bpp] = img[y0:y0 + h, x0 * bpp:(x0 + w) * bpp].reshape(-1)
    return out


def unpack_model(images, bpps, rect, packed):
    """The images after unpacking `packed` into rectangle (x0, w, y0, h): slice assignment, every other byte kept."""
    import numpy as np
    x0, w, y0, h = rect
    offs, _ = packed_layout(bpps, w, h)
    out = [np.array(img, dtype=np.uint8, copy=True) for img in images]
    for img, bpp, off in zip(out, bpps, offs):
        img[y0:y0 + h, x0 * bpp:(x0 + w) * bpp] = packed[off:off + w * h * bpp].reshape(h, w * bpp)
    return out


# ---- restatement of history_reach_check_kernel (csrc/strip_copy.hip) ----------------------------------------------------------
def held_region(bounds, slot, motion_halo):
    """[lo, hi) along the axis a slot holds exact history for: its strip grown by SR_SPATIAL_HALO + motion_halo, clipped."""
    length = bounds[-1]
    grow = SPATIAL_HALO + motion_halo
    return max(bounds[slot] - grow, 0), min(bounds[slot + 1] + grow, length)


def read_range(p, mv, n):
    """Conservative [lo, hi] pixel range of the temporal read of pixel p (index along the axis) whose stored half-precision motion
    component is mv, in an image n pixels long; None when the range lies outside the image."""
    import math
    import numpy as np
    m = float(np.float32(np.float16(mv)))
    c = (p + 0.5) - m * n
    e = abs(m) * n / 1024.0 + 1.0
    lo, hi = max(math.floor(c - e - 0.5), 0), min(math.ceil(c + e + 0.5), n - 1)
    return (lo, hi) if lo <= hi else None


def counted(p, mv, n, held):
    r = read_range(p, mv, n)
    return r is not None and (r[0] < held[0] or r[1] >= held[1])


def half_bits_to_f32(bits):
    import numpy as np
    with np.errstate(invalid="ignore"):                       # signalling NaN patterns convert to quiet ones
        return np.asarray(bits, dtype=np.uint16).view(np.float16).astype(np.float32)


NO_HISTORY, NOT_A_MOTION, IN_RANGE = 0, 1, 2


def reach_f32(motion, pos, n, cols, clip=True):
    """The kernel's per-pixel decision up to the held test, operation for operation in fp32 (numpy rounds every operation on its
    own: no contraction). motion: uint32 R16G16_SFLOAT words; pos: the pixels' positions along the axis; n: the axis length;
    cols: the axis is x. Returns (kind, lo, hi): kind NO_HISTORY (the other component or this one marks an invalid reprojection:
    skipped), NOT_A_MOTION (always counted) or IN_RANGE with the clipped integer range [lo, hi] (empty when lo > hi)."""
    import numpy as np
    f = np.float32
    motion = np.asarray(motion, dtype=np.uint32)
    mx, my = half_bits_to_f32(motion & 0xFFFF), half_bits_to_f32(motion >> 16)
    with np.errstate(invalid="ignore", over="ignore"):
        skip = (mx > f(1.5)) | (my > f(1.5))
        m = mx if cols else my
        bad = ~(np.abs(m) <= f(1.5))
        ms = np.where(bad, f(0), m).astype(f)
        c = (np.asarray(pos).astype(f) + f(0.5)) - ms * f(n)
        e = np.abs(ms) * f(n) * f(1.0 / 1024.0) + f(1.0)
        assert c.dtype == f and e.dtype == f
        lo = np.floor(c - e - f(0.5)).astype(np.int64)
        hi = np.ceil(c + e + f(0.5)).astype(np.int64)
    if clip:                                                  # clip=False: the range before the clip (tests measure slack on it)
        lo = np.maximum(lo, 0)
        hi = np.minimum(hi, n - 1)
    kind = np.where(skip, NO_HISTORY, np.where(bad, NOT_A_MOTION, IN_RANGE))
    return kind, lo, hi


def reach_counted_f32(motion, pos, n, cols, held_lo, held_hi):
    """Per pixel: does history_reach_check_kernel count it for the held region [held_lo, held_hi)?"""
    kind, lo, hi = reach_f32(motion, pos, n, cols)
    return (kind == NOT_A_MOTION) | ((kind == IN_RANGE) & (lo <= hi) & ((lo < held_lo) | (hi >= held_hi)))


def reach_counts_f32(motion, pos, n, cols, helds):
    """The count the kernel adds for the pixels given, for each held region [lo, hi) of `helds`."""
    import numpy as np
    kind, lo, hi = reach_f32(motion, pos, n, cols)
    always = int((kind == NOT_A_MOTION).sum())
    live = (kind == IN_RANGE) & (lo <= hi)
    lo, hi = lo[live][None, :], hi[live][None, :]
    helds = np.asarray(helds, dtype=np.int64).reshape(-1, 2)
    return always + ((lo < helds[:, :1]) | (hi >= helds[:, 1:])).sum(axis=1)
