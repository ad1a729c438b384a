"""The three kernels of csrc/strip_copy.hip on their own, through sr_strip_pack / sr_strip_unpack / sr_history_reach_check:
pack and unpack byte for byte against the numpy model of tests/strip_reference.py (packed layout, canaries around every buffer,
every byte outside the rectangle), and the history-reach check count for count against its fp32 restatement, over every half
bit pattern and on the motion planes of rendered frames."""
import ctypes as C
import zlib

import numpy as np
import pytest

import strip_reference as ref
from sunray_amd import abi

pytestmark = pytest.mark.gpu

CANARY = 64
GATHER, EXCHANGE = (16, 2, 4, 4, 4), (48, 48)          # the renderer's two plane sets (multi_renderer.cpp)


@pytest.fixture(scope="module")
def rt():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    from sunray_amd import runtime
    return runtime


# ---- pack / unpack ------------------------------------------------------------------------------------------------------------
class Arena:
    """Several byte buffers in one device allocation, each with a 64-byte canary on both sides and a 64-byte aligned start, all
    filled with random bytes: one upload, one download."""

    def __init__(self, sizes, rng):
        self.spans, off = [], 0
        for n in sizes:
            self.spans.append((off + CANARY, n))
            off += (CANARY + n + CANARY + 255) & ~255
        self.before = rng.integers(0, 256, size=max(off, 256), dtype=np.uint8)
        import torch
        self.dev = torch.from_numpy(self.before.copy()).cuda()
        assert self.dev.data_ptr() % 64 == 0

    def ptr(self, i):
        return self.dev.data_ptr() + self.spans[i][0]

    def download(self):
        return self.dev.cpu().numpy()

    def data(self, host, i):
        o, n = self.spans[i]
        return host[o:o + n]

    def assert_only_data_changed(self, after, allowed, what):
        """Every byte outside the data of the buffers in `allowed` (canaries, gaps, the other buffers) is as it was."""
        keep = np.ones(self.before.size, dtype=bool)
        for i in allowed:
            o, n = self.spans[i]
            keep[o:o + n] = False
        bad = np.flatnonzero(keep & (after != self.before))
        assert bad.size == 0, "%s: %d bytes changed outside the target, first at arena offset %d (spans %s)" % (
            what, bad.size, bad[0], self.spans)


def case(bpps, W, H, x0, w, y0, h, dx=0, dy=0):
    return dict(bpps=tuple(bpps), W=W, H=H, rect=(x0, w, y0, h), rect2=(x0 + dx, w, y0 + dy, h))


def build_cases():
    cs = []
    # access unit 16 / 8 / 4 / 2 for bpp 2, 16 / 8 / 4 for bpp 4 (x0 * 4, W * 4 and w * 4 are multiples of 4: 2 is out of reach),
    # 16 / 8 for bpp 8; the other side of the copy sits at another (x0, y0) of the same alignment class
    for W, x0, w in ((64, 8, 8), (64, 4, 4), (64, 2, 6), (65, 1, 3)):
        cs.append(case([2], W, 5, x0, w, 1, 3, dx=16, dy=1))
    for W, x0, w in ((64, 4, 4), (64, 2, 2), (65, 1, 3)):
        cs.append(case([4], W, 5, x0, w, 1, 3, dx=8, dy=-1))
    for W, x0, w in ((64, 2, 2), (65, 1, 3)):
        cs.append(case([8], W, 4, x0, w, 0, 2, dx=4, dy=2))
    # segment length 1, 63, 64, 65, 127, 129 access units at every access width (one 64-lane sweep, just under / over, two sweeps)
    for L in (1, 63, 64, 65, 127, 129):
        cs.append(case([2], 199, 3, 1, L, 1, 2, dx=2))               # unit 2
        cs.append(case([4, 4], 199, 2, 5, L, 0, 1, dx=3, dy=1))      # unit 4
        cs.append(case([8], 199, 2, 3, L, 0, 2, dx=1))               # unit 8
        cs.append(case([16, 16, 16], 200, 2, 7, L, 1, 1, dx=5, dy=-1))   # unit 16
    cs.append(case(EXCHANGE, 200, 3, 0, 21, 0, 3, dx=100))           # 48-byte pixels: 63 and 129 units of 16
    cs.append(case(EXCHANGE, 200, 3, 150, 43, 1, 2, dx=-77, dy=-1))
    # the renderer's plane sets; n_planes * h = 0, 1, 2, 3 (mod 4): idle waves in the last block; h = 1
    for h in (1, 2, 3, 4, 7):
        cs.append(case(GATHER, 120, 9, 40, 40, 1, h, dx=8, dy=1))
        cs.append(case(EXCHANGE, 72, 9, 30, 16, 2, h, dx=-9))
    for bpps, h in (([2], 1), ([4], 2), ([8, 2, 48], 1), ([16], 4), ([2, 4, 8, 16], 3), ([2, 2, 2, 2, 2], 3)):
        cs.append(case(bpps, 37, 6, 3, 11, 1, h, dx=8, dy=1))
    # position: last row, last column, both, the whole image
    for bpps in (GATHER, [2], [48, 4]):
        cs.append(case(bpps, 50, 7, 10, 13, 4, 3, dx=-4, dy=-3))     # last row
        cs.append(case(bpps, 50, 7, 37, 13, 1, 3))                   # last column
        cs.append(case(bpps, 50, 7, 37, 13, 4, 3))                   # both
        cs.append(case(bpps, 50, 7, 0, 50, 0, 7))                    # whole image
        cs.append(case(bpps, 1, 1, 0, 1, 0, 1))                      # an image of one pixel
    return cs


CASES = build_cases()


def test_case_list_covers_what_it_claims():
    units = {b: set() for b in (2, 4, 8, 16, 48)}
    lengths = {u: set() for u in (16, 8, 4, 2)}
    idle, positions, n_planes = set(), set(), set()
    for c in CASES:
        x0, w, y0, h = c["rect"]
        assert c["W"] <= 200 and c["H"] <= 9
        for r in (c["rect"], c["rect2"]):
            assert r[0] >= 0 and r[2] >= 0 and r[0] + r[1] <= c["W"] and r[2] + r[3] <= c["H"], c
        for b in c["bpps"]:
            u = ref.access_unit(c["W"], x0, w, b)
            assert ref.access_unit(c["W"], c["rect2"][0], w, b) == u, c        # same alignment class on the other side
            units[b].add(u)
            lengths[u].add(w * b // u)
        idle.add(len(c["bpps"]) * h % 4)
        n_planes.add(len(c["bpps"]))
        positions.add((y0 + h == c["H"], x0 + w == c["W"], (w, h) == (c["W"], c["H"])))
    assert units[2] == {16, 8, 4, 2} and units[4] == {16, 8, 4} and units[8] == {16, 8} and units[16] == units[48] == {16}
    for u in (16, 8, 4, 2):
        assert lengths[u] >= {1, 63, 64, 65, 127, 129}, (u, sorted(lengths[u]))
    assert idle == {0, 1, 2, 3} and n_planes == {1, 2, 3, 4, 5}
    assert any(c["rect"][3] == 1 for c in CASES)
    assert {(True, False, False), (False, True, False), (True, True, False), (True, True, True), (False, False, False)} <= positions
    assert any(c["bpps"] == GATHER for c in CASES) and any(c["bpps"] == EXCHANGE for c in CASES)


@pytest.mark.parametrize("c", CASES, ids=lambda c: "%s-W%dH%d-%s" % ("_".join(map(str, c["bpps"])), c["W"], c["H"],
                                                                     "_".join(map(str, c["rect"]))))
def test_pack_and_unpack_equal_the_byte_model(rt, c):
    import torch
    bpps, W, H, rect, rect2 = c["bpps"], c["W"], c["H"], c["rect"], c["rect2"]
    n = len(bpps)
    _, w, _, h = rect
    offs, total = ref.packed_layout(bpps, w, h)
    assert rt.strip_packed_bytes(bpps, w, h) == total
    rng = np.random.default_rng(zlib.crc32(repr(c).encode()))
    tail = 48                                                         # bytes behind the last block: they keep their values
    arena = Arena([W * H * b for b in bpps] * 2 + [total + tail], rng)
    src, dst, pk = list(range(n)), list(range(n, 2 * n)), 2 * n

    def images(host, idx):
        return [arena.data(host, i).reshape(H, W * b) for i, b in zip(idx, bpps)]

    rt.strip_pack([(arena.ptr(i), b) for i, b in zip(src, bpps)], (W, H), rect, arena.ptr(pk))
    torch.cuda.synchronize()
    packed_after = arena.download()
    arena.assert_only_data_changed(packed_after, [pk], "pack %s" % (c,))
    want = ref.pack_model(images(arena.before, src), bpps, rect, arena.data(arena.before, pk))
    got = arena.data(packed_after, pk)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "pack %s: %d packed bytes differ, first at %d (blocks at %s, %d bytes)" % (c, bad.size, bad[0], offs, total)

    # the other side: another set of images with the same bpp list, at rect2
    rt.strip_unpack([(arena.ptr(i), b) for i, b in zip(dst, bpps)], (W, H), rect2, arena.ptr(pk))
    torch.cuda.synchronize()
    after = arena.download()
    arena.assert_only_data_changed(after, [pk] + dst, "unpack %s" % (c,))
    assert (arena.data(after, pk) == got).all(), "unpack %s changed the packed buffer" % (c,)
    want_imgs = ref.unpack_model(images(arena.before, dst), bpps, rect2, want)
    for p, (a, b) in enumerate(zip(images(after, dst), want_imgs)):
        ys, xs = np.nonzero(a != b)
        assert ys.size == 0, "unpack %s: plane %d (bpp %d) differs in %d bytes, first at row %d byte %d" % (
            c, p, bpps[p], ys.size, ys[0], xs[0])
        # the model itself: the rectangle now holds the source rectangle, slice for slice
        s = images(arena.before, src)[p]
        x0, _, y0, _ = rect
        x2, _, y2, _ = rect2
        assert (a[y2:y2 + h, x2 * bpps[p]:(x2 + w) * bpps[p]] == s[y0:y0 + h, x0 * bpps[p]:(x0 + w) * bpps[p]]).all()


def test_rejected_unpack_and_pack_leave_every_byte(rt):
    import torch
    from sunray_amd._lib import SunrayError
    bpps, W, H = (16, 2), 24, 5
    rng = np.random.default_rng(5)
    total = ref.packed_layout(bpps, 8, 3)[1]
    arena = Arena([W * H * b for b in bpps] + [total + 16], rng)
    planes = [(arena.ptr(0), 16), (arena.ptr(1), 2)]
    for call in (rt.strip_unpack, rt.strip_pack):
        for args in ((planes, (W, H), (17, 8, 1, 3), arena.ptr(2)),                      # leaves the image on the right
                     (planes, (W, H), (8, 8, 3, 3), arena.ptr(2)),                       # ... and below
                     (planes, (W, H), (8, 8, 1, 3), arena.ptr(2) + 2),                   # packed not 16-byte aligned
                     ([planes[0], (arena.ptr(1) + 2, 2)], (W, H), (8, 8, 1, 3), arena.ptr(2)),
                     ([planes[0], (arena.ptr(1), 3)], (W, H), (8, 8, 1, 3), arena.ptr(2)),
                     (planes * 3, (W, H), (8, 8, 1, 3), arena.ptr(2))):
            with pytest.raises(SunrayError) as e:
                call(*args)
            assert e.value.code == -1
    torch.cuda.synchronize()
    assert (arena.download() == arena.before).all()


# ---- the history-reach check --------------------------------------------------------------------------------------------------
HALF_ONE, HALF_TWO, HALF_INF, HALF_NAN = 0x3C00, 0x4000, 0x7C00, 0x7E00
OTHER = (0x0000, HALF_ONE, HALF_TWO, HALF_INF, HALF_NAN)
DEALS = ((1, 0), (4099, 12345), (40503, 777))                        # pattern = (k * pixel + s) mod 65536, k odd: a permutation
HELD = ((20, 20), (0, 64), (10, 30), (31, 33), (0, 17), (40, 64))    # empty, full, two interior, touching 0, touching n (n = 64)


class Checker:
    """Queues sr_history_reach_check calls, each with its own counter slot; one read-back."""

    def __init__(self, rt, n_slots, start=0):
        import torch
        from sunray_amd._lib import lib
        self.fn = lib().sr_history_reach_check
        self.counters = torch.full((n_slots,), start, dtype=torch.int64, device="cuda")
        self.base = self.counters.data_ptr()
        self.stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.n = 0

    def add(self, motion, W, H, axis, rect, held, same_slot=False):
        """`same_slot`: into the slot of the call before, which it must add to."""
        x0, w, y0, h = rect
        slot = self.n - 1 if same_slot else self.n
        rc = self.fn(C.c_void_p(motion.data_ptr()), W, H, axis, x0, w, y0, h, held[0], held[1], C.c_void_p(self.base + 8 * slot),
                     self.stream)
        assert rc == 0, rc
        self.n = slot + 1

    def read(self):
        assert self.n == self.counters.numel()
        return self.counters.cpu().numpy()


def to_device(words):
    import torch
    return torch.from_numpy(np.ascontiguousarray(words, dtype=np.uint32).view(np.int32)).cuda()      # same bits


@pytest.mark.parametrize("deal", range(len(DEALS)))
@pytest.mark.parametrize("axis", [abi.AXIS_COLS, abi.AXIS_ROWS])
def test_check_equals_restatement_on_every_half_pattern(rt, axis, deal):
    """All 65 536 half bit patterns (NaNs, infinities, subnormals, both zeros, 1.5 and its neighbours, values below -1.5) in the
    axis component of a 64 x 1024 plane (1024 x 64 for rows: the axis is 64 long either way), the other component 0, 1, 2, +inf or
    NaN, six held intervals; one launch per 64-pixel segment along the axis, so every count pins 64 decisions."""
    cols = axis == abi.AXIS_COLS
    W, H = (64, 1024) if cols else (1024, 64)
    n = 64
    k, s = DEALS[deal]
    pix = np.arange(65536, dtype=np.uint64)
    pattern = ((k * pix + s) % 65536).astype(np.uint32).reshape(H, W)
    assert np.unique(pattern).size == 65536
    pos = np.broadcast_to(np.arange(W)[None, :] if cols else np.arange(H)[:, None], (H, W))
    seg_axis = 1 if cols else 0                                      # a segment runs along the axis: a row (cols) / a column (rows)
    chk = Checker(rt, len(OTHER) * len(HELD) * 1024)
    want, planes = [], []
    for other in OTHER:
        words = (pattern | np.uint32(other << 16)) if cols else ((pattern << np.uint32(16)) | np.uint32(other))
        dev = to_device(words)
        planes.append((words, dev))
        for held in HELD:
            want.append(ref.reach_counted_f32(words, pos, n, cols, *held).sum(axis=seg_axis))
            for t in range(1024):
                chk.add(dev, W, H, axis, (0, 64, t, 1) if cols else (t, 1, 0, 64), held)
    got = chk.read().reshape(len(OTHER), len(HELD), 1024)
    want = np.array(want).reshape(len(OTHER), len(HELD), 1024)
    assert want.min() == 0 and np.unique(want).size > 8            # skipped planes count nothing; the others vary per segment
    bad = np.argwhere(got != want)
    if bad.size:
        o, hl, t = bad[0]
        seg = pattern[t, :] if cols else pattern[:, t]
        rect = (0, 64, t, 1) if cols else (t, 1, 0, 64)
        each = ref.reach_counted_f32(planes[o][0], pos, n, cols, *HELD[hl])
        each = each[t, :] if cols else each[:, t]
        pytest.fail("%d of %d counts differ; first: rectangle (x0, w, y0, h) = %s, held %s, other component 0x%04x: kernel %d, "
                    "restatement %d; patterns along the segment %s; restatement counts %s" % (
                        len(bad), got.size, rect, HELD[hl], OTHER[o], got[o, hl, t], want[o, hl, t],
                        ["0x%04x" % p for p in seg], each.astype(int).tolist()))


def moderate_motion(rng, H, W):
    """Random motion words: mostly small vectors, some large, a few markers and oddities."""
    mv = rng.normal(0.0, 0.08, size=(H, W, 2))
    mv[rng.random((H, W)) < 0.1] *= 8.0
    bits = mv.astype(np.float16).view(np.uint16).astype(np.uint32)
    odd = rng.random((H, W, 2)) < 0.03
    bits[odd] = rng.choice(np.array([0x4000, 0x3E00, 0x3E01, 0xBE01, 0x7C00, 0xFC00, 0x7E00, 0x0001, 0x8000], dtype=np.uint32),
                           size=int(odd.sum()))
    return bits[..., 0] | (bits[..., 1] << np.uint32(16))


@pytest.mark.parametrize("axis", [abi.AXIS_COLS, abi.AXIS_ROWS])
def test_check_adds_to_its_counter_over_any_rectangle(rt, axis):
    """Rectangles of 1, 63, 64, 65, 255 and 257 pixels (one wave, one block, just under and over), as a line and as a block, offset
    inside the image; every counter starts non-zero and is added to."""
    cols = axis == abi.AXIS_COLS
    W, H = 263, 19
    n = W if cols else H
    words = moderate_motion(np.random.default_rng(11), H, W)
    dev = to_device(words)
    pos = np.broadcast_to(np.arange(W)[None, :] if cols else np.arange(H)[:, None], (H, W))
    rects = [(5, 1, 3, 1), (0, 1, 0, 1), (W - 1, 1, H - 1, 1), (7, 63, 2, 1), (9, 21, 1, 3), (3, 7, 4, 9), (2, 64, 5, 1), (11, 8, 6, 8),
             (100, 4, 1, 16), (4, 65, 1, 1), (30, 13, 2, 5), (6, 255, 18, 1), (1, 51, 7, 5), (40, 15, 1, 17), (3, 257, 9, 1),
             (0, W, 0, H), (1, W - 1, 1, H - 1)]
    assert {r[1] * r[3] for r in rects} >= {1, 63, 64, 65, 255, 257}
    helds = [(0, n), (n // 3, n // 3), (n // 4, 3 * n // 4), (0, n // 2), (n // 2, n)]
    START = 1000
    chk = Checker(rt, len(rects) * len(helds) * 2, start=START)
    want = []
    for (x0, w, y0, h) in rects:
        for held in helds:
            c = int(ref.reach_counted_f32(words[y0:y0 + h, x0:x0 + w], pos[y0:y0 + h, x0:x0 + w], n, cols, *held).sum())
            chk.add(dev, W, H, axis, (x0, w, y0, h), held)
            want.append(START + c)
            chk.add(dev, W, H, axis, (x0, w, y0, h), held, same_slot=True)      # adds to what the first call left
            chk.add(dev, W, H, axis, (x0, w, y0, h), (0, 0))          # held nothing: every in-image range counts
            e = int(ref.reach_counted_f32(words[y0:y0 + h, x0:x0 + w], pos[y0:y0 + h, x0:x0 + w], n, cols, 0, 0).sum())
            want[-1] += c
            want.append(START + e)
    got = chk.read()
    want = np.array(want)
    assert (want > START).any()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "slot %d (rectangle %s): kernel %d, restatement %d" % (
        bad[0], rects[bad[0] // (2 * len(helds))], got[bad[0]] - START, want[bad[0]] - START)


# ---- the check on rendered frames, against the reads the pass really made --------------------------------------------------------
@pytest.mark.parametrize("cols", [True, False], ids=["cols", "rows"])
@pytest.mark.parametrize("scene_name", ["cornell_glass_mirror", "small_atrium"])
def test_check_on_rendered_motion_planes_never_misses_a_logged_read(rt, oracle, blue_noise, scene_name, cols):
    """120 x 48 moving-camera frames (tests/history_read_util.py): the kernel runs on the device's motion plane of the frame whose
    reads the oracle logged, over three overlapping bands along the axis and the whole image, for every held interval [a, b) on a
    4-pixel grid. Every count equals the restatement's, and where the kernel counts nothing, no pixel of the rectangle read
    history outside [a, b)."""
    import history_read_util as hr
    from oracle.binding import NO_READ
    W, H = 120, 48
    n = W if cols else H
    axis = abi.AXIS_COLS if cols else abi.AXIS_ROWS
    desc = hr.SCENES[scene_name]()
    gsc = rt.Scene(0).load(desc)
    moves = hr.camera_moves(oracle, scene_name, W, H, cols, blue_noise)
    cuts = [0, n // 3, 2 * n // 3, n]
    # thirds of the axis grown by 8 pixels (with the renderer's 30-pixel halo every rectangle of a 48-pixel axis is nearly the
    # whole axis, and no partial held region could ever satisfy it), and the whole image
    spans = [(max(cuts[s] - 8, 0), min(cuts[s + 1] + 8, n)) for s in range(3)] + [(0, n)]
    rects = [(lo, hi - lo, 0, H) if cols else (0, W, lo, hi - lo) for lo, hi in spans]
    helds = [(a, b) for a in range(0, n + 1, 4) for b in range(a, n + 1, 4)]
    chk = Checker(rt, len(moves) * len(rects) * len(helds))
    pos = np.broadcast_to(np.arange(W)[None, :] if cols else np.arange(H)[:, None], (H, W))
    want, read_lo, read_hi, keep = [], [], [], []
    for label, cam in moves:
        motion, log = hr.ris_pair(oracle, scene_name, W, H, cam, blue_noise)
        gf = rt.DeviceFrame(W, H, blue_noise)
        m0 = rt.camera_matrices(desc.camera_pos, desc.camera_target, desc.fov_y, W, H, None)
        gsc.trace_ris(gf, m0, 0)
        gsc.trace_ris(gf, rt.camera_matrices(cam[0], cam[1], desc.fov_y, W, H, list(m0.view_proj)), 1)
        keep.append(gf)
        di_gi = [(log[..., k].astype(np.int64), log[..., k + 1].astype(np.int64)) for k in (0, 2)]
        inside = [(rx != NO_READ) & (rx >= 0) & (ry >= 0) & (rx < W) & (ry < H) for rx, ry in di_gi]   # the reads the pass made
        along = [rx if cols else ry for rx, ry in di_gi]
        for (x0, w, y0, h) in rects:
            sub = (slice(y0, y0 + h), slice(x0, x0 + w))
            r = np.concatenate([along[k][sub][inside[k][sub]] for k in (0, 1)])
            want.extend(ref.reach_counts_f32(motion[sub], pos[sub], n, cols, helds))
            read_lo.extend([r.min() if r.size else n] * len(helds))
            read_hi.extend([r.max() if r.size else -1] * len(helds))
            for held in helds:
                chk.add(gf.motion, W, H, axis, (x0, w, y0, h), held)
    got = chk.read()
    for gf, (label, cam) in zip(keep, moves):                 # the plane the kernel saw is the plane the restatement saw
        assert (gf.motion.cpu().numpy().view(np.uint32).reshape(H, W) == hr.ris_pair(oracle, scene_name, W, H, cam, blue_noise)[0]).all(), label
    want, read_lo, read_hi = np.array(want), np.array(read_lo), np.array(read_hi)
    held_all = np.array(helds * (len(moves) * len(rects)))
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%d counts differ; first: move %s, rectangle %s, held %s: kernel %d, restatement %d" % (
        bad.size, moves[bad[0] // (len(rects) * len(helds))][0], rects[bad[0] // len(helds) % len(rects)], held_all[bad[0]],
        got[bad[0]], want[bad[0]])
    quiet = got == 0
    missed = quiet & ((read_lo < held_all[:, 0]) | (read_hi >= held_all[:, 1]))
    assert not missed.any(), "the check counted nothing, yet a read left the held region; first: move %s, rectangle %s, held %s, reads %d..%d" % (
        moves[np.flatnonzero(missed)[0] // (len(rects) * len(helds))][0], rects[np.flatnonzero(missed)[0] // len(helds) % len(rects)],
        held_all[np.flatnonzero(missed)[0]], read_lo[np.flatnonzero(missed)[0]], read_hi[np.flatnonzero(missed)[0]])
    partial = (held_all[:, 0] > 0) | (held_all[:, 1] < n)
    assert (quiet & partial).any() and (~quiet).any()         # some partial held region suffices for some rectangle; others do not
