"""CPU half of the node-step probe: the exact reference of tests/node_step_reference.py against things it was not written from —
its t-interval against dense rational point sampling along the ray, its node packing against runtime.decode_node, its exact
inverse against the matrix product — the class counts that keep test_gpu_node_step.py honest (after the free rows are dropped
every class keeps at least 256 must-accept and 256 must-reject rows), and the host side of the two hooks: the refusals of
sr_probe_node_step, which come before anything touches a GPU, and sr_probe_tl_record on transforms whose record is known."""
import ctypes as C
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

from sunray_amd import abi

sys.path.insert(0, os.path.dirname(__file__))
import node_step_reference as ns  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR_ERR_INVALID_ARG = -1
SENTINEL = 0xA5C3E10F


def test_interval_equals_dense_rational_sampling():
    """Small integer boxes and rays (zero components and inverted boxes among them): a point o + t d with t on a grid of 1/12 lies
    inside the box exactly where t lies inside the interval, and the interval's ends are themselves inside."""
    rng = np.random.default_rng(7)
    inside = lambda p, lo, hi: all(lo[a] <= p[a] <= hi[a] for a in range(3))
    some_hit = some_miss = 0
    for case in range(400):
        lo = [Fraction(int(x)) for x in rng.integers(-4, 4, 3)]
        hi = [l + int(x) for l, x in zip(lo, rng.integers(-1 if case % 10 == 0 else 0, 5, 3))]
        o = [Fraction(int(x), 2) for x in rng.integers(-12, 12, 3)]
        d = [Fraction(int(x), 3) for x in rng.integers(-3, 4, 3)]
        if case % 2 and all(h >= l for l, h in zip(lo, hi)):           # every other ray is aimed at a point of the box
            target = [l + (h - l) * Fraction(int(x), 4) for l, h, x in zip(lo, hi, rng.integers(0, 5, 3))]
            steps = int(rng.integers(1, 9))
            d = [(target[a] - o[a]) / steps for a in range(3)]
        got = ns.ray_box_interval(o, d, lo, hi)
        for k in range(-12 * 14, 12 * 14 + 1):
            t = Fraction(k, 12)
            p = [o[a] + t * d[a] for a in range(3)]
            assert inside(p, lo, hi) == (got is not None and got[0] <= t <= got[1]), (case, lo, hi, o, d, t, got)
        if got is None:
            some_miss += 1
            continue
        some_hit += 1
        for end, step in ((got[0], -1), (got[1], 1)):
            if end in (ns.INF, -ns.INF):
                assert all(d[a] == 0 for a in range(3))
                continue
            assert inside([o[a] + end * d[a] for a in range(3)], lo, hi)
            assert not inside([o[a] + (end + Fraction(step, 1000)) * d[a] for a in range(3)], lo, hi)
    assert some_hit > 100 and some_miss > 100


def test_packing_round_trips_through_decode_node():
    from sunray_amd import runtime
    rng = np.random.default_rng(11)
    W, _, po, co = runtime.bvh_layout()
    assert (W, po, co) == (4, ns.PLANE_DWORD, ns.CHILD_DWORD)
    for k in range(200):
        e = rng.choice([-126, -60, -10, 0, 3, 42], size=3)
        scales = np.ldexp(1.0, e).astype(np.float32)
        origin = (rng.integers(-1000, 1000, 3) * scales.astype(np.float64)).astype(np.float32) if k % 2 else rng.uniform(-1e3, 1e3, 3).astype(np.float32)
        q_lo, q_hi = rng.integers(0, 256, 3), rng.integers(0, 256, 3)
        c = k % 4
        words = ns.pack_node(origin, scales, c, q_lo, q_hi)
        lo, hi, child = runtime.decode_node(words)
        box = ns.NodeBox(origin, scales, q_lo, q_hi)
        assert [Fraction(float(x)) for x in lo[c]] == box.dec_lo and [Fraction(float(x)) for x in hi[c]] == box.dec_hi
        assert child[c] == ~((0 << 3) | 1) and all(child[s] == -1 for s in range(4) if s != c)
        for s in range(4):
            if s != c:          # the unused slots decode to 255 / 0: inverted wherever 255 cells are not lost in the origin's rounding
                assert (lo[s] >= hi[s]).all()
        for a in range(3):      # the grid planes are the decoded ones wherever those need no rounding
            if k % 2:
                assert box.grid_lo[a] == box.dec_lo[a] and box.grid_hi[a] == box.dec_hi[a]


def test_exact_inverse_and_object_ray():
    rng = np.random.default_rng(13)
    for k in range(50):
        m = rng.normal(size=12).astype(np.float32)
        R, T = ns.inverse_3x4(m)
        a = [[Fraction(float(m[4 * i + j])) for j in range(3)] for i in range(3)]
        for i in range(3):
            for j in range(3):
                assert sum(R[i][n] * a[n][j] for n in range(3)) == (1 if i == j else 0)
        p = [Fraction(int(x), 7) for x in rng.integers(-50, 50, 3)]
        world = [sum(a[i][j] * p[j] for j in range(3)) + T[i] for i in range(3)]
        assert ns.object_ray(m, world, [Fraction(0)] * 3)[0] == p
    assert ns.inverse_3x4(np.array([1, 2, 3, 0, 2, 4, 6, 0, 0, 0, 1, 0], np.float32)) is None


@pytest.mark.parametrize("name", sorted(set(ns.CLASSES["closest"]) | set(ns.CLASSES["closest_tl"])))
def test_every_class_keeps_both_labels(name):
    rs = ns.row_set(name)
    acc, rej, free = rs.counts()
    print("%s: %d rows, accept %d, reject %d, free %d" % (name, len(rs.rows), acc, rej, free))
    if name.endswith("nonfinite"):
        assert acc == rej == 0 and not rs.finite.any() and len(rs.rows) >= ns.MIN_PER_LABEL
        both = rs.rows["origin"].tolist(), rs.rows["dir"].tolist()
        assert all(not np.isfinite(o + d).all() for o, d in zip(*both))
        return
    assert rs.finite.all() and rej >= ns.MIN_PER_LABEL
    if name.endswith("inverted"):
        assert acc == 0 and free == 0
    else:
        assert acc >= ns.MIN_PER_LABEL
    slots = {c.node.c for c in rs.cases}
    assert slots == {0, 1, 2, 3}
    # the rows the hook takes: one leaf of triangle 0 in the used slot, -1 elsewhere, in every node of the row
    for field in ("node",) + (("mesh_node",) if rs.cases[0].form != ns.ONE else ()):
        child = rs.rows[field][:, ns.CHILD_DWORD:ns.CHILD_DWORD + 4]
        assert ((child == ns.LEAF).sum(axis=1) == 1).all() and ((child == ns.UNUSED).sum(axis=1) == 3).all()
    if rs.cases[0].form != ns.ONE:          # a node that is not under test never decides a row
        assert (rs.boxes[rs.label == ns.ACCEPT] == 8).all()
        if name in ("instances", "baked"):
            assert (rs.boxes == 8).all()


def test_class_sets_hold_what_the_issue_lists():
    graz = ns.row_set("grazing")
    sc = ns.row_set("scales")
    scales = {float(s) for c in sc.cases for s in c.node.scales}
    assert scales == {2.0 ** e for e in ns.SCALE_EXPONENTS}
    assert max(abs(float(x)) for c in sc.cases for x in c.node.origin) == 2.0 ** 44
    assert any(len(set(c.node.scales.tolist())) > 1 for c in sc.cases) and any(c.node.q_lo == [0, 0, 0] and c.node.q_hi == [255] * 3 for c in sc.cases)
    assert any(all(h == l + 1 for l, h in zip(c.node.q_lo, c.node.q_hi)) for c in sc.cases)
    ax = ns.row_set("axis")
    small = np.abs(ax.rows["dir"]) < 1e-20
    assert small.any(axis=1).all() and {1, 2} <= set(small.sum(axis=1).tolist())
    assert (ax.rows["dir"].view(np.uint32) == 0x80000000).any() and (ax.rows["dir"] == 0).any()
    b = ns.row_set("bounds")
    assert set(np.unique(b.rows["tmin"]).tolist()) == {-1.0, 0.0, float(np.float32(0.001)), 0.5}
    assert {float(np.float32(1e4)), float(np.float32(3e38))} <= set(np.unique(b.rows["tmax"]).tolist()) and len(np.unique(b.rows["tmax"])) > 50
    # grazing origins: inside the box and from 1e-2 to 1e4 extents away, on both labels
    for want in (ns.ACCEPT, ns.REJECT):
        far = [float(c.node.box.distance(ns.fr3(c.o))) / float(max(c.node.lo_hi_f64()[1] - c.node.lo_hi_f64()[0]))
               for c, l in zip(graz.cases, graz.label) if l == want]
        assert min(far) == 0.0 or want == ns.REJECT
        assert max(far) > 5e3
    inst = ns.row_set("instances")
    assert np.abs(inst.rows["origin"]).max() > 5e5
    assert any(np.array_equal(c.o2w, ns.IDENTITY) for c in inst.cases)
    k = ns.largest_unbaked_shear()
    assert 8.0 < float(k) < 9.0 and any(c.o2w[1] == k for c in inst.cases)
    baked = ns.row_set("baked")
    assert (baked.rows["instance"][:, 30] & 1).all() and not (inst.rows["instance"][:, 30] & 1).any()


def test_tl_record_hook_on_known_transforms():
    from sunray_amd import runtime
    from sunray_amd._lib import lib
    lo, hi = [-1.0, -2.0, -3.0], [1.0, 2.0, 3.0]
    rec, res = runtime.probe_tl_record(ns.IDENTITY, lo, hi, 3.0, 1.0)
    assert res == abi.TL_RECORD_OK and rec["flags"] == 0 and rec["blas_root"] == 0 and rec["tri_offset"] == 0
    assert np.array_equal(rec["w2o"], ns.IDENTITY) and np.array_equal(rec["o2w"], ns.IDENTITY) and rec["pad_a"] > 0 and rec["pad_b"] > 0
    t = ns.IDENTITY.copy()
    t[[3, 7, 11]] = (1024.0, -8.0, 0.5)
    rec_t, res = runtime.probe_tl_record(t, lo, hi, 3.0, 1.0)
    inv = ns.IDENTITY.copy()
    inv[[3, 7, 11]] = (-1024.0, 8.0, -0.5)
    assert res == abi.TL_RECORD_OK and np.array_equal(rec_t["w2o"], inv) and rec_t["pad_a"] == rec["pad_a"] and rec_t["pad_b"] > rec["pad_b"]
    singular = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0], np.float32)       # a zero scale: baked, walked without a ray transform
    rec_s, res = runtime.probe_tl_record(singular, lo, hi, 3.0, 1.0)
    assert res == abi.TL_RECORD_BAKED and rec_s["flags"] == 1 and np.array_equal(rec_s["w2o"], ns.IDENTITY) and rec_s["pad_a"] == 0 == rec_s["pad_b"]
    assert np.array_equal(rec_s["o2w"], singular)
    huge = ns.IDENTITY * np.float32(3e38)
    assert runtime.probe_tl_record(huge, lo, hi, 3.0, 1.0)[1] == abi.TL_RECORD_NO_FINITE_BOX
    out = np.full(33, SENTINEL, np.uint32)
    assert lib().sr_probe_tl_record(None, None, None, C.c_float(0), C.c_float(0), out.ctypes.data_as(C.c_void_p), None) == SR_ERR_INVALID_ARG
    assert (out == SENTINEL).all() and b"sr_probe_tl_record" in lib().sr_last_error()


def refused_rows():
    """(kind, rows, what) the hook must refuse: a second used child, an inner-node reference, a leaf count other than 1, a leaf of
    another triangle — in the node, and in the mesh node of the two-level kinds."""
    good = ns.row_set("top_grazing").rows[:70].copy()
    out = []
    for kind in sorted(ns.KINDS.values()):
        for field in ("node", "mesh_node") if kind in (abi.NODE_PROBE_CLOSEST_TL, abi.NODE_PROBE_ANY_TL) else ("node",):
            for what, edit in (("a second used child", lambda ch, c: ch.__setitem__((c + 1) % 4, ns.LEAF)),
                               ("an inner-node reference", lambda ch, c: ch.__setitem__(c, 0)),
                               ("an inner-node reference in an unused slot", lambda ch, c: ch.__setitem__((c + 2) % 4, 1)),
                               ("a leaf of two triangles", lambda ch, c: ch.__setitem__(c, 0xFFFFFFFF & ~((0 << 3) | 2))),
                               ("an empty leaf", lambda ch, c: ch.__setitem__(c, 0xFFFFFFFF)),
                               ("a leaf of triangle 1", lambda ch, c: ch.__setitem__(c, 0xFFFFFFFF & ~((1 << 3) | 1)))):
                rows = good.copy()
                i = 69 if field == "node" else 3
                ch = rows[field][i, ns.CHILD_DWORD:ns.CHILD_DWORD + 4]
                edit(ch, int(np.flatnonzero(ch == ns.LEAF)[0]))
                out.append((kind, rows, "%s in %s" % (what, field)))
    return out


def assert_refused(kind, rows_ptr, n, out_ptr, out_words, what):
    from sunray_amd._lib import lib
    assert lib().sr_probe_node_step(C.c_uint32(kind), rows_ptr, C.c_uint32(n), out_ptr) == SR_ERR_INVALID_ARG, what
    assert b"sr_probe_node_step" in lib().sr_last_error()
    assert (out_words == SENTINEL).all(), what + ": a refused call wrote results"


def test_node_step_hook_refuses_before_it_launches():
    """Every refusal is decided on the host, so it is the same call here, without a GPU, as on one: nothing can have been launched."""
    from sunray_amd._lib import lib
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    out = np.full(70 * 6 + 64, SENTINEL, np.uint32)
    for kind, rows, what in refused_rows():
        assert_refused(kind, ptr(rows), 70, ptr(out), out, what)
    good = ns.row_set("top_grazing").rows[:70].copy()
    for kind in (abi.NODE_PROBE_COUNT, 0xFFFFFFFF):
        assert_refused(kind, ptr(good), 70, ptr(out), out, "unknown kind")
    for kind in range(abi.NODE_PROBE_COUNT):
        assert_refused(kind, None, 70, ptr(out), out, "null rows")
        assert_refused(kind, ptr(good), 70, None, out, "null out")
        assert lib().sr_probe_node_step(C.c_uint32(kind), None, C.c_uint32(0), None) == 0       # nothing to do: no pointer is read
    # a mesh node that breaks the rule is none of the one-level kinds' business
    rows = good.copy()
    rows["mesh_node"][:, ns.CHILD_DWORD:ns.CHILD_DWORD + 4] = 0
    assert lib().sr_probe_node_step(C.c_uint32(abi.NODE_PROBE_CLOSEST), ptr(rows), C.c_uint32(0), ptr(out)) == 0
    assert C.sizeof(C.c_uint32) * 84 == abi.NODE_PROBE_ROW.itemsize == 336 and abi.NODE_PROBE_OUT.itemsize == 24


def test_header_names_the_kinds_in_abi_order():
    header = open(os.path.join(ROOT, "include", "sunray_hip.h")).read()
    block = header[header.index("typedef enum SrNodeProbeKind"):header.index("} SrNodeProbeKind;")]
    names = [ln.split(",")[0].split("=")[0].strip() for ln in block.splitlines()[1:] if ln.strip().startswith("SR_NODE_PROBE_")]
    assert names == ["SR_NODE_PROBE_CLOSEST", "SR_NODE_PROBE_ANY", "SR_NODE_PROBE_CLOSEST_TL", "SR_NODE_PROBE_ANY_TL", "SR_NODE_PROBE_KEY",
                     "SR_NODE_PROBE_COUNT"]
    assert [abi.NODE_PROBE_CLOSEST, abi.NODE_PROBE_ANY, abi.NODE_PROBE_CLOSEST_TL, abi.NODE_PROBE_ANY_TL, abi.NODE_PROBE_KEY,
            abi.NODE_PROBE_COUNT] == list(range(6))
