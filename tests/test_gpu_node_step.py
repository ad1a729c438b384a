"""The node step of traverse_ws (sunray_amd/csrc/traverse.h) against exact arithmetic, row by row.

sr_probe_node_step runs the traversal itself — the four ray-list instantiations traverse_ws<ANY, STATS = true, TL> with per-ray
tmin / tmax — on one hand-made node per ray whose only used child is a leaf of one triangle, so `tris` of a row is 1 exactly when
every box test on the way to the leaf accepted. tests/node_step_reference.py labels every row in fractions.Fraction: must accept
(the segment meets the box the builders guarantee the geometry in, or the fp32 triangle test itself reports a hit), must reject
(it misses the box grown by a margin ten times the step's own slack), or free (dropped). Here, per kind and input class: tris == 1
on every must-accept row, tris == 0 on every must-reject row, `boxes` exactly 4 per node stepped, every reported hit equal to the
oracle's intersect_tri (after its transform_point in the two-level form) in every bit, and the existence kinds decide every row as
the closest-hit kinds do. The reference itself is checked in test_node_step_reference_host.py, so no tolerance is restated here.
Run on an MI355X with:  python -m pytest tests/test_gpu_node_step.py -m gpu -q
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

from sunray_amd import abi

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(__file__))
import helper_probe as hp  # noqa: E402
import node_step_reference as ns  # noqa: E402
from test_node_step_reference_host import SENTINEL, assert_refused, refused_rows  # noqa: E402

TAIL = 256
MISS = 0xFFFFFFFF


@pytest.fixture(scope="module")
def rt():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: run them with -m gpu on an MI355X")
    from sunray_amd import runtime
    return runtime


@functools.lru_cache(None)
def device_rows(kind, name):
    """One launch: every row of class `name` through kind `kind`."""
    from sunray_amd import runtime
    return runtime.probe_node_step(ns.KINDS[kind], ns.row_set(name).rows)


def describe(rs, i, out):
    c = rs.cases[i]
    return ("row %d (%s, slot %d): o %s d %s t (%r, %r); node origin %s scales %s q_lo %s q_hi %s%s -> boxes %d tris %d tri %#x t %r"
            % (i, c.form, c.node.c, c.o.tolist(), c.d.tolist(), float(c.tmin), float(c.tmax), c.node.origin.tolist(), c.node.scales.tolist(),
               c.node.q_lo, c.node.q_hi, "" if c.o2w is None else "; o2w %s" % c.o2w.tolist(), out["boxes"][i], out["tris"][i], out["tri"][i],
               float(out["t"][i])))


CASES = [(kind, name) for kind in ns.KINDS for name in ns.CLASSES[kind]]


@pytest.mark.parametrize("kind,name", CASES, ids=["%s-%s" % c for c in CASES])
def test_box_tests_equal_exact_arithmetic(rt, oracle, kind, name):
    rs = ns.row_set(name)
    out = device_rows(kind, name)
    two_level = kind.endswith("_tl")
    hit, bits = ns.expected(rs, oracle)
    if name.endswith("inverted"):              # an inverted box holds nothing: the triangle next to it is never reached
        hit[:] = False
    reached = out["tris"] == 1
    assert ((out["tris"] == 0) | reached).all(), "a leaf of one triangle is tested once or never"
    if not rs.finite.any():                    # non-finite rays: the answer is free, the call returns and no node is stepped twice
        assert (out["boxes"] <= (8 if two_level else 4)).all() and (out["boxes"] % 4 == 0).all()
        return
    must_accept = (rs.label == ns.ACCEPT) | hit
    must_reject = (rs.label == ns.REJECT) & ~hit
    assert not ((rs.label == ns.REJECT) & hit).any(), "the triangle test reports a hit outside the outer box: the row set is wrong"
    print("%s %s: %d rows: %d must accept (%d by a reported hit alone), %d must reject, %d free of which %d accepted"
          % (kind, name, len(rs.rows), must_accept.sum(), (hit & (rs.label != ns.ACCEPT)).sum(), must_reject.sum(),
             (~must_accept & ~must_reject).sum(), (~must_accept & ~must_reject & reached).sum()))
    bad = np.flatnonzero(must_accept & ~reached)
    assert bad.size == 0, "%d must-accept rows were culled; first: %s" % (bad.size, describe(rs, bad[0], out))
    bad = np.flatnonzero(must_reject & reached)
    assert bad.size == 0, "%d must-reject rows were accepted; first: %s" % (bad.size, describe(rs, bad[0], out))
    # boxes: 4 per node stepped — one node in the one-level form; the mesh's root as well where the top-level box accepted
    if not two_level:
        assert (out["boxes"] == 4).all()
    else:
        assert ((out["boxes"] == 4) | (out["boxes"] == 8)).all()
        known = rs.boxes != 0
        bad = np.flatnonzero(known & (out["boxes"] != rs.boxes))
        assert bad.size == 0, "boxes: want %d; %s" % (rs.boxes[bad[0]], describe(rs, bad[0], out))
        assert (out["boxes"][reached] == 8).all()
    # the hit: the oracle's wherever the triangle test reports one (such a row is never culled), a miss everywhere else
    if kind.startswith("any"):
        assert np.array_equal(out["tri"], hit.astype(np.uint32)) and not out["t"].any() and not out["u"].any() and not out["v"].any()
        return
    got = np.stack([out["tri"], out["t"].view(np.uint32), out["u"].view(np.uint32), out["v"].view(np.uint32)], axis=1)
    bad = np.flatnonzero(hit & (got != bits).any(axis=1))
    assert bad.size == 0, "hit differs from the oracle's %s; %s" % (bits[bad[0]].tolist(), describe(rs, bad[0], out))
    assert (out["tri"][~hit] == MISS).all() and (out["t"][~hit] == -1.0).all() and not out["u"][~hit].any() and not out["v"][~hit].any()
    assert hit.sum() >= 10 or name.endswith("inverted"), "too few reported hits to compare"


@pytest.mark.parametrize("level", ["", "_tl"])
def test_existence_queries_decide_like_closest_hit_queries(rt, level):
    for name in ns.CLASSES["closest" + level]:
        rs = ns.row_set(name)
        a, c = device_rows("any" + level, name), device_rows("closest" + level, name)
        f = rs.finite
        assert np.array_equal(a["tris"][f], c["tris"][f]) and np.array_equal(a["boxes"][f], c["boxes"][f]), name
        assert np.array_equal(a["tri"][f] != 0, c["tri"][f] != MISS), name


@pytest.mark.parametrize("kind", list(ns.KINDS))
def test_row_counts_leave_the_tail_untouched(rt, kind):
    """Row counts around the wave and the workgroup: the first n rows are what the full launch gave, the words behind them stay."""
    from sunray_amd._lib import lib
    name = "instances" if kind.endswith("_tl") else "grazing"
    rows, full = ns.row_set(name).rows, device_rows(kind, name)
    w = abi.NODE_PROBE_OUT.itemsize // 4
    for n in (0, 1, 63, 64, 65, 257):
        out = np.full(n * w + TAIL, SENTINEL, np.uint32)
        assert lib().sr_probe_node_step(C.c_uint32(ns.KINDS[kind]), rows.ctypes.data_as(C.c_void_p), C.c_uint32(n), out.ctypes.data_as(C.c_void_p)) == 0
        assert (out[n * w:] == SENTINEL).all(), "%s, n = %d: words behind the last row were written" % (kind, n)
        assert np.array_equal(out[:n * w], full[:n].view(np.uint32).reshape(-1)), "%s, n = %d" % (kind, n)


def test_refusals_write_nothing(rt):
    """A second used child, an inner-node reference, a leaf count other than 1, null pointers, an unknown kind: SR_ERR_INVALID_ARG
    and no word of `out` changes. The decision is the host's (test_node_step_reference_host.py runs the same calls without a GPU)."""
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    out = np.full(70 * 6 + TAIL, SENTINEL, np.uint32)
    for kind, rows, what in refused_rows():
        assert_refused(kind, ptr(rows), 70, ptr(out), out, what)
    good = ns.row_set("top_grazing").rows[:70].copy()
    assert_refused(abi.NODE_PROBE_COUNT, ptr(good), 70, ptr(out), out, "unknown kind")
    for kind in range(abi.NODE_PROBE_COUNT):
        assert_refused(kind, None, 70, ptr(out), out, "null rows")
        assert_refused(kind, ptr(good), 70, None, out, "null out")


def ord_key(bits):
    """numpy's definition of the order-preserving key: -0 counts as +0; non-negative floats get the sign bit set, negative ones
    are inverted — unsigned keys then order like the floats."""
    b = np.where(bits == 0x80000000, 0, bits).astype(np.uint32)
    return np.where(b >> 31, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def test_hit_key_orders_like_the_floats(rt):
    """ord_f32 / unord_f32, the key of the atomic minimum that decides every closest hit, on the float classes of helper_probe.py:
    the numpy definition, the round trip, and strict monotonicity over all finite values with -0 mapped onto +0."""
    bits = np.unique(np.concatenate([hp.class_set(), hp.stratified(), hp.around(np.float32([0.0, 1.0, 0.001, 1e4, 3e38]), 2)]))
    finite = bits[(bits & 0x7FFFFFFF) <= 0x7F800000]                 # infinities included; NaNs have no place in the order
    rows = np.zeros(len(bits), dtype=abi.NODE_PROBE_ROW)
    rows["origin"][:, 0] = bits.view(np.float32)
    rows["origin"][:, 1] = ord_key(bits).view(np.float32)            # a key, by its bits
    out = rt.probe_node_step(abi.NODE_PROBE_KEY, rows)
    nan = (bits & 0x7FFFFFFF) > 0x7F800000
    assert np.array_equal(out["boxes"][~nan], ord_key(bits[~nan]))
    canon = np.where(bits == 0x80000000, 0, bits)
    assert np.array_equal(out["tris"][~nan], canon[~nan]), "unord(ord(f)) is f (and +0 for -0)"
    assert np.array_equal(out["tri"][~nan], canon[~nan]), "unord of numpy's key is the float"
    values = finite.view(np.float32).astype(np.float64)
    order = np.argsort(values, kind="stable")
    keys = out["boxes"][np.searchsorted(bits, finite)][order].astype(np.int64)
    v = values[order]
    assert (np.diff(keys)[np.diff(v) > 0] > 0).all() and (np.diff(keys)[np.diff(v) == 0] == 0).all()
    assert len(finite) > 20000


def test_tl_record_hook_equals_the_host_two_level_build(rt):
    """Every record sr_probe_tl_record writes is the record the host two-level build writes for the same instance (the words the
    build alone knows — where the mesh's tree and triangles start, the mesh slot — aside)."""
    from sunray_amd import scenes
    v, idx = scenes.uv_sphere(1.0, 6, 6)
    rng = np.random.default_rng(5)
    xf = np.stack([ns.instance_transform(rng, k) for k in range(40)]).astype(np.float32).reshape(-1, 12)
    sc = rt.Scene(0, instancing="two_level").set_top_level_build("host")
    sc.add_mesh(1, v, idx, abi.material())
    sc.set_instances([(1, xf)])
    assert sc.two_level() and not sc.top_level_info().on_device
    records = sc.read_top_level()[2]
    tris = sc.read_mesh_tree(1)["tris"][:, :9].reshape(-1, 3, 3)         # v0, v1, v2 in leaf order
    # the mesh's root block as the mesh-tree build accumulates it (fp32, one operation at a time)
    e1, e2 = tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]
    pad = np.float32(4e-6) * (np.abs(e1) + np.abs(e2))
    lo = np.nextafter(tris.min(axis=1) - pad, np.float32(-np.inf)).min(axis=0)
    hi = np.nextafter(tris.max(axis=1) + pad, np.float32(np.inf)).max(axis=0)
    max_edge, max_abs = float((np.abs(e1) + np.abs(e2)).max()), float(np.abs(tris).max())
    assert len(records) == len(xf)
    n_baked = 0
    for i, m in enumerate(xf):
        rec, res = rt.probe_tl_record(m, lo, hi, max_abs, max_edge)
        want = records[i]
        for f in ("w2o", "o2w", "pad_a", "pad_b", "flags"):
            assert np.array_equal(np.asarray(rec[f]).view(np.uint32), np.asarray(want[f]).view(np.uint32)), (i, f, rec[f], want[f])
        assert (res == abi.TL_RECORD_BAKED) == bool(want["flags"] & 1)
        n_baked += int(res == abi.TL_RECORD_BAKED)
    assert 0 < n_baked < len(xf)
    sc.close()
