"""Row counts and observed slack of the node-step probe -> profiles/node_step_probe.txt.

Per kind and input class of tests/node_step_reference.py: the rows that must be accepted, must be rejected and were dropped as
free, and how much room the box tests left — the smallest miss distance that was still rejected and the largest one that was
accepted among the free rows, both in cells of the node under test (tests/node_step_reference.py miss_cells: the growth of the
box, per face, at which the query would meet it; for an instance's mesh node in object space, its padding not taken off).
Whoever changes the far-side inflation, box_dir or the padding formula reads here how much room there is.

    python scripts/gpu_node_step_probe.py [OUT]        (on an MI355X; default OUT: profiles/node_step_probe.txt)
"""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import node_step_reference as ns  # noqa: E402
from oracle import binding as oracle  # noqa: E402
from sunray_amd import runtime  # noqa: E402


@functools.lru_cache(None)
def misses(name):
    """Miss distance in cells of every finite row of the class that no label makes ACCEPT (NaN elsewhere)."""
    rs = ns.row_set(name)
    out = np.full(len(rs.rows), np.nan)
    for i, c in enumerate(rs.cases):
        if not c.finite or rs.label[i] == ns.ACCEPT:
            continue
        o, d = ns.fr3(c.o), ns.fr3(c.d)
        if c.form == ns.TL_MESH:
            o, d = ns.object_ray(c.o2w, o, d)
        out[i] = ns.miss_cells(o, d, ns.fr(c.tmin), ns.fr(c.tmax), c.node.box)
    return out


def main():
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "node_step_probe.txt")
    oracle.build()
    lines = ["Node-step probe: row counts and observed slack (scripts/gpu_node_step_probe.py, tests/test_gpu_node_step.py)",
             "",
             "accept / reject / free: rows the exact reference labels must-accept (a reported triangle hit included), must-reject, neither.",
             "culled at: the smallest miss distance, in cells of the node under test, of a row the device still culled (any label).",
             "kept at:   the largest miss distance of a free row the device accepted (0: the query meets the decoded box). '-': no such row.",
             "wrong:     must-accept rows culled + must-reject rows accepted (the test asserts 0).",
             "Reading the two distances: a cell is the unit of the node's own grid, the step's slack is relative to the distance walked.",
             "'scales' mixes grid scales per axis (2^-126 next to 2^42), where one rounding on a coarse axis is far beyond 2^20 cells of a fine",
             "one: the line 'one scale' holds its rows with one scale on all axes. 'bounds' rows are free by their t range (a segment",
             "that ends within 1e-4 of the box), not by a distance in space. 'instances' counts cells of the mesh node in object space",
             "with the instance's padding pad_a * |o|_inf + pad_b (up to 4 object units at |o| = 1e6) still in the distance.",
             "",
             "%-11s %-14s %6s %7s %7s %6s %12s %12s %6s" % ("kind", "class", "rows", "accept", "reject", "free", "culled at", "kept at", "wrong")]
    for kind in ns.KINDS:
        for name in ns.CLASSES[kind]:
            rs = ns.row_set(name)
            out = runtime.probe_node_step(ns.KINDS[kind], rs.rows)
            if not rs.finite.any():
                lines.append("%-11s %-14s %6d %7s %7s %6s %12s %12s %6s  (non-finite rays: max boxes %d)"
                             % (kind, name, len(rs.rows), "-", "-", "-", "-", "-", "-", out["boxes"].max()))
                continue
            hit, _ = ns.expected(rs, oracle)
            if name.endswith("inverted"):
                hit[:] = False
            accept, reject = (rs.label == ns.ACCEPT) | hit, (rs.label == ns.REJECT) & ~hit
            free = ~accept & ~reject
            reached = out["tris"] == 1
            m = misses(name)
            culled = m[~reached & ~np.isnan(m)]
            kept = m[free & reached & ~np.isnan(m)]
            fmt = lambda v: "-" if v.size == 0 else "%.4g" % v
            lines.append("%-11s %-14s %6d %7d %7d %6d %12s %12s %6d"
                         % (kind, name, len(rs.rows), accept.sum(), reject.sum(), free.sum(), fmt(culled.min() if culled.size else culled),
                            fmt(kept.max() if kept.size else kept), (accept & ~reached).sum() + (reject & reached).sum()))
            if name.endswith("scales"):
                one = np.array([len(set(c.node.scales.tolist())) == 1 for c in rs.cases])
                culled, kept = m[one & ~reached & ~np.isnan(m)], m[one & free & reached & ~np.isnan(m)]
                lines.append("%-11s %-14s %6d %7d %7d %6d %12s %12s %6d"
                             % ("", "  one scale", one.sum(), (one & accept).sum(), (one & reject).sum(), (one & free).sum(),
                                fmt(culled.min() if culled.size else culled), fmt(kept.max() if kept.size else kept),
                                (one & accept & ~reached).sum() + (one & reject & reached).sum()))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(dst)), exist_ok=True)
    with open(dst, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
