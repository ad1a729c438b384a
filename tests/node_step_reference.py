"""Exact-arithmetic reference of the traversal's node step, and the input classes of its probe (sr_probe_node_step).

One row = one ray against a tree of one hand-made quantised node whose single used child is a leaf of one triangle (the two-level
forms: a top-level node, one instance, the root node of its mesh). The device reports whether the leaf was reached (`tris`), which
is 1 exactly when every box test on the way accepted. This module says what that answer must be, in fractions.Fraction:

  node packing        pack_node: the inverse of runtime.decode_node
  what a node means   NodeBox: per axis the grid planes origin + q * scale exactly, the fp32 planes the kernel's fma decodes, and
                      from them the GEOMETRY box — where the builders guarantee the child's geometry lies: a guard band of GUARD
                      cells inside the grid planes and not outside the decoded ones (both coincide wherever the planes are fp32
                      numbers) — and the OUTER box, the union of both grown by a margin
  exact t-interval    ray_box_interval: of an fp32 ray inside a box with rational planes (a zero direction component: closed slab)
  two-level           object_ray: M^-1 (o - T), M^-1 d with M inverted exactly from the fp32 o2w
  labels              ACCEPT  the open segment (tmin, tmax) meets the geometry box (of every node on the way), or the fp32 triangle
                              test itself reports a hit (a hit the triangle test reports is never culled)
                      REJECT  the whole line misses the outer box, or the outer box lies wholly beyond tmax * (1 + 1e-4), or wholly
                              before t_lo * (1 + 1e-4) with the kernel's own lower bound t_lo = min(tmin, 0) - |tmin| <= 0
                      FREE    everything between: dropped

The outer box's margin per face is cell / 4 + 1e-5 * L (+ the instance record's pad_a * |o|_inf + pad_b in the two-level form), L the
distance from the ray origin to the box. It is derived, not measured: the step's slack in t is the far-side inflation 5e-7 * |t|
plus a handful of 2^-24 roundings of quantities no larger than |t| + extent / |d|, under 1e-6 * (L + extent) in space; a quarter
cell is about 1e-3 * extent; the margin is wider than the slack by more than ten times. All three REJECT clauses use the outer
box, so a plane distance that rounds across zero or across tmax cannot turn a REJECT row.

Domain of the generators: grid scales 2^-126 .. 2^42, node origins up to 2^44, directions whose largest
component is far above 2^-100 (box_dir replaces smaller components for the box test, which is only harmless next to a component
of ordinary size), ray origins up to 1e4 node extents away (1e3 for inverted planes), instance transforms up to the baking limit.
"""
import functools
import math
import os
import sys
from fractions import Fraction

import numpy as np

from sunray_amd import abi

sys.path.insert(0, os.path.dirname(__file__))
import helper_probe as hp  # noqa: E402
import tree_build_reference as tbr  # noqa: E402

f32 = np.float32
INF = math.inf
GUARD = tbr.GUARD
ACCEPT, REJECT, FREE = 1, -1, 0
LEAF, UNUSED = 0xFFFFFFFE, 0xFFFFFFFF           # ~((0 << 3) | 1), -1
PLANE_DWORD, CHILD_DWORD, SCALE_DWORDS = 4, 12, tbr.SCALE_DWORDS
MIN_PER_LABEL = 256
ONE, TL_MESH, TL_TOP, TL_BAKED = "one", "tl_mesh", "tl_top", "tl_baked"       # which node of which form a row puts to the test
KINDS = {"closest": abi.NODE_PROBE_CLOSEST, "any": abi.NODE_PROBE_ANY, "closest_tl": abi.NODE_PROBE_CLOSEST_TL, "any_tl": abi.NODE_PROBE_ANY_TL}
ONE_LEVEL_CLASSES = ("grazing", "axis", "scales", "bounds", "inverted", "nonfinite")
CLASSES = {"closest": ONE_LEVEL_CLASSES, "any": ONE_LEVEL_CLASSES,
           "closest_tl": tuple("top_" + c for c in ONE_LEVEL_CLASSES) + ("instances", "baked"),
           "any_tl": tuple("top_" + c for c in ONE_LEVEL_CLASSES) + ("instances", "baked")}
REL_T = Fraction(1, 10000)
IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], dtype=f32)


def fr(x):
    """The exact value of a finite float."""
    return Fraction(float(x))


def fr3(v):
    return [fr(x) for x in v]


def f32_bits(x):
    return int(np.asarray(x, dtype=f32).view(np.uint32))


# ---- nodes ----------------------------------------------------------------------------------------------------------------------
def pack_node(origin, scales, c, q_lo, q_hi):
    """The 16 dwords of a node with child slot c in use (a leaf of triangle 0 alone): the inverse of runtime.decode_node.
    origin: 3 floats; scales: 3 powers of two; q_lo / q_hi: 3 bytes each; the other slots are inverted boxes (255 / 0), unused."""
    n = np.zeros(16, dtype=np.uint32)
    for a in range(3):
        n[a] = f32_bits(origin[a])
        n[SCALE_DWORDS[a]] = f32_bits(scales[a])
        assert math.frexp(float(scales[a]))[0] == 0.5 and 0 <= q_lo[a] <= 255 and 0 <= q_hi[a] <= 255
        n[PLANE_DWORD + a] = (0xFFFFFFFF & ~(0xFF << (8 * c))) | (int(q_lo[a]) << (8 * c))
        n[PLANE_DWORD + 3 + a] = int(q_hi[a]) << (8 * c)
    n[CHILD_DWORD:CHILD_DWORD + 4] = UNUSED
    n[CHILD_DWORD + c] = LEAF
    return n


class NodeBox:
    """The used child's box of a packed node, exactly: grid planes, decoded (fp32) planes, cells."""

    def __init__(self, origin, scales, q_lo, q_hi):
        q_lo, q_hi = [int(q) for q in q_lo], [int(q) for q in q_hi]
        self.cell = [fr(s) for s in scales]
        self.grid_lo = [fr(origin[a]) + q_lo[a] * self.cell[a] for a in range(3)]
        self.grid_hi = [fr(origin[a]) + q_hi[a] * self.cell[a] for a in range(3)]
        self.dec_lo = [fr(tbr.decode(q_lo[a], f32(scales[a]), f32(origin[a]))) for a in range(3)]
        self.dec_hi = [fr(tbr.decode(q_hi[a], f32(scales[a]), f32(origin[a]))) for a in range(3)]
        self.inverted = any(q_lo[a] > q_hi[a] for a in range(3))

    def geometry(self):
        """Where the builders guarantee the child's geometry: GUARD cells inside the grid planes, not outside the decoded ones."""
        return ([max(self.grid_lo[a] + GUARD * self.cell[a], self.dec_lo[a]) for a in range(3)],
                [min(self.grid_hi[a] - GUARD * self.cell[a], self.dec_hi[a]) for a in range(3)])

    def decoded(self):
        return self.dec_lo, self.dec_hi

    def grown(self, cells=Fraction(0), space=Fraction(0)):
        """The union of the grid box and the decoded box, every face moved outward by `cells` cells plus `space`."""
        return ([min(self.grid_lo[a], self.dec_lo[a]) - cells * self.cell[a] - space for a in range(3)],
                [max(self.grid_hi[a], self.dec_hi[a]) + cells * self.cell[a] + space for a in range(3)])

    def distance(self, o):
        """Euclidean distance of the point o from the decoded box (a rational within 2^-32 relative of the root)."""
        d2 = Fraction(0)
        for a in range(3):
            d = max(self.dec_lo[a] - o[a], o[a] - self.dec_hi[a], 0)
            d2 += d * d
        p, q = d2.numerator, d2.denominator
        return Fraction(math.isqrt((p * q) << 64), q << 32)


def ray_box_interval(o, d, lo, hi):
    """[t_enter, t_exit] of the line o + t d (Fractions) inside the box lo .. hi (Fractions), +-inf where unbounded, or None where
    the line misses the box or the box is inverted. A zero direction component: the slab is closed, lo <= o <= hi."""
    enter, leave = -INF, INF
    for a in range(3):
        if lo[a] > hi[a]:
            return None
        if d[a] == 0:
            if not (lo[a] <= o[a] <= hi[a]):
                return None
            continue
        t1, t2 = (lo[a] - o[a]) / d[a], (hi[a] - o[a]) / d[a]
        if t1 > t2:
            t1, t2 = t2, t1
        enter, leave = max(enter, t1), min(leave, t2)
    return (enter, leave) if enter <= leave else None


def t_lo_of(tmin):
    """The kernel's lower bound of a query: min(tmin, 0) - |tmin| (exact here; <= 0)."""
    return min(tmin, 0) - abs(tmin)


def label_box(o, d, tmin, tmax, box, extra=Fraction(0)):
    """ACCEPT / REJECT / FREE of one node's box test for the exact ray (o, d) (Fractions) over (tmin, tmax); `extra`: further
    margin in space (the padding of the two-level form)."""
    if box.inverted:
        return REJECT
    g = ray_box_interval(o, d, *box.geometry())
    if g is not None and g[0] < tmax and g[1] > tmin:
        return ACCEPT
    margin = Fraction(1, 100000) * box.distance(o) + extra
    r = ray_box_interval(o, d, *box.grown(Fraction(1, 4), margin))
    if r is None or r[0] > tmax * (1 + REL_T) or r[1] < t_lo_of(tmin) * (1 + REL_T):
        return REJECT
    return FREE


def miss_cells(o, d, tmin, tmax, box, limit=1 << 20):
    """How far the query misses the box, in cells: the smallest uniform growth of the decoded / grid box (cells per face) at which
    the line meets it within [t_lo, tmax]; 0 where it already does, `limit` where that growth does not reach it. Bisection, 1/64 cell."""
    if box.inverted:
        return float(limit)
    t_lo = t_lo_of(tmin)

    def meets(g):
        r = ray_box_interval(o, d, *box.grown(g))
        return r is not None and r[0] <= tmax and r[1] >= t_lo
    if meets(Fraction(0)):
        return 0.0
    if not meets(Fraction(limit)):
        return float(limit)
    lo, hi = Fraction(0), Fraction(1)
    while not meets(hi):
        lo, hi = hi, hi * 2
    while hi - lo > max(hi / 64, Fraction(1, 64)):
        mid = (lo + hi) / 2
        lo, hi = (lo, mid) if meets(mid) else (mid, hi)
    return float(hi)


def inverse_3x4(o2w):
    """(R, T): the exact inverse R of the 3x3 part of the fp32 transform and its translation T, as Fractions; None: singular."""
    m = [fr(x) for x in o2w]
    a = [[m[0], m[1], m[2]], [m[4], m[5], m[6]], [m[8], m[9], m[10]]]
    c = [[a[(i + 1) % 3][(j + 1) % 3] * a[(i + 2) % 3][(j + 2) % 3] - a[(i + 1) % 3][(j + 2) % 3] * a[(i + 2) % 3][(j + 1) % 3] for j in range(3)]
         for i in range(3)]
    det = sum(a[0][j] * c[0][j] for j in range(3))
    if det == 0:
        return None
    return [[c[j][i] / det for j in range(3)] for i in range(3)], [m[3], m[7], m[11]]


def object_ray(o2w, o, d):
    """The exact object-space ray M^-1 (o - T), M^-1 d of the world-space ray (o, d) (Fractions)."""
    R, T = inverse_3x4(o2w)
    p = [o[k] - T[k] for k in range(3)]
    return [sum(R[i][k] * p[k] for k in range(3)) for i in range(3)], [sum(R[i][k] * d[k] for k in range(3)) for i in range(3)]


# ---- cases ----------------------------------------------------------------------------------------------------------------------
class Node:
    def __init__(self, origin, scales, c, q_lo, q_hi):
        self.origin, self.scales = np.asarray(origin, dtype=f32), np.asarray(scales, dtype=f32)
        self.c, self.q_lo, self.q_hi = c, [int(q) for q in q_lo], [int(q) for q in q_hi]
        self.box = NodeBox(self.origin, self.scales, self.q_lo, self.q_hi)

    def words(self):
        return pack_node(self.origin, self.scales, self.c, self.q_lo, self.q_hi)

    def lo_hi_f64(self):
        g_lo, g_hi = self.box.geometry()
        return np.array([float(x) for x in g_lo]), np.array([float(x) for x in g_hi])


def covering_node(c, points):
    """A node whose used child is a box far larger than everything in `points` (finite floats): the node that is not under test."""
    r = max([abs(float(p)) for p in points if math.isfinite(float(p))] + [2.0 ** -120])
    e = min(max(math.frexp(r)[1] + 4, -119), 126)          # 2^e >= 8 r
    return Node([-(2.0 ** e)] * 3, [2.0 ** (e - 7)] * 3, c, [0, 0, 0], [255, 255, 255])


class Case:
    """One row before it is packed: the ray, the node under test, where it stands (`form`), and for the two-level forms the
    instance transform. `tri`: three fp32 vertices (object space; world space for a baked instance and the one-level form)."""

    def __init__(self, form, o, d, tmin, tmax, node, tri, o2w=None):
        self.form, self.node, self.o2w = form, node, o2w
        self.o, self.d = np.asarray(o, dtype=f32), np.asarray(d, dtype=f32)
        self.tmin, self.tmax = f32(tmin), f32(tmax)
        self.tri = np.asarray(tri, dtype=f32).reshape(3, 3)
        self.finite = bool(np.isfinite(self.o).all() and np.isfinite(self.d).all())


def triangle_in(node, rng):
    """An fp32 triangle inside the node's geometry box (its vertices in the middle 80 % of every axis)."""
    lo, hi = node.lo_hi_f64()
    if (hi <= lo).any():            # an inverted or empty box holds nothing: any triangle near it will do
        lo, hi = np.minimum(lo, hi), np.maximum(lo, hi) + 1e-30
    u = rng.uniform(0.1, 0.9, size=(3, 3))
    return (lo[None, :] + u * (hi - lo)[None, :]).astype(f32)


def point_on(tri, rng):
    """A point of the triangle's interior (float64): rays aimed at it are the ones whose reported hits get compared."""
    w = rng.dirichlet([2.0, 2.0, 2.0])
    return w @ tri.astype(np.float64)


def moderate_node(rng, c, mixed=None):
    """A node of ordinary size on exact grid planes: scales 2^-10 .. 2^2 (one per axis if `mixed`), origin a multiple of the scale."""
    mixed = rng.random() < 0.5 if mixed is None else mixed
    e = rng.integers(-10, 3, size=3) if mixed else np.repeat(rng.integers(-10, 3), 3)
    s = np.ldexp(1.0, e)
    origin = rng.integers(-4000, 4000, size=3) * s
    q_lo = rng.integers(0, 200, size=3)
    q_hi = np.minimum(q_lo + rng.integers(1, 56, size=3), 255)
    return Node(origin, s, c, q_lo, q_hi)


def boundary_target(node, rng, outward_cells):
    """A point on a corner, an edge or a face of the node's geometry box, moved outward (negative: inward) by `outward_cells` cells on
    the axes that sit on a face; the other axes lie inside."""
    lo, hi = node.lo_hi_f64()
    cell = node.scales.astype(np.float64)
    on_face = rng.permutation(3) < rng.integers(1, 4)          # 1 axis: a face, 2: an edge, 3: a corner
    p = lo + rng.uniform(0.05, 0.95, 3) * (hi - lo)
    for a in range(3):
        if on_face[a]:
            p[a] = hi[a] + outward_cells * cell[a] if rng.random() < 0.5 else lo[a] - outward_cells * cell[a]
    return p


def aimed_ray(rng, target, origin):
    """The fp32 ray from `origin` through `target`: d = target - origin, scaled by a power of two (so that t at the target stays
    within 2^-3 .. 2^3); the roundings of both move the ray, which is why labels come from the exact ray."""
    o = np.asarray(origin, dtype=f32)
    d = ((np.asarray(target, dtype=np.float64) - o.astype(np.float64)) * 2.0 ** int(rng.integers(-3, 4))).astype(f32)
    return o, d


def random_unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


DISTANCES = (0.0, 1e-2, 1.0, 10.0, 1e2, 1e3, 1e4)      # of a ray origin from its target, in node extents; 0: inside the box


def origin_for(node, rng, target, k):
    lo, hi = node.lo_hi_f64()
    if DISTANCES[k % len(DISTANCES)] == 0.0:
        return lo + rng.uniform(0.05, 0.95, 3) * (hi - lo)
    return target + random_unit(rng) * DISTANCES[k % len(DISTANCES)] * float(np.max(hi - lo))


def gen_grazing(rng, k):
    node = moderate_node(rng, k % 4)
    tri = triangle_in(node, rng)
    if (k // 4) % 2 == 0:
        out = -rng.choice([0.0, 1e-3, 0.02, 0.3])                        # accept side: on the geometry box or slightly inside
        target = point_on(tri, rng) if k % 5 == 4 else boundary_target(node, rng, out)      # every fifth at the triangle itself
        origin = origin_for(node, rng, target, k // 8)
    else:                                                                # reject side: outward 0..3 cells and the margin's share of L
        target = boundary_target(node, rng, 0.0)
        origin = origin_for(node, rng, target, k // 8)
        dist = float(np.linalg.norm(origin - target))
        target = boundary_target(node, rng, rng.uniform(0.0, 3.0) + rng.uniform(0.0, 4e-5) * dist / float(node.scales.min()))
    o, d = aimed_ray(rng, target, origin)
    return Case(ONE, o, d, 0.001, 1e4, node, tri)


SMALL_DIRS = (0.0, -0.0, 1e-45, -3e-42, 1e-35, -1e-35, 1e-29, -1e-29)      # zeros, denormals, below and above box_dir's 2^-100


def gen_axis(rng, k):
    node = moderate_node(rng, k % 4)
    lo, hi = node.lo_hi_f64()
    cell = node.scales.astype(np.float64)
    small = rng.permutation(3) < (1 + (k // 4) % 2)                      # one or two components
    tri = triangle_in(node, rng)
    inside = point_on(tri, rng) if k % 2 else lo + rng.uniform(0.05, 0.95, 3) * (hi - lo)
    u = random_unit(rng)
    o64 = inside - u * rng.uniform(1.5, 10.0) * float(np.max(hi - lo))
    d = u.astype(f32)
    o = o64.astype(f32)
    where = (k // 8) % 3                                                 # on a decoded plane, inside the slab, outside it
    for a in range(3):
        if not small[a]:
            continue
        d[a] = f32(rng.choice(SMALL_DIRS))
        upper = rng.random() < 0.5
        plane = tbr.decode(node.q_hi[a] if upper else node.q_lo[a], node.scales[a], node.origin[a])
        if where == 0:
            o[a] = plane
        elif where == 1:
            o[a] = f32(inside[a])
        else:
            o[a] = f32(float(plane) + (1 if upper else -1) * rng.choice([0.3, 1.0, 3.0]) * cell[a])
    return Case(ONE, o, d, 0.001, 1e4, node, tri)


SCALE_EXPONENTS = (-126, -60, -10, 0, 42)


def gen_scales(rng, k):
    c = k % 4
    mixed = (k // 4) % 2 == 1
    e = rng.choice(SCALE_EXPONENTS, size=3) if mixed else np.repeat(rng.choice(SCALE_EXPONENTS), 3)
    s = np.ldexp(1.0, e)
    pattern = (k // 8) % 5
    q_lo, q_hi = [(np.zeros(3, int), np.full(3, 255)), (np.zeros(3, int), np.ones(3, int)), (np.full(3, 254), np.full(3, 255)),
                  (None, None), (None, None)][pattern]
    if q_lo is None:
        q_lo = rng.integers(0, 255, size=3)
        q_hi = q_lo + 1 if pattern == 3 else np.minimum(q_lo + rng.integers(1, 100, size=3), 255)
    origin_kind = (k // 40) % 4
    if origin_kind == 0:
        origin = np.zeros(3)
    elif origin_kind == 1:
        origin = np.floor(rng.uniform(-1.0, 1.0, size=3) * np.minimum(2.0 ** 20, 2.0 ** 44 / s)) * s    # on the grid: the planes are fp32 numbers
    elif origin_kind == 2:
        origin = np.where(e >= 22, rng.choice([-1.0, 1.0], size=3) * 2.0 ** 44, rng.integers(-(1 << 22), 1 << 22, size=3) * s)   # up to 2^44
    else:
        origin = (rng.uniform(-1.0, 1.0, size=3) * np.minimum(3000.0, 2.0 ** 44 / s) * np.maximum(s, 2.0 ** -100)).astype(f32)   # off the grid, as the builders place it
    node = Node(np.clip(origin, -3e38, 3e38), s, c, q_lo, q_hi)
    side = (k // 160) % 2
    tri = triangle_in(node, rng)
    target = boundary_target(node, rng, -rng.choice([0.0, 0.02, 0.3]) if side == 0 else rng.uniform(0.3, 3.0))
    if side == 0 and k % 3 == 2:
        target = point_on(tri, rng)
    lo, hi = node.lo_hi_f64()
    dist = (0.0, 1.0, 100.0)[(k // 320) % 3]
    origin_pt = lo + rng.uniform(0.05, 0.95, 3) * (hi - lo) if dist == 0.0 else target + random_unit(rng) * dist * float(np.max(hi - lo))
    o = origin_pt.astype(f32)
    d64 = target - o.astype(np.float64)
    m = float(np.max(np.abs(d64)))
    if m > 0:                                                            # a direction of ordinary size: the largest component in [1, 2)
        d64 = np.ldexp(d64, -math.frexp(m)[1] + 1)
    return Case(ONE, o, d64.astype(f32), (-1.0, 0.0)[(k // 4) % 2], 1e4, node, tri)


def gen_bounds(rng, k):
    node = moderate_node(rng, k % 4)
    lo, hi = node.lo_hi_f64()
    tri = triangle_in(node, rng)
    inside = point_on(tri, rng) if k % 2 else lo + rng.uniform(0.05, 0.95, 3) * (hi - lo)
    u = random_unit(rng)
    ext = float(np.max(hi - lo))
    tau = rng.choice([-3.0, -1.5, -0.7, 0.0, 0.7, 1.5, 3.0, 40.0])       # where the box sits along the ray, in extents
    o = (inside - u * tau * ext).astype(f32)
    d = (u * ext).astype(f32)                                            # the box is about one unit of t long
    tmin = (-1.0, 0.0, 0.001, 0.5)[(k // 4) % 4]
    g = ray_box_interval(fr3(o), fr3(d), *node.box.decoded())
    tmax_kind = (k // 16) % 4
    tmax = (1e4, 3e38)[tmax_kind % 2] if tmax_kind < 2 or g is None or g[0] <= 0 else \
        float(g[0]) * (1.0 + (-1 if tmax_kind == 2 else 1) * rng.choice([3e-7, 1e-5, 3e-4, 1e-2]))     # ends just short of / just past the box
    return Case(ONE, o, d, tmin, tmax, node, tri)


def gen_inverted(rng, k):
    node = moderate_node(rng, k % 4)
    inv = rng.permutation(3) < rng.integers(1, 4)
    node = Node(node.origin, node.scales, node.c, np.where(inv, 255, node.q_lo), np.where(inv, 0, node.q_hi))
    full = Node(node.origin, node.scales, node.c, [0, 0, 0], [255, 255, 255])
    lo, hi = full.lo_hi_f64()
    target = lo + rng.uniform(0.0, 1.0, 3) * (hi - lo)
    dist = (0.0, 1e-2, 1.0, 10.0, 1e2, 1e3)[(k // 4) % 6]
    origin = lo + rng.uniform(0.0, 1.0, 3) * (hi - lo) if dist == 0.0 else target + random_unit(rng) * dist * float(np.max(hi - lo))
    o, d = aimed_ray(rng, target, origin)
    return Case(ONE, o, d, (-1.0, 0.0, 0.001)[(k // 24) % 3], (1e4, 3e38)[(k // 72) % 2], node, triangle_in(full, rng))


def gen_nonfinite(rng, k):
    case = gen_grazing(rng, k)
    bad = f32([np.nan, np.inf, -np.inf][(k // 4) % 3])
    which = rng.permutation(6) < rng.integers(1, 4)                      # one to three of the six components
    for a in range(3):
        if which[a]:
            case.o[a] = bad
        if which[3 + a]:
            case.d[a] = bad
    case.finite = False
    return case


def _translation(t):
    m = IDENTITY.copy()
    m[[3, 7, 11]] = t
    return m


def _linear(a, t=(0, 0, 0)):
    m = np.zeros(12, dtype=f32)
    m.reshape(3, 4)[:, :3] = np.asarray(a, dtype=f32)
    m[[3, 7, 11]] = t
    return m


def _rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q


def _shear(k):
    return [[1, k, 0], [0, 1, 0], [0, 0, 1]]


@functools.lru_cache(None)
def largest_unbaked_shear():
    """The largest fp32 k for which the instance transform [[1, k, 0], [0, 1, 0], [0, 0, 1]] is still not baked."""
    from sunray_amd import runtime
    baked = lambda k: runtime.probe_tl_record(_linear(_shear(k)), [0, 0, 0], [1, 1, 1])[1] == abi.TL_RECORD_BAKED
    lo, hi = f32(1.0), f32(64.0)
    assert not baked(lo) and baked(hi)
    while np.nextafter(lo, hi) < hi:
        mid = f32((float(lo) + float(hi)) / 2)
        lo, hi = (lo, mid) if baked(mid) else (mid, hi)
    return lo


def instance_transform(rng, k):
    """The o2w forms of the two-level class, by turn; those past the baking limit come out baked and join the baked class."""
    turn = k % 10
    far = rng.uniform(-1.0, 1.0, 3) * 2.0 ** rng.integers(0, 21)
    if turn == 0:
        return IDENTITY.copy()
    if turn == 1:
        return _translation(far)
    if turn == 2:
        return _linear(_rotation(rng), far if rng.random() < 0.5 else (0, 0, 0))
    if turn == 3:
        return _linear(np.eye(3) * 10.0 ** rng.uniform(-3, 3), rng.uniform(-10, 10, 3))                  # uniform scale
    if turn == 4:
        return _linear(np.diag(10.0 ** rng.uniform(-0.9, 0.9, 3)))                                       # non-uniform, below the limit
    if turn == 5:
        return _linear(np.diag(10.0 ** rng.uniform(-3, 3, 3)))                                           # non-uniform 1e-3 .. 1e3: mostly baked
    if turn == 6:
        return _linear(_rotation(rng) @ np.diag(10.0 ** rng.uniform(-0.9, 0.9, 3)), rng.uniform(-100, 100, 3))
    if turn == 7:
        return _linear(_shear(rng.choice([0.0, 9.0, 99.0])))                                             # condition 1, 1e2, 1e4
    if turn == 8:
        return _linear(_shear(largest_unbaked_shear()), rng.uniform(-10, 10, 3) if rng.random() < 0.5 else (0, 0, 0))
    return _linear(_rotation(rng) @ np.array(_shear(rng.uniform(0.0, 8.0))), far)


def tl_record_of(o2w, node, tri):
    """The instance record the library writes for this transform over a mesh whose root box is the node's decoded box."""
    from sunray_amd import runtime
    lo, hi = node.box.decoded()
    e1, e2 = tri[1] - tri[0], tri[2] - tri[0]
    rec, res = runtime.probe_tl_record(o2w, [float(x) for x in lo], [float(x) for x in hi], float(np.max(np.abs(tri))),
                                       float(np.max(np.abs(e1) + np.abs(e2))))
    return rec, res


def gen_instances(rng, k):
    """Two-level, mesh node under test. The ray is made in object space like a grazing ray and taken to world space in float64;
    world-space origins reach 1e6 through the translations. Instances past the baking limit get a world-space node instead."""
    o2w = instance_transform(rng, k // 4)
    node = moderate_node(rng, k % 4)
    tri = triangle_in(node, rng)
    rec, res = tl_record_of(o2w, node, tri)
    if res == abi.TL_RECORD_BAKED:
        case = gen_grazing(rng, k)                  # the mesh node is in world space and the ray is not transformed
        return Case(TL_BAKED, case.o, case.d, 0.001, 1e4, case.node, case.tri, o2w)
    m = o2w.astype(np.float64).reshape(3, 4)
    side = (k // 40) % 2
    pad_cells = 0.0
    if side == 0:
        target = point_on(tri, rng) if k % 5 == 4 else boundary_target(node, rng, -rng.choice([0.0, 1e-3, 0.02, 0.3]))
        origin = origin_for(node, rng, target, k // 80)
    else:
        target = boundary_target(node, rng, 0.0)
        origin = origin_for(node, rng, target, k // 80)
        world_o = m[:, :3] @ origin + m[:, 3]
        pad = float(rec["pad_a"]) * float(np.max(np.abs(world_o))) + float(rec["pad_b"])
        dist = float(np.linalg.norm(origin - target))
        pad_cells = (rng.uniform(0.0, 3.0) * pad + rng.uniform(0.0, 4e-5) * dist) / float(node.scales.min())
        target = boundary_target(node, rng, rng.uniform(0.0, 3.0) + pad_cells)
    o = (m[:, :3] @ origin + m[:, 3]).astype(f32)
    d = ((m[:, :3] @ (target - origin)) * 2.0 ** int(rng.integers(-3, 4))).astype(f32)
    return Case(TL_MESH, o, d, 0.001, 1e4, node, tri, o2w)


GENERATORS = {"grazing": gen_grazing, "axis": gen_axis, "scales": gen_scales, "bounds": gen_bounds, "inverted": gen_inverted,
              "nonfinite": gen_nonfinite}
SEEDS = {"grazing": 101, "axis": 202, "scales": 303, "bounds": 404, "inverted": 505, "nonfinite": 606, "instances": 707}
BATCH, MAX_BATCHES = 512, 24


# ---- rows -----------------------------------------------------------------------------------------------------------------------
class RowSet:
    """The rows of one class in one form, packed and labelled. rows: abi.NODE_PROBE_ROW; label: ACCEPT / REJECT / FREE per row from
    the boxes alone (reported hits are added by expected()); boxes: the exact `boxes` counter where the labels fix it, else 0;
    cases: the unpacked rows (profiles); counts: accept, reject, free."""

    def __init__(self, name, cases):
        self.name, self.cases = name, cases
        self.rows = np.zeros(len(cases), dtype=abi.NODE_PROBE_ROW)
        self.label = np.zeros(len(cases), dtype=np.int8)
        self.boxes = np.zeros(len(cases), dtype=np.uint32)
        self.finite = np.array([c.finite for c in cases], dtype=bool)
        for i, c in enumerate(cases):
            self._pack(i, c)

    def _pack(self, i, c):
        r = self.rows[i]
        r["origin"], r["dir"], r["tmin"], r["tmax"] = c.o, c.d, c.tmin, c.tmax
        gid = np.uint32(7 + i % 1000)
        tri = c.tri
        if c.form == ONE:
            rec = np.concatenate([tri[0], tri[1] - tri[0], tri[2] - tri[0]]).astype(f32)      # v0, e1, e2
        else:
            rec = tri.reshape(9)                                                              # v0, v1, v2
        r["tri"][:9] = rec.view(np.uint32)
        r["tri"][9] = gid
        if not c.finite:
            r["node"] = c.node.words()
            if c.form != ONE:
                r["mesh_node"] = covering_node(c.node.c, [1.0]).words()
                r["instance"] = np.frombuffer(tl_record_of(IDENTITY, c.node, tri)[0].tobytes(), dtype=np.uint32)
            return
        o, d, tmin, tmax = fr3(c.o), fr3(c.d), fr(c.tmin), fr(c.tmax)
        if c.form == ONE:
            r["node"] = c.node.words()
            self.label[i] = label_box(o, d, tmin, tmax, c.node.box)
            self.boxes[i] = 4
            return
        lo, hi = c.node.box.decoded()
        reach = [float(x) for x in c.o] + [float(x) for x in lo] + [float(x) for x in hi]
        if c.form == TL_TOP:                                                  # the top-level node under test, a covering mesh node below
            other = covering_node((c.node.c + 1) % 4, reach)
            r["node"], r["mesh_node"] = c.node.words(), other.words()
            rec, res = tl_record_of(IDENTITY, other, tri)
            assert res == abi.TL_RECORD_OK
            top = label_box(o, d, tmin, tmax, c.node.box)
            below = label_box(o, d, tmin, tmax, other.box)
            self.label[i] = top if top != ACCEPT else (ACCEPT if below == ACCEPT else FREE)
            self.boxes[i] = {ACCEPT: 8, REJECT: 4, FREE: 0}[top]
        else:                                                                 # the mesh node under test, a covering top-level node above
            rec, res = tl_record_of(c.o2w, c.node, tri)
            assert (res == abi.TL_RECORD_BAKED) == (c.form == TL_BAKED) and res != abi.TL_RECORD_NO_FINITE_BOX
            if c.form == TL_BAKED:
                oo, od, extra = o, d, Fraction(0)
                world = reach
            else:
                oo, od = object_ray(c.o2w, o, d)
                extra = fr(rec["pad_a"]) * max(abs(x) for x in o) + fr(rec["pad_b"])
                m = c.o2w.astype(np.float64).reshape(3, 4)
                corners = [[float(x) for x in (lo[0], hi[0])], [float(x) for x in (lo[1], hi[1])], [float(x) for x in (lo[2], hi[2])]]
                world = [float(x) for x in c.o] + [float(v) for i0 in (0, 1) for i1 in (0, 1) for i2 in (0, 1)
                                                   for v in m[:, :3] @ np.array([corners[0][i0], corners[1][i1], corners[2][i2]]) + m[:, 3]]
            other = covering_node((c.node.c + 1) % 4, world)
            r["node"], r["mesh_node"] = other.words(), c.node.words()
            above = label_box(o, d, tmin, tmax, other.box)
            mesh = label_box(oo, od, tmin, tmax, c.node.box, extra)
            self.label[i] = mesh if above == ACCEPT else (REJECT if above == REJECT else FREE)
            self.boxes[i] = {ACCEPT: 8, REJECT: 4, FREE: 0}[above]
        r["instance"] = np.frombuffer(rec.tobytes(), dtype=np.uint32)

    @staticmethod
    def merged(name, parts):
        rs = RowSet(name, [])
        rs.cases = [c for p in parts for c in p.cases]
        for f in ("rows", "label", "boxes", "finite"):
            setattr(rs, f, np.concatenate([getattr(p, f) for p in parts]))
        return rs

    def counts(self):
        return int((self.label == ACCEPT).sum()), int((self.label == REJECT).sum()), int((self.finite & (self.label == FREE)).sum())


def _as_top(case):
    c = Case(TL_TOP, case.o, case.d, case.tmin, case.tmax, case.node, case.tri)
    c.finite = case.finite
    return c


def _enough(name, parts):
    acc = sum(p.counts()[0] for p in parts)
    rej = sum(p.counts()[1] for p in parts)
    return rej >= MIN_PER_LABEL and (acc >= MIN_PER_LABEL or name.endswith("inverted"))


@functools.lru_cache(None)
def _build(base, top):
    """The generator `base` run from its fixed seed, batch after batch, until every class it feeds keeps MIN_PER_LABEL ACCEPT rows
    and MIN_PER_LABEL REJECT rows (inverted: REJECT only; nonfinite: one batch, no labels). -> {class name: RowSet}"""
    rng = np.random.default_rng(SEEDS[base])
    gen = gen_instances if base == "instances" else GENERATORS[base]
    names = ("instances", "baked") if base == "instances" else (("top_" if top else "") + base,)
    parts = {n: [] for n in names}
    for b in range(MAX_BATCHES):
        made = [gen(rng, k) for k in range(b * BATCH, (b + 1) * BATCH)]
        if top:
            made = [_as_top(c) for c in made]
        if base == "instances":
            groups = {"instances": [c for c in made if c.form == TL_MESH], "baked": [c for c in made if c.form == TL_BAKED]}
        else:
            groups = {names[0]: made}
        for n, g in groups.items():
            parts[n].append(RowSet(n, g))
        if base == "nonfinite" or all(_enough(n, parts[n]) for n in names):
            break
    return {n: RowSet.merged(n, parts[n]) for n in names}


def row_set(name):
    """The rows of one class of CLASSES."""
    if name in ("instances", "baked"):
        return _build("instances", False)[name]
    top = name.startswith("top_")
    return _build(name[4:] if top else name, top)[name]


# ---- expected hits --------------------------------------------------------------------------------------------------------------
def expected(rs, oracle):
    """(hit[n] bool, gid, t, u, v as uint32 bits [n, 4]) of every row's triangle as the device must report it IF the leaf is
    reached, from the oracle's bit-exact helpers: transform_point for the world-space vertices of the two-level form (not of a
    baked instance), then intersect_tri. Where it reports a hit the row is ACCEPT whatever its boxes say."""
    n = len(rs.rows)
    tri = rs.rows["tri"][:, :9].copy().view(f32).reshape(n, 3, 3)
    forms = np.array([c.form for c in rs.cases])
    if n and forms[0] != ONE:
        xf = (forms == TL_MESH) | (forms == TL_TOP)
        m = rs.rows["instance"][:, 12:24]
        for j in range(3):
            rows = np.concatenate([m, tri[:, j, :].copy().view(np.uint32)], axis=1).astype(np.uint32)
            w = oracle.probe_helper(hp.IDS["transform_point"], rows).view(f32).reshape(n, 3)
            tri[xf, j, :] = w[xf]
        v0, e1, e2 = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    else:
        v0, e1, e2 = tri[:, 0], tri[:, 1], tri[:, 2]
    cols = np.concatenate([rs.rows["origin"], rs.rows["dir"], v0, e1, e2, rs.rows["tmin"][:, None], rs.rows["tmax"][:, None]], axis=1)
    out = oracle.probe_helper(hp.IDS["intersect_tri"], np.ascontiguousarray(cols.astype(f32)).view(np.uint32).reshape(n, 17))
    hit = out[:, 0] != 0
    bits = np.stack([rs.rows["tri"][:, 9], out[:, 1], out[:, 2], out[:, 3]], axis=1)
    return hit, bits
