"""A plain reference of the device tree builder (csrc/bvh_device.h, bvh_gpu.hip, blas_batch.hip), stage by stage, in numpy float32
and Python integers: padded primitive boxes, Morton keys, the stable sort, the binary topology (radix tree after Karras 2012, or
PLOC after Meister & Bittner 2018), binary sizes and walk heights, the height bound, the collapse to 4-wide nodes with its leaf
slots, and the quantisation of every node. It is written from the papers and from the rules the headers state in prose, with
trees as linked Python objects and recursion where the rule is recursive: no parent or flag arrays, no counters, no second walks.

Everything the builder computes is a deterministic function of its input except the numbers nodes get, so `canonical` renumbers a
4-wide tree breadth-first in child order, and two trees that are equal up to numbering become equal arrays.

Constants (node layout, primitives per leaf, stack floors and caps) are arguments: the tests read them from the library."""
import math
import sys
from fractions import Fraction

import numpy as np

f32 = np.float32
F_INF = f32(np.inf)
UNUSED = 0xFFFFFFFF
SCALE_DWORDS = (3, 10, 11)      # the grid scale of x, y, z (csrc/bvh_layout.h; runtime.decode_node reads the same three)
GUARD = Fraction(1, 32)         # guard band around every quantised plane, in cells


class Layout:
    """Node layout and leaf size the reference builds for: runtime.bvh_layout() and runtime.tree_build_limits()."""

    def __init__(self, width, node_dwords, plane_offset, child_offset, leaf_max):
        self.width, self.node_dwords, self.plane_offset, self.child_offset, self.leaf_max = width, node_dwords, plane_offset, child_offset, leaf_max
        self.plane_dwords = width // 4


def deep_recursion():
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 20000))


# ---- primitive boxes --------------------------------------------------------------------------------------------------------
def _padded(lo, hi, e1, e2):
    pad = f32(4e-6) * (np.abs(e1) + np.abs(e2))
    return np.nextafter(lo - pad, -F_INF), np.nextafter(hi + pad, F_INF)


def boxes_of_edge_records(v0, e1, e2):
    """Padded boxes of (v0, e1, e2) triangle records, [n, 3] float32 each -> (lo, hi)."""
    v0, e1, e2 = (np.asarray(x, dtype=f32) for x in (v0, e1, e2))
    p1, p2 = v0 + e1, v0 + e2
    return _padded(np.minimum(v0, np.minimum(p1, p2)), np.maximum(v0, np.maximum(p1, p2)), e1, e2)


def boxes_of_vertex_records(v0, v1, v2):
    """Padded boxes of (v0, v1, v2) mesh records: the edge record's box with e = v - v0, and the vertices themselves."""
    v0, v1, v2 = (np.asarray(x, dtype=f32) for x in (v0, v1, v2))
    e1, e2 = v1 - v0, v2 - v0
    p1, p2 = v0 + e1, v0 + e2
    lo = np.minimum(np.minimum(v0, np.minimum(p1, p2)), np.minimum(v1, v2))
    hi = np.maximum(np.maximum(v0, np.maximum(p1, p2)), np.maximum(v1, v2))
    return _padded(lo, hi, e1, e2)


def centres(lo, hi):
    return f32(0.5) * np.asarray(lo, dtype=f32) + f32(0.5) * np.asarray(hi, dtype=f32)


# ---- Morton keys and the sort -------------------------------------------------------------------------------------------------
def grid_bounds(lo, hi, has_box=None):
    """Union of the boxes (of the rows that have one)."""
    if has_box is not None:
        lo, hi = lo[has_box], hi[has_box]
    return lo.min(axis=0), hi.max(axis=0)


def interleave(qx, qy, qz):
    key = 0
    for bit in range(21):
        key |= ((qx >> bit) & 1) << (3 * bit) | ((qy >> bit) & 1) << (3 * bit + 1) | ((qz >> bit) & 1) << (3 * bit + 2)
    return key


def morton_keys(points, g_lo, g_hi, has_box=None):
    """63-bit keys of float32 points in the grid [g_lo, g_hi], as Python integers; 2^64 - 1 for a row without a box."""
    points = np.asarray(points, dtype=f32)
    ext = (g_hi - g_lo).astype(f32)
    q = np.zeros(points.shape, dtype=np.int64)
    for a in range(3):
        if ext[a] > 0:
            with np.errstate(invalid="ignore"):
                t = (points[:, a] - g_lo[a]) / ext[a]
            t = np.where(np.isnan(t), f32(0), t)
            t = np.minimum(np.maximum(t, f32(0)), f32(1)).astype(f32)
            q[:, a] = np.minimum((t * f32(2097152.0)).astype(np.int64), 2097151)
    keys = [interleave(int(x), int(y), int(z)) for x, y, z in q]
    if has_box is not None:
        keys = [k if ok else (1 << 64) - 1 for k, ok in zip(keys, has_box)]
    return keys


def stable_order(keys):
    """Indices in ascending key order, equal keys in index order."""
    return sorted(range(len(keys)), key=lambda i: keys[i])


# ---- binary trees ---------------------------------------------------------------------------------------------------------------
class Bin:
    """A binary subtree: a single primitive (`pos`, its position in the sorted order) or two children. Box, size and the height of a
    purely binary walk (0 for a subtree that becomes a leaf) follow from the children."""
    __slots__ = ("left", "right", "pos", "size", "height", "lo", "hi")

    def __init__(self, left=None, right=None, pos=None, box=None, leaf_max=None):
        self.left, self.right, self.pos = left, right, pos
        if pos is not None:
            self.size, self.height, (self.lo, self.hi) = 1, 0, box
        else:
            self.size = left.size + right.size
            self.height = 0 if self.size <= leaf_max else 1 + max(left.height, right.height)
            self.lo, self.hi = np.minimum(left.lo, right.lo), np.maximum(left.hi, right.hi)

    def leaves(self):
        """Sorted positions below, depth first, left before right."""
        if self.pos is not None:
            return [self.pos]
        return self.left.leaves() + self.right.leaves()

    def area(self):
        d = self.hi - self.lo
        return d[0] * d[1] + d[1] * d[2] + d[2] * d[0]


def leaf_bins(lo, hi):
    return [Bin(pos=i, box=(lo[i], hi[i])) for i in range(len(lo))]


def radix_split(aug, first, last):
    """Where the range [first, last] of distinct ascending integers splits: the first element whose highest bit that differs
    between the range's ends is set."""
    bit = (aug[first] ^ aug[last]).bit_length() - 1
    s = first + 1
    while not (aug[s] >> bit) & 1:
        s += 1
    return s


def radix_tree(sorted_keys, bins, leaf_max):
    """Top-down: a range of the sorted (key, index) pairs splits where their highest differing bit changes."""
    deep_recursion()
    aug = [(k << 32) | i for i, k in enumerate(sorted_keys)]

    def build(first, last):
        if first == last:
            return bins[first]
        s = radix_split(aug, first, last)
        return Bin(build(first, s - 1), build(s, last), leaf_max=leaf_max)
    return build(0, len(aug) - 1)


def union_areas(boxes, i, j):
    """Surface measure dx*dy + dy*dz + dz*dx of the union of boxes i and j (index arrays), float32."""
    d = np.maximum(boxes[i, 3:], boxes[j, 3:]) - np.minimum(boxes[i, :3], boxes[j, :3])
    return d[..., 0] * d[..., 1] + d[..., 1] * d[..., 2] + d[..., 2] * d[..., 0]


def ploc_neighbours(boxes, radius, spread_ties):
    """The neighbour of every cluster within `radius` positions whose union with it is smallest. Ties: the lowest index; under
    `spread_ties` the nearest in the order, of two at the same distance the partner i ^ 1, then the lowest index."""
    m = len(boxes)
    r = min(radius, m - 1)
    off = np.concatenate([np.arange(-r, 0), np.arange(1, r + 1)])
    i = np.arange(m)[:, None]
    j = i + off[None, :]
    ok = (j >= 0) & (j < m)
    jc = np.clip(j, 0, m - 1)
    area = np.where(ok, union_areas(boxes, np.broadcast_to(i, jc.shape), jc), F_INF)
    assert np.isfinite(area[ok]).all()
    best = area.min(axis=1, keepdims=True)
    if spread_ties:
        rank = 2 * np.abs(off)[None, :] + np.where(jc == (i ^ 1), 0, 1)
        pick = np.where(area == best, rank, 1 << 40).argmin(axis=1)
    else:
        pick = (area == best).argmax(axis=1)
    return jc[np.arange(m), pick]


def ploc_iteration(clusters, boxes, radius, spread_ties, leaf_max):
    """One iteration: mutual nearest neighbours merge into the lower position, children (lower, higher); the rest keep their order."""
    nn = ploc_neighbours(boxes, radius, spread_ties)
    out, out_boxes, merged = [], [], 0
    for i, c in enumerate(clusters):
        j = int(nn[i])
        if int(nn[j]) != i:
            out.append(c); out_boxes.append(boxes[i])
        elif i < j:
            b = Bin(c, clusters[j], leaf_max=leaf_max)
            out.append(b); out_boxes.append(np.concatenate([b.lo, b.hi]))
            merged += 1
    return out, np.array(out_boxes, dtype=f32), nn, merged


def ploc_tree(bins, radius, spread_ties, leaf_max):
    clusters = list(bins)
    boxes = np.array([np.concatenate([b.lo, b.hi]) for b in bins], dtype=f32)
    while len(clusters) > 1:
        clusters, boxes, _, merged = ploc_iteration(clusters, boxes, radius, spread_ties, leaf_max)
        assert merged >= 1
    return clusters[0]


# ---- height bound -----------------------------------------------------------------------------------------------------------------
def median_height(k, leaf_max):
    """H(k): walk height of the median-split tree over k primitives."""
    h = 0
    while k > leaf_max:
        k, h = (k + 1) // 2, h + 1
    return h


def median_tree(leaves, leaf_max):
    """Over leaves lo .. hi - 1 the split falls behind position lo + ceil((hi - lo) / 2) - 1: the left half takes the odd one."""
    if len(leaves) == 1:
        return leaves[0]
    k = (len(leaves) + 1) // 2
    return Bin(median_tree(leaves[:k], leaf_max), median_tree(leaves[k:], leaf_max), leaf_max=leaf_max)


def single_leaves(node):
    if node.pos is not None:
        return [node]
    return single_leaves(node.left) + single_leaves(node.right)


def bound_height(root, cap, leaf_max):
    """-> (tree, subtrees rebuilt, primitives in them, the sorted positions of each). Allowance A = cap at the root, one less per level; a subtree with
    h <= A is kept whole; a split whose children both satisfy H(size) <= A - 1 is kept; otherwise the subtree is rebuilt as the
    median-split tree over its own leaves in depth-first order."""
    deep_recursion()
    stat = [0, 0]

    def rule(node, allowance):
        if node.height <= allowance:
            return node
        if all(median_height(c.size, leaf_max) <= allowance - 1 for c in (node.left, node.right)):
            return Bin(rule(node.left, allowance - 1), rule(node.right, allowance - 1), leaf_max=leaf_max)
        stat[0] += 1; stat[1] += node.size
        rebuilt.append(node.leaves())
        return median_tree(single_leaves(node), leaf_max)
    rebuilt = []
    return rule(root, cap), stat[0], stat[1], rebuilt


# ---- collapse to wide nodes ----------------------------------------------------------------------------------------------------
class Wide:
    """One 4-wide node: per child either a Wide or (first slot, [sorted positions in slot order])."""
    __slots__ = ("children",)

    def __init__(self, children):
        self.children = children


def collapse(root, budget, layout):
    """-> (Wide root, order: sorted position per leaf slot, max_stack). The inner child of largest area is opened (the first on
    ties) while every child's need + nk <= budget, nk the children before the opening; a child's budget is budget - (nk - 1).
    Slots follow child order, depth first."""
    deep_recursion()
    order, deepest = [], [0]

    def inner(k):
        return k.size > layout.leaf_max

    def node(b, budget, prefix):
        kids = [b.left, b.right]
        while len(kids) < layout.width:
            best = None
            for i, k in enumerate(kids):
                if inner(k) and (best is None or k.area() > kids[best].area()):
                    best = i
            if best is None:
                break
            nk = len(kids)
            after = kids[:best] + [kids[best].left] + kids[best + 1:] + [kids[best].right]
            if any(k.height + nk > budget for k in after):
                break
            kids = after
        mine = prefix + len(kids) - 1
        deepest[0] = max(deepest[0], mine)
        children = []
        for k in kids:
            if inner(k):
                children.append(node(k, budget - (len(kids) - 1), mine))
            else:
                children.append((len(order), k.leaves()))
                order.extend(k.leaves())
        return Wide(children)
    return node(root, budget, 0), order, deepest[0]


def single_primitive_tree():
    return Wide([(0, [0])]), [0], 0


def emit(wide_root, layout):
    """The node array of a Wide tree, numbered breadth-first in child order (the canonical numbering), child words only."""
    nodes, queue = [], [wide_root]
    for w in queue:      # grows while it runs
        row = np.zeros(layout.node_dwords, dtype=np.uint32)
        row[layout.child_offset:layout.child_offset + layout.width] = UNUSED
        for c, child in enumerate(w.children):
            if isinstance(child, Wide):
                queue.append(child)
                row[layout.child_offset + c] = len(queue) - 1
            else:
                first, prims = child
                row[layout.child_offset + c] = ~((first << 3) | len(prims)) & 0xFFFFFFFF
        nodes.append(row)
    return np.array(nodes, dtype=np.uint32)


# ---- node quantisation ----------------------------------------------------------------------------------------------------------
def round_to_f32(x):
    """A Fraction rounded once to float32 (nearest, ties to even; overflow to infinity)."""
    if x == 0:
        return f32(0)
    sign, x = (-1, -x) if x < 0 else (1, x)
    e = x.numerator.bit_length() - x.denominator.bit_length()
    if Fraction(2) ** e > x:
        e -= 1
    q = max(e, -126) - 23
    m = x / Fraction(2) ** q
    n = m.numerator // m.denominator
    rest = m - n
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and n & 1):
        n += 1
    v = Fraction(n) * Fraction(2) ** q
    if v >= Fraction(2) ** 128:
        return sign * F_INF
    return f32(sign * float(v))


def _sum_if_exact(a, b):
    """a + b in float64 where that sum is exact (two-sum leaves no error), else None."""
    s = a + b
    if not math.isfinite(s):
        return None
    bb = s - a
    return s if (a - (s - bb)) + (b - bb) == 0.0 else None


def decode(q, scale, origin):
    """fma(q, scale, origin) in float32: the product and the sum exactly, rounded once. q * scale is exact in float64; where the
    float64 sum is exact too, its rounding to float32 is the single rounding, otherwise fractions do it."""
    s = _sum_if_exact(float(q) * float(scale), float(origin))
    if s is not None:
        return f32(s)
    return round_to_f32(Fraction(q) * Fraction(float(scale)) + Fraction(float(origin)))


def cells(x, origin, scale, guard=0.0):
    """(x - origin) / scale + guard exactly, as a float64 where every step is exact (the division is by a power of two), else as
    a Fraction."""
    d = _sum_if_exact(float(x), -float(origin))
    if d is not None:
        t = _sum_if_exact(d / float(scale), float(guard))
        if t is not None:
            return t
    return (Fraction(float(x)) - Fraction(float(origin))) / Fraction(float(scale)) + Fraction(guard)


def upper_plane(hi, origin, scale, limit):
    """The lowest q >= 0 with the guard band above hi whose decoded plane is not below hi, searched up to `limit`."""
    q = max(math.ceil(cells(hi, origin, scale, float(GUARD))), 0)
    while q <= limit and decode(q, scale, origin) < hi:
        q += 1
    return q


def lower_plane(lo, origin, scale):
    q = min(max(math.floor(cells(lo, origin, scale, -float(GUARD))), 0), 255)
    while q > 0 and decode(q, scale, origin) > lo:
        q -= 1
    return q


def grid_scale(e):
    return f32(math.ldexp(1.0, e))


def axis_origin(lo_n, hi_n):
    return np.nextafter(f32(lo_n - (hi_n - lo_n) / f32(2048.0)), -F_INF)


def axis_exponent(origin, hi_n, child_hi):
    """The smallest e >= frexp(ext / 255), at least -126, at which every child's upper plane fits in a byte; ext = hi_n - origin."""
    with np.errstate(over="ignore", invalid="ignore"):
        ext = f32(hi_n - origin)
    if not ext < F_INF:
        return 127
    e = -126
    if ext > 0 and f32(ext / f32(255.0)) > 0:
        e = max(math.frexp(float(f32(ext / f32(255.0))))[1], -126)
    while e < 127 and any(upper_plane(h, origin, grid_scale(e), 255) > 255 for h in child_hi):
        e += 1
    return e


def quantise_axis(lo_n, hi_n, child_lo, child_hi):
    """-> (origin, e, [ql], [qh]) of one axis of a node with these real children."""
    origin = axis_origin(lo_n, hi_n)
    e = axis_exponent(origin, hi_n, child_hi)
    scale = grid_scale(e)
    ql = [lower_plane(l, origin, scale) for l in child_lo]
    qh = [min(upper_plane(h, origin, scale, 254), 255) for h in child_hi]
    return origin, e, ql, qh


def quantise_tree(nodes, slot_lo, slot_hi, layout):
    """Fills origin, scales and planes of every node of `nodes` (child words set) from the primitive boxes by leaf slot; a child's
    box is the union of the primitives below it. -> the root's box."""
    deep_recursion()
    W, co, po, pd = layout.width, layout.child_offset, layout.plane_offset, layout.plane_dwords

    def fill(i):
        row = nodes[i]
        boxes = []
        for c in range(W):
            ref = int(row[co + c])
            if ref < 0x80000000:
                boxes.append(fill(ref))
            else:
                v = ~ref & 0xFFFFFFFF
                first, cnt = v >> 3, v & 7
                boxes.append((slot_lo[first:first + cnt].min(axis=0), slot_hi[first:first + cnt].max(axis=0)) if cnt else None)
        real = [b for b in boxes if b is not None]
        lo_n = np.min([b[0] for b in real], axis=0)
        hi_n = np.max([b[1] for b in real], axis=0)
        row[:co] = 0
        for a in range(3):
            origin, e, ql, qh = quantise_axis(lo_n[a], hi_n[a], [b[0][a] for b in real], [b[1][a] for b in real])
            row[a] = np.array([origin], dtype=f32).view(np.uint32)[0]
            row[SCALE_DWORDS[a]] = (e + 127) << 23
            k = 0
            for c in range(W):
                l, h = 255, 0      # an unused child's box is inverted
                if boxes[c] is not None:
                    l, h = ql[k], qh[k]
                    k += 1
                row[po + a * pd + c // 4] |= l << (8 * (c % 4))
                row[po + (3 + a) * pd + c // 4] |= h << (8 * (c % 4))
        return lo_n, hi_n
    return fill(0)


# ---- the whole builder ----------------------------------------------------------------------------------------------------------
class Built:
    """nodes (canonical numbering), order (primitive per leaf slot), slot_of_prim, n_nodes, max_stack, the height bound's report;
    `refused`: the binary tree is taller than the cap and is not rebalanced, or cannot be."""
    refused = False


def build(prim_lo, prim_hi, layout, radius, stack_floor, stack_cap, rebalance=False, spread_ties=False, has_box=None, single_ok=False):
    """The tree over primitives with these padded boxes. radius 0: radix tree, otherwise PLOC with that search radius; rows without
    a box (has_box) sort last and stay out of the tree; single_ok: one primitive makes a one-node tree (mesh trees)."""
    prim_lo, prim_hi = np.asarray(prim_lo, dtype=f32), np.asarray(prim_hi, dtype=f32)
    out = Built()
    g_lo, g_hi = grid_bounds(prim_lo, prim_hi, has_box)
    out.keys = morton_keys(centres(prim_lo, prim_hi), g_lo, g_hi, has_box)
    sorted_prims = stable_order(out.keys)
    n = len(sorted_prims) if has_box is None else int(np.count_nonzero(has_box))
    sorted_prims = sorted_prims[:n]
    s_lo, s_hi = prim_lo[sorted_prims], prim_hi[sorted_prims]
    out.sorted_prims, out.radius, out.rebuilt_sets = sorted_prims, radius, []
    out.height_before = out.height_after = out.subtrees_rebuilt = out.prims_rebuilt = 0
    if n == 1 and single_ok:
        wide, order, out.max_stack = single_primitive_tree()
    else:
        bins = leaf_bins(s_lo, s_hi)
        root = ploc_tree(bins, radius, spread_ties, layout.leaf_max) if radius else radix_tree([out.keys[p] for p in sorted_prims], bins, layout.leaf_max)
        out.binary_before = root
        out.height_before = out.height_after = root.height
        if root.height > stack_cap:
            if not rebalance or median_height(n, layout.leaf_max) > stack_cap:
                out.refused = True
                return out
            root, out.subtrees_rebuilt, out.prims_rebuilt, rebuilt = bound_height(root, stack_cap, layout.leaf_max)
            out.rebuilt_sets = [frozenset(sorted_prims[p] for p in leaves) for leaves in rebuilt]
            out.height_after = root.height
        out.binary = root
        floor = min(stack_floor, stack_cap) if rebalance else stack_floor
        out.budget = max(root.height, floor)
        wide, order, out.max_stack = collapse(root, out.budget, layout)
    out.nodes = emit(wide, layout)
    out.order = np.array([sorted_prims[p] for p in order], dtype=np.uint32)
    out.slot_of_prim = np.zeros(len(prim_lo), dtype=np.uint32)
    out.slot_of_prim[out.order] = np.arange(n, dtype=np.uint32)
    quantise_tree(out.nodes, prim_lo[out.order], prim_hi[out.order], layout)
    out.n_nodes = len(out.nodes)
    return out


# ---- comparing trees --------------------------------------------------------------------------------------------------------------
def canonical(nodes, layout):
    """The tree renumbered breadth-first in child order, inner references rewritten."""
    nodes = np.asarray(nodes, dtype=np.uint32)
    co, W = layout.child_offset, layout.width
    visit, new_of = [0], {0: 0}
    for old in visit:      # grows while it runs
        for c in range(W):
            ref = int(nodes[old, co + c])
            if ref < 0x80000000:
                assert ref < len(nodes) and ref not in new_of, "node %d is referenced twice or out of range" % ref
                new_of[ref] = len(visit)
                visit.append(ref)
    out = nodes[visit].copy()
    for row in out:
        for c in range(W):
            if int(row[co + c]) < 0x80000000:
                row[co + c] = new_of[int(row[co + c])]
    return out


def prims_below(nodes, i, prim_of_slot, layout):
    found = []
    for c in range(layout.width):
        ref = int(nodes[i, layout.child_offset + c])
        if ref < 0x80000000:
            found += prims_below(nodes, ref, prim_of_slot, layout) if ref < len(nodes) else []
        else:
            v = ~ref & 0xFFFFFFFF
            found += [int(p) for p in prim_of_slot[v >> 3:(v >> 3) + (v & 7)]]
    return found


def child_prims(nodes, i, prim_of_slot, layout):
    """Per child of node i: None (unused), or the primitives below it (a leaf's in slot order, a node's sorted)."""
    out = []
    for c in range(layout.width):
        ref = int(nodes[i, layout.child_offset + c])
        if ref == UNUSED:
            out.append(None)
        elif ref < 0x80000000:
            out.append(("node", sorted(prims_below(nodes, ref, prim_of_slot, layout))))
        else:
            v = ~ref & 0xFFFFFFFF
            out.append(("leaf", [int(p) for p in prim_of_slot[v >> 3:(v >> 3) + (v & 7)]]))
    return out


def differing_field(a, b, layout):
    """Which part of the geometry of two nodes with equal child words differs first."""
    po = layout.plane_offset
    if (a[:3] != b[:3]).any():
        return "origin"
    if any(a[d] != b[d] for d in SCALE_DWORDS):
        return "scale"
    if (a[po:po + 6 * layout.plane_dwords] != b[po:po + 6 * layout.plane_dwords]).any():
        return "plane"
    return "other words"


def stage_of(built, got, got_prim_of_slot, layout, field):
    """The stage a difference in `field` points to, given the reference's build. Boxes come from the quantiser. Equal sets in another
    order inside a leaf come from the order below it. Child sets that are all subtrees of the reference's binary tree come from the
    collapse; others that lie inside the subtrees the height bound rebuilt, from that pass. Every subtree of a radix tree is a range
    of the sorted order: a set that is not comes from the keys or the sort."""
    if field in ("origin", "scale", "plane"):
        return "node quantisation"
    if built is None or not hasattr(built, "binary"):
        return "topology"
    if field == "leaf range":
        return "the order of the primitives in a leaf: ties of the sort, or the order of a binary node's two children"
    family = set()

    def collect(b):
        family.add(frozenset(built.sorted_prims[p] for p in b.leaves()))
        if b.pos is None:
            collect(b.left); collect(b.right)
    deep_recursion()
    collect(built.binary)
    odd = [frozenset(c[1]) for i in range(len(got)) for c in child_prims(got, i, got_prim_of_slot, layout) if c and frozenset(c[1]) not in family]
    if not odd:
        return "collapse, or the order of a binary node's two children"
    if built.rebuilt_sets and all(any(o <= r for r in built.rebuilt_sets) for o in odd):
        return "height bound"
    if built.radius:
        return "Morton keys, sort or PLOC"
    position = {p: k for k, p in enumerate(built.sorted_prims)}
    ranges = all(max(position[p] for p in o) - min(position[p] for p in o) + 1 == len(o) for o in odd)
    return "radix tree" if ranges else "Morton keys or sort"


def assert_trees_equal(got_nodes, got_prim_of_slot, want_nodes, want_prim_of_slot, layout, what, built=None):
    """Both trees in the canonical numbering are equal arrays; otherwise the message names the first differing node, the field
    (child set, leaf range, origin, scale or plane), the stage that points to (with the reference's `built`) and the primitive-id sets below the two nodes. The topology of the whole tree is
    compared before any box, so that a different split is not reported as the different planes it also causes."""
    got, want = canonical(got_nodes, layout), canonical(want_nodes, layout)
    co, W = layout.child_offset, layout.width

    def fail(i, field):
        cg, cw = child_prims(got, i, got_prim_of_slot, layout), child_prims(want, i, want_prim_of_slot, layout)
        raise AssertionError("%s: node %d (breadth-first) differs in its %s (stage: %s)\n  device    %s\n  reference %s\n  primitives below, per child:\n  device    %s\n"
                             "  reference %s" % (what, i, field, stage_of(built, got, got_prim_of_slot, layout, field), [hex(int(x)) for x in got[i]], [hex(int(x)) for x in want[i]], cg, cw))
    for i in range(min(len(got), len(want))):
        cg, cw = child_prims(got, i, got_prim_of_slot, layout), child_prims(want, i, want_prim_of_slot, layout)
        if [c and (c[0], sorted(c[1])) for c in cg] != [c and (c[0], sorted(c[1])) for c in cw]:
            fail(i, "child set")
        if cg != cw or (got[i, co:co + W] != want[i, co:co + W]).any():
            fail(i, "leaf range")
    assert len(got) == len(want), "%s: %d nodes, the reference has %d" % (what, len(got), len(want))
    for i in range(len(got)):
        if (got[i] != want[i]).any():
            fail(i, differing_field(got[i], want[i], layout))
    a, b = got.view(np.uint8).reshape(-1), want.view(np.uint8).reshape(-1)
    assert int((a != b).sum()) == 0, "%s: %d of %d bytes differ" % (what, int((a != b).sum()), a.size)
