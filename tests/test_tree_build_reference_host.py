"""The reference of the device tree builder (tests/tree_build_reference.py) checked against itself on the CPU, stage by stage, so
that it is not fitted to what the device produces: the recursive radix tree against Karras's per-node procedure, the PLOC search
against brute force, the collapse against a walk of its own result, the quantiser against the nearest covering values, the height
bound against its contract. The device is compared with the reference in tests/test_gpu_tree_build_reference.py."""
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tree_build_reference as ref  # noqa: E402

from sunray_amd import abi, runtime  # noqa: E402

f32 = np.float32


@pytest.fixture(scope="module")
def layout():
    return ref.Layout(*runtime.bvh_layout(), runtime.tree_build_limits(abi.TREE_KIND_MESH, 1)[0])


def random_boxes(rng, n, spread=1.0, size=0.2):
    lo = rng.uniform(-spread, spread, size=(n, 3)).astype(f32)
    return lo, (lo + rng.uniform(0.0, size, size=(n, 3)).astype(f32)).astype(f32)


def nested(b):
    """A binary tree as nested tuples of sorted positions."""
    return b.pos if b.pos is not None else (nested(b.left), nested(b.right))


def test_the_library_names_its_limits():
    assert runtime.tree_build_limits(abi.TREE_KIND_MESH, 1)[0] >= 1
    def median_depth(n):      # levels of a median split down to leaves of at most two, the root's and the leaves' included
        c, need = (n + 1) // 2, 2
        while c > 1:
            c, need = (c + 1) // 2, need + 1
        return need
    assert [median_depth(n) for n in (1, 2, 3, 5, 64, 65)] == [2, 2, 3, 4, 7, 8]
    for n in (1, 2, 3, 5, 63, 64, 65, 257, 960, 4096, 1 << 20, 1 << 30):
        assert runtime.tree_build_limits(abi.TREE_KIND_MESH, n)[1] == min(max(median_depth(n) + 6, 6), 31)      # the host builder's depth for that size
        assert runtime.tree_build_limits(abi.TREE_KIND_TOP_LEVEL, n)[1] == median_depth(n)
        assert runtime.tree_build_limits(abi.TREE_KIND_ONE_LEVEL, n)[1] == 31
    from sunray_amd._lib import lib
    assert lib().sr_tree_build_limits(3, 1, None, None) == -1 and b"sr_tree_build_limits" in lib().sr_last_error()
    assert lib().sr_tree_build_limits(0, 1, None, None) == 0


# ---- radix tree -------------------------------------------------------------------------------------------------------------
def karras_tree(keys):
    """Karras 2012, section 4, literally: every inner node i finds its direction, its range by doubling and bisection, and its
    split by bisection, all through delta(i, j) = length of the common prefix of the 64-bit keys, the 32-bit index appended on ties,
    -1 outside the list. -> nested tuples from inner node 0."""
    n = len(keys)

    def delta(i, j):
        if j < 0 or j >= n:
            return -1
        if keys[i] != keys[j]:
            return 64 - (keys[i] ^ keys[j]).bit_length()
        return 64 + 32 - (i ^ j).bit_length()
    left, right = {}, {}
    for i in range(n - 1):
        d = 1 if delta(i, i + 1) - delta(i, i - 1) >= 0 else -1
        d_min = delta(i, i - d)
        l_max = 2
        while delta(i, i + l_max * d) > d_min:
            l_max *= 2
        length, t = 0, l_max // 2
        while t >= 1:
            if delta(i, i + (length + t) * d) > d_min:
                length += t
            t //= 2
        j = i + length * d
        d_node = delta(i, j)
        s, t = 0, length
        while True:
            t = (t + 1) // 2
            if delta(i, i + (s + t) * d) > d_node:
                s += t
            if t <= 1:
                break
        gamma = i + s * d + min(d, 0)
        left[i] = ("leaf", gamma) if min(i, j) == gamma else ("node", gamma)
        right[i] = ("leaf", gamma + 1) if max(i, j) == gamma + 1 else ("node", gamma + 1)

    def tree(ref_):
        return ref_[1] if ref_[0] == "leaf" else (tree(left[ref_[1]]), tree(right[ref_[1]]))
    return tree(("node", 0))


def key_lists():
    rng = np.random.default_rng(11)
    yield "two keys", [3, 9]
    yield "all keys equal", [0x123456789ABCDEF] * 37
    yield "two equal keys", [5, 5]
    yield "runs of equal keys", sorted([7] * 5 + [8] * 1 + [0x4000000000000000] * 9 + [0x4000000000000001] * 2 + [0x7FFFFFFFFFFFFFFF] * 4)
    yield "keys differing only in bit 0", [10] * 6 + [11] * 7
    yield "keys differing only in bit 62", [5] * 3 + [5 | 1 << 62] * 5
    yield "one key per bit", sorted(1 << b for b in range(63))
    yield "boxless rows last", sorted(int(k) for k in rng.integers(0, 1 << 63, size=20)) + [(1 << 64) - 1] * 3
    for n in (2, 3, 17, 64, 65, 300):
        yield "%d random keys" % n, sorted(int(k) for k in rng.integers(0, 1 << 63, size=n))
        yield "%d random keys of 6 bits" % n, sorted(int(k) for k in rng.integers(0, 64, size=n))


@pytest.mark.parametrize("name,keys", list(key_lists()), ids=[k for k, _ in key_lists()])
def test_radix_tree_is_karrass(name, keys, layout):
    bins = ref.leaf_bins(*random_boxes(np.random.default_rng(1), len(keys)))
    assert nested(ref.radix_tree(keys, bins, layout.leaf_max)) == karras_tree(keys), name


# ---- PLOC -------------------------------------------------------------------------------------------------------------------
def brute_force_neighbour(boxes, i, radius, spread_ties):
    """All pairs inside the window, the ties as the rule states them."""
    def area(j):
        d = np.maximum(boxes[i, 3:], boxes[j, 3:]) - np.minimum(boxes[i, :3], boxes[j, :3])
        return d[0] * d[1] + d[1] * d[2] + d[2] * d[0]
    cand = [j for j in range(len(boxes)) if j != i and abs(j - i) <= radius]
    if spread_ties:
        return min(cand, key=lambda j: (area(j), abs(j - i), 0 if j == i ^ 1 else 1, j))
    return min(cand, key=lambda j: (area(j), j))


def ploc_inputs():
    rng = np.random.default_rng(5)
    lo, hi = random_boxes(rng, 150)
    order = np.argsort(lo[:, 0], kind="stable")
    yield "150 boxes along x", lo[order], hi[order]
    yield "40 identical boxes", np.zeros((40, 3), f32), np.ones((40, 3), f32)
    yield "9 identical boxes", np.zeros((9, 3), f32), np.ones((9, 3), f32)
    yield "33 flat identical boxes", np.zeros((33, 3), f32), np.tile(np.array([1, 0, 0], f32), (33, 1))
    lo, hi = random_boxes(rng, 64, size=0.0)
    yield "points on a grid (many equal areas)", np.round(lo * 2) / 2, np.round(lo * 2) / 2 + f32(0.5)


@pytest.mark.parametrize("spread_ties", [False, True])
@pytest.mark.parametrize("radius", [1, 2, 16])
@pytest.mark.parametrize("name,lo,hi", list(ploc_inputs()), ids=[x[0] for x in ploc_inputs()])
def test_ploc_search_is_brute_force_and_every_iteration_merges(name, lo, hi, radius, spread_ties, layout):
    clusters = ref.leaf_bins(lo.astype(f32), hi.astype(f32))
    boxes = np.concatenate([lo, hi], axis=1).astype(f32)
    iterations = 0
    while len(clusters) > 1:
        want = [brute_force_neighbour(boxes, i, radius, spread_ties) for i in range(len(boxes))]
        m = len(clusters)
        clusters, boxes, nn, merged = ref.ploc_iteration(clusters, boxes, radius, spread_ties, layout.leaf_max)
        assert [int(j) for j in nn] == want, "%s, iteration %d" % (name, iterations)
        assert merged >= 1 and len(clusters) == m - merged
        iterations += 1
    assert sorted(clusters[0].leaves()) == list(range(len(lo)))
    if spread_ties and "identical" in name:
        assert iterations == math.ceil(math.log2(len(lo))), "identical boxes halve every iteration"


def test_ploc_with_a_radius_of_the_whole_list_merges_the_closest_pair_first(layout):
    rng = np.random.default_rng(8)
    for n in (2, 5, 40):
        lo, hi = random_boxes(rng, n)
        boxes = np.concatenate([lo, hi], axis=1)
        i, j = np.triu_indices(n, 1)
        areas = ref.union_areas(boxes, i, j)
        k = int(np.argmin(areas))
        assert (areas == areas[k]).sum() == 1
        for radius in (n, n + 7):
            clusters, _, _, _ = ref.ploc_iteration(ref.leaf_bins(lo, hi), boxes, radius, False, layout.leaf_max)
            assert [int(i[k]), int(j[k])] in [c.leaves() for c in clusters]


# ---- collapse ---------------------------------------------------------------------------------------------------------------
def binary_trees(layout):
    rng = np.random.default_rng(21)
    for n in (2, 3, 5, 64, 65, 300):
        lo, hi = random_boxes(rng, n)
        keys = sorted(int(k) for k in rng.integers(0, 1 << 20, size=n))
        yield "radix %d" % n, ref.radix_tree(keys, ref.leaf_bins(lo, hi), layout.leaf_max), n
        yield "ploc %d" % n, ref.ploc_tree(ref.leaf_bins(lo, hi), 4, False, layout.leaf_max), n
    lo, hi = random_boxes(rng, 63)
    yield "chain 63", ref.radix_tree(sorted(1 << b for b in range(63)), ref.leaf_bins(lo, hi), layout.leaf_max), 63


def walk_need(nodes, i, layout):
    """Entries a depth-first walk holds below node i: k - 1 siblings wait while the deepest child is walked."""
    k, deepest = 0, 0
    for c in range(layout.width):
        r = int(nodes[i, layout.child_offset + c])
        if r < 0x80000000:
            k, deepest = k + 1, max(deepest, walk_need(nodes, r, layout))
        elif r != ref.UNUSED:
            k += 1
    return k - 1 + deepest


def slot_range(nodes, i, layout):
    """(first, end) of the slots below node i; children take consecutive ranges in child order."""
    first = end = None
    for c in range(layout.width):
        r = int(nodes[i, layout.child_offset + c])
        if r == ref.UNUSED:
            continue
        if r < 0x80000000:
            a, b = slot_range(nodes, r, layout)
        else:
            v = ~r & 0xFFFFFFFF
            a, b = v >> 3, (v >> 3) + (v & 7)
            assert 1 <= (v & 7) <= layout.leaf_max
        assert end is None or a == end, "node %d: child %d starts at slot %d, the previous one ended at %d" % (i, c, a, end)
        first, end = a if first is None else first, b
    return first, end


def test_collapse_gives_every_primitive_one_slot_within_the_budget(layout):
    for name, root, n in binary_trees(layout):
        for extra in (0, 1, 3, 40):
            budget = max(root.height, 1) + extra      # the root is a node even over a leaf's worth of primitives: two children, one entry
            wide, order, max_stack = ref.collapse(root, budget, layout)
            nodes = ref.emit(wide, layout)
            assert sorted(order) == list(range(n)), name
            assert slot_range(nodes, 0, layout) == (0, n), name
            assert max_stack == walk_need(nodes, 0, layout) <= budget, (name, budget)
            if extra == 40 and n > 2 * layout.width * layout.leaf_max:
                assert all(int(r) != ref.UNUSED for r in nodes[0, layout.child_offset:layout.child_offset + layout.width]), "a free budget fills the root"
    wide, order, max_stack = ref.single_primitive_tree()
    assert (order, max_stack, len(ref.emit(wide, layout))) == ([0], 0, 1)


# ---- quantiser --------------------------------------------------------------------------------------------------------------
def check_axis(lo_n, hi_n, child_lo, child_hi, what):
    origin, e, ql, qh = ref.quantise_axis(lo_n, hi_n, child_lo, child_hi)
    scale = ref.grid_scale(e)
    assert origin < lo_n and -126 <= e <= 127, what
    ext = f32(hi_n - origin)
    start = max(math.frexp(float(f32(ext / f32(255.0))))[1], -126) if ext > 0 and f32(ext / f32(255.0)) > 0 else -126
    fits = lambda ee: all(ref.upper_plane(h, origin, ref.grid_scale(ee), 255) <= 255 for h in child_hi)
    assert e >= start and (e == 127 or fits(e)) and (e == start or not fits(e - 1)), "%s: exponent %d (from %d)" % (what, e, start)
    exact = lambda q: Fraction(q) * Fraction(float(scale)) + Fraction(float(origin))
    for l, h, q_lo, q_hi in zip(child_lo, child_hi, ql, qh):
        assert 0 <= q_lo <= 255 and 0 <= q_hi <= 255
        assert ref.round_to_f32(exact(q_lo)) == ref.decode(q_lo, scale, origin) and ref.round_to_f32(exact(q_hi)) == ref.decode(q_hi, scale, origin)
        assert ref.decode(q_lo, scale, origin) <= l, "%s: the lower plane %d does not cover %r" % (what, q_lo, l)
        if e < 127:
            assert ref.decode(q_hi, scale, origin) >= h, "%s: the upper plane %d does not cover %r" % (what, q_hi, h)
        covers_lo = lambda q: ref.decode(q, scale, origin) <= l and exact(q) <= Fraction(float(l)) - ref.GUARD * Fraction(float(scale))
        covers_hi = lambda q: ref.decode(q, scale, origin) >= h and exact(q) >= Fraction(float(h)) + ref.GUARD * Fraction(float(scale))
        assert q_lo == 255 or not covers_lo(q_lo + 1), "%s: the lower plane %d could be one cell up" % (what, q_lo)
        assert q_hi == 0 or not covers_hi(q_hi - 1), "%s: the upper plane %d could be one cell down" % (what, q_hi)
        assert q_lo == 0 or covers_lo(q_lo) and (e == 127 or covers_hi(q_hi)), "%s: a plane without its guard band" % what


def test_quantised_planes_are_the_nearest_covering_ones():
    rng = np.random.default_rng(31)
    for k in range(10000):
        n = int(rng.integers(1, 5))
        centre = f32(rng.normal() * 10.0 ** rng.integers(-3, 4))
        size = f32(10.0 ** rng.uniform(-6, 3))
        lo = (centre + size * rng.uniform(0, 1, size=n)).astype(f32)
        hi = (lo + size * rng.uniform(0, 1, size=n) * (rng.uniform(size=n) > 0.2)).astype(f32)
        check_axis(lo.min(), hi.max(), list(lo), list(hi), "set %d" % k)


@pytest.mark.parametrize("name,lo,hi", [
    ("zero extent", [1.5, 1.5], [1.5, 1.5]),
    ("zero extent at zero", [0.0], [0.0]),
    ("extent 1e-18", [0.0, 4e-19], [1e-18, 1e-18]),
    ("extent 1e-18 far from zero", [3.0, 3.0], [3.0 + 1e-18, 3.0]),
    ("extent 1e15", [-5e14, 0.0, 1e-18], [5e14, 1e-18, 2e-18]),
    ("extent 1e15 with a thin child", [0.0, 1e15], [1e15, 1e15]),
    ("a child equal to the node", [-1.0, -1.0, 0.25], [2.0, 0.5, 2.0]),
    ("one real child", [-7.25], [9.0]),
    ("an extent near the largest finite number", [-1.5e38, 0.0], [1.5e38, 1.0]),
    ("subnormal extent", [0.0], [1e-44])])
def test_quantiser_edge_sets(name, lo, hi):
    lo, hi = [f32(x) for x in lo], [f32(x) for x in hi]
    check_axis(min(lo), max(hi), lo, hi, name)


def test_round_to_f32_rounds_once():
    assert ref.round_to_f32(Fraction(1) + Fraction(1, 1 << 24)) == f32(1.0)                                  # a tie goes to even
    assert ref.round_to_f32(Fraction(1) + Fraction(1, 1 << 24) + Fraction(1, 1 << 80)) == np.nextafter(f32(1.0), f32(2.0))   # float64 first would lose the last term
    assert ref.round_to_f32(Fraction(3, 1 << 150)) == np.nextafter(f32(0), f32(1)) * f32(2) and ref.round_to_f32(Fraction(-1, 3)) == f32(-1.0 / 3.0)
    assert ref.decode(255, f32(2.0 ** -60), f32(1.0)) == f32(1.0) and ref.decode(3, f32(0.5), f32(-1.5)) == f32(0.0)


# ---- height bound -----------------------------------------------------------------------------------------------------------
def is_median(t):
    """Whether t is the median-split tree over its leaves: every left half takes the odd one."""
    return t.pos is not None or (t.left.size == (t.size + 1) // 2 and is_median(t.left) and is_median(t.right))


def check_bounded(before, after, seen):
    """Outside the subtrees that are median-split trees over the input's leaves in their order, `after` is `before`: the input's
    own subtree where it was kept whole, the input's split where the rule went on below. seen: [kept whole, splits kept, rebuilt]."""
    if after is before:
        seen[0] += before.pos is None
    elif after.left.leaves() == before.left.leaves() and after.right.leaves() == before.right.leaves():
        seen[1] += 1
        check_bounded(before.left, after.left, seen)
        check_bounded(before.right, after.right, seen)
    else:
        assert after.leaves() == before.leaves() and is_median(after)
        seen[2] += 1


def test_height_bound_keeps_what_fits_and_rebuilds_the_rest(layout):
    assert [ref.median_height(k, 2) for k in (1, 2, 3, 4, 5, 63, 64, 65, 960)] == [0, 0, 1, 1, 2, 5, 5, 6, 9]
    t = ref.median_tree(ref.leaf_bins(*random_boxes(np.random.default_rng(2), 7)), layout.leaf_max)
    assert nested(t) == (((0, 1), (2, 3)), ((4, 5), 6))                  # the split falls behind lo + ceil(n / 2) - 1
    cases, seen = 0, [0, 0, 0]
    for name, root, n in binary_trees(layout):
        floor = ref.median_height(n, layout.leaf_max)
        for cap in sorted({floor, floor + 1, (floor + root.height) // 2, root.height - 1}):
            if not floor <= cap < root.height:
                continue
            after, rebuilt, prims, _ = ref.bound_height(root, cap, layout.leaf_max)
            assert after.height <= cap, (name, cap, after.height)
            assert after.leaves() != [] and sorted(after.leaves()) == list(range(n)) and rebuilt >= 1
            check_bounded(root, after, seen)
            assert prims >= rebuilt * (layout.leaf_max + 1)
            cases += 1
        same, rebuilt, _, _ = ref.bound_height(root, root.height, layout.leaf_max)
        assert same is root and rebuilt == 0
    assert cases >= 10 and min(seen) >= 5, seen


# ---- canonical numbering ----------------------------------------------------------------------------------------------------
def test_canonical_numbering_and_the_mismatch_message(layout):
    rng = np.random.default_rng(4)
    lo, hi = random_boxes(rng, 40)
    b = ref.build(lo, hi, layout, 0, 10, 26)
    perm = np.concatenate([[0], 1 + rng.permutation(b.n_nodes - 1)])      # new number of every node; the root stays
    shuffled = np.zeros_like(b.nodes)
    for old in range(b.n_nodes):
        row = b.nodes[old].copy()
        for c in range(layout.width):
            if int(row[layout.child_offset + c]) < 0x80000000:
                row[layout.child_offset + c] = perm[int(row[layout.child_offset + c])]
        shuffled[perm[old]] = row
    assert b.n_nodes > 4 and (shuffled != b.nodes).any()
    ref.assert_trees_equal(shuffled, b.order, b.nodes, b.order, layout, "renumbered")
    for dword, field in ((1, "origin"), (ref.SCALE_DWORDS[2], "scale"), (layout.plane_offset + 4, "plane")):
        bad = shuffled.copy()
        bad[perm[3], dword] ^= 1 << 8
        with pytest.raises(AssertionError, match=r"node 3 \(breadth-first\) differs in its %s \(stage: node quantisation\)" % field):
            ref.assert_trees_equal(bad, b.order, b.nodes, b.order, layout, "one bit")
    other = ref.build(lo, hi, layout, 16, 10, 26)
    with pytest.raises(AssertionError, match=r"differs in its child set \(stage: Morton keys, sort or PLOC\)(.|\n)*primitives below"):
        ref.assert_trees_equal(b.nodes, b.order, other.nodes, other.order, layout, "another topology", other)


# ---- rows without a box -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [0, 16])
def test_rows_without_a_box_sort_last_and_stay_out_of_the_tree(radius, layout):
    """No instance list a scene accepts reaches the device's top-level build with a boxless row (a mesh of no triangles is refused,
    every other boxless record sends the list to the host), so this part of the builder's contract is held here: the tree over a
    list with NaN rows is the tree over the rows that have a box, with the instance numbers of the full list."""
    rng = np.random.default_rng(17)
    lo, hi = random_boxes(rng, 70)
    has_box = np.ones(70, dtype=bool)
    has_box[[0, 13, 14, 69]] = False
    lo[~has_box], hi[~has_box] = np.nan, np.nan
    full = ref.build(lo, hi, layout, radius, 6, 30, spread_ties=True, has_box=has_box)
    kept = np.nonzero(has_box)[0]
    part = ref.build(lo[kept], hi[kept], layout, radius, 6, 30, spread_ties=True)
    assert all(k == (1 << 64) - 1 for k, ok in zip(full.keys, has_box) if not ok) and max(k for k, ok in zip(full.keys, has_box) if ok) < 1 << 63
    assert (full.nodes == part.nodes).all() and (full.order == kept[part.order]).all() and (full.n_nodes, full.max_stack) == (part.n_nodes, part.max_stack)
