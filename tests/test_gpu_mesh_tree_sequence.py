"""What carries over between the paths of mesh-tree maintenance in ONE two-level scene (csrc/api.cpp maintain_mesh_trees,
build_mesh_trees_device, two_level_build): the node ranges, the cached refit set, the currency of the device mesh rows and the
baked flag. The other suites exercise each path in a scene made for it; here one scene goes through refits, the batched and the
per-mesh device build in one call, a refit over device-built level ranges, a baked instance that comes and goes, an updated
Static mesh, a mesh replaced in its slot and the settle rebuild. After every step the reports are the values written out below
(derived from the rules in the comments of api.cpp), the queries of a fixed ray set equal those of a FRESH scene loaded from
the same description bit for bit, and every mesh's tree holds its triangles. Times are compared with 0.0 only."""
import ctypes as C
import dataclasses
import os
import sys

import numpy as np
import pytest

from sunray_amd import abi, scenes

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_mesh_refit import Heuristic, state_fields, tree_contains_its_triangles  # noqa: E402
from test_gpu_mesh_tree_batch import batch_scene, grid_mesh  # noqa: E402
from test_gpu_mesh_tree_build import SEVEN_BOX, seven_meshes, walk_stack  # noqa: E402
from test_gpu_mesh_update import mesh_of, push  # noqa: E402
from test_gpu_parity import assert_bits_equal  # noqa: E402
from test_gpu_top_level_build import LEAF_MAX  # noqa: E402
from test_oracle_trace import random_rays  # noqa: E402

U, F, S, NONE = abi.OP_UPDATE, abi.OP_FAST_BUILD, abi.OP_SLOW_BUILD, abi.OP_NONE
SOMETIMES, STATIC = abi.BUILD_SOMETIMES_CHANGES, abi.BUILD_STATIC
MESH, TOP = abi.TREE_KIND_MESH, abi.TREE_KIND_TOP_LEVEL
ON_DEVICE, BAKED, STATIC_MESH = abi.MESH_TREE_ON_DEVICE, abi.MESH_TREE_HOST_BAKED_INSTANCE, abi.MESH_TREE_HOST_STATIC_MESH
BIG, FLOOR, NEW = 50, 2, 60
KEYS = [1, 6, 7, BIG]       # SometimesChanges: 1, 65 and 960 triangles (the batch takes them), SR_BLAS_BATCH_MAX_TRIS + 1 (the per-mesh build)
TRIS = {1: 1, FLOOR: 2, 6: 65, 7: 960, BIG: abi.BLAS_BATCH_MAX_TRIS + 1}
SQUASH = np.array([1, 0, 0, 0.5, 0, 0, 0, 1.2, 0, 0, 1, 0.3], dtype=np.float32)      # singular: the instance gets a baked copy of its mesh


@pytest.fixture(scope="module")
def rt():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    from sunray_amd import runtime
    return runtime


def five_meshes():
    """Meshes 1, 2 (the Static floor quad), 6 and 7 of seven_meshes with their instances, and a grid one triangle above the batch's
    limit: mesh slots 0 .. 4 in this order, six instances."""
    base = seven_meshes()
    keep = [1, FLOOR, 6, 7]
    meshes = [mesh_of(base, k) for k in keep] + [grid_mesh(BIG, TRIS[BIG])]
    instances = [(k, xs) for k, xs in base.instances if k in keep] + [(BIG, [scenes.translate(0.5, 1.2, -1.5)])]
    desc = dataclasses.replace(base, name="five_meshes", meshes=meshes, instances=instances)
    assert [len(m.indices) // 3 for m in desc.meshes] == [TRIS[m.key] for m in desc.meshes] and sum(len(xs) for _, xs in instances) == 6
    return desc


def instancing(gsc):
    from sunray_amd._lib import lib
    mode, now = C.c_uint32(), C.c_uint32()
    assert lib().sr_scene_instancing(gsc._h, C.byref(mode), C.byref(now)) == 0
    return (mode.value, now.value)


def reports(gsc):
    """Every field but the times of the five reports; the times that must be 0.0 (timing is off, or nothing of the kind ran) as booleans."""
    u, t, b, top = gsc.mesh_update_info(), gsc.mesh_tree_info(), gsc.mesh_tree_batch_info(), gsc.top_level_info()
    hm, ht = gsc.tree_height_info(MESH), gsc.tree_height_info(TOP)
    return {"update": (u.dirty_meshes, u.reshaded, u.blas_rebuilt, u.blas_refitted), "update_times_zero": (u.flatten_ms == 0.0, u.refit_ms == 0.0),
            "host_built_nothing": u.blas_build_ms == 0.0,
            "trees": (t.mode, t.auto_threshold, t.built_on_device, t.built_on_host, t.reason), "trees_time_zero": t.device_build_ms == 0.0,
            "last_built": (t.n_nodes, t.max_stack),
            "batch": (b.mode, b.max_tris, b.batched, b.passed_on, b.launches, b.reserved), "batch_time_zero": b.batch_ms == 0.0,
            "top": (top.on_device, top.reason, top.mode, top.auto_threshold, top.n_boxes, top.n_instances),
            "top_tree": (top.n_nodes, top.max_stack, top.blas_stack),
            "mesh_height": (hm.mode, hm.mesh_tree_cap, hm.on_device, hm.cap), "top_height": (ht.mode, ht.mesh_tree_cap, ht.on_device, ht.cap),
            "mesh_heights": (hm.height_before, hm.height_after, hm.subtrees_rebuilt, hm.prims_rebuilt),
            "top_heights": (ht.height_before, ht.height_after, ht.subtrees_rebuilt, ht.prims_rebuilt),
            "instancing": instancing(gsc)}


class Fresh:
    """Closest-hit and existence queries of a fresh scene loaded from a description, for the fixed ray set."""

    def __init__(self, rt):
        self.rt = rt
        self.rays = random_rays(4000, 41, box=SEVEN_BOX)
        self.rd = rt.rays_to_device(self.rays)

    def queries(self, gsc):
        n = len(self.rays)
        return self.rt.hits_from_device(gsc.trace_closest(self.rd, n)).copy(), gsc.trace_any(self.rd, n).cpu().numpy().view(np.uint32).copy()

    def equal(self, gsc, desc, what):
        fresh = self.rt.Scene(0, instancing="two_level").load(desc)
        want_hits, want_any = self.queries(fresh)
        fresh.close()
        hits, occluded = self.queries(gsc)
        assert (want_hits["t"] >= 0).mean() > 0.03
        assert_bits_equal(want_hits, hits, "closest hits against a fresh scene, " + what)
        assert np.array_equal(want_any, occluded), "existence queries against a fresh scene, " + what


@pytest.mark.parametrize("topology", ["lbvh", "ploc16"])
def test_one_scene_through_every_path(rt, monkeypatch, topology):
    monkeypatch.setenv("SR_FAST_BUILD", topology)
    desc = five_meshes()
    keys = list(KEYS)
    gsc = batch_scene(rt, desc, keys).set_top_level_build("device")
    fresh = Fresh(rt)
    want = {k: Heuristic(SOMETIMES) for k in keys}
    last = {k: None for k in keys}
    last_built = (0, 0)                 # SrMeshTreeInfo.n_nodes, max_stack: of the last mesh of the last device build, kept until the next
    heights = {"mesh": (0, 0, 0, 0), "top": None, "top_cap": None, "big_stack": 0}     # the records of the last device builds: nothing else rewrites them

    def check(what, keys, update, trees, batch, top, mesh_height, static_last=NONE, baked=False):
        """The reports after one step. update: (dirty, rebuilt, refitted); trees: (on device, on host, reason); batch: (batched, passed
        on, launches); top: (on device, reason, boxes, instances); mesh_height: (on device, cap) of the last device mesh-tree build."""
        nonlocal last_built
        got = reports(gsc)
        print("%s %s: %s" % (topology, what, got))
        assert got["update"] == (update[0], 0, update[1], update[2]), what           # reshaded counts the one-level form's in-place updates
        assert got["update_times_zero"] == (True, True) and got["trees_time_zero"] and got["batch_time_zero"], what      # timing is off
        if trees[1] == 0 and update[1] == trees[0]:
            assert got["host_built_nothing"], what
        assert got["trees"] == (abi.MESH_TREE_BUILD_DEVICE, 0xFFFFFFFF) + trees, what      # REFUSE: auto never builds on the device
        assert got["batch"] == (abi.BLAS_BATCH_ON, abi.BLAS_BATCH_MAX_TRIS) + batch + (0,), what
        assert got["top"] == top[:2] + (abi.TL_BUILD_DEVICE, 4096) + top[2:], what
        assert got["instancing"] == (2, 1) and gsc.two_level(), what
        trees_now = {m.key: gsc.read_mesh_tree(m.key) for m in desc.meshes}
        for k, tree in trees_now.items():
            assert tree_contains_its_triangles(rt, tree, "%s %s, mesh %d" % (topology, what, k)) == len(tree["nodes"])
        if trees[0]:                    # a device build: the figures of the last mesh of its set, the largest slot
            built = [m.key for m in desc.meshes if m.key in keys][-1]
            last_built = (len(trees_now[built]["nodes"]), got["last_built"][1])
            assert walk_stack(rt, trees_now[built]["nodes"]) == got["last_built"][1] <= abi.MESH_TREE_STACK_CAP, what      # what a walk of it needs
            before, after, subtrees, prims = got["mesh_heights"]        # REFUSE: a tree that was taken fitted as its builder made it
            assert before == after >= 1 and (subtrees, prims) == (0, 0), what
            heights["mesh"] = got["mesh_heights"]
        assert got["mesh_heights"] == heights["mesh"], what
        assert got["last_built"] == last_built, what
        n_nodes, max_stack, blas_stack = got["top_tree"]
        stats = gsc.bvh_stats()
        assert n_nodes >= 1 and stats.max_stack == max_stack + LEAF_MAX + blas_stack + 1 <= abi.TL_STACK_CAP, what
        tl_nodes = gsc.read_top_level()[0]
        walks = {k: walk_stack(rt, tree["nodes"]) for k, tree in trees_now.items()}
        print("%s %s: a walk of the top level needs %d, of the mesh trees %s" % (topology, what, walk_stack(rt, tl_nodes), walks))
        assert len(tl_nodes) == n_nodes and walk_stack(rt, tl_nodes) == max_stack, what
        # every mesh is instanced: blas_stack is what a walk of the deepest tree needs (a baked copy, which cannot be read back, may need more)
        assert (max(walks.values()) <= blas_stack if baked else max(walks.values()) == blas_stack) and blas_stack <= abi.MESH_TREE_STACK_CAP, what
        if trees[0] or trees[1]:        # the stack need the device reported for the large mesh's tree stands until the host rebuilds it
            heights["big_stack"] = last_built[1] if trees[0] else 0
        assert blas_stack >= heights["big_stack"], what
        if not baked:                   # the nodes in use are the top level's and every mesh's, whichever path built or kept them
            assert stats.n_nodes == n_nodes + sum(len(t["nodes"]) for t in trees_now.values()), what
        assert got["mesh_height"] == (abi.HEIGHT_BOUND_REFUSE, 0) + mesh_height, what
        assert got["top_height"][:3] == (abi.HEIGHT_BOUND_REFUSE, 0, top[0]), what
        if top[0]:                      # a device build of the top level writes its record anew; a host build leaves it but for on_device
            assert got["top_height"][3] == abi.TL_STACK_CAP - blas_stack - LEAF_MAX - 1, what
            before, after, subtrees, prims = got["top_heights"]
            assert before == after >= 1 and (subtrees, prims) == (0, 0), what
            heights["top"], heights["top_cap"] = got["top_heights"], got["top_height"][3]
        assert (got["top_heights"], got["top_height"][3]) == (heights["top"], heights["top_cap"]), what
        for k in keys:
            if any(m.key == k for m in desc.meshes):
                bt, st, op = gsc.mesh_as_state(k)
                assert (bt, state_fields(st), op) == (SOMETIMES, want[k].fields(), last[k]), (what, k)
        bt, st, op = gsc.mesh_as_state(FLOOR)
        assert (bt, state_fields(st), op) == (STATIC, (0, 0, 0), static_last), what
        assert gsc.as_state()[1] == F, what
        fresh.equal(gsc, desc, "%s %s" % (topology, what))

    def done(keys, op):
        for k in keys:
            want[k].done(op)
            last[k] = op

    def deformed(keys, step):
        return scenes.deform(desc, keys, float(step), amplitude=0.05)

    tl_device = (1, abi.TL_ON_DEVICE, 6, 6)
    tl_host_not_resident = (0, abi.TL_HOST_NOT_TWO_LEVEL, 6, 6)
    # 1. eight deformations: refits; the set is the same from the second on, so its rows and node lists are reused
    for step in range(1, 9):
        assert [want[k].next_op(True) for k in keys] == [U] * 4
        desc = deformed(keys, step)
        push(gsc, desc, keys)
        done(keys, U)
        check("refit %d" % step, keys, (4, 0, 4), (0, 0, ON_DEVICE), (0, 0, 0), tl_device, (0, 0))
    # 2. the ninth: every mesh asks for its fast build; the batch takes the three small ones, the per-mesh build the large one
    assert [want[k].next_op(True) for k in keys] == [F] * 4
    desc = deformed(keys, 9)
    push(gsc, desc, keys)
    done(keys, F)
    check("batch and per-mesh build", keys, (4, 4, 0), (4, 0, ON_DEVICE), (3, 0, 1), tl_device, (1, abi.MESH_TREE_STACK_CAP))
    # 3. the tenth: a refit over the level ranges the two device builds returned (another node list than before: the cache was void)
    assert [want[k].next_op(True) for k in keys] == [U] * 4
    desc = deformed(keys, 10)
    push(gsc, desc, keys)
    done(keys, U)
    check("refit of device-built trees", keys, (4, 0, 4), (0, 0, ON_DEVICE), (0, 0, 0), tl_device, (1, abi.MESH_TREE_STACK_CAP))
    # 4. an instance of mesh 6 with a singular transform joins while all four are updated: the new list holds a baked copy, so every
    #    pending tree goes to the host (each counts as a fast build there), and so does the top level: the arrays are not resident
    desc = dataclasses.replace(deformed(keys, 11), instances=[(k, list(xs) + ([SQUASH] if k == 6 else [])) for k, xs in desc.instances])
    push(gsc, desc, keys)
    done(keys, F)
    check("a baked instance joins", keys, (4, 4, 0), (0, 4, BAKED), (0, 0, 0), (0, abi.TL_HOST_NOT_TWO_LEVEL, 7, 7), (1, abi.MESH_TREE_STACK_CAP),
          baked=True)
    assert gsc.bvh_stats().tri_bytes == (sum(TRIS.values()) + TRIS[6]) * 48          # the baked copy sits behind the mesh trees
    # 5. it leaves again, nothing is updated: the device top-level build re-concatenates without the copy and uploads the rows anew
    desc = dataclasses.replace(desc, instances=[(k, list(xs)[:1] if k == 6 else xs) for k, xs in desc.instances])
    gsc.set_instances(desc.instances)
    done(keys, NONE)
    check("the baked instance leaves", keys, (0, 0, 0), (0, 0, ON_DEVICE), (0, 0, 0), tl_device, (1, abi.MESH_TREE_STACK_CAP))
    assert gsc.bvh_stats().tri_bytes == sum(TRIS.values()) * 48
    # 6. the Static mesh is updated next to the four: its tree is invalid, so nothing is resident and the host builds all five
    desc = deformed(keys + [FLOOR], 12)
    push(gsc, desc, keys + [FLOOR])
    done(keys, F)
    check("a Static mesh is updated", keys, (5, 5, 0), (0, 5, STATIC_MESH), (0, 0, 0), tl_host_not_resident, (1, abi.MESH_TREE_STACK_CAP), static_last=F)
    # 7. mesh 6 is removed and a sphere added into its slot (LIFO reuse): only the new tree is built, all are concatenated anew ...
    gsc.remove(6)
    sv, si = scenes.uv_sphere(0.5, 10, 5)
    new = scenes.MeshDesc(NEW, sv, si, mesh_of(desc, 6).material)
    assert gsc.add_mesh(NEW, sv, si, new.material) == 2
    gsc.set_mesh_build_type(NEW, SOMETIMES)
    desc = dataclasses.replace(desc, meshes=[new if m.key == 6 else m for m in desc.meshes],
                               instances=[((NEW, [scenes.translate(2.0, -0.5, 1.2)]) if k == 6 else (k, xs)) for k, xs in desc.instances])
    keys = [1, NEW, 7, BIG]
    want[NEW], last[NEW] = Heuristic(SOMETIMES), S        # the first build of a mesh is the quality build and leaves its state alone
    gsc.set_instances(desc.instances)
    done([1, 7, BIG], NONE)
    check("a mesh replaced in its slot", keys, (0, 1, 0), (0, 1, ON_DEVICE), (0, 0, 0), tl_host_not_resident, (1, abi.MESH_TREE_STACK_CAP))
    #    ... and the four refit from their new bases
    assert [want[k].next_op(True) for k in keys] == [U] * 4
    desc = deformed(keys, 13)
    push(gsc, desc, keys)
    done(keys, U)
    check("refit after the replacement", keys, (4, 0, 4), (0, 0, ON_DEVICE), (0, 0, 0), tl_device, (1, abi.MESH_TREE_STACK_CAP))
    # 8. quiet frames until a mesh settles: the four changed in the same call, so they settle together, rebuilt on the host
    frames = 0
    while True:
        ops = [want[k].next_op(False) for k in keys]
        gsc.end_frame()
        frames += 1
        assert len(set(ops)) == 1 and ops[0] in (NONE, S) and frames < 64
        done(keys, ops[0])
        for k in keys:
            bt, st, op = gsc.mesh_as_state(k)
            assert (bt, state_fields(st), op) == (SOMETIMES, want[k].fields(), ops[0]), (frames, k)
        if ops[0] == S:
            break
    got = reports(gsc)
    print("%s settled: %s" % (topology, got))
    assert got["update"] == (4, 0, 4, 4)                     # the counters of the last set_instances, and the host's four rebuilds since
    assert got["trees"][2:] == (0, 0, ON_DEVICE) and got["batch"][2:5] == (0, 0, 0)
    assert got["top"] == (0, abi.TL_HOST_QUALITY_BUILD, abi.TL_BUILD_DEVICE, 4096, 6, 6) and got["instancing"] == (2, 1)
    assert got["mesh_heights"] == heights["mesh"] and got["mesh_height"][2:] == (1, abi.MESH_TREE_STACK_CAP)      # quiet frames and the settle rebuild leave the records
    assert (got["top_heights"], got["top_height"][2:]) == (heights["top"], (0, heights["top_cap"]))
    for m in desc.meshes:
        tree_contains_its_triangles(rt, gsc.read_mesh_tree(m.key), "%s settled, mesh %d" % (topology, m.key))
    fresh.equal(gsc, desc, "%s after the settle rebuild" % topology)
    gsc.close()
