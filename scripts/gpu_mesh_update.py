"""Cost of animating a mesh: Scene.update_mesh + set_instances against the only route there was before (remove + add_mesh +
set_instances), on the 1M-triangle heightfield (one mesh) and on instanced_field(300) (a blob mesh instanced 100 times).

  route          one animation step through update_mesh + set_instances, for each op (update, fast_build, slow_build): wall clock
                 of both calls and the split of sr_scene_mesh_update_info (validation + host copy, H2D, instance + light tables,
                 flatten + reshade kernel, refit kernels; the kernel times from HIP events)
  remove_add     the same step through remove + add_mesh + set_instances (any library)
  transform_only a transform-only Update (no mesh changed): wall clock, and the plain flatten / refit kernel times where the
                 library reports them; against `route update` this shows what the shading rewrite adds to the flatten
  drift          both passes of a 1080p frame after 1, 4 and 8 refits of a progressively deformed mesh against a fresh SAH build
                 of the same vertices
  two_level      the step in the two-level form: the whole set_instances and the host rebuild of the dirty mesh's tree
  device_route   (--device-compare only) the step with the vertices taken from a host pointer (update_mesh) or from a device
                 tensor prepared before the clock starts (update_mesh_device), on the heightfield and instanced_field(300) in the
                 one-level form (SR_OP_UPDATE) and on a 250 000-triangle updatable sphere in the two-level form (device refit)

Median (min-max) of 20 calls after 3 warm-ups, every step in a fresh child process under its own time limit; stops at the
first step that fails.

  python scripts/gpu_mesh_update.py [--out profiles/mesh_update.json] [--label NAME] [--only STEP]

  python scripts/gpu_mesh_update.py --device-compare PARENT_LIB [--out profiles/mesh_update_device.json]

A library without update_mesh (SUNRAY_HIP_LIB pointing at a build of an older commit) runs remove_add and transform_only only;
--label keeps its figures apart (e.g. --label parent) in the same output file. --device-compare measures, in one run, the
host-pointer route of the library at PARENT_LIB (a build of the parent commit, loaded through SUNRAY_HIP_LIB), the host-pointer
route of this tree and the device-pointer route, each case in a fresh child process, and writes the verdicts next to the figures:
the device route is justified on the heightfield if it beats this tree's host route by more than the two min-max spreads
combined, and this tree's host route must not be slower than the parent's by more than those spreads."""
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS, WARMUP = 20, 3
SCENES = ("heightfield_1m", "instanced_field_300")
OPS = {"update": 3, "fast_build": 2, "slow_build": 1}


def has_update_mesh():
    from sunray_amd._lib import lib
    return hasattr(lib(), "sr_scene_update_mesh")


def make(what, form="flat"):
    """-> (scene, desc, key of the animated mesh, [vertex array A, B] to alternate between)."""
    from sunray_amd import runtime as rt, scenes
    desc = scenes.heightfield() if what == "heightfield_1m" else scenes.instanced_field(300)
    key = 1
    m = next(x for x in desc.meshes if x.key == key)
    verts = [scenes.deform_vertices(m.vertices, m.indices, ph) for ph in (1.0, 2.0)]
    sc = rt.Scene(0, instancing=form).load(desc)
    return sc, desc, m, verts


def stats(xs):
    import numpy as np
    return {"median": float(np.median(xs)), "min": float(np.min(xs)), "max": float(np.max(xs))}


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def instance_arrays(desc):
    from sunray_amd.runtime import _instance_arrays
    return _instance_arrays(desc.instances)


def set_list(sc, arrays):
    from sunray_amd._lib import check, lib
    keys, counts, xf = arrays
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    return timed(lambda: check(lib().sr_scene_set_instances(sc._h, p(keys), p(counts), C.c_uint32(len(keys)), p(xf))))


def step_route(what, op):
    sc, desc, m, verts = make(what)
    arrays = instance_arrays(desc)
    sc.enable_timing(True)
    rows = []
    for k in range(WARMUP + REPS):
        t_upd = timed(lambda: sc.update_mesh(m.key, verts[k & 1]))
        sc.force_next_op(OPS[op])
        t_set = set_list(sc, arrays)
        assert sc.as_state()[1] == OPS[op]
        i = sc.mesh_update_info()
        assert i.dirty_meshes == 1 and i.reshaded == (1 if op == "update" else 0)
        rows.append((t_upd + t_set, t_upd, t_set, i.validate_copy_ms, i.h2d_ms, i.tables_ms, i.flatten_ms, i.refit_ms))
    rows = rows[WARMUP:]
    names = ("step_ms", "update_mesh_ms", "set_instances_ms", "validate_copy_ms", "h2d_ms", "tables_ms", "flatten_reshade_ms", "refit_ms")
    out = {n: stats([r[j] for r in rows]) for j, n in enumerate(names)}
    out["triangles"], out["calls"] = int(sc.bvh_stats().n_triangles), REPS
    return out


def step_remove_add(what):
    sc, desc, m, verts = make(what)
    arrays = instance_arrays(desc)
    rows = []
    for k in range(WARMUP + REPS):
        t_mesh = timed(lambda: (sc.remove(m.key), sc.add_mesh(m.key, verts[k & 1], m.indices, m.material)))
        t_set = set_list(sc, arrays)
        rows.append((t_mesh + t_set, t_mesh, t_set))
    rows = rows[WARMUP:]
    out = {n: stats([r[j] for r in rows]) for j, n in enumerate(("step_ms", "remove_add_ms", "set_instances_ms"))}
    out["triangles"], out["calls"], out["op"] = int(sc.bvh_stats().n_triangles), REPS, int(sc.as_state()[1])
    return out


def step_transform_only(what):
    import numpy as np
    sc, desc, m, verts = make(what)
    keys, counts, xf = instance_arrays(desc)
    lists = [xf, xf.copy()]
    lists[1][:, 7] += np.float32(0.01)
    info = has_update_mesh()
    wall, rows = [], []
    for timing in ((False, True) if info else (False,)):          # wall clock with the event timing off, as a renderer runs it; then the kernel times
        sc.enable_timing(timing)
        for k in range(WARMUP + REPS):
            sc.force_next_op(OPS["update"])
            t = set_list(sc, (keys, counts, lists[(k + 1) & 1]))
            assert sc.as_state()[1] == OPS["update"]
            if k < WARMUP:
                continue
            if not timing:
                wall.append(t)
            else:
                i = sc.mesh_update_info()
                assert i.reshaded == 0
                rows.append((i.tables_ms, i.flatten_ms, i.refit_ms))
    out = {"set_instances_ms": stats(wall)}
    out.update({n: stats([r[j] for r in rows]) for j, n in enumerate(("tables_ms", "flatten_ms", "refit_ms")) if rows})
    out["triangles"], out["calls"] = int(sc.bvh_stats().n_triangles), REPS
    return out


def step_drift(what):
    from sunray_amd import runtime as rt, scenes
    sc, desc, m, _ = make(what)
    arrays = instance_arrays(desc)
    W, H = 1920, 1080
    fr = rt.DeviceFrame(W, H, scenes.white_noise_rgba8())

    def frame_ms(scene):
        scene.enable_timing(True)
        prev, t = None, []
        for f in range(8):
            mat = rt.camera_matrices(desc.camera_pos, desc.camera_target, desc.fov_y, W, H, prev)
            prev = list(mat.view_proj)
            scene.trace_ris(fr, mat, f); scene.trace_final(fr, mat, f)
            t.append(scene.read_timing(0)[0] + scene.read_timing(1)[0])
        return stats(t[3:])
    out, v, refits = {"extent": "%dx%d" % (W, H)}, m.vertices, 0
    for target in (1, 4, 8):
        while refits < target:                              # progressive: every step deforms the step before
            refits += 1
            v = scenes.deform_vertices(v, m.indices, float(refits), amplitude=0.25)
            sc.update_mesh(m.key, v)
            sc.force_next_op(OPS["update"])
            set_list(sc, arrays)
        refitted = frame_ms(sc)
        probe = rt.Scene(0).load(scenes.with_mesh_vertices(desc, m.key, v))      # a fresh SAH build of the same vertices
        fresh = frame_ms(probe)
        probe.close()
        out["after_%d_refits" % target] = {"refitted_frame_ms": refitted, "fresh_sah_frame_ms": fresh}
    return out


def step_two_level(what):
    sc, desc, m, verts = make(what, "two_level")
    arrays = instance_arrays(desc)
    rows = []
    for k in range(WARMUP + REPS):
        t_upd = timed(lambda: sc.update_mesh(m.key, verts[k & 1]))
        t_set = set_list(sc, arrays)
        i = sc.mesh_update_info()
        assert sc.two_level() and i.blas_rebuilt == 1
        rows.append((t_upd + t_set, t_upd, t_set, i.blas_build_ms))
    rows = rows[WARMUP:]
    out = {n: stats([r[j] for r in rows]) for j, n in enumerate(("step_ms", "update_mesh_ms", "set_instances_ms", "mesh_tree_rebuild_ms"))}
    out["triangles"], out["mesh_triangles"], out["calls"] = int(sc.bvh_stats().n_triangles), len(m.indices) // 3, REPS
    return out


DEVICE_CASES = ("heightfield_1m", "instanced_field_300", "sphere_250k")


def step_device_route(case, route):
    """route: "host" (update_mesh from numpy) or "device" (update_mesh_device from a tensor that is ready before the clock starts)."""
    import torch
    from sunray_amd import abi, runtime as rt, scenes
    two_level = case == "sphere_250k"
    if two_level:
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        from gpu_mesh_refit import make as make_sphere
        desc, keys = make_sphere("250k")
        m = desc.meshes[0]
        verts = [scenes.deform_vertices(m.vertices, m.indices, ph) for ph in (1.0, 2.0)]
        sc = rt.Scene(0, instancing="two_level").load(desc)
        sc.set_mesh_build_type(keys[0], abi.BUILD_RAPIDLY_CHANGING)
    else:
        sc, desc, m, verts = make(case)
    arrays = instance_arrays(desc)
    tensors = [torch.from_numpy(v.view("u1").copy()).to("cuda:0") for v in verts] if route == "device" else None
    torch.cuda.synchronize()
    has_info = hasattr(sc, "mesh_vertex_info") and hasattr(rt.lib(), "sr_scene_mesh_vertex_info")
    wall, rows = [], []
    for timing in (False, True):          # wall clock with the event timing off, as a renderer runs it; then the kernel times
        sc.enable_timing(timing)
        for k in range(WARMUP + REPS):
            if route == "device":
                t_upd = timed(lambda: sc.update_mesh_device(m.key, tensors[k & 1]))
            else:
                t_upd = timed(lambda: sc.update_mesh(m.key, verts[k & 1]))
            sc.force_next_op(OPS["update"])
            t_set = set_list(sc, arrays)
            i = sc.mesh_update_info()
            if two_level:
                assert sc.two_level() and (i.blas_refitted, i.blas_rebuilt) == (1, 0)
            else:
                assert sc.as_state()[1] == OPS["update"] and (i.dirty_meshes, i.reshaded) == (1, 1)
            if k < WARMUP:
                continue
            if not timing:
                wall.append((t_upd + t_set, t_upd, t_set, i.validate_copy_ms, i.h2d_ms, i.tables_ms))
            else:
                vi = sc.mesh_vertex_info(m.key) if has_info else None
                rows.append((vi.check_ms if vi else 0.0, vi.copy_ms if vi else 0.0, i.flatten_ms, i.refit_ms))
    out = {n: stats([r[j] for r in wall]) for j, n in enumerate(("step_ms", "update_mesh_ms", "set_instances_ms", "validate_copy_ms", "h2d_ms", "tables_ms"))}
    out.update({n: stats([r[j] for r in rows]) for j, n in enumerate(("check_ms", "copy_ms", "flatten_reshade_ms", "refit_ms"))})
    if has_info:
        vi = sc.mesh_vertex_info(m.key)
        out["host_fetches"], out["host_stale"] = int(vi.host_fetches), int(vi.host_stale)
        assert route != "device" or (vi.host_fetches, vi.host_stale, vi.last_from_device) == (0, 1, 1)
    out["triangles"], out["mesh_vertices"], out["calls"], out["form"] = int(sc.bvh_stats().n_triangles), len(m.vertices), REPS, "two_level" if two_level else "flat"
    return out


def device_compare(parent_lib, out_path):
    """The three routes of every case, one after the other in fresh processes; figures and verdicts into out_path."""
    doc = {"workload": ("one animation step (vertex update + sr_scene_set_instances) of one mesh: the 999 698-triangle heightfield and "
                        "instanced_field(300) in the one-level form (SR_OP_UPDATE), a 250 000-triangle updatable sphere in the two-level form "
                        "(device refit); median (min-max) of %d calls after %d warm-ups, wall clock around the calls with the event timing off, "
                        "check_ms / copy_ms / kernel times from HIP events in a second loop; the device tensor is prepared before the clock starts"
                        % (REPS, WARMUP)), "cases": {}}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")
    for case in DEVICE_CASES:
        node = doc["cases"].setdefault(case, {})
        for name, route, lib_path in (("parent_host", "host", parent_lib), ("host", "host", None), ("device", "device", None)):
            env = dict(os.environ)
            env.pop("SUNRAY_HIP_LIB", None)
            if lib_path:
                env["SUNRAY_HIP_LIB"] = os.path.abspath(lib_path)
            node[name] = run_step(["device_route", case, route], 420, env)
            save()
            print("%-22s %-12s %s" % (case, name, json.dumps({k: (round(v["median"], 3) if isinstance(v, dict) else v) for k, v in node[name].items()})), flush=True)
        spread = lambda r: r["step_ms"]["max"] - r["step_ms"]["min"]        # noqa: E731
        med = lambda r: r["step_ms"]["median"]                               # noqa: E731
        node["verdict"] = {
            "device_gain_ms": med(node["host"]) - med(node["device"]), "device_spreads_ms": spread(node["host"]) + spread(node["device"]),
            "device_beats_host": med(node["host"]) - med(node["device"]) > spread(node["host"]) + spread(node["device"]),
            "host_loss_vs_parent_ms": med(node["host"]) - med(node["parent_host"]), "host_spreads_ms": spread(node["host"]) + spread(node["parent_host"]),
            "host_not_slower_than_parent": med(node["host"]) - med(node["parent_host"]) <= spread(node["host"]) + spread(node["parent_host"])}
        save()
        print("%-22s verdict      %s" % (case, json.dumps(node["verdict"])), flush=True)


def run_step(args, limit, env=None):
    """One step in a fresh process under its own time limit; its JSON result is the last line it prints."""
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step"] + args
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, env=env)
    if r.returncode != 0:
        print("step %s ended with status %d: stopping here" % (" ".join(args), r.returncode), flush=True)
        sys.exit(r.returncode)
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    argv = sys.argv[1:]
    if argv[:1] == ["--step"]:
        fn = {"route": step_route, "remove_add": step_remove_add, "transform_only": step_transform_only, "drift": step_drift, "two_level": step_two_level,
              "device_route": step_device_route}[argv[1]]
        print(json.dumps(fn(*argv[2:])))
        return
    if "--device-compare" in argv:
        device_compare(argv[argv.index("--device-compare") + 1], argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "mesh_update_device.json"))
        return
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "mesh_update.json")
    label = argv[argv.index("--label") + 1] if "--label" in argv else "this"
    doc = json.load(open(out_path)) if os.path.exists(out_path) else {}
    doc["workload"] = ("one animation step of mesh 1 (heightfield: 999 698 triangles, one instance; instanced_field(300): 528 triangles, 100 instances); "
                       "median (min-max) of %d calls after %d warm-ups, wall clock around the calls, kernel times from HIP events" % (REPS, WARMUP))
    res = doc.setdefault(label, {})

    def save():                                                    # after every step: a later failure keeps what was measured
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")
    steps = []
    for what in SCENES:
        steps += [["remove_add", what], ["transform_only", what]]
        if has_update_mesh():
            steps += [["route", what, op] for op in OPS] + [["two_level", what]]
    if has_update_mesh():
        steps.append(["drift", SCENES[0]])
    if "--only" in argv:                                           # e.g. --only transform_only: re-measure one kind of step
        steps = [x for x in steps if x[0] == argv[argv.index("--only") + 1]]
    for args in steps:
        r = run_step(args, 420)
        node = res
        for a in args[:-1]:
            node = node.setdefault(a, {})
        node[args[-1]] = r
        save()
        print("%-40s %s" % (" ".join(args), json.dumps({k: (round(v["median"], 3) if isinstance(v, dict) and "median" in v else v) for k, v in r.items()})), flush=True)


if __name__ == "__main__":
    main()
