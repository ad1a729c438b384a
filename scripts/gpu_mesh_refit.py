"""Cost of animating a mesh in the two-level form: the sr_scene_set_instances that applies a sr_scene_update_mesh, with the mesh
Static (its tree is rebuilt on the host, every mesh's records are uploaded again, the top level is built on the host: the only
path there was before sr_scene_set_mesh_build_type) against the mesh RapidlyChanging (device refit of its tree).

  step CASE TYPE   one animation step (update_mesh + set_instances), TYPE = static | updatable: wall clock of set_instances with the
                   event timing off, then, with it on, the split sr_scene_mesh_update_info / sr_scene_top_level_info report: host
                   tree build, record-rewrite kernel, refit launches, top-level build. The updatable run forces SR_OP_UPDATE, so
                   every measured step is a refit (the heuristic would make every ninth a host rebuild, i.e. a `static` step).
  drift            device time of one 1080p RIS + final frame after eight consecutive refits of a progressively deformed mesh,
                   against the same frame after a fresh host build of the same vertices (what the eight-update limit bounds)

Cases: one deforming sphere of 1 k, 21 k, 250 k and 1 M triangles (four instances, over a ground quad), and 100 deforming spheres of
1 k triangles each. Median (min-max) of 20 calls after 3 warm-ups, every step in a fresh child process under its own time limit;
stops at the first step that fails.

  python scripts/gpu_mesh_refit.py [--out profiles/mesh_refit.json] [--label NAME] [--only CASE]

A library without sr_scene_set_mesh_build_type (SUNRAY_HIP_LIB pointing at a build of an older commit) runs the static steps only;
--label keeps its figures apart (e.g. --label parent) in the same output file."""
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS, WARMUP = 20, 3
# case -> (segments, rings, meshes): 2 * segments * (rings - 1) triangles per sphere
CASES = {"1k": (32, 17, 1), "21k": (128, 83, 1), "250k": (500, 251, 1), "1m": (1000, 501, 1), "100x1k": (32, 17, 100)}


def has_build_type():
    from sunray_amd._lib import lib
    return hasattr(lib(), "sr_scene_set_mesh_build_type")


def make(case):
    """-> (description, keys of the deforming meshes)."""
    import numpy as np
    from sunray_amd import abi, scenes
    seg, rings, n = CASES[case]
    s = scenes.SceneDesc("refit_" + case, camera_pos=(0.0, 6.0, 16.0), camera_target=(0.0, 1.0, 0.0), fov_y=50.0)
    v, idx = scenes.uv_sphere(1.0, seg, rings)
    mat = abi.material(base_color=(0.7, 0.5, 0.3, 1.0), roughness=0.4)
    rng = np.random.default_rng(3)
    keys = []
    for m in range(n):
        s.meshes.append(scenes.MeshDesc(m + 1, v, idx, mat))
        keys.append(m + 1)
        xs = [scenes.rotate_y(float(rng.uniform(0, 6.28)), float(rng.uniform(-8, 8)), float(rng.uniform(0.8, 3.0)), float(rng.uniform(-8, 8)), float(rng.uniform(0.5, 1.2)))
              for _ in range(4 if n == 1 else 1)]
        s.instances.append((m + 1, xs))
    gv, gi = scenes.quad((-20, 0, -20), (-20, 0, 20), (20, 0, 20), (20, 0, -20), (0, 1, 0))
    s.meshes.append(scenes.MeshDesc(n + 1, gv, gi, abi.material(base_color=(0.7, 0.7, 0.7, 1.0), roughness=0.8)))
    s.instances.append((n + 1, [scenes.translate(0, 0, 0)]))
    lv, li = scenes.quad((-1, 0, -1), (1, 0, -1), (1, 0, 1), (-1, 0, 1), (0, -1, 0))
    s.meshes.append(scenes.MeshDesc(n + 2, lv, li, abi.material(base_color=(1, 1, 1, 1), emissive_factor=(1.0, 0.95, 0.85), emissive_strength=18.0)))
    s.instances.append((n + 2, [scenes.translate(0.0, 9.0, 0.0, 2.0)]))
    return s, keys


def stats(xs):
    import numpy as np
    return {"median": float(np.median(xs)), "min": float(np.min(xs)), "max": float(np.max(xs))}


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def set_list(sc, arrays):
    from sunray_amd._lib import check, lib
    keys, counts, xf = arrays
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    return timed(lambda: check(lib().sr_scene_set_instances(sc._h, p(keys), p(counts), C.c_uint32(len(keys)), p(xf))))


def step_case(case, kind):
    from sunray_amd import abi, runtime as rt, scenes
    from sunray_amd.runtime import _instance_arrays
    desc, keys = make(case)
    m = desc.meshes[0]
    verts = [scenes.deform_vertices(m.vertices, m.indices, ph) for ph in (1.0, 2.0)]       # every sphere takes the same two poses
    sc = rt.Scene(0, instancing="two_level").load(desc)
    if kind == "updatable":
        for k in keys:
            sc.set_mesh_build_type(k, abi.BUILD_RAPIDLY_CHANGING)
    arrays = _instance_arrays(desc.instances)
    wall, upd, rows = [], [], []
    for timing in (False, True):          # wall clock with the event timing off, as a renderer runs it; then the kernel times
        sc.enable_timing(timing)
        for k in range(WARMUP + REPS):
            t_upd = timed(lambda: [sc.update_mesh(key, verts[k & 1]) for key in keys])
            if kind == "updatable":
                sc.force_next_op(abi.OP_UPDATE)
            t_set = set_list(sc, arrays)
            i, tl = sc.mesh_update_info(), sc.top_level_info()
            assert sc.two_level()
            if kind == "updatable":
                assert (i.blas_refitted, i.blas_rebuilt) == (len(keys), 0), (i.blas_refitted, i.blas_rebuilt)
            else:
                assert i.blas_rebuilt == len(keys)
            if k < WARMUP:
                continue
            if not timing:
                wall.append(t_set); upd.append(t_upd)
            else:
                rows.append((i.blas_build_ms, i.flatten_ms, i.refit_ms, tl.build_ms))
    out = {"set_instances_ms": stats(wall), "update_mesh_ms": stats(upd)}
    out.update({n: stats([r[j] for r in rows]) for j, n in enumerate(("mesh_tree_build_ms", "rewrite_kernel_ms", "refit_kernels_ms", "top_level_ms"))})
    out["mesh_triangles"], out["meshes"], out["calls"], out["top_level_on_device"] = len(m.indices) // 3, len(keys), REPS, int(sc.top_level_info().on_device)
    return out


def step_drift():
    from sunray_amd import abi, runtime as rt, scenes
    from sunray_amd.runtime import _instance_arrays
    desc, keys = make("250k")
    m = desc.meshes[0]
    sc = rt.Scene(0, instancing="two_level").load(desc)
    sc.set_mesh_build_type(keys[0], abi.BUILD_RAPIDLY_CHANGING)
    arrays = _instance_arrays(desc.instances)
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
        scene.enable_timing(False)
        return stats(t[3:])
    v = m.vertices
    for refit in range(1, 9):                                   # progressive: every step deforms the step before
        v = scenes.deform_vertices(v, m.indices, float(refit), amplitude=0.25)
        sc.update_mesh(keys[0], v)
        set_list(sc, arrays)
        assert sc.mesh_update_info().blas_refitted == 1
    refitted = frame_ms(sc)
    probe = rt.Scene(0, instancing="two_level").load(scenes.with_mesh_vertices(desc, keys[0], v))     # a fresh host build of the same vertices
    fresh = frame_ms(probe)
    probe.close()
    return {"extent": "%dx%d" % (W, H), "mesh_triangles": len(m.indices) // 3, "refits": 8, "refitted_frame_ms": refitted, "fresh_build_frame_ms": fresh}


def run_step(args, limit):
    """One step in a fresh process under its own time limit; its JSON result is the last line it prints."""
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step"] + args
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    if r.returncode != 0:
        print("step %s ended with status %d: stopping here" % (" ".join(args), r.returncode), flush=True)
        sys.exit(r.returncode)
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    argv = sys.argv[1:]
    if argv[:1] == ["--step"]:
        print(json.dumps(step_drift() if argv[1] == "drift" else step_case(argv[1], argv[2])))
        return
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "mesh_refit.json")
    label = argv[argv.index("--label") + 1] if "--label" in argv else "this"
    doc = json.load(open(out_path)) if os.path.exists(out_path) else {}
    doc["workload"] = ("two-level form, sr_scene_set_instances after sr_scene_update_mesh of one deforming sphere (four instances) or of 100 spheres; "
                       "median (min-max) of %d calls after %d warm-ups, wall clock with the event timing off, kernel times from HIP events" % (REPS, WARMUP))
    res = doc.setdefault(label, {})

    def save():                                                    # after every step: a later failure keeps what was measured
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")
    steps = []
    for case in CASES:
        steps += [[case, "static"]] + ([[case, "updatable"]] if has_build_type() else [])
    if has_build_type():
        steps.append(["drift"])
    if "--only" in argv:
        steps = [x for x in steps if x[0] == argv[argv.index("--only") + 1]]
    for args in steps:
        r = run_step(args, 300)
        node = res
        for a in args[:-1]:
            node = node.setdefault(a, {})
        node[args[-1]] = r
        save()
        print("%-20s %s" % (" ".join(args), json.dumps({k: (round(v["median"], 3) if isinstance(v, dict) and "median" in v else v) for k, v in r.items()})), flush=True)


if __name__ == "__main__":
    main()
