"""Cost of the frame's light table on the host (SR_LIGHTS_HOST, the default) against on the device (SR_LIGHTS_DEVICE): one animation
step (vertex update from a device pointer + sr_scene_set_instances, SR_OP_UPDATE in the one-level form) on

  heightfield_emissive   heightfield() with the terrain's material made emissive: 999 698 lights, the terrain updated by device pointer
  instanced_field_lamp   instanced_field(300) with its lamp quad (2 triangles x 4 instances) deformed: small and launch-bound
  skinned_emissive       the skinned fixture (tests/golden/skinned_bar.glb) with emissive skinned meshes, posed through skin_mesh
  blob_transform_only    100 instances of an emissive 528-triangle blob (52 800 lights), transforms change, no mesh update

for three columns: the library at PARENT_LIB (a build of the parent commit, loaded through SUNRAY_HIP_LIB), this library in host
mode and this library in device mode. Median (min-max) of 20 steps after 3 warm-ups, one fresh process per cell under its own time
limit, wall clock with the event timing off; a second loop with the timing on gives the SrLightTableInfo split. Stops at the first
cell that fails.

  python scripts/gpu_light_table.py PARENT_LIB [--out profiles/light_table.json]

The rule, set beforehand: device mode is justified on a scene where it beats this library's host mode by more than the two
min-max spreads combined, and this library's host mode must not be slower than the parent's by more than those spreads."""
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS, WARMUP = 20, 3
CASES = ("heightfield_emissive", "instanced_field_lamp", "skinned_emissive", "blob_transform_only")
UPDATE = 3
GLOW = (1.0, 0.9, 0.7, 2.0)


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


def make(case):
    """-> (desc, update(scene, k) or None, [instance arrays] to alternate between)."""
    import numpy as np
    import torch
    from sunray_amd import abi, runtime as rt, scenes
    from sunray_amd.runtime import _instance_arrays
    if case == "skinned_emissive":
        path = os.path.join(ROOT, "tests", "golden", "skinned_bar.glb")
        parsed, g = rt.gltf_parse(path), rt.Gltf(path)
        desc, rigs = scenes.SceneDesc("skinned_bar"), {}
        for b, blas in enumerate(parsed["blases"]):
            mat = blas["material"].copy()
            skin, inf = g.blas_skin(b)
            if skin >= 0:
                rigs[b + 1] = inf
                mat["emissive_factor"] = GLOW
            desc.meshes.append(scenes.MeshDesc(b + 1, blas["vertices"], blas["indices"], mat))
        desc.instances = [(b + 1, [t]) for b, t in parsed["instances"]]
        poses = [g.pose(0, t, 0)[1] for t in (0.19, 0.38)]
        n_joints = len(g.skin(0)[1])

        def prepare(sc):
            for key, inf in rigs.items():
                sc.set_mesh_skin(key, inf, n_joints)

        def update(sc, k):
            for key in rigs:
                sc.skin_mesh(key, poses[k & 1])
        return desc, prepare, update, [_instance_arrays(desc.instances)] * 2
    if case == "blob_transform_only":
        desc = scenes.SceneDesc("emissive_blobs")
        v, idx = scenes.uv_sphere(1.0, 24, 12)
        desc.meshes.append(scenes.MeshDesc(1, v, idx, abi.material(base_color=(1, 1, 1, 1), emissive_factor=GLOW[:3], emissive_strength=GLOW[3])))
        gv, gi = scenes.quad((-30, 0, -30), (-30, 0, 30), (30, 0, 30), (30, 0, -30), (0, 1, 0))
        desc.meshes.append(scenes.MeshDesc(2, gv, gi, abi.material(base_color=(0.7, 0.7, 0.7, 1.0), roughness=0.8)))
        lists = []
        for phase in (0.0, 0.05):
            xf = [scenes.rotate_y(0.3 * i + phase, 2.5 * (i % 10) - 11.0, 1.5 + phase, 2.5 * (i // 10) - 11.0, 0.5) for i in range(100)]
            lists.append(_instance_arrays([(1, xf), (2, [scenes.translate(0, 0, 0)])]))
        desc.instances = [(1, xf), (2, [scenes.translate(0, 0, 0)])]
        return desc, None, None, lists
    if case == "heightfield_emissive":
        desc, key = scenes.heightfield(), 1
        m = next(x for x in desc.meshes if x.key == key)
        mat = m.material.copy()
        mat["emissive_factor"] = GLOW
        desc.meshes = [scenes.MeshDesc(m.key, m.vertices, m.indices, mat) if x.key == key else x for x in desc.meshes]
    else:
        desc = scenes.instanced_field(300)
        instanced = {k for k, _ in desc.instances}
        key = next(x.key for x in desc.meshes if float(x.material["emissive_factor"][3]) > 0 and x.key in instanced)
    m = next(x for x in desc.meshes if x.key == key)
    tensors = [torch.from_numpy(np.ascontiguousarray(scenes.deform_vertices(m.vertices, m.indices, ph)).view("u1").copy()).to("cuda:0") for ph in (1.0, 2.0)]
    torch.cuda.synchronize()
    return desc, None, (lambda sc, k: sc.update_mesh_device(key, tensors[k & 1])), [_instance_arrays(desc.instances)] * 2


def step(case, mode):
    from sunray_amd import runtime as rt
    desc, prepare, update, lists = make(case)
    sc = rt.Scene(0, instancing="flat")
    has_mode = hasattr(rt.lib(), "sr_scene_set_light_table_build")
    assert has_mode or mode == "host"
    if has_mode:
        sc.set_light_table_build(mode)
    sc.load(desc)
    if prepare:
        prepare(sc)
    wall, rows = [], []
    for timing in (False, True):          # wall clock with the event timing off, as a renderer runs it; then the split
        sc.enable_timing(timing)
        for k in range(WARMUP + REPS):
            t_upd = timed(lambda: update(sc, k)) if update else 0.0
            sc.force_next_op(UPDATE)
            t_set = set_list(sc, lists[k & 1])
            assert sc.as_state()[1] == UPDATE
            if k < WARMUP:
                continue
            if not timing:
                wall.append((t_upd + t_set, t_upd, t_set, sc.mesh_update_info().tables_ms))
            elif has_mode:
                i = sc.light_table_info()
                assert i.on_device == (1 if mode == "device" else 0)
                rows.append((i.positions_ms, i.table_ms, i.host_ms, i.positions_rewritten, i.entries_uploaded, i.arena_uploads))
    out = {n: stats([r[j] for r in wall]) for j, n in enumerate(("step_ms", "update_ms", "set_instances_ms", "tables_ms"))}
    if rows:
        out.update({n: stats([r[j] for r in rows]) for j, n in enumerate(("positions_kernel_ms", "table_kernel_ms", "host_path_ms"))})
        out["positions_rewritten"], out["entries_uploaded_after_warmup"], out["arena_uploads_after_warmup"] = int(rows[-1][3]), int(sum(r[4] for r in rows)), int(sum(r[5] for r in rows))
        i = sc.light_table_info()
        out["num_lights"], out["arena_entries"], out["arena_fetches"] = int(i.num_lights), int(i.arena_entries), int(i.arena_fetches)
    out["host_fetches"] = int(sum(sc.mesh_vertex_info(m.key).host_fetches for m in desc.meshes))
    out["triangles"], out["calls"] = int(sc.bvh_stats().n_triangles), REPS
    return out


def run_step(args, limit, env):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step"] + args
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, env=env)
    if r.returncode != 0:
        print("step %s ended with status %d: stopping here" % (" ".join(args), r.returncode), flush=True)
        sys.exit(r.returncode)
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    argv = sys.argv[1:]
    if argv[:1] == ["--step"]:
        print(json.dumps(step(*argv[1:])))
        return
    parent_lib = argv[0]
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "light_table.json")
    doc = {"workload": ("one animation step (vertex update from a device pointer + sr_scene_set_instances, SR_OP_UPDATE, one-level form); median (min-max) of "
                        "%d steps after %d warm-ups, one process per cell, wall clock with the event timing off; kernel and host-path times from a second "
                        "loop with the timing on" % (REPS, WARMUP)), "cases": {}}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")
    for case in CASES:
        node = doc["cases"].setdefault(case, {})
        for name, mode, lib_path in (("parent", "host", parent_lib), ("host", "host", None), ("device", "device", None)):
            env = dict(os.environ)
            env.pop("SUNRAY_HIP_LIB", None)
            env.pop("SR_LIGHT_TABLE", None)
            if lib_path:
                env["SUNRAY_HIP_LIB"] = os.path.abspath(lib_path)
            node[name] = run_step([case, mode], 300, env)
            save()
            print("%-22s %-8s %s" % (case, name, json.dumps({k: (round(v["median"], 3) if isinstance(v, dict) else v) for k, v in node[name].items()})), flush=True)
        spread = lambda r: r["step_ms"]["max"] - r["step_ms"]["min"]        # noqa: E731
        med = lambda r: r["step_ms"]["median"]                               # noqa: E731
        node["verdict"] = {
            "device_gain_ms": med(node["host"]) - med(node["device"]), "device_spreads_ms": spread(node["host"]) + spread(node["device"]),
            "device_beats_host": med(node["host"]) - med(node["device"]) > spread(node["host"]) + spread(node["device"]),
            "host_loss_vs_parent_ms": med(node["host"]) - med(node["parent"]), "host_spreads_ms": spread(node["host"]) + spread(node["parent"]),
            "host_not_slower_than_parent": med(node["host"]) - med(node["parent"]) <= spread(node["host"]) + spread(node["parent"])}
        save()
        print("%-22s verdict  %s" % (case, json.dumps(node["verdict"])), flush=True)


if __name__ == "__main__":
    main()
