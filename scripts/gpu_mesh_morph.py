"""Cost of blending a mesh's morph targets with the library's kernel (Scene.pose_mesh) against the routes there were before it, on
the 1M-triangle heightfield (one mesh, 501 264 vertices) with 16 synthetic targets attached (position, normal and tangent deltas
on every vertex), of which 1, 4 and 16 are active, one pose per step alternating between two sets of weights:

  morph          (a) Scene.pose_mesh with weights: the whole call (wall clock) and SrMeshMorphInfo.morph_ms (kernel + read-back,
                     events), with copy_ms of the same call: the device-to-device copy of the posed vertices into the mesh's buffer
  torch_device   (b) the fastest route before: the same blend computed by torch ops on the GPU (timed with events), then
                     Scene.update_mesh_device (wall clock; check_ms and copy_ms)
  numpy_host     (c) the blend computed by numpy on the host, then Scene.update_mesh through the host pointer (3 calls: it is slow)
  morph_skin     (d) the price of the unfused second pass: Scene.pose_mesh with weights and the joint matrices of a synthetic rig of
                     64 joints (two kernels, the morphed vertices cross memory once more) against Scene.skin_mesh alone

Every step is followed by the set_instances that applies it (SR_OP_UPDATE, forced; reported, not part of the comparison: it is
the same work on every route). Median (min-max) of 20 calls after 3 warm-ups, every route in a fresh child process under its own
time limit; stops at the first route that fails. No figure is fixed in advance: the result is what profiles/mesh_morph.json says.

  python scripts/gpu_mesh_morph.py [--out profiles/mesh_morph.json] [--only ROUTE]
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

REPS, WARMUP, HOST_REPS, N_TARGETS, ACTIVE = 20, 3, 3, 16, (1, 4, 16)
ROUTES = ("morph", "torch_device", "numpy_host", "morph_skin")


def stats(xs):
    import numpy as np
    return {"median": float(np.median(xs)), "min": float(np.min(xs)), "max": float(np.max(xs))}


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def deltas_for(m):
    """16 targets for mesh m: a smooth bump per target, with normal and tangent deltas that lean with it -> [16, n] abi.MORPH_DELTA."""
    import numpy as np
    from sunray_amd import abi
    x, z = m.vertices["position"][:, 0], m.vertices["position"][:, 2]
    d = np.zeros((N_TARGETS, len(m.vertices)), dtype=abi.MORPH_DELTA)
    for k in range(N_TARGETS):
        bump = (0.05 * np.sin(0.9 * (k + 1) * x + 0.3 * k) * np.cos(0.7 * (k + 1) * z)).astype(np.float32)
        d["position"][k][:, 1] = bump
        d["normal"][k][:, 0], d["normal"][k][:, 2] = -0.5 * bump, 0.25 * bump
        d["tangent"][k][:, 1] = 0.5 * bump
    return d


def make():
    """-> (scene, desc, the heightfield mesh, deltas [16, n])."""
    from sunray_amd import runtime as rt, scenes
    desc = scenes.heightfield()
    m = next(x for x in desc.meshes if x.key == 1)
    sc = rt.Scene(0, instancing="flat").load(desc)
    sc.enable_timing(True)
    return sc, desc, m, deltas_for(m)


def weights(n_active, k):
    """n_active weights that are not 0, spread over the 16 targets; two sets in turn."""
    import numpy as np
    w = np.zeros(N_TARGETS, dtype=np.float32)
    w[(np.arange(n_active) * N_TARGETS) // n_active] = (0.3 + 0.05 * np.arange(n_active)) * (1.0 if k & 1 else -0.5)
    return w


def apply(sc, desc):
    sc.force_next_op(3)
    return timed(lambda: sc.set_instances(desc.instances))


def route_morph():
    sc, desc, m, d = make()
    sc.set_mesh_morph(m.key, d)
    out = {"vertices": len(m.vertices), "targets": N_TARGETS, "calls": REPS}
    for n_active in ACTIVE:
        rows = []
        for k in range(WARMUP + REPS):
            t_call = timed(lambda: sc.pose_mesh(m.key, weights(n_active, k)))
            t_set = apply(sc, desc)
            info = sc.mesh_morph_info(m.key)
            assert info.n_active == n_active
            rows.append((t_call, info.morph_ms, sc.mesh_vertex_info(m.key).copy_ms, t_set))
        rows = rows[WARMUP:]
        out["active_%d" % n_active] = {n: stats([r[j] for r in rows]) for j, n in enumerate(("pose_mesh_call_ms", "morph_ms", "copy_ms", "set_instances_ms"))}
    return out


def torch_blend(base, D, w):
    """The blend of [n, 24] float records with the deltas D [16, n, 12] by torch ops: positions, normalised normals and tangents."""
    import torch
    s = torch.zeros_like(D[0])
    for k in range(len(w)):
        if w[k] != 0:
            s = torch.add(s, D[k], alpha=float(w[k]))
    out = base.clone()
    out[:, 0:3] = base[:, 0:3] + s[:, 0:3]
    out[:, 4:7] = torch.nn.functional.normalize(base[:, 4:7] + s[:, 4:7], dim=1)
    out[:, 8:11] = torch.nn.functional.normalize(base[:, 8:11] + s[:, 8:11], dim=1)
    return out


def route_torch_device():
    import torch
    sc, desc, m, d = make()
    base = torch.from_numpy(m.vertices.view("<f4").reshape(len(m.vertices), -1).copy()).to("cuda:0")
    D = torch.from_numpy(d.view("<f4").reshape(N_TARGETS, len(m.vertices), 12).copy()).to("cuda:0")
    out = {"vertices": len(m.vertices), "targets": N_TARGETS, "calls": REPS}
    for n_active in ACTIVE:
        rows = []
        for k in range(WARMUP + REPS):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            w = weights(n_active, k)
            t0 = time.perf_counter()
            ev[0].record()
            posed = torch_blend(base, D, w)
            ev[1].record()
            torch.cuda.synchronize()
            t_pose = (time.perf_counter() - t0) * 1e3
            t_call = timed(lambda: sc.update_mesh_device(m.key, posed))
            t_set = apply(sc, desc)
            i = sc.mesh_vertex_info(m.key)
            rows.append((t_call, t_pose, ev[0].elapsed_time(ev[1]), i.check_ms, i.copy_ms, t_set))
        rows = rows[WARMUP:]
        names = ("update_mesh_device_call_ms", "torch_blend_wall_ms", "torch_blend_events_ms", "check_ms", "copy_ms", "set_instances_ms")
        out["active_%d" % n_active] = {n: stats([r[j] for r in rows]) for j, n in enumerate(names)}
    return out


def route_numpy_host():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import morph_reference as ref
    sc, desc, m, d = make()
    out = {"vertices": len(m.vertices), "targets": N_TARGETS, "calls": HOST_REPS}
    for n_active in ACTIVE:
        rows = []
        for k in range(1 + HOST_REPS):
            posed = []
            t_pose = timed(lambda: posed.append(ref.morph_model(m.vertices, d, weights(n_active, k))[0]))
            t_call = timed(lambda: sc.update_mesh(m.key, posed[0]))
            t_set = apply(sc, desc)
            rows.append((t_call, t_pose, t_set))
        rows = rows[1:]
        out["active_%d" % n_active] = {n: stats([r[j] for r in rows]) for j, n in enumerate(("update_mesh_call_ms", "numpy_blend_ms", "set_instances_ms"))}
    return out


def route_morph_skin():
    import gpu_mesh_skin as skin
    sc, desc, m, inf, mats = skin.make()
    d, n = deltas_for(m), len(m.vertices)
    sc.set_mesh_skin(m.key, inf, skin.N_JOINTS)
    sc.set_mesh_morph(m.key, d)
    out = {"vertices": n, "targets": N_TARGETS, "joints": skin.N_JOINTS, "calls": REPS}
    rows = []
    for k in range(WARMUP + REPS):
        t_call = timed(lambda: sc.skin_mesh(m.key, mats[k & 1]))
        apply(sc, desc)
        rows.append((t_call, sc.mesh_skin_info(m.key).skin_ms))
    rows = rows[WARMUP:]
    out["skin_alone"] = {"skin_mesh_call_ms": stats([r[0] for r in rows]), "skin_ms": stats([r[1] for r in rows])}
    for n_active in ACTIVE:
        rows = []
        for k in range(WARMUP + REPS):
            t_call = timed(lambda: sc.pose_mesh(m.key, weights(n_active, k), mats[k & 1]))
            apply(sc, desc)
            rows.append((t_call, sc.mesh_morph_info(m.key).morph_ms))
        rows = rows[WARMUP:]
        out["active_%d" % n_active] = {"pose_mesh_call_ms": stats([r[0] for r in rows]), "morph_and_skin_ms": stats([r[1] for r in rows])}
    return out


def summary(res):
    out = {}
    for n_active in ACTIVE:
        key = "active_%d" % n_active
        row = {}
        if "morph" in res:
            row["morph"] = res["morph"][key]["pose_mesh_call_ms"]["median"]
            row["morph_kernel"] = res["morph"][key]["morph_ms"]["median"]
        if "torch_device" in res:
            b = res["torch_device"][key]
            row["torch_device"] = b["torch_blend_wall_ms"]["median"] + b["update_mesh_device_call_ms"]["median"]
        if "numpy_host" in res:
            c = res["numpy_host"][key]
            row["numpy_host"] = c["numpy_blend_ms"]["median"] + c["update_mesh_call_ms"]["median"]
        if "morph_skin" in res:
            e = res["morph_skin"]
            row["morph_and_skin_kernels"] = e[key]["morph_and_skin_ms"]["median"]
            row["skin_kernel_alone"] = e["skin_alone"]["skin_ms"]["median"]
            row["second_pass_ms"] = e[key]["morph_and_skin_ms"]["median"] - e["skin_alone"]["skin_ms"]["median"]
        out[key] = row
    return {"whole_step_ms": out}


def main():
    args = sys.argv[1:]
    if args[:1] == ["--child"]:
        routes = {"morph": route_morph, "torch_device": route_torch_device, "numpy_host": route_numpy_host, "morph_skin": route_morph_skin}
        print("RESULT " + json.dumps(routes[args[1]]()))
        return
    out_path = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles", "mesh_morph.json")
    only = args[args.index("--only") + 1] if "--only" in args else None
    res = {}
    for route in ROUTES:
        if only and route != only:
            continue
        p = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--child", route], capture_output=True, text=True)
        line = next((ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")), None)
        if p.returncode != 0 or line is None:
            print("%s failed (exit %d):\n%s" % (route, p.returncode, (p.stdout + p.stderr)[-3000:]))
            sys.exit(1)             # nothing more is started on the GPU after a failure
        res[route] = json.loads(line[len("RESULT "):])
        print(route, json.dumps(res[route]))
    res["summary"] = summary(res)
    print("summary", json.dumps(res["summary"]))
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(out_path)


if __name__ == "__main__":
    main()
