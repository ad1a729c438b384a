"""Cost of posing a mesh with the library's skinning kernel (Scene.skin_mesh) against the routes there were before it, on the
1M-triangle heightfield (one mesh, 501 264 vertices) with a synthetic rig of 64 joints (four influences per vertex), one pose per
step alternating between two sets of joint matrices:

  skin           (a) Scene.skin_mesh: the whole call (wall clock) and SrMeshSkinInfo.skin_ms (kernel + 4-byte read-back, events),
                     with copy_ms of the same call, (d): the device-to-device copy of the posed vertices into the mesh's buffer
  torch_device   (b) the fastest route before: the same pose computed by torch ops on the GPU (linear blend of positions, cofactor
                     normals, tangents; timed with events), then Scene.update_mesh_device (wall clock; check_ms and copy_ms)
  numpy_host     (c) the pose computed by numpy on the host, then Scene.update_mesh through the host pointer (5 calls: it is slow)

Every step is followed by the set_instances that applies it (SR_OP_UPDATE, forced; reported, not part of the comparison: it is
the same work on every route). Median (min-max) of 20 calls after 3 warm-ups, every route in a fresh child process under its own
time limit; stops at the first route that fails. The verdict compares (a)'s whole call with (b)'s update_mesh_device call plus
1.25 x (d): the kernel moves 1.125 x the bytes of a copy and replaces the separate check kernel; a quarter is allowed for the
launch and the matrix gather.

  python scripts/gpu_mesh_skin.py [--out profiles/mesh_skin.json] [--only ROUTE]
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS, WARMUP, HOST_REPS, N_JOINTS = 20, 3, 5, 64
ROUTES = ("skin", "torch_device", "numpy_host")


def stats(xs):
    import numpy as np
    return {"median": float(np.median(xs)), "min": float(np.min(xs)), "max": float(np.max(xs))}


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def make():
    """-> (scene, desc, the heightfield mesh, influences, [joint matrices A, B])."""
    import numpy as np
    from sunray_amd import abi, runtime as rt, scenes
    desc = scenes.heightfield()
    m = next(x for x in desc.meshes if x.key == 1)
    n = len(m.vertices)
    # joints on an 8 x 8 grid over the field; a vertex leans on the four joints around it with bilinear weights
    x, z = m.vertices["position"][:, 0], m.vertices["position"][:, 2]
    u = (x - x.min()) / (x.max() - x.min()) * 6.999
    v = (z - z.min()) / (z.max() - z.min()) * 6.999
    iu, iv = u.astype(np.int64), v.astype(np.int64)
    fu, fv = (u - iu).astype(np.float32), (v - iv).astype(np.float32)
    inf = np.zeros(n, dtype=abi.SKIN_INFLUENCE)
    inf["joint"] = np.stack([iv * 8 + iu, iv * 8 + iu + 1, (iv + 1) * 8 + iu, (iv + 1) * 8 + iu + 1], axis=1)
    inf["weight"] = np.stack([(1 - fu) * (1 - fv), fu * (1 - fv), (1 - fu) * fv, fu * fv], axis=1)
    mats = []
    for phase in (0.4, 0.9):
        M = np.zeros((N_JOINTS, 3, 4), dtype=np.float32)
        for j in range(N_JOINTS):
            a = 0.15 * np.sin(phase + 0.37 * j)
            M[j] = [[np.cos(a), -np.sin(a), 0, 0], [np.sin(a), np.cos(a), 0, 0.3 * np.sin(phase * 2 + j)], [0, 0, 1, 0]]
        mats.append(M)
    sc = rt.Scene(0, instancing="flat").load(desc)
    sc.enable_timing(True)
    return sc, desc, m, inf, mats


def apply(sc, desc):
    sc.force_next_op(3)
    return timed(lambda: sc.set_instances(desc.instances))


def route_skin():
    sc, desc, m, inf, mats = make()
    sc.set_mesh_skin(m.key, inf, N_JOINTS)
    rows = []
    for k in range(WARMUP + REPS):
        t_call = timed(lambda: sc.skin_mesh(m.key, mats[k & 1]))
        t_set = apply(sc, desc)
        rows.append((t_call, sc.mesh_skin_info(m.key).skin_ms, sc.mesh_vertex_info(m.key).copy_ms, t_set))
    rows = rows[WARMUP:]
    out = {n: stats([r[j] for r in rows]) for j, n in enumerate(("skin_mesh_call_ms", "skin_ms", "copy_ms", "set_instances_ms"))}
    out["vertices"], out["joints"], out["calls"] = len(m.vertices), N_JOINTS, REPS
    return out


def torch_pose(rest, joints, weights, M):
    """Linear-blend skinning of [n, 24] float records by torch ops: positions, cofactor normals, tangents."""
    import torch
    B = (weights[:, :, None, None] * M[joints]).sum(dim=1)                       # [n, 3, 4]
    A = B[:, :, :3]
    out = rest.clone()
    out[:, 0:3] = torch.einsum("nrc,nc->nr", A, rest[:, 0:3]) + B[:, :, 3]
    cof = torch.stack([torch.linalg.cross(A[:, 1], A[:, 2]), torch.linalg.cross(A[:, 2], A[:, 0]), torch.linalg.cross(A[:, 0], A[:, 1])], dim=1)
    out[:, 4:7] = torch.nn.functional.normalize(torch.einsum("nrc,nc->nr", cof, rest[:, 4:7]), dim=1)
    out[:, 8:11] = torch.nn.functional.normalize(torch.einsum("nrc,nc->nr", A, rest[:, 8:11]), dim=1)
    return out


def route_torch_device():
    import numpy as np
    import torch
    sc, desc, m, inf, mats = make()
    rest = torch.from_numpy(m.vertices.view("<f4").reshape(len(m.vertices), -1).copy()).to("cuda:0")
    joints = torch.from_numpy(inf["joint"].astype(np.int64)).to("cuda:0")
    weights = torch.from_numpy(inf["weight"].copy()).to("cuda:0")
    rows = []
    for k in range(WARMUP + REPS):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        t0 = time.perf_counter()
        ev[0].record()
        posed = torch_pose(rest, joints, weights, torch.from_numpy(mats[k & 1]).to("cuda:0"))
        ev[1].record()
        torch.cuda.synchronize()
        t_pose = (time.perf_counter() - t0) * 1e3
        t_call = timed(lambda: sc.update_mesh_device(m.key, posed))
        t_set = apply(sc, desc)
        i = sc.mesh_vertex_info(m.key)
        rows.append((t_call, t_pose, ev[0].elapsed_time(ev[1]), i.check_ms, i.copy_ms, t_set))
    rows = rows[WARMUP:]
    names = ("update_mesh_device_call_ms", "torch_pose_wall_ms", "torch_pose_events_ms", "check_ms", "copy_ms", "set_instances_ms")
    out = {n: stats([r[j] for r in rows]) for j, n in enumerate(names)}
    out["vertices"], out["calls"] = len(m.vertices), REPS
    return out


def route_numpy_host():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import skin_reference as ref
    sc, desc, m, inf, mats = make()
    rows = []
    for k in range(1 + HOST_REPS):
        posed = []
        t_pose = timed(lambda: posed.append(ref.skin_model(m.vertices, inf, mats[k & 1])[0]))
        t_call = timed(lambda: sc.update_mesh(m.key, posed[0]))
        t_set = apply(sc, desc)
        rows.append((t_call, t_pose, t_set))
    rows = rows[1:]
    out = {n: stats([r[j] for r in rows]) for j, n in enumerate(("update_mesh_call_ms", "numpy_pose_ms", "set_instances_ms"))}
    out["vertices"], out["calls"] = len(m.vertices), HOST_REPS
    return out


def verdict(res):
    a, b = res["skin"], res["torch_device"]
    allowed = b["update_mesh_device_call_ms"]["median"] + 1.25 * a["copy_ms"]["median"]
    return {"skin_mesh_call_ms": a["skin_mesh_call_ms"]["median"], "allowed_ms": allowed,
            "rule": "skin_mesh call <= update_mesh_device call + 1.25 x copy_ms", "met": bool(a["skin_mesh_call_ms"]["median"] <= allowed),
            "whole_step_ms": {"skin": a["skin_mesh_call_ms"]["median"],
                              "torch_device": b["torch_pose_wall_ms"]["median"] + b["update_mesh_device_call_ms"]["median"],
                              "numpy_host": (res["numpy_host"]["numpy_pose_ms"]["median"] + res["numpy_host"]["update_mesh_call_ms"]["median"]) if "numpy_host" in res else None}}


def main():
    args = sys.argv[1:]
    if args[:1] == ["--child"]:
        print("RESULT " + json.dumps({"skin": route_skin, "torch_device": route_torch_device, "numpy_host": route_numpy_host}[args[1]]()))
        return
    out_path = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles", "mesh_skin.json")
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
    if "skin" in res and "torch_device" in res:
        res["verdict"] = verdict(res)
        print("verdict", json.dumps(res["verdict"]))
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(out_path)


if __name__ == "__main__":
    main()
