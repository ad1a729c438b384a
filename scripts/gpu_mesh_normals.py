"""Cost of one step of a deforming mesh whose producer knows only the new positions, on the 1M-triangle heightfield (one mesh,
501 264 vertices, valence 6) and on the Cornell box's sphere (482 vertices, 32 entries at the poles), the positions alternating
between two waves:

  frame          (a) Scene.update_mesh_positions with a device tensor (sr_scene_update_mesh_positions_device): the whole call (wall
                     clock) and SrMeshFrameInfo.frame_ms (both kernels + read-back, events), with copy_ms of the same call, under
                     SR_FRAME_NORMALS alone and with SR_FRAME_TANGENTS
  torch_device   (b) what a caller writes today: cross, index_add_ (float atomics), normalise, the 96-byte records assembled by torch
                     ops on the GPU (wall clock and events), then Scene.update_mesh_device (wall clock; check_ms and copy_ms)
  numpy_host     (c) scenes.deform_vertices' arithmetic (float64 cross, np.add.at, normalise) on the host, then Scene.update_mesh
                     through the host pointer (3 calls: it is slow)

(b) and (c) exist without this feature: they are the yardstick, (a) is not compared with itself. Every step is followed by the
set_instances that applies it (SR_OP_UPDATE, forced; reported, not part of the comparison: it is the same work on every route).
Median (min-max) of 20 calls after 3 warm-ups, every route in a fresh child process under its own time limit; stops at the first
route that fails. No figure is fixed in advance: the result is what profiles/mesh_normals.json says, next to the compiler's
resource report of normals.hip.

  python scripts/gpu_mesh_normals.py [--out profiles/mesh_normals.json] [--only ROUTE]
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS, WARMUP, HOST_REPS = 20, 3, 3
ROUTES = ("frame", "torch_device", "numpy_host")
MESHES = ("heightfield", "sphere")


def stats(xs):
    import numpy as np
    return {"median": float(np.median(xs)), "min": float(np.min(xs)), "max": float(np.max(xs))}


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def make(which):
    """-> (scene, desc, the deforming mesh)."""
    from sunray_amd import runtime as rt, scenes
    desc, key = (scenes.heightfield(), 1) if which == "heightfield" else (scenes.cornell_box(), 7)
    m = next(x for x in desc.meshes if x.key == key)
    sc = rt.Scene(0, instancing="flat").load(desc)
    sc.enable_timing(True)
    return sc, desc, m


def wave(m, k):
    """Positions of step k, float32 [n, 3]: the rest positions moved along the rest normals; two waves in turn."""
    import numpy as np
    p, n = m.vertices["position"], m.vertices["normal"]
    s = np.float32(0.05) * np.sin(np.float32(1.7) * p[:, 0:1] + np.float32(1.1) * p[:, 2:3] + np.float32(0.6 * (k & 1)))
    return np.ascontiguousarray((p + n * s).astype(np.float32))


def apply(sc, desc):
    sc.force_next_op(3)
    return timed(lambda: sc.set_instances(desc.instances))


def route_frame(which):
    import torch
    sc, desc, m = make(which)
    pos = [torch.from_numpy(wave(m, k)).to("cuda:0") for k in (0, 1)]
    out = {"vertices": len(m.vertices), "triangles": len(m.indices) // 3, "calls": REPS}
    for name, tangents in (("normals", False), ("normals_tangents", True)):
        sc.set_mesh_frame(m.key, normals=False)
        sc.update_mesh(m.key, m.vertices)
        sc.set_mesh_frame(m.key, tangents=tangents)
        info = sc.mesh_frame_info(m.key)
        out["groups"], out["entries"], out["max_valence"] = info.n_groups, info.n_entries, info.max_valence
        rows = []
        for k in range(WARMUP + REPS):
            t_call = timed(lambda: sc.update_mesh_positions(m.key, pos[k & 1]))
            t_set = apply(sc, desc)
            rows.append((t_call, sc.mesh_frame_info(m.key).frame_ms, sc.mesh_vertex_info(m.key).copy_ms, t_set))
        rows = rows[WARMUP:]
        out[name] = {n: stats([r[j] for r in rows]) for j, n in enumerate(("update_mesh_positions_call_ms", "frame_ms", "copy_ms", "set_instances_ms"))}
    return out


def torch_records(rest, idx, pos, rest_normal):
    """The caller's route: face vectors, a scatter-add per corner (float atomics: the sums differ from run to run), the side the
    rest normals face, normalise, and the [n, 24] float records around the new positions."""
    import torch
    p0 = pos[idx[:, 0]]
    face = torch.cross(pos[idx[:, 1]] - p0, pos[idx[:, 2]] - p0, dim=1)
    acc = torch.zeros_like(pos)
    for j in range(3):
        acc.index_add_(0, idx[:, j], face)
    acc = torch.where((acc * rest_normal).sum(dim=1, keepdim=True) < 0, -acc, acc)
    out = rest.clone()
    out[:, 0:3] = pos
    out[:, 4:7] = torch.nn.functional.normalize(acc, dim=1)
    return out


def route_torch_device(which):
    import torch
    sc, desc, m = make(which)
    rest = torch.from_numpy(m.vertices.view("<f4").reshape(len(m.vertices), -1).copy()).to("cuda:0")
    idx = torch.from_numpy(m.indices.astype("int64").reshape(-1, 3)).to("cuda:0")
    rest_normal = rest[:, 4:7].contiguous()
    pos = [torch.from_numpy(wave(m, k)).to("cuda:0") for k in (0, 1)]
    rows = []
    for k in range(WARMUP + REPS):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        t0 = time.perf_counter()
        ev[0].record()
        records = torch_records(rest, idx, pos[k & 1], rest_normal)
        ev[1].record()
        torch.cuda.synchronize()
        t_make = (time.perf_counter() - t0) * 1e3
        t_call = timed(lambda: sc.update_mesh_device(m.key, records))
        t_set = apply(sc, desc)
        i = sc.mesh_vertex_info(m.key)
        rows.append((t_call, t_make, ev[0].elapsed_time(ev[1]), i.check_ms, i.copy_ms, t_set))
    rows = rows[WARMUP:]
    names = ("update_mesh_device_call_ms", "torch_records_wall_ms", "torch_records_events_ms", "check_ms", "copy_ms", "set_instances_ms")
    out = {"vertices": len(m.vertices), "calls": REPS}
    out["normals"] = {n: stats([r[j] for r in rows]) for j, n in enumerate(names)}
    return out


def numpy_records(m, pos):
    import numpy as np
    v = m.vertices.copy()
    idx = np.asarray(m.indices, dtype=np.int64).reshape(-1, 3)
    q, n = pos.astype(np.float64), v["normal"].astype(np.float64)
    face = np.cross(q[idx[:, 1]] - q[idx[:, 0]], q[idx[:, 2]] - q[idx[:, 0]])
    acc = np.zeros_like(q)
    for j in range(3):
        np.add.at(acc, idx[:, j], face)
    ln = np.linalg.norm(acc, axis=1)
    ok = ln > 1e-20
    flip = np.where(np.einsum("ij,ij->i", acc, n) < 0.0, -1.0, 1.0)
    v["position"] = pos
    v["normal"] = np.where(ok[:, None], acc / np.where(ok, ln, 1.0)[:, None] * flip[:, None], n).astype(np.float32)
    return v


def route_numpy_host(which):
    sc, desc, m = make(which)
    rows = []
    for k in range(1 + HOST_REPS):
        made = []
        t_make = timed(lambda: made.append(numpy_records(m, wave(m, k))))
        t_call = timed(lambda: sc.update_mesh(m.key, made[0]))
        t_set = apply(sc, desc)
        rows.append((t_call, t_make, t_set))
    rows = rows[1:]
    out = {"vertices": len(m.vertices), "calls": HOST_REPS}
    out["normals"] = {n: stats([r[j] for r in rows]) for j, n in enumerate(("update_mesh_call_ms", "numpy_records_ms", "set_instances_ms"))}
    return out


def spread(s):
    return s["max"] - s["min"]


def summary(res):
    """Whole-step medians of the three routes per mesh, and whether (a) is below (b) by more than the two spreads together."""
    out = {}
    for which in MESHES:
        row = {}
        a = res.get("frame", {}).get(which)
        b = res.get("torch_device", {}).get(which)
        c = res.get("numpy_host", {}).get(which)
        if a:
            row["frame"] = a["normals"]["update_mesh_positions_call_ms"]["median"]
            row["frame_spread"] = spread(a["normals"]["update_mesh_positions_call_ms"])
            row["frame_kernels"] = a["normals"]["frame_ms"]["median"]
            row["frame_with_tangents"] = a["normals_tangents"]["update_mesh_positions_call_ms"]["median"]
            row["frame_kernels_with_tangents"] = a["normals_tangents"]["frame_ms"]["median"]
        if b:
            n = b["normals"]
            row["torch_device"] = n["torch_records_wall_ms"]["median"] + n["update_mesh_device_call_ms"]["median"]
            row["torch_device_spread"] = spread(n["torch_records_wall_ms"]) + spread(n["update_mesh_device_call_ms"])
        if c:
            row["numpy_host"] = c["normals"]["numpy_records_ms"]["median"] + c["normals"]["update_mesh_call_ms"]["median"]
        if a and b:
            row["frame_below_torch_by_more_than_both_spreads"] = bool(row["torch_device"] - row["frame"] > row["frame_spread"] + row["torch_device_spread"])
        out[which] = row
    return {"whole_step_ms": out}


def main():
    args = sys.argv[1:]
    if args[:1] == ["--child"]:
        routes = {"frame": route_frame, "torch_device": route_torch_device, "numpy_host": route_numpy_host}
        print("RESULT " + json.dumps(routes[args[1]](args[2])))
        return
    out_path = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles", "mesh_normals.json")
    only = args[args.index("--only") + 1] if "--only" in args else None
    res = {}
    for route in ROUTES:
        if only and route != only:
            continue
        for which in MESHES:
            p = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--child", route, which], capture_output=True, text=True)
            line = next((ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")), None)
            if p.returncode != 0 or line is None:
                print("%s / %s failed (exit %d):\n%s" % (route, which, p.returncode, (p.stdout + p.stderr)[-3000:]))
                sys.exit(1)             # nothing more is started on the GPU after a failure
            res.setdefault(route, {})[which] = json.loads(line[len("RESULT "):])
            print(route, which, json.dumps(res[route][which]))
    res["summary"] = summary(res)
    from sunray_amd import build
    res["kernel_resources"] = build.kernel_resources("normals.hip") if os.path.exists(build.resources_path("normals.hip")) else "no report next to this build"
    print("summary", json.dumps(res["summary"]))
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(out_path)


if __name__ == "__main__":
    main()
