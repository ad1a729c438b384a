"""Cost of one posing step of a crowd of small rigged meshes: the per-mesh loop (one sr_scene_pose_mesh per mesh: each a batch
of one item, with its own upload, memset, posing launch, read-back, scatter launch and three waits) against sr_scene_pose_meshes
(one of each for the whole crowd) in the same build.

Cases: 1, 10, 100 and 1 000 copies of a rigged sphere of 256 triangles (16 x 9, 130 vertices) and of 1 024 triangles (32 x 17, 514
vertices), the sizes of the batched tree build's table, skinned with four joints; and 100 copies of the 1 024-triangle sphere with
three morph targets and the skin (the fused path). Both paths are timed at the C entry points with their arguments packed
beforehand, so that neither pays for Python's packing. Wall clock of the step with the event timing off; then, with it on, the
device time: pose_ms + scatter_ms of the batch, the sum of the per-mesh skin_ms / morph_ms and copy_ms of the loop. Median
(min - max) of REPS steps after WARMUP, the two paths alternating.

  python scripts/gpu_pose_batch.py [--out profiles/pose_batch.json] [--only CASE]... [--label NAME] [--add-resources]

--label NAME keeps the run under "runs"[NAME] of the output file next to the runs already there: two builds of the library
(SUNRAY_HIP_LIB selects one) measured in one session, as profiles/pose_one_path.json holds the commit that made the single calls
batches of one and its parent.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPS, WARMUP = 20, 3
# name -> (sphere segments, rings, copies, morph targets)
CASES = {}
for copies in (1, 10, 100, 1000):
    CASES["%dx256" % copies] = (16, 9, copies, 0)
    CASES["%dx1k" % copies] = (32, 17, copies, 0)
CASES["100x1k fused"] = (32, 17, 100, 3)
N_JOINTS = 4


def stats(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1], "n": len(xs)}


def make(case):
    from sunray_amd import abi, runtime as rt, scenes
    nu, nv, copies, n_targets = CASES[case]
    v, idx = scenes.uv_sphere(1.0, nu, nv)
    grey = abi.material(base_color=(0.8, 0.8, 0.8, 1.0), roughness=0.5)
    desc = scenes.SceneDesc(case)
    side = int(np.ceil(np.sqrt(copies)))
    for k in range(copies):
        desc.meshes.append(scenes.MeshDesc(k + 1, v, idx, grey))
        desc.instances.append((k + 1, [scenes.translate(3.0 * (k % side), 0.0, 3.0 * (k // side))]))
    sc = rt.Scene(0, instancing="two_level").load(desc)
    n = len(v)
    inf = np.zeros(n, dtype=abi.SKIN_INFLUENCE)
    inf["joint"] = np.stack([np.arange(n) % N_JOINTS, (np.arange(n) + 1) % N_JOINTS, np.zeros(n), np.zeros(n)], axis=1)
    inf["weight"][:, 0], inf["weight"][:, 1] = 0.75, 0.25
    deltas = None
    if n_targets:
        deltas = np.zeros((n_targets, n), dtype=abi.MORPH_DELTA)
        for t in range(n_targets):
            deltas["position"][t] = 0.05 * (t + 1) * v["normal"][:, :3]
    for k in range(copies):
        sc.set_mesh_build_type(k + 1, abi.BUILD_RAPIDLY_CHANGING)
        sc.set_mesh_skin(k + 1, inf, N_JOINTS)
        if deltas is not None:
            sc.set_mesh_morph(k + 1, deltas)
    sc.set_instances(desc.instances)
    return sc, desc, len(v), len(idx) // 3


def pose_arrays(copies, n_targets, step):
    """Per copy its own joint matrices (a rotation about y by an angle of its own, rising with the step) and weights."""
    M = np.zeros((copies, N_JOINTS, 3, 4), dtype=np.float32)
    for j in range(N_JOINTS):
        a = 0.01 * step + 0.001 * np.arange(copies) + 0.1 * j
        M[:, j, 0, 0], M[:, j, 0, 2], M[:, j, 1, 1], M[:, j, 2, 0], M[:, j, 2, 2] = np.cos(a), np.sin(a), 1.0, -np.sin(a), np.cos(a)
    w = np.full((copies, max(n_targets, 1)), 0.25 + 0.01 * step, dtype=np.float32)
    return M, w


def measure(case):
    from sunray_amd import abi
    from sunray_amd._lib import check, lib
    sc, desc, n_vertices, n_triangles = make(case)
    copies, n_targets = CASES[case][2], CASES[case][3]
    L = lib()

    def packed(step):
        M, w = pose_arrays(copies, n_targets, step)
        rows = (abi.SrPoseItem * copies)()
        for k in range(copies):
            rows[k].key = k + 1
            rows[k].weights = w[k].ctypes.data if n_targets else None
            rows[k].joint_matrices = M[k].ctypes.data
            rows[k].n_targets, rows[k].n_joints = n_targets, N_JOINTS
        return rows, (M, w)

    def loop(rows):
        t0 = time.perf_counter()
        for k in range(copies):
            it = rows[k]
            rc = L.sr_scene_pose_mesh(sc._h, C.c_uint64(it.key), C.c_void_p(it.weights), C.c_uint32(it.n_targets), C.c_void_p(it.joint_matrices), C.c_uint32(it.n_joints), None)
            if rc != 0:
                check(rc)
        return (time.perf_counter() - t0) * 1e3

    def batch(rows):
        t0 = time.perf_counter()
        rc = L.sr_scene_pose_meshes(sc._h, rows, C.c_uint32(copies), None)
        dt = (time.perf_counter() - t0) * 1e3
        check(rc)
        return dt

    def device_ms_of_loop():
        total = 0.0
        for k in range(copies):
            total += (sc.mesh_morph_info(k + 1).morph_ms if n_targets else sc.mesh_skin_info(k + 1).skin_ms) + sc.mesh_vertex_info(k + 1).copy_ms
        return total

    out = {"copies": copies, "vertices_per_mesh": n_vertices, "triangles_per_mesh": n_triangles, "morph_targets": n_targets, "joints": N_JOINTS}
    wall = {"loop": [], "batch": []}
    for step in range(WARMUP + REPS):
        rows, keep = packed(step)
        a, b = loop(rows), batch(rows)
        if step >= WARMUP:
            wall["loop"].append(a); wall["batch"].append(b)
    sc.enable_timing(True)
    dev = {"loop": [], "batch_pose": [], "batch_scatter": []}
    for step in range(WARMUP + REPS):
        rows, keep = packed(100 + step)
        loop(rows)
        d = device_ms_of_loop()
        batch(rows)
        info = sc.pose_batch_info()
        if step >= WARMUP:
            dev["loop"].append(d); dev["batch_pose"].append(info.pose_ms); dev["batch_scatter"].append(info.scatter_ms)
    sc.enable_timing(False)
    info = sc.pose_batch_info()
    out["batch_info"] = {"items": info.items, "vertices": info.vertices, "blocks": info.blocks, "upload_bytes": info.upload_bytes,
                         "launches": info.launches, "read_backs": info.read_backs, "fused": info.fused, "skin_only": info.skin_only}
    out["wall_ms"] = {k: stats(v) for k, v in wall.items()}
    out["device_ms"] = {k: stats(v) for k, v in dev.items()}
    lo, ba = out["wall_ms"]["loop"], out["wall_ms"]["batch"]
    out["verdict"] = "batch wins" if ba["max"] < lo["min"] else "loop wins" if lo["max"] < ba["min"] else "ranges overlap"
    out["speedup_of_medians"] = lo["median"] / ba["median"]
    sc.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_batch.json"))
    ap.add_argument("--only", action="append", help="a case to run (may be given several times); default: all")
    ap.add_argument("--label", help="keep this run under runs[LABEL] of the output file, next to the runs already there")
    ap.add_argument("--add-resources", action="store_true", help="add the compiler's resource report of pose_batch.hip to an existing file; no GPU")
    args = ap.parse_args()
    if args.add_resources:                               # on the machine that built the library: the compiler's report into the file
        from sunray_amd import build
        result = json.load(open(args.out))
        result["kernel_resources"] = {name.split("srd")[1][2:].split("EPK")[0]: r for name, r in build.kernel_resources("pose_batch.hip").items()}
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        return
    result = {"what": "one posing step: per-mesh sr_scene_pose_mesh loop against sr_scene_pose_meshes, wall clock and device (event) milliseconds",
              "reps": REPS, "warmup": WARMUP, "cases": {}}
    if args.label:
        whole = json.load(open(args.out)) if os.path.exists(args.out) else {"what": result["what"], "reps": REPS, "warmup": WARMUP, "runs": {}}
        result = whole["runs"][args.label] = {"library": os.path.basename(os.environ.get("SUNRAY_HIP_LIB", "the product library")), "cases": {}}
    for case in CASES:
        if args.only and case not in args.only:
            continue
        result["cases"][case] = measure(case)
        c = result["cases"][case]
        print("%-14s loop %8.3f (%.3f - %.3f) ms   batch %8.3f (%.3f - %.3f) ms   %s" % (
            case, c["wall_ms"]["loop"]["median"], c["wall_ms"]["loop"]["min"], c["wall_ms"]["loop"]["max"],
            c["wall_ms"]["batch"]["median"], c["wall_ms"]["batch"]["min"], c["wall_ms"]["batch"]["max"], c["verdict"]), flush=True)
        with open(args.out, "w") as f:
            json.dump(whole if args.label else result, f, indent=1)
            f.write("\n")
    print(args.out)


if __name__ == "__main__":
    main()
