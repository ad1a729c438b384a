"""Cost of one crowd step, evaluation plus posing, up to the posed vertices and the instance tables, by three paths of one build:

  A  sr_gltf_pose per actor (instance transforms, then the skin's joint matrices) + sr_scene_pose_meshes + sr_scene_set_instances
  B  sr_clip_pose_host per actor (the baked clip on the host) + the same two device calls: what the bake alone buys
  C  sr_scene_pose_actors (clip_pose_kernel in front of the posing kernel) + sr_scene_set_instances_device

Cases: 1, 10, 100 and 1 000 actors of a rig of 4 and of 64 joints (a chain of that many nodes, each turned by a LINEAR rotation
channel of 4 keys; one skinned and one unskinned quad of 4 vertices per actor, so that evaluation and not vertex work is what is
measured). Every path is timed at the C entry points with its arguments packed beforehand. Wall clock of the step with the event
timing off; then, with it on, the device time (A, B: pose_ms + scatter_ms + the instance tables' tables_ms; C: clip_ms + pose_ms +
scatter_ms + tables_ms). "eval" is the host evaluation part of A and B alone. Median (min - max) of REPS steps after WARMUP, the
paths alternating.

  python scripts/gpu_clip_pose.py [--out profiles/clip_pose.json] [--only CASE]...
"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REPS, WARMUP = 20, 3
CASES = {"%dx%dj" % (actors, joints): (actors, joints) for joints in (4, 64) for actors in (1, 10, 100, 1000)}


def stats(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1], "n": len(xs)}


def measure(case, tmp):
    import torch
    from clip_util import crowd, shape_rig
    from sunray_amd import abi, runtime as rt
    from sunray_amd._lib import check, lib
    actors, joints = CASES[case]
    path = os.path.join(tmp, case + ".glb")
    n_nodes = shape_rig(path, chain=joints, joints=joints, channels=joints, keys=4)
    desc, g, keys, rigs, layout, rows, skins, ib = crowd(rt, path, actors)
    sc = rt.Scene(0, instancing="two_level").load(desc)
    for key, (inf, nj) in rigs.items():
        sc.set_mesh_build_type(key, abi.BUILD_RAPIDLY_CHANGING)
        sc.set_mesh_skin(key, inf, nj)
    sc.set_instances(desc.instances)
    clip = g.bake_clip(0)
    cid = sc.attach_clip(clip)
    L, ni = lib(), len(rows)
    assert list(rows) == list(range(ni))                    # one instance a blas, in blas order: a copy's rows are its own, in order
    duration = clip.info.duration_seconds
    jm, xf = np.zeros((actors, joints, 12), np.float32), np.zeros((actors * ni, 12), np.float32)
    jm_at = [C.c_void_p(jm[a].ctypes.data) for a in range(actors)]
    xf_at = [C.c_void_p(xf[a * ni:].ctypes.data) for a in range(actors)]
    skinned_key = [keys[a][skins.index(0)] for a in range(actors)]
    pose_rows = (abi.SrPoseItem * actors)()
    for a in range(actors):
        pose_rows[a].key, pose_rows[a].joint_matrices, pose_rows[a].n_joints = skinned_key[a], jm_at[a].value, joints
    lkeys, lcounts = np.array([k for k, _ in layout], np.uint64), np.array([c for _, c in layout], np.uint32)
    args = rt.ActorArgs([(cid, 0.0, None, None, a * ni) for a in range(actors)], [(skinned_key[a], a, 0, None) for a in range(actors)])
    d_xf = torch.zeros((actors * ni, 12), dtype=torch.float32, device="cuda:0")
    d_ptr = C.c_void_p(d_xf.data_ptr())
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731

    def times_of(step):
        return [C.c_float((0.013 * step + duration * a / actors) % duration) for a in range(actors)]

    def device_calls_host_fed():
        rc = L.sr_scene_pose_meshes(sc._h, pose_rows, C.c_uint32(actors), None)
        if rc == 0:
            rc = L.sr_scene_set_instances(sc._h, p(lkeys), p(lcounts), C.c_uint32(len(lkeys)), p(xf))
        return rc

    def path_a(ts):
        t0 = time.perf_counter()
        rc = 0
        for a in range(actors):
            rc |= L.sr_gltf_pose(g._h, C.c_int32(0), ts[a], xf_at[a], C.c_uint32(0), None)
            rc |= L.sr_gltf_pose(g._h, C.c_int32(0), ts[a], None, C.c_uint32(0), jm_at[a])
        t1 = time.perf_counter()
        rc |= device_calls_host_fed()
        t2 = time.perf_counter()
        check(rc)
        return (t2 - t0) * 1e3, (t1 - t0) * 1e3

    def path_b(ts):
        t0 = time.perf_counter()
        rc = 0
        for a in range(actors):
            rc |= L.sr_clip_pose_host(clip._h, ts[a], None, jm_at[a], xf_at[a])
        t1 = time.perf_counter()
        rc |= device_calls_host_fed()
        t2 = time.perf_counter()
        check(rc)
        return (t2 - t0) * 1e3, (t1 - t0) * 1e3

    def path_c(ts):
        t0 = time.perf_counter()
        for a in range(actors):
            args.actors[a].time_seconds = ts[a]
        rc = L.sr_scene_pose_actors(sc._h, args.actors, C.c_uint32(actors), args.items, C.c_uint32(actors), d_ptr, C.c_uint32(0), None)
        if rc == 0:
            rc = L.sr_scene_set_instances_device(sc._h, p(lkeys), p(lcounts), C.c_uint32(len(lkeys)), d_ptr, None)
        t1 = time.perf_counter()
        check(rc)
        return (t1 - t0) * 1e3, 0.0

    out = {"actors": actors, "joints": joints, "nodes": n_nodes, "channels": clip.info.n_channels, "vertices_per_mesh": 4, "instances_per_actor": ni}
    wall = {"A": [], "B": [], "C": [], "A_eval": [], "B_eval": []}
    for step in range(WARMUP + REPS):
        ts = times_of(step)
        a, b, c = path_a(ts), path_b(ts), path_c(ts)
        if step >= WARMUP:
            wall["A"].append(a[0]); wall["B"].append(b[0]); wall["C"].append(c[0]); wall["A_eval"].append(a[1]); wall["B_eval"].append(b[1])
    sc.enable_timing(True)
    dev = {"A": [], "B": [], "C": [], "C_clip": []}
    for step in range(WARMUP + REPS):
        ts = times_of(100 + step)
        got = {}
        for name, fn in (("A", path_a), ("B", path_b)):
            fn(ts)
            i = sc.pose_batch_info()
            got[name] = i.pose_ms + i.scatter_ms + sc.instance_update_info().tables_ms
        path_c(ts)
        i = sc.actor_pose_info()
        got["C"], got["C_clip"] = i.clip_ms + i.pose_ms + i.scatter_ms + sc.instance_update_info().tables_ms, i.clip_ms
        if step >= WARMUP:
            for k, v in got.items():
                dev[k].append(v)
    sc.enable_timing(False)
    out["upload_bytes"] = {"A_B": sc.pose_batch_info().upload_bytes, "C": sc.actor_pose_info().upload_bytes}
    out["wall_ms"] = {k: stats(v) for k, v in wall.items()}
    out["device_ms"] = {k: stats(v) for k, v in dev.items()}
    out["eval_us_per_actor"] = {k: 1e3 * out["wall_ms"][k + "_eval"]["median"] / actors for k in ("A", "B")}
    w = out["wall_ms"]

    def verdict(x, y):
        return "%s wins" % y if w[y]["max"] < w[x]["min"] else "%s wins" % x if w[x]["max"] < w[y]["min"] else "ranges overlap"
    out["verdict"] = {"B against A": verdict("A", "B"), "C against A": verdict("A", "C"), "C against B": verdict("B", "C")}
    sc.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_pose.json"))
    ap.add_argument("--only", action="append", help="a case to run (may be given several times); default: all")
    args = ap.parse_args()
    result = {"what": "one crowd step (evaluation + posing + instance tables): A sr_gltf_pose per actor, B sr_clip_pose_host per actor, C sr_scene_pose_actors; "
                      "wall clock and device (event) milliseconds", "reps": REPS, "warmup": WARMUP, "cases": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for case in CASES:
            if args.only and case not in args.only:
                continue
            c = result["cases"][case] = measure(case, tmp)
            print("%-9s" % case + "".join("   %s %8.3f (%.3f - %.3f) ms" % (k, c["wall_ms"][k]["median"], c["wall_ms"][k]["min"], c["wall_ms"][k]["max"]) for k in "ABC") +
                  "   " + c["verdict"]["C against A"], flush=True)
            with open(args.out, "w") as f:
                json.dump(result, f, indent=1)
                f.write("\n")
    print(args.out)


if __name__ == "__main__":
    main()
