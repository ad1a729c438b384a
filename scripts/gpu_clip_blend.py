"""Cost of one step of a crowd whose every actor cross-fades between two clips, evaluation plus posing, up to the posed vertices and
the instance tables, by three paths of one build:

  H  the host route, what a cross-fade cost before: per actor two sr_clip_sample_host, sr_clip_blend_host and
     sr_clip_compose_records_host, then sr_scene_pose_meshes + sr_scene_set_instances
  D  sr_scene_pose_actors_blended (clip_blend_kernel in front of the posing kernel) + sr_scene_set_instances_device
  P  the same crowd without a fade: sr_scene_pose_actors + sr_scene_set_instances_device: what the second source and the blend add

Cases: 100 and 1 000 actors of a rig of 64 joints (a chain of that many nodes, each turned by a LINEAR rotation channel of 4 keys;
one skinned and one unskinned quad of 4 vertices per actor, so that evaluation and not vertex work is what is measured). Both
sources are the animated clip, attached twice, each at its own time; the weight runs over (0, 1). Every path is timed at the C entry
points with its arguments packed beforehand. Wall clock of the step with the event timing off; then, with it on, the device time
(H: pose_ms + scatter_ms + tables_ms; D, P: clip_ms + pose_ms + scatter_ms + tables_ms). "eval" is the host evaluation part of H
alone. Median (min - max) of REPS steps after WARMUP, the paths alternating.

  python scripts/gpu_clip_blend.py [--out profiles/clip_blend.json] [--only CASE]...
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
CASES = {"%dx%dj" % (actors, joints): (actors, joints) for joints in (64,) for actors in (100, 1000)}


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
    ida, idb = sc.attach_clip(clip), sc.attach_clip(clip)
    L, ni = lib(), len(rows)
    assert list(rows) == list(range(ni))                    # one instance a blas, in blas order: a copy's rows are its own, in order
    duration = clip.info.duration_seconds
    jm, xf = np.zeros((actors, joints, 12), np.float32), np.zeros((actors * ni, 12), np.float32)
    trs_a, trs_b, trs = (np.zeros(n_nodes, abi.NODE_TRS) for _ in range(3))
    jm_at = [C.c_void_p(jm[a].ctypes.data) for a in range(actors)]
    xf_at = [C.c_void_p(xf[a * ni:].ctypes.data) for a in range(actors)]
    skinned_key = [keys[a][skins.index(0)] for a in range(actors)]
    pose_rows = (abi.SrPoseItem * actors)()
    for a in range(actors):
        pose_rows[a].key, pose_rows[a].joint_matrices, pose_rows[a].n_joints = skinned_key[a], jm_at[a].value, joints
    lkeys, lcounts = np.array([k for k, _ in layout], np.uint64), np.array([c for _, c in layout], np.uint32)
    items = [(skinned_key[a], a, 0, None) for a in range(actors)]
    blended = rt.BlendedActorArgs([(ida, 0.0, idb, 0.0, 0.5, None, None, a * ni) for a in range(actors)], items)
    plain = rt.ActorArgs([(ida, 0.0, None, None, a * ni) for a in range(actors)], items)
    d_xf = torch.zeros((actors * ni, 12), dtype=torch.float32, device="cuda:0")
    d_ptr = C.c_void_p(d_xf.data_ptr())
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    pa, pb, pt = p(trs_a), p(trs_b), p(trs)

    def times_of(step):
        """Per actor: A's time, B's time, the weight (never an end weight: those cost the blend nothing)."""
        return [(C.c_float((0.013 * step + duration * a / actors) % duration), C.c_float((0.4 * duration + 0.017 * step + duration * a / actors) % duration),
                 C.c_float(0.05 + 0.9 * ((0.07 * step + a / actors) % 1.0))) for a in range(actors)]

    def path_h(ts):
        t0 = time.perf_counter()
        rc = 0
        for a in range(actors):
            rc |= L.sr_clip_sample_host(clip._h, ts[a][0], pa)
            rc |= L.sr_clip_sample_host(clip._h, ts[a][1], pb)
            rc |= L.sr_clip_blend_host(pa, pb, C.c_uint32(n_nodes), ts[a][2], pt)
            rc |= L.sr_clip_compose_records_host(clip._h, pt, None, jm_at[a], xf_at[a], None)
        t1 = time.perf_counter()
        rc |= L.sr_scene_pose_meshes(sc._h, pose_rows, C.c_uint32(actors), None)
        if rc == 0:
            rc = L.sr_scene_set_instances(sc._h, p(lkeys), p(lcounts), C.c_uint32(len(lkeys)), p(xf))
        t2 = time.perf_counter()
        check(rc)
        return (t2 - t0) * 1e3, (t1 - t0) * 1e3

    def path_d(ts):
        t0 = time.perf_counter()
        for a in range(actors):
            row = blended.actors[a]
            row.time_seconds, row.time_seconds_b, row.weight = ts[a]
        rc = L.sr_scene_pose_actors_blended(sc._h, blended.actors, C.c_uint32(actors), blended.items, C.c_uint32(actors), d_ptr, C.c_uint32(0), None)
        if rc == 0:
            rc = L.sr_scene_set_instances_device(sc._h, p(lkeys), p(lcounts), C.c_uint32(len(lkeys)), d_ptr, None)
        t1 = time.perf_counter()
        check(rc)
        return (t1 - t0) * 1e3, 0.0

    def path_p(ts):
        t0 = time.perf_counter()
        for a in range(actors):
            plain.actors[a].time_seconds = ts[a][0]
        rc = L.sr_scene_pose_actors(sc._h, plain.actors, C.c_uint32(actors), plain.items, C.c_uint32(actors), d_ptr, C.c_uint32(0), None)
        if rc == 0:
            rc = L.sr_scene_set_instances_device(sc._h, p(lkeys), p(lcounts), C.c_uint32(len(lkeys)), d_ptr, None)
        t1 = time.perf_counter()
        check(rc)
        return (t1 - t0) * 1e3, 0.0

    out = {"actors": actors, "joints": joints, "nodes": n_nodes, "channels_per_source": clip.info.n_channels, "vertices_per_mesh": 4, "instances_per_actor": ni}
    wall = {"H": [], "D": [], "P": [], "H_eval": []}
    for step in range(WARMUP + REPS):
        ts = times_of(step)
        h, d, pl = path_h(ts), path_d(ts), path_p(ts)
        if step >= WARMUP:
            wall["H"].append(h[0]); wall["D"].append(d[0]); wall["P"].append(pl[0]); wall["H_eval"].append(h[1])
    sc.enable_timing(True)
    dev = {"H": [], "D": [], "P": [], "D_clip": [], "P_clip": []}
    for step in range(WARMUP + REPS):
        ts = times_of(100 + step)
        got = {}
        path_h(ts)
        i = sc.pose_batch_info()
        got["H"] = i.pose_ms + i.scatter_ms + sc.instance_update_info().tables_ms
        for name, fn in (("D", path_d), ("P", path_p)):
            fn(ts)
            i = sc.actor_pose_info()
            got[name], got[name + "_clip"] = i.clip_ms + i.pose_ms + i.scatter_ms + sc.instance_update_info().tables_ms, i.clip_ms
        if step >= WARMUP:
            for k, v in got.items():
                dev[k].append(v)
    sc.enable_timing(False)
    path_d(times_of(0))
    upload_d = sc.actor_pose_info().upload_bytes
    path_p(times_of(0))
    out["upload_bytes"] = {"H": sc.pose_batch_info().upload_bytes, "D": upload_d, "P": sc.actor_pose_info().upload_bytes}
    out["wall_ms"] = {k: stats(v) for k, v in wall.items()}
    out["device_ms"] = {k: stats(v) for k, v in dev.items()}
    out["eval_us_per_actor"] = {"H": 1e3 * out["wall_ms"]["H_eval"]["median"] / actors}
    w = out["wall_ms"]

    def verdict(x, y):
        return "%s wins" % y if w[y]["max"] < w[x]["min"] else "%s wins" % x if w[x]["max"] < w[y]["min"] else "ranges overlap"
    out["verdict"] = {"D against H": verdict("H", "D"), "P against D": verdict("D", "P")}
    sc.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_blend.json"))
    ap.add_argument("--only", action="append", help="a case to run (may be given several times); default: all")
    args = ap.parse_args()
    result = {"what": "one step of a crowd that cross-fades between two clips (evaluation + posing + instance tables): H two sr_clip_sample_host, sr_clip_blend_host and "
                      "sr_clip_compose_records_host per actor, D sr_scene_pose_actors_blended, P sr_scene_pose_actors without a fade; wall clock and device (event) "
                      "milliseconds", "reps": REPS, "warmup": WARMUP, "cases": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for case in CASES:
            if args.only and case not in args.only:
                continue
            c = result["cases"][case] = measure(case, tmp)
            print("%-9s" % case + "".join("   %s %8.3f (%.3f - %.3f) ms" % (k, c["wall_ms"][k]["median"], c["wall_ms"][k]["min"], c["wall_ms"][k]["max"]) for k in "HDP") +
                  "   " + c["verdict"]["D against H"] + "; " + c["verdict"]["P against D"], flush=True)
            with open(args.out, "w") as f:
                json.dump(result, f, indent=1)
                f.write("\n")
    print(args.out)


if __name__ == "__main__":
    main()
