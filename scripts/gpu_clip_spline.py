"""Cost of CUBICSPLINE clips on the device against LINEAR ones, and what the cubic branch costs the LINEAR path, for one step
of a crowd (evaluation + posing, without the instance tables):

  a  sr_scene_pose_actors on the CUBICSPLINE clip                                             this build
  b  sr_scene_pose_actors on the LINEAR clip                                                  this build
  c  sr_scene_pose_actors on the LINEAR clip                                                  the parent commit's library (--parent-lib)
  d  the host route under SR_CUBICSPLINE_SAMPLE: sr_gltf_pose per actor, then sr_scene_pose_meshes    this build
  ma / mb / mc   the same three for 1 000 morphed actors whose weights come from their clip: a CUBICSPLINE `weights` channel
                 (clip_spline_weights_kernel), a LINEAR one (clip_weights_kernel), the LINEAR one on the parent's library

Crowd: 1 000 actors of a rig of 64 joints (clip_util.shape_rig: a chain of 64 nodes, each turned by a rotation channel of 4 keys;
one skinned quad per actor); the cubic file is the same file with every sampler turned into a CUBICSPLINE one on the same keys
(clip_spline_util.cubic_copy, tangents of the neighbouring keys' slope). Morphs: one quad of 52 targets per actor on a `weights`
channel of 4 keys, the cubic file made the same way. A library is chosen when the process starts (SUNRAY_HIP_LIB), so each
variant is measured in child processes of its own, this build and the parent's alternating, ROUNDS rounds of REPS / ROUNDS steps
after WARMUP each; within a process its paths alternate step by step. Wall clock with the event timing off; then, in a second
pass, the device time (clip_ms + pose_ms + scatter_ms), clip_ms alone and, for ma, the spline weights kernel alone. Median
(min - max) of REPS steps.

  python scripts/gpu_clip_spline.py [--out profiles/clip_spline.json] [--parent-lib PATH]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REPS, WARMUP, ROUNDS = 20, 3, 2
ACTORS, JOINTS, TARGETS = 1000, 64, 52


def stats(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1], "n": len(xs)}


def worker(parent, reps, first_step):
    """One process on one library -> {path: {"wall": [...], "device": [...], "clip": [...], "spline": [...]}}."""
    import torch
    from clip_morph_util import one_morphed_quad
    from clip_spline_util import cubic_copy
    from clip_util import crowd, shape_rig
    from sunray_amd import abi, runtime as rt
    from sunray_amd._lib import check, lib
    L = lib()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for kind in ("rig", "morph"):
            linear_path, cubic_path = os.path.join(tmp, kind + "_linear.glb"), os.path.join(tmp, kind + "_cubic.glb")
            if kind == "rig":
                shape_rig(linear_path, chain=JOINTS, joints=JOINTS, channels=JOINTS, keys=4)
            else:
                morph_duration = one_morphed_quad(linear_path, TARGETS)
            cubic_copy(linear_path, cubic_path, tangent=1.0)
            desc, g, keys, rigs, layout, rows, skins, ib = crowd(rt, linear_path, ACTORS)
            sc = rt.Scene(0, instancing="two_level").load(desc)
            for key, (inf, nj) in rigs.items():
                sc.set_mesh_build_type(key, abi.BUILD_RAPIDLY_CHANGING)
                sc.set_mesh_skin(key, inf, nj)
            if kind == "morph":
                deltas = g.blas_morph(0)[0]
                for a in range(ACTORS):
                    sc.set_mesh_build_type(keys[a][0], abi.BUILD_RAPIDLY_CHANGING)
                    sc.set_mesh_morph(keys[a][0], deltas)
            sc.set_instances(desc.instances)
            clips = {"b": g.bake_clip(0)}
            gc = None
            if not parent:
                gc = rt.Gltf(cubic_path)
                gc.set_cubicspline(True)
                clips["a"] = gc.bake_clip(0)
            ids = {k: sc.attach_clip(c) for k, c in clips.items()}
            duration = clips["b"].info.duration_seconds if kind == "rig" else morph_duration     # a clip's own duration counts no `weights` channel
            ni = len(rows)
            blas = skins.index(0) if kind == "rig" else 0
            item = (lambda a: (keys[a][blas], a, 0, None)) if kind == "rig" else (lambda a: (keys[a][0], a, None, rt.ClipWeights(0)))
            args = {k: rt.ActorArgs([(ids[k], 0.0, None, None, a * ni) for a in range(ACTORS)], [item(a) for a in range(ACTORS)]) for k in clips}
            d_xf = torch.zeros((ACTORS * ni, 12), dtype=torch.float32, device="cuda:0")
            d_ptr = C.c_void_p(d_xf.data_ptr())
            jm, xf = np.zeros((ACTORS, JOINTS, 12), np.float32), np.zeros((ACTORS * ni, 12), np.float32)
            jm_at = [C.c_void_p(jm[a].ctypes.data) for a in range(ACTORS)]
            xf_at = [C.c_void_p(xf[a * ni:].ctypes.data) for a in range(ACTORS)]
            pose_rows = (abi.SrPoseItem * ACTORS)()
            for a in range(ACTORS if kind == "rig" else 0):
                pose_rows[a].key, pose_rows[a].joint_matrices, pose_rows[a].n_joints = keys[a][blas], jm_at[a].value, JOINTS

            def times_of(step):
                return [C.c_float((0.013 * step + duration * a / ACTORS) % duration) for a in range(ACTORS)]

            def device_path(k, ts):
                t0 = time.perf_counter()
                for a in range(ACTORS):
                    args[k].actors[a].time_seconds = ts[a]
                rc = L.sr_scene_pose_actors(sc._h, args[k].actors, C.c_uint32(ACTORS), args[k].items, C.c_uint32(ACTORS), d_ptr, C.c_uint32(0), None)
                t1 = time.perf_counter()
                check(rc)
                return (t1 - t0) * 1e3

            def host_path(ts):
                t0 = time.perf_counter()
                rc = 0
                for a in range(ACTORS):
                    rc |= L.sr_gltf_pose(gc._h, C.c_int32(0), ts[a], xf_at[a], C.c_uint32(0), jm_at[a])
                rc |= L.sr_scene_pose_meshes(sc._h, pose_rows, C.c_uint32(ACTORS), None)
                t1 = time.perf_counter()
                check(rc)
                return (t1 - t0) * 1e3
            names = {"a": "a", "b": "c" if parent else "b"} if kind == "rig" else {"a": "ma", "b": "mc" if parent else "mb"}
            paths = [(names[k], (lambda ts, k=k: device_path(k, ts))) for k in sorted(clips)]
            if kind == "rig" and not parent:
                paths.append(("d", host_path))
            for name, _ in paths:
                out[name] = {"wall": [], "device": [], "clip": [], "spline": []}
            for timing in (False, True):
                sc.enable_timing(timing)
                for step in range(WARMUP + reps):
                    ts = times_of(first_step + step + (100 if timing else 0))
                    for name, fn in paths:
                        ms = fn(ts)
                        if step < WARMUP:
                            continue
                        if not timing:
                            out[name]["wall"].append(ms)
                        elif name == "d":
                            i = sc.pose_batch_info()
                            out[name]["device"].append(i.pose_ms + i.scatter_ms)
                        else:
                            i = sc.actor_pose_info()
                            out[name]["device"].append(i.clip_ms + i.pose_ms + i.scatter_ms)
                            out[name]["clip"].append(i.clip_ms)
                            if name == "ma":
                                sp = sc.spline_pose_info()
                                assert (sp.spline_weight_rows, sp.plain_weight_rows, i.launches) == (ACTORS, 0, 4)
                                out[name]["spline"].append(sp.spline_weights_ms)
            sc.enable_timing(False)
            sc.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_spline.json"))
    ap.add_argument("--parent-lib", help="the parent commit's libsunray_hip.so: cases c and mc (left out without it)")
    ap.add_argument("--worker", choices=("this", "parent"), help=argparse.SUPPRESS)
    ap.add_argument("--reps", type=int, default=REPS // ROUNDS, help=argparse.SUPPRESS)
    ap.add_argument("--first-step", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        print("RESULT " + json.dumps(worker(args.worker == "parent", args.reps, args.first_step)))
        return
    samples = {}
    for rnd in range(ROUNDS):
        for variant in ("this", "parent"):
            if variant == "parent" and not args.parent_lib:
                continue
            env = dict(os.environ)
            env.pop("SUNRAY_HIP_LIB", None)
            if variant == "parent":
                env["SUNRAY_HIP_LIB"] = os.path.abspath(args.parent_lib)
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", variant, "--reps", str(REPS // ROUNDS), "--first-step", str(rnd * 50)]
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                raise SystemExit("the %s worker of round %d failed (%d)" % (variant, rnd, r.returncode))
            got = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
            for name, lists in got.items():
                for k, v in lists.items():
                    samples.setdefault(name, {}).setdefault(k, []).extend(v)
            print("round %d, %s: %s" % (rnd, variant, ", ".join(sorted(got))), flush=True)
    what = {"a": "pose_actors, CUBICSPLINE clip, this build", "b": "pose_actors, LINEAR clip, this build", "c": "pose_actors, LINEAR clip, the parent's library",
            "d": "sr_gltf_pose per actor under SAMPLE + pose_meshes, this build", "ma": "clip weights, CUBICSPLINE set, this build (clip_spline_weights_kernel)",
            "mb": "clip weights, LINEAR set, this build (clip_weights_kernel)", "mc": "clip weights, LINEAR set, the parent's library"}
    result = {"what": "one crowd step (evaluation + posing): %d actors of %d joints; %d morphed actors of %d targets; wall clock and device (event) milliseconds"
                      % (ACTORS, JOINTS, ACTORS, TARGETS), "reps": REPS, "warmup": WARMUP, "rounds": ROUNDS, "paths": {k: v for k, v in what.items() if k in samples},
              "wall_ms": {}, "device_ms": {}, "clip_ms": {}, "spline_weights_ms": {}}
    for name, lists in samples.items():
        result["wall_ms"][name] = stats(lists["wall"])
        result["device_ms"][name] = stats(lists["device"])
        if lists["clip"]:
            result["clip_ms"][name] = stats(lists["clip"])
        if lists["spline"]:
            result["spline_weights_ms"][name] = stats(lists["spline"])

    def verdict(table, x, y):
        t = result[table]
        if x not in t or y not in t:
            return "not measured"
        return "%s is faster" % y if t[y]["max"] < t[x]["min"] else "%s is faster" % x if t[x]["max"] < t[y]["min"] else "ranges overlap"
    result["verdict"] = {"%s: %s against %s" % (table, x, y): verdict(table, x, y) for table in ("wall_ms", "device_ms", "clip_ms")
                         for x, y in (("a", "b"), ("b", "c"), ("a", "d"), ("ma", "mb"), ("mb", "mc")) if not (table == "clip_ms" and y == "d")}
    for name in samples:
        w, d = result["wall_ms"][name], result["device_ms"][name]
        print("%-3s wall %8.3f (%.3f - %.3f) ms   device %8.3f (%.3f - %.3f) ms   %s" % (name, w["median"], w["min"], w["max"], d["median"], d["min"], d["max"], what[name]))
    for k, v in result["verdict"].items():
        print("%-28s %s" % (k, v))
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(args.out)


if __name__ == "__main__":
    main()
