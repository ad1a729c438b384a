"""Cost of one step of a crowd of morphed characters, weight evaluation plus posing, by three paths of one build:

  A  sr_gltf_morph_weights per actor, then sr_scene_pose_actors with host weights: the path before clip weights existed
  B  sr_clip_weights_host per actor (the baked set on the host), then the same call: what the bake alone buys
  C  sr_scene_pose_actors with SR_ACTOR_CLIP_WEIGHTS (clip_weights_kernel in front of the posing kernel)

Cases: 1, 10, 100 and 1 000 actors, each with one morphed quad of 4 vertices and of 4 and of 52 targets on a LINEAR `weights`
channel of 4 keys, so that the evaluation and not the vertex work is what is measured. Every path is timed at the C entry points
with its arguments packed beforehand. Wall clock of the step with the event timing off; then, with it on, the device time (clip_ms
+ pose_ms + scatter_ms). clip_ms covers clip_pose_kernel and, in C, clip_weights_kernel: "C_weights" is C's clip_ms less A's, the
same actors without the weights kernel, step by step. "eval" is the host evaluation part of A and B alone. Median (min - max) of
REPS steps after WARMUP, the paths alternating.

  python scripts/gpu_clip_morph.py [--out profiles/clip_morph.json] [--only CASE]...
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
CASES = {"%dx%dt" % (actors, targets): (actors, targets) for targets in (4, 52) for actors in (1, 10, 100, 1000)}


def stats(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1], "n": len(xs)}


def measure(case, tmp):
    from clip_morph_util import one_morphed_quad
    from clip_util import crowd
    from sunray_amd import abi, runtime as rt
    from sunray_amd._lib import check, lib
    actors, targets = CASES[case]
    path = os.path.join(tmp, case + ".glb")
    duration = one_morphed_quad(path, targets)
    desc, g, keys, rigs, layout, rows, skins, ib = crowd(rt, path, actors)
    sc = rt.Scene(0, instancing="two_level").load(desc)
    deltas = g.blas_morph(0)[0]
    for a in range(actors):
        sc.set_mesh_build_type(keys[a][0], abi.BUILD_RAPIDLY_CHANGING)
        sc.set_mesh_morph(keys[a][0], deltas)
    sc.set_instances(desc.instances)
    clip = g.bake_clip(0)
    cid = sc.attach_clip(clip)
    L = lib()
    w = np.zeros((actors, targets), np.float32)
    w_at = [C.c_void_p(w[a].ctypes.data) for a in range(actors)]
    host = rt.ActorArgs([(cid, 0.0, None, None, 0) for a in range(actors)], [(keys[a][0], a, None, w[a]) for a in range(actors)])
    for a in range(actors):
        host.items[a].weights = w_at[a].value                  # the rows of `w` themselves, which A and B fill
    device = rt.ActorArgs([(cid, 0.0, None, None, 0) for a in range(actors)], [(keys[a][0], a, None, rt.ClipWeights(0)) for a in range(actors)])

    def times_of(step):
        return [C.c_float((0.013 * step + duration * a / actors) % duration) for a in range(actors)]

    def call(args, ts):
        for a in range(actors):
            args.actors[a].time_seconds = ts[a]
        return L.sr_scene_pose_actors(sc._h, args.actors, C.c_uint32(actors), args.items, C.c_uint32(actors), None, C.c_uint32(0), None)

    def path_a(ts):
        t0 = time.perf_counter()
        rc = 0
        for a in range(actors):
            rc |= L.sr_gltf_morph_weights(g._h, C.c_int32(0), ts[a], C.c_uint32(0), w_at[a], C.c_uint32(targets))
        t1 = time.perf_counter()
        rc |= call(host, ts)
        t2 = time.perf_counter()
        check(rc)
        return (t2 - t0) * 1e3, (t1 - t0) * 1e3

    def path_b(ts):
        t0 = time.perf_counter()
        rc = 0
        for a in range(actors):
            rc |= L.sr_clip_weights_host(clip._h, ts[a], C.c_uint32(0), w_at[a], C.c_uint32(targets))
        t1 = time.perf_counter()
        rc |= call(host, ts)
        t2 = time.perf_counter()
        check(rc)
        return (t2 - t0) * 1e3, (t1 - t0) * 1e3

    def path_c(ts):
        t0 = time.perf_counter()
        rc = call(device, ts)
        t1 = time.perf_counter()
        check(rc)
        return (t1 - t0) * 1e3, 0.0

    out = {"actors": actors, "targets": targets, "keys": 4, "vertices_per_mesh": 4}
    wall = {"A": [], "B": [], "C": [], "A_eval": [], "B_eval": []}
    for step in range(WARMUP + REPS):
        ts = times_of(step)
        a, b, c = path_a(ts), path_b(ts), path_c(ts)
        if step >= WARMUP:
            wall["A"].append(a[0]); wall["B"].append(b[0]); wall["C"].append(c[0]); wall["A_eval"].append(a[1]); wall["B_eval"].append(b[1])
    sc.enable_timing(True)
    dev = {"A": [], "B": [], "C": [], "C_weights": []}
    uploads = {}
    for step in range(WARMUP + REPS):
        ts = times_of(100 + step)
        got, clip_ms = {}, {}
        for name, fn in (("A", path_a), ("B", path_b), ("C", path_c)):
            fn(ts)
            i = sc.actor_pose_info()
            got[name], clip_ms[name], uploads[name] = i.clip_ms + i.pose_ms + i.scatter_ms, i.clip_ms, i.upload_bytes
            assert (i.launches, i.weight_items) == ((4, actors) if name == "C" else (3, 0))
        got["C_weights"] = clip_ms["C"] - clip_ms["A"]
        if step >= WARMUP:
            for k, v in got.items():
                dev[k].append(v)
    sc.enable_timing(False)
    out["upload_bytes"] = {"A_B": uploads["A"], "C": uploads["C"]}
    out["wall_ms"] = {k: stats(v) for k, v in wall.items()}
    out["device_ms"] = {k: stats(v) for k, v in dev.items()}
    out["eval_us_per_actor"] = {k: 1e3 * out["wall_ms"][k + "_eval"]["median"] / actors for k in ("A", "B")}
    wm = out["wall_ms"]

    def verdict(x, y):
        return "%s wins" % y if wm[y]["max"] < wm[x]["min"] else "%s wins" % x if wm[x]["max"] < wm[y]["min"] else "ranges overlap"
    out["verdict"] = {"B against A": verdict("A", "B"), "C against A": verdict("A", "C"), "C against B": verdict("B", "C")}
    sc.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_morph.json"))
    ap.add_argument("--only", action="append", help="a case to run (may be given several times); default: all")
    args = ap.parse_args()
    result = {"what": "one step of a crowd of morphed characters (weight evaluation + posing): A sr_gltf_morph_weights per actor, B sr_clip_weights_host per actor, "
                      "C clip weights on the device; wall clock and device (event) milliseconds", "reps": REPS, "warmup": WARMUP, "cases": {}}
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
