"""Cost of layered morph weights (SR_ACTORS_LAYER_WEIGHTS) for one step of a crowd of morphed actors, evaluation plus posing up to
the posed vertices, by the paths of one build:

  U  sr_scene_pose_actors_layered without the flag: the weights are the base layer's (clip_weights_kernel / clip_spline_weights_kernel)
  W  the same call with the flag: the weights go through the stack (clip_layer_weights_kernel)
  H  the host route to the same vertices: sr_clip_weights_layers_host per item, then sr_scene_pose_meshes
  B  at two layers only: the same crowd through sr_scene_pose_actors_blended (both layers unmasked overrides for this comparison's W2)
  K  the kernels alone, from events: clip_layer_weights_kernel on one-layer CUBICSPLINE rows (SrLayerWeightsInfo.weights_ms) against
     clip_spline_weights_kernel on the same rows through sr_scene_pose_actors (SrSplinePoseInfo.spline_weights_ms)

Case: 1 000 actors, each one quad of 52 morph targets on a `weights` channel of 4 keys, at 1, 2, 4 and 8 layers. Layer l takes the
LINEAR clip where l is even and its CUBICSPLINE copy (clip_spline_util.cubic_copy) where l is odd; layer l > 0 is additive where l is
even and an override otherwise, and is masked (0.5 on the mesh node) where l % 4 is 1 or 2. Every path is timed at the C entry
points with its arguments packed beforehand. Wall clock, median (min - max) of REPS steps after WARMUP, the paths alternating.
--parent-lib runs U alone in a process of its own, once on this build's library and once on another build's (SUNRAY_HIP_LIB): the
unflagged call is what the parent commit does, so the two must overlap.

  python scripts/gpu_clip_layer_weights.py [--out profiles/clip_layer_weights.json] [--parent-lib PATH]
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
REPS, WARMUP = 20, 3
ACTORS, TARGETS, LAYER_COUNTS = 1000, 52, (1, 2, 4, 8)


def stats(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1], "n": len(xs)}


def verdict(w, x, y):
    return "%s wins" % y if w[y]["max"] < w[x]["min"] else "%s wins" % x if w[x]["max"] < w[y]["min"] else "ranges overlap"


def measure(tmp, unflagged_only):
    from clip_morph_util import one_morphed_quad
    from clip_spline_util import cubic_copy
    from clip_util import crowd
    from sunray_amd import abi, runtime as rt
    from sunray_amd._lib import LIB_PATH, check, lib
    actors = ACTORS
    linear_path, cubic_path = os.path.join(tmp, "linear.glb"), os.path.join(tmp, "cubic.glb")
    duration = one_morphed_quad(linear_path, TARGETS)
    cubic_copy(linear_path, cubic_path, tangent=1.0)
    c = crowd(rt, linear_path, actors)
    desc, g, keys = c[0], c[1], c[2]
    sc = rt.Scene(0).load(desc)
    deltas = g.blas_morph(0)[0]
    for a in range(actors):
        sc.set_mesh_morph(keys[a][0], deltas)
    gc = rt.Gltf(cubic_path)
    gc.set_cubicspline(True)
    clips = [g.bake_clip(0), gc.bake_clip(0)]
    ids = [sc.attach_clip(cl) for cl in clips]
    n_nodes = clips[0].info.n_nodes
    half = np.full(n_nodes, 0.5, np.float32)
    L = lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    items = [(keys[a][0], a, None, rt.ClipWeights(0)) for a in range(actors)]
    out = {"library": os.path.basename(os.path.dirname(LIB_PATH)) + "/" + os.path.basename(LIB_PATH), "actors": actors, "targets": TARGETS, "cases": {}}

    def t_of(step, a, l):
        return (0.013 * step + 0.11 * l + duration * a / actors) % duration

    mask_id = sc.attach_node_mask(half)
    for n_layers in LAYER_COUNTS:
        additive = [l > 0 and l % 2 == 0 for l in range(n_layers)]
        masked = [l % 4 in (1, 2) for l in range(n_layers)]
        weight = [1.0 if l == 0 else 0.3 + 0.05 * l for l in range(n_layers)]
        stack = lambda unmasked: [(ids[l % 2], 0.0, weight[l], "additive" if additive[l] else "override", mask_id if masked[l] and not unmasked else None, 0.0)   # noqa: E731
                                  for l in range(n_layers)]
        layered = rt.LayeredActorArgs([(stack(n_layers == 2), None, None, 0) for a in range(actors)], items)

        def call_layered(step, flags):
            t0 = time.perf_counter()
            for a in range(actors):
                for l in range(n_layers):
                    row = layered.layers[layered.first_layer[a] + l]
                    row.time_seconds, row.ref_time_seconds = t_of(step, a, l), t_of(step, a, l + 8)
            check(L.sr_scene_pose_actors_layered(sc._h, layered.actors, C.c_uint32(actors), layered.items, C.c_uint32(actors), None, C.c_uint32(flags), None))
            return (time.perf_counter() - t0) * 1e3

        names = ["U"] if unflagged_only else ["U", "W", "H"] + (["B"] if n_layers == 2 else [])
        wall = {k: [] for k in names + (["H_eval"] if not unflagged_only else [])}
        if not unflagged_only:
            host_clips = (C.c_void_p * n_layers)(*[clips[l % 2]._h for l in range(n_layers)])
            host_masks = (C.c_void_p * n_layers)(*[half.ctypes.data if masked[l] and n_layers != 2 else None for l in range(n_layers)])
            host_rows = (abi.SrClipLayer * n_layers)()
            for l in range(n_layers):
                host_rows[l].weight, host_rows[l].mode, host_rows[l].mask_id = weight[l], abi.LAYER_ADDITIVE if additive[l] else abi.LAYER_OVERRIDE, abi.LAYER_NO_MASK
            host_w = np.zeros((actors, TARGETS), np.float32)
            pose_rows = (abi.SrPoseItem * actors)()
            for a in range(actors):
                pose_rows[a].key, pose_rows[a].weights, pose_rows[a].n_targets = keys[a][0], host_w[a].ctypes.data, TARGETS
            blended = rt.BlendedActorArgs([(ids[0], 0.0, ids[1], 0.0, weight[1] if n_layers > 1 else 0.0, None, None, 0) for a in range(actors)], items)

            def path_h(step):
                t0 = time.perf_counter()
                rc = 0
                for a in range(actors):
                    for l in range(n_layers):
                        host_rows[l].time_seconds, host_rows[l].ref_time_seconds = t_of(step, a, l), t_of(step, a, l + 8)
                    rc |= L.sr_clip_weights_layers_host(host_clips, host_rows, host_masks, C.c_uint32(n_layers), C.c_uint32(0), C.c_void_p(host_w[a].ctypes.data), C.c_uint32(TARGETS))
                t1 = time.perf_counter()
                rc |= L.sr_scene_pose_meshes(sc._h, pose_rows, C.c_uint32(actors), None)
                check(rc)
                return (time.perf_counter() - t0) * 1e3, (t1 - t0) * 1e3

            def path_b(step):
                t0 = time.perf_counter()
                for a in range(actors):
                    row = blended.actors[a]
                    row.time_seconds, row.time_seconds_b = t_of(step, a, 0), t_of(step, a, 1)
                check(L.sr_scene_pose_actors_blended(sc._h, blended.actors, C.c_uint32(actors), blended.items, C.c_uint32(actors), None, C.c_uint32(0), None))
                return (time.perf_counter() - t0) * 1e3

        for step in range(WARMUP + REPS):
            got = {"U": call_layered(step, 0)}
            if not unflagged_only:
                got["W"] = call_layered(step, abi.ACTORS_LAYER_WEIGHTS)
                got["H"], got["H_eval"] = path_h(step)
                if n_layers == 2:
                    got["B"] = path_b(step)
            if step >= WARMUP:
                for k, v in got.items():
                    wall[k].append(v)
        w = {k: stats(v) for k, v in wall.items()}
        case = out["cases"]["%d layers" % n_layers] = {"layers": n_layers, "additive_layers": sum(additive), "masked_layers": sum(masked), "wall_ms": w}
        if not unflagged_only:
            sc.enable_timing(True)
            kernel_ms = []
            for step in range(WARMUP + REPS):
                call_layered(100 + step, abi.ACTORS_LAYER_WEIGHTS)
                if step >= WARMUP:
                    kernel_ms.append(sc.layer_weights_info().weights_ms)
            sc.enable_timing(False)
            call_layered(0, abi.ACTORS_LAYER_WEIGHTS)
            i, wi = sc.actor_pose_info(), sc.layer_weights_info()
            case.update({"upload_bytes": i.upload_bytes, "rows": wi.rows, "samples": wi.samples, "cubic_samples": wi.cubic_samples, "table_bytes": wi.table_bytes,
                         "layer_weights_kernel_ms": stats(kernel_ms),
                         "verdict": {"W against U (the cost of the flag)": verdict(w, "U", "W"), "W against H": verdict(w, "H", "W")}})
            if n_layers == 2:
                case["verdict"]["W against B (pose_actors_blended)"] = verdict(w, "B", "W")
        print("%d layers" % n_layers + "".join("   %s %8.3f (%.3f - %.3f) ms" % (k, w[k]["median"], w[k]["min"], w[k]["max"]) for k in names) + "   " +
              "; ".join("%s: %s" % kv for kv in case.get("verdict", {}).items()), flush=True)

    if not unflagged_only:                                    # K: the two kernels alone on the same one-layer cubic rows
        one = rt.LayeredActorArgs([([(ids[1], 0.0, 1.0, "override", None, 0.0)], None, None, 0) for a in range(actors)], items)
        plain = rt.ActorArgs([(ids[1], 0.0, None, None, 0) for a in range(actors)], items)
        sc.enable_timing(True)
        ms = {"clip_layer_weights_kernel": [], "clip_spline_weights_kernel": []}
        for step in range(WARMUP + REPS):
            for a in range(actors):
                one.layers[a].time_seconds = plain.actors[a].time_seconds = t_of(step, a, 0)
            check(L.sr_scene_pose_actors_layered(sc._h, one.actors, C.c_uint32(actors), one.items, C.c_uint32(actors), None, C.c_uint32(abi.ACTORS_LAYER_WEIGHTS), None))
            k_new = sc.layer_weights_info().weights_ms
            check(L.sr_scene_pose_actors(sc._h, plain.actors, C.c_uint32(actors), plain.items, C.c_uint32(actors), None, C.c_uint32(0), None))
            k_old, rows = sc.spline_pose_info().spline_weights_ms, sc.spline_pose_info().spline_weight_rows
            assert rows == actors
            if step >= WARMUP:
                ms["clip_layer_weights_kernel"].append(k_new); ms["clip_spline_weights_kernel"].append(k_old)
        sc.enable_timing(False)
        k = {name: stats(v) for name, v in ms.items()}
        out["one_layer_cubic_rows_kernel_ms"] = dict(k, verdict=verdict(k, "clip_spline_weights_kernel", "clip_layer_weights_kernel"))
        print("K" + "".join("   %s %.4f (%.4f - %.4f) ms" % (name, v["median"], v["min"], v["max"]) for name, v in k.items()) + "   " + out["one_layer_cubic_rows_kernel_ms"]["verdict"], flush=True)
    sc.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_layer_weights.json"))
    ap.add_argument("--parent-lib", help="a build of the parent commit: U alone is measured on it too, in a process of its own")
    ap.add_argument("--unflagged-only", action="store_true", help="only U (for another build's library, which need not know the flag)")
    args = ap.parse_args()
    result = {"what": "one step of a crowd of morphed layer stacks (evaluation + posing): U sr_scene_pose_actors_layered, W the same with SR_ACTORS_LAYER_WEIGHTS, "
                      "H sr_clip_weights_layers_host per item + sr_scene_pose_meshes, B sr_scene_pose_actors_blended; wall clock milliseconds", "reps": REPS, "warmup": WARMUP}
    with tempfile.TemporaryDirectory() as tmp:
        result.update(measure(tmp, args.unflagged_only))
    if args.parent_lib:                                        # U alone, a process per library: like with like
        alone = {}
        for label, path in (("this_library", None), ("parent_library", args.parent_lib)):
            with tempfile.TemporaryDirectory() as tmp:
                side = os.path.join(tmp, "alone.json")
                env = dict(os.environ)
                env.pop("SUNRAY_HIP_LIB", None)
                if path:
                    env["SUNRAY_HIP_LIB"] = os.path.abspath(path)
                subprocess.check_call([sys.executable, os.path.abspath(__file__), "--unflagged-only", "--out", side], env=env)
                alone[label] = {name: case["wall_ms"]["U"] for name, case in json.load(open(side))["cases"].items()}
        result["U_alone"] = alone
        for name, u in alone["parent_library"].items():
            mine = alone["this_library"][name]
            result["cases"][name]["verdict"]["U alone against the parent library's U alone"] = "ranges overlap" if u["min"] <= mine["max"] and mine["min"] <= u["max"] else "ranges apart"
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(args.out)


if __name__ == "__main__":
    main()
