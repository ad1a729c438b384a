"""Cost of one step of a crowd whose every actor is a stack of layers, evaluation plus posing, up to the posed vertices and the
instance tables, by the paths of one build:

  H  the host route: per actor one sr_clip_sample_host per sample taken (two for an additive layer), sr_clip_layers_host and
     sr_clip_compose_records_host, then sr_scene_pose_meshes + sr_scene_set_instances
  D  sr_scene_pose_actors_layered (clip_layers_kernel in front of the posing kernel) + sr_scene_set_instances_device
  B  at two layers only: the same crowd through sr_scene_pose_actors_blended (the top layer unmasked for this comparison's D2)
  P, F  the unchanged entry points sr_scene_pose_actors and sr_scene_pose_actors_blended on their own crowd: run the script a second
     time with SUNRAY_HIP_LIB naming another build's library and --entry-points-only to compare them across builds

Case: 1 000 actors of a rig of 64 joints (a chain of that many nodes, each turned by a LINEAR rotation channel of 4 keys; one skinned
and one unskinned quad per actor) at 1, 2, 4 and 8 layers. Layer l > 0 is additive where l is even and an override otherwise, and is
masked (a per-node mask that varies) where l % 4 is 1 or 2. Every path is timed at the C entry points with its arguments packed
beforehand. Wall clock, median (min - max) of REPS steps after WARMUP, the paths alternating.

  python scripts/gpu_clip_layers.py [--out profiles/clip_layers.json] [--entry-points-only]
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
ACTORS, JOINTS, LAYER_COUNTS = 1000, 64, (1, 2, 4, 8)


def stats(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1], "n": len(xs)}


def verdict(w, x, y):
    return "%s wins" % y if w[y]["max"] < w[x]["min"] else "%s wins" % x if w[x]["max"] < w[y]["min"] else "ranges overlap"


def measure(tmp, entry_points_only):
    import torch
    from clip_util import crowd, shape_rig
    from sunray_amd import abi, runtime as rt
    from sunray_amd._lib import LIB_PATH, check, lib
    actors, joints = ACTORS, JOINTS
    path = os.path.join(tmp, "rig.glb")
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
    assert list(rows) == list(range(ni))
    duration = clip.info.duration_seconds
    skinned_key = [keys[a][skins.index(0)] for a in range(actors)]
    lkeys, lcounts = np.array([k for k, _ in layout], np.uint64), np.array([c for _, c in layout], np.uint32)
    items = [(skinned_key[a], a, 0, None) for a in range(actors)]
    d_xf = torch.zeros((actors * ni, 12), dtype=torch.float32, device="cuda:0")
    d_ptr = C.c_void_p(d_xf.data_ptr())
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    out = {"library": os.path.basename(os.path.dirname(LIB_PATH)) + "/" + os.path.basename(LIB_PATH), "actors": actors, "joints": joints, "nodes": n_nodes,
           "channels_per_clip": clip.info.n_channels, "cases": {}}

    def t_of(step, a, l):
        return (0.013 * step + 0.11 * l + duration * a / actors) % duration

    def tables_device():
        return L.sr_scene_set_instances_device(sc._h, p(lkeys), p(lcounts), C.c_uint32(len(lkeys)), d_ptr, None)

    # the unchanged entry points
    plain = rt.ActorArgs([(ida, 0.0, None, None, a * ni) for a in range(actors)], items)
    blended = rt.BlendedActorArgs([(ida, 0.0, idb, 0.0, 0.5, None, None, a * ni) for a in range(actors)], items)

    def path_p(step):
        t0 = time.perf_counter()
        for a in range(actors):
            plain.actors[a].time_seconds = t_of(step, a, 0)
        rc = L.sr_scene_pose_actors(sc._h, plain.actors, C.c_uint32(actors), plain.items, C.c_uint32(actors), d_ptr, C.c_uint32(0), None) or tables_device()
        check(rc)
        return (time.perf_counter() - t0) * 1e3

    def path_f(step):
        t0 = time.perf_counter()
        for a in range(actors):
            row = blended.actors[a]
            row.time_seconds, row.time_seconds_b, row.weight = t_of(step, a, 0), t_of(step, a, 1), 0.05 + 0.9 * ((0.07 * step + a / actors) % 1.0)
        rc = L.sr_scene_pose_actors_blended(sc._h, blended.actors, C.c_uint32(actors), blended.items, C.c_uint32(actors), d_ptr, C.c_uint32(0), None) or tables_device()
        check(rc)
        return (time.perf_counter() - t0) * 1e3

    wall = {"P": [], "F": []}
    for step in range(WARMUP + REPS):
        got = {"P": path_p(step), "F": path_f(step)}
        if step >= WARMUP:
            for k, v in got.items():
                wall[k].append(v)
    out["entry_points_wall_ms"] = {k: stats(v) for k, v in wall.items()}
    if entry_points_only:
        sc.close()
        return out

    vary = ((np.arange(n_nodes) * 37 % 101) / 100.0).astype(np.float32)
    mask_id = sc.attach_node_mask(vary)
    jm, xf = np.zeros((actors, joints, 12), np.float32), np.zeros((actors * ni, 12), np.float32)
    jm_at = [C.c_void_p(jm[a].ctypes.data) for a in range(actors)]
    xf_at = [C.c_void_p(xf[a * ni:].ctypes.data) for a in range(actors)]
    pose_rows = (abi.SrPoseItem * actors)()
    for a in range(actors):
        pose_rows[a].key, pose_rows[a].joint_matrices, pose_rows[a].n_joints = skinned_key[a], jm_at[a].value, joints
    for n_layers in LAYER_COUNTS:
        additive = [l > 0 and l % 2 == 0 for l in range(n_layers)]
        masked = [l % 4 in (1, 2) for l in range(n_layers)]
        weight = [1.0 if l == 0 else 0.3 + 0.05 * l for l in range(n_layers)]
        stack = lambda a: [((ida, idb)[l % 2], 0.0, weight[l], "additive" if additive[l] else "override", mask_id if masked[l] else None, 0.0) for l in range(n_layers)]     # noqa: E731
        layered = rt.LayeredActorArgs([(stack(a), None, None, a * ni) for a in range(actors)], items)
        cur = [np.zeros(n_nodes, abi.NODE_TRS) for _ in range(n_layers)]
        ref = [np.zeros(n_nodes, abi.NODE_TRS) for _ in range(n_layers)]
        final = np.zeros(n_nodes, abi.NODE_TRS)
        cp, rp, rules = (C.c_void_p * n_layers)(), (C.c_void_p * n_layers)(), (abi.SrClipLayerRule * n_layers)()
        for l in range(n_layers):
            cp[l], rp[l] = cur[l].ctypes.data, ref[l].ctypes.data if additive[l] else None
            rules[l].weight, rules[l].mode, rules[l].mask = weight[l], abi.LAYER_ADDITIVE if additive[l] else abi.LAYER_OVERRIDE, vary.ctypes.data if masked[l] else None

        def path_h(step):
            t0 = time.perf_counter()
            rc = 0
            for a in range(actors):
                for l in range(n_layers):
                    rc |= L.sr_clip_sample_host(clip._h, C.c_float(t_of(step, a, l)), C.c_void_p(cp[l]))
                    if additive[l]:
                        rc |= L.sr_clip_sample_host(clip._h, C.c_float(t_of(step, a, l + 8)), C.c_void_p(rp[l]))
                rc |= L.sr_clip_layers_host(cp, rp, rules, C.c_uint32(n_layers), C.c_uint32(n_nodes), p(final))
                rc |= L.sr_clip_compose_records_host(clip._h, p(final), None, jm_at[a], xf_at[a], None)
            t1 = time.perf_counter()
            rc |= L.sr_scene_pose_meshes(sc._h, pose_rows, C.c_uint32(actors), None)
            if rc == 0:
                rc = L.sr_scene_set_instances(sc._h, p(lkeys), p(lcounts), C.c_uint32(len(lkeys)), p(xf))
            check(rc)
            return (time.perf_counter() - t0) * 1e3, (t1 - t0) * 1e3

        def path_d(step):
            t0 = time.perf_counter()
            for a in range(actors):
                for l in range(n_layers):
                    row = layered.layers[layered.first_layer[a] + l]
                    row.time_seconds, row.ref_time_seconds = t_of(step, a, l), t_of(step, a, l + 8)
            rc = L.sr_scene_pose_actors_layered(sc._h, layered.actors, C.c_uint32(actors), layered.items, C.c_uint32(actors), d_ptr, C.c_uint32(0), None) or tables_device()
            check(rc)
            return (time.perf_counter() - t0) * 1e3

        names = ["H", "D"] + (["F"] if n_layers == 2 else [])
        wall = {k: [] for k in names + ["H_eval"]}
        for step in range(WARMUP + REPS):
            h, d = path_h(step), path_d(step)
            f = path_f(step) if n_layers == 2 else None
            if step >= WARMUP:
                wall["H"].append(h[0]); wall["H_eval"].append(h[1]); wall["D"].append(d)
                if f is not None:
                    wall["F"].append(f)
        sc.enable_timing(True)
        clip_ms = []
        for step in range(WARMUP + REPS):
            path_d(100 + step)
            if step >= WARMUP:
                clip_ms.append(sc.actor_pose_info().clip_ms)
        sc.enable_timing(False)
        path_d(0)
        i, li = sc.actor_pose_info(), sc.layer_pose_info()
        w = {k: stats(v) for k, v in wall.items()}
        case = out["cases"]["%d layers" % n_layers] = {
            "layers": n_layers, "additive_layers": sum(additive), "masked_layers": sum(masked), "samples_per_actor": n_layers + sum(additive),
            "upload_bytes": i.upload_bytes, "layer_table_bytes": li.layer_table_bytes, "wall_ms": w, "clip_kernel_ms": stats(clip_ms),
            "verdict": {"D against H": verdict(w, "H", "D")}}
        if n_layers == 2:
            case["verdict"]["D against F (pose_actors_blended, an unmasked fade)"] = verdict(w, "F", "D")
        print("%d layers" % n_layers + "".join("   %s %8.3f (%.3f - %.3f) ms" % (k, w[k]["median"], w[k]["min"], w[k]["max"]) for k in names) + "   " +
              "; ".join("%s: %s" % kv for kv in case["verdict"].items()), flush=True)
    sc.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_layers.json"))
    ap.add_argument("--entry-points-only", action="store_true", help="only sr_scene_pose_actors and sr_scene_pose_actors_blended (for another build's library)")
    args = ap.parse_args()
    result = {"what": "one step of a crowd of layer stacks (evaluation + posing + instance tables): H the host route, D sr_scene_pose_actors_layered, "
                      "F sr_scene_pose_actors_blended, P sr_scene_pose_actors; wall clock milliseconds", "reps": REPS, "warmup": WARMUP}
    with tempfile.TemporaryDirectory() as tmp:
        result.update(measure(tmp, args.entry_points_only))
    e = result["entry_points_wall_ms"]
    print("".join("   %s %8.3f (%.3f - %.3f) ms" % (k, e[k]["median"], e[k]["min"], e[k]["max"]) for k in "PF"))
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(args.out)


if __name__ == "__main__":
    main()
