"""Cost of the ninth step of an animated mesh in the two-level form: the sr_scene_set_instances that applies a forced
SR_OP_FAST_BUILD to updatable meshes, with the mesh trees built on the host (binned SAH + re-upload of every mesh's records: the
only path there was before sr_scene_set_mesh_tree_build) against the device build (srk_blas_build).

  step CASE MODE   one such step (update_mesh + force_next_op(FAST_BUILD) + set_instances), MODE = host | device: wall clock of
                   set_instances with the event timing off, then, with it on, the split sr_scene_mesh_update_info /
                   sr_scene_mesh_tree_info / sr_scene_top_level_info report: host tree build, device tree build, top-level build
  quality          device time of one 1080p RIS + final frame on the 250 k sphere after a device build, against the same frame
                   after a host SAH build of the same vertices (recorded, no bound: the settle rebuild restores the SAH tree);
                   where the 250 k sphere's device tree is refused for depth, the largest sphere the device takes stands in

Cases: one deforming sphere of 1 k, 4 k, 21 k, 65 k, 250 k and 1 M triangles (four instances, over a ground quad), and 100 deforming spheres
of 1 k triangles each, all at their ninth update. Median (min-max) of 20 calls after 3 warm-ups, every step in a fresh child
process under its own time limit; stops at the first step that fails.

  python scripts/gpu_mesh_tree_build.py [--out profiles/mesh_tree_build.json] [--label NAME] [--only CASE] [--leg rebalance | batch]

--leg rebalance (-> profiles/mesh_tree_rebalance.json): the device steps run under SR_HEIGHT_BOUND_REBALANCE (MODE = rebalance:
a tree taller than 26 entries is made to fit on the device instead of going to the host) and record height before / after and what
was rebuilt; the threshold derived is the one SR_MESH_TREE_BUILD_AUTO uses under that switch (kBlasDeviceMinTrisBounded).

--leg batch (-> profiles/mesh_tree_batch.json): the small-mesh cases 1k, 4k, 100x1k, 100x4k and 1000x256, each on the host, on the
device per mesh (MODE = device) and on the device through the batched build (MODE = batch: sr_scene_set_mesh_tree_batch, one launch,
a workgroup per mesh); the batched steps record how many meshes the batch built, handed on, and in how many launches. The claim it
tests: batched beats both the host and the parent commit by more than the two spreads combined (`batch_verdict` per case).

A library without sr_scene_set_mesh_tree_build (SUNRAY_HIP_LIB pointing at a build of an older commit) runs the host steps only;
--label keeps its figures apart (e.g. --label parent) in the same output file. With the labels `this` and `parent` both present
the script derives the threshold of SR_MESH_TREE_BUILD_AUTO: the smallest measured single-mesh size at which the device beats both
the host and the parent by more than the two spreads combined, rounded up to a power of two."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gpu_mesh_refit as base  # noqa: E402  (the scenes, the statistics and the timed set_instances of the refit measurement)

REPS, WARMUP = base.REPS, base.WARMUP
base.CASES["4k"] = (64, 33, 1)
base.CASES["65k"] = (256, 129, 1)
base.CASES["100x4k"] = (64, 33, 100)
base.CASES["1000x256"] = (16, 9, 1000)
ORDER = ["1k", "4k", "21k", "65k", "250k", "1m", "100x1k"]
BATCH_ORDER = ["1k", "4k", "100x1k", "100x4k", "1000x256"]


def has_tree_build():
    from sunray_amd._lib import lib
    return hasattr(lib(), "sr_scene_set_mesh_tree_build")


def has_batch():
    from sunray_amd._lib import lib
    return hasattr(lib(), "sr_scene_set_mesh_tree_batch")


def has_height_bound():
    from sunray_amd._lib import lib
    return hasattr(lib(), "sr_scene_set_tree_height_bound")


def tree_info(sc):
    import ctypes as C
    from sunray_amd import abi
    from sunray_amd._lib import check, lib
    info = abi.SrMeshTreeInfo()
    check(lib().sr_scene_mesh_tree_info(sc._h, C.byref(info)))
    return info


def scene_for(case, mode):
    from sunray_amd import abi, runtime as rt
    desc, keys = base.make(case)
    sc = rt.Scene(0, instancing="two_level").load(desc)
    for k in keys:
        sc.set_mesh_build_type(k, abi.BUILD_RAPIDLY_CHANGING)
    if has_tree_build():
        sc.set_mesh_tree_build("device" if mode in ("rebalance", "batch") else mode)
        if mode == "batch":
            sc.set_mesh_tree_batch("on")
        if mode == "rebalance":
            sc.set_tree_height_bound("rebalance")
    else:
        assert mode == "host"
    return desc, keys, sc


def step_case(case, mode):
    from sunray_amd import abi, scenes
    from sunray_amd.runtime import _instance_arrays
    desc, keys, sc = scene_for(case, mode)
    m = desc.meshes[0]
    verts = [scenes.deform_vertices(m.vertices, m.indices, ph) for ph in (1.0, 2.0)]       # every sphere takes the same two poses
    arrays = _instance_arrays(desc.instances)
    wall, rows = [], []
    for timing in (False, True):          # wall clock with the event timing off, as a renderer runs it; then the split
        sc.enable_timing(timing)
        for k in range(WARMUP + REPS):
            for key in keys:
                sc.update_mesh(key, verts[k & 1])
            sc.force_next_op(abi.OP_FAST_BUILD)
            t_set = base.set_list(sc, arrays)
            i, tl = sc.mesh_update_info(), sc.top_level_info()
            assert sc.two_level() and (i.blas_refitted, i.blas_rebuilt) == (0, len(keys)), (i.blas_refitted, i.blas_rebuilt)
            dev_ms = batch_ms = 0.0
            if has_tree_build():
                ti = tree_info(sc)
                refused = mode != "host" and ti.reason == abi.MESH_TREE_HOST_STACK_BUDGET      # deeper than a mesh tree may be: the host took over
                assert (ti.built_on_device, ti.built_on_host) == ((len(keys), 0) if mode != "host" and not refused else (0, len(keys))), (ti.built_on_device, ti.built_on_host, ti.reason)
                dev_ms = ti.device_build_ms
            if mode == "batch":
                bi = sc.mesh_tree_batch_info()
                assert bi.batched + bi.passed_on == len(keys) and bi.launches >= 1, (bi.batched, bi.passed_on, bi.launches)
                batch_ms = bi.batch_ms
            if k < WARMUP:
                continue
            if not timing:
                wall.append(t_set)
            else:
                rows.append((i.blas_build_ms, dev_ms, tl.build_ms, batch_ms))
    out = {"set_instances_ms": base.stats(wall)}
    out.update({n: base.stats([r[j] for r in rows]) for j, n in enumerate(("host_tree_build_ms", "device_tree_build_ms", "top_level_ms"))})
    if mode == "batch":
        bi = sc.mesh_tree_batch_info()
        out["batch_ms"] = base.stats([r[3] for r in rows])
        out["batched"], out["passed_on"], out["launches"] = int(bi.batched), int(bi.passed_on), int(bi.launches)
    out["mesh_triangles"], out["meshes"], out["calls"] = len(m.indices) // 3, len(keys), REPS
    if has_tree_build() and mode != "host":
        ti = tree_info(sc)
        out["built_on_device"], out["host_reason"] = int(ti.built_on_device), int(ti.reason)
        if ti.built_on_device:
            out["device_tree_nodes"], out["device_tree_stack"] = int(ti.n_nodes), int(ti.max_stack)
        if mode == "rebalance":           # of the last mesh built
            hi = sc.tree_height_info(abi.TREE_KIND_MESH)
            out.update(height_before=int(hi.height_before), height_after=int(hi.height_after), subtrees_rebuilt=int(hi.subtrees_rebuilt),
                       prims_rebuilt=int(hi.prims_rebuilt), cap=int(hi.cap))
    return out


def step_quality(case, mode="device"):
    from sunray_amd import abi, runtime as rt, scenes
    from sunray_amd.runtime import _instance_arrays
    desc, keys, sc = scene_for(case, mode)
    m = desc.meshes[0]
    arrays = _instance_arrays(desc.instances)
    W, H = 1920, 1080
    fr = rt.DeviceFrame(W, H, scenes.white_noise_rgba8())

    def frame_ms(scene):
        scene.enable_timing(True)
        prev, t = None, []
        for f in range(8):
            mat = rt.camera_matrices(desc.camera_pos, desc.camera_target, desc.fov_y, W, H, prev)
            prev = list(mat.view_proj)
            scene.trace_ris(fr, mat, f); scene.trace_final(fr, mat, f)
            t.append(scene.read_timing(0)[0] + scene.read_timing(1)[0])
        scene.enable_timing(False)
        return base.stats(t[3:])
    v = scenes.deform_vertices(m.vertices, m.indices, 1.0)      # the first pose of the timed steps
    sc.update_mesh(keys[0], v)
    sc.force_next_op(abi.OP_FAST_BUILD)
    base.set_list(sc, arrays)
    ti = tree_info(sc)
    assert (ti.built_on_device, ti.built_on_host) == (1, 0)
    built = frame_ms(sc)
    probe = rt.Scene(0, instancing="two_level").load(scenes.with_mesh_vertices(desc, keys[0], v))     # a host SAH build of the same vertices
    fresh = frame_ms(probe)
    nodes_host = len(probe.read_mesh_tree(keys[0])["nodes"])
    probe.close()
    return {"extent": "%dx%d" % (W, H), "mesh_triangles": len(m.indices) // 3, "device_built_frame_ms": built, "host_sah_frame_ms": fresh,
            "device_tree_nodes": int(ti.n_nodes), "host_tree_nodes": nodes_host}


def run_step(args, limit):
    """One step in a fresh process under its own time limit; its JSON result is the last line it prints."""
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step"] + args
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    if r.returncode != 0:
        print("step %s ended with status %d: stopping here" % (" ".join(args), r.returncode), flush=True)
        sys.exit(r.returncode)
    return json.loads(r.stdout.strip().splitlines()[-1])


def derive_threshold(doc, device="device"):
    """-> (threshold or None, text): the rule kTlDeviceMinBoxes was set by, over the single-mesh cases in ascending size."""
    this, parent = doc.get("this", {}), doc.get("parent", {})
    this = {c: dict(v, device=v[device]) if device in v else {k: x for k, x in v.items() if k != "device"} for c, v in this.items() if isinstance(v, dict)}
    spread = lambda s: s["max"] - s["min"]      # noqa: E731
    for case in ORDER[:-1]:
        try:
            h, d, p = (x["set_instances_ms"] for x in (this[case]["host"], this[case]["device"], parent[case]["host"]))
        except KeyError:
            continue
        if not this[case]["device"].get("built_on_device"):
            continue                                  # refused for depth: that step timed the host
        if h["median"] - d["median"] > spread(h) + spread(d) and p["median"] - d["median"] > spread(p) + spread(d):
            n = this[case]["device"]["mesh_triangles"]
            t = 1 << (n - 1).bit_length()
            if not any(this[c]["device"].get("built_on_device") and this[c]["device"]["mesh_triangles"] >= t for c in ORDER[:-1] if "device" in this.get(c, {})):
                return None, ("device beats host and parent by more than the combined spreads at %d triangles, which rounds up to %d, and no measured size "
                              "from there on is built on the device (refused for depth): no size qualifies, auto mode stays on the host" % (n, t))
            return t, "device beats host and parent by more than the combined spreads from %d triangles on" % n
    return None, "no measured size qualifies: auto mode stays on the host"


def batch_verdicts(doc):
    """-> {case: text}: whether the batched step beats the host, the parent commit's host and the per-mesh device step by more than
    the two spreads of 20 calls combined."""
    this, parent = doc.get("this", {}), doc.get("parent", {})
    spread = lambda s: s["max"] - s["min"]      # noqa: E731
    out = {}
    for case in BATCH_ORDER:
        try:
            b = this[case]["batch"]["set_instances_ms"]
        except KeyError:
            continue
        said = []
        for name, other in (("host", this.get(case, {}).get("host")), ("parent", parent.get(case, {}).get("host")), ("device per mesh", this.get(case, {}).get("device"))):
            if not other:
                said.append("%s: not measured" % name)
                continue
            o = other["set_instances_ms"]
            gap, both = o["median"] - b["median"], spread(o) + spread(b)
            said.append("%s: %s (%.3g against %.3g ms, spreads %.3g)" % (name, "wins" if gap > both else "loses" if -gap > both else "within the spreads", b["median"], o["median"], both))
        out[case] = "; ".join(said)
    return out


def main():
    argv = sys.argv[1:]
    if argv[:1] == ["--step"]:
        print(json.dumps(step_quality(*argv[2:4]) if argv[1] == "quality" else step_case(argv[1], argv[2])))
        return
    leg = argv[argv.index("--leg") + 1] if "--leg" in argv else ""
    device = "rebalance" if leg == "rebalance" else "device"
    default_out = {"rebalance": "mesh_tree_rebalance.json", "batch": "mesh_tree_batch.json"}.get(leg, "mesh_tree_build.json")
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", default_out)
    label = argv[argv.index("--label") + 1] if "--label" in argv else "this"
    doc = json.load(open(out_path)) if os.path.exists(out_path) else {}
    doc["workload"] = ("two-level form, sr_scene_set_instances after sr_scene_update_mesh + a forced SR_OP_FAST_BUILD of one deforming sphere (four instances) "
                       "or of 100 or 1000 spheres; median (min-max) of %d calls after %d warm-ups, wall clock with the event timing off, the split with it on" % (REPS, WARMUP))
    res = doc.setdefault(label, {})

    def save():                                                    # after every step: a later failure keeps what was measured
        if leg == "batch":
            doc["batch_verdict"] = batch_verdicts(doc)
        else:
            doc["auto_threshold"], doc["auto_threshold_rule"] = derive_threshold(doc, device)
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")
    steps = []
    on_device = has_tree_build() and (device == "device" or has_height_bound())      # an older library runs the host steps only
    for case in (BATCH_ORDER if leg == "batch" else ORDER):
        steps += [[case, "host"]] + ([[case, device]] if on_device else []) + ([[case, "batch"]] if leg == "batch" and on_device and has_batch() else [])
    if on_device and leg != "batch":
        steps.append(["quality"])
    if "--only" in argv:
        steps = [x for x in steps if x[0] == argv[argv.index("--only") + 1]]
    for args in steps:
        if args == ["quality"]:         # on the 250 k sphere, or the largest measured sphere whose device tree fits the stack budget
            taken = [c for c in ORDER[:-1] if res.get(c, {}).get(device, {}).get("built_on_device")]
            if not taken:
                continue
            r = run_step(["quality", "250k" if "250k" in taken else taken[-1], device], 300)
        else:
            r = run_step(args, 300)
        node = res
        for a in args[:-1]:
            node = node.setdefault(a, {})
        node[args[-1]] = r
        save()
        print("%-20s %s" % (" ".join(args), json.dumps({k: (round(v["median"], 3) if isinstance(v, dict) and "median" in v else v) for k, v in r.items()})), flush=True)


if __name__ == "__main__":
    main()
