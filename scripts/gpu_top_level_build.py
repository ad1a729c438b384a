"""Top-level build of the two-level form, host path against device path (sr_scene_set_top_level_build).

Build time: sr_scene_set_instances with a changed list, wall clock around the call (arrays prepared beforehand) plus the
records / tree split of sr_scene_top_level_info, median and min-max of 20 calls after 3 warm-ups, for 1 000 .. 1 000 000
instances of a 60-triangle mesh and for the 10 000 x 10 080-triangle scene of tests/test_gpu_two_level.py.
Trace cost: both passes of that scene's frame (HIP events of the library) on the host-built and on the device-built top level.

  python scripts/gpu_top_level_build.py [--out profiles/top_level_build.json] [--label NAME] [--counts N,N,...]

runs every step in a fresh child process under its own time limit and stops at the first one that fails. A library without the
device path (SUNRAY_HIP_LIB pointing at an older build) is measured in HOST mode only; --label keeps its figures apart
(e.g. --label parent) in the same output file; --counts measures those instance counts only and adds them to it."""
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COUNTS = (1000, 2048, 4096, 10000, 100000, 1000000)
BIG = "10000x10080"
REPS, WARMUP = 20, 3


def transforms(n, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    ang = rng.uniform(0, 2 * np.pi, n)
    s = rng.uniform(0.2, 0.5, n)
    side = 60.0 * max(1.0, (n / 10000.0) ** (1.0 / 3.0))          # the density of the 10 000-instance scene at every count
    xf = np.zeros((n, 12), dtype=np.float32)
    xf[:, 0] = s * np.cos(ang); xf[:, 2] = s * np.sin(ang); xf[:, 5] = s; xf[:, 8] = -s * np.sin(ang); xf[:, 10] = s * np.cos(ang)
    xf[:, 3] = rng.uniform(-side, side, n); xf[:, 7] = rng.uniform(0.3, 0.3 + side / 10.0, n); xf[:, 11] = rng.uniform(-side, side, n)
    return xf


def has_device_path():
    from sunray_amd._lib import lib
    return hasattr(lib(), "sr_scene_set_top_level_build")


def make_scene(what, mode):
    """-> (scene, keys, counts, [transform array A, B]): a standing two-level scene and two lists to alternate between."""
    import numpy as np
    from sunray_amd import abi, runtime as rt, scenes
    sc = rt.Scene(0, instancing="two_level")
    if has_device_path():
        sc.set_top_level_build(mode)
    if what == BIG:
        n = 10000
        v, idx = scenes.uv_sphere(1.0, 72, 71)
        gv, gi = scenes.quad((-80, 0, -80), (-80, 0, 80), (80, 0, 80), (80, 0, -80), (0, 1, 0))
        lv, li = scenes.quad((-1, 0, -1), (1, 0, -1), (1, 0, 1), (-1, 0, 1), (0, -1, 0))
        sc.add_mesh(1, v, idx, abi.material(base_color=(0.6, 0.5, 0.4, 1.0), roughness=0.6))
        sc.add_mesh(2, gv, gi, abi.material(base_color=(0.7, 0.7, 0.7, 1.0), roughness=0.8))
        sc.add_mesh(3, lv, li, abi.material(base_color=(1, 1, 1, 1), emissive_factor=(1, 1, 1), emissive_strength=30.0))
        rest = np.array([scenes.translate(0, 0, 0)] + [scenes.translate(20.0 * np.cos(k), 25.0, 20.0 * np.sin(k), 6.0) for k in range(6)], dtype=np.float32).reshape(7, 12)
        keys, counts = np.array([1, 2, 3], dtype=np.uint64), np.array([n, 1, 6], dtype=np.uint32)
    else:
        n = int(what)
        v, idx = scenes.uv_sphere(1.0, 6, 6)
        sc.add_mesh(1, v, idx, abi.material())
        rest = np.zeros((0, 12), dtype=np.float32)
        keys, counts = np.array([1], dtype=np.uint64), np.array([n], dtype=np.uint32)
    a = transforms(n, 3)
    b = a.copy()
    b[::2, 7] += np.float32(0.5)
    return sc, keys, counts, [np.ascontiguousarray(np.concatenate([x, rest])) for x in (a, b)]


def set_list(sc, keys, counts, xf):
    from sunray_amd._lib import check, lib
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    t0 = time.perf_counter()
    check(lib().sr_scene_set_instances(sc._h, p(keys), p(counts), C.c_uint32(len(keys)), p(xf)))
    return (time.perf_counter() - t0) * 1e3


def step_build(what, mode):
    import numpy as np
    sc, keys, counts, lists = make_scene(what, mode)
    set_list(sc, keys, counts, lists[0])                           # the quality build
    wall, rec, tree = [], [], []
    for k in range(WARMUP + REPS):
        ms = set_list(sc, keys, counts, lists[(k + 1) & 1])
        if k < WARMUP:
            continue
        wall.append(ms)
        if has_device_path():
            info = sc.top_level_info()
            assert info.on_device == (1 if mode == "device" else 0), "mode %s, but on_device %d (reason %d)" % (mode, info.on_device, info.reason)
            rec.append(info.records_ms); tree.append(info.tree_ms)
    out = {"wall_ms_median": float(np.median(wall)), "wall_ms_min": float(np.min(wall)), "wall_ms_max": float(np.max(wall)), "calls": REPS}
    if rec:
        out.update({"records_ms_median": float(np.median(rec)), "tree_ms_median": float(np.median(tree)), "top_level_nodes": int(sc.top_level_info().n_nodes),
                    "top_level_stack": int(sc.top_level_info().max_stack)})
    return out


def step_trace(mode):
    import numpy as np
    from sunray_amd import abi, runtime as rt, scenes
    sc, keys, counts, lists = make_scene(BIG, mode)
    set_list(sc, keys, counts, lists[0])
    set_list(sc, keys, counts, lists[1])                           # the changed list: built by `mode`
    assert sc.top_level_info().on_device == (1 if mode == "device" else 0)
    out = {"top_level_nodes": int(sc.top_level_info().n_nodes)}
    cfg = abi.SrTraceConfig.reference()
    sc.enable_timing(True)
    for W, H in ((640, 360), (1920, 1080)):
        fr = rt.DeviceFrame(W, H, scenes.white_noise_rgba8())
        prev, t = None, []
        for f in range(10):
            m = rt.camera_matrices((0.0, 30.0, 95.0), (0.0, 2.0, 0.0), 45.0, W, H, prev)
            prev = list(m.view_proj)
            sc.trace_ris(fr, m, f, cfg); sc.trace_final(fr, m, f, cfg)
            t.append((sc.read_timing(0)[0], sc.read_timing(1)[0]))
        t = np.array(t[2:])
        out["%dx%d" % (W, H)] = {"ris_ms": float(t[:, 0].mean()), "final_ms": float(t[:, 1].mean()), "frame_ms": float(t.sum(axis=1).mean()), "frames": len(t)}
    return out


def run_step(args, limit):
    """One step in a fresh process under its own time limit; its JSON result is the last line it prints."""
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step"] + args
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    if r.returncode != 0:
        print("step %s ended with status %d: stopping here" % (" ".join(args), r.returncode), flush=True)
        sys.exit(r.returncode)
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    argv = sys.argv[1:]
    if argv[:1] == ["--step"]:
        res = step_build(argv[2], argv[3]) if argv[1] == "build" else step_trace(argv[2])
        print(json.dumps(res))
        return
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "top_level_build.json")
    label = argv[argv.index("--label") + 1] if "--label" in argv else "this"
    modes = ("host", "device") if has_device_path() else ("host",)
    doc = json.load(open(out_path)) if os.path.exists(out_path) else {}
    doc["workload"] = ("sr_scene_set_instances with a changed list on a standing two-level scene; N instances of a 60-triangle mesh, and 10 000 instances of a "
                       "10 080-triangle mesh + ground + 6 lamps; median (min-max) of %d calls after %d warm-ups, wall clock around the call" % (REPS, WARMUP))
    res = doc.setdefault(label, {})

    def save():                                                    # after every step: a later failure keeps what was measured
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")
    only = argv[argv.index("--counts") + 1].split(",") if "--counts" in argv else None
    for what in only or [str(c) for c in COUNTS] + [BIG]:
        for mode in modes:
            r = run_step(["build", what, mode], 300)
            res.setdefault("build", {}).setdefault(what, {})[mode] = r
            save()
            print("%-12s %-6s %9.3f ms (%.3f - %.3f)%s" % (what, mode, r["wall_ms_median"], r["wall_ms_min"], r["wall_ms_max"],
                                                           "  records %.3f tree %.3f" % (r["records_ms_median"], r["tree_ms_median"]) if "tree_ms_median" in r else ""), flush=True)
    if len(modes) == 2 and not only:
        for mode in modes:
            r = run_step(["trace", mode], 300)
            res.setdefault("trace_10000x10080", {})[mode + "_built_top_level"] = r
            save()
            print("trace, %s-built top level: %s" % (mode, json.dumps(r)), flush=True)


if __name__ == "__main__":
    main()
