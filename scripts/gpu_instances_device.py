"""A frame's instance transforms taken from device memory (sr_scene_set_instances_device) against the host round trip.

One step of N instances of a 60-triangle mesh whose transforms torch produces on the device, on a standing scene: the two-level
form with the top level built on the device, and the one-level form with a forced in-place update (up to 100 000 instances: the
one-level form flattens N x 60 triangles). Three columns, wall clock around everything the caller has to do, median (min-max) of
20 calls after 3 warm-ups:

  roundtrip  tensor.cpu() + sr_scene_set_instances       (with --label parent and SUNRAY_HIP_LIB: the library before this path)
  device     sr_scene_set_instances_device on the tensor (its kernel's time, SrInstanceUpdateInfo.tables_ms, from five further
             calls with sr_scene_enable_timing on)

  python scripts/gpu_instances_device.py [--out profiles/instances_device.json] [--label NAME] [--counts N,N,...]

runs every step in a fresh child process under its own time limit and stops at the first one that fails. A library without
the device path is measured in the roundtrip column only; --label keeps its figures apart in the same output file."""
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COUNTS = (1000, 10000, 100000, 1000000)
ONE_LEVEL_MAX = 100000
REPS, WARMUP, TIMED = 20, 3, 5
OP_FAST_BUILD, OP_UPDATE = 2, 3


def has_device_path():
    from sunray_amd._lib import lib
    return hasattr(lib(), "sr_scene_set_instances_device")


def base_transforms(n, seed=3):
    """[n, 12] float32 on the device, made there: a rotation about y, a uniform scale, a position in a box of constant density."""
    import math
    import torch
    g = torch.Generator(device="cuda:0").manual_seed(seed)
    u = torch.rand((n, 5), generator=g, device="cuda:0", dtype=torch.float32)
    ang, s = u[:, 0] * (2 * math.pi), 0.2 + 0.3 * u[:, 1]
    side = 60.0 * max(1.0, (n / 10000.0) ** (1.0 / 3.0))
    xf = torch.zeros((n, 12), device="cuda:0", dtype=torch.float32)
    xf[:, 0] = s * torch.cos(ang); xf[:, 2] = s * torch.sin(ang); xf[:, 5] = s; xf[:, 8] = -s * torch.sin(ang); xf[:, 10] = s * torch.cos(ang)
    xf[:, 3] = (2 * u[:, 2] - 1) * side; xf[:, 7] = 0.3 + u[:, 3] * side / 10.0; xf[:, 11] = (2 * u[:, 4] - 1) * side
    return xf


def step(form, n, column):
    import numpy as np
    import torch
    from sunray_amd import abi, runtime as rt, scenes
    from sunray_amd._lib import check, lib
    sc = rt.Scene(0, instancing="two_level" if form == "two_level" else "flat")
    if form == "two_level":
        sc.set_top_level_build("device")
    v, idx = scenes.uv_sphere(1.0, 6, 6)
    sc.add_mesh(1, v, idx, abi.material())
    keys, counts = np.array([1], dtype=np.uint64), np.array([n], dtype=np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    base = base_transforms(n)

    def host_call(xf):
        check(lib().sr_scene_set_instances(sc._h, p(keys), p(counts), C.c_uint32(1), p(xf)))
    if form == "one_level":
        sc.force_next_op(OP_FAST_BUILD)                            # the first structure by the device fast build, not the host's quality build
    host_call(np.ascontiguousarray(base.cpu().numpy()))
    if form == "two_level":
        host_call(np.ascontiguousarray(base.cpu().numpy()))        # standing: from here a changed list is built on the device
    wall, part, kernel = [], [], []
    for k in range(WARMUP + REPS + (TIMED if column == "device" else 0)):
        cur = base.clone()
        cur[:, 7] += 0.5 * (k & 1)                                 # this step's transforms, by torch, on the device
        torch.cuda.synchronize()
        timed = k >= WARMUP + REPS
        if timed and k == WARMUP + REPS:
            sc.enable_timing(True)
        if form == "one_level":
            sc.force_next_op(OP_UPDATE)
        t0 = time.perf_counter()
        if column == "device":
            sc.set_instances_device([(1, n)], cur)
            t1 = t0
        else:
            host = cur.cpu().numpy()
            t1 = time.perf_counter()
            host_call(host)
        t2 = time.perf_counter()
        if column == "device":
            info = sc.instance_update_info()
            assert info.from_device == 1 and info.host_fetches == 0 and info.layout_rebuilt == (1 if k == 0 else 0), (info.host_fetches, info.fetch_reason, info.layout_rebuilt)
            if timed:
                kernel.append(info.tables_ms)
        if form == "two_level":
            assert sc.top_level_info().on_device == 1, sc.top_level_info().reason
        else:
            assert sc.as_state()[1] == OP_UPDATE
        if k >= WARMUP and not timed:
            wall.append((t2 - t0) * 1e3); part.append((t2 - t1) * 1e3)
    out = {"wall_ms_median": float(np.median(wall)), "wall_ms_min": float(np.min(wall)), "wall_ms_max": float(np.max(wall)), "calls": REPS}
    if column == "device":
        out["tables_ms_median"] = float(np.median(kernel))
    else:
        out.update({"set_instances_ms_median": float(np.median(part)), "set_instances_ms_min": float(np.min(part)), "set_instances_ms_max": float(np.max(part))})
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
        print(json.dumps(step(argv[1], int(argv[2]), argv[3])))
        return
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "instances_device.json")
    label = argv[argv.index("--label") + 1] if "--label" in argv else "this"
    columns = ("roundtrip", "device") if has_device_path() else ("roundtrip",)
    doc = json.load(open(out_path)) if os.path.exists(out_path) else {}
    doc["workload"] = ("one step of N instances of a 60-triangle mesh whose transforms torch produces on the device, on a standing scene: two-level form with the top "
                       "level built on the device, one-level form with a forced in-place update; roundtrip = tensor.cpu() + sr_scene_set_instances, device = "
                       "sr_scene_set_instances_device; median (min-max) of %d calls after %d warm-ups, wall clock around the call(s)" % (REPS, WARMUP))
    res = doc.setdefault(label, {})

    def save():                                                    # after every step: a later failure keeps what was measured
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")
    only = [int(c) for c in argv[argv.index("--counts") + 1].split(",")] if "--counts" in argv else None
    for form in ("two_level", "one_level"):
        for n in only or COUNTS:
            if form == "one_level" and n > ONE_LEVEL_MAX:
                continue
            for column in columns:
                r = run_step([form, str(n), column], 240)
                res.setdefault(form, {}).setdefault(str(n), {})[column] = r
                save()
                extra = "  kernel %.3f" % r["tables_ms_median"] if "tables_ms_median" in r else "  set_instances %.3f" % r["set_instances_ms_median"]
                print("%-10s %8d %-9s %9.3f ms (%.3f - %.3f)%s" % (form, n, column, r["wall_ms_median"], r["wall_ms_min"], r["wall_ms_max"], extra), flush=True)


if __name__ == "__main__":
    main()
