"""Frame time of the multi-device Renderer on the bench scene (1M triangles, 1920x1080), two frames in flight.

  python scripts/gpu_multi_renderer_frames.py                      1 slot and 2 / 4 rehearsal slots (all on device 0), and
                                                                   1 / 2 / 4 / 8 real devices where that many are visible
  python scripts/gpu_multi_renderer_frames.py --slots 4 --frames 20 --no-json
                                                                   one configuration, for a run under
                                                                   rocprofv3 --kernel-trace --stats -d DIR -- python ...
  python scripts/gpu_multi_renderer_frames.py --kernel-stats DIR --slots 4 --frames 20
                                                                   adds the per-frame time of strip_pack / strip_unpack /
                                                                   history_reach_check from that run's *kernel_stats.csv

Results go to profiles/multi_renderer_frames.json (merged with what is there). Whatever was not run stays "not measured".
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "multi_renderer_frames.json")
KERNELS = ("strip_pack_kernel", "strip_unpack_kernel", "history_reach_check_kernel")


def ms_per_frame(devices, frames, warmup=6):
    from sunray_amd import runtime as rt, scenes
    desc = scenes.heightfield(708)
    r = rt.Renderer((1920, 1080)) if devices is None else rt.Renderer((1920, 1080), devices=devices)
    for m in desc.meshes:
        r.load_mesh(m.key, m.vertices, m.indices, m.material)
    cam = (desc.camera_pos, desc.camera_target, desc.fov_y)
    for _ in range(warmup):
        r.wait_frame(r.render(cam, desc.instances))
    t0 = time.perf_counter()
    prev = None
    for _ in range(frames):
        f = r.render(cam, desc.instances)
        if prev is not None:
            r.wait_frame(prev)
        prev = f
    r.wait_frame(prev)
    dt = (time.perf_counter() - t0) / frames * 1e3
    overflow = r.history_overflow()
    r.close()
    return dt, overflow


def kernel_stats(directory, frames, warmup=6):
    """{kernel: ms per frame} from rocprofv3's kernel statistics (TotalDurationNs over every launch of the run)."""
    files = glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise SystemExit("no *kernel_stats.csv under %s" % directory)
    out = {k: 0.0 for k in KERNELS}
    for row in csv.DictReader(open(files[0])):
        for k in KERNELS:
            if k in row.get("Name", ""):
                out[k] += float(row["TotalDurationNs"]) / 1e6 / (frames + warmup)
    return out


def merge(update):
    data = json.load(open(OUT)) if os.path.exists(OUT) else {}
    data.update(update)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(update, indent=1, sort_keys=True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--slots", type=int, default=0, help="one rehearsal configuration only (0 = the whole sweep)")
    ap.add_argument("--no-json", action="store_true")
    ap.add_argument("--kernel-stats", default=None)
    a = ap.parse_args()
    if a.kernel_stats:
        ks = kernel_stats(a.kernel_stats, a.frames)
        merge({"kernel_ms_per_frame_%d_rehearsal_slots" % a.slots: ks})
        return
    import torch
    if a.slots:
        dt, ov = ms_per_frame([0] * a.slots if a.slots > 1 else None, a.frames)
        print("%d slot(s): %.3f ms/frame, history overflow %d" % (a.slots, dt, ov))
        if not a.no_json:
            merge({"rehearsal_ms_per_frame": {str(a.slots): dt}})
        return
    res = {"rehearsal_ms_per_frame": {}, "devices_ms_per_frame": {}, "visible_devices": torch.cuda.device_count(),
           "frames": a.frames, "workload": "heightfield(708), 1920x1080, two frames in flight, column strips, equal cut"}
    for n in (1, 2, 4):
        dt, ov = ms_per_frame(None if n == 1 else [0] * n, a.frames)
        assert ov == 0, "history overflow %d with %d slots" % (ov, n)
        res["rehearsal_ms_per_frame"][str(n)] = dt
    for n in (1, 2, 4, 8):
        if torch.cuda.device_count() < n:
            res["devices_ms_per_frame"][str(n)] = "not measured (%d visible devices)" % torch.cuda.device_count()
            continue
        dt, ov = ms_per_frame(None if n == 1 else list(range(n)), a.frames)
        assert ov == 0
        res["devices_ms_per_frame"][str(n)] = dt
    if not a.no_json:
        merge(res)


if __name__ == "__main__":
    main()
