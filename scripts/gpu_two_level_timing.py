"""ms per frame of the two-level form (kernel variants V & 4) on three scenes, with the harness calls and the content check of
scripts/gpu_config_regression.py, whose table holds one-level rows only:

    python scripts/gpu_two_level_timing.py [label]

Per row: undisturbed device time of the two passes, mean of frames 3..9 (profiles/node_step_diet_config_regression.txt)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from sunray_amd import abi, scenes, runtime as rt
label = sys.argv[1] if len(sys.argv) > 1 else "HEAD"
ref = abi.SrTraceConfig.reference()
for name, d in (("two-level Cornell box", scenes.cornell_box()), ("two-level instanced field 120", scenes.instanced_field(120)), ("two-level heightfield 1M", scenes.heightfield(708))):
    sc = rt.Scene(0, instancing="two_level").load(d)
    assert sc.two_level()
    W, H = 1920, 1080
    fr = rt.DeviceFrame(W, H, scenes.white_noise_rgba8())
    prev = None
    sc.enable_timing(True)
    rows = []
    for f in range(10):
        m = rt.camera_matrices(d.camera_pos, d.camera_target, d.fov_y, W, H, prev)
        prev = list(m.view_proj)
        sc.trace_ris(fr, m, f, ref); sc.trace_final(fr, m, f, ref)
        rows.append((sc.read_timing(0)[0], sc.read_timing(1)[0]))
    sc.enable_timing(False)
    r = np.array(rows[3:])
    crc = int(torch.sum(fr.raw_color.view(torch.int32).to(torch.int64) & 0xFFFF).item()) & 0xFFFFFFFF
    print("%-7s %-32s ris %6.3f + final %6.3f = %6.3f ms | sum16 %08x" % (label, name, r[:, 0].mean(), r[:, 1].mean(), r.mean(axis=0).sum(), crc), flush=True)
    del fr, sc
