"""A swarm of instances whose transforms never visit the host (Renderer.render_device_transforms, the library's
sr_scene_set_instances_device): some thousand small spheres circle above a floor under a few lamps; a few lines of torch move
them on the GPU each frame and hand the [n, 12] tensor over, the library validates it and writes its per-instance tables with
one kernel, and in the two-level form (the default here) the top-level tree is rebuilt on the device too. Writes the last
frame as a PNG.

    python examples/instance_swarm.py [out.png] [--instances 4000] [--frames 24] [--size 640x360] [--one-level]

--one-level: the one-level form instead, where the same call updates the flattened structure in place or fast-rebuilds it on
the device, as the heuristic picks.

Needs a GPU: the product path has no CPU fallback.
"""
import argparse
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from png import write_png  # noqa: E402

BODY, FLOOR, LAMP = 1, 2, 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default="swarm.png")
    ap.add_argument("--instances", type=int, default=4000)
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--size", default="640x360")
    ap.add_argument("--one-level", action="store_true")
    args = ap.parse_args()
    import torch
    from sunray_amd import abi, runtime as rt, scenes
    if not args.one_level:
        os.environ.setdefault("SR_INSTANCING", "two_level")         # read when the renderer creates its scene
        os.environ.setdefault("SR_TL_BUILD", "device")
    w, h = (int(v) for v in args.size.split("x"))
    n = args.instances
    r = rt.Renderer((w, h))
    r.load_mesh(BODY, *scenes.uv_sphere(1.0, 6, 6), abi.material(base_color=(0.8, 0.45, 0.25, 1.0), roughness=0.4))
    r.load_mesh(FLOOR, *scenes.quad((-40, 0, -40), (-40, 0, 40), (40, 0, 40), (40, 0, -40), (0, 1, 0)), abi.material(base_color=(0.7, 0.7, 0.7, 1.0), roughness=0.8))
    r.load_mesh(LAMP, *scenes.quad((-1, 0, -1), (1, 0, -1), (1, 0, 1), (-1, 0, 1), (0, -1, 0)),
                abi.material(base_color=(1, 1, 1, 1), emissive_factor=(1.0, 0.95, 0.85), emissive_strength=40.0))
    layout = [(BODY, n), (FLOOR, 1), (LAMP, 4)]
    camera = ((0.0, 14.0, 34.0), (0.0, 4.0, 0.0), 45.0)
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(5)
    u = torch.rand((n, 4), generator=g, device=dev)
    radius, height, phase, size = 4.0 + 18.0 * u[:, 0], 1.0 + 9.0 * u[:, 1], 2 * math.pi * u[:, 2], 0.15 + 0.25 * u[:, 3]
    fixed = np.stack([scenes.translate(0.0, 0.0, 0.0)] + [scenes.translate(12.0 * math.cos(k * math.pi / 2), 16.0, 12.0 * math.sin(k * math.pi / 2), 3.0) for k in range(4)])
    fixed = torch.from_numpy(fixed).to(dev)                          # the floor and the four lamps stay where they are
    xf = torch.zeros((n + 5, 12), dtype=torch.float32, device=dev)
    xf[n:] = fixed
    for f in range(args.frames):
        # the swarm's step, where the transforms live: every body circles the axis at its own pace and bobs
        ang = phase + 0.02 * f * (30.0 / radius)
        xf[:n, 0] = size; xf[:n, 5] = size; xf[:n, 10] = size
        xf[:n, 3] = radius * torch.cos(ang)
        xf[:n, 7] = height + 0.5 * torch.sin(3.0 * ang)
        xf[:n, 11] = radius * torch.sin(ang)
        r.wait_frame(r.render_device_transforms(camera, layout, xf))
    host = xf.cpu().numpy()
    instances = [(BODY, list(host[:n])), (FLOOR, [host[n]]), (LAMP, list(host[n + 1:]))]
    image = r.render_to_host_memory(camera, instances)              # lets the temporal accumulation settle on the last pose
    write_png(args.out, image)
    print("You can find your render here: %s" % args.out)


if __name__ == "__main__":
    main()
