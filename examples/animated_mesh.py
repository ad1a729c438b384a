"""A deforming mesh through Renderer.update_mesh (the reference's Blas::update, acceleration_structure/blas.rs:285-310): the
Cornell box's sphere ripples for a number of frames; every frame replaces the sphere's vertices in place and renders, the
acceleration structure is updated in place (re-flatten + refit) or, after the update budget, fast-rebuilt on the device, as the
heuristic picks; it is never torn down and rebuilt on the host. The sphere is declared RapidlyChanging (the reference's
BuildType of a BLAS that is built with ALLOW_UPDATE): where the scene stands in the two-level form (SR_INSTANCING=two_level, or a
scene large enough for the automatic choice) its own tree is then refitted on the device as well. Writes the last frame as a PNG.

    python examples/animated_mesh.py [out.png] [--frames 24] [--size 640x480] [--height-bound rebalance] [--device-vertices [--recompute-normals] [--device-lights]]

--height-bound rebalance: a device fast build whose tree comes out taller than the traversal stack allows is rebalanced on the
device instead of going to the host builder (Renderer.set_tree_height_bound; the default, refuse, is the library's).

--device-vertices: the sphere is deformed with torch ops on the GPU and handed over as a tensor (Renderer.update_mesh_device):
the vertices never visit the host, the library validates them on the device and copies device to device.

--recompute-normals (with --device-vertices): the ripple hands over POSITIONS only, a [n, 3] float32 tensor, and the library
recomputes the sphere's normals and tangents on the device from them (Renderer.set_mesh_frame / update_mesh_positions): the
rippling sphere is shaded with the normals of its own surface.

--device-lights (with --device-vertices): the ceiling light ripples too, and the frame's light table is built on the device
(Renderer.set_light_table_build("device")): the emissive mesh's vertices never visit the host either.

Needs a GPU: the product path has no CPU fallback.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from png import write_png  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default="animated.png")
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--size", default="640x480")
    ap.add_argument("--height-bound", choices=["refuse", "rebalance"], default="refuse")
    ap.add_argument("--device-vertices", action="store_true")
    ap.add_argument("--device-lights", action="store_true")
    ap.add_argument("--recompute-normals", action="store_true")
    args = ap.parse_args()
    if args.recompute_normals and not args.device_vertices:
        ap.error("--recompute-normals goes with --device-vertices")
    if args.device_lights and not args.device_vertices:
        ap.error("--device-lights goes with --device-vertices")
    from sunray_amd import abi, runtime as rt, scenes
    w, h = (int(v) for v in args.size.split("x"))
    desc = scenes.cornell_box()
    sphere = next(m for m in desc.meshes if m.key == 7)
    r = rt.Renderer((w, h))
    r.set_tree_height_bound(args.height_bound)
    if args.device_lights:
        r.set_light_table_build("device")
    for m in desc.meshes:
        r.load_mesh(m.key, m.vertices, m.indices, m.material)
    r.set_mesh_build_type(sphere.key, abi.BUILD_RAPIDLY_CHANGING)
    if args.recompute_normals:
        r.set_mesh_frame(sphere.key, tangents=True)
    camera = (desc.camera_pos, desc.camera_target, desc.fov_y)
    if args.device_vertices:
        import torch
        rest = torch.from_numpy(sphere.vertices.view("<f4").reshape(len(sphere.vertices), -1).copy()).to("cuda:0")   # [n, 24] floats: 96-byte records
        lamp = next(m for m in desc.meshes if m.key == 6)
        lamp_rest = torch.from_numpy(lamp.vertices.view("<f4").reshape(len(lamp.vertices), -1).copy()).to("cuda:0")
    for f in range(args.frames):
        if f and args.device_lights:
            posed = lamp_rest.clone()
            posed[:, 1] = lamp_rest[:, 1] - 0.05 * (1.0 + torch.sin(lamp_rest[:, 0] * 4.0 + 0.3 * f))      # the light's corners bob below the ceiling
            r.update_mesh_device(lamp.key, posed)
        if f and args.device_vertices:
            # a ripple along the rest normal, computed where the vertices live
            pos, nrm = rest[:, 0:3], rest[:, 4:7]
            wave = 0.08 * torch.sin(9.0 * pos[:, 1:2] + 5.0 * pos[:, 0:1] + 0.25 * f)
        if f and args.recompute_normals:
            r.update_mesh_positions(sphere.key, (pos + wave * nrm).contiguous())      # positions only: the library makes the shading frame
        elif f and args.device_vertices:
            posed = rest.clone()                                                      # whole records: the normals keep their rest direction
            posed[:, 0:3] = pos + wave * nrm
            r.update_mesh_device(sphere.key, posed)
        elif f:
            r.update_mesh(sphere.key, scenes.deform_vertices(sphere.vertices, sphere.indices, 0.25 * f, amplitude=0.08))
        r.wait_frame(r.render(camera, desc.instances))
    image = r.render_to_host_memory(camera, desc.instances)       # lets the temporal accumulation settle on the last pose
    write_png(args.out, image)
    print("You can find your render here: %s" % args.out)


if __name__ == "__main__":
    main()
