"""A rigged glTF file played on the GPU: the loader hands out the rig (skins, JOINTS_0 / WEIGHTS_0) and evaluates the animation,
Renderer.attach_skins gives every skinned mesh its bind pose and influences, and every frame Renderer.pose_scene samples the
animation, skins the meshes with the library's kernel (the posed vertices never visit the host) and returns the instance
transforms for the frame. Writes the last frame as a PNG.

    python examples/skinned_gltf.py [file.glb] [--animation 0] [--frames 48] [--size 640x480] [--out skinned.png] [--device-lights] [--cubicspline]

--device-lights: the frame's light table is built on the device (Renderer.set_light_table_build("device")), so that a skinned
mesh with an emissive material never visits the host either.

--cubicspline: CUBICSPLINE samplers are sampled instead of refused (Gltf.set_cubicspline, before anything is posed):
--animation 1 --cubicspline plays the fixture's "spline" animation.

Default file: tests/golden/skinned_bar.glb. Needs a GPU: the product path has no CPU fallback.
"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from png import write_png  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("file", nargs="?", default=os.path.join(os.path.dirname(HERE), "tests", "golden", "skinned_bar.glb"))
    ap.add_argument("--animation", type=int, default=0)
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--size", default="640x480")
    ap.add_argument("--out", default="skinned.png")
    ap.add_argument("--camera", default="0.8,1.4,7.0,0.8,1.0,0.0,45", help="position, target, vertical field of view in degrees")
    ap.add_argument("--device-lights", action="store_true")
    ap.add_argument("--cubicspline", action="store_true", help="sample CUBICSPLINE animation samplers (Gltf.set_cubicspline) instead of refusing them; animation 1 of the fixture has one")
    ap.add_argument("--batch-trees", action="store_true", help="build the small meshes' trees in one batched device launch when their ninth update asks for a fast build")
    args = ap.parse_args()
    from sunray_amd import runtime as rt
    w, h = (int(v) for v in args.size.split("x"))
    c = [float(v) for v in args.camera.split(",")]
    camera = (tuple(c[0:3]), tuple(c[3:6]), c[6])
    gltf = rt.Gltf(args.file)
    if args.cubicspline:                             # before anything is posed or baked
        gltf.set_cubicspline(True)
    n_skins, n_animations = gltf.rig_counts()
    if not 0 <= args.animation < n_animations:
        sys.exit("%s has %d animation(s); --animation %d is not one of them" % (args.file, n_animations, args.animation))
    name, duration, n_channels, n_ignored = gltf.animation(args.animation)
    print("%s: %d skin(s), animation %d '%s': %.3f s, %d channel(s)%s" % (
        args.file, n_skins, args.animation, name, duration, n_channels, ", %d morph-target channel(s) ignored" % n_ignored if n_ignored else ""))
    r = rt.Renderer((w, h))
    if args.device_lights:
        r.set_light_table_build("device")
    if args.batch_trees:
        r.set_mesh_tree_batch("on")
    loaded = r.load_scene(gltf)
    r.attach_skins(gltf, loaded)
    instances = loaded.instances
    for f in range(args.frames):
        instances = r.pose_scene(gltf, loaded, args.animation, duration * f / max(args.frames - 1, 1))
        r.wait_frame(r.render(camera, instances))
    image = r.render_to_host_memory(camera, instances)       # lets the temporal accumulation settle on the last pose
    write_png(args.out, image)
    print("You can find your render here: %s" % args.out)


if __name__ == "__main__":
    main()
