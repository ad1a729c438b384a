"""A glTF file with morph targets (blend shapes) and a rig played on the GPU: the loader hands out the targets and the rig and
evaluates the animation, Renderer.attach_skins and Renderer.attach_morphs give every mesh its influences and its deltas, and every
frame Renderer.pose_scene samples the joint and the weight channels, blends the targets and then skins the result with the
library's kernels (morph first, then skin; the posed vertices never visit the host) and returns the instance transforms for the
frame. Writes the last frame as a PNG.

    python examples/morph_gltf.py [file.glb] [--animation 0] [--frames 48] [--size 640x480] [--out morph.png] [--device-lights] [--device-clips] [--cubicspline] [--additive-layer ANIM]

--device-lights: the frame's light table is built on the device (Renderer.set_light_table_build("device")), so that a posed mesh
with an emissive material never visits the host either.

--device-clips: the animation is baked once (Gltf.bake_clip) and attached, and every frame is one Renderer.pose_actors: the GPU samples
the joint channels and the weight channels of the clip (ClipWeights), so neither the joint matrices, nor the morph weights, nor the
instance transforms come from host memory. A mesh whose weight channel the loader refuses (CUBICSPLINE) is left unmorphed.

--additive-layer ANIM (with --device-clips): animation ANIM is baked too and played as an additive layer at weight 1, against its
own pose at time 0, on top of --animation (the file's first unless given): every frame is one Renderer.pose_actors_layered with
layer_weights=True, so the morph weights go through the stack as well: a blink or a breath on top of whatever the body plays.
--animation 0 --additive-layer 1 --cubicspline adds the fixture's "spline" animation onto its first.

--cubicspline: CUBICSPLINE samplers are sampled instead of refused (Gltf.set_cubicspline, before anything is posed or baked):
--animation 1 --cubicspline plays the fixture's "spline" animation, on either path.

Default file: tests/golden/morph_bar.glb. Needs a GPU: the product path has no CPU fallback.
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
    ap.add_argument("file", nargs="?", default=os.path.join(os.path.dirname(HERE), "tests", "golden", "morph_bar.glb"))
    ap.add_argument("--animation", type=int, default=0)
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--size", default="640x480")
    ap.add_argument("--out", default="morph.png")
    ap.add_argument("--camera", default="0.8,1.4,7.0,0.8,1.0,0.0,45", help="position, target, vertical field of view in degrees")
    ap.add_argument("--device-lights", action="store_true")
    ap.add_argument("--cubicspline", action="store_true", help="sample CUBICSPLINE animation samplers (Gltf.set_cubicspline) instead of refusing them; animation 1 of the fixture has one")
    ap.add_argument("--device-clips", action="store_true")
    ap.add_argument("--additive-layer", type=int, default=None, metavar="ANIM", help="with --device-clips: play animation ANIM as an additive layer over --animation, with layered morph weights")
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
    if args.additive_layer is not None and (not args.device_clips or not 0 <= args.additive_layer < n_animations):
        sys.exit("--additive-layer needs --device-clips and one of the file's %d animation(s)" % n_animations)
    name, duration, n_channels, n_ignored = gltf.animation(args.animation)
    morphed = [(b, gltf.blas_morph(b)[0]) for b in range(gltf.n_blases)]
    n_targets = sum(len(d) for _, d in morphed if d is not None)
    print("%s: %d skin(s), %d morph target(s) on %d mesh(es), animation %d '%s': %.3f s, %d channel(s), %d of them weights" % (
        args.file, n_skins, n_targets, sum(d is not None for _, d in morphed), args.animation, name, duration, n_channels, n_ignored))
    r = rt.Renderer((w, h))
    if args.device_lights:
        r.set_light_table_build("device")
    if args.batch_trees:
        r.set_mesh_tree_batch("on")
    loaded = r.load_scene(gltf)
    r.attach_skins(gltf, loaded)
    r.attach_morphs(gltf, loaded)
    instances = loaded.instances
    if args.device_clips:
        import torch
        clip = gltf.bake_clip(args.animation)
        cid = r.attach_clip(clip)
        layer_clip = None if args.additive_layer is None else gltf.bake_clip(args.additive_layer)
        layer_id, layer_duration = (None, 0.0) if layer_clip is None else (r.attach_clip(layer_clip), gltf.animation(args.additive_layer)[1])
        items = []
        for b, d in morphed:
            skin = gltf.blas_skin(b)[0]
            weights = None
            if d is not None:
                refusals = [m["error"] for m in (cl.morph(b) for cl in (clip, layer_clip) if cl is not None) if m["state"] == 2]      # abi.CLIP_MORPH_UNAVAILABLE
                if refusals:                # with layered weights every layer's set must be there
                    print("mesh %d: its weights are not played: %s" % (b, refusals[0]))
                else:
                    weights = rt.ClipWeights(b)
            if skin >= 0 or weights is not None:
                items.append((int(loaded.keys[b]), 0, skin if skin >= 0 else None, weights))
        out = torch.zeros((loaded.n_transforms, 12), dtype=torch.float32, device="cuda:%d" % r.devices[0])
        rows = loaded.instance_rows(0)
        for f in range(args.frames):
            u = f / max(args.frames - 1, 1)
            if layer_id is None:
                r.pose_actors([(cid, duration * u, None, rows, 0)], items, out)
            else:
                stack = [(cid, duration * u, 1.0, "override", None, 0.0), (layer_id, layer_duration * u, 1.0, "additive", None, 0.0)]
                r.pose_actors_layered([(stack, None, rows, 0)], items, out, layer_weights=True)
            r.wait_frame(r.render_device_transforms(camera, loaded.layout(), out))
        info = r.actor_pose_info()
        if layer_id is not None:
            wi = r.layer_weights_info()
            print("layered weights: %d item(s), %d set sample(s) a frame, %d of them cubic" % (wi.rows, wi.samples, wi.cubic_samples))
        print("pose_actors: %d launches, %d read-back, %d bytes uploaded a frame, %d item(s) with clip weights" % (info.launches, info.read_backs, info.upload_bytes, info.weight_items))
        instances = loaded.grouped(out.cpu().numpy())
    else:
        for f in range(args.frames):
            instances = r.pose_scene(gltf, loaded, args.animation, duration * f / max(args.frames - 1, 1))
            r.wait_frame(r.render(camera, instances))
    for b, d in morphed:
        if d is not None:
            info = r.replica_scene(0).mesh_morph_info(int(loaded.keys[b]))
            print("mesh %d: %d target(s), %d active in the last pose, %d pose(s)" % (b, info.n_targets, info.n_active, info.posed))
    image = r.render_to_host_memory(camera, instances)       # lets the temporal accumulation settle on the last pose
    write_png(args.out, image)
    print("You can find your render here: %s" % args.out)


if __name__ == "__main__":
    main()
