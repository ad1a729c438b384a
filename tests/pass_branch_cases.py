"""Small frames that drive trace_ris / trace_final down the branches the parity scenes do not reach. A case is a scene description,
an extent (at most 64 x 48), at most five frames, each with its own frame_count, camera and config, and optionally bytes written
into the frame buffers between the two passes of a frame. tests/test_pass_branches_host.py asserts, with the oracle's branch log
(oracle/binding.py: RIS_BITS, FINAL_BITS), that every case reaches what it is there for; tests/test_gpu_pass_branches.py renders
the same cases with the HIP passes and compares every buffer with the oracle's, bit for bit.

Outcomes no input reaches (UNREACHABLE, argued here once; profiles/pass_branch_coverage.txt lists them by line):
  * di_hist_neg, gi_hist_neg: the history pixel is (int)(p + j) with p = prev_uv * extent >= 0 (prev_valid) and a jitter
    j = rnd() - 0.5 >= -0.5, so p + j > -1 and the truncating conversion gives 0 at the least: pcx < 0, pcy < 0, gx < 0, gy < 0
    cannot happen.
  * no_lights (both passes): the instance tables are padded with one dummy record when no instance is emissive, so num_lights >= 1
    for every scene that can be traced. The "no_lights" case renders that dummy record (a zero-area triangle at the origin).
  * gif_behind: combined.W > 0 needs p_hat_final > 1e-3, and gi_target_pdf multiplies by max(dot(n, w), 0) of the very
    w = (sample_pos - hitPos) / max(|.|, 1e-4) from which the next lines compute gi_NdotL: W > 0 implies gi_NdotL > 0. The
    injected case still holds GI samples behind the surface; they end with W = 0.
  * to_ufloat of a negative, of a value >= 65536, of infinity or NaN, and its shift beyond 31 bits: the stored value is
    lerp(albedo, 1, metallic) with an albedo k / 255 and a metallic clamped to [0, 1], or the literal 0 of a sky pixel; it is 0, or at
    least 2^-24 (the smallest half-precision metallic), and at most 1. The log has no bits for those exits.
"""
import numpy as np

from sunray_amd import abi, scenes

MAX_W, MAX_H, MAX_FRAMES = 64, 48, 5
MIN_PIXELS = 8                      # pixels that must take each outcome a case is there for (searched draws: the one pixel named)
UNREACHABLE = {"ris": {"di_hist_neg", "gi_hist_neg", "no_lights"}, "final": {"no_lights", "gif_behind"}}
BOX_CAMERA = ((0.0, 1.0, 3.4), (0.0, 1.0, 0.0))


def config(**over):
    cfg = abi.SrTraceConfig.reference()
    for k, v in over.items():
        setattr(cfg, k, v)
    return cfg


class Frame:
    """One frame of a case. `patch(bufs)`: called between the two passes with the frame's current buffers as numpy arrays
    (depth, normal, reservoirs, reservoirs_gi of the current parity) to overwrite in place; `relight`: instance list set between
    the two passes."""

    def __init__(self, frame_count, camera=BOX_CAMERA, cfg=None, patch=None, relight=None):
        self.frame_count, self.camera, self.cfg, self.patch, self.relight = frame_count, camera, cfg or config(), patch, relight


class Case:
    def __init__(self, name, scene, W, H, frames, ris=(), final=(), pixel=None):
        """`ris` / `final`: the outcomes of the branch log the case is there for; `pixel`: (x, y, frame index) where a searched draw
        must show them, None: on MIN_PIXELS pixels of any frames."""
        assert W <= MAX_W and H <= MAX_H and len(frames) <= MAX_FRAMES
        self.name, self.scene, self.W, self.H, self.frames, self.pixel = name, scene, W, H, frames, pixel
        self.want = {"ris": tuple(ris), "final": tuple(final)}

    def __repr__(self):
        return self.name


# ---- scenes ---------------------------------------------------------------------------------------------------------------------
def small_box(lamp_strength=10.0, lamp_copies=()):
    """The Cornell box with a 224-triangle sphere (236 triangles); `lamp_copies`: further instances of the lamp quad."""
    s = scenes.cornell_box()
    sv, si = scenes.uv_sphere(0.4, 16, 8)
    s.meshes[-1] = scenes.MeshDesc(7, sv, si, s.meshes[-1].material)
    if lamp_strength != 10.0:
        s.meshes[5].material = abi.material(base_color=(0.8, 0.8, 0.8, 1.0), roughness=0.5, emissive_factor=(1.0, 1.0, 1.0), emissive_strength=lamp_strength)
    if lamp_copies:
        s.instances[5] = (6, [abi.IDENTITY_TRANSFORM.copy()] + [scenes.translate(*t) for t in lamp_copies])
    return s


LAMPS_BEHIND_THE_CAMERA = ((0.0, 0.0, 3.0), (-0.8, 0.0, 3.2), (0.8, 0.0, 3.2))    # seen by no camera ray, lighting floor and back wall


def box_with_screen():
    """small_box plus a screen left of the sphere, leaning back (normal (0, 0.6, 0.8)): it faces the camera and the lamp, and the world
    origin, where the all-zero sample of a reservoir that took none sits, lies behind it (and on or in front of every other surface)."""
    s = small_box()
    v, i = scenes.quad((-0.9, 0.1, 0.6), (-0.2, 0.1, 0.6), (-0.2, 0.9, 0.0), (-0.9, 0.9, 0.0), (0, 0.6, 0.8))
    s.meshes.append(scenes.MeshDesc(8, v, i, abi.material(base_color=(0.6, 0.7, 0.5, 1.0), roughness=0.5)))
    s.instances.append((8, [abi.IDENTITY_TRANSFORM.copy()]))
    return s


def one_lamp_left(desc):
    inst = list(desc.instances)
    inst[5] = (6, [abi.IDENTITY_TRANSFORM.copy()])
    return inst


ALBEDO_STEPS = (0, 1, 4, 7, 8, 9, 15, 16, 17, 23, 24, 25, 40, 47, 48, 49, 80, 1008, 1016, 1023, 1024, 1032)


def albedo_strip():
    """Upright black quads side by side across the view, metallic k * 2^-24 for k in ALBEDO_STEPS: half-precision denormals (k < 1024)
    and the first normals. The stored denoiser albedo lerp(0, 1, metallic) = metallic lies in the denormal range of the 11-bit
    channels (unit 2^-20 = 16 steps: exact ties at k = 8, 24, 40) and of the 10-bit channel (unit 2^-19: ties at k = 16, 48, 80),
    with both neighbours of the first ties; k = 0 takes the zero exit, 1023 rounds up into the first normal, 1024 is it."""
    s = scenes.SceneDesc("albedo_strip", camera_pos=BOX_CAMERA[0], camera_target=BOX_CAMERA[1], fov_y=45.0)
    n = len(ALBEDO_STEPS)
    x0, dx = -1.8, 3.6 / n
    for i, k in enumerate(ALBEDO_STEPS):
        v, idx = scenes.quad((x0 + i * dx, -0.5, 0), (x0 + (i + 1) * dx, -0.5, 0), (x0 + (i + 1) * dx, 2.5, 0), (x0 + i * dx, 2.5, 0), (0, 0, 1))
        s.meshes.append(scenes.MeshDesc(10 + i, v, idx, abi.material(base_color=(0.0, 0.0, 0.0, 1.0), metallic=float(np.ldexp(float(k), -24)), roughness=0.5)))
        s.instances.append((10 + i, [abi.IDENTITY_TRANSFORM.copy()]))
    lv, li = scenes.quad((-0.5, 2.4, 1.0), (0.5, 2.4, 1.0), (0.5, 2.4, 2.0), (-0.5, 2.4, 2.0), (0, -1, 0))
    s.meshes.append(scenes.MeshDesc(1, lv, li, abi.material(roughness=0.5, emissive_factor=(1.0, 1.0, 1.0), emissive_strength=8.0)))
    s.instances.append((1, [abi.IDENTITY_TRANSFORM.copy()]))
    return s


def head_on_quad():
    """A metal quad (roughness 0.15: no ReSTIR, the walk takes the BRDF bounce; metallic 1 and white: always the specular lobe) in the
    plane z = 0, seen from (0, 0, 3) along -z. With odd extents the centre pixel has inUV = (0.5, 0.5) exactly, its ray is (0, 0, -1)
    and its view vector equals the normal (0, 0, 1) bit for bit: lensq == 0 in sample_ggx_vndf. No other pixel can: one frame gives
    one such pixel, five frames five. A lamp behind the camera catches the reflected rays."""
    s = scenes.SceneDesc("head_on_quad", camera_pos=(0.0, 0.0, 3.0), camera_target=(0.0, 0.0, 0.0), fov_y=45.0)
    v, i = scenes.quad((-2, -2, 0), (2, -2, 0), (2, 2, 0), (-2, 2, 0), (0, 0, 1))
    s.meshes.append(scenes.MeshDesc(1, v, i, abi.material(base_color=(1.0, 1.0, 1.0, 1.0), metallic=1.0, roughness=0.15)))
    s.instances.append((1, [abi.IDENTITY_TRANSFORM.copy()]))
    lv, li = scenes.quad((-3, -3, 5), (-3, 3, 5), (3, 3, 5), (3, -3, 5), (0, 0, -1))
    s.meshes.append(scenes.MeshDesc(2, lv, li, abi.material(roughness=0.5, emissive_factor=(1.0, 0.9, 0.8), emissive_strength=3.0)))
    s.instances.append((2, [abi.IDENTITY_TRANSFORM.copy()]))
    return s


def _box_mesh(lo, hi):
    """Axis-aligned box, outward normals, 12 triangles."""
    (x0, y0, z0), (x1, y1, z1) = lo, hi
    faces = [(((x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1)), (0, 0, 1)), (((x1, y0, z0), (x0, y0, z0), (x0, y1, z0), (x1, y1, z0)), (0, 0, -1)),
             (((x1, y0, z1), (x1, y0, z0), (x1, y1, z0), (x1, y1, z1)), (1, 0, 0)), (((x0, y0, z0), (x0, y0, z1), (x0, y1, z1), (x0, y1, z0)), (-1, 0, 0)),
             (((x0, y1, z1), (x1, y1, z1), (x1, y1, z0), (x0, y1, z0)), (0, 1, 0)), (((x0, y0, z0), (x1, y0, z0), (x1, y0, z1), (x0, y0, z1)), (0, -1, 0))]
    vs, idx = [], []
    for k, (p, n) in enumerate(faces):
        v, i = scenes.quad(p[0], p[1], p[2], p[3], n)
        vs.append(v); idx.append(i + 4 * k)
    return np.concatenate(vs), np.concatenate(idx).astype(np.uint32)


def _room_inward(lo, hi, key0, material, s):
    """The six faces of a box seen from inside, one mesh each (inward normals)."""
    (x0, y0, z0), (x1, y1, z1) = lo, hi
    faces = [(((x0, y0, z1), (x1, y0, z1), (x1, y0, z0), (x0, y0, z0)), (0, 1, 0)), (((x0, y1, z0), (x1, y1, z0), (x1, y1, z1), (x0, y1, z1)), (0, -1, 0)),
             (((x0, y0, z0), (x1, y0, z0), (x1, y1, z0), (x0, y1, z0)), (0, 0, 1)), (((x1, y0, z1), (x0, y0, z1), (x0, y1, z1), (x1, y1, z1)), (0, 0, -1)),
             (((x0, y0, z1), (x0, y0, z0), (x0, y1, z0), (x0, y1, z1)), (1, 0, 0)), (((x1, y0, z0), (x1, y0, z1), (x1, y1, z1), (x1, y1, z0)), (-1, 0, 0))]
    for k, (p, n) in enumerate(faces):
        v, i = scenes.quad(p[0], p[1], p[2], p[3], n)
        s.meshes.append(scenes.MeshDesc(key0 + k, v, i, material))
        s.instances.append((key0 + k, [abi.IDENTITY_TRANSFORM.copy()]))


def glass_block():
    """A long glass block (ior 1.5) seen obliquely: rays entering through the front face meet the side faces at grazing angles from
    inside (total internal reflection), those crossing to the back face leave steeply (absorption along the inside path)."""
    s = small_box()
    s.name = "glass_block"
    v, i = _box_mesh((-0.35, 0.3, -0.9), (0.35, 1.5, 0.9))
    s.meshes[-1] = scenes.MeshDesc(7, v, i, abi.material(base_color=(0.7, 0.9, 0.8, 1.0), roughness=0.05, transmission=1.0, ior=1.5))
    s.instances[-1] = (7, [abi.IDENTITY_TRANSFORM.copy()])
    s.camera_pos, s.camera_target = (0.9, 1.2, 3.2), (0.0, 0.9, 0.0)
    return s


def facing_mirrors():
    """Two large mirrors face each other across the camera: every camera ray bounces between them until virtual_bounces runs out
    (RIS pass) or the walk of the final pass dies in Russian roulette."""
    s = scenes.SceneDesc("facing_mirrors", camera_pos=(0.0, 0.0, 0.5), camera_target=(0.0, 0.0, -1.0), fov_y=45.0)
    mirror = abi.material(base_color=(0.95, 0.95, 0.95, 1.0), metallic=1.0, roughness=0.02)
    v, i = scenes.quad((-60, -60, -1), (60, -60, -1), (60, 60, -1), (-60, 60, -1), (0, 0, 1))
    s.meshes.append(scenes.MeshDesc(1, v, i, mirror)); s.instances.append((1, [abi.IDENTITY_TRANSFORM.copy()]))
    v, i = scenes.quad((60, -60, 1), (-60, -60, 1), (-60, 60, 1), (60, 60, 1), (0, 0, -1))
    s.meshes.append(scenes.MeshDesc(2, v, i, mirror)); s.instances.append((2, [abi.IDENTITY_TRANSFORM.copy()]))
    lv, li = scenes.quad((-0.2, 0.9, -0.2), (0.2, 0.9, -0.2), (0.2, 0.9, 0.2), (-0.2, 0.9, 0.2), (0, -1, 0))
    s.meshes.append(scenes.MeshDesc(3, lv, li, abi.material(roughness=0.5, emissive_factor=(1.0, 1.0, 1.0), emissive_strength=6.0)))
    s.instances.append((3, [abi.IDENTITY_TRANSFORM.copy()]))
    return s


def dark_corridor():
    """A closed corridor of a dark (albedo 0.02) dielectric of roughness 0.15 with a small lamp: no ReSTIR (roughness <= 0.2), the walk
    bounces until its throughput falls under 0.001 or Russian roulette ends it."""
    s = scenes.SceneDesc("dark_corridor", camera_pos=(0.0, 1.0, 2.5), camera_target=(0.0, 1.0, -3.0), fov_y=45.0)
    _room_inward((-1, 0, -3), (1, 2, 3), 1, abi.material(base_color=(0.02, 0.02, 0.02, 1.0), roughness=0.15), s)
    lv, li = scenes.quad((-0.3, 1.99, -1.3), (0.3, 1.99, -1.3), (0.3, 1.99, -0.7), (-0.3, 1.99, -0.7), (0, -1, 0))
    s.meshes.append(scenes.MeshDesc(9, lv, li, abi.material(roughness=0.5, emissive_factor=(1.0, 1.0, 1.0), emissive_strength=10.0)))
    s.instances.append((9, [abi.IDENTITY_TRANSFORM.copy()]))
    return s


# ---- bytes written between the two passes ------------------------------------------------------------------------------------------
def primary_rays(camera, fov_y, W, H):
    """(origin, directions [H, W, 3]) of the camera rays, float64 (good to 1e-6: the patches that use them keep margins of 5e-4)."""
    pos, tgt = np.array(camera[0], dtype=np.float64), np.array(camera[1], dtype=np.float64)
    f = (tgt - pos) / np.linalg.norm(tgt - pos)
    s = np.cross(f, (0.0, 1.0, 0.0)); s /= np.linalg.norm(s)
    u = np.cross(s, f)
    th = np.tan(np.radians(fov_y) / 2.0)
    x = ((np.arange(W) + 0.5) / W * 2.0 - 1.0) * th * W / H
    y = -((np.arange(H) + 0.5) / H * 2.0 - 1.0) * th
    d = x[None, :, None] * s + y[:, None, None] * u + f
    return pos, d / np.linalg.norm(d, axis=-1, keepdims=True)


def _snorm_bytes(normal_img):
    return normal_img.view(np.int8).reshape(-1, 4)[:, :3].astype(np.int32)


def uniform_blocks(normal_img, depth_img, W, H, size=8):
    """Top-left corners of non-overlapping size x size blocks whose pixels all store the same normal and a finite depth, scan order."""
    nrm, dep = normal_img.reshape(H, W), depth_img.reshape(H, W)
    taken, out = np.zeros((H, W), dtype=bool), []
    for y in range(0, H - size + 1, 2):
        for x in range(0, W - size + 1, 2):
            b = nrm[y:y + size, x:x + size]
            if taken[y:y + size, x:x + size].any() or (b != b[0, 0]).any() or (dep[y:y + size, x:x + size] >= 0x7C00).any():
                continue
            taken[y:y + size, x:x + size] = True
            out.append((x, y))
    return out, taken


def pack_normal(oracle, n):
    return int(oracle.lib().orc_pack_normal(*[float(c) for c in n]))


def inject_patterns(oracle, desc, W, H, num_lights):
    """The patch of the injected-state case: each pattern goes into one 8 x 8 block (neighbours read neighbours) and into one isolated
    pixel. Blocks and pixels are chosen from the frame itself (uniform normal, finite depth), so the same bytes land in the host and
    in the device frame, which hold the same bits at that point."""
    def patch(bufs):
        res, gi, depth, normal = bufs["reservoirs"], bufs["reservoirs_gi"], bufs["depth"], bufs["normal"]
        blocks, taken = uniform_blocks(normal, depth, W, H)
        nb = _snorm_bytes(normal)
        origin, dirs = primary_rays((desc.camera_pos, desc.camera_target), desc.fov_y, W, H)
        dist = np.array([oracle.lib().orc_f16_to_f32(int(h)) for h in depth], dtype=np.float64).reshape(H, W)
        hit = (origin + dirs * dist[..., None]).reshape(-1, 3)
        n_f = nb / 127.0
        lone = [(x, y) for y in range(1, H - 1, 3) for x in range(1, W - 1, 3) if not taken[y, x] and depth[y * W + x] < 0x7C00]
        assert len(blocks) >= 13 and len(lone) >= 13, (len(blocks), len(lone))
        ceiling = [b for b in blocks if (nb[b[1] * W + b[0]] == (0, -127, 0)).all()]
        assert ceiling, "no 8 x 8 block of the ceiling: nothing stores a -127 byte to turn into -128"
        blocks.remove(ceiling[0])
        blocks.insert(12, ceiling[0])
        leaning = [b for b in blocks if (nb[b[1] * W + b[0]] != 0).sum() == 2]       # the one surface whose normal is not along an axis
        assert leaning, "no 8 x 8 block of the screen"
        blocks.remove(leaning[0])
        blocks.insert(5, leaning[0])                                   # w_tiny: zero samples whose position, the origin, is behind

        def pixels_of(k):
            bx, by = blocks[k]
            px = [(by + j) * W + bx + i for j in range(8) for i in range(8)] + [lone[k][1] * W + lone[k][0]]
            return np.array(px)

        def light(px, **fields):
            res["W"][px] = np.maximum(res["W"][px], np.float32(1.0))       # W > 0, finite
            for k, v in fields.items():
                res[k][px] = v

        names = ("idx_num_lights", "idx_plus_7", "idx_all_ones", "w_inf", "m_huge", "w_tiny", "light_behind", "gi_behind", "gi_near",
                 "gi_cos_old_zero", "gi_w_inf", "depth_inf", "normal_minus_128")
        for k, name in enumerate(names):
            px = pixels_of(k)
            if name == "idx_num_lights":
                light(px, light_idx=num_lights)
            elif name == "idx_plus_7":
                light(px, light_idx=num_lights + 7)
            elif name == "idx_all_ones":
                light(px, light_idx=0xFFFFFFFF)
            elif name == "w_inf":
                res["W"][px] = np.float32(np.inf)
            elif name == "m_huge":
                light(px, M=np.float32(1e30))
            elif name == "w_tiny":                     # weights far under the 1e-4 floor of the update test: merged, hardly ever taken
                res["W"][px] = np.float32(1e-9)
            elif name == "light_behind":
                light(px, light_pos=(hit[px] - 0.5 * n_f[px]).astype(np.float32))
            elif name in ("gi_behind", "gi_near", "gi_cos_old_zero", "gi_w_inf"):
                gi["W"][px] = np.float32(np.inf if name == "gi_w_inf" else 1.0)
                gi["M"][px] = np.float32(1e30 if name == "gi_w_inf" else 1.0)
                gi["w_sum"][px] = np.float32(1.0)
                gi["sample_radiance"][px] = np.float32(2.0)
                if name == "gi_behind":
                    gi["sample_pos"][px] = (hit[px] - 0.5 * n_f[px]).astype(np.float32)
                elif name == "gi_near":                # 0.0015 off the pixel's own hit point: the final visibility segment is too short to trace
                    gi["sample_pos"][px] = (hit[px] + 0.0015 * n_f[px]).astype(np.float32)
                    gi["sample_normal_packed"][px] = [pack_normal(oracle, -n_f[p]) for p in px]
                elif name == "gi_cos_old_zero":        # the sample's surface faces away from the pixels that would reuse it
                    gi["sample_pos"][px] = (hit[px] + 0.5 * n_f[px]).astype(np.float32)
                    gi["sample_normal_packed"][px] = [pack_normal(oracle, n_f[p]) for p in px]
            elif name == "depth_inf":
                depth[px] = 0x7C00
            elif name == "normal_minus_128":
                b = normal.view(np.uint8).reshape(-1, 4)
                sel = b[px]
                assert (sel == 0x81).any()
                sel[sel == 0x81] = 0x80
                b[px] = sel
    return patch


def near_wall_samples(oracle, desc, W, H):
    """The patch of the close-up case: the camera is 4 mm from the back wall, so all hit points lie within about 2 mm of each other; every
    pixel's GI reservoir gets one common sample half a millimetre in front of the wall's centre point. Whatever neighbour a pixel picks,
    the segment to that sample is at most 0.002 long for all but the outermost pixels: no visibility query is issued for it."""
    def patch(bufs):
        gi = bufs["reservoirs_gi"]
        p = np.array(desc.camera_target, dtype=np.float32) + np.array((0.0, 0.0, 0.0005), dtype=np.float32)
        gi["sample_pos"][:] = p
        gi["sample_normal_packed"][:] = pack_normal(oracle, (0.0, 0.0, -1.0))
        gi["sample_radiance"][:] = np.float32(1.5)
        gi["W"][:] = np.float32(1.0)
        gi["M"][:] = np.float32(1.0)
        gi["w_sum"][:] = np.float32(1.0)
    return patch


def focused_samples(oracle, desc, W, H):
    """Every pixel of the back wall gets one common GI sample 5 cm in front of the wall's centre, facing the wall. A pixel that reuses
    it from a neighbour at least 2.2 times as far from the centre as itself has a Jacobian (d_old / d_new)^3 above 10: clamped."""
    def patch(bufs):
        gi, depth = bufs["reservoirs_gi"], bufs["depth"]
        nb = _snorm_bytes(bufs["normal"])
        dist = np.array([oracle.lib().orc_f16_to_f32(int(h)) for h in depth])
        wall = np.nonzero((nb == (0, 0, 127)).all(axis=1) & (dist > 4.0) & (dist < 10.0))[0]
        assert len(wall) > 200
        gi["sample_pos"][wall] = np.array((0.0, 1.0, -0.95), dtype=np.float32)
        gi["sample_normal_packed"][wall] = pack_normal(oracle, (0.0, 0.0, -1.0))
        gi["sample_radiance"][wall] = np.float32(1.0)
        gi["W"][wall] = np.float32(1.0)
        gi["M"][wall] = np.float32(1.0)
        gi["w_sum"][wall] = np.float32(1.0)
    return patch


# ---- searched draws ------------------------------------------------------------------------------------------------------------------
# rnd() returns exactly 1.0f when its 32-bit result is >= 0xFFFFFF80. DRAWS[name] = (x, y, k, frame_count): in a DRAW_W-wide frame
# with that frame_count the k-th draw (from 0) of pixel (x, y) is such a result; found with find_draw_frames below, confirmed with
# orc_rnd_stream by the host test. (8, 10) is a floor pixel under the lamp; (8, 6) lies on the back wall, which has the world origin in
# front of it: a reservoir left with weight but without a sample (position 0, 0, 0) keeps its W there through the visibility test.
DRAW_W, DRAW_H = 16, 12
DRAWS = {"draw_one_ris_index": (8, 10, 0, 6726715), "draw_one_ris_update": (8, 6, 3, 2703067), "draw_one_gi_direction": (8, 10, 1, 42239183),
         "draw_one_gi_nee_index": (8, 10, 2, 10444307), "draw_one_final_nee_index": (8, 10, 0, 6726715)}


def find_draw_frames(px, py, W, draws, start=0, chunk=1 << 24):
    """{k: smallest frame_count >= start whose k-th draw for pixel (px, py) of a W-wide launch is 1.0f}, by a vectorised search."""
    found, base = {}, start
    pix = np.uint32(py * W + px)
    with np.errstate(over="ignore"):
        while len(found) < len(draws) and base < (1 << 32):
            frames = np.arange(base, min(base + chunk, 1 << 32), dtype=np.uint64).astype(np.uint32)
            seed = scenes._pcg_hash(pix ^ scenes._pcg_hash(frames.copy()))
            for k in range(max(draws) + 1):
                seed = seed * np.uint32(747796405) + np.uint32(2891336453)
                if k in draws and k not in found:
                    word = ((seed >> ((seed >> np.uint32(28)) + np.uint32(4))) ^ seed) * np.uint32(277803737)
                    hits = np.nonzero(((word >> np.uint32(22)) ^ word) >= np.uint32(0xFFFFFF80))[0]
                    if hits.size:
                        found[k] = int(frames[hits[0]])
            base += chunk
    return found


def _cases():
    box = small_box
    pan = [Frame(0),
           Frame(1, ((0.0, 1.0, 3.4), (0.9, 1.6, 0.0))),       # turned right and up: the previous view lies left and below
           Frame(2, ((0.0, 1.0, 3.4), (-0.9, 0.4, 0.0))),      # turned left and down: the previous view lies right and above
           Frame(3, ((0.0, 1.0, -0.3), (0.0, 1.0, -1.0))),     # deep in the box, facing the back wall
           Frame(4)]                                            # back out: the previous camera is behind most of what is seen
    cases = [
        Case("pan", box, 64, 48, pan,
             ris=("prev_behind", "prev_x_neg", "prev_y_neg", "prev_x_high", "prev_y_high", "prev_valid", "di_hist_inside", "gi_hist_inside", "gi_ndotl_pos", "taken")),
        # from inside the box, where every pixel sees a wall, turning a little further right and down each frame: the right and the bottom
        # edge of the previous view cross walls, and the jittered history pixel of some pixels next to those edges falls off them
        Case("pan_edges", box, 64, 48, [Frame(k, ((0.0, 1.0, 0.8), (0.15 * k, 1.0 - 0.12 * k, -1.0))) for k in range(5)],
             ris=("di_hist_x_high", "di_hist_y_high", "gi_hist_x_high", "gi_hist_y_high", "prev_x_high", "prev_y_high")),
        Case("no_lights", lambda: small_box(lamp_strength=0.0), 48, 32,
             [Frame(0), Frame(1), Frame(2, cfg=config(enable_restir=0))],
             ris=("audition", "idx_in_range", "nee_idx_in_range"), final=("nee_idx_in_range", "vndf_below", "rr_survive", "rr_die", "diffuse_bounce")),
        Case("albedo_strip", albedo_strip, 64, 48, [Frame(0), Frame(1)],
             ris=("uf_zero", "uf_down", "uf_up", "uf_tie_down", "uf_tie_up", "uf_normal")),
        Case("head_on", head_on_quad, 33, 25, [Frame(f) for f in range(5)], final=("vndf_head_on",), pixel=(16, 12, None)),
        Case("glass_block", glass_block, 64, 48, [Frame(0), Frame(1)], ris=("tir",), final=("tir", "reflect", "refract_in", "refract_out")),
        Case("facing_mirrors", facing_mirrors, 48, 32, [Frame(0, ((0.0, 0.0, 0.5), (0.0, 0.0, -1.0)), config(virtual_bounces=6)),
                                                        Frame(1, ((0.0, 0.0, 0.5), (0.0, 0.0, -1.0)), config(virtual_bounces=6))],
             ris=("no_diffuse",), final=("rr_survive", "throughput_break", "vndf_above")),
        Case("dark_corridor", dark_corridor, 48, 32, [Frame(0, ((0.0, 1.0, 2.5), (0.0, 1.0, -3.0))), Frame(1, ((0.0, 1.0, 2.5), (0.0, 1.0, -3.0)))],
             final=("throughput_break", "rr_die", "vndf_above", "diffuse_bounce", "bright_break")),
    ]
    focus = small_box()
    cases.append(Case("injected_focus", lambda: focus, 48, 32, [Frame(0, patch=focused_samples(_oracle(), focus, 48, 32))],
                      final=("gi_jacobian_clamped", "gi_merged", "gif_repeat")))
    injected = box_with_screen()
    cases.append(Case("injected", lambda: injected, 64, 48, [Frame(0, patch=inject_patterns(_oracle(), injected, 64, 48, 2))],
                      final=("center_idx_out", "center_merged", "neighbor_idx_out", "neighbor_merged", "neighbor_depth_reject", "di_zero_sample",
                             "di_behind", "di_query", "gi_self", "gi_cos_zero", "gif_short", "gi_merged", "gif_query", "gif_repeat")))
    close_up = small_box()
    close_up.camera_pos, close_up.camera_target = (0.0, 1.0, -0.996), (0.0, 1.0, -1.0)
    cases.append(Case("injected_close_up", lambda: close_up, 32, 24,
                      [Frame(0, (close_up.camera_pos, close_up.camera_target), patch=near_wall_samples(_oracle(), close_up, 32, 24))],
                      final=("gi_short", "gif_short", "gi_merged")))
    relit = small_box(lamp_copies=LAMPS_BEHIND_THE_CAMERA)
    cases.append(Case("relit_between_passes", lambda: relit, 48, 32, [Frame(0, relight=one_lamp_left(relit)), Frame(1, relight=one_lamp_left(relit))],
                      final=("center_idx_out", "neighbor_idx_out", "center_merged", "neighbor_merged")))
    draws = (("draw_one_ris_index", config(), ("idx_clamped",), ()),
             # one candidate: its update test is draw 3, and nothing later can take a sample after all
             ("draw_one_ris_update", config(ris_candidates=1), ("first_not_taken",), ()),
             ("draw_one_gi_direction", config(ris_candidates=0), ("gi_ndotl_zero",), ()),     # r2 = 1: the bounce lies in the surface
             ("draw_one_gi_nee_index", config(ris_candidates=0), ("nee_idx_clamped",), ()),
             ("draw_one_final_nee_index", config(enable_restir=0), (), ("nee_idx_clamped",)))
    for name, cfg, ris, final in draws:
        x, y, k, frame_count = DRAWS[name]
        cases.append(Case(name, box, DRAW_W, DRAW_H, [Frame(frame_count, cfg=cfg)], ris=ris, final=final, pixel=(x, y, 0)))
    return cases


def _oracle():
    from oracle import binding
    return binding


_built = None


def cases():
    global _built
    if _built is None:
        _built = _cases()
    return _built


# ---- the oracle's frames -------------------------------------------------------------------------------------------------------------
BUFFERS = ("depth", "normal", "diffuse", "motion", "reservoirs", "reservoirs_gi", "raw_color")
_reference = {}


def current_buffers(frame, f):
    """The buffers a patch may write, of parity f & 1, as the arrays `frame` (a HostFrame) itself holds."""
    return {"depth": frame.depth, "normal": frame.normal, "reservoirs": frame.reservoirs[f & 1], "reservoirs_gi": frame.reservoirs_gi[f & 1]}


def oracle_frames(oracle, case, blue_noise):
    """Renders the case with the oracle, branch log on. Returns a list with, per frame: the compared buffers after the RIS pass (before any
    patch) and after the final pass, the branch log [H, W, 2] and the ray counters of the frame. Computed once."""
    if case.name in _reference:
        return _reference[case.name]
    desc = case.scene()
    W, H = case.W, case.H
    osc = oracle.OracleScene().load(desc)
    of = oracle.HostFrame(W, H, blue_noise)
    log = np.zeros((H, W, 2), dtype=np.uint32)
    osc.set_branch_log(log)
    out, prev = [], None
    for fr in case.frames:
        f = fr.frame_count
        if fr.relight is not None:
            osc.set_instances(desc.instances)
        m = oracle.camera_matrices(fr.camera[0], fr.camera[1], desc.fov_y, W, H, prev)
        prev = list(m.view_proj)
        log[:] = 0
        osc.reset_counters()
        rec = {}
        if fr.cfg.enable_restir:
            osc.trace_ris(of, m, f, fr.cfg)
        rec["after_ris"] = snapshot(of, f)
        if fr.patch is not None:
            fr.patch(current_buffers(of, f))
        if fr.relight is not None:
            osc.set_instances(fr.relight)
        osc.trace_final(of, m, f, fr.cfg)
        rec["after_final"] = snapshot(of, f)
        rec["log"] = log.copy()
        c = osc.counters()
        rec["counters"] = (c.closest_queries, c.any_queries)
        out.append(rec)
    osc.set_branch_log(None)
    osc.close()
    _reference[case.name] = out
    return out


def snapshot(frame, f):
    return {"depth": frame.depth.copy(), "normal": frame.normal.copy(), "diffuse": frame.diffuse.copy(), "motion": frame.motion.copy(),
            "reservoirs": frame.reservoirs[f & 1].copy(), "reservoirs_gi": frame.reservoirs_gi[f & 1].copy(), "raw_color": frame.raw_color.copy()}


def count_bits(log_word, names, table):
    """{name: pixels of `log_word` ([H, W] uint32) with the bit of `name` set}."""
    return {n: int(((log_word & np.uint32(table[n])) != 0).sum()) for n in names}
