"""ctypes binding of the CPU oracle (oracle/_build/liboracle.so).

ORACLE — TEST INFRASTRUCTURE, NOT PRODUCT CODE. Only tests/, __graft_entry__.smoke() and bench.py's
cpu_baseline leg import this module. Parity status: UNPINNED (the reference holds no golden vectors
for this path; the oracle is pinned by the hand-derived KATs in tests/golden/ only).
"""
import ctypes as C
import os
import subprocess

import numpy as np

from sunray_amd import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "_build", "liboracle.so")
_lib = None


def build(force=False):
    """Compile the oracle with its Makefile (gcc only; no GPU, no reference sources needed)."""
    if force or not os.path.exists(_LIB_PATH):
        subprocess.check_call(["make", "-C", _HERE, "_build/liboracle.so"])
    return _LIB_PATH


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            build()
        L = C.CDLL(_LIB_PATH)
        L.orc_scene_create.restype = C.c_void_p
        L.orc_f16_to_f32.restype = C.c_float
        L.orc_exp.restype = C.c_float
        L.orc_exp.argtypes = [C.c_float]
        L.orc_log.restype = C.c_float
        L.orc_log.argtypes = [C.c_float]
        L.orc_pow.restype = C.c_float
        L.orc_pow.argtypes = [C.c_float, C.c_float]
        L.orc_smith_v_ggx.restype = C.c_float
        L.orc_smith_g1_ggx.restype = C.c_float
        L.orc_smoothstep.restype = C.c_float
        for name in ("orc_smith_v_ggx", "orc_smoothstep"):
            getattr(L, name).argtypes = [C.c_float] * 3
        L.orc_smith_g1_ggx.argtypes = [C.c_float] * 2
        L.orc_f32_to_f16.argtypes = [C.c_float]
        L.orc_f16_to_f32.argtypes = [C.c_uint32]
        L.orc_pack_normal.argtypes = [C.c_float] * 3
        L.orc_pack_unorm_4x8.argtypes = [C.c_float] * 4
        L.orc_pack_rgba8_snorm.argtypes = [C.c_float] * 4
        L.orc_pack_half_2x16.argtypes = [C.c_float] * 2
        L.orc_pack_snorm_2x16.argtypes = [C.c_float] * 2
        L.orc_pack_b10g11r11.argtypes = [C.c_float] * 3
        for name in ("orc_pack_normal", "orc_pack_unorm_4x8", "orc_pack_rgba8_snorm", "orc_pack_half_2x16",
                     "orc_pack_snorm_2x16", "orc_pack_b10g11r11", "orc_f32_to_f16", "orc_pcg_hash",
                     "orc_init_rng", "orc_rnd_stream"):
            getattr(L, name).restype = C.c_uint32
        _lib = L
    return _lib


def usable_cores():
    """CPUs this process may actually use: affinity mask capped by the cgroup CPU quota."""
    n = len(os.sched_getaffinity(0))
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, -(-int(quota) // int(period))))
    except (OSError, ValueError):
        pass
    return n


def set_threads(n):
    lib().orc_set_threads(C.c_int(n))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _f3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


def unpack_normal(p):
    out = (C.c_float * 3)()
    lib().orc_unpack_normal(C.c_uint32(p), out)
    return np.array(list(out), dtype=np.float32)


def probe_helper_layout(fn):
    """(input dwords, output dwords) of one row of helper `fn` (the SrProbeHelper ids of include/sunray_hip.h), None if unknown."""
    i, o = C.c_uint32(), C.c_uint32()
    if lib().orc_probe_helper_layout(C.c_uint32(fn), C.byref(i), C.byref(o)) != 0:
        return None
    return i.value, o.value


def probe_helper(fn, rows):
    """orc_probe_helper: helper `fn` of the oracle on every row of `rows` (uint32, n x input dwords) -> uint32, n x output dwords."""
    layout = probe_helper_layout(fn)
    if layout is None:
        raise ValueError("orc_probe_helper knows no helper %d" % fn)
    iw, ow = layout
    rows = np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1, iw)
    out = np.zeros((rows.shape[0], ow), dtype=np.uint32)
    if lib().orc_probe_helper(C.c_uint32(fn), _p(rows), C.c_uint32(rows.shape[0]), _p(out)) != 0:
        raise ValueError("orc_probe_helper refused helper %d" % fn)
    return out


NO_READ = -2 ** 31    # read-log marker (orc_scene.h, kNoRead)

# Branch log (OracleScene.set_branch_log): bit k of a pixel's word is set when the pass took the outcome named k-th here.
# Word 0, trace_ris (ray_gen_ris.slang; the numbers are lines of oracle/orc_passes.cpp as it stood before the log was added):
RIS_BITS = (
    "prev_behind",           # :150 prev_clip.w <= 0.01
    "prev_x_neg", "prev_y_neg", "prev_x_high", "prev_y_high",    # :155, each side of the screen the reprojection can leave by
    "prev_valid",            # :155 reprojection on screen
    "di_hist_neg",           # :217 pcx < 0 or pcy < 0 (unreachable: (int)(x) of an x > -1 is 0)
    "di_hist_x_high", "di_hist_y_high", "di_hist_inside",        # :217
    "gi_hist_neg",           # :319 gx < 0 or gy < 0 (unreachable, as di_hist_neg)
    "gi_hist_x_high", "gi_hist_y_high", "gi_hist_inside",        # :319
    "no_lights",             # :176 / :272 num_lights == 0 (unreachable: the instance tables always hold the dummy record)
    "audition",              # :176 lights and a rough surface: the candidates are drawn
    "idx_clamped", "idx_in_range",                               # :179 candidate index, rnd() == 1.0f or less
    "first_not_taken",       # :199 the first candidate with a weight is not taken: the reservoir holds no sample yet has w_sum > 0
    "taken",                 # :199
    "gi_ndotl_zero", "gi_ndotl_pos",                             # :261
    "nee_idx_clamped", "nee_idx_in_range",                       # :274
    "tir",                   # :139 total internal reflection
    "no_diffuse",            # :165 every virtual bounce was glass or mirror
    # to_ufloat (orc_utils.h:208-234) of the stored denoiser albedo, any of its three channels:
    "uf_zero",               # :222 below the smallest denormal's half
    "uf_down", "uf_up",      # :231 denormal range, rounded down / up
    "uf_tie_down", "uf_tie_up",                                  # :231 denormal range, exact tie to the even neighbour below / above
    "uf_normal",             # :216
)
# Word 1, trace_final (ray_gen_final.slang):
FINAL_BITS = (
    "tir", "reflect", "refract_in", "refract_out",               # :405-413 glass: total internal reflection; the three ways on
    "bright_break",          # :394 brightness > 1
    "throughput_break",      # :596 p < 0.001
    "rr_survive", "rr_die",  # :598 Russian roulette
    "vndf_below", "vndf_above",                                  # :582 VNDF sample under the horizon or not
    "vndf_head_on",          # orc_utils.h:116 lensq == 0
    "diffuse_bounce",        # :591
    "no_lights",             # :419 num_lights == 0 (unreachable, as in RIS_BITS)
    "center_idx_out", "center_merged",                           # :424 W > 0 and light_idx >= num_lights, or merged
    "neighbor_idx_out", "neighbor_merged",                       # :448
    "neighbor_depth_reject",                                     # :444
    "di_zero_sample",        # :456 w_sum > 0 and no merge took its sample: the held sample is all zeros
    "di_behind", "di_query",                                     # :465
    "gi_self",               # :481 GI neighbour is the own pixel
    "gi_cos_zero",           # :502
    "gi_jacobian_clamped",   # :504 above 10
    "gi_short",              # :507 segment to the neighbour's sample <= 0.002: no query is issued
    "gi_merged",             # :510
    "gif_behind", "gif_query",                                   # :520
    "gif_repeat",            # :521 asks about the segment :507 asked about (the sample came from a neighbour)
    "gif_short",             # :521 segment <= 0.002: no query is issued
    "nee_idx_clamped", "nee_idx_in_range",                       # :531
)
RIS_BIT = {name: 1 << k for k, name in enumerate(RIS_BITS)}
FINAL_BIT = {name: 1 << k for k, name in enumerate(FINAL_BITS)}
assert len(RIS_BITS) <= 32 and len(FINAL_BITS) <= 32


class OracleScene:
    """Oracle counterpart of sunray_amd.Scene: same methods, numpy (host) buffers."""

    def __init__(self):
        self._h = C.c_void_p(lib().orc_scene_create())
        self._keep = []

    def close(self):
        if self._h:
            lib().orc_scene_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add_mesh(self, key, vertices, indices, material):
        v = np.ascontiguousarray(vertices, dtype=abi.VERTEX)
        i = np.ascontiguousarray(indices, dtype=np.uint32)
        m = np.ascontiguousarray(material, dtype=abi.MATERIAL)
        slot = lib().orc_scene_add_mesh(self._h, C.c_uint64(key), _p(v), C.c_uint32(len(v)), _p(i), C.c_uint32(len(i)), _p(m))
        if slot < 0:
            raise ValueError("oracle add_mesh rejected the mesh (same checks as Renderer::load_mesh, lib.rs:880-899)")
        return slot

    def add_blas(self, key, vertices, indices, material, emissive):
        v = np.ascontiguousarray(vertices, dtype=abi.VERTEX)
        i = np.ascontiguousarray(indices, dtype=np.uint32)
        m = np.ascontiguousarray(material, dtype=abi.MATERIAL)
        e = np.ascontiguousarray(emissive, dtype=abi.EMISSIVE_TRIANGLE)
        slot = lib().orc_scene_add_blas(self._h, C.c_uint64(key), _p(v), C.c_uint32(len(v)), _p(i), C.c_uint32(len(i)), _p(m),
                                        _p(e) if len(e) else None, C.c_uint32(len(e)))
        if slot < 0:
            raise ValueError("oracle add_blas rejected the mesh")
        return slot

    def remove(self, key):
        lib().orc_scene_remove(self._h, C.c_uint64(key))

    def add_image(self, pixels):
        a = np.ascontiguousarray(pixels, dtype=np.uint8)
        ch = 1 if a.ndim == 2 else a.shape[2]
        slot = lib().orc_scene_add_image(self._h, _p(a), C.c_uint32(a.shape[1]), C.c_uint32(a.shape[0]), C.c_uint32(ch))
        if slot < 0:
            raise ValueError("oracle add_image rejected the image")
        return slot

    def add_sampler(self, min_filter, mag_filter, address_mode_u, address_mode_v):
        d = abi.SrSamplerDesc(min_filter, mag_filter, address_mode_u, address_mode_v)
        slot = lib().orc_scene_add_sampler(self._h, C.byref(d))
        if slot < 0:
            raise ValueError("oracle add_sampler rejected the sampler")
        return slot

    def sample_texture(self, image, sampler, u, v, fallback=(0.0, 0.0, 0.0, 0.0)):
        out = (C.c_float * 4)()
        lib().orc_sample_texture(self._h, C.c_uint32(image), C.c_uint32(sampler), C.c_float(u), C.c_float(v), (C.c_float * 4)(*fallback), out)
        return np.array(list(out), dtype=np.float32)

    def set_instances(self, instances):
        keys = np.array([k for k, _ in instances], dtype=np.uint64)
        counts = np.array([len(t) for _, t in instances], dtype=np.uint32)
        xf = np.array([np.asarray(t, dtype=np.float32).reshape(12) for _, ts in instances for t in ts], dtype=np.float32).reshape(-1, 12)
        if len(xf) == 0:
            xf = np.zeros((1, 12), dtype=np.float32)
        rc = lib().orc_scene_set_instances(self._h, _p(keys), _p(counts), C.c_uint32(len(keys)), _p(np.ascontiguousarray(xf)))
        if rc != 0:
            raise ValueError("frame_instance_data: instance references a BLAS key that was never loaded")

    def load(self, desc):
        for img in desc.images:
            self.add_image(img)
        for smp in desc.samplers:
            self.add_sampler(*smp)
        for m in desc.meshes:
            self.add_mesh(m.key, m.vertices, m.indices, m.material)
        self.set_instances(desc.instances)
        return self

    def set_brute_force(self, on):
        lib().orc_scene_set_brute_force(self._h, C.c_int(1 if on else 0))

    def set_read_log(self, log):
        """Test aid: `log`, a C-contiguous int32 array [height, width, 4], receives per pixel the temporal-history reads
        (pcx, pcy, gx, gy) that the following trace_ris calls compute, before their in-image test, NO_READ where the temporal
        branch is not taken; None switches the log off (the default: nothing changes)."""
        if log is not None:
            assert log.dtype == np.int32 and log.flags["C_CONTIGUOUS"] and log.shape[-1] == 4
        self._read_log = log
        lib().orc_scene_set_read_log(self._h, None if log is None else _p(log))

    def set_branch_log(self, log):
        """Test aid: `log`, a C-contiguous uint32 array [height, width, 2], receives per pixel the branch outcomes the following
        trace_ris (word 0, RIS_BITS) and trace_final (word 1, FINAL_BITS) calls take; each pass clears its word of a pixel before
        it starts on it. None switches the log off (the default: nothing changes)."""
        if log is not None:
            assert log.dtype == np.uint32 and log.flags["C_CONTIGUOUS"] and log.shape[-1] == 2
        self._branch_log = log
        lib().orc_scene_set_branch_log(self._h, None if log is None else _p(log))

    def tables(self):
        tp, ip, ep = C.c_void_p(), C.c_void_p(), C.c_void_p()
        nt, nl, ne, ntri = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        lib().orc_scene_get_tables(self._h, C.byref(tp), C.byref(nt), C.byref(ip), C.byref(nl), C.byref(ep), C.byref(ne), C.byref(ntri))
        def arr(ptr, n, dt):
            if n == 0:
                return np.zeros(0, dtype=dt)
            buf = (C.c_char * (n * dt.itemsize)).from_address(ptr.value)
            return np.frombuffer(buf, dtype=dt).copy()
        return {"transforms": arr(tp, nt.value, abi.TRANSFORM), "indirection": arr(ip, nl.value, abi.EMISSIVE_INDIRECTION),
                "emissive_triangles": arr(ep, ne.value, abi.EMISSIVE_TRIANGLE), "num_lights": nl.value,
                "n_triangles": ntri.value}

    def trace_closest(self, rays):
        rays = np.ascontiguousarray(rays, dtype=abi.RAY)
        hits = np.zeros(len(rays), dtype=abi.HIT)
        lib().orc_trace_closest(self._h, _p(rays), C.c_uint32(len(rays)), _p(hits))
        return hits

    def trace_any(self, rays):
        rays = np.ascontiguousarray(rays, dtype=abi.RAY)
        occ = np.zeros(len(rays), dtype=np.uint32)
        lib().orc_trace_any(self._h, _p(rays), C.c_uint32(len(rays)), _p(occ))
        return occ

    def shade_closest_hit(self, hits):
        hits = np.ascontiguousarray(hits, dtype=abi.HIT)
        out = np.zeros(len(hits), dtype=abi.RAY_PAYLOAD)
        lib().orc_shade_closest_hit(self._h, _p(hits), C.c_uint32(len(hits)), _p(out))
        return out

    def any_hit_ignores(self, hits):
        out = np.zeros(len(hits), dtype=np.uint32)
        lib().orc_any_hit(self._h, _p(hits), C.c_uint32(len(hits)), _p(out))
        return out

    def _params(self, frame, matrices, frame_count, config, tile=None):
        p = abi.SrRtParams()
        p.scene = None
        p.raw_color = frame.raw_color.ctypes.data
        p.depth_img = frame.depth.ctypes.data
        p.normal_img = frame.normal.ctypes.data
        p.diffuse_img = frame.diffuse.ctypes.data
        p.motion_vec_img = frame.motion.ctypes.data
        self._m = matrices
        p.matrices = C.pointer(matrices)
        p.blue_noise_tex = frame.blue_noise.ctypes.data
        p.blue_noise_h, p.blue_noise_w = frame.blue_noise.shape[:2]
        p.reservoirs[0], p.reservoirs[1] = frame.reservoirs[0].ctypes.data, frame.reservoirs[1].ctypes.data
        p.reservoirs_gi[0], p.reservoirs_gi[1] = frame.reservoirs_gi[0].ctypes.data, frame.reservoirs_gi[1].ctypes.data
        p.primary_payload = frame.primary.ctypes.data     # written by trace_ris for the tests, never read by trace_final
        p.frame_count = frame_count
        p.use_srgb = 0
        p.width, p.height = frame.width, frame.height
        if tile:                      # (y0, h) rows, or (y0, h, x0, w) rows x columns; h == 0 / w == 0: all of them
            p.tile_y0, p.tile_h = tile[0], tile[1]
            if len(tile) == 4:
                p.tile_x0, p.tile_w = tile[2], tile[3]
        p.config = config
        return p

    def trace_ris(self, frame, matrices, frame_count, config=None, tile=None):
        p = self._params(frame, matrices, frame_count, config or abi.SrTraceConfig.reference(), tile)
        lib().orc_trace_ris(self._h, C.byref(p))

    def trace_final(self, frame, matrices, frame_count, config=None, tile=None):
        p = self._params(frame, matrices, frame_count, config or abi.SrTraceConfig.reference(), tile)
        lib().orc_trace_final(self._h, C.byref(p))

    def reset_counters(self):
        lib().orc_reset_counters(self._h)

    def counters(self):
        c = abi.SrRayCounters()
        lib().orc_read_counters(self._h, C.byref(c))
        return c


class HostFrame:
    """Frame buffers in host memory with the layouts of SrRtParams (numpy)."""

    def __init__(self, width, height, blue_noise):
        self.width, self.height = width, height
        n = width * height
        self.raw_color = np.zeros((n, 4), dtype=np.float32)
        self.depth = np.zeros(n, dtype=np.uint16)
        self.normal = np.zeros(n, dtype=np.uint32)
        self.diffuse = np.zeros(n, dtype=np.uint32)
        self.motion = np.zeros(n, dtype=np.uint32)
        self.reservoirs = [np.zeros(n, dtype=abi.RESERVOIR), np.zeros(n, dtype=abi.RESERVOIR)]
        self.reservoirs_gi = [np.zeros(n, dtype=abi.RESERVOIR_GI), np.zeros(n, dtype=abi.RESERVOIR_GI)]
        self.blue_noise = np.ascontiguousarray(blue_noise, dtype=np.uint8)
        self.accum = [np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)]
        self.denoise = [np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)]
        self.output = np.zeros(n, dtype=np.uint32)
        self.primary = np.zeros(n, dtype=abi.RAY_PAYLOAD)     # camera-ray payloads as trace_ris sees them (test aid)


def post_chain(frame, frame_count, exposure=1.0, denoise_passes=4, stages=("temporal", "denoise", "tonemap")):
    """The oracle's temporal_accumulation -> a-trous denoise -> postprocess on a HostFrame."""
    p = abi.post_params(frame, frame_count, lambda a: a.ctypes.data, exposure, denoise_passes)
    if "temporal" in stages:
        lib().orc_post_temporal(C.byref(p))
    if "denoise" in stages:
        lib().orc_post_denoise(C.byref(p))
    if "tonemap" in stages:
        lib().orc_post_tonemap(C.byref(p))


def camera_matrices(pos, target, fov_y, width, height, prev_view_proj=None):
    m = abi.SrMatrices()
    prev = None
    if prev_view_proj is not None:
        prev = (C.c_float * 16)(*[float(x) for x in prev_view_proj])
    lib().orc_camera_matrices(_f3(pos), _f3(target), C.c_float(fov_y), C.c_uint32(width), C.c_uint32(height), prev, C.byref(m))
    return m
