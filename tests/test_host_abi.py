"""CPU-side checks of the product library: it loads, exports every symbol include/sunray_hip.h
declares, its host-side data preparation (H1..H6) equals the oracle's, the BVH builder produces a
valid tree, and device entry points fail loudly without a GPU. No compute calls need a GPU here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from sunray_amd import _lib, abi, runtime as rt, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def has_gpu():
    import torch
    return torch.cuda.is_available()


def test_library_exports_every_declared_symbol():
    header = open(os.path.join(ROOT, "include", "sunray_hip.h")).read()
    declared = set(re.findall(r"\b(sr_[a-z0-9_]+)\s*\(", header))
    assert declared == set(_lib.SYMBOLS), declared ^ set(_lib.SYMBOLS)
    L = _lib.lib()
    for name in declared:
        assert hasattr(L, name), name
    assert L.sr_version() == 1


def test_abi_struct_sizes_match_header():
    assert C.sizeof(abi.SrRtParams) == 184 and C.sizeof(abi.SrTraceConfig) == 40 and C.sizeof(abi.SrMatrices) == 256
    assert C.sizeof(abi.SrRayCounters) == 48 and C.sizeof(abi.SrStripRects) == 56 and C.sizeof(abi.SrStripTransfer) == 16
    assert C.sizeof(abi.SrStripPlane) == 16 and abi.SrStripPlane.bpp.offset == 8
    assert abi.SrRtParams.primary_payload.offset == 104 and abi.SrRtParams.frame_count.offset == 112
    cfg = abi.SrTraceConfig()
    _lib.lib().sr_trace_config_default(C.byref(cfg))
    ref = abi.SrTraceConfig.reference()
    assert bytes(cfg) == bytes(ref)
    assert (cfg.max_bounces, cfg.shadow_bounces, cfg.ris_candidates, cfg.virtual_bounces, cfg.enable_restir) == (10, 5, 16, 20, 1)


def test_camera_matrices_match_oracle_and_closed_form(oracle):
    for pos, tgt, fov, w, h in [((0, 0, 1), (0, 0, 0), 45.0, 256, 256), ((13, 30, 25), (0, 13, 0), 45.0, 1600, 1200),
                                ((0.0, 11.0, 21.0), (0.0, 0.5, 0.0), 60.0, 1920, 1080)]:
        a = rt.camera_matrices(pos, tgt, fov, w, h)
        b = oracle.camera_matrices(pos, tgt, fov, w, h)
        assert bytes(a) == bytes(b)
        vi = np.array(list(a.view_inverse)).reshape(4, 4)
        pi = np.array(list(a.proj_inverse)).reshape(4, 4)
        vp = np.array(list(a.view_proj)).reshape(4, 4)
        assert not np.array(list(a.prev_view_proj)).any()          # zero on the first frame (lib.rs:410)
        assert np.allclose(vi[:3, 3], pos, atol=1e-5)              # origin = V^-1 (0,0,0,1)
        # SURVEY §8a H1 closed form: P^-1 (dx,dy,1,1).xyz = (dx*aspect*tan, -dy*tan, -1)
        t = np.tan(np.radians(fov) / 2)
        v = pi @ np.array([0.3, -0.7, 1, 1])
        assert np.allclose(v[:3], [0.3 * (w / h) * t, 0.7 * t, -1], atol=1e-5) and abs(v[3] - 0.01) < 1e-4
        # view_proj * (target) lands on the optical axis
        c = vp @ np.array(list(tgt) + [1.0])
        assert abs(c[0] / c[3]) < 1e-4 and abs(c[1] / c[3]) < 1e-4
    a2 = rt.camera_matrices((0, 0, 1), (0, 0, 0), 45.0, 256, 256, prev_view_proj=list(a.view_proj))
    assert list(a2.prev_view_proj) == list(a.view_proj)
    with pytest.raises(_lib.SunrayError):
        rt.camera_matrices((0, 0, 1), (0, 0, 0), 45.0, 0, 256)


def test_material_and_emissive_derivation_match_oracle(oracle):
    m = rt.material_new((0.1, 0.2, 0.3, 1.0), 0.4, 0.6, (1.0, 0.5, 0.25), 3.0, 0.7, 1.45)
    mo = np.zeros((), dtype=abi.MATERIAL)
    oracle.lib().orc_material_new((C.c_float * 4)(0.1, 0.2, 0.3, 1.0), C.c_float(0.4), C.c_float(0.6), (C.c_float * 3)(1.0, 0.5, 0.25),
                                  C.c_float(3.0), C.c_float(0.7), C.c_float(1.45), mo.ctypes.data_as(C.c_void_p))
    assert m.tobytes() == mo.tobytes() == abi.material((0.1, 0.2, 0.3, 1.0), 0.4, 0.6, (1.0, 0.5, 0.25), 3.0, 0.7, 1.45).tobytes()
    assert m["alpha_mode"] == 0 and m["alpha_cutoff"] == 0 and m["normal_image"] == abi.NULL_TEXTURE  # material.rs:74-75
    v, i = scenes.quad((-0.3, 1.99, -0.3), (0.3, 1.99, -0.3), (0.3, 1.99, 0.3), (-0.3, 1.99, 0.3), (0, -1, 0))
    et = rt.emissive_triangles_from_mesh(v, i, m)
    assert len(et) == 2 and np.allclose(et[0]["emission"], [3.0, 1.5, 0.75, 0.0])   # factor * strength (lib.rs:901-906)
    assert np.allclose(et[1]["v2"], [-0.3, 1.99, 0.3, 0.0])
    # not emissive when every component of factor*strength is <= 0 (lib.rs:907)
    assert len(rt.emissive_triangles_from_mesh(v, i, abi.material(emissive_factor=(1, 1, 1), emissive_strength=0.0))) == 0
    # count query (out = NULL, cap = 0) is fine; out = NULL with cap > 0 is a caller bug, not a silent no-op
    from sunray_amd._lib import lib, SunrayError, check
    vv, ii, mm = np.ascontiguousarray(v, dtype=abi.VERTEX), np.ascontiguousarray(i, dtype=np.uint32), np.ascontiguousarray(m, dtype=abi.MATERIAL)
    n = C.c_uint32()
    args = (vv.ctypes.data_as(C.c_void_p), C.c_uint32(len(vv)), ii.ctypes.data_as(C.c_void_p), C.c_uint32(len(ii)), mm.ctypes.data_as(C.c_void_p))
    check(lib().sr_emissive_triangles_from_mesh(*args, None, C.c_uint32(0), C.byref(n)))
    assert n.value == 2
    with pytest.raises(SunrayError) as e:
        check(lib().sr_emissive_triangles_from_mesh(*args, None, C.c_uint32(4), C.byref(n)))
    assert e.value.code == -1 and "cap > 0" in e.value.description


def _world_tris(desc):
    out = []
    meshes = {m.key: m for m in desc.meshes}
    for key, xs in desc.instances:
        m = meshes[key]
        P = m.vertices["position"].astype(np.float32)
        for x in xs:
            M = np.asarray(x, dtype=np.float32).reshape(3, 4)
            W = (P @ M[:, :3].T + M[:, 3]).astype(np.float32)
            t = W[m.indices.reshape(-1, 3)]
            out.append(np.concatenate([t[:, 0], t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]], axis=1))
    return np.concatenate(out).astype(np.float32)


def _check_bvh(nodes, tris, max_depth, max_stack, stack_limit=31):
    """Walks the quantised wide nodes exactly as the kernel decodes them (traverse.h, bvh_layout.h)."""
    W = rt.bvh_layout()[0]
    n = len(tris)
    seen = np.zeros(n, dtype=int)
    depth_seen = [0]
    slack = [0.0]

    def rec(node, depth):
        depth_seen[0] = max(depth_seen[0], depth)
        lo4, hi4, ch = rt.decode_node(nodes[node])
        lo_all, hi_all = np.full(3, np.inf), np.full(3, -np.inf)
        stack_below, n_real = 0, 0
        for c in range(W):
            lo, hi = lo4[c], hi4[c]
            if ch[c] >= 0:
                assert ch[c] > node  # children always follow their parent (depth-first on the host, breadth-first on the device)
                l2, h2, sb = rec(int(ch[c]), depth + 1)
                stack_below = max(stack_below, sb)
            else:
                v = (~int(ch[c])) & 0xFFFFFFFF
                first, cnt = v >> 3, v & 7
                assert cnt <= 4
                if cnt == 0:
                    assert (lo > hi).all()  # unused child decodes to an inverted box
                    continue
                tt = tris[first:first + cnt]
                seen[first:first + cnt] += 1
                p0 = tt[:, 0:3]
                allp = np.concatenate([p0, p0 + tt[:, 3:6], p0 + tt[:, 6:9]])
                l2, h2 = allp.min(0), allp.max(0)
            n_real += 1
            # every decoded box strictly contains the GEOMETRY below it (a descendant's decoded box may
            # stick out of an ancestor's: each level rounds outward on its own grid)
            assert (lo < l2).all() and (hi > h2).all()
            ext = np.maximum(hi4[ch_real(ch)].max(0) - lo4[ch_real(ch)].min(0), 1e-30)
            slack[0] = max(slack[0], float((((l2 - lo) + (hi - h2)) / ext).max()))
            lo_all, hi_all = np.minimum(lo_all, l2), np.maximum(hi_all, h2)
        return lo_all, hi_all, stack_below + max(n_real - 1, 0)

    def ch_real(ch):
        return np.array([c >= 0 or ((~int(c)) & 7) != 0 for c in ch])

    _, _, need = rec(0, 1)
    assert (seen == 1).all()
    assert sorted(tris[:, 9].view(np.uint32)) == list(range(n))
    assert depth_seen[0] == max_depth
    assert need == max_stack <= stack_limit   # kStackMax (traverse.h): the builder narrows nodes where the budget is tight
    return slack[0]


@pytest.mark.parametrize("scene_fn", [scenes.cornell_box, scenes.cornell_glass_mirror, lambda: scenes.heightfield(n=64, n_lights=3)])
def test_host_bvh_is_a_valid_tree(scene_fn):
    w = _world_tris(scene_fn())
    _check_bvh(*rt.host_bvh(w))


def test_host_bvh_small_and_degenerate_inputs():
    w = _world_tris(scenes.cornell_box())
    for k in (0, 1, 3, 4, 5, 9):
        nodes, tris, md, ms = rt.host_bvh(w[:k])
        assert len(tris) == k and len(nodes) >= 1  # the root is always an inner node
        _check_bvh(nodes, tris, md, ms)
    # 5000 identical triangles: SAH cannot split, the median fallback must keep depth bounded
    same = np.tile(w[:1], (5000, 1))
    _check_bvh(*rt.host_bvh(same))
    # a long line of tiny triangles: depth guard
    line = np.tile(w[:1], (3000, 1))
    line[:, 0] += np.arange(3000, dtype=np.float32) ** 2
    _check_bvh(*rt.host_bvh(line))


def test_device_entry_points_fail_loudly_without_gpu():
    if has_gpu():
        pytest.skip("GPU present")
    with pytest.raises(_lib.SunrayError) as e:
        rt.Scene(0)
    assert e.value.code == -2 and "hip" in e.value.description.lower()
    p = abi.SrRtParams()
    L = _lib.lib()
    assert L.sr_trace_ris(C.byref(p), None) == -1 and b"scene is null" in L.sr_last_error()
    assert L.sr_trace_final(None, None) == -1
    assert L.sr_trace_closest(None, None, 0, None, None) == -1


def test_default_noise_texture_equals_scene_generator():
    for w, h, seed in [(128, 128, 7), (16, 8, 3), (1, 1, 0)]:
        assert (rt.default_noise_texture(w, h, seed) == scenes.white_noise_rgba8(w, h, seed)).all()
    assert _lib.lib().sr_default_noise_texture(0, 4, 1, None) == -1


def test_renderer_argument_errors_and_no_gpu_failure():
    L = _lib.lib()
    h = C.c_void_p()
    assert L.sr_renderer_create(0, 0, 16, C.byref(h)) == -1 and b"Renderer::new" in L.sr_last_error()
    assert L.sr_renderer_create(0, 16, 16, None) == -1
    assert L.sr_renderer_resize(None, 4, 4) == -1
    assert L.sr_renderer_load_mesh(None, C.c_uint64(1), None, 0, None, 0, None) == -1
    assert L.sr_renderer_render(None, None, None, C.c_float(45.0), None, None, 0, None, None, None) == -1
    assert L.sr_renderer_wait_frame(None, C.c_uint64(0)) == -1
    assert L.sr_renderer_render_to_host_memory(None, None, None, C.c_float(45.0), None, None, 0, None, None) == -1
    assert L.sr_renderer_destroy(None) == 0
    if not has_gpu():
        with pytest.raises(_lib.SunrayError) as e:   # no CPU fallback: creation itself fails without a device
            rt.Renderer((32, 32))
        assert e.value.code == -2


class AsStateRef:
    """acceleration_structure/mod.rs:62-148 restated in Python (MAX_UPDATES_BEFORE_REBUILD = 8, FRAMES_TO_SETTLE = 16)."""

    def __init__(self, build_type):
        self.changing = build_type == abi.BUILD_RAPIDLY_CHANGING
        self.quiet = self.updates = 0

    def next_op(self, changed):
        if not self.changing:
            return abi.OP_UPDATE if changed else abi.OP_NONE
        if changed:
            return abi.OP_FAST_BUILD if self.updates >= 8 else abi.OP_UPDATE
        return abi.OP_SLOW_BUILD if self.quiet + 1 >= 16 else abi.OP_NONE

    def mark_built(self, op):
        if op == abi.OP_UPDATE:
            if self.changing:
                self.updates += 1; self.quiet = 0
            else:
                self.changing, self.quiet, self.updates = True, 0, 1
        elif op == abi.OP_FAST_BUILD:
            self.changing, self.quiet, self.updates = True, 0, 0
        elif op == abi.OP_SLOW_BUILD:
            self.changing, self.quiet, self.updates = False, 0, 0
        elif self.changing:
            self.quiet += 1


def test_as_state_heuristic_matches_restatement_and_documented_behaviour():
    L = _lib.lib()
    rng = np.random.default_rng(4)
    for build_type in (abi.BUILD_RAPIDLY_CHANGING, abi.BUILD_SOMETIMES_CHANGES, abi.BUILD_STATIC):
        st, ref = abi.SrAsState(), AsStateRef(build_type)
        L.sr_as_state_initial(build_type, C.byref(st))
        for changed in rng.random(600) < np.repeat(rng.random(30), 20):          # bursts of activity and quiet stretches
            op = L.sr_as_state_next_op(C.byref(st), int(changed))
            assert op == ref.next_op(bool(changed))
            L.sr_as_state_mark_built(C.byref(st), op)
            ref.mark_built(op)
            assert (st.changing, st.frames_without_changes, st.number_of_updates_since_last_rebuild) == (int(ref.changing), ref.quiet, ref.updates)
    # the documented cycle for a structure that changes every frame: 8 updates, then a fast rebuild, repeat
    st = abi.SrAsState()
    L.sr_as_state_initial(abi.BUILD_SOMETIMES_CHANGES, C.byref(st))
    ops = []
    for _ in range(20):
        op = L.sr_as_state_next_op(C.byref(st), 1); L.sr_as_state_mark_built(C.byref(st), op); ops.append(op)
    U, F, S, N = abi.OP_UPDATE, abi.OP_FAST_BUILD, abi.OP_SLOW_BUILD, abi.OP_NONE
    assert ops == [U] * 8 + [F] + [U] * 8 + [F] + [U] * 2
    # then quiet: 15 idle frames, the 16th settles with a quality rebuild, afterwards nothing
    ops = []
    for _ in range(18):
        op = L.sr_as_state_next_op(C.byref(st), 0); L.sr_as_state_mark_built(C.byref(st), op); ops.append(op)
    assert ops == [N] * 15 + [S] + [N] * 2 and st.changing == 0


def test_strip_partition_and_plans_equal_the_python_originals():
    """csrc/multi_gpu.cpp (sr_partition_*, sr_balanced_bounds, sr_axis_cost_from_tiles, sr_history_exchange_plan, sr_strip_rects)
    against the Python implementations of rounds 1-2 (tests/strip_reference.py): world sizes 2, 3, 4, 8, both axes, equal and
    cost-balanced cuts, motion halos 0 / 7 / 40, on the bench extent and a ragged one; then the error behaviour."""
    import strip_reference as ref
    from sunray_amd import distributed as sd
    rng = np.random.default_rng(11)
    assert sd.SPATIAL_HALO == ref.SPATIAL_HALO == abi.SPATIAL_HALO == 30
    for W, H in ((1920, 1080), (203, 77), (64, 4096)):
        for axis in ("cols", "rows"):
            length = W if axis == "cols" else H
            tiles_x, tiles_y = (W + 7) // 8, (H + 7) // 8
            tile_costs = rng.integers(0, 1 << 20, size=tiles_x * tiles_y).astype(np.float64)
            tile_costs[rng.random(tile_costs.size) < 0.3] = 0.0                       # sky tiles
            cost_ref = ref.axis_cost_from_tiles(tile_costs, tiles_x, axis, length)
            cost = sd.axis_cost_from_tiles(tile_costs, tiles_x, axis, length)
            assert cost.shape == cost_ref.shape and (cost == cost_ref).all()
            for world in (2, 3, 4, 8):
                for min_size, max_share in ((8, 2.5), (32, 2.5), (1, 1.2)):
                    assert sd.balanced_bounds(cost, world, min_size, max_share) == ref.balanced_bounds(cost_ref, world, min_size, max_share)
                for bounds in (None, ref.balanced_bounds(cost_ref, world, min_size=sd.SPATIAL_HALO + 2)):
                    a, b = sd.Partition(W, H, world, axis, bounds), ref.Partition(W, H, world, axis, bounds)
                    assert a.bounds == b.bounds and a.sizes() == b.sizes() and a.length == b.length
                    for rank in range(world):
                        assert a.span(rank) == b.span(rank)
                        for grow in (0, 30, 37, 70, 5000):
                            assert a.grown(rank, grow) == b.grown(rank, grow)
                        a0, n = b.span(rank)
                        assert a.tile(a0, n) == b.tile(a0, n)
                        # launch rectangles: RIS over strip + spatial halo with the counting window on the strip, final pass on the strip
                        r = a.rects(rank)
                        g0, gn = b.grown(rank, ref.SPATIAL_HALO)
                        assert (r.ris_y0, r.ris_h, r.ris_x0, r.ris_w) == b.tile(g0, gn) and (r.final_y0, r.final_h, r.final_x0, r.final_w) == b.tile(a0, n)
                        assert r.empty == (1 if n == 0 else 0) and r.count_window == (1 if n > 0 else 0)
                        if n > 0:
                            assert (r.count_x0, r.count_cols, r.count_y0, r.count_rows) == ((a0, n, 0, 0) if axis == "cols" else (0, 0, a0, n))
                    for motion_halo in (0, 7, 40):
                        assert sd.history_exchange_plan(a, motion_halo) == ref.history_exchange_plan(b, motion_halo)
    one = sd.Partition(640, 360, 1, "cols")
    r = one.rects(0)
    assert (r.ris_x0, r.ris_w, r.count_window, r.empty) == (0, 640, 0, 0) and sd.history_exchange_plan(one, 40) == []
    # errors
    L = _lib.lib()
    h = C.c_void_p()
    assert L.sr_partition_create(C.c_uint32(64), C.c_uint32(64), C.c_uint32(0), C.c_uint32(0), None, C.byref(h)) == -1
    assert L.sr_partition_create(C.c_uint32(64), C.c_uint32(64), C.c_uint32(2), C.c_uint32(5), None, C.byref(h)) == -1
    assert L.sr_partition_create(C.c_uint32(64), C.c_uint32(64), C.c_uint32(2), C.c_uint32(0), (C.c_uint32 * 3)(0, 40, 63), C.byref(h)) == -1
    assert L.sr_partition_create(C.c_uint32(64), C.c_uint32(64), C.c_uint32(2), C.c_uint32(0), (C.c_uint32 * 3)(0, 70, 64), C.byref(h)) == -1
    with pytest.raises(ValueError):
        sd.Partition(64, 64, 2, "diag")
    with pytest.raises(ValueError):
        sd.Partition(64, 64, 2, "cols", [0, 10])
    p = sd.Partition(64, 64, 2)
    a, n = C.c_uint32(), C.c_uint32()
    assert L.sr_partition_span(p._h, C.c_uint32(2), C.c_uint32(0), C.byref(a), C.byref(n)) == -1
    cnt = C.c_uint32()
    assert L.sr_history_exchange_plan(p._h, C.c_uint32(4), None, C.c_uint32(3), C.byref(cnt)) == -1       # out == NULL with cap > 0
    assert L.sr_history_exchange_plan(p._h, C.c_uint32(4), None, C.c_uint32(0), C.byref(cnt)) == 0 and cnt.value == 2
    out = (C.c_uint32 * 3)()
    assert L.sr_balanced_bounds((C.c_double * 4)(1.0, float("nan"), 1.0, 1.0), C.c_uint32(4), C.c_uint32(2), C.c_uint32(1), C.c_double(2.5), out) == -1
    assert L.sr_balanced_bounds(None, C.c_uint32(4), C.c_uint32(2), C.c_uint32(1), C.c_double(2.5), out) == -1


def test_missing_library_is_an_import_error(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    monkeypatch.setattr(_lib, "_lib", None)
    with pytest.raises(ImportError):
        _lib.lib()


def test_pass_kernels_stay_inside_their_register_budget():
    """The compiler's own report for the two pass kernels (kept by sunray_amd.build next to the object). One-level variants run
    4 waves per SIMD: at most the handful of registers that are parked once outside the loops may spill. The two-level variants
    run 3 waves per SIMD and must not spill at all: with 35-43 spilled registers in the stealing loop final_kernel<6> gave results
    that depended on unrelated edits."""
    from sunray_amd import build
    res = build.kernel_resources()
    seen = 0
    for name, r in res.items():
        for kind in ("ris_kernelILi", "final_kernelILi"):
            if kind in name:
                v = int(name.split(kind)[1].split("E")[0])
                seen += 1
                if v & 4:
                    assert r["occupancy"] == 3 and r["vgpr_spills"] == 0, (name, r)
                else:
                    assert r["occupancy"] == 4 and r["vgpr_spills"] <= 6, (name, r)
    assert seen == 16
