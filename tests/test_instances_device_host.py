"""The host side of sr_scene_set_instances_device that needs no GPU: the new symbols, the layout of SrInstanceUpdateInfo, the
null refusals, and sr_instance_tables_host (the one host definition of the DevInstance table) against a numpy float32
restatement of srh::world_to_object_3x3, one operation per statement so that nothing can be fused. Equal means bit for bit;
where the host's own word is a NaN, only "is a NaN" is compared (the rule of the light table's tests)."""
import ctypes as C

import numpy as np

from sunray_amd import abi
from sunray_amd._lib import lib

ERR_INVALID_ARG = -1
F = np.float32


def edge_transforms():
    """The transforms every table test uses at the first and last index, by name."""
    c, s = F(np.cos(0.7)), F(np.sin(0.7))
    denormal = np.array([1], dtype=np.uint32).view(np.float32)[0] * F(4096)         # 2^-137
    t = {
        "identity": [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0],
        "rotation with non-uniform scale": [c * F(2), -s * F(0.5), 0, 3, s * F(2), c * F(0.5), 0, -4, 0, 0, 7, 5],
        "mirror": [-1, 0, 0, 1, 0, 1.5, 0.25, 2, 0, 0, 2, 3],
        "tiny and huge entries": [1e-30, -1e18, 0, 1e18, 1e18, 1e-30, 0, -1e-30, 0, 0, -1e-30, 1e18],
        "negative zeros": [1, -0.0, -0.0, -0.0, -0.0, 2, -0.0, 0, -0.0, -0.0, -3, -0.0],
        "one denormal entry": [1, denormal, 0, 0, 0, 1, 0, 0, 0, 0, 1, denormal],
        "zero scale on one axis": [1, 0, 0, 2, 0, 0, 0, 3, 0, 0, 1, 4],
    }
    return {k: np.array(v, dtype=np.float32) for k, v in t.items()}


def world_to_object_restated(m):
    """srh::world_to_object_3x3 in numpy float32 scalars: adjugate, (a00*c00 + a01*c01) + a02*c02, 1 / det, the products."""
    a00, a01, a02, a10, a11, a12, a20, a21, a22 = (F(m[i]) for i in (0, 1, 2, 4, 5, 6, 8, 9, 10))

    def cof(p, q, r, s):
        x = F(p * q)
        y = F(r * s)
        return F(x - y)
    with np.errstate(all="ignore"):
        c00 = cof(a11, a22, a12, a21)
        c01 = cof(a12, a20, a10, a22)
        c02 = cof(a10, a21, a11, a20)
        p0 = F(a00 * c00)
        p1 = F(a01 * c01)
        p2 = F(a02 * c02)
        s0 = F(p0 + p1)
        det = F(s0 + p2)
        r = F(F(1.0) / det)
        out = [F(c00 * r), F(cof(a02, a21, a01, a22) * r), F(cof(a01, a12, a02, a11) * r),
               F(c01 * r), F(cof(a00, a22, a02, a20) * r), F(cof(a02, a10, a00, a12) * r),
               F(c02 * r), F(cof(a01, a20, a00, a21) * r), F(cof(a00, a11, a01, a10) * r)]
    return np.array(out, dtype=np.float32)


def dev_instances_restated(xf):
    """The DevInstance table of [n, 12] transforms by the restatement: w2o[0..8], o2w[0..8] the 3x3 part, the other words 0."""
    out = np.zeros(len(xf), dtype=abi.DEV_INSTANCE)
    for i, m in enumerate(xf):
        out["w2o"][i, :9] = world_to_object_restated(m)
        out["o2w"][i, :9] = m.reshape(3, 4)[:, :3].ravel()
    return out


def host_tables(xf):
    xf = np.ascontiguousarray(xf, dtype=np.float32).reshape(-1, 12)
    out = np.zeros(max(len(xf), 1), dtype=abi.DEV_INSTANCE)
    assert lib().sr_instance_tables_host(xf.ctypes.data_as(C.c_void_p), C.c_uint32(len(xf)), out.ctypes.data_as(C.c_void_p)) == 0
    return out[:len(xf)]


def assert_words_equal_nan_rule(want, got, what):
    """Bit for bit, except where `want` holds a NaN: there `got` must hold a NaN too, of any payload."""
    w = np.ascontiguousarray(want).view(np.uint32).reshape(-1)
    g = np.ascontiguousarray(got).view(np.uint32).reshape(-1)
    assert w.shape == g.shape, what
    wn, gn = np.isnan(w.view(np.float32)), np.isnan(g.view(np.float32))
    assert np.array_equal(wn, gn), "%s: NaN words differ in %d places" % (what, int((wn != gn).sum()))
    nd = int((w[~wn] != g[~wn]).sum())
    assert nd == 0, "%s: %d of %d words differ" % (what, nd, w.size)


def test_new_symbols_load_and_the_info_struct_is_48_bytes():
    L = lib()
    for name in ("sr_scene_set_instances_device", "sr_scene_instance_update_info", "sr_scene_read_instance_tables", "sr_instance_tables_host",
                 "sr_renderer_render_device_transforms"):
        assert getattr(L, name) is not None
    assert C.sizeof(abi.SrInstanceUpdateInfo) == 48
    assert abi.DEV_INSTANCE.itemsize == 96 and abi.FLAT_INSTANCE.itemsize == 64


def test_null_arguments_are_refused():
    L = lib()
    info = abi.SrInstanceUpdateInfo()
    assert L.sr_scene_set_instances_device(None, None, None, C.c_uint32(0), None, None) == ERR_INVALID_ARG
    assert L.sr_last_error() == b"frame_instance_data: null argument"
    assert L.sr_scene_instance_update_info(None, C.byref(info)) == ERR_INVALID_ARG
    assert L.sr_scene_read_instance_tables(None, None, None) == ERR_INVALID_ARG
    assert L.sr_instance_tables_host(None, C.c_uint32(1), None) == ERR_INVALID_ARG
    assert L.sr_instance_tables_host(None, C.c_uint32(0), None) == 0


def test_host_rule_equals_the_numpy_restatement_bit_for_bit():
    edges = edge_transforms()
    xf = np.stack(list(edges.values()))
    got, want = host_tables(xf), dev_instances_restated(xf)
    for i, name in enumerate(edges):
        assert_words_equal_nan_rule(want[i:i + 1], got[i:i + 1], name)
    # what the edge cases are there for
    assert np.array_equal(got["w2o"][0, :9], np.eye(3, dtype=np.float32).ravel())
    names = list(edges)
    assert not np.isfinite(got["w2o"][names.index("zero scale on one axis"), :9]).all()      # det == 0: inf and NaN words
    assert np.isfinite(got["w2o"][names.index("mirror"), :9]).all()
    assert (got["w2o"][:, 9:] == 0).all() and (got["o2w"][:, 9:] == 0).all()
    # a few hundred general transforms as well
    rng = np.random.default_rng(11)
    xf = rng.normal(size=(300, 12)).astype(np.float32) * np.float32(3.0)
    assert_words_equal_nan_rule(dev_instances_restated(xf), host_tables(xf), "300 random transforms")


def test_instance_tables_kernel_does_not_spill():
    from sunray_amd import build
    res = build.kernel_resources("instances.hip")
    mine = [r for name, r in res.items() if "instance_tables_kernel" in name]
    assert len(mine) == 1, sorted(res)
    assert mine[0]["scratch"] == 0 and mine[0]["vgpr_spills"] == 0 and mine[0]["sgpr_spills"] == 0, mine[0]
    assert mine[0]["lds"] == 256 * (3 + 7) * 16 and mine[0]["occupancy"] >= 4, mine[0]      # the packed transforms and rows of seven pieces
    assert any("light_table_kernel" in name for name in build.kernel_resources("lights.hip"))      # that report is still its own
