"""The host side of batched posing (sr_pose_batch_plan, abi.SrPoseItem / abi.SrPoseBatchInfo, the argument checks of
Scene.pose_meshes / Renderer.pose_meshes, the compiler's report for pose_batch.hip). Nothing here needs a GPU."""
import ctypes as C
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

from sunray_amd import abi, runtime as rt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_UNSUPPORTED = -5
MESH_SET = (3, 4, 63, 64, 65, 257, 1026, 256, 512)


def plan_restated(counts):
    """sr_pose_batch_plan in numpy: ceil(n / 256) blocks an item, in item order; records packed in item order."""
    counts = np.asarray(counts, dtype=np.uint64)
    blocks = (counts + np.uint64(255)) // np.uint64(256)
    first = np.concatenate([[0], np.cumsum(blocks)[:-1]]).astype(np.uint64) if len(counts) else np.zeros(0, np.uint64)
    base = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.uint64) if len(counts) else np.zeros(0, np.uint64)
    return first, base, int(blocks.sum())


def assert_plan(counts, what):
    first, base, blocks = rt.pose_batch_plan(counts)
    wf, wb, wn = plan_restated(counts)
    assert blocks == wn and np.array_equal(first.astype(np.uint64), wf) and np.array_equal(base, wb), what
    return first, base, blocks


def test_plan_equals_the_restatement():
    first, base, blocks = assert_plan(MESH_SET, "the mesh set")
    assert list(first) == [0, 1, 2, 3, 4, 5, 7, 12, 13] and blocks == 15 and int(base[-1]) == sum(MESH_SET[:-1])
    first, base, blocks = assert_plan([1] * 1000, "1000 items of one vertex")
    assert blocks == 1000 and list(first[:3]) == [0, 1, 2] and list(base[-2:]) == [998, 999]
    for order in itertools.permutations((255, 256, 257)):
        first, _, blocks = assert_plan(order, order)
        assert blocks == 4 and first[1] == (2 if order[0] == 257 else 1)
    assert_plan([0, 5, 0, 256, 0], "items without vertices take no block")
    assert rt.pose_batch_plan([])[2] == 0
    assert_plan([0xFFFFFFFF], "the largest mesh alone")
    assert_plan([0x7FFFFFFF, 0x7FFFFFFF, 1], "2^32 - 1 vertices")


def test_plan_refuses_what_the_launch_cannot_index():
    """Large counts only: the call reads n_items words and writes nothing."""
    first, base = np.full(128, 0xABCDABCD, np.uint32), np.full(128, 0xABCDABCD, np.uint64)
    blocks = C.c_uint32(77)

    def plan(counts):
        counts = np.asarray(counts, dtype=np.uint32)
        return rt.lib().sr_pose_batch_plan(counts.ctypes.data_as(C.c_void_p), C.c_uint32(len(counts)), first.ctypes.data_as(C.c_void_p),
                                           base.ctypes.data_as(C.c_void_p), C.byref(blocks))
    for what, counts, text in (("2^32 vertices", [0x80000000, 0x80000000], "pose_batch_plan: the batch holds 4294967296 vertices, 2^32 or more"),
                               ("2^31 blocks", [0xFFFFFFFF] * 128, "pose_batch_plan: the batch needs 2147483648 blocks, 2^31 or more")):
        assert plan(counts) == ERR_UNSUPPORTED and rt.lib().sr_last_error().decode() == text, (what, rt.lib().sr_last_error())
        assert (first == 0xABCDABCD).all() and (base == 0xABCDABCD).all() and blocks.value == 77, what
    assert plan([0xFFFFFFFF] * 127) == ERR_UNSUPPORTED and b"vertices" in rt.lib().sr_last_error()     # one item fewer: 2^31 - 2^24 blocks pass


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_struct_layouts_match_the_header(tmp_path):
    """ctypes against the compiler's sizeof / offsetof of include/sunray_hip.h."""
    fields = {"SrPoseItem": [f[0] for f in abi.SrPoseItem._fields_], "SrPoseBatchInfo": [f[0] for f in abi.SrPoseBatchInfo._fields_]}
    src = ['#include <cstddef>\n#include <cstdio>\n#include "sunray_hip.h"\nint main() {']
    for name, fs in fields.items():
        src.append('printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        src += ['printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (name, f, name, f) for f in fs]
    src.append("return 0; }")
    cpp, exe = tmp_path / "layout.cpp", tmp_path / "layout"
    cpp.write_text("\n".join(src))
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(cpp), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    want = {}
    for name, fs in fields.items():
        cls = getattr(abi, name)
        want[name] = str(C.sizeof(cls))
        want.update({"%s.%s" % (name, f): str(getattr(cls, f).offset) for f in fs})
    assert got == want
    assert want["SrPoseItem"] == "32" and want["SrPoseBatchInfo"] == "80"


class _Handle:
    """A Scene / Renderer whose handle must never be reached: the checks raise first."""
    def __getattr__(self, name):
        raise AssertionError("the library was reached (%s)" % name)


@pytest.mark.parametrize("method", [rt.Scene.pose_meshes, rt.Renderer.pose_meshes], ids=["Scene", "Renderer"])
def test_argument_checks_raise_before_the_library_is_called(method):
    w, M = np.ones(3, np.float32), np.zeros((2, 12), np.float32)
    cases = {
        "not a sequence": 7,
        "an item that is no tuple": [5],
        "an item of two values": [(1, w)],
        "neither stage": [(1, w, M), (2, None, None)],
        "float64 weights": [(1, w.astype(np.float64), None)],
        "weights in two dimensions": [(1, w.reshape(1, 3), None)],
        "no weights": [(1, np.zeros(0, np.float32), None)],
        "a list of weights": [(1, [1.0, 0.0], None)],
        "float64 matrices": [(1, None, M.astype(np.float64))],
        "matrices of another shape": [(1, w, np.zeros((2, 16), np.float32))],
        "no joints": [(1, None, np.zeros((0, 12), np.float32))],
    }
    for what, items in cases.items():
        with pytest.raises(ValueError) as e:
            method(_Handle(), items)
        assert str(e.value).startswith("pose_meshes: "), (what, e.value)
    with pytest.raises(ValueError, match="pose_meshes: item 1: pose_mesh: neither weights nor joint matrices given"):
        method(_Handle(), [(1, w, M), (2, None, None)])
    rows, n, keep = rt._pose_items([(2 ** 40 + 1, w, None), (9, None, M.reshape(2, 3, 4))])
    assert n.value == 2 and (rows[0].key, rows[0].n_targets, rows[0].n_joints, rows[0].joint_matrices) == (2 ** 40 + 1, 3, 0, None)
    assert (rows[1].weights, rows[1].n_joints) == (None, 2) and rows[1].joint_matrices == keep[1][1].ctypes.data and rows[0].weights == keep[0][0].ctypes.data


def test_posing_kernels_are_in_the_resource_report():
    """pose_batch.hip, the one source of posing kernels: no scratch, no spills, the LDS tile of 256 vertices at seven 16-byte slots
    each, four waves a SIMD or more, and the registers DESIGN §4 records for pose_batch_kernel; the scatter kernel uses no LDS."""
    from sunray_amd import build
    res = build.kernel_resources("pose_batch.hip")
    pose = [r for name, r in res.items() if "pose_batch_kernel" in name]
    scatter = [r for name, r in res.items() if "pose_batch_scatter_kernel" in name]
    assert len(pose) == 1 and len(scatter) == 1 and len(res) == 2, sorted(res)
    for r in pose + scatter:
        assert r["scratch"] == 0 and r["vgpr_spills"] == 0 and r["sgpr_spills"] == 0 and r["occupancy"] >= 4, r
    assert pose[0]["lds"] == 256 * 7 * 16 and scatter[0]["lds"] == 0
    assert pose[0]["vgprs"] == 44, pose[0]
