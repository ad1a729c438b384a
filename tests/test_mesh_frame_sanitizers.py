"""The host side of the mesh frame (sr_mesh_frame_adjacency, sr_mesh_frame_host: csrc/mesh_frame.cpp) under AddressSanitizer +
UndefinedBehaviorSanitizer, as a stand-alone program (tests/native/mesh_frame_asan.cpp, g++, that one host source only): hand-made
meshes, an index out of range, an index count that is no triangle list, zero vertices, counting calls with NULL outputs, and a few
hundred seeded random small meshes. The bad inputs are refused, nothing crashes, the sanitizers stay silent."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sunray_amd", "csrc")
FLAGS = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


def test_mesh_frame_host_side_under_sanitizers(tmp_path):
    exe = str(tmp_path / "mesh_frame_asan")
    subprocess.check_call(["g++"] + FLAGS + ["-I", CSRC, os.path.join(ROOT, "tests", "native", "mesh_frame_asan.cpp"), os.path.join(CSRC, "mesh_frame.cpp"), "-o", exe])
    out = subprocess.run([exe, "300"], capture_output=True, text=True, env=ENV)
    assert out.returncode == 0 and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stdout[-3000:] + out.stderr[-3000:]
    assert "mesh_frame ok: 5 hand-made meshes, 300 random meshes" in out.stdout, out.stdout
