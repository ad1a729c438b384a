"""CUBICSPLINE sampling on the host (the loader under SR_CUBICSPLINE_SAMPLE and the host rules over baked cubic clips) under
AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program (tests/native/clip_spline_asan.cpp, g++, host sources
only): the default's refusals, the bit chain from the loader through the clip, and the blend host rules at the end weights, over
the committed fixtures. Nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sunray_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden")
FLAGS = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-pthread"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


def test_spline_host_rule_under_sanitizers(tmp_path):
    exe = str(tmp_path / "clip_spline_asan")
    subprocess.check_call(["g++"] + FLAGS + ["-I", CSRC, os.path.join(ROOT, "tests", "native", "clip_spline_asan.cpp"), os.path.join(CSRC, "gltf_load.cpp"),
                                             os.path.join(CSRC, "clip_host.cpp"), os.path.join(CSRC, "jpeg_decode.cpp"), "-lz", "-o", exe])
    out = subprocess.run([exe] + [os.path.join(GOLDEN, name) for name in ("spline_rig.glb", "skinned_bar.glb", "morph_bar.glb")], capture_output=True, text=True, env=ENV)
    assert out.returncode == 0 and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stdout + out.stderr[-3000:]
    assert "clip spline ok: " in out.stdout
    samples, weights = int(out.stdout.split()[3]), int(out.stdout.split()[6])
    assert samples > 2000 and weights > 100, out.stdout
