"""The host side of batched posing (sr_pose_batch_plan and the staging layout: csrc/pose_batch_plan.cpp) under AddressSanitizer +
UndefinedBehaviorSanitizer, as a stand-alone program (tests/native/pose_batch_asan.cpp, g++, that one host source only): the counts
of test_pose_batch_host.py, items without vertices, counts at the 32-bit edge, batches that must be refused with nothing written,
and seeded random batches. Nothing crashes, the sanitizers stay silent."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sunray_amd", "csrc")
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


def test_pose_batch_plan_under_sanitizers(tmp_path):
    exe = str(tmp_path / "pose_batch_asan")
    subprocess.check_call(["g++"] + FLAGS + ["-I", CSRC, os.path.join(ROOT, "tests", "native", "pose_batch_asan.cpp"), os.path.join(CSRC, "pose_batch_plan.cpp"), "-o", exe])
    out = subprocess.run([exe, "300"], capture_output=True, text=True, env=ENV)
    assert out.returncode == 0 and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stdout[-3000:] + out.stderr[-3000:]
    assert "pose_batch ok: 12 plans, 5 refusals, 300 random batches" in out.stdout, out.stdout
