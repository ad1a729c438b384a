"""The host side of sr_scene_set_instances_device (csrc/host_prep.cpp: instance_tables_host, frame_instance_layout,
frame_instance_transforms, instance_list_sizes / instance_list_limits) under AddressSanitizer + UndefinedBehaviorSanitizer, as a
stand-alone program (tests/native/instances_asan.cpp, g++, that one host source only): no instance, one, 774 over four entries,
2^20, and counts that sum to just under and to exactly the 2^28-instance limit. Nothing crashes, the sanitizers stay silent."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sunray_amd", "csrc")
FLAGS = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


def test_instance_host_side_under_sanitizers(tmp_path):
    exe = str(tmp_path / "instances_asan")
    subprocess.check_call(["g++"] + FLAGS + ["-I", CSRC, os.path.join(ROOT, "tests", "native", "instances_asan.cpp"), os.path.join(CSRC, "host_prep.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, env=ENV)
    assert out.returncode == 0 and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stdout[-3000:] + out.stderr[-3000:]
    assert "instances ok: layouts of 0, 0, 1, 774 and 1048576 instances, limits at 2^28" in out.stdout, out.stdout
