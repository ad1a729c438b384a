"""The host side of the node-step probe (sr_probe_node_step's row validation and packing: csrc/node_probe_rows.cpp) under
AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program (tests/native/node_probe_asan.cpp, g++, that one host source
only): row counts around the wave and workgroup sizes in every kind with every array at its exact size, every child word the hook
must refuse in the first, a middle and the last row, null pointers, unknown kinds. The bad inputs are refused, the packed arrays
are the rows' parts, nothing crashes, the sanitizers stay silent."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sunray_amd", "csrc")
FLAGS = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


def test_node_probe_host_side_under_sanitizers(tmp_path):
    exe = str(tmp_path / "node_probe_asan")
    subprocess.check_call(["g++"] + FLAGS + ["-I", CSRC, os.path.join(ROOT, "tests", "native", "node_probe_asan.cpp"), os.path.join(CSRC, "node_probe_rows.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, env=ENV)
    assert out.returncode == 0 and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stdout[-3000:] + out.stderr[-3000:]
    assert "node_probe ok: 35 packed calls over 5 kinds" in out.stdout, out.stdout
