"""The host rule of layer stacks of baked clips (sr_clip_subtree_mask, sr_clip_layers_host, sr_clip_pose_layers_host) under
AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program (tests/native/clip_layers_asan.cpp, g++, host sources
only): one layer and two override layers against the rules they extend byte for byte, the identities of the rule, stacks of 1..8
layers with subtree masks and additive layers over exactly sized buffers, and the refusals, over the committed fixtures. Nothing is
loaded into Python."""
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


def test_layers_host_rule_under_sanitizers(tmp_path):
    exe = str(tmp_path / "clip_layers_asan")
    subprocess.check_call(["g++"] + FLAGS + ["-I", CSRC, os.path.join(ROOT, "tests", "native", "clip_layers_asan.cpp"), os.path.join(CSRC, "gltf_load.cpp"),
                                             os.path.join(CSRC, "clip_host.cpp"), os.path.join(CSRC, "jpeg_decode.cpp"), "-lz", "-o", exe])
    out = subprocess.run([exe] + [os.path.join(GOLDEN, name) for name in ("clip_rig.glb", "skinned_bar.glb")], capture_output=True, text=True, env=ENV)
    assert out.returncode == 0 and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stdout + out.stderr[-3000:]
    assert "clip layers ok: " in out.stdout
    assert int(out.stdout.split()[3]) > 1000, out.stdout
