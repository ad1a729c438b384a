"""The host rule of layered morph weights (sr_clip_layer_weights_host, sr_clip_weights_layers_host) under AddressSanitizer +
UndefinedBehaviorSanitizer, as a stand-alone program (tests/native/clip_layer_weights_asan.cpp, g++, host sources only): stacks of
1..8 layers in every mode / mask / interpolation mix of the committed fixtures over exactly sized buffers, one layer and two override
layers against the rules they extend byte for byte, and the refusals. Nothing is loaded into Python."""
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


def test_layer_weights_host_rule_under_sanitizers(tmp_path):
    exe = str(tmp_path / "clip_layer_weights_asan")
    subprocess.check_call(["g++"] + FLAGS + ["-I", CSRC, os.path.join(ROOT, "tests", "native", "clip_layer_weights_asan.cpp"), os.path.join(CSRC, "gltf_load.cpp"),
                                             os.path.join(CSRC, "clip_host.cpp"), os.path.join(CSRC, "jpeg_decode.cpp"), "-lz", "-o", exe])
    out = subprocess.run([exe] + [os.path.join(GOLDEN, name) for name in ("morph_bar.glb", "clip_rig.glb")], capture_output=True, text=True, env=ENV)
    assert out.returncode == 0 and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stdout + out.stderr[-3000:]
    assert "clip layer weights ok: " in out.stdout
    assert int(out.stdout.split()[4]) > 1000, out.stdout
