"""The host rule of cross-fades between baked clips (sr_clip_blend_compatible, sr_clip_blend_host, sr_clip_compose_records_host,
sr_clip_pose_blend_host, sr_clip_blend_weights_host) under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program
(tests/native/clip_blend_asan.cpp, g++, host sources only): the end weights and a clip blended with itself against the unblended
rule byte for byte, compatibility within a file and across files, and the refusals, over the committed fixtures. Nothing is loaded
into Python."""
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


def test_blend_host_rule_under_sanitizers(tmp_path):
    exe = str(tmp_path / "clip_blend_asan")
    subprocess.check_call(["g++"] + FLAGS + ["-I", CSRC, os.path.join(ROOT, "tests", "native", "clip_blend_asan.cpp"), os.path.join(CSRC, "gltf_load.cpp"),
                                             os.path.join(CSRC, "clip_host.cpp"), os.path.join(CSRC, "jpeg_decode.cpp"), "-lz", "-o", exe])
    out = subprocess.run([exe] + [os.path.join(GOLDEN, name) for name in ("clip_rig.glb", "skinned_bar.glb", "morph_bar.glb")], capture_output=True, text=True, env=ENV)
    assert out.returncode == 0 and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stdout + out.stderr[-3000:]
    assert "clip blend ok: " in out.stdout
    poses, weights = int(out.stdout.split()[3]), int(out.stdout.split()[5])
    assert poses > 2000 and weights > 100, out.stdout
