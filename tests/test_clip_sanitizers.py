"""sr_gltf_bake_clip and the host rule (sr_clip_sample_host / sr_clip_compose_host / sr_clip_pose_host) under AddressSanitizer +
UndefinedBehaviorSanitizer, as a stand-alone program (tests/native/clip_asan.cpp, g++, host sources only): the fixture, whose
baked clips must agree with sr_gltf_pose byte for byte, the variants a bake refuses, and byte-level mutants that may be refused
anywhere but must not crash. Nothing is loaded into Python."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sunray_amd", "csrc")
FLAGS = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-pthread"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


def test_bake_and_host_rule_under_sanitizers(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_clip_gltf
    exe = str(tmp_path / "clip_asan")
    subprocess.check_call(["g++"] + FLAGS + ["-I", CSRC, os.path.join(ROOT, "tests", "native", "clip_asan.cpp"), os.path.join(CSRC, "gltf_load.cpp"),
                                             os.path.join(CSRC, "clip_host.cpp"), os.path.join(CSRC, "jpeg_decode.cpp"), "-lz", "-o", exe])
    broken = []
    for name in make_clip_gltf.VARIANTS:
        broken.append(str(tmp_path / (name + ".glb")))
        make_clip_gltf.build(name).write_glb(broken[-1])
    out = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "clip_rig.glb"), str(tmp_path / "m.glb"), "1500"] + broken,
                         capture_output=True, text=True, env=ENV)
    assert out.returncode == 0 and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stdout + out.stderr[-3000:]
    assert "clip ok: %d broken variants" % len(make_clip_gltf.VARIANTS) in out.stdout
    assert int(out.stdout.split(",")[-1].split()[0]) > 100, out.stdout      # many mutants still open and go through the bake
