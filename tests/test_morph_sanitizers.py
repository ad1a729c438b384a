"""The glTF loader's morph read-outs (sr_gltf_blas_morph, sr_gltf_morph_weights) under AddressSanitizer + UndefinedBehaviorSanitizer,
as a stand-alone program (tests/native/morph_asan.cpp, g++, host sources only): the fixture, broken variants of it that must be
refused by the new calls and never by sr_gltf_open, and byte-level mutants that may be refused anywhere but must not crash."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sunray_amd", "csrc")
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-pthread"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


def test_morph_read_outs_under_sanitizers(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_morph_gltf
    exe = str(tmp_path / "morph_asan")
    subprocess.check_call(["g++"] + FLAGS + ["-I", CSRC, os.path.join(ROOT, "tests", "native", "morph_asan.cpp"), os.path.join(CSRC, "gltf_load.cpp"),
                                             os.path.join(CSRC, "jpeg_decode.cpp"), "-lz", "-o", exe])
    broken = []
    for name in make_morph_gltf.VARIANTS:
        broken.append(str(tmp_path / (name + ".glb")))
        make_morph_gltf.build(name).write_glb(broken[-1])
    out = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "morph_bar.glb"), str(tmp_path / "m.glb"), "1500"] + broken,
                         capture_output=True, text=True, env=ENV)
    assert out.returncode == 0 and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stdout + out.stderr[-3000:]
    assert "morph ok: %d broken variants" % len(make_morph_gltf.VARIANTS) in out.stdout
    assert int(out.stdout.split(",")[-1].split()[0]) > 100, out.stdout      # many mutants still open and go through the new calls
