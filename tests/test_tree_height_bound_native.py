"""The height bound's rule restated on the host (tests/native/height_bound.cpp: the device's links / walk / rebuild steps, one loop
iteration per thread) under AddressSanitizer + UndefinedBehaviorSanitizer, over random binary trees and chains and every cap from
H(n) up: the result is a binary tree over the same leaves with h(root) <= cap, kept subtrees are untouched, rebuilt ones are
median-split trees over their own leaves in depth-first order. The product path stays the device kernels."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-pthread"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


def test_height_bound_rule_under_sanitizers(tmp_path):
    exe = str(tmp_path / "height_bound")
    subprocess.check_call(["g++"] + FLAGS + [os.path.join(ROOT, "tests", "native", "height_bound.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, env=ENV)
    assert out.returncode == 0 and "height bound ok" in out.stdout and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, \
        out.stdout + out.stderr[-3000:]
