"""The device's inline helpers (sunray_amd/csrc/rt_device.h, traverse.h) against the oracle's, function by function.

DESIGN.md section 3 rests on the two sides running the same fp32 program. The frames of the parity tests reach each helper only
with the values a render happens to produce; here sr_probe_helper runs one helper per thread on the input sets of
tests/helper_probe.py — float classes (zeros, denormals, infinities, NaN payloads), every exponent, every tie of every
float-to-code conversion, every code of every code-to-float conversion, the cut-offs and denormal results of the pinned
transcendentals, the edge cases of the BRDF, reservoir and triangle helpers — and every row must equal orc_probe_helper's:
integer-coded results in every bit, float results in every bit unless both are NaN (x86 and the GPU make default NaNs of different
sign, and no stored buffer is compared on NaN bits). The oracle's side of the same rows is held against float64 definitions in
test_helper_probe_host.py, so no tolerance is restated here.
Run on an MI355X with:  python -m pytest tests/test_gpu_helper_probe.py -m gpu -q
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from sunray_amd import abi

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(__file__))
import helper_probe as hp  # noqa: E402

SENTINEL = 0xA5C3E10F
TAIL = 256
SR_ERR_INVALID_ARG = -1


@pytest.fixture(scope="module")
def rt():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: run them with -m gpu on an MI355X")
    from sunray_amd import runtime
    return runtime


def to_device(a):
    import torch
    return torch.tensor(np.ascontiguousarray(a).view(np.int32), device="cuda")      # copies: the input sets are read-only


def to_host(t):
    return t.cpu().numpy().view(np.uint32)


def test_row_layouts_match_the_library(rt, oracle):
    from sunray_amd._lib import SunrayError
    assert len(abi.PROBE_HELPERS) == len(hp.LAYOUT)
    for name, fn in hp.IDS.items():
        assert rt.probe_helper_layout(fn) == hp.LAYOUT[name][:2] == oracle.probe_helper_layout(fn), name
    for fn in (len(abi.PROBE_HELPERS), 0xFFFFFFFF):
        with pytest.raises(SunrayError) as e:
            rt.probe_helper_layout(fn)
        assert e.value.code == SR_ERR_INVALID_ARG
        assert oracle.probe_helper_layout(fn) is None


@pytest.mark.parametrize("name", list(hp.IDS))
def test_device_helper_equals_oracle(rt, oracle, name):
    import torch
    rows = hp.input_set(name)
    want = oracle.probe_helper(hp.IDS[name], rows)
    d_in = to_device(rows)
    d_out = torch.zeros(want.size, dtype=torch.int32, device="cuda")
    assert rt.probe_helper(hp.IDS[name], d_in, d_out) == len(rows)
    torch.cuda.synchronize()
    got = to_host(d_out).reshape(want.shape)
    msg = hp.mismatch(name, rows, got, want)
    assert msg is None, msg


@pytest.mark.parametrize("name", ["build_onb", "merge", "intersect_tri"])
def test_probe_kernel_row_counts_and_refusals(rt, oracle, name):
    """The probe kernel itself: for row counts around the wave and block sizes the first n rows are right and the words behind them
    are untouched; an unknown helper, or a null pointer with n > 0, is refused with SR_ERR_INVALID_ARG and writes nothing."""
    import torch
    from sunray_amd._lib import lib
    fn = hp.IDS[name]
    iw, ow, _ = hp.LAYOUT[name]
    rows = np.resize(hp.input_set(name), (100003, iw))          # the set, repeated up to the largest count
    want = oracle.probe_helper(fn, rows)
    d_in = to_device(rows)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    fresh = lambda n: torch.full((n * ow + TAIL,), SENTINEL - (1 << 32), dtype=torch.int32, device="cuda")
    for n in (0, 1, 63, 64, 65, 255, 256, 257, 100003):
        d_out = fresh(n)
        assert lib().sr_probe_helper(C.c_uint32(fn), ptr(d_in), C.c_uint32(n), ptr(d_out), stream) == 0
        torch.cuda.synchronize()
        got = to_host(d_out)
        assert (got[n * ow:] == SENTINEL).all(), "%s, n = %d: words behind the last row were written" % (name, n)
        msg = hp.mismatch(name, rows[:n], got[:n * ow].reshape(n, ow), want[:n])
        assert msg is None, "n = %d: %s" % (n, msg)
    d_out = fresh(64)
    refused = [(len(abi.PROBE_HELPERS), ptr(d_in), 64, ptr(d_out)), (0xFFFFFFFF, ptr(d_in), 64, ptr(d_out)),
               (fn, None, 64, ptr(d_out)), (fn, ptr(d_in), 64, None), (fn, None, 1, None)]
    for f, i, n, o in refused:
        assert lib().sr_probe_helper(C.c_uint32(f), i, C.c_uint32(n), o, stream) == SR_ERR_INVALID_ARG
        assert lib().sr_last_error()
    assert lib().sr_probe_helper(C.c_uint32(fn), None, C.c_uint32(0), None, stream) == 0        # nothing to do: no pointer is read
    torch.cuda.synchronize()
    assert (to_host(d_out) == SENTINEL).all()
