"""The device helpers that divide a small integer by 255, 127 or 32767 (rt_device.h, div_small_int_exact) over their whole input
domains, through the helper probe, bit for bit against numpy's fp32 division (IEEE, correctly rounded): every byte in each channel
of unpack_unorm_rgb, every signed byte of unsnorm8, all 65 536 signed halves in both fields of unpack_snorm_2x16, and
unpack_normal on all 65 536 values of its low field against 17 values of its high one."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(__file__))
import helper_probe as hp  # noqa: E402

F32 = np.float32


@pytest.fixture(scope="module")
def rt():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (select them with -m gpu on a machine that has one)")
    from sunray_amd import runtime
    return runtime


def probe(rt, name, codes):
    import torch
    rows = np.ascontiguousarray(codes, dtype=np.uint32).reshape(-1, 1)
    assert hp.LAYOUT[name][0] == 1
    ow = hp.LAYOUT[name][1]
    d_in = torch.from_numpy(rows.view(np.int32).copy()).cuda()
    d_out = torch.zeros(len(rows) * ow, dtype=torch.int32, device="cuda")
    n = rt.probe_helper(hp.IDS[name], d_in, d_out)
    torch.cuda.synchronize()
    assert n == len(rows)
    return d_out.cpu().numpy().view(np.uint32).reshape(n, ow)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def s16(u):
    return (u & np.uint32(0xFFFF)).astype(np.uint16).view(np.int16).astype(np.float32)


def snorm16(u):
    return np.clip(s16(u) / F32(32767.0), F32(-1.0), F32(1.0)).astype(np.float32)


def test_every_byte_over_255(rt):
    b = np.arange(256, dtype=np.uint32)
    codes = b | (np.roll(b, 85) << np.uint32(8)) | (np.roll(b, 170) << np.uint32(16)) | (np.roll(b, 31) << np.uint32(24))
    got = probe(rt, "unpack_unorm_rgb", codes)
    want = np.stack([bits(((codes >> np.uint32(s)) & np.uint32(0xFF)).astype(np.float32) / F32(255.0)) for s in (0, 8, 16)], axis=1)
    for c in range(3):
        assert set(((codes >> np.uint32(8 * c)) & np.uint32(0xFF)).tolist()) == set(range(256))
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1))[:8]


def test_every_signed_byte_over_127(rt):
    codes = np.concatenate([np.arange(256, dtype=np.uint32), np.arange(256, dtype=np.uint32) | np.uint32(0x5A5A5A00)])   # upper bits are ignored
    got = probe(rt, "unsnorm8", codes)
    i = (codes & np.uint32(0xFF)).astype(np.uint8).view(np.int8).astype(np.float32)
    want = bits(np.maximum(i / F32(127.0), F32(-1.0))).reshape(-1, 1)
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1))[:8]


def test_every_signed_half_over_32767(rt):
    lo = np.arange(65536, dtype=np.uint32)
    codes = lo | (lo[::-1] << np.uint32(16))
    got = probe(rt, "unpack_snorm_2x16", codes)
    want = np.stack([bits(snorm16(codes)), bits(snorm16(codes >> np.uint32(16)))], axis=1)
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1))[:8]


def test_unpack_normal_on_every_low_half(rt):
    lo = np.arange(65536, dtype=np.uint32)
    hi = np.rint(np.linspace(0, 65535, 17)).astype(np.uint32)
    codes = (lo[None, :] | (hi[:, None] << np.uint32(16))).reshape(-1)
    got = probe(rt, "unpack_normal", codes)
    x, y = snorm16(codes), snorm16(codes >> np.uint32(16))
    z = ((F32(1.0) - np.abs(x)) - np.abs(y)).astype(np.float32)
    t = np.maximum(-z, F32(0.0))
    x = (x + np.where(x >= 0, -t, t)).astype(np.float32)
    y = (y + np.where(y >= 0, -t, t)).astype(np.float32)
    r = (F32(1.0) / np.sqrt(((x * x + y * y) + z * z).astype(np.float32))).astype(np.float32)
    want = np.stack([bits(x * r), bits(y * r), bits(z * r)], axis=1)
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1))[:8]
