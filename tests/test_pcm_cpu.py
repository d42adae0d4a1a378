"""Integer PCM in (mtr_engine_process_host_pcm / _device_pcm): the surface and the conversion contract, without a GPU.

The contract (include/mtr_engine.h, MTR_PCM_*): S16 x * 2^-15 and S24 x * 2^-23 exactly, S32 (float) x * 2^-31 with the
int-to-float conversion rounding to nearest even.  The yardstick is numpy's `x.astype(np.float32) * np.float32(2.0 ** -k)`,
and mtr_pcm_decode_host must equal it BIT FOR BIT: it is what the GPU decode is held against (tests/test_gpu_pcm.py).
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import meters.lv2_amd as M

HERE = os.path.dirname(os.path.abspath(__file__))
NEW = ("mtr_engine_process_host_pcm", "mtr_engine_process_device_pcm", "mtr_pcm_sample_bytes", "mtr_pcm_decode_host",
       "mtr_engine_pcm_stats")
COUNTS = (0, 1, 7, 16, 1001)


def test_header_declares_and_library_exports_the_pcm_entry_points():
    names = M.exported_symbols()
    for n in NEW:
        assert n in names, f"{n} is not declared in include/mtr_engine.h"
        assert hasattr(M.lib, n), f"{n} is declared but libmtr_engine.so does not export it"
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "mtr_engine.h")).read()
    assert re.search(r"#define\s+MTR_ABI_VERSION\s+2\b", hdr)          # (an addition inside version 2)
    assert M.lib.mtr_abi_version() == 2
    for name, val in (("MTR_PCM_S16", 1), ("MTR_PCM_S24", 2), ("MTR_PCM_S32", 3)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), hdr), name
    assert (M.PCM_S16, M.PCM_S24, M.PCM_S32) == (1, 2, 3)


def test_binding_has_the_pcm_methods():
    for m in ("process_pcm", "process_device_pcm", "pcm_stats"):
        assert callable(getattr(M.Engine, m, None)), m
    assert callable(getattr(M, "pcm_decode", None))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _decode_at(fmt, raw, n, shift):
    """mtr_pcm_decode_host on n samples whose bytes `raw` start `shift` bytes into a fresh buffer"""
    buf = np.zeros(raw.size + shift + 16, np.uint8)
    buf[shift:shift + raw.size] = raw
    out = np.full(n + 4, np.float32(123.0))                           # ... and nothing behind the n-th float is written
    assert M.lib.mtr_pcm_decode_host(fmt, buf.ctypes.data + shift, n, out.ctypes.data) == 0
    assert (out[n:] == 123.0).all()
    return out[:n]


def _pack24(v):
    """int values in [-2^23, 2^23) as packed little-endian 3-byte samples"""
    return np.ascontiguousarray(np.asarray(v, np.int64).astype("<i4")).view(np.uint8).reshape(-1, 4)[:, :3].reshape(-1).copy()


def test_s16_every_value_is_exact():
    x = np.arange(-32768, 32768).astype(np.int16)
    want = x.astype(np.float32) * np.float32(2.0 ** -15)
    assert np.array_equal(_bits(M.pcm_decode(M.PCM_S16, x)), _bits(want))
    assert want[0] == -1.0 and want[-1] == np.float32(32767 / 32768)
    raw = x.astype("<i2").view(np.uint8)
    for n in COUNTS:
        for shift in (0, 2):
            assert np.array_equal(_bits(_decode_at(M.PCM_S16, raw[:2 * n], n, shift)), _bits(want[:n])), (n, shift)


def test_s24_is_exact():
    rng = np.random.default_rng(24)
    v = np.concatenate([[0x7fffff, -0x800000, -1, 1, 0], rng.integers(-(1 << 23), 1 << 23, 4000)])   # 0x800000 and 0xffffff as two's complement
    raw = _pack24(v)
    assert tuple(raw[:12]) == (0xff, 0xff, 0x7f, 0, 0, 0x80, 0xff, 0xff, 0xff, 1, 0, 0)
    want = v.astype(np.int32).astype(np.float32) * np.float32(2.0 ** -23)
    assert want[0] == np.float32(1 - 2.0 ** -23) and want[1] == -1.0 and want[2] == np.float32(-2.0 ** -23)
    assert np.array_equal(_bits(M.pcm_decode(M.PCM_S24, raw)), _bits(want))
    assert M.pcm_decode(M.PCM_S24, raw.reshape(5, -1)).shape == (5, v.size // 5)
    for n in COUNTS:
        for shift in (0, 1, 2, 3):
            assert np.array_equal(_bits(_decode_at(M.PCM_S24, raw[:3 * n], n, shift)), _bits(want[:n])), (n, shift)


def test_s32_rounds_to_nearest_even():
    rng = np.random.default_rng(32)
    edge = [-(1 << 31), (1 << 31) - 1, (1 << 24) + 1, -((1 << 24) + 1), (1 << 24) + 3, 0x7fffffbf, 0x7fffffc0, 0x7fffff40, 0, 1, -1]
    v = np.concatenate([edge, rng.integers(-(1 << 31), 1 << 31, 4000)]).astype(np.int32)
    want = v.astype(np.float32) * np.float32(2.0 ** -31)
    got = M.pcm_decode(M.PCM_S32, v)
    assert np.array_equal(_bits(got), _bits(want))
    # the cases by hand: INT32_MIN -> -1, INT32_MAX -> 1, ties to even, the last value below 2^31 that does not round up to it
    assert got[0] == -1.0 and got[1] == 1.0
    assert got[2] == np.float32(2.0 ** -7) and got[3] == np.float32(-2.0 ** -7)              # 2^24 + 1 -> 2^24
    assert got[4] == np.float32((2.0 ** 24 + 4) * 2.0 ** -31)                                # 2^24 + 3 -> 2^24 + 4
    assert got[5] == np.float32(1 - 2.0 ** -24) and got[6] == 1.0                            # 0x7fffffbf -> 0x7fffff80, 0x7fffffc0 (a tie) -> 2^31
    assert got[7] == np.float32((2.0 ** 31 - 256) * 2.0 ** -31)                              # 0x7fffff40 (a tie) -> 0x7fffff00, the even one
    raw = v.astype("<i4").view(np.uint8)
    for n in COUNTS:
        for shift in (0, 1, 2, 3):
            assert np.array_equal(_bits(_decode_at(M.PCM_S32, raw[:4 * n], n, shift)), _bits(want[:n])), (n, shift)


def test_sample_bytes_and_argument_errors():
    assert [M.lib.mtr_pcm_sample_bytes(f) for f in (M.PCM_S16, M.PCM_S24, M.PCM_S32, 0, 4, -1)] == [2, 3, 4, 0, 0, 0]
    src = np.zeros(64, np.uint8)
    dst = np.zeros(16, np.float32)
    for fmt in (0, 4, -1):
        assert M.lib.mtr_pcm_decode_host(fmt, src.ctypes.data, 4, dst.ctypes.data) == -1, fmt
    for fmt in (M.PCM_S16, M.PCM_S24, M.PCM_S32):
        assert M.lib.mtr_pcm_decode_host(fmt, None, 4, dst.ctypes.data) == -1
        assert M.lib.mtr_pcm_decode_host(fmt, src.ctypes.data, 4, None) == -1
    # a NULL engine is refused before anything else, whatever the rest
    assert M.lib.mtr_engine_process_host_pcm(None, src.ctypes.data, M.PCM_S16, 4, 4, None) == -1
    assert M.lib.mtr_engine_process_device_pcm(None, src.ctypes.data, M.PCM_S16, 4, 4, None, None) == -1
    a, b, ms = C.c_uint64(), C.c_uint64(), C.c_float()
    assert M.lib.mtr_engine_pcm_stats(None, C.byref(a), C.byref(b), C.byref(ms)) == -1


def test_pcm_decode_refuses_wrong_arrays():
    with pytest.raises(ValueError):
        M.pcm_decode(M.PCM_S16, np.zeros(4, np.float32))
    with pytest.raises(ValueError):
        M.pcm_decode(M.PCM_S32, np.zeros(4, np.int16))
    with pytest.raises(ValueError):
        M.pcm_decode(M.PCM_S24, np.zeros(4, np.uint8))                  # not whole 3-byte samples
