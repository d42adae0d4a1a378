"""Plane layouts without a GPU (include/mtr_planes.h): mtr_plane_decode_host — the definition k_plane and every call with a plane
layout are held against (tests/test_gpu_planes.py) — against numpy indexing, bit for bit, in all four formats; its argument errors; the
new symbols exported and declared."""
import ctypes as C

import numpy as np
import pytest

import meters.lv2_amd as M

NEW = ["mtr_engine_plane_layout", "mtr_engine_plane_stats", "mtr_engine_set_plane_layout", "mtr_plane_decode_host"]
FORMATS = ["f32", "s16", "s24", "s32"]
BITS = {"f32": 32, "s16": 16, "s24": 24, "s32": 32}
# (P, map): the identity at every width, repeats, P < C, P > C
LAYOUTS = [(P, tuple(range(P))) for P in range(1, 9)] + [(1, (0, 0)), (2, (1, 0)), (4, (3, 1)), (6, (0, 1, 2, 4, 5)), (3, (2,)), (2, (1, 1, 0, 0, 1)),
                                                         (8, (7, 0, 3, 3, 5, 1, 6, 2)), (3, (2, 2, 2, 0, 0, 1, 1, 1))]


def _fmt(name):
    return {"f32": 0, "s16": M.PCM_S16, "s24": M.PCM_S24, "s32": M.PCM_S32}[name]


def test_symbols_exported_and_declared():
    assert M.exported_symbols("mtr_planes.h") == NEW
    assert not set(NEW) & set(M.exported_symbols())                      # (mtr_engine.h itself declares what it declared)
    for n in NEW:
        assert hasattr(M.lib, n), n


def _codes(rng, name, shape):
    """integer codes of the format's width, the extreme ones among them"""
    k = BITS[name] - 1
    q = rng.integers(-(1 << k), 1 << k, size=shape, dtype=np.int64)
    flat = q.reshape(-1)
    flat[::7] = (1 << k) - 1
    flat[3::11] = -(1 << k)
    flat[5::13] = 0
    flat[6::17] = -1
    return q


def _want_int(q, name):
    """the contract of mtr_pcm_decode_host: the code in the top bits of an int32, converted (round to nearest even) and scaled by 2^-31"""
    top = (q << (32 - BITS[name])).astype(np.int32)
    return top.astype(np.float32) * np.float32(2.0 ** -31)


def _buffer(rng, name, P, n, stride, lead):
    """(bytes, planes): a byte buffer of `lead` junk bytes, then P planes `stride` samples apart, the n samples of each followed by junk;
    planes [P, n] as float32 bit patterns (f32) or integer codes"""
    sb = BITS[name] // 8
    buf = np.full(lead + P * stride * sb + 8, 0xFF, np.uint8)             # 0xFF..: NaN as f32, -1 as integers; overwritten where it matters
    if name == "f32":
        bits = rng.integers(0, 1 << 32, size=(P, n), dtype=np.uint64).astype(np.uint32)
        bits.reshape(-1)[::5] = 0x7FC12345                               # quiet NaNs with payloads, a signalling one, infinities, -0
        bits.reshape(-1)[2::9] = 0xFFA00001
        bits.reshape(-1)[4::13] = 0x7F800000
        bits.reshape(-1)[1::17] = 0x80000000
        planes, raw = bits, bits.view(np.uint8).reshape(P, n * 4)
    else:
        planes = _codes(rng, name, (P, n))
        raw = planes.astype("<i4").view(np.uint8).reshape(P, n, 4)[:, :, :sb] if name != "s32" else planes.astype("<i4").view(np.uint8).reshape(P, n, 4)
        if name == "s16":
            raw = planes.astype("<i2").view(np.uint8).reshape(P, n, 2)
        raw = np.ascontiguousarray(raw).reshape(P, n * sb)
    for p in range(P):
        at = lead + p * stride * sb
        buf[at: at + n * sb] = raw[p]
        junk = np.array([np.nan, np.inf, 1e30, -np.inf], np.float32).view(np.uint8) if name == "f32" else np.array([0xFF, 0x7F, 0x00, 0x80], np.uint8)
        gap = (stride - n) * sb
        buf[at + n * sb: at + n * sb + gap] = np.resize(junk, gap)
    return buf, planes


@pytest.mark.parametrize("name", FORMATS)
def test_plane_decode_is_numpy_indexing(name):
    rng = np.random.default_rng(BITS[name] + len(name))
    sb = BITS[name] // 8
    for P, m in LAYOUTS:
        for n, extra, lead in ((1, 0, 0), (3, 2, sb), (4, 1, 0), (7, 3, 1 if name == "s24" else sb), (257, 5, 5 * sb), (64, 0, 3 if name == "s24" else 0)):
            stride = n + extra
            buf, planes = _buffer(rng, name, P, n, stride, lead)
            # the planes as a VIEW of the buffer: [P, n] samples, `stride` samples apart, starting `lead` bytes in (S24: on any byte)
            body = buf[lead: lead + P * stride * sb].reshape(P, stride * sb)[:, : n * sb]
            view = body if name == "s24" else body.view({"f32": np.float32, "s16": np.int16, "s32": np.int32}[name]) if lead % sb == 0 else None
            assert view is not None and view.base is not None
            got = M.plane_decode(_fmt(name), view, m)
            assert got.shape == (n, len(m)) and got.dtype == np.float32
            sel = planes[list(m)].T                                          # [n, C]
            if name == "f32":
                assert np.array_equal(got.view(np.uint32), sel)              # bit patterns: a NaN keeps its payload
            else:
                assert np.array_equal(got.view(np.uint32), _want_int(sel, name).view(np.uint32))
            # ... and the C entry point itself, with the stride spelt out
            out = np.full((n, len(m)), 7.0, np.float32)
            mm = np.array(m, np.uint8)
            assert M.lib.mtr_plane_decode_host(_fmt(name), buf.ctypes.data + lead, n, stride, P, mm.ctypes.data, len(m), out.ctypes.data) == 0
            assert np.array_equal(out.view(np.uint32), got.view(np.uint32))


def test_s24_planes_on_odd_bytes_and_batches():
    """[S, P, n * 3] packed bytes whose planes start on odd bytes, a leading batch axis, a window of longer planes"""
    rng = np.random.default_rng(24)
    S, P, total, t0, n = 3, 3, 50, 7, 21
    q = _codes(rng, "s24", (S, P, total))
    raw = np.ascontiguousarray(q.astype("<i4").view(np.uint8).reshape(S, P, total, 4)[..., :3]).reshape(-1)
    buf = np.concatenate([np.zeros(1, np.uint8), raw])                    # every plane now starts on an odd byte (total * 3 = 150 is even)
    x = buf[1:].reshape(S, P, total * 3)
    assert x.ctypes.data % 2 == 1
    win = x[:, :, t0 * 3: (t0 + n) * 3]
    got = M.plane_decode(M.PCM_S24, win, (2, 0))
    assert got.shape == (S, n, 2)
    want = _want_int(q[:, [2, 0], t0: t0 + n].transpose(0, 2, 1), "s24")
    assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(want).view(np.uint32))
    with pytest.raises(ValueError):
        M.plane_decode(M.PCM_S24, win, (2, 0), stride=total + 1)          # not what the view says


def test_extreme_codes_decode_exactly():
    for name in ("s16", "s24", "s32"):
        k = BITS[name] - 1
        codes = np.array([[-(1 << k), (1 << k) - 1, 0, -1, 1]], np.int64)
        x = codes.astype(np.int16 if name == "s16" else np.int32)
        if name == "s24":
            x = np.ascontiguousarray(codes.astype("<i4").view(np.uint8).reshape(1, 5, 4)[:, :, :3]).reshape(1, 15)
        got = M.plane_decode(_fmt(name), x, (0,))[:, 0]
        want = np.array([-1.0, ((1 << k) - 1) / 2.0 ** k, 0.0, -(2.0 ** -k), 2.0 ** -k])
        assert np.array_equal(got.astype(np.float64), want.astype(np.float32).astype(np.float64)), (name, got)
        if name != "s32":
            assert np.array_equal(got.astype(np.float64), want)          # 16 and 24 bits are exact in f32


def test_argument_errors():
    L = M.lib
    src = np.zeros((4, 16), np.float32)
    dst = np.full((16, 2), 5.0, np.float32)
    ok = np.array([0, 1], np.uint8)

    def call(fmt=0, s=src.ctypes.data, n=16, stride=16, P=4, m=ok.ctypes.data, Cn=2, d=dst.ctypes.data):
        return L.mtr_plane_decode_host(fmt, s, n, stride, P, m, Cn, d)

    assert call() == 0
    dst[:] = 5.0
    assert call(m=np.array([0, 4], np.uint8).ctypes.data) == -1           # an entry >= P
    assert call(P=1) == -1                                                # ... entry 1 >= 1
    assert call(P=0) == -1
    assert call(P=9) == -1
    assert call(m=None) == -1
    assert call(Cn=0) == -1 and call(Cn=9) == -1
    assert call(stride=15) == -1                                          # stride < n_frames
    assert call(fmt=4) == -1 and call(fmt=-1) == -1
    assert call(s=None) == -1 and call(d=None) == -1
    assert b"plane" in L.mtr_last_error()
    assert np.all(dst == 5.0)                                             # nothing written by a refused call
    assert call(n=0, s=None, d=None) == 0                                 # nothing to do
    with pytest.raises(ValueError):
        M.plane_decode(0, src, None, n_channels=2)                        # map=None is the identity: 4 planes are 4 channels
    assert M.plane_decode(0, src, None).shape == (16, 4)
    with pytest.raises(ValueError):
        M.plane_decode(0, src.astype(np.float64), (0, 1))
    with pytest.raises(ValueError):
        M.plane_decode(0, src.T, (0, 1))                                  # the last axis is not contiguous
    with pytest.raises(M.EngineError):
        M.plane_decode(0, src, (0, 4))
