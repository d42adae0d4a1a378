"""The goniometer's oversampling without a GPU (include/mtr_gonio_os.h): the restatement of tests/_gonio_os.py against what the reference's
Resampler wrote into tests/golden/gonio_os.npz and — where the reference-built checker oracle/_ref/libmeters_ref.so is there — against the
live object, driven through the C++ symbols the checker exports; then the engine's host helpers mtr_gonio_os_table / mtr_gonio_os_hpw
against the restatement.  Every comparison is equality of bytes.

The golden file: 128 stereo frames of uniform noise in [-1, 1) with frame 40 at 1e-30 and frame 41 at 0 (so that the 1e-20f terms of the
sum matter), and for f = 2, 4 and 32 what a Resampler set up as setup_src sets it up (setup (48000, 48000 f, 2, 12, 1.0), then 8192 zero
frames in, 8192 f points out) gave for them, fed in blocks of 64, 1 and 63 frames."""
import ctypes as C
import os

import numpy as np
import pytest

import _gonio
import _gonio_os as OS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "gonio_os.npz")
REF = os.path.join(ROOT, "oracle", "_ref", "libmeters_ref.so")
U32 = np.uint32


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(U32)


class LiveResampler:
    """LV2M::Resampler of the reference-built checker as setup_src (gui/goniometer.c:155-189) sets it up: sizeof 152; inp_count, out_count,
    inp_data, out_data at bytes 0 / 4 / 8 / 16, _table at 40, whose _ctab lies at 16"""

    def __init__(self, lib, f, rate=48000):
        self.lib, self.f = lib, f
        self.obj = C.create_string_buffer(152)
        self.p = C.cast(self.obj, C.c_void_p)
        for n, args in (("_ZN4LV2M9ResamplerC1Ev", [C.c_void_p]), ("_ZN4LV2M9ResamplerD1Ev", [C.c_void_p]), ("_ZN4LV2M9Resampler7processEv", [C.c_void_p]),
                        ("_ZN4LV2M9Resampler5setupEjjjjd", [C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_double])):
            getattr(lib, n).argtypes = args
            getattr(lib, n).restype = C.c_int
        lib._ZN4LV2M9ResamplerC1Ev(self.p)
        assert lib._ZN4LV2M9Resampler5setupEjjjjd(self.p, rate, rate * f, 2, 12, 1.0) == 0
        out = self.process(np.zeros((8192, 2), np.float32))                # the "q/d initialize" of :183-188
        assert not out.any()

    def process(self, x):
        """x float32 [n, 2] -> float32 [n f, 2]"""
        x = np.ascontiguousarray(x, np.float32)
        out = np.full((x.shape[0] * self.f, 2), np.nan, np.float32)
        C.c_uint.from_buffer(self.obj, 0).value = x.shape[0]
        C.c_uint.from_buffer(self.obj, 4).value = out.shape[0]
        C.c_void_p.from_buffer(self.obj, 8).value = x.ctypes.data
        C.c_void_p.from_buffer(self.obj, 16).value = out.ctypes.data
        assert self.lib._ZN4LV2M9Resampler7processEv(self.p) == 0
        left = C.c_uint.from_buffer(self.obj, 4).value
        if x.shape[0] == 8192 and not x.any():                             # (the priming call leaves the 23 f points the window still owes)
            return out[:out.shape[0] - left]
        assert left == 0 and C.c_uint.from_buffer(self.obj, 0).value == 0  # one frame in, f points out
        return out

    def table(self):
        tab = C.c_void_p.from_buffer(self.obj, 40).value
        ctab = C.c_void_p.from_address(tab + 16).value
        return np.ctypeslib.as_array(C.cast(ctab, C.POINTER(C.c_float)), ((self.f + 1) * 12,)).copy().reshape(self.f + 1, 12)

    def close(self):
        self.lib._ZN4LV2M9ResamplerD1Ev(self.p)


def in_blocks(fn, x, blocks):
    out, pos = [], 0
    while pos < x.shape[0]:
        for n in blocks:
            n = min(n, x.shape[0] - pos)
            if n:
                out.append(fn(x[pos:pos + n]))
                pos += n
    return np.concatenate(out)


def restated(x, f, blocks):
    """the restatement over x [T, 2] cut into `blocks` (repeating), its history carried from cut to cut"""
    st = {"h": None}

    def step(seg):
        pts, st["h"] = OS.upsample(seg[None], f, st["h"])
        return pts[0]
    return in_blocks(step, x, blocks)


def test_the_restatement_is_the_golden_file():
    g = np.load(GOLDEN)
    x = g["x"]
    assert x.shape == (128, 2) and x.dtype == np.float32 and (x[40] == np.float32(1e-30)).all() and (x[41] == 0).all()
    for f in (2, 4, 32):
        want = g["f%d" % f]
        assert want.shape == (128 * f, 2)
        got = restated(x, f, [64, 1, 63])
        assert np.array_equal(bits(got), bits(want)), (f, np.argwhere(bits(got) != bits(want))[:4].tolist())
        assert np.array_equal(bits(OS.upsample(x[None], f)[0][0]), bits(want)), f           # ... and uncut
        assert not np.array_equal(bits(want[::f]), bits(x))                                 # phase 0 is no copy of the input


@pytest.mark.skipif(not os.path.exists(REF), reason="needs the reference-built checker (oracle/_ref, built where the reference is)")
@pytest.mark.parametrize("f", [2, 3, 4, 32])
def test_the_restatement_is_the_live_resampler(f):
    lib = C.CDLL(REF)
    x = np.random.default_rng(50 + f).uniform(-1, 1, (5000, 2)).astype(np.float32)
    x[100], x[101], x[3000:3030] = 1e-30, 0, 0
    cuts = [64, 1, 1920, 7, 3008]
    assert sum(cuts) == 5000
    r = LiveResampler(lib, f)
    try:
        assert np.array_equal(bits(r.table()), bits(OS.table(f)))
        want = in_blocks(r.process, x, cuts)
    finally:
        r.close()
    assert want.shape == (5000 * f, 2)
    assert np.array_equal(bits(restated(x, f, cuts)), bits(want))
    assert np.array_equal(bits(OS.upsample(x[None], f)[0][0]), bits(want))


def test_the_host_helpers_are_the_restatement():
    import meters.lv2_amd as M
    for f in range(2, 33):
        assert np.array_equal(bits(M.gonio_os_table(f)), bits(OS.table(f))), f
        for rate in (44100.0, 48000.0, 96000.0):
            assert bits(M.gonio_os_hpw(rate, f)) == bits(OS.hpw(rate, f)), (f, rate)
    for rate in (44100.0, 48000.0, 96000.0):                               # factor 1: the hpw of mtr_gonio_derive
        assert bits(M.gonio_os_hpw(rate, 1)) == bits(_gonio.derive(rate).hpw) == bits(M.gonio_derive(rate).hpw)
    assert float(OS.hpw(48000.0, 4)) > float(OS.hpw(48000.0, 1))


def test_the_pure_helpers_refuse_bad_factors():
    import meters.lv2_amd as M
    for f in (0, 33):
        with pytest.raises(M.EngineError) as ei:
            M.gonio_os_table(f)
        assert ei.value.code == M.engine.ERR_ARG
        with pytest.raises(M.EngineError) as ei:
            M.gonio_os_hpw(48000.0, f)
        assert ei.value.code == M.engine.ERR_ARG
    with pytest.raises(M.EngineError) as ei:
        M.gonio_os_table(1)                                                # (factor 1 has no table)
    assert ei.value.code == M.engine.ERR_ARG
