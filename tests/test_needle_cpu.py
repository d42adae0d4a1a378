"""MTR_METER_NEEDLE (Vumeterdsp, Iec1ppmdsp, Iec2ppmdsp, Msppmdsp for a batch) without a GPU: the coefficients against the restatements
of the four init () functions, the new symbols, what mtr_engine_create accepts and the NULL-engine answers of the entry points."""
import ctypes as C
import os
import re

import numpy as np
import pytest

F = C.c_float
NEW = ("mtr_needle_coef", "mtr_engine_needle_configure", "mtr_engine_needle_set_gain", "mtr_engine_needle_read",
       "mtr_engine_needle_series", "mtr_engine_needle_reset")
INC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
RATES = [44100.0, 48000.0, 96000.0, 8000.0]


class Vu(C.Structure):
    _fields_ = [("z1", F), ("z2", F), ("m", F), ("res", C.c_int), ("w", F), ("g", F)]


class Ppm(C.Structure):
    _fields_ = [("z1", F), ("z2", F), ("m", F), ("res", C.c_int), ("w1", F), ("w2", F), ("w3", F), ("g", F)]


@pytest.fixture(scope="module")
def M():
    import meters.lv2_amd as m
    return m


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("fs", RATES)
def test_coefficients_are_the_restatements(M, oracle, fs):
    lib = C.CDLL(oracle.lib._name)                                 # (a handle of its own: the session's keeps its argtypes)
    for f in ("mo_ppm_init_iec1", "mo_ppm_init_iec2"):
        getattr(lib, f).argtypes = [C.POINTER(Ppm), F]
        getattr(lib, f).restype = None
    lib.mo_vu_init.argtypes = [C.POINTER(Vu), F]
    lib.mo_vu_init.restype = None
    v = Vu()
    lib.mo_vu_init(C.byref(v), fs)
    got = M.needle_coef(M.NEEDLE_VU, fs)
    assert np.array_equal(_bits(got), _bits([v.w, np.float32(4) * np.float32(v.w), 0.0, v.g])), (fs, got)
    for kind, init in ((M.NEEDLE_IEC1, lib.mo_ppm_init_iec1), (M.NEEDLE_IEC2, lib.mo_ppm_init_iec2), (M.NEEDLE_MS, lib.mo_ppm_init_iec2)):
        p = Ppm()
        init(C.byref(p), fs)
        got = M.needle_coef(kind, fs)
        assert np.array_equal(_bits(got), _bits([p.w1, p.w2, p.w3, p.g])), (kind, fs, got)


def test_unknown_kind_and_null(M):
    out = np.zeros(4, np.float32)
    for kind in (0, 3, 16, 15):
        assert M.lib.mtr_needle_coef(kind, 48000.0, out.ctypes.data) == M.engine.ERR_ARG, kind
    assert M.lib.mtr_needle_coef(M.NEEDLE_VU, 48000.0, None) == M.engine.ERR_ARG


def test_symbols_and_abi(M):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(INC, "mtr_needle.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(mtr_[a-z0-9_]+)\s*\(", txt))) == sorted(NEW)
    for name, bit in (("VU", 1), ("IEC1", 2), ("IEC2", 4), ("MS", 8)):
        assert re.search(r"#define\s+MTR_NEEDLE_%s\s+%du\b" % (name, bit), txt)
    main = open(os.path.join(INC, "mtr_engine.h")).read()
    assert re.search(r'^#include "mtr_needle.h"', main, flags=re.M)
    assert re.search(r"#define\s+MTR_METER_NEEDLE\s+0x800u", main) and re.search(r"#define\s+MTR_ABI_VERSION\s+2\b", main)
    names = M.exported_symbols("mtr_needle.h")                     # (what mtr_engine.h itself declares is pinned: tests/test_frames_cpu.py)
    assert not set(NEW) & set(M.exported_symbols())
    for n in NEW:
        assert n in names, n
        assert hasattr(M.lib, n), n
    assert M.lib.mtr_abi_version() == 2
    for n in ("needle_configure", "needle_set_gain", "needle_read", "needle_series", "needle_reset"):
        assert hasattr(M.Engine, n), n
    assert (M.METER_NEEDLE, M.NEEDLE_VU, M.NEEDLE_IEC1, M.NEEDLE_IEC2, M.NEEDLE_MS) == (0x800, 1, 2, 4, 8)


def _create(M, n_channels, meters):
    cfg = M.engine._Config(struct_size=C.sizeof(M.engine._Config), meters=meters, n_streams=4, n_channels=n_channels,
                           sample_rate=48000.0, device=0)
    h = C.c_void_p()
    rc = M.lib.mtr_engine_create(C.byref(cfg), C.byref(h))
    if h.value:
        M.lib.mtr_engine_destroy(h)
    return rc


def test_create_accepts_mono_and_stereo(M):
    E = M.engine
    for ch in (1, 2):
        assert _create(M, ch, M.METER_NEEDLE) in (0, E.ERR_NODEVICE), M.lib.mtr_last_error()
        assert _create(M, ch, M.METER_NEEDLE | M.METER_KMETER | M.METER_DR14) in (0, E.ERR_NODEVICE), M.lib.mtr_last_error()
    assert _create(M, 2, M.METER_NEEDLE | M.METER_EBU | M.METER_TRUEPEAK | M.METER_STCORR) in (0, E.ERR_NODEVICE)
    assert _create(M, 5, M.METER_NEEDLE | M.METER_EBU) == E.ERR_UNSUPPORTED
    assert _create(M, 2, 0x1000) == E.ERR_ARG and _create(M, 2, 0x100 | M.METER_NEEDLE) == E.ERR_ARG
    assert _create(M, 2, 0x400) == E.ERR_ARG and _create(M, 2, 0x400 | M.METER_NEEDLE) == E.ERR_ARG    # (0x100 and 0x400 stay no meters)


def test_null_engine_is_an_argument_error(M):
    E, lib = M.engine, M.lib
    a, st = np.zeros(2, np.float32), np.zeros(4, np.float32)
    n, d = C.c_uint32(), C.c_uint32()
    assert lib.mtr_engine_needle_configure(None, 4, 0, 0) == E.ERR_ARG
    assert lib.mtr_engine_needle_set_gain(None, 0, -6.0) == E.ERR_ARG
    assert lib.mtr_engine_needle_read(None, 4, 0, 1, a.ctypes.data, st.ctypes.data) == E.ERR_ARG
    assert lib.mtr_engine_needle_series(None, 4, 0, 1, a.ctypes.data, 1, C.byref(n), C.byref(d)) == E.ERR_ARG
    assert lib.mtr_engine_needle_reset(None) == E.ERR_ARG
