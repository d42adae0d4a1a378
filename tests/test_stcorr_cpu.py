"""MTR_METER_STCORR (Stcorrdsp for a batch) without a GPU: the coefficients against the restatement of Stcorrdsp::init, what
mtr_engine_create accepts (its argument checks run before the device check), the new symbols and their NULL-engine answers."""
import ctypes as C
import os
import re

import numpy as np
import pytest

F = C.c_float
NEW = ("mtr_stcorr_coef", "mtr_engine_stcorr_set_period", "mtr_engine_stcorr_read", "mtr_engine_stcorr_series", "mtr_engine_stcorr_reset")


class Stcorr(C.Structure):
    _fields_ = [(n, F) for n in ("zl", "zr", "zlr", "zll", "zrr", "w1", "w2")]


@pytest.fixture(scope="module")
def M():
    import meters.lv2_amd as m
    return m


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("fs", [8000.0, 44100.0, 48000.0, 96000.0, 192000.0])
def test_coefficients_are_the_restatements(M, oracle, fs):
    lib = oracle.lib
    lib.mo_stcorr_init.argtypes = [C.POINTER(Stcorr), C.c_int, F, F]
    lib.mo_stcorr_init.restype = None
    c = Stcorr()
    lib.mo_stcorr_init(C.byref(c), int(fs), 2e3, 0.3)
    got = M.stcorr_coef(fs)
    assert np.array_equal(_bits(got), _bits([c.w1, c.w2])), (fs, got, c.w1, c.w2)
    assert abs(1.0 - float(got[0])) < 1.0                     # the first stage is stable from 8 kHz up (1 - w1 = -0.57 there)


def test_coef_rejects_null(M):
    assert M.lib.mtr_stcorr_coef(48000.0, None) == M.engine.ERR_ARG


def _create(M, n_channels, meters, **kw):
    cfg = M.engine._Config(struct_size=C.sizeof(M.engine._Config), meters=meters, n_streams=4, n_channels=n_channels,
                           sample_rate=48000.0, device=0, **kw)
    h = C.c_void_p()
    rc = M.lib.mtr_engine_create(C.byref(cfg), C.byref(h))
    if h.value:
        M.lib.mtr_engine_destroy(h)
    return rc


def test_bit_value(M):
    assert M.METER_STCORR == 0x200


def test_create_accepts_stereo_stcorr(M):
    E = M.engine
    assert _create(M, 2, M.METER_STCORR) in (0, E.ERR_NODEVICE), M.lib.mtr_last_error()
    for other in (M.METER_EBU | M.METER_TRUEPEAK, M.METER_KMETER | M.METER_DR14, M.METER_SPECTR30 | M.METER_TPBALLIST):
        assert _create(M, 2, M.METER_STCORR | other) in (0, E.ERR_NODEVICE), (other, M.lib.mtr_last_error())


def test_create_refuses_mono_and_surround_stcorr(M):
    E = M.engine
    assert _create(M, 1, M.METER_STCORR) == E.ERR_UNSUPPORTED
    assert _create(M, 1, M.METER_STCORR | M.METER_KMETER) == E.ERR_UNSUPPORTED
    assert _create(M, 5, M.METER_EBU | M.METER_STCORR) == E.ERR_UNSUPPORTED
    assert _create(M, 3, M.METER_STCORR) == E.ERR_UNSUPPORTED


def test_0x100_is_still_no_meter(M):
    assert _create(M, 2, 0x100) == M.engine.ERR_ARG
    assert _create(M, 2, 0x100 | M.METER_STCORR) == M.engine.ERR_ARG
    assert _create(M, 2, 0x400) == M.engine.ERR_ARG


def test_symbols_and_abi(M):
    # the declarations live in include/mtr_stcorr.h, which mtr_engine.h includes (the set mtr_engine.h itself declares is pinned)
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, "mtr_stcorr.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(mtr_[a-z0-9_]+)\s*\(", txt))) == sorted(NEW)
    main = open(os.path.join(inc, "mtr_engine.h")).read()
    assert re.search(r'^#include "mtr_stcorr.h"', main, flags=re.M)
    assert re.search(r"#define\s+MTR_METER_STCORR\s+0x200u", main) and re.search(r"#define\s+MTR_ABI_VERSION\s+2\b", main)
    for n in NEW:
        assert hasattr(M.lib, n), n
    assert M.lib.mtr_abi_version() == 2
    for n in ("stcorr_set_period", "stcorr_read", "stcorr_series", "stcorr_reset"):
        assert hasattr(M.Engine, n), n


def test_null_engine_is_an_argument_error(M):
    E, lib = M.engine, M.lib
    corr, st = np.zeros(1, np.float32), np.zeros(5, np.float32)
    n, d = C.c_uint32(), C.c_uint32()
    assert lib.mtr_engine_stcorr_set_period(None, 0, 0) == E.ERR_ARG
    assert lib.mtr_engine_stcorr_read(None, 0, 1, corr.ctypes.data, st.ctypes.data) == E.ERR_ARG
    assert lib.mtr_engine_stcorr_series(None, 0, 1, corr.ctypes.data, 1, C.byref(n), C.byref(d)) == E.ERR_ARG
    assert lib.mtr_engine_stcorr_reset(None) == E.ERR_ARG
