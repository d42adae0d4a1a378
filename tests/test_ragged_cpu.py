"""Ragged batches for STCORR and NEEDLE (include/mtr_ragged.h): the surface and the block arithmetic, without a GPU.

mtr_series_cut is the arithmetic behind mtr_engine_series_points — how many whole blocks of the reading series a stream completes in a
call, and whether a truncated one follows — and the engine counts with the same function (csrc/mtr_series.h).  Here it is held against
a count made frame by frame.  The behaviour of the calls is held by tests/test_gpu_ragged.py.
"""
import ctypes as C
import os
import re

import pytest

import meters.lv2_amd as M

HERE = os.path.dirname(os.path.abspath(__file__))
NEW = ("mtr_engine_process_device_ragged", "mtr_engine_process_host_ragged", "mtr_engine_series_points", "mtr_series_cut")
ERR_ARG = -1


def test_header_declares_and_library_exports_the_ragged_entry_points():
    names = M.exported_symbols("mtr_ragged.h")
    assert set(names) == set(NEW)
    for n in NEW:
        assert hasattr(M.lib, n), f"{n} is declared but libmtr_engine.so does not export it"
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "mtr_engine.h")).read()
    assert re.search(r'^#include "mtr_ragged.h"', hdr, flags=re.M)      # (a client of mtr_engine.h sees them)
    assert re.search(r"#define\s+MTR_ABI_VERSION\s+2\b", hdr)          # (an addition inside version 2)
    assert M.lib.mtr_abi_version() == 2


def test_binding_has_the_ragged_methods():
    for m in ("process_device_ragged", "process_ragged", "series_points"):
        assert callable(getattr(M.Engine, m, None)), m
    assert callable(M.series_cut)


@pytest.mark.parametrize("fn", NEW[:3])
def test_null_engine_is_an_argument_error(fn):
    """No device needed: a NULL engine is refused before anything else (MTR_ERR_ARG)."""
    f = getattr(M.lib, fn)
    args = {"mtr_engine_process_device_ragged": [None, None, 0, 0, None, None], "mtr_engine_process_host_ragged": [None, None, 0, 0, None],
            "mtr_engine_series_points": [None, M.METER_STCORR, 0, 0, None]}[fn]
    assert f(*args) == ERR_ARG


def brute(fill, P, n_frames, frames):
    """a host that feeds the stream its `frames` frames one by one into blocks of P, the first of which holds `fill` already, and stops
    there: whole blocks, and whether it has to close an open one (period 0: the call is the block)"""
    closes = 0 < frames < n_frames
    if P == 0:
        return 0, int(closes)
    whole, j = 0, fill
    for _ in range(frames):
        j += 1
        if j == P:
            whole, j = whole + 1, 0
    return whole, int(closes and j > 0)


def test_series_cut_against_a_frame_by_frame_count():
    n = 0
    for P in (0, 1, 4, 5, 16, 17):
        for fill in sorted({0, 1, P // 2, max(P - 1, 0)}):
            if P and fill >= P:
                continue
            for n_frames in (1, 3, 16, 17, 40):
                for frames in range(n_frames + 1):      # 0, block boundaries and one frame past them, n_frames - 1, n_frames
                    assert M.series_cut(fill, P, n_frames, frames) == brute(fill, P, n_frames, frames), (fill, P, n_frames, frames)
                    n += 1
    assert n > 1000
    # the cases by name: fill = P - 1, frames = 0, frames on a block boundary and one past it, period 0
    assert M.series_cut(15, 16, 40, 1) == (1, 0)
    assert M.series_cut(15, 16, 40, 2) == (1, 1)
    assert M.series_cut(15, 16, 40, 0) == (0, 0)
    assert M.series_cut(3, 16, 40, 13) == (1, 0) and M.series_cut(3, 16, 40, 14) == (1, 1)
    assert M.series_cut(3, 16, 40, 40) == (2, 0)                        # an open stream: the lock-step count, nothing truncated
    assert M.series_cut(0, 0, 40, 0) == (0, 0) and M.series_cut(0, 0, 40, 39) == (0, 1) and M.series_cut(0, 0, 40, 40) == (0, 0)
    # large values: 64-bit arithmetic
    assert M.series_cut(2 ** 31, 2 ** 32 + 1, 2 ** 40, 2 ** 33) == ((2 ** 31 + 2 ** 33) // (2 ** 32 + 1), 1)


def test_series_cut_argument_errors():
    whole, partial = C.c_uint64(), C.c_uint32()
    f = M.lib.mtr_series_cut
    assert f(16, 16, 10, 5, C.byref(whole), C.byref(partial)) == ERR_ARG      # fill >= period > 0
    assert f(17, 16, 10, 5, C.byref(whole), C.byref(partial)) == ERR_ARG
    assert f(0, 16, 10, 11, C.byref(whole), C.byref(partial)) == ERR_ARG      # frames > n_frames
    assert f(0, 0, 10, 11, C.byref(whole), C.byref(partial)) == ERR_ARG
    assert f(0, 16, 10, 5, None, C.byref(partial)) == ERR_ARG
    assert f(0, 16, 10, 5, C.byref(whole), None) == ERR_ARG
    assert f(5, 0, 10, 5, C.byref(whole), C.byref(partial)) == 0             # (period 0 has no fill to check)
    with pytest.raises(M.EngineError):
        M.series_cut(16, 16, 10, 5)
