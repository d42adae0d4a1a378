"""The loudness log (include/mtr_loudlog.h) without a GPU: what the header declares, what the library exports and the binding offers,
and the NULL-engine answers of the four entry points."""
import ctypes as C
import os
import re

import numpy as np
import pytest

NEW = ("mtr_engine_loudlog_set_period", "mtr_engine_loudlog_period", "mtr_engine_loudlog_series", "mtr_engine_loudlog_reset")
INC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")


@pytest.fixture(scope="module")
def M():
    import meters.lv2_amd as m
    return m


def test_header_declares_exactly_the_four():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(INC, "mtr_loudlog.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(mtr_[a-z0-9_]+)\s*\(", txt))) == sorted(NEW)
    assert re.search(r"#define\s+MTR_LOUDLOG_SAMPLE\s+0\b", txt) and re.search(r"#define\s+MTR_LOUDLOG_MAX\s+1\b", txt)


def test_engine_header_includes_it_inside_abi_2(M):
    main = open(os.path.join(INC, "mtr_engine.h")).read()
    assert re.search(r'^#include "mtr_loudlog.h"', main, flags=re.M)
    assert re.search(r"#define\s+MTR_ABI_VERSION\s+2\b", main)
    assert M.lib.mtr_abi_version() == 2
    assert not set(NEW) & set(M.exported_symbols())             # (mtr_engine.h itself declares what it declared)


def test_library_exports_and_engine_binds(M):
    for n in NEW:
        assert hasattr(M.lib, n), n
    for n in ("loudlog_set_period", "loudlog_period", "loudlog_series", "loudlog_reset"):
        assert hasattr(M.Engine, n), n
    assert (M.LOUDLOG_SAMPLE, M.LOUDLOG_MAX) == (0, 1)


def test_null_engine_is_an_argument_error(M):
    E, lib = M.engine, M.lib
    a, b = np.zeros(1, np.float32), np.zeros(1, np.float32)
    n, d = np.zeros(1, np.uint32), np.zeros(1, np.uint32)
    p, c, m = C.c_uint32(), C.c_uint32(), C.c_int()
    assert lib.mtr_engine_loudlog_set_period(None, 1, 1, 0) == E.ERR_ARG
    assert lib.mtr_engine_loudlog_period(None, C.byref(p), C.byref(c), C.byref(m)) == E.ERR_ARG
    assert lib.mtr_engine_loudlog_series(None, 0, 1, a.ctypes.data, b.ctypes.data, 1, n.ctypes.data, d.ctypes.data) == E.ERR_ARG
    assert lib.mtr_engine_loudlog_reset(None) == E.ERR_ARG
