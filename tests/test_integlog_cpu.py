"""The integration log (include/mtr_integlog.h) without a GPU: what the header declares, what the library exports and the binding offers,
the NULL-engine answers of the entry points, and mtr_integlog_cut — the arithmetic a host sizes its capacity with — against a loop that
walks the fragments one by one as Ebu_r128_proc::process does (ebumeter/ebu_r128_proc.cc:236: `if (++_div2 == 10)`)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

NEW = ("mtr_engine_integlog_set_every", "mtr_engine_integlog_every", "mtr_engine_integlog_series", "mtr_engine_integlog_reset",
       "mtr_integlog_cut")
INC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")


@pytest.fixture(scope="module")
def M():
    import meters.lv2_amd as m
    return m


def test_header_declares_exactly_the_five():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(INC, "mtr_integlog.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(mtr_[a-z0-9_]+)\s*\(", txt))) == sorted(NEW)


def test_engine_header_includes_it_inside_abi_2(M):
    main = open(os.path.join(INC, "mtr_engine.h")).read()
    assert re.search(r'^#include "mtr_integlog.h"', main, flags=re.M)
    assert re.search(r"#define\s+MTR_ABI_VERSION\s+2\b", main)
    assert M.lib.mtr_abi_version() == 2
    assert not set(NEW) & set(M.exported_symbols())             # (mtr_engine.h itself declares what it declared)
    assert sorted(M.exported_symbols("mtr_integlog.h")) == sorted(NEW)


def test_library_exports_and_engine_binds(M):
    for n in NEW:
        assert hasattr(M.lib, n), n
    for n in ("integlog_set_every", "integlog_every", "integlog_series", "integlog_reset", "_need_integlog"):
        assert hasattr(M.Engine, n), n
    assert callable(M.integlog_cut)
    assert M.INTEGLOG_FIELDS == ("I", "I_thr", "Rmin", "Rmax", "R_thr")


def test_null_engine_is_an_argument_error(M):
    E, lib = M.engine, M.lib
    v = [np.zeros(1, np.float32) for _ in range(5)]
    n, d = np.zeros(1, np.uint32), np.zeros(1, np.uint32)
    k, c = C.c_uint32(), C.c_uint32()
    assert lib.mtr_engine_integlog_set_every(None, 1, 1) == E.ERR_ARG
    assert lib.mtr_engine_integlog_every(None, C.byref(k), C.byref(c)) == E.ERR_ARG
    assert lib.mtr_engine_integlog_series(None, 0, 1, *[a.ctypes.data for a in v], 1, n.ctypes.data, d.ctypes.data) == E.ERR_ARG
    assert lib.mtr_engine_integlog_reset(None) == E.ERR_ARG


def brute(div2, evaluations, K, n_fragments):
    ev = pt = 0
    for _ in range(n_fragments):
        div2 += 1
        if div2 == 10:
            div2 = 0
            ev += 1
            if (evaluations + ev) % K == 0:
                pt += 1
    return ev, pt


def test_cut_against_a_fragment_by_fragment_count(M):
    for div2 in range(10):
        for K in (1, 2, 3, 7):
            for so_far in (0, 1, 5, 13):
                for n in range(46):
                    assert M.integlog_cut(div2, so_far, K, n) == brute(div2, so_far, K, n), (div2, so_far, K, n)
    # one large count: 2^40 + 7 fragments behind div2 = 6 and 2^33 + 1 evaluations, a point every 2^20
    n, so_far, K = 2 ** 40 + 7, 2 ** 33 + 1, 2 ** 20
    ev = (6 + n) // 10
    assert M.integlog_cut(6, so_far, K, n) == (ev, (so_far + ev) // K - so_far // K)
    assert M.integlog_cut(9, 0, 1, 1) == (1, 1) and M.integlog_cut(0, 0, 1, 9) == (0, 0)
    assert M.integlog_cut(3, 4, 0, 100) == (10, 0)                      # (K = 0: the log is off)


def test_cut_argument_errors(M):
    E, cut = M.engine, M.lib.mtr_integlog_cut
    ev, pt = C.c_uint64(), C.c_uint64()
    assert cut(10, 0, 1, 5, C.byref(ev), C.byref(pt)) == E.ERR_ARG
    assert cut(0, 0, 2 ** 20 + 1, 5, C.byref(ev), C.byref(pt)) == E.ERR_ARG
    assert cut(0, 0, 1, 5, None, C.byref(pt)) == E.ERR_ARG and cut(0, 0, 1, 5, C.byref(ev), None) == E.ERR_ARG
    assert cut(0, 2 ** 64 - 1, 1, 10, C.byref(ev), C.byref(pt)) == E.ERR_ARG
    assert cut(0, 0, 2 ** 20, 5, C.byref(ev), C.byref(pt)) == 0
