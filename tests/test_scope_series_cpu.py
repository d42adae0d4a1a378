"""The scope's reading series (include/mtr_scope_series.h) without a GPU: the header and the symbols, the binding's ctypes signatures
against the header's declarations, and mtr_scope_series_cut — the function a process call's step cuts the series with — against a
brute-force count, with its argument errors.  What the entry points compute is held on the GPU (tests/test_gpu_scope_series.py)."""
import ctypes as C
import os
import re

import numpy as np

import meters.lv2_amd as M

HERE = os.path.dirname(os.path.abspath(__file__))
INC = os.path.join(os.path.dirname(HERE), "include")
NEW = ["mtr_engine_scope_series", "mtr_engine_scope_series_config", "mtr_engine_scope_set_series", "mtr_scope_series_cut"]
MASKS = dict(LEVEL=1, LR=2, PHASE=4, PLEVEL=8, PEAK=16, POWER_L=32, POWER_R=64, ALL=127)
ERR_ARG = -1


def header():
    return open(os.path.join(INC, "mtr_scope_series.h")).read()


def test_the_header_declares_the_four_functions_and_the_masks():
    assert M.exported_symbols("mtr_scope_series.h") == NEW
    txt = header()
    for name, v in MASKS.items():
        assert re.search(r"#define\s+MTR_SCOPE_F_%s\s+%du\b" % (name, v), txt), name
        assert getattr(M, "SCOPE_F_" + name) == v
    scope = open(os.path.join(INC, "mtr_scope.h")).read()
    assert re.search(r'^#include "mtr_scope_series\.h"$', scope, re.M)
    assert not set(NEW) & set(M.exported_symbols())                    # (mtr_engine.h itself declares what it declared)
    main = open(os.path.join(INC, "mtr_engine.h")).read()
    assert re.search(r"#define\s+MTR_ABI_VERSION\s+2\b", main) and M.lib.mtr_abi_version() == 2   # (an addition inside version 2)


def test_the_library_exports_them_and_the_binding_has_the_methods():
    for n in NEW:
        assert hasattr(M.lib, n), f"{n} is declared but libmtr_engine.so does not export it"
    for n in ("scope_set_series", "scope_series_config", "scope_series"):
        assert callable(getattr(M.Engine, n))
    assert callable(M.scope_series_cut)


CTYPE = {"uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "uint32_t*": C.POINTER(C.c_uint32), "uint64_t*": C.POINTER(C.c_uint64),
         "float*": C.c_void_p, "mtr_engine*": C.c_void_p}            # (arrays and the handle go in as addresses)


def test_the_ctypes_signatures_match_the_header():
    txt = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    seen = []
    for ret, name, args in re.findall(r"\b(int)\s+(mtr_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", txt):
        want = []
        for a in args.split(","):
            m = re.match(r"\s*(?:const\s+)?([a-z0-9_]+)\s*(\*?)\s*[a-z0-9_]+\s*$", a)
            assert m, (name, a)
            want.append(CTYPE[m.group(1) + m.group(2)])
        fn = getattr(M.lib, name)
        assert list(fn.argtypes) == want, (name, fn.argtypes, want)
        assert fn.restype is C.c_int                                   # (ctypes' default: the status code)
        seen.append(name)
    assert sorted(seen) == NEW


def brute(fill, hop, since, every, n):
    an = pt = 0
    for _ in range(n):
        fill += 1
        if fill == hop:
            fill, an = 0, an + 1
            if every:
                since += 1
                if since == every:
                    since, pt = 0, pt + 1
    return an, pt


def test_the_cut_against_a_brute_force_count():
    rng = np.random.default_rng(27)
    cases = []
    for i in range(3000):
        hop = int(rng.integers(64, 400))
        every = int(rng.choice([0, 1, 1, 2, 3, 5, 25, 1000]))
        fill = int(rng.integers(0, hop))
        since = int(rng.integers(0, every)) if every else 0
        kind = i % 5
        n = (0, int(rng.integers(0, hop - fill)), int(rng.integers(0, 40 * hop)), hop - fill, int(rng.integers(0, 3 * hop)))[kind]
        cases.append((fill, hop, since, every, n))
    seen = dict(zero=0, no_analysis=0, k1=0, k_large=0, points=0)
    for c in cases:
        got, want = M.scope_series_cut(*c), brute(*c)
        assert got == want, (c, got, want)
        fill, hop, since, every, n = c
        seen["zero"] += n == 0
        seen["no_analysis"] += n > 0 and want[0] == 0
        seen["k1"] += every == 1 and want[0] > 0 and want[1] == want[0]
        seen["k_large"] += every > want[0] > 0 and want[1] == 0
        seen["points"] += want[1] > 0
    print(seen)
    assert min(seen.values()) >= 50, seen
    # sizes no loop reaches: the sum fill + n_frames does not overflow, and a hop at either end of its range
    assert M.scope_series_cut(63, 64, 0, 1, 2 ** 64 - 1) == ((2 ** 64 - 1 + 63) // 64, (2 ** 64 - 1 + 63) // 64)
    assert M.scope_series_cut(2 ** 20 - 1, 2 ** 20, 2 ** 20 - 1, 2 ** 20, 1) == (1, 1)
    assert M.scope_series_cut(0, 1920, 4, 5, 1919) == (0, 0) and M.scope_series_cut(1, 1920, 4, 5, 1919) == (1, 1)
    assert M.scope_series_cut(0, 1920, 7, 0, 19200) == (10, 0)          # (K = 0: the series is off, since is not looked at)


def test_the_argument_errors_of_the_cut():
    an, pt = C.c_uint64(7), C.c_uint64(7)
    cut = M.lib.mtr_scope_series_cut
    for bad in ((64, 64, 0, 1, 10), (100, 64, 0, 1, 10), (0, 64, 1, 1, 10), (0, 64, 5, 3, 10), (0, 63, 0, 1, 10), (0, 0, 0, 1, 10),
                (0, 2 ** 20 + 1, 0, 1, 10)):
        assert cut(*bad, C.byref(an), C.byref(pt)) == ERR_ARG, bad
        assert M.lib.mtr_last_error()
    assert cut(0, 64, 0, 1, 10, None, C.byref(pt)) == ERR_ARG and cut(0, 64, 0, 1, 10, C.byref(an), None) == ERR_ARG
    assert (an.value, pt.value) == (7, 7)                              # (nothing written on an error)
    assert cut(0, 64, 0, 1, 128, C.byref(an), C.byref(pt)) == 0 and (an.value, pt.value) == (2, 2)


def test_a_null_engine_is_an_argument_error():
    k = C.c_uint32()
    assert M.lib.mtr_engine_scope_set_series(None, 1, 16, 127) == ERR_ARG
    assert M.lib.mtr_engine_scope_series_config(None, C.byref(k), None, None) == ERR_ARG
    assert M.lib.mtr_engine_scope_series(None, 0, 0, None, None, None, None, None, None, None, 0, None, None) == ERR_ARG
    assert M.lib.mtr_last_error()
