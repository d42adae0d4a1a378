"""The true-peak bar's reading series (include/mtr_tpb.h): the surface, without a GPU.  What the entry points compute is held on the GPU:
tests/test_gpu_tpb_series.py."""
import os
import re

import meters.lv2_amd as M

HERE = os.path.dirname(os.path.abspath(__file__))
NEW = ["mtr_engine_tpb_period", "mtr_engine_tpb_series", "mtr_engine_tpb_set_period"]
ERR_ARG = -1


def test_the_new_header_declares_exactly_the_three_entry_points():
    assert M.exported_symbols("mtr_tpb.h") == NEW


def test_mtr_engine_h_includes_the_header_and_declares_none_of_them_itself():
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "mtr_engine.h")).read()
    assert re.search(r'^#include "mtr_tpb\.h"$', hdr, re.M)
    assert not set(NEW) & set(M.exported_symbols())
    assert re.search(r"#define\s+MTR_ABI_VERSION\s+2\b", hdr) and M.lib.mtr_abi_version() == 2   # (an addition inside version 2)


def test_the_library_exports_them_and_the_binding_has_the_methods():
    for n in NEW:
        assert hasattr(M.lib, n), f"{n} is declared but libmtr_engine.so does not export it"
    for n in ("tpb_set_period", "tpb_period", "tpb_series"):
        assert callable(getattr(M.Engine, n))


def test_a_null_engine_is_an_argument_error():
    assert M.lib.mtr_engine_tpb_set_period(None, 4800, 16) == ERR_ARG
    assert M.lib.mtr_engine_tpb_period(None, None, None) == ERR_ARG
    assert M.lib.mtr_engine_tpb_series(None, 0, 0, None, None, 0, None, None) == ERR_ARG
    assert M.lib.mtr_last_error()
