"""Track lengths for the true-peak bar (include/mtr_tpb_ends.h): the surface, without a GPU.  What the entry points compute is held on the
GPU: tests/test_gpu_tpb_ends.py."""
import os
import re

import numpy as np

import meters.lv2_amd as M

HERE = os.path.dirname(os.path.abspath(__file__))
NEW = ["mtr_engine_process_device_tpb", "mtr_engine_process_host_tpb", "mtr_engine_tpb_points"]
ERR_ARG = -1


def test_the_header_declares_the_three_entry_points_and_the_library_exports_them():
    assert M.exported_symbols("mtr_tpb_ends.h") == NEW
    assert not set(NEW) & set(M.exported_symbols()) and not set(NEW) & set(M.exported_symbols("mtr_ends.h"))
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "mtr_engine.h")).read()
    assert re.search(r'^#include "mtr_tpb_ends\.h"$', hdr, re.M)
    assert hdr.index('#include "mtr_ends.h"') < hdr.index('#include "mtr_tpb_ends.h"') < hdr.index("mtr_engine_stream_frames (")
    assert re.search(r"#define\s+MTR_ABI_VERSION\s+2\b", hdr) and M.lib.mtr_abi_version() == 2   # (an addition inside version 2)
    for n in NEW:
        assert hasattr(M.lib, n), f"{n} is declared but libmtr_engine.so does not export it"


def test_the_binding_has_the_three_methods():
    for n in ("process_device_tpb", "process_tpb", "tpb_points"):
        assert callable(getattr(M.Engine, n))
    assert M.Engine._FAMILY["tpb"][0] == "mtr_engine_process_device_tpb"


def test_null_arguments_are_argument_errors_under_the_pairs_own_name():
    """without a device: the checks come before anything is queued"""
    f = np.zeros(1, np.uint64)
    x = np.zeros(8, np.float32)
    for args in ((None, x.ctypes.data, 4, 4, f.ctypes.data, None), (None, None, 0, 0, f.ctypes.data, None), (None, x.ctypes.data, 4, 4, None, None)):
        assert M.lib.mtr_engine_process_device_tpb(*args) == ERR_ARG
        assert M.lib.mtr_last_error() == b"mtr_engine_process_device_tpb: null argument"
        assert M.lib.mtr_engine_process_host_tpb(*args[:5]) == ERR_ARG
        assert M.lib.mtr_last_error() == b"mtr_engine_process_host_tpb: null argument"
    assert M.lib.mtr_engine_tpb_points(None, 0, 0, f.ctypes.data) == ERR_ARG
    assert M.lib.mtr_engine_tpb_points(None, 0, 0, None) == ERR_ARG
    assert M.lib.mtr_last_error()
