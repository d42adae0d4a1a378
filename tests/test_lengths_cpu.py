"""Per-stream lengths (mtr_engine_process_*_lengths): the surface, without a GPU.

The C ABI declares and exports the two entry points and the per-stream frame counter inside ABI version 2, and the Python
binding has the three methods a library-metering host calls.  The behaviour is held by tests/test_gpu_lengths.py.
"""
import os
import re

import pytest

import meters.lv2_amd as M

HERE = os.path.dirname(os.path.abspath(__file__))
NEW = ("mtr_engine_process_device_lengths", "mtr_engine_process_host_lengths", "mtr_engine_stream_frames")


def test_header_declares_and_library_exports_the_lengths_entry_points():
    names = M.exported_symbols()
    for n in NEW:
        assert n in names, f"{n} is not declared in include/mtr_engine.h"
        assert hasattr(M.lib, n), f"{n} is declared but libmtr_engine.so does not export it"
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "mtr_engine.h")).read()
    assert re.search(r"#define\s+MTR_ABI_VERSION\s+2\b", hdr)          # (an addition inside version 2)
    assert M.lib.mtr_abi_version() == 2


def test_binding_has_the_lengths_methods():
    for m in ("process_device_lengths", "process_lengths", "stream_frames"):
        assert callable(getattr(M.Engine, m, None)), m


@pytest.mark.parametrize("fn", ["mtr_engine_process_device_lengths", "mtr_engine_process_host_lengths"])
def test_null_engine_is_an_argument_error(fn):
    """No device needed: a NULL engine is refused before anything else (MTR_ERR_ARG)."""
    f = getattr(M.lib, fn)
    args = [None, None, 0, 0, None] + ([None] if fn.endswith("device_lengths") else [])
    assert f(*args) == -1
    assert M.lib.mtr_engine_stream_frames(None, 0, 0, None, None) == -1
