"""Track lengths for the whole-track meters (mtr_engine_process_*_tracks): the surface, without a GPU.

The C ABI declares (include/mtr_tracks.h, which mtr_engine.h includes next to the _lengths pair) and exports the two entry points
inside ABI version 2, and the Python binding has the two methods.  The behaviour is held by tests/test_gpu_tracks.py.
"""
import os
import re

import pytest

import meters.lv2_amd as M

HERE = os.path.dirname(os.path.abspath(__file__))
NEW = ("mtr_engine_process_device_tracks", "mtr_engine_process_host_tracks")


def test_header_declares_and_library_exports_the_tracks_entry_points():
    names = M.exported_symbols("mtr_tracks.h")
    assert set(names) == set(NEW)
    for n in NEW:
        assert hasattr(M.lib, n), f"{n} is declared but libmtr_engine.so does not export it"
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "mtr_engine.h")).read()
    assert re.search(r'^#include "mtr_tracks.h"', hdr, flags=re.M)      # (a client of mtr_engine.h sees them)
    assert re.search(r"#define\s+MTR_ABI_VERSION\s+2\b", hdr)          # (an addition inside version 2)
    assert M.lib.mtr_abi_version() == 2


def test_binding_has_the_tracks_methods():
    for m in ("process_device_tracks", "process_tracks"):
        assert callable(getattr(M.Engine, m, None)), m


@pytest.mark.parametrize("fn", NEW)
def test_null_engine_is_an_argument_error(fn):
    """No device needed: a NULL engine is refused before anything else (MTR_ERR_ARG)."""
    f = getattr(M.lib, fn)
    args = [None, None, 0, 0, None] + ([None] if fn.endswith("device_tracks") else [])
    assert f(*args) == -1
