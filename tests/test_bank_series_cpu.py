"""The 30-band bank's reading series (include/mtr_spectr.h) without a GPU: the surface, and the condition under which the GPU comparison
(tests/test_gpu_bank_series.py) can see a block end that is one frame off.  What the entry points compute is held on the GPU."""
import os
import re

import numpy as np
import pytest

import _bank as B
import _bank_series as BS
import meters.lv2_amd as M

HERE = os.path.dirname(os.path.abspath(__file__))
NEW = ["mtr_engine_spectr_period", "mtr_engine_spectr_series", "mtr_engine_spectr_set_period"]
ERR_ARG = -1


def test_the_new_header_declares_exactly_the_three_entry_points():
    assert M.exported_symbols("mtr_spectr.h") == NEW


def test_mtr_engine_h_includes_the_header_and_declares_none_of_them_itself():
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "mtr_engine.h")).read()
    assert re.search(r'^#include "mtr_spectr\.h"$', hdr, re.M)
    assert hdr.index("mtr_engine_spectrum (") < hdr.index('#include "mtr_spectr.h"') < hdr.index('#include "mtr_kmeter.h"')
    own = M.exported_symbols()
    assert not set(NEW) & set(own)
    for n in ("mtr_engine_spectr_set_speed", "mtr_engine_spectr_reset_peak", "mtr_engine_spectrum"):   # (those three stay where they were)
        assert n in own
    assert re.search(r"#define\s+MTR_ABI_VERSION\s+2\b", hdr) and M.lib.mtr_abi_version() == 2   # (an addition inside version 2)
    txt = open(os.path.join(os.path.dirname(HERE), "include", "mtr_spectr.h")).read()
    assert re.search(r"#define\s+MTR_SPECTR_PEAK_HOLD\s+0\b", txt) and re.search(r"#define\s+MTR_SPECTR_PEAK_BLOCK\s+1\b", txt)
    assert (M.SPECTR_PEAK_HOLD, M.SPECTR_PEAK_BLOCK) == (0, 1) == (BS.HOLD, BS.BLOCK)


def test_the_library_exports_them_and_the_binding_has_the_methods():
    for n in NEW:
        assert hasattr(M.lib, n), f"{n} is declared but libmtr_engine.so does not export it"
    for n in ("spectr_set_period", "spectr_period", "spectr_series"):
        assert callable(getattr(M.Engine, n))


def test_a_null_engine_is_an_argument_error():
    assert M.lib.mtr_engine_spectr_set_period(None, 4800, 16, 0) == ERR_ARG
    assert M.lib.mtr_engine_spectr_period(None, None, None, None) == ERR_ARG
    assert M.lib.mtr_engine_spectr_series(None, 0, 0, None, None, None, None, 0, None, None) == ERR_ARG
    assert M.lib.mtr_last_error()


# ---- what the GPU comparison can see ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("speed", [15.0, 1.0])
@pytest.mark.parametrize("P", [100, 129, 300])
def test_the_comparison_sees_a_block_end_one_frame_off(oracle, P, speed):
    """A series whose every block is cut one frame early (the first block has P - 1 frames) or late (P + 1) differs from the true one by
    more than 10 x BANK_REL in val, in at least one band of EVERY point: an engine that misplaced its block ends by a frame could not
    pass tests/test_gpu_bank_series.py's comparison with the oracle.  (Measured: all points; 99 % of the val entries at speed 15, 97 %
    at speed 1.)"""
    x = B.stream_input(0)
    true = BS.oracle_series(oracle, x, P, speed=speed)["val"].astype(np.float64)
    assert len(true) == B.T_CALLS // P
    for first in (P - 1, P + 1):
        off = BS.oracle_series(oracle, x, P, speed=speed, first=first)["val"].astype(np.float64)
        n = min(len(true), len(off))
        assert n >= len(true) - 1
        moved = np.abs(off[:n] - true[:n]) / true[:n] > 10 * B.BANK_REL
        print("speed %g P %d first block %d: %d of %d points seen, %.1f %% of the val entries" % (speed, P, first, moved.any(1).sum(), n, 100 * moved.mean()))
        assert moved.any(1).all(), (speed, P, first, np.flatnonzero(~moved.any(1)))


def test_the_peak_modes_differ_on_that_input(oracle):
    """MTR_SPECTR_PEAK_BLOCK against MTR_SPECTR_PEAK_HOLD at P = 100: val identical, max different in about a quarter of the entries
    (measured: 27 %) — wherever a block's own maximum lies below what was held before it"""
    x = B.stream_input(0)
    hold, block = BS.oracle_series(oracle, x, 100, BS.HOLD), BS.oracle_series(oracle, x, 100, BS.BLOCK)
    assert np.array_equal(BS.bits(hold["val"]), BS.bits(block["val"])) and np.array_equal(BS.bits(hold["val_db"]), BS.bits(block["val_db"]))
    differ = BS.bits(hold["max"]) != BS.bits(block["max"])
    print("max differs in %.1f %% of the entries" % (100 * differ.mean()))
    assert 0.2 < differ.mean() < 0.35
    assert (block["max"] <= hold["max"]).all() and np.array_equal(BS.bits(hold["max"][0]), BS.bits(block["max"][0]))
