"""MTR_METER_SURROUND (sur_run for a batch: C K-meters and up to four pair correlations, 3 .. 8 channels) without a GPU: the header and
the symbols, what mtr_engine_create accepts, the NULL-engine answers, the pick path at 6 and 8 picked channels, and the golden
vectors of the reference build replayed bit for bit by the composition the GPU tests use as their yardstick (tests/_sur.py)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
INC = os.path.join(os.path.dirname(HERE), "include")
NEW = ("mtr_engine_surround_set_pairs", "mtr_engine_surround_pairs", "mtr_engine_surround_set_period", "mtr_engine_surround_read",
       "mtr_engine_surround_pair_states", "mtr_engine_surround_series", "mtr_engine_surround_reset")


@pytest.fixture(scope="module")
def M():
    import meters.lv2_amd as m
    return m


def test_symbols_and_abi(M):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(INC, "mtr_surround.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(mtr_[a-z0-9_]+)\s*\(", txt))) == sorted(NEW)
    main = open(os.path.join(INC, "mtr_engine.h")).read()
    assert re.search(r'^#include "mtr_surround.h"', main, flags=re.M)
    assert re.search(r"#define\s+MTR_METER_SURROUND\s+0x2000u", main) and re.search(r"#define\s+MTR_ABI_VERSION\s+2\b", main)
    names = M.exported_symbols("mtr_surround.h")                   # (what mtr_engine.h itself declares is pinned: tests/test_frames_cpu.py)
    assert not set(NEW) & set(M.exported_symbols())
    for n in NEW:
        assert n in names, n
        assert hasattr(M.lib, n), n
    assert M.lib.mtr_abi_version() == 2
    for n in ("surround_set_pairs", "surround_pairs", "surround_set_period", "surround_read", "surround_pair_states", "surround_series",
              "surround_reset"):
        assert hasattr(M.Engine, n), n
    assert M.METER_SURROUND == 0x2000


def _create(M, n_channels, meters):
    cfg = M.engine._Config(struct_size=C.sizeof(M.engine._Config), meters=meters, n_streams=4, n_channels=n_channels,
                           sample_rate=48000.0, device=0)
    h = C.c_void_p()
    rc = M.lib.mtr_engine_create(C.byref(cfg), C.byref(h))
    if h.value:
        M.lib.mtr_engine_destroy(h)
    return rc


def test_what_create_accepts(M):
    """(the argument checks run before the device check)"""
    E, SUR = M.engine, M.METER_SURROUND
    for ch in range(3, 9):
        assert _create(M, ch, SUR) in (0, E.ERR_NODEVICE), (ch, M.lib.mtr_last_error())
    for ch in (3, 4, 5):
        for m in (M.METER_EBU, M.METER_TRUEPEAK, M.METER_EBU | M.METER_TRUEPEAK):
            assert _create(M, ch, SUR | m) in (0, E.ERR_NODEVICE), (ch, m, M.lib.mtr_last_error())
    # 6 .. 8 channels take it alone: with anything else they stay the argument error every engine of more than 5 channels was
    for ch in (6, 7, 8):
        assert _create(M, ch, SUR | M.METER_EBU) == E.ERR_ARG
        assert _create(M, ch, SUR | M.METER_TRUEPEAK) == E.ERR_ARG
        assert _create(M, ch, M.METER_EBU | M.METER_TRUEPEAK) == E.ERR_ARG
        assert _create(M, ch, M.METER_KMETER) == E.ERR_ARG
    assert _create(M, 9, SUR) == E.ERR_ARG
    for ch in (1, 2):
        assert _create(M, ch, SUR) == E.ERR_UNSUPPORTED
        assert _create(M, ch, SUR | M.METER_KMETER) == E.ERR_UNSUPPORTED
    assert _create(M, 5, SUR | M.METER_KMETER) == E.ERR_UNSUPPORTED       # (3 .. 5 channels: EBU, TRUEPEAK and SURROUND alone)
    assert _create(M, 2, 0x1000) == E.ERR_ARG and _create(M, 6, 0x1000) == E.ERR_ARG and _create(M, 5, 0x1000 | SUR) == E.ERR_ARG
    assert _create(M, 2, 0x4000) == E.ERR_ARG


def test_plan_query_follows_create(M):
    assert M.plan_query(4, 48000, meters=M.METER_SURROUND, n_channels=6)["layout"] == 3           # (no K-weighting kernel in it)
    assert M.plan_query(4, 48000, meters=M.METER_SURROUND | M.METER_EBU | M.METER_TRUEPEAK, n_channels=5)["layout"] == 8
    for ch, m in ((6, M.METER_SURROUND | M.METER_EBU), (8, M.METER_EBU), (9, M.METER_SURROUND)):
        with pytest.raises(M.EngineError) as err:
            M.plan_query(4, 48000, meters=m, n_channels=ch)
        assert err.value.code == M.engine.ERR_ARG


def test_null_engine_is_an_argument_error(M):
    E, lib = M.engine, M.lib
    a, b = np.zeros(4, np.uint8), np.zeros(4, np.uint8)
    f = np.zeros(64, np.float32)
    n, d = C.c_uint32(), C.c_uint32()
    assert lib.mtr_engine_surround_set_pairs(None, a.ctypes.data, b.ctypes.data) == E.ERR_ARG
    assert lib.mtr_engine_surround_pairs(None, a.ctypes.data, b.ctypes.data) == E.ERR_ARG
    assert lib.mtr_engine_surround_set_period(None, 4800, 4) == E.ERR_ARG
    assert lib.mtr_engine_surround_read(None, 0, 1, f.ctypes.data, f.ctypes.data, f.ctypes.data) == E.ERR_ARG
    assert lib.mtr_engine_surround_pair_states(None, 0, 1, f.ctypes.data) == E.ERR_ARG
    assert lib.mtr_engine_surround_series(None, 0, 1, f.ctypes.data, f.ctypes.data, f.ctypes.data, 1, C.byref(n), C.byref(d)) == E.ERR_ARG
    assert lib.mtr_engine_surround_reset(None) == E.ERR_ARG


@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
def test_pick_path_takes_up_to_eight_channels(M, fmt):
    """mtr_pick_decode_host with 6 and 8 picked channels is numpy indexing (tests/test_frames_cpu.py pins 1 .. 5); 9 is still refused"""
    import test_frames_cpu as tf
    for fc, m in ((6, (0, 1, 2, 4, 5, 3)), (8, (0, 1, 2, 4, 5, 3)), (8, (7, 6, 5, 4, 3, 2, 1, 0)), (6, (5, 5, 0, 1, 2, 3, 4, 0)), (8, (0, 1, 2, 3, 4, 5, 6))):
        for n in (0, 1, 7, 1001):
            raw, want = tf._source(fmt, n, fc, 900 + 10 * fmt + fc)
            for shift in ((0, 1, 3) if fmt else (0, 4)):
                got = tf._pick_at(fmt, raw, n, fc, m, shift)
                ref = np.ascontiguousarray(want[:, list(m)])
                assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (fmt, fc, m, n, shift)
    src, dst = np.zeros(1024, np.uint8), np.zeros(64, np.float32)
    nine = np.arange(9, dtype=np.uint8) % 8
    assert M.lib.mtr_pick_decode_host(fmt, src.ctypes.data, 4, 8, nine.ctypes.data, 9, dst.ctypes.data) == -1
    assert M.lib.mtr_pick_decode_host(fmt, src.ctypes.data, 4, 9, nine.ctypes.data, 8, dst.ctypes.data) == -1
    assert (dst == 0).all()


@pytest.mark.parametrize("fs", [48000, 44100])
@pytest.mark.parametrize("nch", [8, 5])
def test_the_composition_replays_the_reference_build(oracle, fs, nch):
    """tests/golden/golden_surround_v1.npz (written from oracle/_ref by tests/golden/make_golden_surround.py) bit for bit"""
    import _sur
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_golden_surround as mk
    z = np.load(os.path.join(HERE, "golden", "golden_surround_v1.npz"))
    assert os.path.getsize(os.path.join(HERE, "golden", "golden_surround_v1.npz")) < 100 * 1024
    x = mk.signal(float(fs))[:, :nch]
    assert x.shape == (fs, nch)
    n = fs // mk.B
    ends = [mk.B * (k + 1) for k in range(n)]
    level, peak, corr, _ = _sur.run_oracle(_sur.bind(oracle.lib), fs, np.ascontiguousarray(x), ends, pairs=mk.CASES[nch])
    tag = f"{nch}_{fs}"
    for name, got in (("level", level), ("peak", peak), ("corr", corr)):
        want = z[f"{name}_{tag}"]
        assert want.shape == got.shape and want.dtype == np.float32
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, tag)
    assert level.any() and peak.any() and corr.any()


def test_the_restatements_follow_the_oracle(oracle):
    """the float64 restatements of tests/_sur.py (the GPU tests' measure of the reference's own rounding) sit where they should:
    within 1e-5 of the oracle on plain noise, and flushed where it is on samples that are not finite"""
    import _sur
    fs, nch = 48000, 6
    x = _sur.signals(12000, fs, nch, seed=3, S=3)
    x[1, 5000, 2] = np.nan
    x[2, 7999, 4] = np.inf                                            # the last frame of a block: Kmeterdsp keeps the Inf
    x[2, 9000, 1] = np.inf
    ends = [4000, 8000, 12000]
    lib = _sur.bind(oracle.lib)
    w12 = (np.float32(6.28) * np.float32(2e3) / np.float32(fs), np.float32(1) / (np.float32(0.3) * np.float32(fs)))
    lv, co, st = _sur.run_exact(fs, w12, x, ends)
    for s in range(3):
        level, _, corr, states = _sur.run_oracle(lib, fs, x[s], ends)
        fin = np.isfinite(level)
        assert np.array_equal(fin, np.isfinite(lv[:, s])), (s, level, lv[:, s])
        assert np.all(_sur.rel(lv[:, s][fin], level[fin], np.abs(level[fin])) < 1e-5), (s, level, lv[:, s])
        assert np.array_equal(level == 0, lv[:, s] == 0)
        assert np.all(np.abs(co[:, s] - corr) < 1e-5), (s, corr, co[:, s])
        assert np.all(_sur.rel(st[:, s], states, _sur.scale_of(states)) < 1e-4)
