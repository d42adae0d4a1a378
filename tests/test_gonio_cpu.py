"""MTR_METER_GONIO (the goniometer's M/S point image, auto gain and reading series for a batch) without a GPU: the header and the
symbols, what mtr_engine_create accepts, the NULL-engine answers, mtr_gonio_derive bit for bit against the restatement of
tests/_gonio.py — the GPU tests' yardstick — and that restatement against facts that follow from the formulas."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _gonio

HERE = os.path.dirname(os.path.abspath(__file__))
INC = os.path.join(os.path.dirname(HERE), "include")
NEW = ("mtr_gonio_derive", "mtr_engine_gonio_configure", "mtr_engine_gonio_config", "mtr_engine_gonio_set_gain", "mtr_engine_gonio_image",
       "mtr_engine_gonio_read", "mtr_engine_gonio_blocks", "mtr_engine_gonio_series", "mtr_engine_gonio_image_clear", "mtr_engine_gonio_reset",
       "mtr_engine_gonio_timing")


@pytest.fixture(scope="module")
def M():
    import meters.lv2_amd as m
    return m


def test_symbols_and_abi(M):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(INC, "mtr_gonio.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(mtr_[a-z0-9_]+)\s*\(", txt))) == sorted(NEW)
    main = open(os.path.join(INC, "mtr_engine.h")).read()
    assert re.search(r'^#include "mtr_gonio.h"', main, flags=re.M)
    assert main.index('#include "mtr_gonio.h"') > main.index('#include "mtr_scope.h"')     # behind the other meter headers
    assert re.search(r"#define\s+MTR_METER_GONIO\s+0x20000u", main) and re.search(r"#define\s+MTR_ABI_VERSION\s+2\b", main)
    names = M.exported_symbols("mtr_gonio.h")
    assert not set(NEW) & set(M.exported_symbols())                # (what mtr_engine.h itself declares is pinned: tests/test_frames_cpu.py)
    for n in NEW:
        assert n in names, n
        assert hasattr(M.lib, n), n
    assert M.lib.mtr_abi_version() == 2
    for n in ("gonio_configure", "gonio_config", "gonio_set_gain", "gonio_image", "gonio_read", "gonio_blocks", "gonio_series",
              "gonio_image_clear", "gonio_reset"):
        assert hasattr(M.Engine, n), n
    assert M.METER_GONIO == 0x20000 and callable(M.gonio_derive)


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
    E, GO = M.engine, M.METER_GONIO
    assert _create(M, 2, GO) in (0, E.ERR_NODEVICE), M.lib.mtr_last_error()
    every = M.METER_EBU | M.METER_TRUEPEAK | M.METER_STCORR | M.METER_NEEDLE | M.METER_SCOPE
    assert _create(M, 2, GO | every) in (0, E.ERR_NODEVICE), M.lib.mtr_last_error()
    for ch in (1, 3, 4, 5):
        assert _create(M, ch, GO) == E.ERR_UNSUPPORTED, ch
    assert _create(M, 2, 0x10000) == E.ERR_ARG and _create(M, 2, 0x10000 | GO) == E.ERR_ARG
    assert _create(M, 2, 0x40000) == E.ERR_ARG


def test_null_engine_is_an_argument_error(M):
    E, lib = M.engine, M.lib
    cfg = M.gonio_config()
    b = C.c_uint64()
    f = np.zeros(8, np.float32)
    assert lib.mtr_engine_gonio_configure(None, C.byref(cfg)) == E.ERR_ARG
    assert lib.mtr_engine_gonio_config(None, C.byref(cfg), None) == E.ERR_ARG
    assert lib.mtr_engine_gonio_set_gain(None, 1.0) == E.ERR_ARG
    assert lib.mtr_engine_gonio_image(None, 0, 1, None, None, None, None) == E.ERR_ARG
    assert lib.mtr_engine_gonio_read(None, 0, 1, f.ctypes.data, None, None) == E.ERR_ARG
    assert lib.mtr_engine_gonio_blocks(None, C.byref(b), None) == E.ERR_ARG
    assert lib.mtr_engine_gonio_series(None, 0, 1, 0, 1, f.ctypes.data, None, None) == E.ERR_ARG
    assert lib.mtr_engine_gonio_image_clear(None) == E.ERR_ARG
    assert lib.mtr_engine_gonio_reset(None) == E.ERR_ARG
    assert lib.mtr_engine_gonio_timing(None, 0, None, None, None) == E.ERR_ARG
    assert lib.mtr_gonio_derive(None, 48000.0, C.byref(M.GonioDerived())) == E.ERR_ARG
    assert lib.mtr_gonio_derive(C.byref(cfg), 48000.0, None) == E.ERR_ARG


def _bits(v):
    return np.asarray(v, np.float32).view(np.uint32).tolist()


@pytest.mark.parametrize("rate,p0", [(44100.0, 1764), (48000.0, 1920), (96000.0, 3840)])
@pytest.mark.parametrize("dials", [None, (0.0, 100.0, 0.0, 100.0)])
@pytest.mark.parametrize("P", [0, 480])
def test_derive_bit_for_bit(M, rate, p0, dials, P):
    for shift in (1, 2, 3):
        got = M.gonio_derive(rate, period_frames=P, capacity=8, shift=shift, autogain=1, dials=dials)
        want = _gonio.derive(rate, P, dials or _gonio.DIALS, shift)
        assert got.period_frames == want.P == (P or p0)
        assert got.G == want.G == {1: 187, 2: 94, 3: 47}[shift]
        assert _bits([got.hpw, got.attack[0], got.attack[1], got.g_target, got.g_rms]) == \
            _bits([want.hpw, want.attack[0], want.attack[1], want.g_target, want.g_rms])
    if dials:                                                              # target dial 0: exp (1.8); rms dial 100: 1
        assert got.g_target == np.float32(np.exp(1.8)) and got.g_rms == 1.0


def test_bad_configurations(M):
    E = M.engine
    d = M.GonioDerived()

    def rc(**kw):
        c = M.gonio_config(**kw)
        return M.lib.mtr_gonio_derive(C.byref(c), 48000.0, C.byref(d))

    assert rc() == 0 and d.period_frames == 1920 and d.G == 94
    assert rc(period_frames=64, capacity=1) == 0 and rc(period_frames=1 << 20, capacity=1) == 0
    for kw in (dict(period_frames=63, capacity=4), dict(period_frames=(1 << 20) + 1, capacity=4), dict(shift=4), dict(period_frames=480),
               dict(gain=float("nan")), dict(gain=-1.0), dict(gain=float("inf")), dict(point_width=float("nan")), dict(autogain=3),
               dict(dials=(54, 58, 40, 101)), dict(dials=(float("nan"), 58, 40, 50)), dict(tune_piece=63), dict(tune_piece=(1 << 20) + 1)):
        assert rc(**kw) == E.ERR_ARG, kw
    c = M.gonio_config(autogain=1)
    c.g_attack = 10.0                                                      # dials without autogain 2
    assert M.lib.mtr_gonio_derive(C.byref(c), 48000.0, C.byref(d)) == E.ERR_ARG
    c = M.gonio_config()
    c.struct_size = 8
    assert M.lib.mtr_gonio_derive(C.byref(c), 48000.0, C.byref(d)) == E.ERR_ARG
    assert M.lib.mtr_gonio_derive(C.byref(M.gonio_config()), 4000.0, C.byref(d)) == E.ERR_ARG
    # shift "0" is the default, not a shift of its own
    assert M.gonio_derive(48000.0, shift=0).G == 94


# ---- the restatement against what follows from the formulas ---------------------------------------------------------------------------

def test_silence_paints_nothing():
    g = _gonio.Gonio(3, 48000.0, P=480).run(np.zeros((3, 2000, 2), np.float32))
    assert (g.drawn == 0).all() and (g.clipped == 0).all() and (g.skipped == 2000).all() and not g.img.any()
    assert len(g.series) == 4 and g.j == 80
    # (lp creeps by 1e-12f per frame: far below a cell)
    assert (g.last_x == _gonio.CENTER).all() and (np.abs(g.lp0) < 1e-8).all()


@pytest.mark.parametrize("gain", [1.0, 2.5])
def test_a_constant_left_channel_settles_on_one_cell(gain):
    """L = a, R = 0: lp0 -> a, ax = ay = a, so x = y = 186.5 - 100 a gain; behind the approach every point lands in that one cell"""
    a = 0.4
    x = np.zeros((1, 8000, 2), np.float32)
    x[:, :, 0] = a
    g = _gonio.Gonio(1, 48000.0, P=1920, gain=gain).run(x[:, :4000])
    assert abs(float(g.lp0[0]) - a) < 1e-5
    target = 186.5 - 100 * a * gain
    assert abs(float(g.last_x[0]) - target) < 1.5 and abs(float(g.last_y[0]) - target) < 1.5     # within the skip rule's sqrt (2)
    g.image_clear()
    g.run(x[:, 4000:])
    assert g.drawn[0] == 0 and g.skipped[0] == 4000                       # settled: nothing moves sqrt (2) any more
    # ... and on the way there every point lay on the diagonal x = y, the last ones in the target's cell
    g2 = _gonio.Gonio(1, 48000.0, P=1920, gain=gain).run(x)
    ys, xs = np.nonzero(g2.img[0])
    assert (ys == xs).all()
    c = int(np.rint(np.float32(g2.last_x[0] - np.float32(0.875)))) >> 2
    assert g2.img[0, c, c] > 0 and abs(c - int(target - 0.875) // 4) <= 1


def test_every_frame_is_counted_once():
    T = 3000
    x = _gonio.signals(16, T, seed=5)
    for kw in (dict(gain=1.0), dict(gain=4.0), dict(autogain=True), dict(shift=1), dict(shift=3)):
        g = _gonio.Gonio(16, 48000.0, P=480, **kw).run(x)
        assert ((g.drawn + g.clipped + g.skipped) == T).all(), kw
        assert (g.img.reshape(16, -1).sum(axis=1, dtype=np.uint64) == g.drawn).all(), kw
        gs, ds, cs = g.series_arrays()
        assert gs.shape == (16, T // 480)
        assert (ds.sum(axis=1) <= g.drawn).all() and (cs.sum(axis=1) <= g.clipped).all()
    _gonio.coverage(_gonio.Gonio(16, 48000.0, P=480, gain=4.0).run(x), T)


def test_cutting_the_audio_changes_nothing():
    x = _gonio.signals(8, 2500, seed=6)
    a = _gonio.Gonio(8, 48000.0, P=100, autogain=True).run(x)
    b = _gonio.Gonio(8, 48000.0, P=100, autogain=True)
    for lo, hi in ((0, 1), (1, 256), (256, 513), (513, 2500)):
        b.run(x[:, lo:hi])
    assert np.array_equal(a.img, b.img) and np.array_equal(a.gain.view(np.uint32), b.gain.view(np.uint32))
    assert all(np.array_equal(p.view(np.uint32), q.view(np.uint32)) for p, q in zip(a.series_arrays(), b.series_arrays()))


def test_the_gain_of_a_quiet_stream_runs_to_the_floor_at_p_480():
    """P = 480 at 48 kHz: elapsed = .01, so .03 + .007 logf (.01) < 0 and the attack factor of :524 on the side where the target lies above
    the gain is NEGATIVE: the gain of a quiet stream (target 100) moves away from the target until the floor of :527 holds it.  The
    reference's own behaviour at such a short display update; reproduced, not repaired."""
    d = _gonio.derive(48000.0, 480)
    assert d.attack[1] < 0 < d.attack[0]
    d25 = _gonio.derive(48000.0, 0)
    assert d25.attack[1] > 0 and d25.attack[0] > 0                         # the plugin's own period has none of it
    g = _gonio.Gonio(2, 48000.0, P=480, autogain=True).run(np.zeros((2, 480 * 40, 2), np.float32))
    gs = g.series_arrays()[0]
    assert (np.diff(gs[0].astype(np.float64)) <= 0).all() and gs[0, 0] < 1.0
    assert gs[0, -1] == np.float32(.001) and g.gain[0] == np.float32(.001)
