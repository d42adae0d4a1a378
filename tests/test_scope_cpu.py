"""MTR_METER_SCOPE (the stereoscope's and the phase wheel's FFT analysis for a batch) without a GPU: the header and the symbols, what
mtr_engine_create accepts, the NULL-engine answers, the window bit for bit, and the restatement of tests/_scope.py — the GPU tests'
yardstick — checked against what it must give on a sine and on silence, and for how many bins of the GPU tests' signals its bound on
the balance is stated at all; the numpy mirror of the kernel's passes against the DFT and against eps (W); and the census of the windows
the GPU modules run."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _scope

HERE = os.path.dirname(os.path.abspath(__file__))
INC = os.path.join(os.path.dirname(HERE), "include")
NEW = ("mtr_scope_window", "mtr_engine_scope_configure", "mtr_engine_scope_config", "mtr_engine_scope_read", "mtr_engine_scope_analyses",
       "mtr_engine_scope_reset")


@pytest.fixture(scope="module")
def M():
    import meters.lv2_amd as m
    return m


def test_symbols_and_abi(M):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(INC, "mtr_scope.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(mtr_[a-z0-9_]+)\s*\(", txt))) == sorted(NEW)
    main = open(os.path.join(INC, "mtr_engine.h")).read()
    assert re.search(r'^#include "mtr_scope.h"', main, flags=re.M)
    assert re.search(r"#define\s+MTR_METER_SCOPE\s+0x8000u", main) and re.search(r"#define\s+MTR_ABI_VERSION\s+2\b", main)
    names = M.exported_symbols("mtr_scope.h")
    assert not set(NEW) & set(M.exported_symbols())                # (what mtr_engine.h itself declares is pinned: tests/test_frames_cpu.py)
    for n in NEW:
        assert n in names, n
        assert hasattr(M.lib, n), n
    assert M.lib.mtr_abi_version() == 2
    for n in ("scope_configure", "scope_config", "scope_read", "scope_analyses", "scope_reset"):
        assert hasattr(M.Engine, n), n
    assert M.METER_SCOPE == 0x8000


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
    E, SC = M.engine, M.METER_SCOPE
    assert _create(M, 2, SC) in (0, E.ERR_NODEVICE), M.lib.mtr_last_error()
    for m in (M.METER_EBU | M.METER_TRUEPEAK, M.METER_STCORR | M.METER_KMETER, M.METER_NEEDLE, M.METER_DR14 | M.METER_SPECTR30 | M.METER_TPBALLIST):
        assert _create(M, 2, SC | m) in (0, E.ERR_NODEVICE), (m, M.lib.mtr_last_error())
    for ch in (1, 3, 4, 5):
        assert _create(M, ch, SC) == E.ERR_UNSUPPORTED, ch
    assert _create(M, 5, SC | M.METER_EBU) == E.ERR_UNSUPPORTED
    assert _create(M, 2, 0x10000) == E.ERR_ARG and _create(M, 2, 0x10000 | SC) == E.ERR_ARG
    assert _create(M, 2, 0x4000) == E.ERR_ARG and _create(M, 2, 0x4000 | SC) == E.ERR_ARG
    assert _create(M, 6, SC) == E.ERR_ARG                              # (6 .. 8 channels: the surround meter alone)


def test_null_engine_is_an_argument_error(M):
    E, lib = M.engine, M.lib
    f = np.zeros(8, np.float32)
    w, h, t, n = C.c_uint32(), C.c_uint32(), C.c_float(), C.c_uint64()
    assert lib.mtr_engine_scope_configure(None, 1024, 0, 1e-6) == E.ERR_ARG
    assert lib.mtr_engine_scope_config(None, C.byref(w), C.byref(h), C.byref(t)) == E.ERR_ARG
    assert lib.mtr_engine_scope_read(None, 0, 1, f.ctypes.data, None, None, None, None, None, None) == E.ERR_ARG
    assert lib.mtr_engine_scope_analyses(None, C.byref(n)) == E.ERR_ARG
    assert lib.mtr_engine_scope_reset(None) == E.ERR_ARG
    assert lib.mtr_scope_window(1024, None) == E.ERR_ARG


def test_window_bit_for_bit(M):
    E = M.engine
    for W in _scope.WINDOWS:
        got, want = M.scope_window(W), _scope.window(W)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), W
        assert got[0] == 0 and abs(float(got.astype(np.float64).sum()) - 2.0) < 1e-5
    out = np.full(40000, 7, np.float32)
    for W, rc in ((128, E.ERR_UNSUPPORTED), (12288, E.ERR_UNSUPPORTED), (6144, E.ERR_UNSUPPORTED), (1000, E.ERR_ARG), (32768, E.ERR_ARG),
                  (0, E.ERR_ARG), (64, E.ERR_ARG), (1025, E.ERR_ARG)):
        assert M.lib.mtr_scope_window(W, out.ctypes.data) == rc, W
    assert (out == 7).all()


@pytest.mark.parametrize("W", _scope.WINDOWS)
def test_a_sine_at_a_bin_centre_reads_its_amplitude(W):
    """the meaning of the 2 / sum normalisation: power = A^2 at the sine's bin, to 1e-5"""
    A, k = 0.3, W // 8 + 3
    x = np.zeros((W, 2), np.float32)
    x[:, 0] = (A * np.sin(2 * np.pi * k * np.arange(W) / W + 0.4)).astype(np.float32)
    x[:, 1] = (0.5 * A * np.cos(2 * np.pi * (k + 9) * np.arange(W) / W)).astype(np.float32)
    sc, n = _scope.run(x, W, W)
    assert n == 1
    assert abs(float(sc.power[0, k]) / A ** 2 - 1) < 1e-5 and abs(float(sc.power[1, k + 9]) / (0.5 * A) ** 2 - 1) < 1e-5
    assert abs(sc.p64[0, k] / A ** 2 - 1) < 1e-5
    assert int(np.argmax(sc.power[0])) == k and int(np.argmax(sc.power[1])) == k + 9
    assert sc.power[0, 0] == 0 and sc.power[0, W // 2 - 1] == 0          # never written


def test_silence_after_one_analysis():
    W = 1024
    sc, n = _scope.run(np.zeros((2 * W, 2), np.float32), W, W)
    assert n == 2
    s = slice(1, W // 2 - 1)
    assert (sc.lr[s] == np.float32(.5)).all() and (sc.level[s] == 0).all()
    assert (sc.phase == 0).all() and (sc.plevel == -100).all()
    assert sc.level[0] == -100 and sc.level[W // 2 - 1] == -100 and sc.lr[0] == np.float32(.5)
    assert 0 < float(sc.peak) < 1e-14                                    # two + 1e-15


def test_default_hop():
    assert _scope.default_hop(48000) == 1920 and _scope.default_hop(44100) == 1764 and _scope.default_hop(8000) == 320
    assert _scope.default_hop(22050) == 882 and _scope.default_hop(11025) == 441


def test_how_many_bins_the_bounds_cover():
    """tests/test_gpu_scope.py holds lr to 4 eps N / m on the bins whose m is at least LR_FLOOR of N, and lets at most 1 % of a case's
    bins fall outside that; it compares phase and plevel where no restated power lies within 1e-4 of the threshold, and lets at most 0.1 %
    of the bins lie there.  The restatement alone shows the seeds stay inside both caps (for the second: they leave no bin out)."""
    import test_gpu_scope as tg
    for W, hk in tg.CASES:
        H = tg.hop_of(W, hk)
        x = tg.signal_of(W, H)
        for s in range(x.shape[0]):
            sc = _scope.Scope(W).analyse(_scope.windowed(x[s], W, H, tg.NA - 1, _scope.window(W)))
            assert not tg.near_threshold(sc).any(), (W, H, s)
            rho, _ = _scope.ratios(x[s], W, H)
            out = float(np.mean(rho * tg.LR_FLOOR > 1))
            print(f"W {W} H {H} stream {s}: {100 * out:.3f} % of the bins below {tg.LR_FLOOR} N (below 1e-3 N: {100 * float(np.mean(rho > 1e3)):.2f} %)")
            assert out <= 0.01, (W, H, s, out)
    assert len(tg.CASES) == 21


@pytest.mark.parametrize("W", _scope.WINDOWS)
def test_the_mirror_of_the_kernels_passes(W):
    """_scope.mirror_fft restates k_scope's pass structure (radix-4 passes, the lane remap, the radix-2 pass of an odd log2 W, X [k] at
    slot bitrev (k)).  In complex128 it is the DFT: to 1e-13 of the norm.  In complex64, with the twiddles rounded once from double as the
    host makes them, it is what the kernel computes up to the device's contraction of cmul — and the yardstick for eps (W): on the
    signals of the GPU tests' CASES its |sqrt p - sqrt p64| / N must stay under the bound the kernel is held to."""
    import test_gpu_scope as tg
    rng = np.random.default_rng(300 + W)
    z = rng.normal(0, 1, (3, W)) + 1j * rng.normal(0, 1, (3, W))
    ref = np.fft.fft(z, axis=-1)
    d128 = float(np.linalg.norm(_scope.mirror_fft(z) - ref) / np.linalg.norm(ref))
    assert d128 <= 1e-13, (W, d128)
    win, worst = _scope.window(W), 0.0
    for hk in ("default", "quarter", "777"):
        H = tg.hop_of(W, hk)
        x = tg.signal_of(W, H)
        for s in range(x.shape[0]):
            fw = _scope.windowed(x[s], W, H, tg.NA - 1, win)
            sc = _scope.Scope(W).analyse(fw)
            p = _scope.mirror_powers(fw)
            assert p.dtype == np.float32
            worst = max(worst, float(np.max(np.abs(np.sqrt(p.astype(np.float64)) - np.sqrt(sc.p64)))) / sc.N)
    print(f"W {W}: the mirror in complex128: {d128:.2e} of the norm; in complex64: largest |sqrt p - sqrt p64| = {worst:.3e} N = "
          f"{worst / _scope.eps(W):.4f} of eps (W)")
    assert worst <= _scope.eps(W), (W, worst)


def test_every_window_is_run_by_every_scope_module(M):
    """the census: the windows of test_gpu_scope.CASES, of the series module's POINT_CASES and of test_gpu_scope_any.SHAPES are each
    exactly _scope.WINDOWS, and those are exactly the windows mtr_scope_window takes — an eighth window cannot arrive untested"""
    import test_gpu_scope as tg
    import test_gpu_scope_any as ta
    import test_gpu_scope_series as ts
    want = set(_scope.WINDOWS)
    assert len(_scope.WINDOWS) == len(want) == 7
    assert {W for W, _ in tg.CASES} == want
    assert {W for W, _, _ in ts.POINT_CASES} == want
    assert {W for W, _ in ta.SHAPES} == want
    out = np.zeros(1 << 17, np.float32)
    took = {W for W in range((1 << 17) + 1) if M.lib.mtr_scope_window(W, out.ctypes.data) == 0}
    assert took == want
