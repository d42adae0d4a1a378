"""k_seg's screened products against its dense form, bit for bit.

The screened form (the default) runs the first of each 16-column chunk's three products and completes a chunk only where
one of its outputs may reach the running peak (mtr_seg.hip: SCREEN); MTR_SEG_SCREEN=0, read at engine creation, forces the
dense form.  The peaks must be the same bits on every input — only the time may depend on the data — and the loudness
path, which the screen does not touch, the same too."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from make_golden import tri_noise  # noqa: E402


@pytest.fixture(scope="module")
def M():
    import meters.lv2_amd as m
    return m


def _engine(M, screen, *a, **kw):
    old = os.environ.get("MTR_SEG_SCREEN")
    os.environ["MTR_SEG_SCREEN"] = "1" if screen else "0"
    try:
        return M.Engine(*a, **kw)
    finally:
        if old is None:
            del os.environ["MTR_SEG_SCREEN"]
        else:
            os.environ["MTR_SEG_SCREEN"] = old


def _run(M, screen, x, calls, fs=48000.0, meters=None, **kw):
    meters = meters if meters is not None else (M.METER_EBU | M.METER_TRUEPEAK)
    with _engine(M, screen, x.shape[0], fs, meters, **kw) as e:
        if meters & M.METER_EBU:
            e.integr_start()
        pos, per_call = 0, []
        for n in calls:
            e.process(np.ascontiguousarray(x[:, pos:pos + n]))
            per_call.append(np.array([[r.truepeak_call[0], r.truepeak_call[1]] for r in e.results()], np.float32))
            pos += n
        return dict(tp=e.truepeak(), per_call=np.stack(per_call), o9=e.out9() if meters & M.METER_EBU else None,
                    seg=e.seg_stats(), refine=e.refine_stats())


def _same(a, b, tag):
    assert a["seg"][0] > 0, (tag, "k_seg did not run", a["seg"])
    assert a["seg"] == b["seg"], tag
    assert np.array_equal(a["tp"].view(np.uint32), b["tp"].view(np.uint32)), (tag, a["tp"], b["tp"])
    assert np.array_equal(a["per_call"].view(np.uint32), b["per_call"].view(np.uint32)), tag
    if a["o9"] is not None:
        assert np.array_equal(a["o9"].view(np.uint32), b["o9"].view(np.uint32)), tag
    scr, fin = a["refine"]
    assert 0 < scr and fin <= scr, (tag, a["refine"])
    assert b["refine"] == (0, 0), (tag, "the dense form counts nothing", b["refine"])


def _both(M, x, calls, tag, **kw):
    a = _run(M, True, x, calls, **kw)
    b = _run(M, False, x, calls, **kw)
    _same(a, b, tag)
    return a


def _synth(M, S, T, kind, seed=777, fs=48000.0):
    import torch
    buf = torch.empty((S, T, 2), dtype=torch.float32, device="cuda")
    M.synth_fill_device(buf.data_ptr(), S, T, T, seed, fs, kind, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return buf.cpu().numpy()


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_screen_bench_signals(M, kind):
    """The bench's three syntheses (0 stationary noise, 1 programme, 2 noise under a rising level): same bits, and on noise and
    programme the screen completes fewer than half of the chunks it screens."""
    S, T = 16, 48000 * 4
    x = _synth(M, S, T, kind)
    a = _both(M, x, [T], "signal %d" % kind, tune_segments=4, tune_layout=7)
    scr, fin = a["refine"]
    if kind in (0, 1):
        assert fin < 0.5 * scr, (kind, a["refine"])


def test_screen_levels_and_sines(M):
    """Tiny levels (1e-30, below 2^-97: the clamped scale, f16 subnormals), sines whose inter-sample peaks are well above
    their sample peaks, and level jumps of 2^40 that force rescales and flushes of the accumulators' maxima."""
    T = 2400 * 30 + 517
    t = np.arange(T) / 48000.0
    rows = [tri_noise(T, 11, 1e-30), tri_noise(T, 12, 2.0 ** -110),
            np.stack([np.sin(2 * np.pi * 997 * t + 0.3), np.sin(2 * np.pi * 997 * t + 1.1)], 1).astype(np.float32) * 0.7,
            np.stack([np.sin(2 * np.pi * 11999 * t + 0.2), np.sin(2 * np.pi * 11999 * t + 2.0)], 1).astype(np.float32)]
    jump = tri_noise(T, 13, 2.0 ** -40)
    for k, pos in enumerate((5000, 31000, 60000)):
        jump[pos:] *= np.float32(2.0 ** 40) if k != 1 else np.float32(2.0 ** -40)
    rows.append(jump)
    up = tri_noise(T, 14, 1.0) * np.float32(2.0 ** -40)
    up[20000:] *= np.float32(2.0 ** 40)
    rows.append(up)
    x = np.stack(rows).astype(np.float32)
    _both(M, x, [T], "levels", tune_segments=3, tune_layout=7)


def test_screen_nan_inf(M):
    T = 2400 * 20
    x = np.stack([tri_noise(T, 20 + s, 0.5) for s in range(5)]).astype(np.float32)
    x[0, 7000, 0] = np.nan
    x[1, 15000, 1] = np.inf
    x[2, 30000:30016, :] = -np.inf
    x[3, 100, 0] = np.nan
    x[3, 40000, 1] = np.nan
    _both(M, x, [T], "nan/inf", tune_segments=3, tune_layout=7)


def test_screen_44k1_truepeak_only_ragged(M):
    """44.1 kHz (tiles that end inside a step), the true peak alone, and a ragged batch whose last wave has dead lanes."""
    fs = 44100.0
    T = 2205 * 24 + 777
    x = np.stack([tri_noise(T, 30 + s, 2.0 ** -(s % 5), period=30000) for s in range(7)]).astype(np.float32)
    _both(M, x, [T], "44.1k", fs=fs, tune_segments=3, tune_layout=7)
    _both(M, x, [T], "44.1k tp", fs=fs, meters=M.METER_TRUEPEAK, tune_segments=3, tune_layout=7)
    _both(M, x, [T], "48k tp ragged", meters=M.METER_TRUEPEAK, tune_segments=5, tune_layout=7)


@pytest.mark.parametrize("fs", [48000.0, 44100.0])
def test_screen_streaming_in_arbitrary_chunks(M, fs):
    T = int(fs) * 6 + 123
    x = np.stack([tri_noise(T, 40 + s, 0.8, period=20000) for s in range(3)]).astype(np.float32)
    frag = int(fs) // 20
    calls = [frag * 13 + 5, frag * 40 - 5, 333, frag * 20, T - (frag * 73 + 333)]
    _both(M, x, calls, "chunks %g" % fs, fs=fs, tune_segments=2, tune_layout=7)
