"""k_seg's screen with the stream reference, against the dense form bit for bit.

The screened form (the default) lets a chunk pass its check where its first-product values stay eps under the largest value
the launch has already counted for the column's (stream, channel) — the maximum over the wave's lanes of the same stream —
and reads a chunk's lo operands only where it completes (mtr_seg.hip: SCREEN and the stream reference).  MTR_SEG_SCREEN=0,
read at engine creation, forces the dense form.  Held here: the peaks of the call (truepeak_call), the hold (truepeak) and
the loudness outputs are the same bits, on segment levels far apart (the converted reference overflows and underflows),
segment counts that make streams straddle lane groups and waves, neighbouring streams of very different level, NaN / Inf,
per-stream lengths whose closing segments go to k_kwtp16_len, 44.1 kHz, the true peak alone and streaming in arbitrary
chunks; and, on the bench programme, the share of chunks that complete."""
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


def _run(M, screen, x, calls, fs=48000.0, meters=None, lengths=None, **kw):
    """calls: frames per call; lengths (optional): [calls][S] frames of each stream in each call (process_lengths)."""
    meters = meters if meters is not None else (M.METER_EBU | M.METER_TRUEPEAK)
    with _engine(M, screen, x.shape[0], fs, meters, tune_layout=7, **kw) as e:
        if meters & M.METER_EBU:
            e.integr_start()
        pos, per_call = 0, []
        for k, n in enumerate(calls):
            blk = np.ascontiguousarray(x[:, pos:pos + n])
            if lengths is None:
                e.process(blk)
            else:
                e.process_lengths(blk, np.asarray(lengths[k], np.uint64))
            per_call.append(np.array([[r.truepeak_call[0], r.truepeak_call[1]] for r in e.results()], np.float32))
            pos += n
        return dict(tp=e.truepeak(), per_call=np.stack(per_call), o9=e.out9() if meters & M.METER_EBU else None,
                    seg=e.seg_stats(), refine=e.refine_stats())


def _both(M, x, calls, tag, **kw):
    a = _run(M, True, x, calls, **kw)
    b = _run(M, False, x, calls, **kw)
    assert a["seg"][0] > 0, (tag, "k_seg did not run", a["seg"])
    assert a["seg"] == b["seg"], tag
    assert np.array_equal(a["tp"].view(np.uint32), b["tp"].view(np.uint32)), (tag, a["tp"], b["tp"])
    assert np.array_equal(a["per_call"].view(np.uint32), b["per_call"].view(np.uint32)), (tag, a["per_call"], b["per_call"])
    if a["o9"] is not None:
        assert np.array_equal(a["o9"].view(np.uint32), b["o9"].view(np.uint32)), tag
    scr, fin = a["refine"]
    assert 0 < scr and fin <= scr, (tag, a["refine"])
    assert b["refine"] == (0, 0), (tag, "the dense form counts nothing", b["refine"])
    return a, b


def _sine(T, f, a, ph=(0.3, 1.1), fs=48000.0):
    t = np.arange(T) / fs
    return (np.stack([np.sin(2 * np.pi * f * t + ph[0]), np.sin(2 * np.pi * f * t + ph[1])], 1) * a).astype(np.float32)


@pytest.mark.parametrize("loud_first", [True, False])
def test_levels_far_apart_within_a_stream(M, loud_first):
    """Segments far apart in level within one stream, the loud one first or last: 2^40 (1 and 2^-40), 2^130 (2^30 and
    2^-100: the quiet columns' converted reference overflows to +Inf) and 2^200 (2^100 and 2^-100, the true peak alone: a level
    that jumps inside a segment leaves the loud columns a reference that underflows until it is renewed)."""
    T = 2400 * 40
    q = T // 4

    def row(seed, hi, lo, sig=None):
        x = tri_noise(T, seed, 1.0, period=9000) if sig is None else sig
        g = np.full(T, lo, np.float32)
        if loud_first:
            g[:q] = hi
        else:
            g[3 * q:] = hi
        return x * g[:, None]

    rows = [row(50, 1.0, 2.0 ** -40), row(51, 2.0 ** 30, 2.0 ** -100),
            row(52, 1.0, 2.0 ** -40, sig=_sine(T, 11999, 0.7))]     # inter-sample peaks above the sample peaks: pm decides
    _both(M, np.stack(rows).astype(np.float32), [T], "levels far apart", tune_segments=4)
    jump = tri_noise(T, 53, 1.0, period=9000) * np.float32(2.0 ** -100)
    jump[T * 5 // 8:] *= np.float32(2.0 ** 100)
    jump[T * 5 // 8:] *= np.float32(2.0 ** 100)
    rows += [row(54, 2.0 ** 100, 2.0 ** -100), jump]
    _both(M, np.stack(rows).astype(np.float32), [T], "levels far apart, tp", meters=M.METER_TRUEPEAK, tune_segments=4)


@pytest.mark.parametrize("segs", [1, 3, 5, 7, 8, 13])
def test_segment_counts_and_neighbour_levels(M, segs):
    """Streams straddle 4-, 8- and 16-lane groups and waves; neighbouring streams differ by up to 2^60 in level, so a
    reference that leaked across streams would let a quiet stream's records pass."""
    T = 2400 * 26 + 311
    S = 13
    rows = []
    for s in range(S):
        lvl = 2.0 ** (30 if s % 3 == 0 else (-30 if s % 3 == 1 else 0))
        x = tri_noise(T, 60 + s, 1.0, period=7000 + 1000 * s) * np.float32(lvl)
        if s % 4 == 2:
            x += _sine(T, 11999 - 7 * s, 0.3 * lvl) * np.float32(np.linspace(0.1, 1.0, T, dtype=np.float32))[:, None]
        rows.append(x)
    x = np.stack(rows).astype(np.float32)
    _both(M, x, [T], "segments %d" % segs, tune_segments=segs)


def test_nan_inf_in_segments_of_one_stream(M):
    """Inf in one segment and NaN in another of the same stream (the reference becomes Inf; NaN chunks fail the check), and
    a channel that is NaN throughout."""
    T = 2400 * 24
    S = 6
    x = np.stack([tri_noise(T, 70 + s, 0.5, period=5000) for s in range(S)]).astype(np.float32)
    x[0, 3000, 0] = np.inf
    x[0, 40000, 0] = np.nan
    x[1, 50000, 1] = -np.inf
    x[1, 2000:2016, 1] = np.nan
    x[2, :, 0] = np.nan
    x[3, 30000, :] = np.inf
    x[3, 30001, :] = np.nan
    x[4, 100:200, 1] = np.nan
    _both(M, x, [T], "nan/inf", tune_segments=4)


def test_lengths_closing_segment_and_empty_stream(M):
    """Per-stream lengths: stream 0 closes 300 frames into its third segment; its loudest sample (1.0) lies 10 frames before
    its end, in a segment whose peak goes to k_kwtp16_len (the phase-0 delay leaves that sample uncounted), while its counted
    segments hold a rising sine whose inter-sample peaks decide the result: a reference fed from the closing segment would let
    them pass.  Stream 1 has length 0; stream 2 runs open; stream 3 closes at a segment boundary."""
    T = 2400 * 40
    seg = T // 4
    S = 4
    x = np.stack([tri_noise(T, 80 + s, 0.2, period=6000) for s in range(S)]).astype(np.float32)
    E0 = 2 * seg + 300
    x[0] = _sine(T, 11999, 0.5) * np.linspace(0.1, 1.0, T, dtype=np.float32)[:, None]
    x[0, E0 - 10, :] = 1.0
    x[0, E0:, :] = 7.0                                    # past the end: never read
    x[1, :, :] = 3.0
    lengths = [[E0, 0, T, 3 * seg]]
    a, b = _both(M, x, [T], "lengths", lengths=lengths, tune_segments=4)
    assert a["tp"][1, 0] == 0 and a["tp"][1, 1] == 0, a["tp"][1]


def test_44k1_truepeak_only_and_streaming(M):
    """44.1 kHz (tiles that end inside a step), the true peak alone, and streaming in arbitrary chunks with a loud first call
    and quiet later ones: no call's reference may reach the next call's truepeak_call."""
    fs = 44100.0
    T = 2205 * 24 + 777
    x = np.stack([tri_noise(T, 90 + s, 2.0 ** -(3 * (s % 5)), period=30000) for s in range(7)]).astype(np.float32)
    _both(M, x, [T], "44.1k", fs=fs, tune_segments=3)
    _both(M, x, [T], "44.1k tp", fs=fs, meters=M.METER_TRUEPEAK, tune_segments=5)
    for fs in (48000.0, 44100.0):
        T = int(fs) * 6 + 123
        frag = int(fs) // 20
        calls = [frag * 13 + 5, frag * 40 - 5, 333, frag * 20, T - (frag * 73 + 333)]
        x = np.stack([tri_noise(T, 95 + s, 0.8, period=20000) for s in range(5)]).astype(np.float32)
        x[:, :calls[0]] *= np.float32(2.0 ** 20)             # the first call loud, the rest 2^20 below it
        x[:, calls[0] + calls[1]:] *= np.float32(2.0 ** -10)
        a, _ = _both(M, x, calls, "chunks %g" % fs, fs=fs, tune_segments=3)
        assert (a["per_call"][1] < a["per_call"][0]).all(), a["per_call"]


def test_completion_share_on_the_bench_programme(M):
    """1024 streams x 10 s of the bench programme (synth kind 1) at the bench's own segmentation (8 per stream): at most
    7 % of the screened chunks complete (the screen without the stream reference completes 21.5 %)."""
    import torch
    S, T, fs = 1024, 480000, 48000.0
    buf = torch.empty((S, T, 2), dtype=torch.float32, device="cuda")
    M.synth_fill_device(buf.data_ptr(), S, T, T, 777, fs, 1, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    with M.Engine(S, fs, M.METER_EBU | M.METER_TRUEPEAK, tune_segments=8, tune_layout=7) as e:
        e.integr_start()
        e.process_device(buf.data_ptr(), T, T, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        scr, fin = e.refine_stats()
        assert e.seg_stats()[0] == 1
    del buf
    assert scr > 0
    assert fin <= 0.07 * scr, (scr, fin, fin / scr)
