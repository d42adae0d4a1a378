"""k_seg's screen on inputs that move its vote bounds in every way, against the dense form bit for bit.

The screened form (the default) votes on each chunk with eps and R' of the chunk's column, which the column's owner lane
computes every step and hands to the accumulator lanes through LDS (mtr_seg.hip: SCREEN, the stream reference).  That
exchange is ordered by the LDS queue alone, without fences.  MTR_SEG_SCREEN=0, read at engine creation, forces the dense
form.  Held here: the peaks and loudness outputs are the dense form's bits, and the chunks screened and completed
(refine_stats) are, to the last digit, what the library of the commit before this file counted on the same inputs, when
fences still drained the LDS queue around the exchange (COUNTS below).  A bound that arrives a step late or from another
column (a stale, too small eps passes chunks that must complete; a stale R' after a rescale is off by the scale's ratio; a
loud neighbour's R' lets a quiet stream's chunks pass) need not move a peak, but it moves the counts.  A build with the
exchange's reads in front of its writes (every vote with the bounds of the step before) fails every case of this file on the
counts alone (its peaks are the dense ones), and one with the reads taken from the neighbouring column fails every case on
the peaks (profiles/r16_kseg_bounds/test_mutant.txt).  The inputs:

  * a staircase level under every stream's noise: x 1.5 at frames 0, 16, 32 and 48 mod 64, so the running maximum and the
    reference change in steps of every residue mod 4, with a constant level behind the last rise (one case holds the
    level for two seconds);
  * a slowly ramped 11 999 Hz sine in every third stream: its inter-sample records grow by less than the lo products add;
  * neighbouring streams at 2^30, 1 and 2^-30;
  * a jump of 2^100 x 2^100 inside a segment (the true peak alone), which rescales;
  * per-stream lengths that close a stream inside a segment (the -inf bounds of the columns whose peak does not count).

13 streams x (26 tiles + 311 frames) with 1, 5 and 8 segments per stream: streams straddle 16-lane rows and waves."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from make_golden import tri_noise  # noqa: E402

S = 13

# (chunks screened, chunks completed) per case: counted by the fenced exchange of the commit before this file.  They are a
# property of the inputs and of the screen's rule (mtr_seg.hip: SCREEN), not of how the bounds travel.
COUNTS = {
    "segments 1": (31200, 8698), "segments 5": (14400, 3747), "segments 8": (12000, 3076), "hold": (33600, 3509),
    "44.1k": (13232, 3477), "jump, tp": (14400, 3482), "lengths": (14400, 3957),
}


@pytest.fixture(scope="module")
def M():
    import meters.lv2_amd as m
    return m


def _engine(M, mode, *a, **kw):
    old = os.environ.get("MTR_SEG_SCREEN")
    os.environ["MTR_SEG_SCREEN"] = str(mode)
    try:
        return M.Engine(*a, **kw)
    finally:
        if old is None:
            del os.environ["MTR_SEG_SCREEN"]
        else:
            os.environ["MTR_SEG_SCREEN"] = old


def _run(M, mode, x, fs=48000.0, meters=None, lengths=None, **kw):
    meters = meters if meters is not None else (M.METER_EBU | M.METER_TRUEPEAK)
    with _engine(M, mode, x.shape[0], fs, meters, tune_layout=7, **kw) as e:
        if meters & M.METER_EBU:
            e.integr_start()
        if lengths is None:
            e.process(x)
        else:
            e.process_lengths(x, np.asarray(lengths, np.uint64))
        per_call = np.array([[r.truepeak_call[0], r.truepeak_call[1]] for r in e.results()], np.float32)
        return dict(tp=e.truepeak(), per_call=per_call, o9=e.out9() if meters & M.METER_EBU else None,
                    seg=e.seg_stats(), refine=e.refine_stats())


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def _both(M, x, tag, **kw):
    """The screened form (1) and the dense form (0)."""
    x = np.ascontiguousarray(x)
    r1, r0 = (_run(M, mode, x, **kw) for mode in (1, 0))
    print(tag, "seg", r1["seg"], "refine: screened", r1["refine"], "dense", r0["refine"])
    assert r1["seg"][0] > 0, (tag, "k_seg did not run", r1["seg"])
    assert r1["seg"] == r0["seg"], tag
    assert _bits_equal(r1["tp"], r0["tp"]), (tag, r1["tp"], r0["tp"])
    assert _bits_equal(r1["per_call"], r0["per_call"]), (tag, r1["per_call"], r0["per_call"])
    if r1["o9"] is not None:
        assert _bits_equal(r1["o9"], r0["o9"]), tag
    assert tuple(r1["refine"]) == COUNTS[tag], (tag, "votes differ from the fenced exchange's", r1["refine"], COUNTS[tag])
    assert r0["refine"] == (0, 0), (tag, "the dense form counts nothing", r0["refine"])
    return r1


def _staircase(T, s, rise_until):
    """x 1.5 about every 2900 frames up to frame rise_until, at frames 0, 16, 32, 48 mod 64 in turn; 1 behind the last rise."""
    at = [64 * (45 * i + 3 * s + 5) + 16 * ((i + s) % 4) for i in range(64)]
    at = [f for f in at if f < rise_until]
    g = np.ones(T, np.float32)
    for f in at:
        g[:f] *= np.float32(1.0 / 1.5)
    return g


def _sine(T, f, fs):
    t = np.arange(T) / fs
    return np.stack([np.sin(2 * np.pi * f * t + 0.3), np.sin(2 * np.pi * f * t + 1.1)], 1)


_cache = {}


def _programme(T, fs=48000.0, rise_until=None):
    """Never modified by a test (tests that need a variant copy it)."""
    key = (T, fs, rise_until)
    if key not in _cache:
        rows = []
        for s in range(S):
            lvl = np.float32(2.0 ** (30, 0, -30)[s % 3])
            x = tri_noise(T, 200 + s, 1.0, period=7000 + 1000 * s) * _staircase(T, s, rise_until or T)[:, None]
            if s % 3 == 2:
                x = x + (_sine(T, 11999 - 7 * s, fs) * (0.3 * np.linspace(0.1, 1.0, T))[:, None]).astype(np.float32)
            rows.append((x * lvl).astype(np.float32))
        x = np.stack(rows)
        x.setflags(write=False)
        _cache[key] = x
    return _cache[key]


T48 = 2400 * 26 + 311


@pytest.mark.parametrize("segs", [1, 5, 8])
def test_staircase_ramp_and_neighbour_levels(M, segs):
    """The programme above at 1, 5 and 8 segments per stream (13, 65 and 104 lanes: rows and waves are straddled)."""
    _both(M, _programme(T48), "segments %d" % segs, tune_segments=segs)


def test_level_held_for_two_seconds(M):
    """The staircases rise during the first 1.3 s and the level then stands for 2 s: thousands of steps whose bounds do not
    move."""
    T = T48 + 96000
    _both(M, _programme(T, rise_until=T48), "hold", tune_segments=5)


def test_44k1(M):
    """44.1 kHz: tiles end inside a step."""
    T = 2205 * 26 + 311
    _both(M, _programme(T, fs=44100.0), "44.1k", fs=44100.0, tune_segments=5)


def test_truepeak_only_with_a_level_jump(M):
    """The true peak alone; one stream jumps by 2^100 x 2^100 inside a segment, which rescales its column: the step behind
    the jump must vote with bounds in the new scale."""
    x = _programme(T48).copy()
    jump = tri_noise(T48, 231, 1.0, period=9000) * np.float32(2.0 ** -100)
    jump[T48 * 5 // 8:] *= np.float32(2.0 ** 100)
    jump[T48 * 5 // 8:] *= np.float32(2.0 ** 100)
    x[6] = jump
    r = _both(M, x, "jump, tp", meters=M.METER_TRUEPEAK, tune_segments=5)
    assert r["tp"][6].max() > 2.0 ** 90, r["tp"][6]


def test_lengths_close_streams_inside_a_segment(M):
    """Per-stream lengths: stream 2 (a ramped sine) closes 300 frames into its third segment, stream 8 (another) 1000 frames
    before the end, stream 4 is empty and stream 7 closes on a segment boundary: the closing segments' columns carry -inf
    bounds next to live ones."""
    x = _programme(T48).copy()
    lengths = [T48] * S
    lengths[2] = 2400 * 11 + 300
    lengths[8] = T48 - 1000
    lengths[4] = 0
    lengths[7] = 2400 * 16
    x[2, lengths[2]:] = 7.0                                # past the end: never read
    r = _both(M, x, "lengths", lengths=lengths, tune_segments=5)
    assert r["tp"][4, 0] == 0 and r["tp"][4, 1] == 0, r["tp"][4]
