"""k_seg's lazy form (MTR_SEG_SCREEN=3): the screened step without the lo halves of the f16 split, which a completing chunk builds
on the spot from the stream's f32 samples (mtr_seg.hip: LAZY, lazy_lo), against form 2 (the lo words of every step in the ring)
and the dense form (0), bit for bit.

A lo word built late is the ring's word only if it is made from the very samples the ring was filled from — the previous
segment's, the call's history, the zeros in front of a first call, the zeros behind a last segment's cut step — under the scale
its step was split in, with every rescale since replayed.  A wrong word is off by about 2^-11 of its sample, which moves an
interpolated peak by many f32 ulps but no sample peak: so every stream here carries an fs/4 sine at 45 degrees (the true peak lies
between two equal samples) and the cases put a stream's record — one equal adjacent pair well above the rest — exactly where the
window of its chunk reaches into one of those places.

Held for every case: truepeak, truepeak_call and out9 of forms 3 and 2 are the dense form's bits, seg_stats are equal, form 3
screens and completes exactly the chunks form 2 does (refine_stats equal to the last digit, completions > 0), and the dense form
counts nothing.  Calls with per-stream ends (process_lengths) stay on form 2 under MTR_SEG_SCREEN=3 — the LEN instantiations have no
lazy form — which the last test holds through the same comparison.

13 streams x (26 tiles + 311 frames), neighbouring streams at 2^30, 1 and 2^-30: with 3, 5 and 8 segments per stream the streams
straddle 16-lane rows and waves, and 13 x 5 = 65 units leave a wave with one live lane and 63 shadows.
profiles/r29_kseg_lazy_lo/test_mutant.txt: what this file does with builds that have one wrong line each.  A materialiser that reads
the buffer for the history fails it; one that splits every window slot under the current scale does NOT (the split commutes with a
power-of-two scale outside the f16 subnormals, so its words differ by a subnormal quantum at most: the file says why case 2 cannot
see that on the peaks)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from make_golden import tri_noise  # noqa: E402

S = 13
T48 = 2400 * 26 + 311
SEG5 = (0, 6, 11, 16, 21, 26)                              # first tiles of 26 tiles in 5 segments (6, 5, 5, 5, 5)


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


def _run(M, mode, x, calls, fs=48000.0, meters=None, lengths=None, **kw):
    """calls: frames per call; lengths (optional): frames of each stream in the (one) call (process_lengths)."""
    meters = meters if meters is not None else (M.METER_EBU | M.METER_TRUEPEAK)
    with _engine(M, mode, x.shape[0], fs, meters, tune_layout=7, **kw) as e:
        if meters & M.METER_EBU:
            e.integr_start()
        pos, per_call = 0, []
        for n in calls:
            blk = np.ascontiguousarray(x[:, pos:pos + n])
            if lengths is None:
                e.process(blk)
            else:
                e.process_lengths(blk, np.asarray(lengths, np.uint64))
            per_call.append(np.array([[r.truepeak_call[0], r.truepeak_call[1]] for r in e.results()], np.float32))
            pos += n
        return dict(tp=e.truepeak(), per_call=np.stack(per_call), o9=e.out9() if meters & M.METER_EBU else None,
                    seg=e.seg_stats(), refine=e.refine_stats())


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def _all(M, x, tag, calls=None, **kw):
    """Forms 3 and 2 against the dense form (0)."""
    x = np.ascontiguousarray(x)
    calls = calls or [x.shape[1]]
    r3, r2, r0 = (_run(M, mode, x, calls, **kw) for mode in (3, 2, 0))
    print(tag, "seg", r3["seg"], "screened, completed: form 3", r3["refine"], "form 2", r2["refine"], "dense", r0["refine"])
    assert r3["seg"][0] > 0, (tag, "k_seg did not run", r3["seg"])
    assert r3["seg"] == r0["seg"] and r2["seg"] == r0["seg"], tag
    for name, r in (("form 3", r3), ("form 2", r2)):
        assert _bits_equal(r["tp"], r0["tp"]), (tag, name, r["tp"], r0["tp"])
        assert _bits_equal(r["per_call"], r0["per_call"]), (tag, name, r["per_call"], r0["per_call"])
        if r0["o9"] is not None:
            assert _bits_equal(r["o9"], r0["o9"]), (tag, name)
    assert r3["refine"] == r2["refine"], (tag, "form 3 screens and completes the chunks form 2 does", r3["refine"], r2["refine"])
    assert r3["refine"][0] > 0 and r3["refine"][1] > 0, (tag, r3["refine"])
    assert r0["refine"] == (0, 0), (tag, "the dense form counts nothing", r0["refine"])
    return r3, r0


def _sine45(T, lo=0.3, hi=1.0):
    """fs/4 at 45 degrees, amplitude lo .. hi over T: samples at 0.707 of the amplitude, the peak half-way between them;
    the channels in opposite phase of the ramp's fine structure (the right one 3 % lower)."""
    n = np.arange(T)
    s = np.sin(0.5 * np.pi * n + 0.25 * np.pi) * np.linspace(lo, hi, T)
    return np.stack([s, -0.97 * s], 1).astype(np.float32)


_cache = {}


def _level(s):
    return np.float32(2.0 ** (30, 0, -30)[s % 3])


def _programme(T):
    """Never modified by a test (tests that need a variant copy it)."""
    if T not in _cache:
        rows = []
        for s in range(S):
            x = tri_noise(T, 400 + s, 0.1, period=7000 + 1000 * s) + _sine45(T, 0.3 + 0.01 * s, 1.0 + 0.02 * s)
            rows.append((x * _level(s)).astype(np.float32))
        x = np.stack(rows)
        x.setflags(write=False)
        _cache[T] = x
    return _cache[T]


def _record(x, s, m, lvl=None, amp=3.0):
    """The stream's record: an equal adjacent pair at frames m, m + 1, the channels in opposite sign, well above whatever else the
    stream holds (the programme stays under 1.5): its true peak lies between the two samples and is found by the chunk that holds
    output frame m + 24."""
    lvl = _level(s) if lvl is None else np.float32(lvl)
    x[s, m:m + 2, 0] = np.float32(amp) * lvl
    x[s, m:m + 2, 1] = np.float32(-0.97 * amp) * lvl


def _inter_sample(r, x, streams, key="tp", frames=slice(None)):
    """the streams' peaks lie between the samples (what makes a wrong lo word move a peak)"""
    for s in streams:
        assert (r[key][s] > 1.05 * np.abs(x[s, frames]).max(0)).all(), (s, r[key][s], np.abs(x[s, frames]).max(0))


@pytest.mark.parametrize("segs", [1, 3, 5, 8])
def test_inter_sample_peaks_and_neighbour_levels(M, segs):
    """Case 1.  The programme at 1, 3, 5 and 8 segments per stream (13, 39, 65 and 104 lanes)."""
    x = _programme(T48)
    r3, _ = _all(M, x, "segments %d" % segs, tune_segments=segs)
    _inter_sample(r3, x, range(S))


def test_truepeak_only(M):
    """Case 1, the true peak alone (the instantiations without the recurrence)."""
    x = _programme(T48)
    r3, _ = _all(M, x, "tp", meters=M.METER_TRUEPEAK, tune_segments=5)
    _inter_sample(r3, x, range(S))


@pytest.mark.parametrize("k1", [40, 26])
def test_rescales_inside_a_live_window(M, k1):
    """Case 2.  Every stream jumps by 2^k1 (the f16 ratio of the rescale rounds to 0: >= 2^25) on frame 8 of a step and by 2^13 again
    20 frames later, on frame 12 of the next step: two rescales within one 64-sample window.  The stream's record is a pair r = s mod 4
    steps behind the second jump (r = 0: the pair is the jump, in the very step of the rescale); its chunk, 24 frames later, has a
    window that holds words split under three scales (r = 0: the 48 taps reach 3 frames in front of the first jump), two (r = 1) or one
    with rescaled words under zero taps (r = 2, 3).  The frames between the jumps carry a pair of their own, 2^13 below the record."""
    x = _programme(T48).copy()
    for s in range(S):
        at = 2400 * 2 + 16 * (97 * s) + 8                      # (spread over the segments' interiors)
        j2 = at + 20
        x[s, :at] *= np.float32(2.0 ** -(k1 + 13))
        x[s, at:j2] *= np.float32(2.0 ** -13)
        _record(x, s, at + 8, lvl=_level(s) * np.float32(2.0 ** -13))
        _record(x, s, j2 + 16 * (s % 4))
    r3, _ = _all(M, x, "two rescales, 2^%d" % k1, tune_segments=5)
    _inter_sample(r3, x, range(S))


def test_records_in_the_first_steps_of_a_segment(M):
    """Case 3, segments.  Each stream's record is found in step 0, 1 or 2 of one of its segments 1 .. 4 (output frames 4, 20 and 36 of
    the segment: the pair lies 20 or 4 frames in front of the segment or 12 behind its start), where the chunk's window reaches 44,
    28 and 12 frames into the previous segment — samples the lane never loaded in its main loop."""
    x = _programme(T48).copy()
    for s in range(S):
        start = 2400 * SEG5[1 + s % 4]
        _record(x, s, start + (-20, -4, 12)[(s // 4) % 3])
    r3, _ = _all(M, x, "segment starts", tune_segments=5)
    _inter_sample(r3, x, range(S))


def test_records_in_the_first_steps_of_a_call(M):
    """Case 3, calls.  Two calls, neither a whole number of tiles: the first ends 5 frames short of a tile, so the second call's
    launch starts 5 frames into it and the windows of its first steps hold those 5 frames and the history (a.hist: the first call's
    last 47 frames).  The second call's record of stream s is found in step 0, 1 or 2 of its launch (the pair 15 frames in front of
    the call, inside the history; on its frame 1, in front of the launch; on its frame 17).  The first call's record sits on its
    frames 0 or 12 (steps 1 and 2): the windows reach into the zeros in front of a first call."""
    n1 = 2400 * 9 + 2395
    x = _programme(T48).copy()
    for s in range(S):
        _record(x, s, (0, 12)[s % 2])
        _record(x, s, n1 + 5 + (-20, -4, 12)[s % 3], amp=2.0)
    r3, _ = _all(M, x, "call starts", calls=[n1, T48 - n1], tune_segments=5)
    assert (r3["per_call"][0] > 1.05 * np.abs(x[:, :n1]).max(1)).all(), r3["per_call"][0]
    assert (r3["per_call"][1] > 1.05 * np.abs(x[:, n1:]).max(1)).all(), r3["per_call"][1]


def test_44k1_records_in_the_last_steps_of_a_launch(M):
    """Case 4.  44.1 kHz: a lane's last tile ends 14 frames into the launch's last step (6 x 2205 = 826 x 16 + 14), which runs dense,
    its rows behind the tile's end masked and — in a stream's last segment — its frames behind the end read as zeros.  Each stream's
    record is found in that step (output frame end - 6) or in the step before it (end - 22), at the end of segment s mod 5: the
    last segment of streams 4 and 9."""
    T = 2205 * 26 + 311
    x = _programme(T).copy()
    for s in range(S):
        end = 2205 * SEG5[1 + s % 5]
        _record(x, s, end - 24 - (6, 22)[(s // 5) % 2])
    r3, _ = _all(M, x, "44.1k", fs=44100.0, tune_segments=5)
    _inter_sample(r3, x, range(S))


def test_one_inf_and_one_nan_sample(M):
    """Case 5.  Stream 3 holds one Inf sample and stream 4 one NaN sample, each in both channels' windows of completing chunks (the
    streams' records follow 20 frames behind them); their neighbours are unaffected."""
    x = _programme(T48).copy()
    x[3, 30000, 0] = np.inf
    x[4, 41000, 1] = np.nan
    _record(x, 3, 30020)
    _record(x, 4, 41020)
    _record(x, 2, 30020)
    _record(x, 5, 41020)
    r3, _ = _all(M, x, "inf / nan", tune_segments=5)
    _inter_sample(r3, x, (0, 1, 2, 5, 6, 7))
    assert np.isinf(r3["tp"][3, 0]) and np.isfinite(r3["tp"][3, 1]) and np.isfinite(r3["tp"][4]).all(), (r3["tp"][3], r3["tp"][4])


def test_lengths_stay_on_form_2(M):
    """Case 6.  process_lengths with ends inside a window (stream 2 closes 300 frames into its third segment, 4 frames behind a
    step's start; stream 8 3000 frames before the end; stream 4 is empty; stream 7 closes on a segment boundary).  The kernels that
    take per-stream ends have no lazy form: under MTR_SEG_SCREEN=3 such a call runs form 2, so its counts are form 2's to the last
    digit and its results the dense bits."""
    x = _programme(T48).copy()
    lengths = [T48] * S
    lengths[2] = 2400 * 11 + 300
    lengths[8] = T48 - 3000
    lengths[4] = 0
    lengths[7] = 2400 * 16
    for s in (2, 8):
        _record(x, s, lengths[s] - 24 - 40)
    x[2, lengths[2]:] = 7.0                                # past the end: never read
    r3, _ = _all(M, x, "lengths", lengths=lengths, tune_segments=5)
    assert r3["tp"][4, 0] == 0 and r3["tp"][4, 1] == 0, r3["tp"][4]
