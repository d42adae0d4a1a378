"""k_seg's screen with completed interpolated peaks in the stream's reference (MTR_SEG_SCREEN=2, the default), against the
screen without them (1) and the dense form (0), bit for bit.

Under rule 2 a step that completes chunks hands what they found to the owner lanes' pkf at once (mtr_seg.hip: peek_pm), and
from there it reaches the stream's reference R; under rule 1 R sees interpolated values only at a flush, so in effect it is
the stream's sample peak.  A reference that is too large — a neighbouring column's value, a value in the wrong scale, one of a
lane whose peak does not count, one of an earlier call — lets chunks pass that hold the stream's true peak, and the result is
too small; a peek that puts a foreign value into pkf makes it too large.  So every stream here carries an fs/4 sine at 45
degrees (samples at 0.707 of its amplitude, the true peak between them) that rises to the end under triangle-enveloped noise:
the stream's peak is an inter-sample value, found late, behind thousands of steps in which a wrong reference would have stood.

Held for every case: truepeak, truepeak_call and out9 of rules 2 and 1 are the dense form's bits, seg_stats are equal, rules
2 and 1 screen the same number of chunks, the dense form counts nothing, and rule 2 completes fewer chunks than rule 1 (both
printed; rule 2's counts are not pinned).  Two builds with one wrong line each fail this file on the peaks
(profiles/r28_kseg_ref_completed/test_mutant.txt): a peek whose owner reads the neighbouring column's exchange words, and an
offer to the reference without the peak_ok gate.

13 streams x (26 tiles + 311 frames), neighbouring streams at 2^30, 1 and 2^-30: with 3, 5 and 8 segments per stream the
streams straddle 16-lane rows and waves, and 13 x 5 = 65 units leave a wave with one live lane and 63 shadows."""
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
    """Rules 2 and 1 against the dense form (0)."""
    x = np.ascontiguousarray(x)
    calls = calls or [x.shape[1]]
    r2, r1, r0 = (_run(M, mode, x, calls, **kw) for mode in (2, 1, 0))
    print(tag, "seg", r2["seg"], "screened, completed: rule 2", r2["refine"], "rule 1", r1["refine"], "dense", r0["refine"])
    assert r2["seg"][0] > 0, (tag, "k_seg did not run", r2["seg"])
    assert r2["seg"] == r0["seg"] and r1["seg"] == r0["seg"], tag
    for name, r in (("rule 2", r2), ("rule 1", r1)):
        assert _bits_equal(r["tp"], r0["tp"]), (tag, name, r["tp"], r0["tp"])
        assert _bits_equal(r["per_call"], r0["per_call"]), (tag, name, r["per_call"], r0["per_call"])
        if r0["o9"] is not None:
            assert _bits_equal(r["o9"], r0["o9"]), (tag, name)
    assert r2["refine"][0] == r1["refine"][0] > 0, (tag, "the rules screen the same chunks", r2["refine"], r1["refine"])
    assert r0["refine"] == (0, 0), (tag, "the dense form counts nothing", r0["refine"])
    assert r2["refine"][1] < r1["refine"][1], (tag, "rule 2 completes no fewer chunks than rule 1", r2["refine"], r1["refine"])
    return r2, r0


def _sine45(T, lo=0.3, hi=1.0):
    """fs/4 at 45 degrees, amplitude lo .. hi over T: samples at 0.707 of the amplitude, the peak half-way between them;
    the channels in opposite phase of the ramp's fine structure (the right one 3 % lower)."""
    n = np.arange(T)
    s = np.sin(0.5 * np.pi * n + 0.25 * np.pi) * np.linspace(lo, hi, T)
    return np.stack([s, -0.97 * s], 1).astype(np.float32)


_cache = {}


def _programme(T, fs=48000.0):
    """Never modified by a test (tests that need a variant copy it)."""
    key = (T, fs)
    if key not in _cache:
        rows = []
        for s in range(S):
            lvl = np.float32(2.0 ** (30, 0, -30)[s % 3])
            x = tri_noise(T, 400 + s, 0.1, period=7000 + 1000 * s) + _sine45(T, 0.3 + 0.01 * s, 1.0 + 0.02 * s)
            rows.append((x * lvl).astype(np.float32))
        x = np.stack(rows)
        x.setflags(write=False)
        _cache[key] = x
    return _cache[key]


def _inter_sample(r, x, streams):
    """the streams' peaks lie between the samples (what makes a wrong reference move a peak)"""
    for s in streams:
        assert (r["tp"][s] > 1.05 * np.abs(x[s]).max(0)).all(), (s, r["tp"][s], np.abs(x[s]).max(0))


@pytest.mark.parametrize("segs", [1, 3, 5, 8])
def test_inter_sample_peaks_and_neighbour_levels(M, segs):
    """The programme at 1, 3, 5 and 8 segments per stream (13, 39, 65 and 104 lanes)."""
    x = _programme(T48)
    r2, _ = _all(M, x, "segments %d" % segs, tune_segments=segs)
    _inter_sample(r2, x, range(S))


def test_truepeak_only(M):
    x = _programme(T48)
    r2, _ = _all(M, x, "tp", meters=M.METER_TRUEPEAK, tune_segments=5)
    _inter_sample(r2, x, range(S))


@pytest.mark.parametrize("up", [True, False])
def test_level_jump_of_2_13_inside_a_segment(M, up):
    """Streams 1, 6 and 11 change level by 2^13 and 2^20 inside a segment, behind hundreds of completions.  Up: the column is
    rescaled, pm leaves through flush_pm in the old scale, and the final peak is an inter-sample value in the new one (a peek
    with a stale un, or one that found a stale exchange word, would be off by the ratio).  Down (loud first, quiet after): the
    peak stays the loud part's inter-sample value, in the scale the column keeps."""
    x = _programme(T48).copy()
    for s, at, k in ((1, T48 * 5 // 8, 13), (6, T48 // 3 + 7, 20), (11, T48 - 5000, 13)):
        if up:
            x[s, :at] *= np.float32(2.0 ** -k)
        else:
            x[s, at:] *= np.float32(2.0 ** -k)
    r2, _ = _all(M, x, "jump %s" % ("up" if up else "down"), tune_segments=5)
    _inter_sample(r2, x, (1, 6, 11))


def test_truepeak_only_jump_of_2_200(M):
    """The true peak alone; stream 6 jumps by 2^100 x 2^100 inside a segment and its peak is an inter-sample value behind the
    jump."""
    x = _programme(T48).copy()
    at = T48 * 5 // 8
    x[6] = x[7]                                            # (level 1)
    x[6, :at] *= np.float32(2.0 ** -100)
    x[6, at:] *= np.float32(2.0 ** 100)
    r2, _ = _all(M, x, "jump 2^200, tp", meters=M.METER_TRUEPEAK, tune_segments=5)
    assert r2["tp"][6].max() > 2.0 ** 99, r2["tp"][6]
    _inter_sample(r2, x, (6,))


def test_lengths_close_streams_inside_a_segment(M):
    """Per-stream lengths.  Stream 2 closes 300 frames into its third segment and stream 8 3000 frames before the end, each with
    its loudest samples (twice the amplitude the stream ever reaches) 10 .. 7 frames before its end: the phase-0 delay leaves
    them uncounted, the closing segment's lane (!peak_ok) holds them in pk0 and, once a neighbouring column has completed a
    chunk, what the truncated windows make of them in pm and — peeked — in pkf.  None of it may reach the reference: the
    closing segment itself runs at half the level (its peak, which another kernel takes, does not decide), so the counted
    peak is an inter-sample value at the end of the segment in front of it, hundreds of steps later in the launch than the
    loud samples.  Stream 4 is empty and stream 7 closes on a segment boundary."""
    x = _programme(T48).copy()
    lengths = [T48] * S
    lengths[2] = 2400 * 11 + 300
    lengths[8] = T48 - 3000
    lengths[4] = 0
    lengths[7] = 2400 * 16
    for s, tile in ((2, 11), (8, 21)):                     # (26 tiles in 5 segments: 6, 5, 5, 5, 5)
        E = lengths[s]
        lvl = np.float32(2.0 ** (30, 0, -30)[s % 3])
        x[s, 2400 * tile:] *= np.float32(0.5)
        x[s, E - 10:E - 6, :] = (np.array([[2.6, -2.6], [-2.6, 2.6], [2.6, -2.6], [-2.6, 2.6]], np.float32) * lvl)
    x[2, lengths[2]:] = 7.0                                # past the end: never read
    r2, _ = _all(M, x, "lengths", lengths=lengths, tune_segments=5)
    assert r2["tp"][4, 0] == 0 and r2["tp"][4, 1] == 0, r2["tp"][4]
    for s in (2, 8):                                       # the loud samples are not counted, and the peak lies between samples
        lvl = 2.0 ** (30, 0, -30)[s % 3]
        assert (r2["tp"][s] < 2.0 * lvl).all(), (s, r2["tp"][s])
        assert (r2["tp"][s] > 1.05 * np.abs(x[s, :lengths[s] - 24]).max(0)).all(), (s, r2["tp"][s])


def test_nan_and_inf_in_one_stream_of_a_row(M):
    """Inf and NaN samples in streams 3 and 4, next to streams that stay finite."""
    x = _programme(T48).copy()
    x[3, 30000, 0] = np.inf
    x[3, 9000, 1] = np.nan
    x[3, 9100:9116, 1] = np.nan
    x[4, :, 0] = np.nan
    x[4, 50000, 1] = -np.inf
    r2, _ = _all(M, x, "nan/inf", tune_segments=5)
    _inter_sample(r2, x, (0, 1, 2, 5, 6))


def test_44k1(M):
    """44.1 kHz: tiles end inside a step."""
    T = 2205 * 26 + 311
    x = _programme(T, fs=44100.0)
    r2, _ = _all(M, x, "44.1k", fs=44100.0, tune_segments=5)
    _inter_sample(r2, x, range(S))


def test_two_calls_loud_then_quiet(M):
    """Two calls on one engine, the first 2^10 above the second: pkf, pm and the reference start every call from zero, so the
    second call's truepeak_call is the dense one (an inter-sample value 2^10 below the first call's; the first call's last
    100 frames are at the second one's level, as the second call counts the last 24 of them)."""
    x = np.concatenate([_programme(T48) * np.float32(2.0 ** 10), _programme(T48)], 1)
    x[:, T48 - 100:T48] *= np.float32(2.0 ** -10)          # (the second call counts the first one's last 24 frames: quiet too)
    r2, _ = _all(M, x, "two calls", calls=[T48, T48], tune_segments=5)
    assert (r2["per_call"][1] * 512 < r2["per_call"][0]).all(), r2["per_call"]
    assert (r2["per_call"][1] > 1.05 * np.abs(x[:, T48:]).max(1)).all(), r2["per_call"]
