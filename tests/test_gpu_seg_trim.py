"""k_seg's screened step on inputs that reach every slot of its vote and every way through its completions, against the
dense form bit for bit.

The screened form (the default) votes on each chunk's first product: the maximum of the twelve values a lane holds (rows
4 kg .. 4 kg + 3 of three phases) plus the column's bound against the column's records (mtr_seg.hip: SCREEN); the failing
chunks of a step complete behind its one branch.  MTR_SEG_SCREEN=0, read at engine creation, forces the dense form.  Held
here: the peaks, the per-call peaks and the loudness outputs are the dense form's bits, and the chunks screened and
completed (refine_stats) are, to the last digit, what the library of the commit before this file counted on the same
inputs (COUNTS below).  The counts are a property of the inputs and of the screen's rule, not of how many instructions the
step takes for it: a vote that loses one of its twelve values, or takes another chunk's records, need not move a peak, but
it moves the counts (profiles/r23_kseg_trim/test_mutant.txt).  The inputs:

  * quiet noise with one band-limited burst per stream, whose largest interpolated value lies 1/4, 2/4 or 3/4 of a frame
    behind a frame of every residue mod 16, in the left channel, the right channel or both: over the six cases every (row,
    phase) of a step's outputs holds a stream's record, with each channel choice for every row;
  * carriers whose level rises by 3 % every 16 frames for 40 steps, in every stream and every segment at the same step: all
    eight chunks of a step fail, forty steps running; and the same rise in the left channel of one stream and the right
    channel of another alone, whose columns lie in block 0 and block 3: chunks 0 and 7 complete, the six between them do not;
  * one NaN, or one Inf, in one frame of the one column that rises, so that its votes alone decide its chunk;
  * 44.1 kHz (tiles that end inside a step) and the true peak alone; a call that ends 7 frames behind its last tile, so
    that the launch's last two steps count phase 0 frame by frame, with the call's largest sample among those frames;
  * per-stream lengths that close a stream inside a segment and inside a rise.

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
TILES = 26

# (chunks screened, chunks completed) per case: counted by the library of the commit before this file, on these inputs.
COUNTS = {
    "records 1/0": (31200, 412), "records 1/1": (31200, 409), "records 5/0": (14400, 1743), "records 5/1": (14400, 1818),
    "records 8/0": (12000, 1441), "records 8/1": (12000, 1828),
    "rising 1": (31200, 1634), "rising 5": (14400, 1663), "rising 8": (12000, 2832), "chunks 0 and 7": (14400, 1598),
    "none": (14400, 1639), "nan": (14400, 1638), "inf": (14400, 2113),
    "44.1k": (13232, 1559), "44.1k tp": (13232, 1559), "tp": (14400, 1663),
    "last steps 48000": (14400, 1663), "last steps 44100": (13232, 1559), "lengths": (14400, 1449),
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
    assert tuple(r1["refine"]) == COUNTS[tag], (tag, "votes differ from the parent's", r1["refine"], COUNTS[tag])
    assert r0["refine"] == (0, 0), (tag, "the dense form counts nothing", r0["refine"])
    return r1


def _frames(fs=48000.0, extra=311):
    return int(fs) // 20 * TILES + extra


# ---- the record in every accumulator position -------------------------------------------------------------------------

def _burst(T, t0, amp):
    """A Hann-windowed sinc (cut-off 0.4 fs) centred on the fractional frame t0: its interpolated maximum lies at t0."""
    n = np.arange(T, dtype=np.float64) - t0
    w = np.where(np.abs(n) < 40.0, 0.5 + 0.5 * np.cos(np.pi * n / 40.0), 0.0)
    return (amp * np.sinc(0.8 * n) * w).astype(np.float32)


def _records(ci, variant):
    """Stream s of case (ci, variant) is combination i = 39 variant + 13 ci + s of 78: row i % 16, phase (i // 16) % 3 and
    channels (i + i // 48) % 3 — the first 48 are every (row, phase) once, and every row with each channel choice."""
    T = _frames()
    tile = 2400
    rows = []
    for s in range(S):
        i = 39 * variant + 13 * ci + s
        row, phase, chan = i % 16, (i // 16) % 3, (i + i // 48) % 3
        x = tri_noise(T, 500 + i, 2.0 ** -9, period=9000 + 500 * s).copy()
        t0 = tile * (3 + (7 * i) % 20) + 800 + row + (phase + 1) / 4.0
        b = _burst(T, t0, 0.25 + 0.01 * s)
        if chan in (0, 2):
            x[:, 0] += b
        if chan in (1, 2):
            x[:, 1] += b * np.float32(0.75 if chan == 2 else 1.0)
        rows.append(x)
    return np.stack(rows)


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("ci,segs", [(0, 1), (1, 5), (2, 8)])
def test_record_in_every_row_and_phase(M, ci, segs, variant):
    _both(M, _records(ci, variant), "records %d/%d" % (segs, variant), tune_segments=segs)


# ---- many completions in one step, and in consecutive steps -------------------------------------------------------------

RISE_TILES = (2, 7, 12, 17, 22)          # with five segments per stream (6 + 5 + 5 + 5 + 5 tiles, every lane 6 tiles long):
RISE_AT = 400                            # the same step of every lane


def _envelope(T, tile):
    """Zero but in the rises: 1.03 x every 16 frames for 40 steps from frame RISE_AT of the tiles RISE_TILES, each rise
    from where the one before stopped — every step of every rise sets its stream's record."""
    g = np.zeros(T, np.float64)
    level = 1.0
    for k in RISE_TILES:
        f0 = tile * k + RISE_AT
        for st in range(40):
            level *= 1.03
            g[f0 + 16 * st:f0 + 16 * st + 16] = level
    return g


_cache = {}


def _rising(fs=48000.0, extra=311, only=None):
    """Two sines per stream (3 kHz and up: several crests per step) under the envelope, over quiet noise.  `only`:
    {stream: channel} — the sines there alone, noise everywhere else.  Never modified by a test (they copy it)."""
    key = (fs, extra, None if only is None else tuple(sorted(only.items())))
    if key not in _cache:
        T = _frames(fs, extra)
        tile = int(fs) // 20
        t = np.arange(T) / fs
        env = _envelope(T, tile)
        rows = []
        for s in range(S):
            f = 3000.0 + 137.0 * s
            c = np.stack([np.sin(2 * np.pi * f * t + 0.3 * s), np.sin(2 * np.pi * (f + 411.0) * t + 1.1 + 0.2 * s)], 1)
            g = np.zeros((T, 2))
            if only is None:
                g[:] = env[:, None]
            elif s in only:
                g[:, only[s]] = env
            x = (0.02 * c * g).astype(np.float32) + tri_noise(T, 700 + s, 2.0 ** -12, period=8000 + 300 * s)
            rows.append(x.astype(np.float32))
        x = np.stack(rows)
        x.setflags(write=False)
        _cache[key] = x
    return _cache[key]


@pytest.mark.parametrize("segs", [1, 5, 8])
def test_every_chunk_completes_forty_steps_running(M, segs):
    r = _both(M, _rising(), "rising %d" % segs, tune_segments=segs)
    assert r["refine"][1] >= 8 * 40, r["refine"]


def test_chunks_0_and_7_alone(M):
    """Five segments per stream: stream 1 is columns 5..9 (block 0), stream 11 columns 55..59 (block 3)."""
    _both(M, _rising(only={1: 0, 11: 1}), "chunks 0 and 7", tune_segments=5)


@pytest.mark.parametrize("what", ["none", "nan", "inf"])
def test_one_nan_or_inf_inside_a_rise(M, what):
    """One column rises alone: the right channel of stream 11 in its third segment, noise everywhere else, so chunk 7
    completes on that column's votes.  With a NaN in one frame of the rise, the steps whose windows hold it vote on first
    products that are NaN in every row — a lane whose twelve values are all NaN votes with +0, as the dense fold counts
    none of them — and behind an Inf on NaN and Inf.  "none" is the same rise without either."""
    x = _rising(only={}).copy()
    lo = 2400 * 12 + RISE_AT
    x[11, lo:lo + 640, 1] = _rising(only={11: 1})[11, lo:lo + 640, 1]
    if what != "none":
        x[11, lo + 16 * 20 + 5, 1] = np.nan if what == "nan" else np.inf
    r = _both(M, x, what, tune_segments=5)
    assert np.isinf(r["tp"][11, 1]) == (what == "inf"), r["tp"][11]


# ---- tiles that end inside a step, the true peak alone, the launch's last steps -----------------------------------------------

def test_44k1(M):
    _both(M, _rising(fs=44100.0), "44.1k", fs=44100.0, tune_segments=5)


def test_44k1_truepeak_only(M):
    _both(M, _rising(fs=44100.0), "44.1k tp", fs=44100.0, meters=M.METER_TRUEPEAK, tune_segments=5)


def test_truepeak_only(M):
    _both(M, _rising(), "tp", meters=M.METER_TRUEPEAK, tune_segments=5)


@pytest.mark.parametrize("fs", [48000.0, 44100.0])
def test_call_ends_seven_frames_behind_its_last_tile(M, fs):
    """Phase 0 of the call stops 24 frames in front of its end, 17 frames inside the last tile: the last two steps of the
    launch count their frames one by one.  The largest samples of streams 3 and 9 stand on both sides of that frame."""
    x = _rising(fs=fs, extra=7).copy()
    T = x.shape[1]
    x[3, T - 24 - 3, 0] = 900.0                  # the last frames phase 0 of this call counts
    x[3, T - 24 + 2, 1] = 1000.0                 # ... and one it leaves to the next call (the interpolated peaks still see it)
    x[9, T - 24 - 1, 1] = -800.0
    x[9, T - 24, 0] = 1100.0
    r = _both(M, x, "last steps %g" % fs, fs=fs, tune_segments=5)
    assert r["tp"][3, 0] >= 900.0 and r["tp"][9, 1] >= 800.0, (r["tp"][3], r["tp"][9])


# ---- per-stream lengths ---------------------------------------------------------------------------------------------------

def test_lengths_close_streams_inside_a_segment(M):
    """Stream 2 closes inside the rise of its third segment, stream 8 1000 frames before the end, stream 4 is empty and
    stream 7 closes on a segment boundary: the closing segments' columns carry -inf bounds next to live ones."""
    x = _rising().copy()
    T = x.shape[1]
    lengths = [T] * S
    lengths[2] = 2400 * 12 + RISE_AT + 16 * 13 + 3
    lengths[8] = T - 1000
    lengths[4] = 0
    lengths[7] = 2400 * 16
    x[2, lengths[2]:] = 7.0                                # past the end: never read
    r = _both(M, x, "lengths", lengths=lengths, tune_segments=5)
    assert r["tp"][4, 0] == 0 and r["tp"][4, 1] == 0, r["tp"][4]
