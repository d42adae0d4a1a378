"""k_seg's screened step — eight first products back to back, the votes behind them as lane masks, one branch per step — against
the dense form (MTR_SEG_SCREEN=0), bit for bit, on inputs that make chunks fail their votes where the step's order matters:

  * clicks that set new records in every stream at once: several failing chunks in one step, in every block and channel;
  * records in the last block (chunks 6 and 7), whose windows' oldest quarter the step's own ring stores overwrite;
  * a rescale in the step whose products hold a record, and in the step behind it;
  * records in the launch's last two steps (the last one runs the dense products);
  * 44.1 kHz (tiles that end inside a step), per-stream lengths, and a stream fed in arbitrary pieces across calls.

Every record is an equal adjacent pair, whose peak lies between its samples: each stream's counted peak (and each long call's) is a
value a completed chunk computed, which the test checks, so a completion that computes anything else changes the bits compared.
Every run also checks the chunk counters behind mtr_engine_refine_stats: the screened form counts its chunks and completes some
(but not all) of them, the dense form counts nothing."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _signals as sig  # noqa: E402


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


def _run(M, screen, x, calls, fs, lengths=None, meters=None, **kw):
    meters = meters if meters is not None else (M.METER_EBU | M.METER_TRUEPEAK)
    with _engine(M, screen, x.shape[0], fs, meters, tune_layout=7, **kw) as e:
        if meters & M.METER_EBU:
            e.integr_start()
        pos, per_call = 0, []
        for n in calls:
            piece = np.ascontiguousarray(x[:, pos:pos + n])
            if lengths is None:
                e.process(piece)
            else:
                e.process_lengths(piece, np.clip(lengths - pos, 0, n).astype(np.uint64))
            per_call.append(np.array([[r.truepeak_call[0], r.truepeak_call[1]] for r in e.results()], np.float32))
            pos += n
        return dict(tp=e.truepeak(), per_call=np.stack(per_call), o9=e.out9() if meters & M.METER_EBU else None,
                    seg=e.seg_stats(), refine=e.refine_stats())


def _inter_sample(res, x, calls, tag, lengths=None):
    """The peaks the comparison rests on must be values the products computed, not samples: every stream's counted peak lies
    more than 10 % above every sample it could have counted (the records are equal adjacent pairs: 1.27 x the sample)."""
    S, T = x.shape[0], x.shape[1]
    ends = np.full(S, T, np.int64) if lengths is None else np.asarray(lengths, np.int64)
    for s in range(S):
        if ends[s] < 4800:
            continue
        top = np.abs(x[s, :ends[s] - (24 if ends[s] == T else 48)]).max(axis=0)
        assert np.all(res["tp"][s] > 1.1 * top), (tag, "stream %d: the peak is a sample" % s, res["tp"][s], top)
    pos = 0
    for k, n in enumerate(calls):
        if lengths is None and n >= 24000:
            top = np.abs(x[:, pos:pos + n - 48]).max(axis=1)
            held = top >= 0.02                            # (windows that hold a record)
            assert held.sum() >= S, (tag, "call %d: too few records" % k)
            assert np.all(res["per_call"][k][held] > 1.1 * top[held]), (tag, "call %d: a peak is a sample" % k)
        pos += n


def _both(M, x, calls, tag, fs=48000.0, **kw):
    a = _run(M, True, x, calls, fs, **kw)
    b = _run(M, False, x, calls, fs, **kw)
    assert a["seg"][0] > 0, (tag, "k_seg did not run", a["seg"])
    assert a["seg"] == b["seg"], tag
    assert np.array_equal(a["tp"].view(np.uint32), b["tp"].view(np.uint32)), (tag, a["tp"], b["tp"])
    assert np.array_equal(a["per_call"].view(np.uint32), b["per_call"].view(np.uint32)), tag
    if a["o9"] is not None:
        assert np.array_equal(a["o9"].view(np.uint32), b["o9"].view(np.uint32)), tag
    scr, fin = a["refine"]
    assert scr > 0 and 0 < fin < scr, (tag, "the votes failed nowhere or everywhere", a["refine"])
    assert b["refine"] == (0, 0), (tag, "the dense form counts nothing", b["refine"])
    _inter_sample(a, x, calls, tag, kw.get("lengths"))
    return a


def _pair(x, s, p, c, g):
    """A record whose peak lies between two samples: two equal adjacent samples (the interpolator gives 1.27 x their value)."""
    x[s, p:p + 2, c] = np.float32(g)


def _records(T, S, fs, seed, P):
    """Quiet noise with records of rising size at the same frames in every stream (each a new record: its chunks fail their votes),
    records of its own in the last block of the wave (streams S - 4 .. S - 1 with 4 segments: chunks 6, 7), records in the launch's
    last two steps (streams 0 .. 7), and two streams that rescale (13, 14).  Every record is an equal adjacent pair, so every
    stream's peak is an interpolated value of a chunk that completed.

    The rescale streams sit at 1.4e-5 (their scale: a cap of 2^-5), with one record of 0.03 at frame P (interpolated peak 0.038,
    output frame P + 24) and one sample of 0.032 behind it, which reaches the cap: at 48 kHz with P = 0 mod 16 the record's products
    run in the step of the rescale (stream 13: the sample in that step) or in the step before it (stream 14: a step later)."""
    x = np.stack([sig.lcg_noise(T, seed + s, 0.01) for s in range(S)]).astype(np.float32)
    rng = np.random.default_rng(seed)
    pos = np.sort(rng.choice(np.arange(64, T - 64), size=40, replace=False))
    for k, p in enumerate(pos):
        for c in (0, 1):
            x[:, p:p + 2, c] = np.float32(0.03 * 1.07 ** k) * np.float32(1.0 if k % 2 else -1.0)
    for k, p in enumerate(range(T // 3, T - 200, 2011)):
        for s in range(S - 4, S):
            _pair(x, s, p + 5, k & 1, 0.5 + 0.01 * k)
            _pair(x, s, p + 21, 1 - (k & 1), 0.51 + 0.01 * k)
    for s in range(8):                                # the launch's last step (dense products) and the step before it
        for c in (0, 1):
            _pair(x, s, T - 36 if s < 4 else T - 52, c, 3.0)
    for s, d in ((S - 3, 37), (S - 2, 53)):
        x[s] = sig.lcg_noise(T, seed + 100 + s, 1.4e-5)
        for c in (0, 1):
            _pair(x, s, P, c, 0.03)
        x[s, P + d, :] = np.float32(0.032)
    return x


def test_step_vote_records_48k(M):
    """16 streams x 4 segments: one full wave (64 lanes, every block and channel)."""
    fs, S = 48000.0, 16
    T = 2400 * 40
    x = _records(T, S, fs, 100, 60000)
    _both(M, x, [T], "48k", fs=fs, tune_segments=4)
    _both(M, x, [T], "48k tp", fs=fs, meters=M.METER_TRUEPEAK, tune_segments=4)


def test_step_vote_records_44k1(M):
    fs, S = 44100.0, 16
    T = 2205 * 40 + 391
    x = _records(T, S, fs, 200, 60000)
    _both(M, x, [T], "44.1k", fs=fs, tune_segments=4)
    _both(M, x, [T], "44.1k tp", fs=fs, meters=M.METER_TRUEPEAK, tune_segments=4)


@pytest.mark.parametrize("fs", [48000.0, 44100.0])
def test_step_vote_records_lengths(M, fs):
    """Per-stream lengths: streams that end early (records behind the end must not count), at the end, and one with no frames."""
    S = 16
    tile = int(fs) // 20
    T = tile * 40
    x = _records(T, S, fs, 300, 60000)
    lengths = np.full(S, T, np.int64)
    lengths[1], lengths[6], lengths[13], lengths[15] = T // 3 + 17, T - 700, 60000 + 300, 0
    _both(M, x, [T], "lengths %g" % fs, fs=fs, lengths=lengths, tune_segments=4)


@pytest.mark.parametrize("fs", [48000.0, 44100.0])
def test_step_vote_records_streaming(M, fs):
    """The same records fed in pieces that split steps and tiles: every call a launch of its own, with its own last step."""
    S = 16
    tile = int(fs) // 20
    T = tile * 60 + 211
    x = _records(T, S, fs, 400, 60000)
    calls = [tile * 17 + 5, tile * 25 - 5, 333, tile * 10, T - (tile * 52 + 333)]
    _both(M, x, calls, "pieces %g" % fs, fs=fs, tune_segments=2)
