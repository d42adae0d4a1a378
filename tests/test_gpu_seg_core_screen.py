"""k_seg's core form (MTR_SEG_SCREEN=4, the default): each chunk screened with the taps' 32-sample core — three MFMAs, one per 16 of
the chunk's 48 rows, each over the one 8-aligned stretch of the window closest to those rows' taps (mtr_seg.hip: the core screen,
CORE) — against the dense form (0), bit for bit, and against form 3, whose chunks it screens.

The core product leaves out up to 2.6 % of a full-scale sample per output (the taps outside a row's stretch), and the vote's bound
eps' pays for that.  A bound without that term passes chunks whose outputs set a record by less than the dropped taps carry, so
stream 7 here carries its records exactly there: 64-frame blocks, each the window of one step, whose samples follow the signs of
row 13's taps (frame 4, phase 2: the row that drops the most) — at amplitude A under the dropped taps, A / 2 under the kept ones —
so that the row's output, 1.30 A, exceeds every sample, while the core sees 1.27 A of it; A rises by 1 % from block to block, so each
block's record exceeds the last by less than the 2 % the dropped taps hold.  The other streams are test_gpu_seg_lazy_lo.py's: an fs/4
sine at 45 degrees under noise, neighbours at 2^30, 1 and 2^-30, 13 streams x (26 tiles + 311 frames), 3 / 5 / 8 segments.

Held for every case: truepeak, truepeak_call and out9 of form 4 are the dense form's bits, seg_stats are equal, form 4 screens exactly
the chunks form 3 screens and completes more than none (not the same ones: its bound is wider), and the dense form counts nothing.  A
call with per-stream ends runs form 2 under MTR_SEG_SCREEN=4 as under 3: its counts are form 2's.
profiles/r30_kseg_core/test_mutant.txt: what this file and test_seg_core_bound.py do with builds that have one wrong line each."""
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
DROP = 7                                                   # the stream whose records sit in the dropped taps (level 1)
ROW_F, ROW_P = 4, 1                                        # row n = 3 f + p = 13 of the frame-major list: fragment 0, stretch [8, 40)


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


def _all(M, x, tag, calls=None, other=3, **kw):
    """Form 4 against the dense form (0) and against `other` (3: the same chunks screened; 2 for a call with per-stream ends: the
    same counts)."""
    x = np.ascontiguousarray(x)
    calls = calls or [x.shape[1]]
    r4, r3, r0 = (_run(M, mode, x, calls, **kw) for mode in (4, other, 0))
    print(tag, "seg", r4["seg"], "screened, completed: form 4", r4["refine"], "form %d" % other, r3["refine"], "dense", r0["refine"])
    assert r4["seg"][0] > 0, (tag, "k_seg did not run", r4["seg"])
    assert r4["seg"] == r0["seg"] and r3["seg"] == r0["seg"], tag
    assert _bits_equal(r4["tp"], r0["tp"]), (tag, r4["tp"], r0["tp"])
    assert _bits_equal(r4["per_call"], r0["per_call"]), (tag, r4["per_call"], r0["per_call"])
    if r0["o9"] is not None:
        assert _bits_equal(r4["o9"], r0["o9"]), tag
    assert r4["refine"][0] == r3["refine"][0] > 0, (tag, "form 4 screens the chunks form %d does" % other, r4["refine"], r3["refine"])
    assert r4["refine"][1] > 0, (tag, r4["refine"])
    if other == 2:
        assert r4["refine"] == r3["refine"], (tag, "a call with per-stream ends runs form 2", r4["refine"], r3["refine"])
    assert r0["refine"] == (0, 0), (tag, "the dense form counts nothing", r0["refine"])
    return r4, r0


def _sine45(T, lo=0.3, hi=1.0):
    """fs/4 at 45 degrees, amplitude lo .. hi over T: samples at 0.707 of the amplitude, the peak half-way between them."""
    n = np.arange(T)
    s = np.sin(0.5 * np.pi * n + 0.25 * np.pi) * np.linspace(lo, hi, T)
    return np.stack([s, -0.97 * s], 1).astype(np.float32)


def _level(s):
    return np.float32(2.0 ** (30, 0, -30)[s % 3])


_cache = {}


def _taps48(M):
    """g[3][48]: phases 1 - 3 in window order (g[p][i] multiplies x[n - 47 + i])."""
    tab = M.fir_table()
    g = np.zeros((3, 48), np.float32)
    for ph in range(1, 4):
        for i in range(48):
            g[ph - 1, i] = tab[24 * ph + i] if i < 24 else tab[24 * (4 - ph) + (47 - i)]
    return g


def _dropped_stream(M, T, a0=1e-3, stop=None):
    """64-frame blocks on absolute frames 64 k .. 64 k + 63 = the window of the step whose outputs are frames 64 k + 48 .. 64 k + 63
    (tiles, and with them every segment, start on a multiple of 16): window position t holds sign (g[t - 1 - f]) x (A under the row's
    dropped taps — outside [8, 40) — and A / 2 under its kept ones), zero outside the row's 48 taps; A = a0 x 1.01^k.  Silent from
    `stop` on, so that the stream's last record is one k_seg finds.  The right channel is the left one negated, 3 % lower."""
    g = _taps48(M)[ROW_P]
    pat = np.zeros(64)
    for t in range(64):
        i = t - 1 - ROW_F
        if 0 <= i < 48:
            pat[t] = np.sign(g[i]) * (0.5 if 8 <= t < 40 else 1.0)
    # The sixteen positions outside the row's taps (53 .. 63 and 0 .. 4: zero taps for the row, so its output is untouched) carry
    # 0.3 A: the alternation of the dropped taps continued behind position 52 and inverted in front of position 5.  Left at zero,
    # the windows that straddle two blocks and have the alternating run under their middle taps reach 1.40 A (phase 1, 12 frames
    # into a block) and the records would be theirs — rows whose cores see them; so the next-largest output is 1.20 A.
    for k, t in enumerate(list(range(53, 64)) + list(range(0, 5))):
        pat[t] = pat[52] * (-1.0) ** (k + 1) * (0.3 if k < 11 else -0.3)
    nb = T // 64
    amp = a0 * 1.01 ** np.arange(nb)
    left = np.zeros(T)
    left[:nb * 64] = (amp[:, None] * pat[None, :]).reshape(-1)
    if stop is not None:
        left[stop:] = 0.0
    return np.stack([left, -0.97 * left], 1).astype(np.float32)


def _programme(M, T):
    """Never modified by a test (tests that need a variant copy it)."""
    if T not in _cache:
        rows = []
        for s in range(S):
            x = tri_noise(T, 400 + s, 0.1, period=7000 + 1000 * s) + _sine45(T, 0.3 + 0.01 * s, 1.0 + 0.02 * s)
            rows.append((x * _level(s)).astype(np.float32))
        rows[DROP] = _dropped_stream(M, T, stop=(T - 311) - 128 if T == T48 else None)
        x = np.stack(rows)
        x.setflags(write=False)
        _cache[T] = x
    return _cache[T]


def _records_in_dropped_taps(r, x):
    """Stream 7's peak is the last block's row-13 output: 1.30 of the largest sample, of which the core sees 1.27."""
    mx = np.abs(x[DROP]).max(0)
    assert (r["tp"][DROP] > 1.29 * mx).all() and (r["tp"][DROP] < 1.31 * mx).all(), (r["tp"][DROP], mx)


@pytest.mark.parametrize("segs", [3, 5, 8])
def test_ebu_and_truepeak(M, segs):
    """The programme at 3, 5 and 8 segments per stream (39, 65 and 104 lanes: streams straddle 16-lane rows and waves)."""
    x = _programme(M, T48)
    r4, _ = _all(M, x, "segments %d" % segs, tune_segments=segs)
    _records_in_dropped_taps(r4, x)


def test_truepeak_only(M):
    """The true peak alone (the instantiations without the recurrence)."""
    x = _programme(M, T48)
    r4, _ = _all(M, x, "tp", meters=M.METER_TRUEPEAK, tune_segments=5)
    _records_in_dropped_taps(r4, x)


def test_44k1(M):
    """44.1 kHz: tiles of 2205 frames end inside a step, and the launch's last step runs dense with masked rows."""
    T = 2205 * 26 + 311
    _all(M, _programme(M, T), "44.1k", fs=44100.0, tune_segments=5)


@pytest.mark.parametrize("cuts", [(2400 * 9 + 2395,), (2400 * 7 + 100, 2400 * 19 + 1)])
def test_two_and_three_calls(M, cuts):
    """Calls that are no whole number of tiles: the later launches start inside a tile, their first windows hold the history, and the
    first call's hold the zeros in front of it."""
    x = _programme(M, T48)
    edges = (0,) + tuple(cuts) + (T48,)
    _all(M, x, "%d calls" % (len(cuts) + 1), calls=[b - a for a, b in zip(edges[:-1], edges[1:])], tune_segments=5)


def test_level_jump_inside_a_window(M):
    """Every stream but the block stream jumps by 2^26 on frame 8 of a step and by 2^13 again 20 frames later: two rescales within one
    64-sample window, whose words under the dropped taps were split under other scales than those under the core."""
    x = _programme(M, T48).copy()
    for s in range(S):
        if s == DROP:
            continue
        at = 2400 * 2 + 16 * (97 * s) + 8
        x[s, :at] *= np.float32(2.0 ** -39)
        x[s, at:at + 20] *= np.float32(2.0 ** -13)
    r4, _ = _all(M, x, "two rescales", tune_segments=5)
    _records_in_dropped_taps(r4, x)


def test_silent_nan_and_inf_streams(M):
    """Stream 1 is silent (eps' = CORE_K_ABS against a reference of zero), stream 3 holds one Inf sample and stream 4 one NaN
    sample; stream 10's NaN sits on the last frame of a 64-frame block, under the zero padding of every row of the step that ends there
    and under the dropped taps of the next step's rows.  Their neighbours are unaffected."""
    x = _programme(M, T48).copy()
    x[1] = 0.0
    x[3, 30000, 0] = np.inf
    x[4, 41000, 1] = np.nan
    x[10, 64 * 500 + 63, 0] = np.nan
    r4, _ = _all(M, x, "silent / inf / nan", tune_segments=5)
    assert r4["tp"][1, 0] == 0 and r4["tp"][1, 1] == 0
    assert np.isinf(r4["tp"][3, 0]) and np.isfinite(r4["tp"][3, 1]) and np.isfinite(r4["tp"][4]).all() and np.isfinite(r4["tp"][10]).all()
    _records_in_dropped_taps(r4, x)


def test_lengths_give_form_2s_counts(M):
    """process_lengths with ends inside a window, an empty stream and one that closes on a segment boundary: the kernels that take
    per-stream ends have no core form, so under MTR_SEG_SCREEN=4 the call runs form 2."""
    x = _programme(M, T48).copy()
    lengths = [T48] * S
    lengths[2] = 2400 * 11 + 300
    lengths[8] = T48 - 3000
    lengths[4] = 0
    lengths[DROP] = 2400 * 16
    x[2, lengths[2]:] = 7.0                                # past the end: never read
    r4, _ = _all(M, x, "lengths", other=2, lengths=lengths, tune_segments=5)
    assert r4["tp"][4, 0] == 0 and r4["tp"][4, 1] == 0, r4["tp"][4]
