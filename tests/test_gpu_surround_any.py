"""Track lengths for the surround meter on the GPU (include/mtr_any.h: mtr_engine_process_*_any on a SURROUND engine; the LEN instantiations
of k_sur_pieces and k_sur_final, mtr_surround.hip).

Per stream the result must be sur_run's after exactly its own frames: _sur.run_oracle (O, fs, x[s][:total_s], ends_s), the composition of
the oracle's Kmeterdsp / Stcorrdsp.  The bounds are those of tests/test_gpu_surround.py, whose `compare` is used as it is: 2 D + 4 * 2^-23
against the float64 restatement for levels, correlations and pair states, with one sur_run per call also 1e-5 on the level; `peak` exact.

Without a period, three calls at 48 kHz: 1023 frames whole; n2 frames through _any; 2000 frames dense.  Two sets of ends for call 2:
  "one piece"   n2 = 3 * 4096 + 6 = 12294 frames.  The planner cuts a call without a period at `chunk` = 14224 frames (mtr_sur_geometry at
                48 kHz: warm = 112, chunk = (8 * 1792 - 112) & ~3), so this call is ONE piece of seven tiles.  Ends: n2 (open), 0, 1 and 3
                (no whole group), 1022 (inside the first tile, not a multiple of 4), 7001 (a later tile, 7001 mod 4 = 1), n2 - 1.
  "pieces"      n2 = 2 * 14224 + 4102 = 32550 frames: three pieces, [0, 14224), [14224, 28448), [28448, 32550).  Ends: n2 (open), 0,
                14224 (exactly on the first piece boundary), 20001 (inside the second piece), 30003 (inside the third), 28448 (on the
                second boundary), 14225 (one frame into the second piece: a piece of one frame).
With P = 2407 (P mod 4 = 3; capacity 4, below the open stream's six points): 1023 frames whole — the open block then stands inside a group
of four —, 5 P + 100 = 12135 frames through _any, 3000 frames dense.  The blocks end at call-2 frames 1384, 3791, 6198, 8605, 11012.  Ends:
12135 (open), 0, 700 (inside the block open on entry: r = 1723), 3791 (exactly on a boundary, r = 0: no extra point), 3793 (r = 2), 7199
(r = 1001 in a later block, r mod 4 = 1), 11010 (r = 2405: inside the block's dropped trailing frames).  series_points equals mtr_series_cut
per stream, the truncated point sits at the index of the whole blocks, the rows are 0.0f behind a closed stream's points.
Rows are longer than the audio; at and behind every stream's end — inside the call's buffer too — stands a poison: 0, 7.0 (a frame read
by mistake moves a sum) or NaN, and all three must give the same bits."""
import math

import numpy as np
import pytest

import _sur
import test_gpu_surround as tg

pytestmark = pytest.mark.gpu
FS, S = 48000, 7
N1, N3 = 1023, 2000
CHUNK = 14224
SETS = {"one piece": (3 * 4096 + 6, [3 * 4096 + 6, 0, 1, 3, 1022, 7001, 3 * 4096 + 5]),
        "pieces": (2 * CHUNK + 4102, [2 * CHUNK + 4102, 0, CHUNK, 20001, 30003, 2 * CHUNK, CHUNK + 1])}
ERR_ARG, ERR_UNSUPPORTED = -1, -2
bits = tg.bits


@pytest.fixture(scope="module")
def M():
    import meters.lv2_amd as m
    return m


@pytest.fixture(scope="module")
def O(oracle):
    return _sur.bind(oracle.lib)


def chunk_of(M, fs):
    """mtr_sur_geometry restated: |1 - w1|^J < 2^-48, warm = J rounded up past a multiple of 7, chunk = what eight tiles leave, on four"""
    w1 = float(M.stcorr_coef(float(fs))[0])
    J = min(max(math.ceil(-48.0 * math.log(2.0) / math.log(abs(1.0 - w1))), 1), 4 * 1792)
    warm = (int(J) + 7) // 7 * 7
    return (8 * 1792 - warm) & ~3


def own_frames(which, s):
    n2, ends = SETS[which]
    return (N1, ends[s], N3 if ends[s] == n2 else 0)


def rows(x, which, poison):
    """[S, T + 41, C]: every stream's own frames, `poison` at and behind its end"""
    n2, ends = SETS[which]
    buf = np.full((S, N1 + n2 + N3 + 41, x.shape[2]), np.float32(poison), np.float32)
    for s in range(S):
        n = sum(own_frames(which, s))
        buf[s, :n] = x[s, :n]
    return buf


def snap(e):
    return e.surround_read() + (e.surround_pair_states(),)


def run_any(M, nch, which, poison, host=False, meters=None):
    """the three calls -> (readings behind each call, the blob behind the last)"""
    import torch
    n2, ends = SETS[which]
    x = signal_of(nch, which)
    buf = rows(x, which, poison)
    W = buf.shape[1]
    fr = np.array(ends, np.uint64)
    rec = []
    with M.Engine(S, float(FS), M.METER_SURROUND if meters is None else meters, n_channels=nch) as e:
        if host:
            e.set_host_chunk_bytes(3 * ((n2 + 3) & ~3) * nch * 4)         # three streams per view: three views
            e.process(np.ascontiguousarray(buf[:, :N1]))
            rec.append(snap(e))
            e.process_any(np.ascontiguousarray(buf[:, N1:N1 + n2]), fr)
            rec.append(snap(e))
            e.process(np.ascontiguousarray(buf[:, N1 + n2:N1 + n2 + N3]))
            rec.append(snap(e))
        else:
            dev = torch.from_numpy(buf).cuda()
            st = torch.cuda.current_stream().cuda_stream
            e.process_device(dev.data_ptr(), N1, W, st)
            rec.append(snap(e))
            e.process_device_any(dev.data_ptr() + N1 * nch * 4, n2, fr, W, st)
            rec.append(snap(e))
            e.process_device(dev.data_ptr() + (N1 + n2) * nch * 4, N3, W, st)
            rec.append(snap(e))
            del dev
        frames, closed = e.stream_frames()
        assert frames.tolist() == [sum(own_frames(which, s)) for s in range(S)]
        assert closed.tolist() == [ends[s] < n2 for s in range(S)]
        blob = e.state_export()
    return rec, blob


_sig = {}


def signal_of(nch, which):
    """_sur.signals; in call 2 the frames behind a stream's last whole group of four — Kmeterdsp drops them (kmeterdsp.cc:79) — are the
    loudest of the stream: a K-meter that counted one of them shows it in `peak`, which is held exactly"""
    if (nch, which) not in _sig:
        n2, ends = SETS[which]
        x = _sur.signals(N1 + n2 + N3, FS, nch, seed=520 + nch, S=S)
        for s, E in enumerate(ends):
            x[s, N1 + (E & ~3):N1 + E] = np.float32(0.97) * np.where(np.arange(nch) % 2, -1, 1).astype(np.float32)
        assert np.abs(x).max() == np.float32(0.97) and (np.abs(x[:, :, :]) >= np.float32(0.97)).sum() == sum(E % 4 for E in ends) * nch
        _sig[nch, which] = x
    return _sig[nch, which]


def same_rec(a, b):
    return all(np.array_equal(bits(u), bits(v)) for ra, rb in zip(a, b) for u, v in zip(ra, rb))


# ---- per stream: sur_run after exactly its own frames ----------------------------------------------------------------------------------

@pytest.mark.parametrize("which", list(SETS))
@pytest.mark.parametrize("nch", [3, 6, 8])
def test_every_stream_is_sur_run_on_its_own_frames(M, O, nch, which):
    assert chunk_of(M, FS) == CHUNK
    n2, ends = SETS[which]
    x = signal_of(nch, which)
    rec, blob = run_any(M, nch, which, 7.0)
    for poison in (0.0, np.nan):                                       # whatever stands at and behind the ends: the same bits
        other, oblob = run_any(M, nch, which, poison)
        assert same_rec(rec, other) and blob == oblob, poison
    for s in range(S):
        fr = own_frames(which, s)
        blocks = np.cumsum([f for f in fr if f]).tolist()              # the sur_runs this stream got
        xs = x[s:s + 1, :blocks[-1]]
        want, exact = tg.yardstick(M, O, FS, xs, blocks)
        # what was read behind each of its blocks: call 1, then call 2 if it got frames of it, then call 3 if it stayed open
        at = [0] + ([1] if fr[1] else []) + ([2] if fr[2] else [])
        got = tuple(np.array([rec[i][k][s:s + 1] for i in at]) for k in range(4))
        tg.compare(f"C {nch} {which} stream {s} ({fr[1]} of {n2})", got, want, exact, tight=True)
        if nch == 3:
            assert not got[2][:, :, 3].any() and not got[3][:, :, 3].any()
        # a closed stream is where its own last frame left it: call 3 (and, at end 0, call 2) changed nothing of it
        # (surround_read arms the K-meters' flag for the next process (): nothing the getters show)
        for i in range(len(at), 3):
            assert all(np.array_equal(bits(rec[i][k][s]), bits(rec[len(at) - 1][k][s])) for k in range(4)), (s, i)


def test_whole_streams_are_the_dense_call(M):
    """frames[s] == n_frames on every stream: bit for bit mtr_engine_process_device"""
    import torch
    nch, which = 6, "pieces"
    n2, _ = SETS[which]
    x = np.ascontiguousarray(signal_of(nch, which)[:, :N1 + n2])
    dev = torch.from_numpy(x).cuda()
    st = torch.cuda.current_stream().cuda_stream
    with M.Engine(S, float(FS), M.METER_SURROUND, n_channels=nch) as a, M.Engine(S, float(FS), M.METER_SURROUND, n_channels=nch) as b:
        for e in (a, b):
            e.process_device(dev.data_ptr(), N1, N1 + n2, st)
        a.process_device(dev.data_ptr() + N1 * nch * 4, n2, N1 + n2, st)
        b.process_device_any(dev.data_ptr() + N1 * nch * 4, n2, np.full(S, n2, np.uint64), N1 + n2, st)
        assert a.state_export() == b.state_export() and not b.stream_frames()[1].any()
        assert all(np.array_equal(bits(u), bits(v)) for u, v in zip(snap(a), snap(b)))


# ---- paths and state -----------------------------------------------------------------------------------------------------------------------

def test_the_host_form_is_the_device_form(M):
    for nch, which in ((5, "one piece"), (6, "pieces")):
        d, dblob = run_any(M, nch, which, 7.0)
        h, hblob = run_any(M, nch, which, np.nan, host=True)
        assert same_rec(d, h) and dblob == hblob, (nch, which)


def test_five_channels_beside_the_loudness_meters(M):
    """EBU | TRUEPEAK | SURROUND through _any: the loudness results are bit for bit _lengths' on an engine without SURROUND, the surround
    readings those of the engine with SURROUND alone"""
    nch, which = 5, "one piece"
    n2, ends = SETS[which]
    buf = rows(signal_of(nch, which), which, np.nan)
    fr = np.array(ends, np.uint64)
    loud = M.METER_EBU | M.METER_TRUEPEAK
    with M.Engine(S, float(FS), loud | M.METER_SURROUND, n_channels=nch) as a, M.Engine(S, float(FS), loud, n_channels=nch) as b:
        rec = []
        for e, call in ((a, a.process_any), (b, b.process_lengths)):
            e.integr_start()
            e.process(np.ascontiguousarray(buf[:, :N1]))
            if e is a:
                rec.append(snap(e))
            call(np.ascontiguousarray(buf[:, N1:N1 + n2]), fr)
            if e is a:
                rec.append(snap(e))
            e.process(np.ascontiguousarray(buf[:, N1 + n2:N1 + n2 + N3]))
            if e is a:
                rec.append(snap(e))
        assert bytes(a.results()) == bytes(b.results()) and not np.isnan(a.out9()).any()
        assert all(np.array_equal(bits(u), bits(v)) for u, v in zip(a.truepeak_channels(), b.truepeak_channels()))
    alone, _ = run_any(M, nch, which, 7.0)
    assert same_rec(rec, alone)


def test_an_imported_stream_is_open_again(M):
    import torch
    nch, which = 6, "one piece"
    n2, ends = SETS[which]
    x = signal_of(nch, which)
    buf = rows(x, which, np.nan)
    dev = torch.from_numpy(buf).cuda()
    st = torch.cuda.current_stream().cuda_stream
    W = buf.shape[1]
    with M.Engine(S, float(FS), M.METER_SURROUND, n_channels=nch) as e:
        e.process_device(dev.data_ptr(), N1, W, st)
        e.process_device_any(dev.data_ptr() + N1 * nch * 4, n2, np.array(ends, np.uint64), W, st)
        assert e.stream_frames()[1].tolist() == [False] + [True] * (S - 1)
        assert e.state_import(e.state_export(4, 2), 4) == 2
        assert e.stream_frames()[1].tolist() == [False, True, True, True, False, False, True]
        before = snap(e)
        e.process_device(dev.data_ptr(), N3, W, st)                    # (any frames: the streams that are open move)
        after = snap(e)
        moved = [not np.array_equal(bits(after[0][s]), bits(before[0][s])) for s in range(S)]
        assert moved == [True, False, False, False, True, True, False]
        e.reset()
        assert not e.stream_frames()[1].any()


def test_refusals_and_arguments(M):
    nch, n = 6, 5000
    x = np.ascontiguousarray(signal_of(nch, "one piece")[:, :n])
    full = np.full(S, n, np.uint64)

    def refused(code, f, *args):
        with pytest.raises(M.EngineError) as err:
            f(*args)
        assert err.value.code == code, (err.value.code, str(err.value))

    with M.Engine(S, float(FS), M.METER_SURROUND, n_channels=nch) as e:
        e.process(x[:, :1000])
        before = (e.state_export(), e.stream_frames()[0].tolist())
        for f in (e.process_lengths, e.process_tracks, e.process_ragged, e.process_ends, e.process_tpb):
            refused(ERR_UNSUPPORTED, f, x, full)
        long = full.copy()
        long[2] = n + 1
        refused(ERR_ARG, e.process_any, x, long)
        assert M.lib.mtr_engine_process_host_any(e._h, x.ctypes.data, n, n, None) == ERR_ARG
        assert M.lib.mtr_engine_process_device_any(e._h, None, n, n, full.ctypes.data, None) == ERR_ARG
        assert (e.state_export(), e.stream_frames()[0].tolist()) == before
        # the period is a setting of an engine that has processed nothing: once _any has closed a stream it cannot be changed before
        # mtr_engine_reset, which reopens every stream — no call with a period ever meets a stream that was closed without one
        cut = full.copy()
        cut[3] = 17
        e.process_any(x, cut)
        assert e.stream_frames()[1].tolist() == [False] * 3 + [True] + [False] * 3
        refused(-7, e.surround_set_period, 2407, 8)
        assert e.stream_frames()[1][3]
        e.reset()
        e.surround_set_period(2407, 8)
        assert not e.stream_frames()[1].any() and not e.series_points(M.METER_SURROUND).any()
    # the one call _any cannot take: with a period, a stream that ends before the group of four frames completes which the call before
    # left open (its last sur_run would drop that whole group, and the state in front of it is not kept): refused, nothing queued
    with M.Engine(S, float(FS), M.METER_SURROUND, n_channels=nch) as e:
        e.surround_set_period(PERIOD, 8)
        e.process(x[:, :1021])                                         # (1021 mod 4 = 1: three frames complete the group)
        before = (e.state_export(), e.stream_frames()[0].tolist(), e.series_points(M.METER_SURROUND).tolist())
        for f in (1, 2):
            cut = full.copy()
            cut[5] = f
            refused(ERR_UNSUPPORTED, e.process_any, x, cut)
            assert (e.state_export(), e.stream_frames()[0].tolist(), e.series_points(M.METER_SURROUND).tolist()) == before
        cut[5] = 3
        e.process_any(x, cut)
        assert e.series_points(M.METER_SURROUND).tolist() == [2, 2, 2, 2, 2, 1, 2] and e.stream_frames()[1].tolist() == [False] * 5 + [True, False]
    with M.Engine(S, float(FS), M.METER_STCORR) as e:
        refused(ERR_ARG, e.series_points, M.METER_SURROUND)


# ---- with a period: the blocks a stream completed, then one last sur_run of what it has of the next ---------------------------------------

PERIOD = 2407                                                          # P mod 4 = 3
P1, P2, P3 = 1023, 5 * PERIOD + 100, 3000                              # call 1 leaves a block open, 1023 frames in: inside a group of four
E0 = PERIOD - P1                                                       # the call-2 frame at which that block ends: 1384; then every 2407
# open; untouched; inside the block open on entry (1723 frames of it: r mod 4 = 3); exactly on a block boundary (r = 0: no extra point);
# r = 2; r = 1001 in a later block (r mod 4 = 1); r = 2405 — inside the block's dropped trailing frames (2404 count)
P_ENDS = [P2, 0, 700, E0 + PERIOD, E0 + PERIOD + 2, E0 + 2 * PERIOD + 1001, E0 + 3 * PERIOD + 2405]
CAP = 4                                                                # the open stream completes six blocks


def p_frames(s):
    return (P1, P_ENDS[s], P3 if P_ENDS[s] == P2 else 0)


_psig = {}


def p_signal(nch):
    """as signal_of: the frames Kmeterdsp drops at the end of a stream's truncated block are the loudest of the stream"""
    if nch not in _psig:
        x = _sur.signals(P1 + P2 + P3, FS, nch, seed=540 + nch, S=S)
        for s, E in enumerate(P_ENDS):
            r = (P1 + E) % PERIOD
            if 0 < E < P2 and r:
                x[s, P1 + E - r % 4:P1 + E] = np.float32(0.97)
        _psig[nch] = x
    return _psig[nch]


def run_period(M, nch, poison, host=False, whole=False):
    import torch
    x = p_signal(nch)
    buf = np.full((S, P1 + P2 + P3 + 41, nch), np.float32(poison), np.float32)
    for s in range(S):
        n = P1 + P2 + P3 if whole else sum(p_frames(s))
        buf[s, :n] = x[s, :n]
    fr = np.full(S, P2, np.uint64) if whole else np.array(P_ENDS, np.uint64)
    W = buf.shape[1]
    with M.Engine(S, float(FS), M.METER_SURROUND, n_channels=nch) as e:
        e.surround_set_period(PERIOD, CAP)
        if host:
            e.set_host_chunk_bytes(3 * ((P2 + 3) & ~3) * nch * 4)
            e.process(np.ascontiguousarray(buf[:, :P1]))
            e.process_any(np.ascontiguousarray(buf[:, P1:P1 + P2]), fr)
            e.process(np.ascontiguousarray(buf[:, P1 + P2:P1 + P2 + P3]))
        else:
            dev = torch.from_numpy(buf).cuda()
            st = torch.cuda.current_stream().cuda_stream
            e.process_device(dev.data_ptr(), P1, W, st)
            e.process_device_any(dev.data_ptr() + P1 * nch * 4, P2, fr, W, st)
            e.process_device(dev.data_ptr() + (P1 + P2) * nch * 4, P3, W, st)
            del dev
        out = dict(series=e.surround_series(), last=e.surround_read(), states=e.surround_pair_states(), points=e.series_points(M.METER_SURROUND),
                   closed=e.stream_frames()[1], blob=e.state_export())
    return out


def same_out(a, b):
    arrs = lambda o: list(o["series"][:3]) + list(o["last"]) + [o["states"]]
    return all(np.array_equal(bits(u), bits(v)) for u, v in zip(arrs(a), arrs(b))) and a["series"][3:] == b["series"][3:] \
        and a["points"].tolist() == b["points"].tolist() and a["blob"] == b["blob"]


@pytest.mark.parametrize("nch", [3, 6, 8])
def test_with_a_period_every_stream_is_sur_run_on_its_own_blocks(M, O, nch):
    x = p_signal(nch)
    got = run_period(M, nch, 7.0)
    assert same_out(got, run_period(M, nch, np.nan))
    lv, pk, co, n_points, dropped = got["series"]
    total = (P1 + P2 + P3) // PERIOD
    assert (n_points, dropped) == (total, total - CAP) == (6, 2) and lv.shape == (S, CAP, nch)     # lock-step: the open stream's
    assert got["closed"].tolist() == [False] + [True] * (S - 1)
    for s in range(S):
        fr = p_frames(s)
        n = sum(fr)
        # the stream's points by mtr_series_cut, call by call; the truncated one sits at the index of the whole blocks
        fill = pts = 0
        for n_call, f in zip((P1, P2, P3), fr):
            whole, partial = M.series_cut(fill, PERIOD, n_call, f)
            pts += whole + partial
            if f < n_call:
                break
            fill = (fill + f) % PERIOD
        ends = [PERIOD * (k + 1) for k in range(n // PERIOD)] + ([n] if n % PERIOD and 0 < fr[1] < P2 else [])
        assert got["points"][s] == pts == len(ends), (s, pts, ends)
        kept = min(pts, CAP)
        assert not lv[s, kept:].any() and not pk[s, kept:].any() and not co[s, kept:].any(), s      # 0.0f behind its own points
        if not pts:
            assert not any(v[s].any() for v in got["last"])
            continue
        want, exact = tg.yardstick(M, O, FS, x[s:s + 1, :ends[-1]], ends)
        at = list(range(kept)) + [pts - 1]                                                          # ... and what surround_read reports: its last
        g = tuple(np.concatenate([ser[s:s + 1, :kept].transpose(1, 0, 2), last[s:s + 1][None]]) for ser, last in zip((lv, pk, co), got["last"]))
        tg.compare(f"C {nch} P {PERIOD} stream {s} ({fr[1]} of {P2}: {pts} points)", g + (None,), want, exact, at=at)
        if s:                                                                                       # closed at a block's end: the pair states stand there
            tg.compare(f"C {nch} P {PERIOD} stream {s} end", tuple(v[s:s + 1][None] for v in got["last"]) + (got["states"][s:s + 1][None],), want, exact, at=[pts - 1])
    assert got["points"].tolist() == [6, 0, 1, 2, 3, 4, 5]


def test_with_a_period_whole_streams_and_the_host_form(M):
    nch = 6
    import torch
    x = p_signal(nch)
    dev = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    st = torch.cuda.current_stream().cuda_stream
    T = x.shape[1]
    with M.Engine(S, float(FS), M.METER_SURROUND, n_channels=nch) as e:
        e.surround_set_period(PERIOD, CAP)
        e.process_device(dev.data_ptr(), P1, T, st)
        e.process_device(dev.data_ptr() + P1 * nch * 4, P2, T, st)
        e.process_device(dev.data_ptr() + (P1 + P2) * nch * 4, P3, T, st)
        dense = dict(series=e.surround_series(), last=e.surround_read(), states=e.surround_pair_states(), points=e.series_points(M.METER_SURROUND),
                     blob=e.state_export())
    assert same_out(dense, run_period(M, nch, np.nan, whole=True))        # frames[s] == n_frames on every stream: the dense call
    assert same_out(run_period(M, nch, 7.0), run_period(M, nch, np.nan, host=True))
