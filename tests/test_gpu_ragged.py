"""Ragged batches for the phase correlation and the needle meters: mtr_engine_process_device_ragged / _host_ragged on the GPU.

The semantics are those of the _tracks pair (a stream advances by frames[s] <= n_frames frames of a call, frames[s] < n_frames closes it
until mtr_engine_reset), for engines of EBU, TRUEPEAK, DR14, KMETER, BITSTATS, SIGDIST, STCORR and NEEDLE in any combination.  Per stream
the result is the reference's after exactly the stream's own frames, fed in the engine's blocks with the last one truncated.  Held here:
  * identity: lengths all n_frames give bit for bit what process_device gives (getters, series, series_points, state blob); the open
    streams of a ragged batch are bit for bit the same streams of a dense batch; on a mask that _tracks takes, _ragged equals _tracks;
  * whatever lies past a stream's end (NaN, Inf, 1e30, denormals) changes nothing of any stream, bit for bit;
  * each closed stream against the restatement (mo_stcorr_*, mo_vu_*, mo_ppm_*, mo_msppm_*) fed exactly its own frames in the same blocks:
    NEEDLE bit for bit (readings, series, z1 / z2), STCORR by the rule of tests/test_gpu_stcorr.py (2 D + 4 * 2^-23, D measured per
    stream from the oracle's distance to the float64 loop); series_points is the number of process () calls the restatement made; the
    series rows hold 0.0f behind a stream's own points;
  * closed streams stay frozen through later calls of every entry; the meters' resets reopen nothing, mtr_engine_reset does;
  * the host form equals the device form bit for bit across three chunks; a pair of 6-channel frames equals the compact stereo call;
  * beside EBU / TRUEPEAK / KMETER the loudness results are bit for bit _lengths', the K-meter's _tracks';
  * 64 streams x 2 s with uniform random lengths against the restatement on eight sampled streams;
  * the meters that take no ragged call, and argument errors, leave the engine unchanged.
The 16 streams of the main cases end: at frame 0 of the first call (closed untouched), at frame 1, inside the first tile, on a tile
boundary, on a period end (r = 0), 1, 3 and 5 frames past it, at n_frames - 1 of a call, exactly at a call's end (closed with 0 by the
next call), one frame into a call, inside the last call, never.
"""
import contextlib

import numpy as np
import pytest

import test_gpu_needle as N
import test_gpu_stcorr as SC
from test_gpu_kmeter import signal as km_signal
from test_gpu_needle import ALL, IEC1, IEC2, KINDS, VU, kinds_of, oracle_run, same
from test_gpu_needle import O as needle_oracle  # noqa: F401  (a fixture)
from test_gpu_stcorr import FLOOR, scale_of, yardstick
from test_gpu_stcorr import O as stcorr_oracle  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu
CALLS = [5000, 3 * 4096 + 6, 1, 40000]
T = sum(CALLS)
ENDS = np.cumsum(CALLS).tolist()                                     # 5000, 17294, 17295, 57295
ERR_ARG, ERR_UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def M():
    import meters.lv2_amd as m
    assert m.engine.ERR_ARG == ERR_ARG and m.engine.ERR_UNSUPPORTED == ERR_UNSUPPORTED
    return m


def lengths(P):
    """the 16 total lengths; P: the period the block ends are counted in (for period 0: a nominal one)"""
    pe = P * max(1, -(-5500 // P))                                   # a period end inside the second call (P = 40000: the fourth)
    L = [0, 1, 700, 4096, pe, pe + 1, pe + 3, pe + 5, ENDS[1] - 1, ENDS[1], ENDS[3] - 1, ENDS[2] + 1, ENDS[0] - 1, 30000, ENDS[0] + 2, T]
    assert len(L) == 16 and all(0 <= v <= T for v in L) and pe + 5 < T
    return L


def frames_per_call(L, calls):
    """frames of every call for a stream of total length L (0 once it has closed)"""
    out, p, done = [], 0, False
    for c in calls:
        f = 0 if done else int(min(max(L - p, 0), c))
        done = done or f < c
        out.append(f)
        p += c
    return out


def blocks_of(L, P, calls=CALLS):
    """(ends of the process () calls of a host that feeds the stream its own L frames in the engine's blocks, the last one truncated;
    whether the stream's state stands at the last of them): blocks of P, or (P = 0) the calls.  A stream whose length is a call's end
    is closed with 0 frames by the next call, untouched: nothing is truncated, and between two blocks its state is an open block's."""
    total, cuts = sum(calls), np.cumsum(calls).tolist()
    if P == 0:
        ends = [c for c in cuts if c <= L]
        if L not in cuts and L > 0:
            ends.append(L)
        return ends, True
    ends = [P * (k + 1) for k in range(L // P)]
    closed_by_zero = L in cuts and L < total
    if L % P and L < total and not closed_by_zero:
        ends.append(L)
    return ends, L % P == 0 or (L < total and not closed_by_zero)


def run_calls(e, ptr, stride, width, calls, Ls=None, entry="ragged", host=None):
    """the calls over a device buffer [S, stride, width] at ptr (or the host array `host` [S, T, width]): dense (Ls None) or ragged"""
    pos = 0
    for i, n in enumerate(calls):
        f = None if Ls is None else np.array([frames_per_call(L, calls)[i] for L in Ls], np.uint64)
        if host is not None:
            blk = np.ascontiguousarray(host[:, pos:pos + n])
            e.process(blk) if f is None else getattr(e, "process_" + entry)(blk, f)
        elif f is None:
            e.process_device(ptr + pos * width * 4, n, stride=stride)
        else:
            getattr(e, "process_device_" + entry)(ptr + pos * width * 4, n, f, stride=stride)
        pos += n


def snap(M, e, needle_period=1):
    """every getter of STCORR / NEEDLE / KMETER / EBU in the engine and each stream's part of the state blob.  (At period 0 needle_read
    arms a new maximum — it writes the state — so it is left to the tests that look at it once.)"""
    m, out = e.meters, {}
    if m & M.METER_STCORR:
        out["sc_corr"], out["sc_state"] = e.stcorr_read()
        out["sc_series"], out["sc_n"], out["sc_dropped"] = e.stcorr_series()
        out["sc_points"] = e.series_points(M.METER_STCORR)
    if m & M.METER_NEEDLE:
        out["nd_points"] = e.series_points(M.METER_NEEDLE)
        for k in kinds_of(e._kinds):
            out[f"nd_series{k}"], out[f"nd_n{k}"], out[f"nd_dropped{k}"] = e.needle_series(k)
            if needle_period:
                out[f"nd_level{k}"], out[f"nd_state{k}"] = e.needle_read(k)
    if m & M.METER_KMETER:
        out["km_rms"], out["km_peak"] = e.kmeter_read()
    if m & (M.METER_EBU | M.METER_TRUEPEAK):
        hm, hs = e.histograms()
        r = e.results()
        out.update(out9=e.out9(), hm=hm, hs=hs,
                   tp=np.array([[x.truepeak[0], x.truepeak[1], x.truepeak_call[0], x.truepeak_call[1]] for x in r], np.float32))
    hdr = 2 * e.state_bytes(1) - e.state_bytes(2)
    out["blob"] = np.stack([np.frombuffer(e.state_export(s, 1), np.uint8)[hdr:] for s in range(e.n_streams)])
    return out


def without_cursors(blob, e):
    """a snapshot's blob rows [S, bytes] of a STCORR | NEEDLE engine with the HOST-owned fields zeroed: each stream's entry carries a copy
    of the engine's lock-step cursors (mtr_stcorr_state.fill, mtr_needle_hdr.fill: written at export from the host's, the same in every
    entry), which move on with the open streams whatever a closed stream does.  The two sections are the entry's last: 32 bytes of
    STCORR, then the needle header (32) and 32 bytes per (kind, channel)."""
    out = blob.copy()
    nd = 32 + len(kinds_of(e._kinds)) * e.n_channels * 32
    sc = out.shape[1] - nd - 32
    out[:, sc + 28:sc + 32] = 0
    out[:, sc + 32 + 8:sc + 32 + 12] = 0
    return out


def rows(s, idx):
    return {k: (np.ascontiguousarray(np.asarray(v)[idx]) if np.ndim(v) else v) for k, v in s.items()}


def assert_same(a, b, what=""):
    assert a.keys() == b.keys()
    for k in a:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), (what, k)


def engine(M, S, fs, meters, chn=2, sc_period=0, nd_kinds=None, nd_period=0, cap=0):
    e = M.Engine(S, float(fs), meters, n_channels=chn)
    if meters & M.METER_EBU:
        e.integr_start()
    if meters & M.METER_STCORR and sc_period:
        e.stcorr_set_period(sc_period, cap)
    e._kinds = 0
    if meters & M.METER_NEEDLE:
        e._kinds = nd_kinds or (ALL if chn == 2 else VU | IEC1 | IEC2)
        e.needle_configure(e._kinds, nd_period, cap)
    return e


_sig = {}


def sc_audio(fs, S=16, extra=0):
    """S streams of tests/test_gpu_stcorr.py's signals (three seeds of its seven), T frames and `extra` frames of silence behind them"""
    if (fs, S) not in _sig:
        x = np.concatenate([SC.signals(T, fs, seed) for seed in range(500, 500 + (S + 6) // 7)])
        _sig[(fs, S)] = np.ascontiguousarray(x[np.arange(S) % len(x) if S > len(x) else np.arange(S)])
    return np.concatenate([_sig[(fs, S)], np.zeros((S, extra, 2), np.float32)], axis=1)


def nd_audio(S, chn, extra=0):
    x = N.signal(S, T)
    if chn == 1:
        x = x[:, :, :1]
    return np.concatenate([x, np.zeros((S, extra, chn), np.float32)], axis=1)


def to_device(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


@contextlib.contextmanager
def needle_rate(fs):
    """tests/test_gpu_needle.py drives its oracle at its module's rate"""
    old, N.FS = N.FS, fs
    try:
        yield
    finally:
        N.FS = old


def poison(x, Ls):
    y = x.copy()
    junk = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 1e-42, -1e-45, 3.0e38], np.float32)
    for s, L in enumerate(Ls):
        n = y.shape[1] - L
        y[s, L:] = np.resize(junk, n * y.shape[2]).reshape(n, y.shape[2])
    return y


# ---- STCORR ----------------------------------------------------------------------------------------------------------------------------

def check_stcorr_stream(O, fs, xs, L, P, corr, state, series, points, who, calls=CALLS):
    """one closed (or open) stream of total length L against the restatement"""
    ends, at_block = blocks_of(L, P, calls)
    assert int(points) == (len(ends) if P else 0), (who, "series_points", int(points), len(ends))
    if P:
        assert not series[len(ends):].any(), (who, "the row behind the stream's own points")
    if not ends:
        assert corr == 0 and (L > 0 or not state.any()), who          # (no process () has ended: no reading; L 0: not touched)
        return
    want, want_st, D, D_rel = yardstick(O, fs, xs[:L], ends)
    d = abs(float(corr) - float(want[-1]))
    assert d <= 2 * D + FLOOR, (who, "reading", D, d)
    if P:
        ds = np.abs(series[:len(ends)].astype(np.float64) - want)
        assert np.all(ds <= 2 * D + FLOOR), (who, "series", D, float(ds.max()), int(ds.argmax()))
        d = max(d, float(ds.max()))
    dr = 0.0
    if at_block:
        sc = scale_of(want_st[-1])
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = np.where(sc > 0, np.abs(state.astype(np.float64) - want_st[-1]) / sc, 0.0)
        dr = float(rel.max())
        assert dr <= 2 * D_rel + FLOOR, (who, "state", D_rel, rel)
    print(f"{who}: {len(ends)} blocks, D {D:.3g} seen {d:.3g} | D_rel {D_rel:.3g} seen {dr:.3g}")


@pytest.mark.parametrize("fs", [48000, 44100])
@pytest.mark.parametrize("per", ["0", "fs/20", "40000"])
def test_stcorr_closed_streams_against_the_restatement(M, stcorr_oracle, fs, per):
    P = {"0": 0, "fs/20": fs // 20, "40000": 40000}[per]
    Ls = lengths(P or fs // 20)
    extra = P                                                        # one more block for the open stream: the lock-step count passes every truncated point
    x = sc_audio(fs, extra=extra)
    cap = (T + extra) // P + 2 if P else 0
    dev = to_device(poison(x, Ls))
    clean = to_device(x)
    with engine(M, 16, fs, M.METER_STCORR, sc_period=P, cap=cap) as e, engine(M, 16, fs, M.METER_STCORR, sc_period=P, cap=cap) as e2:
        run_calls(e, dev.data_ptr(), x.shape[1], 2, CALLS, Ls)
        run_calls(e2, clean.data_ptr(), x.shape[1], 2, CALLS, Ls)
        a, b = snap(M, e), snap(M, e2)
        assert_same(a, b, "poison past the ends")
        frames, closed = e.stream_frames()
        assert frames.tolist() == Ls and closed.tolist() == [L < T for L in Ls]
        if extra:                                                    # a dense call behind: the closed streams stay as they are
            e.process_device(clean.data_ptr() + T * 8, extra, stride=x.shape[1])
            c = snap(M, e)
            assert_same(rows({k: v for k, v in a.items() if k in ("sc_corr", "sc_state", "sc_points", "blob")}, slice(0, 15)),
                        rows({k: v for k, v in c.items() if k in ("sc_corr", "sc_state", "sc_points", "blob")}, slice(0, 15)), "frozen")
            a = c
            assert a["sc_n"] == (T + extra) // P and a["sc_dropped"] == 0
    for s, L in enumerate(Ls):
        Ls_s = L + extra if s == 15 else L                            # (the open stream took the extra block)
        series = a["sc_series"][s] if P else np.zeros(0, np.float32)
        if s == 15 and P:
            ends = [P * (k + 1) for k in range(Ls_s // P)]
            want, _, D, _ = yardstick(stcorr_oracle, fs, x[s], ends)
            assert int(a["sc_points"][s]) == len(ends) == a["sc_n"]
            assert np.all(np.abs(series[:len(ends)].astype(np.float64) - want) <= 2 * D + FLOOR), (fs, P, s)
            continue
        check_stcorr_stream(stcorr_oracle, fs, x[s], L, P, a["sc_corr"][s], a["sc_state"][s], series, a["sc_points"][s], f"fs {fs} P {P} stream {s} L {L}")


def test_stcorr_end_in_a_periods_second_piece(M, stcorr_oracle):
    """P = 40000 and one call of 45000 frames from reset: the first period is cut into two pieces (a piece holds at most 8 tiles less
    the frames that rebuild the first stage), and streams end in the second one, on the cut and one frame to either side of it, around the
    period's end and in the call's second period"""
    fs, P, n = 48000, 40000, 45000
    w1 = float(M.stcorr_coef(float(fs))[0])
    J = int(np.ceil(-48.0 * np.log(2.0) / np.log(abs(1.0 - w1))))
    cut = 8 * 4096 - (J + 16) // 16 * 16                             # mtr_stcorr_geometry: chunk = MAX_TILES * TILE - warm
    assert 32000 < cut < 32768
    Ls = [33000, 39999, 40000, 40001, cut - 1, cut, cut + 1, 44999, cut - 4096, n]
    x = sc_audio(fs, extra=n + P - T)[:len(Ls)]
    assert x.shape[1] == n + P
    dev, clean = to_device(poison(x, Ls)), to_device(x)
    with engine(M, len(Ls), fs, M.METER_STCORR, sc_period=P, cap=4) as e:
        e.process_device_ragged(dev.data_ptr(), n, np.array(Ls, np.uint64), stride=x.shape[1])
        e.process_device(clean.data_ptr() + n * 8, P, stride=x.shape[1])
        a = snap(M, e)
    assert a["sc_n"] == 2
    for s, L in enumerate(Ls[:-1]):
        check_stcorr_stream(stcorr_oracle, fs, x[s], L, P, a["sc_corr"][s], a["sc_state"][s], a["sc_series"][s], a["sc_points"][s],
                            f"second piece: stream {s} L {L}", calls=[n])


# ---- NEEDLE ----------------------------------------------------------------------------------------------------------------------------

def check_needle_stream(O, kinds, xs, L, P, calls, rec, s, who):
    ends, _ = blocks_of(L, P, calls)
    assert int(rec["nd_points"][s]) == (len(ends) if P else 0), (who, "series_points")
    for k in kinds_of(kinds):
        level, state = rec[f"nd_level{k}"][s], rec[f"nd_state{k}"][s]
        if P:
            series = rec[f"nd_series{k}"][s]
            assert not series[len(ends):].any(), (who, k, "the row behind the stream's own points")
        if not ends:
            assert not level.any() and not state.any(), (who, k)
            continue
        want, want_st = oracle_run(O, k, xs[:L], ends, read_at=None if P else {len(ends) - 1})
        if P:
            assert same(series[:len(ends)], want), (who, k, "series", int(np.argmax((series[:len(ends)].view(np.uint32) != want.view(np.uint32)).any(axis=1))))
        assert same(level, want[-1]) and same(state, want_st[-1]), (who, k, level, want[-1], state, want_st[-1])


@pytest.mark.parametrize("chn,fs", [(2, 48000), (1, 44100)])
@pytest.mark.parametrize("P", [0, 16, 4800, 4801])
def test_needle_closed_streams_against_the_restatement(M, needle_oracle, chn, fs, P):
    Ls = lengths(P or 2400)
    extra = P
    x = nd_audio(16, chn, extra)
    cap = (T + extra) // P + 2 if P else 0
    dev, clean = to_device(poison(x, Ls)), to_device(x)
    with engine(M, 16, fs, M.METER_NEEDLE, chn, nd_period=P, cap=cap) as e, engine(M, 16, fs, M.METER_NEEDLE, chn, nd_period=P, cap=cap) as e2:
        kinds = e._kinds
        run_calls(e, dev.data_ptr(), x.shape[1], chn, CALLS, Ls)
        run_calls(e2, clean.data_ptr(), x.shape[1], chn, CALLS, Ls)
        assert_same(snap(M, e, P), snap(M, e2, P), "poison past the ends")
        if extra:
            e.process_device(clean.data_ptr() + T * chn * 4, extra, stride=x.shape[1])
        rec = snap(M, e)
    with needle_rate(fs):
        for s, L in enumerate(Ls):
            xs = x[s] if chn == 2 else x[s, :, 0]
            if s == 15:
                L, calls = L + extra, CALLS + ([extra] if extra else [])
            else:
                calls = CALLS
            check_needle_stream(needle_oracle, kinds, xs, L, P, calls, rec, s, f"chn {chn} fs {fs} P {P} stream {s} L {L}")


@pytest.mark.parametrize("calls", [[21, 40], [21, 1, 40], [21, 1, 1, 40], [270, 40]])
def test_needle_group_of_four_across_calls(M, needle_oracle, calls):
    """A call ends inside a group of four frames, and the next one ends a stream before that group is complete: the group's frames are
    dropped with the truncated block's j & ~3 rule although the chain had entered it — what stood in front of the group is kept from
    call to call.  (270: the group also lies across two staged chunks of 256 frames.)"""
    P, S = 16, 8
    total = sum(calls)
    first = sum(calls[:-1])
    Ls = [first + 1, first + 2, first + 3, first + 4, first + 5, first, calls[0] - 1, total]
    x = N.signal(S, 400)[:, :total + P]
    dev = to_device(poison(x, Ls))
    with engine(M, S, 48000, M.METER_NEEDLE, 2, nd_period=P, cap=64) as e:
        run_calls(e, dev.data_ptr(), x.shape[1], 2, calls, Ls)
        rec = snap(M, e)
    for s, L in enumerate(Ls[:7]):
        check_needle_stream(needle_oracle, ALL, x[s], L, P, calls, rec, s, f"calls {calls} stream {s} L {L}")


# ---- identity, frozen streams, the host form, layouts, combinations, refusals -------------------------------------------------------------

def both(M):
    return M.METER_STCORR | M.METER_NEEDLE


@pytest.mark.parametrize("fs,P_sc,P_nd", [(48000, 2400, 18), (44100, 0, 0)])
def test_identity_with_process_device(M, fs, P_sc, P_nd):
    """lengths all n_frames: bit for bit process_device; the open streams of a ragged batch: bit for bit those of a dense batch"""
    x = sc_audio(fs)
    dev = to_device(x)
    cap = T // 16 + 2
    Ls = lengths(P_sc or 2400)
    with engine(M, 16, fs, both(M), sc_period=P_sc, nd_period=P_nd, cap=cap) as dense, \
         engine(M, 16, fs, both(M), sc_period=P_sc, nd_period=P_nd, cap=cap) as full, \
         engine(M, 16, fs, both(M), sc_period=P_sc, nd_period=P_nd, cap=cap) as ragged:
        run_calls(dense, dev.data_ptr(), T, 2, CALLS)
        run_calls(full, dev.data_ptr(), T, 2, CALLS, [T] * 16)
        run_calls(ragged, dev.data_ptr(), T, 2, CALLS, Ls)
        a, b, c = snap(M, dense, P_nd), snap(M, full, P_nd), snap(M, ragged, P_nd)
        assert_same(a, b, "all lengths n_frames")
        for m, P in ((M.METER_STCORR, P_sc), (M.METER_NEEDLE, P_nd)):
            assert full.series_points(m).tolist() == [T // P if P else 0] * 16
        if P_sc:
            assert a["sc_n"] == T // P_sc
        assert not full.stream_frames()[1].any()
        strip = {k: v for k, v in a.items() if not k.endswith(("points",)) and np.ndim(v)}
        assert_same(rows(strip, [15]), rows({k: c[k] for k in strip}, [15]), "the open stream of the ragged batch")
        if not P_nd:                                                 # period 0: the needles' reading, read once
            for k in KINDS:
                la, lb = dense.needle_read(k), full.needle_read(k)
                assert same(la[0], lb[0]) and same(la[1], lb[1]), k


@pytest.mark.parametrize("fs", [48000, 44100])
def test_ragged_equals_tracks_on_a_tracks_mask(M, fs):
    S, chn = 16, 2
    x = np.stack([km_signal(T, 40 + s, fs) for s in range(S)]).astype(np.float32)
    dev = to_device(x)
    Ls = lengths(2400)
    meters = M.METER_KMETER | M.METER_DR14 | M.METER_TRUEPEAK
    with engine(M, S, fs, meters) as a, engine(M, S, fs, meters) as b:
        run_calls(a, dev.data_ptr(), T, chn, CALLS, Ls, entry="tracks")
        run_calls(b, dev.data_ptr(), T, chn, CALLS, Ls, entry="ragged")
        sa, sb = snap(M, a), snap(M, b)
        sa["dr14"], sb["dr14"] = bytes(a.dr14()), bytes(b.dr14())
        assert sa["dr14"] == sb["dr14"]
        del sa["dr14"], sb["dr14"]
        assert_same(sa, sb, "_ragged against _tracks")


def test_closed_streams_stay_frozen(M):
    fs, P = 48000, 2400
    x = sc_audio(fs, extra=9000)
    dev = to_device(x)
    Ls = lengths(P)
    shut = [s for s, L in enumerate(Ls) if L < T]
    with engine(M, 16, fs, both(M), sc_period=P, nd_period=P, cap=64) as e:
        run_calls(e, dev.data_ptr(), x.shape[1], 2, CALLS, Ls)
        a = snap(M, e)
        keep = [k for k in a if np.ndim(a[k]) and "series" not in k]     # (the series getters' reach grows with the lock-step count)
        base = dev.data_ptr() + T * 8
        e.process_device(base, 3000, stride=x.shape[1])
        e.process(np.ascontiguousarray(x[:, T + 3000:T + 6000]))
        e.process_device_ragged(base + 6000 * 8, 3000, np.full(16, 3000, np.uint64), stride=x.shape[1])
        b = snap(M, e)
        assert not np.array_equal(a["blob"], b["blob"])                           # (the cursors in it have moved: 57295 and 66295 mod P)
        a["blob"], b["blob"] = without_cursors(a["blob"], e), without_cursors(b["blob"], e)
        assert_same(rows({k: a[k] for k in keep}, shut), rows({k: b[k] for k in keep}, shut), "later calls")
        assert e.series_points(M.METER_STCORR)[15] == (T + 9000) // P and b["sc_n"] == (T + 9000) // P
        for k in ("sc_series",) + tuple(f"nd_series{k}" for k in KINDS):
            n = a[k].shape[1]
            assert np.array_equal(a[k][shut].view(np.uint32), b[k][shut][:, :n].view(np.uint32)), k
            for s in shut:
                assert not b[k][s][int(b["sc_points" if k == "sc_series" else "nd_points"][s]):].any(), (k, s)
        e.stcorr_reset()
        e.needle_reset()
        assert e.stream_frames()[1].tolist() == [L < T for L in Ls]              # the meters' resets reopen nothing
        assert not e.series_points(M.METER_STCORR).any() and not e.series_points(M.METER_NEEDLE).any()
        e.process_device(dev.data_ptr(), 5000, stride=x.shape[1])
        assert e.series_points(M.METER_STCORR).tolist() == [0 if L < T else 2 for L in Ls]
        corr, st = e.stcorr_read()
        assert not corr[shut].any() and not st[shut].any()                       # reset, and not touched since
        e.reset()                                                                # reopens every stream
        assert not e.stream_frames()[1].any() and not e.series_points(M.METER_NEEDLE).any()
        e.process_device(dev.data_ptr(), 5000, stride=x.shape[1])
        assert e.series_points(M.METER_STCORR).tolist() == [2] * 16 and e.stcorr_read()[1][:, 2:].all()


def test_host_form_equals_device_form_across_three_chunks(M):
    fs, P = 44100, 2205
    x = sc_audio(fs)
    dev = to_device(x)
    Ls = lengths(P)
    with engine(M, 16, fs, both(M), sc_period=P, nd_period=4801, cap=64) as d, engine(M, 16, fs, both(M), sc_period=P, nd_period=4801, cap=64) as h:
        h.set_host_chunk_bytes(6 * ((max(CALLS) + 1) & ~1) * 8)                  # six streams per chunk: 6 + 5 + 5 after evening out
        run_calls(d, dev.data_ptr(), T, 2, CALLS, Ls)
        run_calls(h, 0, T, 2, CALLS, Ls, host=x)
        assert_same(snap(M, d), snap(M, h), "process_ragged against process_device_ragged")


def test_pair_of_a_six_channel_frame(M):
    fs, P = 48000, 2400
    x = sc_audio(fs)
    wide = np.zeros((16, T, 6), np.float32)
    wide[:, :, 4:6] = x
    wide[:, :, :4] = np.float32(0.3) * x[:, ::-1, :].repeat(2, axis=2)           # something else in the other channels
    Ls = lengths(P)
    dx, dw = to_device(x), to_device(wide)
    with engine(M, 16, fs, M.METER_STCORR, sc_period=P, cap=64) as a, engine(M, 16, fs, M.METER_STCORR, sc_period=P, cap=64) as b:
        b.set_frame_layout(6, [4, 5])
        run_calls(a, dx.data_ptr(), T, 2, CALLS, Ls)
        run_calls(b, dw.data_ptr(), T, 6, CALLS, Ls)
        assert_same(snap(M, a), snap(M, b), "pair {4, 5} of 6-channel frames")


def test_beside_loudness_and_kmeter(M):
    fs, P = 48000, 2400
    x = sc_audio(fs)
    dev = to_device(x)
    Ls = lengths(P)
    with engine(M, 16, fs, M.METER_EBU | M.METER_TRUEPEAK | M.METER_KMETER | both(M), sc_period=P, nd_period=P, cap=64) as e, \
         engine(M, 16, fs, M.METER_EBU | M.METER_TRUEPEAK) as l, engine(M, 16, fs, M.METER_KMETER) as k, \
         engine(M, 16, fs, both(M), sc_period=P, nd_period=P, cap=64) as o:
        run_calls(e, dev.data_ptr(), T, 2, CALLS, Ls)
        run_calls(l, dev.data_ptr(), T, 2, CALLS, Ls, entry="lengths")
        run_calls(k, dev.data_ptr(), T, 2, CALLS, Ls, entry="tracks")
        run_calls(o, dev.data_ptr(), T, 2, CALLS, Ls)
        se, sl, sk, so = snap(M, e), snap(M, l), snap(M, k), snap(M, o)
    for key in ("out9", "hm", "hs", "tp"):
        assert np.ascontiguousarray(se[key]).tobytes() == np.ascontiguousarray(sl[key]).tobytes(), key
    for key in ("km_rms", "km_peak"):
        assert se[key].tobytes() == sk[key].tobytes(), key
    for key in so:
        if key != "blob":
            assert np.ascontiguousarray(se[key]).tobytes() == np.ascontiguousarray(so[key]).tobytes(), key


def test_a_batch_of_uniform_lengths(M, stcorr_oracle, needle_oracle):
    fs, P, S, n = 48000, 4800, 64, 96000
    rng = np.random.default_rng(21)
    Ls = rng.integers(0, n + 1, S).tolist()
    x = np.stack([N.stream(s, n + P) for s in range(S)])
    x[:, n:] = 0
    dev, clean = to_device(poison(x, Ls)), to_device(x)
    with engine(M, S, fs, both(M), sc_period=P, nd_period=P, cap=n // P + 3) as e:
        e.process_device_ragged(dev.data_ptr(), n, np.array(Ls, np.uint64), stride=n + P)
        e.process_device(clean.data_ptr() + n * 8, P, stride=n + P)
        a = snap(M, e)
    sampled = [s for s in range(0, S, 8) if Ls[s] < n]
    assert len(sampled) >= 6
    for s in sampled:
        who = f"batch: stream {s} L {Ls[s]}"
        check_stcorr_stream(stcorr_oracle, fs, x[s], Ls[s], P, a["sc_corr"][s], a["sc_state"][s], a["sc_series"][s], a["sc_points"][s], who, calls=[n])
        check_needle_stream(needle_oracle, ALL, x[s], Ls[s], P, [n], a, s, who)


def test_refusals_leave_the_engine_unchanged(M):
    fs, n = 48000, 6000
    st = np.ascontiguousarray(sc_audio(fs)[:4, :n])
    for meters, chn in ((M.METER_SPECTR30, 2), (M.METER_TPBALLIST, 2), (M.METER_SURROUND, 5), (M.METER_SCOPE, 2),
                        (M.METER_STCORR | M.METER_SCOPE, 2)):
        x = st if chn == 2 else np.ascontiguousarray(np.concatenate([st, st, st[:, :, :1]], axis=2))
        dev = to_device(x)
        with M.Engine(4, float(fs), meters, n_channels=chn) as e:
            e.process_device(dev.data_ptr(), n)
            before = e.state_export()
            f = np.array([n, 100, 0, n], np.uint64)
            assert M.lib.mtr_engine_process_device_ragged(e._h, dev.data_ptr(), n, n, f.ctypes.data, 0) == ERR_UNSUPPORTED, meters
            assert M.lib.mtr_engine_process_host_ragged(e._h, x.ctypes.data, n, n, f.ctypes.data) == ERR_UNSUPPORTED, meters
            assert e.state_export() == before and not e.stream_frames()[1].any()
    dev = to_device(st)
    with engine(M, 4, fs, both(M), sc_period=2400, nd_period=16, cap=8) as e:
        e.process_device(dev.data_ptr(), n)
        before, pts = snap(M, e), e.stream_frames()
        f = np.array([n, 100, n + 1, n], np.uint64)
        assert M.lib.mtr_engine_process_device_ragged(e._h, dev.data_ptr(), n, n, None, 0) == ERR_ARG
        assert M.lib.mtr_engine_process_device_ragged(e._h, dev.data_ptr(), n, n, f.ctypes.data, 0) == ERR_ARG
        assert M.lib.mtr_engine_process_host_ragged(e._h, st.ctypes.data, n, n, None) == ERR_ARG
        assert M.lib.mtr_engine_process_host_ragged(e._h, st.ctypes.data, n, n, f.ctypes.data) == ERR_ARG
        out = np.zeros(4, np.uint64)
        assert M.lib.mtr_engine_series_points(e._h, M.METER_KMETER, 0, 4, out.ctypes.data) == ERR_ARG
        assert M.lib.mtr_engine_series_points(e._h, M.METER_STCORR | M.METER_NEEDLE, 0, 4, out.ctypes.data) == ERR_ARG
        assert M.lib.mtr_engine_series_points(e._h, M.METER_STCORR, 2, 3, out.ctypes.data) == ERR_ARG
        assert_same(before, snap(M, e), "argument errors")
        assert e.stream_frames()[0].tolist() == pts[0].tolist() and not e.stream_frames()[1].any()
    with M.Engine(4, float(fs), M.METER_STCORR) as e:
        out = np.zeros(4, np.uint64)
        assert M.lib.mtr_engine_series_points(e._h, M.METER_NEEDLE, 0, 4, out.ctypes.data) == ERR_ARG      # a meter the engine lacks
