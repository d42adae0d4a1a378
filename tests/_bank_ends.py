"""What the tests of the 30-band bank's track lengths share (include/mtr_ends.h; the ENDS instantiations of k_bank): the shapes, the engine
under a programme of calls with ends, and per stream the two yardsticks — an engine WITHOUT a period that is fed stream s alone in calls of P
frames plus a last call of r frames (tests/_bank_series.dense extended by the truncated call: the existing path, bit for bit), and the
oracle's handle fed the same blocks (the contract of tests/_bank.py).  Test infrastructure.

Five streams of 30 bands are 150 lanes: wave 0 holds streams {0, 1, 2}, wave 1 {2, 3, 4}, wave 2 {4} and 42 dead lanes; streams 2 and 4
straddle two waves.  A call of 600 frames is four whole 128-frame chunks and a partial fifth; P = 100 puts block ends inside chunks."""
import numpy as np

import _bank as B
import _bank_series as BS

S, N, P = 5, 600, 100
FS = 48000.0
# frames[s] of the closing call, all of {0, 1, 2, 99, 100, 101, 127, 128, 129, 256, 257, 599, 600} between them
ENDS = {
    # wave 0: three different ends, one of them 0 beside the open stream 1; wave 1: all of its streams end early (one untouched); wave 2 alike
    "mixed": [129, 600, 0, 257, 99],
    # every wave's streams end early, inside the first chunk: r = 1, 2, 0 (a block's end), 1, 27
    "early": [1, 2, 100, 101, 127],
    # a chunk's end, two chunks' end, one frame short of the call, the whole call; wave 2 has nothing to do at all
    "edges": [128, 256, 599, 600, 0],
}


def batch(T=N, first=0):
    """[S, T, 2]: streams first .. first + S of tests/_bank.py's inputs"""
    return np.stack([B.stream_input(first + s, T) for s in range(S)])


def expected_points(fill, period, n_frames, frames):
    """mtr_series_cut restated: whole blocks + the truncated one of a stream that takes `frames` of a call of n_frames which starts `fill`
    frames into a block -> (whole, partial)"""
    closes = 0 < frames < n_frames
    tot = fill + frames
    return (tot // period if period else 0), int(closes and (period == 0 or tot % period != 0))


def cuts_of(total, period, calls=None):
    """The spectrum_runs of a stream that has `total` frames: blocks of `period` and the truncated one; period 0: the calls (frames per
    call), the last one cut where the stream ends."""
    if period:
        return [period] * (total // period) + ([total % period] if total % period else [])
    out, left = [], total
    for n in calls:
        if left <= 0:
            break
        out.append(min(n, left))
        left -= n
    return out


def _collect(reads):
    if not reads:
        return {k: np.zeros((0, B.NBANDS), np.float32) for k in BS.KEYS}
    return {k: np.stack([r[k] for r in reads]) for k in BS.KEYS}


_YARD, _ORC = {}, {}


# the bank's sections of a stream's entry of the state blob — z, val, max, the dither parity — the last ones of a SPECTR30 engine without a period
BANK_BLOB_BYTES = B.NBANDS * (12 * 8 + 4 + 4) + 4


def yard(M, x, cuts, mode=BS.HOLD, mono=False, speed=B.SPEED, key=None, blob=False):
    """One stream [T, 2] through a ONE-stream engine without a period, one call per entry of `cuts`, mtr_engine_spectrum read after each
    (MTR_SPECTR_PEAK_BLOCK: mtr_engine_spectr_reset_peak after each read) -> (dict of [len (cuts), 30], the final mtr_engine_spectrum of
    the stream as dict of [30]).  key: cache the answer under it (a reference is computed once and shared).  blob: the engine's
    mtr_engine_state_export as a third answer."""
    full = None if key is None else (key, tuple(cuts), mode, mono, speed)
    if full in _YARD:
        return _YARD[full]
    xs = BS.feed(mono, x[None])
    with M.Engine(1, FS, M.METER_SPECTR30, n_channels=1 if mono else 2) as e:
        if speed is not None:
            e.spectr_set_speed(speed)
        reads, pos = [], 0
        for n in cuts:
            e.process(np.ascontiguousarray(xs[:, pos:pos + n]))
            pos += n
            reads.append({k: v[0] for k, v in e.spectrum().items()})
            if mode == BS.BLOCK:
                e.spectr_reset_peak()
        out = (_collect(reads), {k: v[0] for k, v in e.spectrum().items()}) + ((e.state_export(),) if blob else ())
    if full is not None:
        _YARD[full] = out
    return out


def oracle_cuts(oracle, x, cuts, mode=BS.HOLD, mono=False, speed=B.SPEED, key=None):
    """The same through the oracle's handle: one run () per entry of `cuts`, read after each (BLOCK: reset_peak () after each read)
    -> (dict of [len (cuts), 30], the handle's last reading)"""
    full = None if key is None else (key, tuple(cuts), mode, mono, speed)
    if full in _ORC:
        return _ORC[full]
    h = oracle.spectr_stream(FS, 1 if mono else 2)
    if speed is not None:
        h.set_speed(speed)
    x = BS.one(mono, x)
    reads, pos = [], 0
    for n in cuts:
        reads.append(h.run(x[pos:pos + n]))
        pos += n
        if mode == BS.BLOCK:
            h.reset_peak()
    out = (_collect(reads), h.read())
    if full is not None:
        _ORC[full] = out
    return out


def device_rows(x, mono, stride, frames=None):
    """[S, n, 2] -> a flat float32 buffer of [S][stride] frames, NaN behind the call's n frames; frames: NaN behind every stream's own end
    as well (the poison)"""
    xs = BS.feed(mono, x).copy()
    n = xs.shape[1]
    if frames is not None:
        for s, f in enumerate(frames):
            xs[s, int(f):] = np.nan
    rows = np.full((xs.shape[0], stride) + xs.shape[2:], np.nan, np.float32)
    rows[:, :n] = xs
    return rows


def through(M, x, calls, period=0, cap=16, mode=BS.HOLD, mono=False, pad=0, speed=B.SPEED, host=False, poison=False, meters=None,
            chunk_streams=None, after=None):
    """x [S, T, 2] through one engine: calls = [(n, frames or None)], frames [S] the ends of an _ends call, None a plain process call.
    pad: stride - n of the device buffers.  host: process_ends / process instead of the device forms (chunk_streams: streams per view).
    after (e): called behind the last call, its answer returned under "after".  -> dict(spectrum, series, n_points, dropped, points,
    frames, closed, blob)"""
    import torch
    n_s = x.shape[0]
    with M.Engine(n_s, FS, M.METER_SPECTR30 if meters is None else meters, n_channels=1 if mono else 2) as e:
        if speed is not None:
            e.spectr_set_speed(speed)
        if period:
            e.spectr_set_period(period, cap, mode)
        pos = 0
        for n, frames in calls:
            seg = x[:, pos:pos + n]
            pos += n
            if host:
                if chunk_streams:
                    # (a staged row: the call's frames rounded up to 16 bytes, as the host path lays its chunks out)
                    e.set_host_chunk_bytes(chunk_streams * ((n + 3) // 4 * 4 * 4 if mono else (n + 1) // 2 * 2 * 8))
                xs = BS.feed(mono, seg)
                e.process(xs) if frames is None else e.process_ends(xs, frames)
                continue
            d = torch.from_numpy(device_rows(seg, mono, n + pad, frames if poison else None)).cuda()
            if frames is None:
                e.process_device(d.data_ptr(), n, n + pad)
            else:
                e.process_device_ends(d.data_ptr(), n, frames, n + pad)
            e.sync()
            del d
        out = dict(spectrum=e.spectrum(), points=e.spectr_points(), blob=e.state_export(), series=None, n_points=0, dropped=0)
        out["frames"], out["closed"] = e.stream_frames()
        if period:
            out["series"], out["n_points"], out["dropped"] = e.spectr_series()
        if after:
            out["after"] = after(e)
        return out


def same_result(a, b):
    """two answers of through (): bit for bit in everything it returns"""
    ok = BS.same(a["spectrum"], b["spectrum"]) and a["blob"] == b["blob"] and (a["n_points"], a["dropped"]) == (b["n_points"], b["dropped"])
    ok = ok and a["points"].tolist() == b["points"].tolist() and a["frames"].tolist() == b["frames"].tolist() and a["closed"].tolist() == b["closed"].tolist()
    if a["series"] is not None or b["series"] is not None:
        ok = ok and BS.same(a["series"], b["series"])
    return bool(ok)
