"""What the bank's reading-series tests share (include/mtr_spectr.h): the oracle's call-by-call handle fed in blocks of P, the engine
under a programme of calls, and the engine WITHOUT a period fed calls of exactly P frames — the existing path, the bit-for-bit yardstick
of the new one.  Test infrastructure."""
import numpy as np

import _bank as B

KEYS = ("val", "max", "val_db", "max_db")
HOLD, BLOCK = 0, 1         # MTR_SPECTR_PEAK_*


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    """two readings or two series, bit for bit in all four keys"""
    return all(a[k].shape == b[k].shape and np.array_equal(bits(a[k]), bits(b[k])) for k in KEYS)


def feed(mono, x):
    """[S, T, 2] -> what an engine of that width takes (mono: the left channel)"""
    return np.ascontiguousarray(x[:, :, 0]) if mono else np.ascontiguousarray(x)


def one(mono, x):
    """[T, 2] -> what the oracle handle of that width takes"""
    return np.ascontiguousarray(x[:, 0]) if mono else x


def blocks_of(T, P, first=None):
    """the blocks of P frames in T (first: the length of the first one, for a series that is cut elsewhere); the open rest is no block"""
    out, pos = [], 0
    n = P if first is None else first
    while pos + n <= T:
        out.append(n)
        pos += n
        n = P
    return out


def oracle_series(oracle, x, P, mode=HOLD, speed=B.SPEED, mono=False, fs=48000.0, first=None, between=None):
    """One stream [T, 2] through the oracle's handle in blocks of P, read after each -> dict of [points, 30] arrays.  BLOCK: the handle
    gets reset_peak () after each read.  between (handle, k): called in front of block k (controls)."""
    h = oracle.spectr_stream(fs, 1 if mono else 2)
    if speed is not None:
        h.set_speed(speed)
    x = one(mono, x)
    out, pos = [], 0
    for k, n in enumerate(blocks_of(len(x), P, first)):
        if between:
            between(h, k)
        out.append(h.run(x[pos:pos + n]))
        pos += n
        if mode == BLOCK:
            h.reset_peak()
    return {k: np.stack([r[k] for r in out]) if out else np.zeros((0, B.NBANDS), np.float32) for k in KEYS}


_REF = {}


def reference(oracle, s, T, P, mode, mono, speed=B.SPEED):
    """oracle_series of stream s of these tests' batches: computed once, the same whatever the batch's size"""
    key = (s, T, P, mode, mono, speed)
    if key not in _REF:
        _REF[key] = oracle_series(oracle, B.stream_input(s, T), P, mode, speed, mono)
    return _REF[key]


def stack(series):
    """the series of S streams -> one dict of [S, points, 30] arrays"""
    return {k: np.stack([r[k] for r in series]) for k in KEYS}


def through(M, x, P, calls, cap=64, mode=HOLD, speed=B.SPEED, mono=False, process=None, after=None, fs=48000.0):
    """x [S, T, 2] through an engine with period P under `calls` (frames per call) -> (series dict [S, kept, 30], n_points, dropped,
    the final mtr_engine_spectrum).  process (e, frames a .. b): how a call is made (the host path); after (e, i): behind call i."""
    xs = feed(mono, x)
    with M.Engine(x.shape[0], fs, M.METER_SPECTR30, n_channels=1 if mono else 2) as e:
        if speed is not None:
            e.spectr_set_speed(speed)
        e.spectr_set_period(P, cap, mode)
        pos = 0
        for i, n in enumerate(calls):
            if process:
                process(e, pos, pos + n)
            else:
                e.process(np.ascontiguousarray(xs[:, pos:pos + n]))
            pos += n
            if after:
                after(e, i)
        ser, n_points, dropped = e.spectr_series()
        return ser, n_points, dropped, e.spectrum()


def dense(M, x, P, mode=HOLD, speed=B.SPEED, mono=False, fs=48000.0):
    """The engine as it was — no period — fed calls of exactly P frames with mtr_engine_spectrum after each (and, BLOCK,
    mtr_engine_spectr_reset_peak after each read) -> dict of [S, points, 30]"""
    xs = feed(mono, x)
    with M.Engine(x.shape[0], fs, M.METER_SPECTR30, n_channels=1 if mono else 2) as e:
        if speed is not None:
            e.spectr_set_speed(speed)
        out, pos = [], 0
        for n in blocks_of(xs.shape[1], P):
            e.process(np.ascontiguousarray(xs[:, pos:pos + n]))
            pos += n
            out.append(e.spectrum())
            if mode == BLOCK:
                e.spectr_reset_peak()
        if not out:
            return {k: np.zeros((x.shape[0], 0, B.NBANDS), np.float32) for k in KEYS}
        return {k: np.stack([r[k] for r in out], 1) for k in KEYS}
