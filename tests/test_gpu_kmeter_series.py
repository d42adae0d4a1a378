"""The K-meter's reading series (mtr_engine_kmeter_set_period / _period / _series, k_kmeter_blocks + k_kmeter_walk in mtr_kmeter.hip)
against the restatement of jmeters/kmeterdsp.cc (oracle mo_kmeter_*, bit-identical to the reference object:
tests/test_needle_oracle_vs_ref.py), fed exactly each stream's blocks of P frames with a read after each.

Tolerances are those of tests/test_gpu_kmeter.py and tests/test_gpu_surround.py: rms within 1e-5 * max (want, 1e-3) — the filter sums are
re-associated and carried in double — and the peak with its hold / fall-back bit for bit (uint32 views); where the restatement's rms is
0 or not finite, the rms bit for bit too.  The signal is tests/test_gpu_kmeter.py's: a peak that is held and then falls back."""
import ctypes as C
import functools

import numpy as np
import pytest

from test_gpu_kmeter import Kmeter, signal

pytestmark = pytest.mark.gpu
F = C.c_float
ERR_ARG, ERR_UNSUPPORTED, ERR_STATE = -1, -2, -7
OPEN_BYTES = 80                                                # mtr_kmeter_open: 16 bytes of header + 2 x 32 of carry


@pytest.fixture(scope="module")
def M():
    import meters.lv2_amd as m
    assert (m.engine.ERR_ARG, m.engine.ERR_UNSUPPORTED, m.engine.ERR_STATE) == (ERR_ARG, ERR_UNSUPPORTED, ERR_STATE)
    return m


@pytest.fixture(scope="module")
def lib(oracle):
    L = oracle.lib
    L.mo_kmeter_init.argtypes = [C.POINTER(Kmeter), F]
    L.mo_kmeter_process.argtypes = [C.POINTER(Kmeter), C.POINTER(F), C.c_int]
    L.mo_kmeter_read.argtypes = [C.POINTER(Kmeter), C.POINTER(F), C.POINTER(F)]
    return L


@functools.lru_cache(maxsize=None)
def audio(fs, T, S=5):
    x = np.stack([signal(T, 300 + s, fs) for s in range(S)])
    x.setflags(write=False)
    return x


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a) if a.dtype == np.float32 else a, bits(b) if b.dtype == np.float32 else b)


def restate(lib, ch, fs, P, truncated=False):
    """(rms [n], peak [n]) of a host that calls process (p, P) + read on the consecutive blocks of ch; truncated: one last
    process (p, len % P) + read on what is left"""
    k = Kmeter()
    lib.mo_kmeter_init(C.byref(k), fs)
    ch = np.ascontiguousarray(ch, np.float32)
    ends = [P * (i + 1) for i in range(len(ch) // P)]
    if truncated and len(ch) % P:
        ends.append(len(ch))
    rms, peak, pos = [], [], 0
    for e in ends:
        blk = np.ascontiguousarray(ch[pos:e])
        lib.mo_kmeter_process(C.byref(k), blk.ctypes.data_as(C.POINTER(F)), e - pos)
        a, b = F(), F()
        lib.mo_kmeter_read(C.byref(k), C.byref(a), C.byref(b))
        rms.append(a.value)
        peak.append(b.value)
        pos = e
    return np.array(rms, np.float32), np.array(peak, np.float32)


def restate_batch(lib, x, fs, P):
    """[S, n, C] x 2 for x [S, T, C]"""
    r = [[restate(lib, x[s, :, c], fs, P) for c in range(x.shape[2])] for s in range(x.shape[0])]
    return (np.stack([np.stack([r[s][c][i] for c in range(x.shape[2])], -1) for s in range(x.shape[0])]) for i in (0, 1))


def check(rms, peak, want_rms, want_peak, what=""):
    """the issue's rule, point by point"""
    rms, peak, want_rms, want_peak = (np.asarray(v, np.float32) for v in (rms, peak, want_rms, want_peak))
    assert rms.shape == want_rms.shape and peak.shape == want_peak.shape, (what, rms.shape, want_rms.shape)
    assert np.array_equal(bits(peak), bits(want_peak)), (what, "peak", np.argwhere(bits(peak) != bits(want_peak))[:4])
    exact = ~np.isfinite(want_rms) | (want_rms == 0)
    assert np.array_equal(bits(rms)[exact], bits(want_rms)[exact]), (what, "rms where the restatement's is 0 or not finite")
    with np.errstate(invalid="ignore"):
        err = np.abs(rms - want_rms)[~exact]
    tol = 1e-5 * np.maximum(want_rms[~exact], 1e-3)
    assert (err <= tol).all(), (what, "rms", float((err / tol).max()))


def cuts_for(P, T):
    """call lengths that cut: inside a block, inside a group (1, 3, 1023), exactly on a block end, inside the block's last frames (the
    dropped ones where P mod 4 != 0) and on the end again, across several blocks at once, a repeat of the same length, the rest"""
    seq = [P // 2 + 1, 1, 3, 1023]
    seq.append(P - sum(seq) % P)
    seq += [P - 1, 1, 2 * P + 5, 2 * P + 5, P + 2, P + 2]
    out, pos = [], 0
    for n in seq:
        n = min(n, T - pos)
        if n <= 0:
            break
        out.append(n)
        pos += n
    if pos < T:
        out.append(T - pos)
    assert sum(out) == T
    return out


def shaped(x, chn=2):
    """a writable contiguous copy, [S, T, 2] or (mono) [S, T]"""
    return np.array(x if chn == 2 else x[:, :, 0], np.float32, order="C")


def run(M, x, fs, P, calls, cap=1024, chn=2, meters=None, Ls=None, reads=False, setup=None, keep=None):
    """the device call over x [S, T, C]: the series, the counts, (rms, peak) of kmeter_read after every call (reads), the state blob"""
    import torch
    S = x.shape[0]
    dev = torch.from_numpy(shaped(x, chn)).cuda()
    out = {"reads": []}
    with M.Engine(S, fs, meters or M.METER_KMETER, n_channels=chn) as e:
        if setup:
            setup(e)
        e.kmeter_set_period(P, cap)
        pos, done = 0, np.zeros(S, bool)
        for n in calls:
            ptr = dev.data_ptr() + pos * chn * 4
            if Ls is None:
                e.process_device(ptr, n, stride=x.shape[1])
            else:
                f = np.where(done, 0, np.clip(np.asarray(Ls, np.int64) - pos, 0, n)).astype(np.uint64)
                done |= f < n
                e.process_device_ragged(ptr, n, f, stride=x.shape[1])
            pos += n
            if reads:
                a, b = e.kmeter_read(), e.kmeter_read()
                assert same(a[0], b[0]) and same(a[1], b[1]), "two reads in a row differ"
                out["reads"].append((pos, a[0][:, :chn].copy(), a[1][:, :chn].copy()))
        out["rms"], out["peak"], out["n"], out["dropped"] = e.kmeter_series()
        out["read"] = tuple(v[:, :chn].copy() for v in e.kmeter_read())
        out["points"] = e.series_points(M.METER_KMETER)
        hdr = 2 * e.state_bytes(1) - e.state_bytes(2)
        out["blob"] = np.stack([np.frombuffer(e.state_export(s, 1), np.uint8)[hdr:] for s in range(S)])
        if keep:
            keep(e, out)
    del dev
    return out


def period_of(kind, fs):
    return {"min": int(fs) // 20, "4800": 4800, "4803": 4803, "long": 100003, "long twice": 80003}[kind]


@pytest.mark.parametrize("fs", [48000.0, 44100.0])
@pytest.mark.parametrize("chn", [2, 1])
@pytest.mark.parametrize("kind", ["min", "4800", "4803", "long", "long twice"])
def test_series_matches_the_restatement_however_the_calls_cut(M, lib, fs, chn, kind):
    # the kernel's chunk is 32768 frames: 100003 is four pieces and 3 frames dropped, and 4 s hold one such block.  80003 is three pieces
    # and 3 frames dropped, and 4 s hold two: the second starts behind the first's dropped frames, its groups on another alignment, and
    # carries (z1, z2), the held peak and its count through a block of several pieces
    P = period_of(kind, fs)
    T = int(fs) * 4 if kind.startswith("long") else int(fs) * 2 + 77
    x = audio(fs, T)[:, :, :chn]
    want_rms, want_peak = restate_batch(lib, x, fs, P)
    n = T // P
    cut = run(M, x, fs, P, cuts_for(P, T), chn=chn, reads=True)
    one = run(M, x, fs, P, [T], chn=chn)
    for what, got in (("cut", cut), ("one call", one)):
        assert got["n"] == n and got["dropped"] == 0 and (got["points"] == n).all(), what
        check(got["rms"], got["peak"], want_rms, want_peak, what)
    assert same(cut["peak"], one["peak"])                      # cuts do not matter: the peak series bit for bit
    # kmeter_read after every call: the last completed block's, 0.0f before the first
    for pos, rms, peak in cut["reads"]:
        k = pos // P
        assert same(rms, cut["rms"][:, k - 1] if k else np.zeros_like(rms)) and same(peak, cut["peak"][:, k - 1] if k else np.zeros_like(peak)), pos
    # a capacity smaller than the points: the first ones are kept, the rest counted
    if n >= 3:
        few = run(M, x, fs, P, cuts_for(P, T), cap=n - 2, chn=chn)
        assert few["n"] == n and few["dropped"] == 2 and same(few["rms"], cut["rms"][:, :n - 2]) and same(few["peak"], cut["peak"][:, :n - 2])
        assert same(few["read"][0], cut["read"][0]) and same(few["read"][1], cut["read"][1])


def test_streams_do_not_interfere(M):
    fs, P = 48000.0, 4803
    T = int(fs) * 2
    x = audio(fs, T, 7)
    calls = cuts_for(P, T)
    wins = {}

    def windows(e, out):
        for first, count in ((0, 1), (2, 3), (6, 1), (3, 4)):
            wins[first, count] = e.kmeter_series(first, count)

    a = run(M, x, fs, P, calls, keep=windows)
    b = run(M, x, fs, P, calls)
    for k in ("rms", "peak", "blob"):
        assert same(a[k], b[k]), k                             # two runs are bit-identical
    for (first, count), (rms, peak, n, d) in wins.items():
        assert n == a["n"] and d == 0 and same(rms, a["rms"][first:first + count]) and same(peak, a["peak"][first:first + count])
    perm = np.array([4, 0, 6, 2, 5, 1, 3])
    p = run(M, np.ascontiguousarray(x[perm]), fs, P, calls)
    for k in ("rms", "peak", "blob"):
        assert same(p[k], a[k][perm]), k                       # a stream's results do not depend on its slot


@pytest.mark.parametrize("P", [4800, 4803])
def test_samples_that_are_not_finite(M, lib, P):
    fs = 48000.0
    T = int(fs) * 2
    clean = audio(fs, T, 8)
    x = clean.copy()
    Lg = P - P % 4
    spots = {}                                                 # stream -> (frame, channel, value): in block 3 of the stream
    for s, (off, v) in enumerate([(P // 2 + 1, np.nan), (P // 2 + 2, np.inf), (P // 2 + 3, 1e30), (Lg - 1, np.nan), (Lg - 1, np.inf), (Lg - 1, 1e30),
                                  (P - 1, np.inf)]):
        spots[s] = (3 * P + off, s % 2, v)                     # (P mod 4 == 0 has no dropped frames: P - 1 is then the last counted one again)
        x[s, 3 * P + off, s % 2] = v
    if P % 4:
        x[6, 3 * P + Lg, 0] = np.nan                           # ... and the dropped frames of that block hold all three kinds
        x[6, 3 * P + Lg + 1, 1] = 1e30
    calls = cuts_for(P, T)
    got, ref = run(M, x, fs, P, calls), run(M, clean, fs, P, calls)
    want_rms, want_peak = restate_batch(lib, x, fs, P)
    check(got["rms"], got["peak"], want_rms, want_peak)
    # every other stream, the other channel and every block before the sample are those of the run without it
    assert same(got["rms"][7], ref["rms"][7]) and same(got["peak"][7], ref["peak"][7]) and same(got["blob"][7], ref["blob"][7])
    for s, (f, c, v) in spots.items():
        assert same(got["rms"][s, :3], ref["rms"][s, :3]) and same(got["peak"][s, :3], ref["peak"][s, :3]), s
        assert same(got["rms"][s, :, 1 - c], ref["rms"][s, :, 1 - c]) and same(got["peak"][s, :, 1 - c], ref["peak"][s, :, 1 - c]), s
    if P % 4:                                                  # what lies in the dropped frames alone changes nothing at all
        assert same(got["rms"][6], ref["rms"][6]) and same(got["peak"][6], ref["peak"][6]) and same(got["blob"][6], ref["blob"][6])


def test_every_way_in_is_the_device_call(M):
    fs, P, S = 48000.0, 4803, 6
    T = int(fs) * 2
    calls = cuts_for(P, T)
    x = audio(fs, T, S)
    dev = run(M, x, fs, P, calls)

    def via(feed, xs=x, S=S, setup=None):
        with M.Engine(S, fs, M.METER_KMETER) as e:
            if setup:
                setup(e)
            e.kmeter_set_period(P, 1024)
            pos = 0
            for n in calls:
                feed(e, xs[:, pos:pos + n])
                pos += n
            return e.kmeter_series() + e.kmeter_read()

    def equal(got, want):
        return all(same(a, b) if isinstance(a, np.ndarray) else a == b for a, b in zip(got, want))

    want = (dev["rms"], dev["peak"], dev["n"], dev["dropped"], *dev["read"])
    # the host path across three chunks
    assert equal(via(lambda e, b: e.process(np.ascontiguousarray(b)), setup=lambda e: e.set_host_chunk_bytes(2 * max(calls) * 8)), want)
    # a pair {4, 5} of 6-channel frames
    wide = np.random.default_rng(5).uniform(-1, 1, (S, T, 6)).astype(np.float32)
    wide[:, :, 4:6] = x
    assert equal(via(lambda e, b: e.process(np.ascontiguousarray(b)), xs=wide, setup=lambda e: e.set_frame_layout(6, [4, 5])), want)
    # S16 PCM: the device call on the decoded samples
    pcm = np.round(x * 32767).astype(np.int16)
    dec = run(M, M.engine.pcm_decode(M.PCM_S16, pcm), fs, P, calls)
    assert equal(via(lambda e, b: e.process_pcm(np.ascontiguousarray(b)), xs=pcm), (dec["rms"], dec["peak"], dec["n"], dec["dropped"], *dec["read"]))
    # the planar LV2 block path (one stream)
    got = via(lambda e, b: e.process_planar([b[0, :, 0], b[0, :, 1]]), xs=x[:1], S=1)
    assert equal(got, (dev["rms"][:1], dev["peak"][:1], dev["n"], dev["dropped"], dev["read"][0][:1], dev["read"][1][:1]))


def test_beside_other_meters(M):
    fs, S = 48000.0, 5
    T = int(fs) * 2
    x = audio(fs, T, S)
    calls = cuts_for(4803, T)
    all5 = M.METER_EBU | M.METER_TRUEPEAK | M.METER_KMETER | M.METER_STCORR | M.METER_NEEDLE
    kinds = M.NEEDLE_VU | M.NEEDLE_IEC1

    def others(e):
        e.integr_start()
        e.stcorr_set_period(2400, 256)
        e.needle_configure(kinds, 3000, 256)

    def getters(e, out):
        hm, hs = e.histograms()
        out["other"] = [e.out9(), e.truepeak(), hm, hs, *e.stcorr_read(), *e.stcorr_series()]
        for k in (M.NEEDLE_VU, M.NEEDLE_IEC1):
            out["other"] += [*e.needle_series(k), *e.needle_read(k)]

    with_p = run(M, x, fs, 4803, calls, meters=all5, setup=others, keep=getters)
    without = run(M, x, fs, 0, calls, meters=all5, setup=others, keep=getters)
    alone = run(M, x, fs, 4803, calls)
    assert len(with_p["other"]) == len(without["other"])
    for i, (a, b) in enumerate(zip(with_p["other"], without["other"])):
        assert same(a, b) if isinstance(a, np.ndarray) else a == b, i
    for k in ("rms", "peak"):
        assert same(with_p[k], alone[k]), k
    assert with_p["n"] == alone["n"] == T // 4803 and same(with_p["read"][0], alone["read"][0]) and same(with_p["read"][1], alone["read"][1])


# ---- ragged batches ---------------------------------------------------------------------------------------------------------------------
RP = 4800
RCALLS = [1002, 13400, 1, 81597]                               # ends 1002, 14402, 14403, 96000; the first stops at frame 1002 of its block: an open group
RT = sum(RCALLS)
RL = [0, RT, 9600, 9601, 9603, 9605, 14399, 1003, 50000, 1002, 14401, 14404, 1, 700, 4096, 1001]


def ragged_truncates(L):
    """the stream's last block is a truncated one: it ends inside a call and inside a block (an end on a call's end is closed with 0 frames by
    the next call, untouched: its block stays open)"""
    return L % RP != 0 and L < RT and L not in np.cumsum(RCALLS).tolist()


@pytest.fixture(scope="module")
def ragged(M):
    x = audio(48000.0, RT, 16)
    return x, run(M, x, 48000.0, RP, RCALLS, Ls=RL)


def test_ragged_streams_match_the_restatement_fed_their_own_frames(M, lib, ragged):
    x, got = ragged
    for s, L in enumerate(RL):
        tr = ragged_truncates(L)
        want = [restate(lib, x[s, :L, c], 48000.0, RP, truncated=tr) for c in range(2)]
        n = L // RP + (1 if tr else 0)
        assert got["points"][s] == n == len(want[0][0]), (s, L)          # series_points: the restatement's process () count
        check(got["rms"][s, :n], got["peak"][s, :n], np.stack([w[0] for w in want], -1), np.stack([w[1] for w in want], -1), (s, L))
        assert not got["rms"][s, n:].any() and not got["peak"][s, n:].any(), (s, L)   # 0.0f behind the stream's own points
        last = (got["rms"][s, n - 1], got["peak"][s, n - 1]) if n else (np.zeros(2, np.float32),) * 2
        assert same(got["read"][0][s], last[0]) and same(got["read"][1][s], last[1]), (s, L)
    assert got["n"] == RT // RP


def test_ragged_ignores_what_lies_behind_an_end(M, ragged):
    x, got = ragged
    y = x.copy()
    for s, L in enumerate(RL):
        y[s, L:, 0], y[s, L + 1:, 1] = np.nan, np.inf
        y[s, L:L + 1, 1] = 1e30
    p = run(M, y, 48000.0, RP, RCALLS, Ls=RL)
    for k in ("rms", "peak", "blob", "points"):
        assert same(p[k], got[k]), k
    assert same(p["read"][0], got["read"][0]) and same(p["read"][1], got["read"][1])


def test_ragged_with_full_lengths_is_the_dense_call(M, ragged):
    x, _ = ragged
    a, b = run(M, x, 48000.0, RP, RCALLS, Ls=[RT] * 16, reads=True), run(M, x, 48000.0, RP, RCALLS, reads=True)
    for k in ("rms", "peak", "blob", "points"):
        assert same(a[k], b[k]), k
    assert a["n"] == b["n"] and all(same(u[1], v[1]) and same(u[2], v[2]) for u, v in zip(a["reads"], b["reads"]))
    # ... and the open streams of the ragged batch are the dense batch's
    for s, L in enumerate(RL):
        if L == RT:
            assert same(ragged[1]["rms"][s], b["rms"][s]) and same(ragged[1]["peak"][s], b["peak"][s]) and same(ragged[1]["blob"][s], b["blob"][s])


def test_closed_streams_stay_frozen_and_only_the_engine_reset_reopens(M, ragged):
    import torch
    x, got = ragged
    dev = torch.from_numpy(shaped(x)).cuda()
    closed = np.array([L < RT for L in RL])
    with M.Engine(16, 48000.0, M.METER_KMETER) as e:
        e.kmeter_set_period(RP, 64)
        pos, done = 0, np.zeros(16, bool)
        for n in RCALLS:
            f = np.where(done, 0, np.clip(np.array(RL) - pos, 0, n)).astype(np.uint64)
            done |= f < n
            e.process_device_ragged(dev.data_ptr() + pos * 8, n, f, stride=RT)
            pos += n
        assert (e.stream_frames()[1] == closed).all()
        e.process_device(dev.data_ptr(), 10000, stride=RT)               # a later dense call: the LEN kernels with end 0
        rms, peak, n, d = e.kmeter_series()
        assert n == RT // RP + 2
        k = got["rms"].shape[1]
        assert same(rms[closed][:, :k], got["rms"][closed]) and same(peak[closed][:, :k], got["peak"][closed]) and not rms[closed][:, k:].any()
        assert same(e.series_points(M.METER_KMETER)[closed], got["points"][closed])
        hdr = 2 * e.state_bytes(1) - e.state_bytes(2)
        for s in np.flatnonzero(closed):                                 # (the entry's first 16 bytes of the last section are the lock-step cursors)
            a = np.frombuffer(e.state_export(int(s), 1), np.uint8)[hdr:]
            assert same(a[:-OPEN_BYTES], got["blob"][s][:-OPEN_BYTES]) and same(a[-OPEN_BYTES + 16:], got["blob"][s][-OPEN_BYTES + 16:]), s
        assert (rms[~closed][:, k:k + 2] != 0).all()
        e.kmeter_reset()                                                 # reopens nothing, empties the series, keeps P
        assert (e.stream_frames()[1] == closed).all() and e.kmeter_period() == (RP, 64) and e.kmeter_series()[2] == 0
        assert not e.series_points(M.METER_KMETER).any() and not e.kmeter_read()[0].any()
        e.reset()
        assert not e.stream_frames()[1].any() and e.kmeter_period() == (RP, 64)
        e.process_device(dev.data_ptr(), RP, stride=RT)
        assert e.kmeter_series()[2] == 1 and (e.series_points(M.METER_KMETER) == 1).all()
    del dev


# ---- the state blob, refusals, a known answer -------------------------------------------------------------------------------------------
def test_state_travels_mid_block_and_mid_group(M):
    import torch
    fs, P, S = 48000.0, 4803, 5
    T = int(fs) * 2
    x = audio(fs, T, S)
    cut = 2 * P + 1001                                                  # 1001 frames into a block: one frame into a group
    straight = run(M, x, fs, P, [cut, T - cut])
    dev = torch.from_numpy(shaped(x)).cuda()
    with M.Engine(S, fs, M.METER_KMETER) as e:
        e.kmeter_set_period(P, 64)
        e.process_device(dev.data_ptr(), cut, stride=T)
        blob = e.state_export()
        plain = M.Engine(S, fs, M.METER_KMETER)
        assert len(blob) == plain.state_bytes(S) + S * OPEN_BYTES == e.state_bytes(S)
        plain.close()
    with M.Engine(S, fs, M.METER_KMETER) as e:
        e.kmeter_set_period(P, 64)
        assert e.state_import(blob) == S
        e.process_device(dev.data_ptr() + cut * 8, T - cut, stride=T)
        rms, peak, n, d = e.kmeter_series()
        assert n == T // P - 2 and same(rms, straight["rms"][:, 2:]) and same(peak, straight["peak"][:, 2:])
        hdr = 2 * e.state_bytes(1) - e.state_bytes(2)
        assert same(np.stack([np.frombuffer(e.state_export(s, 1), np.uint8)[hdr:] for s in range(S)]), straight["blob"])
    # period 0: the blob is what it is without the call, size and bytes
    blobs = []
    for setp in (False, True):
        with M.Engine(S, fs, M.METER_KMETER) as e:
            if setp:
                e.kmeter_set_period(0, 16)
            e.process_device(dev.data_ptr(), cut, stride=T)
            blobs.append(e.state_export())
    assert blobs[0] == blobs[1]
    del dev


def test_refusals_leave_the_engine_unchanged(M):
    import torch
    fs, P, S = 48000.0, 4800, 5
    T = int(fs) * 2
    x = audio(fs, T, S)
    dev = torch.from_numpy(shaped(x)).cuda()

    def snap(e):
        out = [e.state_export(), *e.kmeter_read(), e.kmeter_period(), e.series_points(M.METER_KMETER)]
        return out + list(e.kmeter_series())

    def unchanged(a, b):
        return all(same(u, v) if isinstance(u, np.ndarray) else u == v for u, v in zip(a, b))

    def refused(code, f, *args):
        with pytest.raises(M.EngineError) as err:
            f(*args)
        assert err.value.code == code, (err.value.code, str(err.value))

    with M.Engine(S, fs, M.METER_KMETER) as e, M.Engine(S, fs, M.METER_KMETER) as other:
        e.kmeter_set_period(P, 64)
        before = snap(e)
        refused(ERR_ARG, e.kmeter_set_period, int(fs) // 20 - 1, 64)     # below the minimum
        assert unchanged(snap(e), before)
        e.process_device(dev.data_ptr(), 7001, stride=T)
        before = snap(e)
        refused(ERR_STATE, e.kmeter_set_period, 2400, 64)                # after a process call
        refused(ERR_STATE, e.kmeter_set_period, 0, 0)
        refused(ERR_UNSUPPORTED, e.process_device_tracks, dev.data_ptr(), 5000, np.full(S, 4000, np.uint64), T)
        refused(ERR_UNSUPPORTED, e.process_tracks, x[:, :5000], np.full(S, 4000, np.uint64))
        other.kmeter_set_period(2400, 64)
        other.process_device(dev.data_ptr(), 7001, stride=T)
        refused(ERR_STATE, e.state_import, other.state_export())         # a blob of another period
        other.reset()
        other.kmeter_set_period(0, 0)
        other.process_device(dev.data_ptr(), 7001, stride=T)
        refused(ERR_STATE, e.state_import, other.state_export())         # ... of none
        other.reset()
        other.kmeter_set_period(P, 64)
        other.process_device(dev.data_ptr(), 7000, stride=T)
        refused(ERR_STATE, e.state_import, other.state_export())         # ... of another fill, on an engine that has moved
        assert unchanged(snap(e), before)
        fresh = snap(other)
        refused(ERR_STATE, other.state_import, before[0][:-1] + bytes([before[0][-1] ^ 1]))   # (a rotten one)
        assert unchanged(snap(other), fresh)
    with M.Engine(S, fs, M.METER_DR14) as e:
        before = e.state_export()
        refused(ERR_ARG, e.kmeter_set_period, P, 64)                     # an engine without the bit
        refused(ERR_ARG, e.kmeter_series)
        refused(ERR_ARG, e.kmeter_period)
        refused(ERR_ARG, e.series_points, M.METER_KMETER)
        assert e.state_export() == before
    del dev


def test_known_answer(M):
    """A full-scale 1 kHz sine reads 1.0 = 0 dB on a K-meter's RMS scale and peak 1.0, at every point from 1 s on."""
    fs, P = 48000.0, 4800
    t = np.arange(int(fs) * 2) / fs
    x = np.sin(2 * np.pi * 1000.0 * t).astype(np.float32)
    with M.Engine(1, fs, M.METER_KMETER, n_channels=1) as e:
        e.kmeter_set_period(P, 64)
        e.process(x[None, :])
        rms, peak, n, d = e.kmeter_series()
    assert n == 20 and d == 0 and rms.shape == (1, 20, 1)
    assert (np.abs(rms[0, 10:, 0] - 1.0) < 1e-3).all() and (np.abs(peak[0, 10:, 0] - 1.0) < 1e-4).all()
