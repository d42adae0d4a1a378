"""Stcorrdsp for a batch (MTR_METER_STCORR, mtr_stcorr.hip) against the restatement of jmeters/stcorrdsp.cc (oracle
mo_stcorr_*, itself bit-identical to the reference object: tests/test_needle_oracle_vs_ref.py).

The oracle is the reference's f32 recurrence; the kernel re-associates the sums, so it is not bit-exact.  The yardstick is how
far the reference itself sits from exact arithmetic: per case D = max over the process () calls of |oracle reading - a float64
restatement of the same recurrence| (a plain Python loop here), and the kernel's reading must lie within 2 D + 4 * 2^-23 of the
oracle's — as far from exact as the reference is, on the other side, plus a floor: three states stored as f32 that enter the
ratio with weights 1, 1/2, 1/2, then one sqrt, multiply, add and divide at half an ulp each, under 4 ulp of 1.0 on a reading
in [-1, 1].  The five states get the same rule relative to their value (zlr, which can cancel to nothing, relative to
sqrt (zll zrr)), with D_rel measured the same way.  No tolerance is written down: every case prints its D and what it saw."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
F = C.c_float
FLOOR = 4.0 * 2.0 ** -23
E20, E10 = float(np.float32(1e-20)), float(np.float32(1e-10))
RATES = [48000, 44100, 192000, 8000]
NAMES = ["independent", "L=R", "R=-0.5L", "R=0.6L+0.4N", "sines 1 rad", "0.6L+0.4N at 1e-4", "silence"]


class Stcorr(C.Structure):
    _fields_ = [(n, F) for n in ("zl", "zr", "zlr", "zll", "zrr", "w1", "w2")]

    def state(self):
        return np.array([self.zl, self.zr, self.zlr, self.zll, self.zrr], np.float32)


@pytest.fixture(scope="module")
def M():
    import meters.lv2_amd as m
    return m


@pytest.fixture(scope="module")
def O(oracle):
    lib = oracle.lib
    lib.mo_stcorr_init.argtypes = [C.POINTER(Stcorr), C.c_int, F, F]
    lib.mo_stcorr_init.restype = None
    lib.mo_stcorr_process.argtypes = [C.POINTER(Stcorr), C.POINTER(F), C.POINTER(F), C.c_int]
    lib.mo_stcorr_process.restype = None
    lib.mo_stcorr_read.argtypes = [C.POINTER(Stcorr)]
    lib.mo_stcorr_read.restype = F
    return lib


def calls_of(fs):
    # below one piece, odd sizes, several pieces, a one-frame call, long calls
    return [1024, 1023, 3 * 4096 + 6, 1, 3, 2 * fs + 1, 512, fs]


def signals(T, fs, seed=500):
    """the seven streams, on the signal of tests/test_gpu_kmeter.py (uniform noise under a 0.7 Hz envelope)"""
    rng = np.random.default_rng(seed)
    t = np.arange(T) / fs
    env = (0.05 + 0.6 * (0.5 + 0.5 * np.sin(2 * np.pi * t * 0.7 + 1.0))).astype(np.float32)

    def noise():
        return rng.uniform(-1, 1, T).astype(np.float32) * env
    x = np.zeros((7, T, 2), np.float32)
    x[0, :, 0], x[0, :, 1] = noise(), noise()
    x[1, :, 0] = noise(); x[1, :, 1] = x[1, :, 0]
    x[2, :, 0] = noise(); x[2, :, 1] = np.float32(-0.5) * x[2, :, 0]
    x[3, :, 0] = noise(); x[3, :, 1] = np.float32(0.6) * x[3, :, 0] + np.float32(0.4) * noise()
    x[4, :, 0] = (0.5 * np.sin(2 * np.pi * 440.0 * t)).astype(np.float32)
    x[4, :, 1] = (0.5 * np.sin(2 * np.pi * 440.0 * t + 1.0)).astype(np.float32)
    x[5] = x[3] * np.float32(1e-4)
    return x


def run_oracle(O, fs, xs, ends):
    """one mo_stcorr_process per block [ends [i - 1], ends [i]): (readings, states) after each"""
    c = Stcorr()
    O.mo_stcorr_init(C.byref(c), int(fs), 2e3, 0.3)
    l, r = np.ascontiguousarray(xs[:, 0]), np.ascontiguousarray(xs[:, 1])
    pl, pr = l.ctypes.data, r.ctypes.data
    out, st, pos = [], [], 0
    for e in ends:
        O.mo_stcorr_process(C.byref(c), C.cast(pl + 4 * pos, C.POINTER(F)), C.cast(pr + 4 * pos, C.POINTER(F)), e - pos)
        pos = e
        out.append(O.mo_stcorr_read(C.byref(c)))
        st.append(c.state())
    return np.array(out, np.float32), np.array(st, np.float32), (float(np.float32(c.w1)), float(np.float32(c.w2)))


def run_exact(w1, w2, xs, ends):
    """the same five updates in float64, the flushes and + 1e-10f at the same ends"""
    ll, rr = xs[:, 0].astype(np.float64).tolist(), xs[:, 1].astype(np.float64).tolist()
    zl = zr = zlr = zll = zrr = 0.0
    out, st, pos = [], [], 0
    fin = math.isfinite
    for e in ends:
        for n in range(pos, e):
            zl += w1 * (ll[n] - zl) + E20
            zr += w1 * (rr[n] - zr) + E20
            zlr += w2 * (zl * zr - zlr)
            zll += w2 * (zl * zl - zll)
            zrr += w2 * (zr * zr - zrr)
        pos = e
        zl, zr = (zl if fin(zl) else 0.0), (zr if fin(zr) else 0.0)
        zlr, zll, zrr = (zlr if fin(zlr) else 0.0) + E10, (zll if fin(zll) else 0.0) + E10, (zrr if fin(zrr) else 0.0) + E10
        out.append(zlr / math.sqrt(zll * zrr + E10))
        st.append((zl, zr, zlr, zll, zrr))
    return np.array(out), np.array(st)


def scale_of(st):
    """what a state's distance is relative to: its own value, for zlr sqrt (zll zrr)"""
    s = np.abs(np.asarray(st, np.float64)).copy()
    s[..., 2] = np.sqrt(s[..., 3] * s[..., 4])
    return s


def yardstick(O, fs, xs, ends):
    want, want_st, (w1, w2) = run_oracle(O, fs, xs, ends)
    ex, ex_st = run_exact(w1, w2, xs, ends)
    D = float(np.max(np.abs(want.astype(np.float64) - ex))) if len(ends) else 0.0
    sc = scale_of(ex_st)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(sc > 0, np.abs(want_st.astype(np.float64) - ex_st) / sc, 0.0)
    return want, want_st, D, (float(rel.max()) if len(ends) else 0.0)


def drive(M, e, x, calls, after=None):
    import torch
    dev = torch.from_numpy(x).cuda()
    st = torch.cuda.current_stream().cuda_stream
    pos = 0
    for i, n in enumerate(calls):
        e.process_device(dev.data_ptr() + pos * 8, n, x.shape[1], st)
        pos += n
        if after:
            after(i)
    e.sync()
    del dev


@pytest.mark.parametrize("fs", RATES)
def test_one_process_per_call(M, O, fs):
    calls = calls_of(fs)
    ends = np.cumsum(calls).tolist()
    x = signals(ends[-1], fs)
    got, got_st = [], []
    with M.Engine(7, float(fs), M.METER_STCORR) as e:
        corr, st = e.stcorr_read()
        assert not corr.any() and not st.any()                            # the constructor's state

        def after(i):
            c, s = e.stcorr_read()
            got.append(c); got_st.append(s)
        drive(M, e, x, calls, after)
    got, got_st = np.array(got), np.array(got_st)                         # [call, stream], [call, stream, 5]
    for s in range(7):
        want, want_st, D, D_rel = yardstick(O, fs, x[s], ends)
        d = np.abs(got[:, s].astype(np.float64) - want)
        sc = scale_of(want_st)
        with np.errstate(divide="ignore", invalid="ignore"):
            ds = np.where(sc > 0, np.abs(got_st[:, s].astype(np.float64) - want_st) / sc, 0.0)
        print(f"fs {fs} P 0 {NAMES[s]}: D {D:.3g} seen {d.max():.3g} | D_rel {D_rel:.3g} seen {ds.max():.3g}")
        assert np.all(d <= 2 * D + FLOOR), (fs, s, D, d)
        assert np.all(ds <= 2 * D_rel + FLOOR), (fs, s, D_rel, ds)


@pytest.mark.parametrize("fs", RATES)
@pytest.mark.parametrize("kind", ["fs/10", "fs/20+7"])
def test_reading_series(M, O, fs, kind):
    P = fs // 10 if kind == "fs/10" else fs // 20 + 7
    calls = calls_of(fs)
    T = sum(calls)
    x = signals(T, fs)
    n = T // P
    ends = [P * (k + 1) for k in range(n)]
    with M.Engine(7, float(fs), M.METER_STCORR) as e:
        e.stcorr_set_period(P, n + 5)
        drive(M, e, x, calls)
        pts, n_points, dropped = e.stcorr_series()
        corr, _ = e.stcorr_read()
        assert M.lib.mtr_engine_stcorr_set_period(e._h, P, 4) == M.engine.ERR_STATE     # it has processed
    assert (n_points, dropped) == (n, 0) and pts.shape == (7, n)
    assert np.array_equal(corr.view(np.uint32), pts[:, -1].view(np.uint32))             # read () = the last completed period
    with M.Engine(7, float(fs), M.METER_STCORR) as e:
        assert M.lib.mtr_engine_stcorr_set_period(e._h, fs // 20 - 1, 4) == M.engine.ERR_ARG    # below the minimum
        e.stcorr_set_period(P, 3)                                                       # a series shorter than the run
        drive(M, e, x, calls)
        few, n2, d2 = e.stcorr_series()
    assert (n2, d2) == (n, n - 3) and np.array_equal(few.view(np.uint32), pts[:, :3].view(np.uint32))
    for s in range(7):
        want, _, D, _ = yardstick(O, fs, x[s], ends)
        d = np.abs(pts[s].astype(np.float64) - want)
        print(f"fs {fs} P {P} {NAMES[s]}: D {D:.3g} seen {d.max():.3g} over {n} points")
        assert np.all(d <= 2 * D + FLOOR), (fs, P, s, D, d.max(), int(d.argmax()))


def test_deterministic(M):
    fs = 48000
    calls = calls_of(fs)
    x = signals(sum(calls), fs, seed=77)
    runs = []
    for _ in range(2):
        with M.Engine(7, float(fs), M.METER_STCORR) as e:
            e.stcorr_set_period(fs // 10, 64)
            drive(M, e, x, calls)
            runs.append((e.stcorr_series()[0], e.stcorr_read()))
    a, b = runs
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    assert np.array_equal(a[1][0].view(np.uint32), b[1][0].view(np.uint32)) and np.array_equal(a[1][1].view(np.uint32), b[1][1].view(np.uint32))


def test_not_finite_samples(M, O):
    """A NaN or Inf sticks in its channel's zl to the end of the process (), where the reference sets the channel's first stage
    and the sums it touched to 0 (then + 1e-10f): exactly so here; the other channel and the next call stay inside the bound."""
    fs = 48000
    calls = [4096, 40000, 5000, 9000, 4096, 3000]
    ends = np.cumsum(calls).tolist()
    x = signals(ends[-1], fs, seed=9)[[0, 3, 4]]
    x[0, ends[0] + 20000, 0] = np.nan                                      # a NaN in L in the middle of call 1
    x[0, ends[2] + 4500, 1] = np.inf                                       # an Inf in R in the middle of call 3
    x[1, ends[1] - 1, 0] = np.nan                                          # the very last frame of call 1
    x[2, ends[0] + 3, 1] = -np.inf                                         # a piece's first frames
    hit = {0: {1: "L", 3: "R"}, 1: {1: "L"}, 2: {1: "R"}}
    got, got_st = [], []
    with M.Engine(3, float(fs), M.METER_STCORR) as e:
        def after(i):
            c, s = e.stcorr_read()
            got.append(c); got_st.append(s)
        drive(M, e, x, calls, after)
    got, got_st = np.array(got), np.array(got_st)
    e10 = np.float32(1e-10)
    for s in range(3):
        want, want_st, D, D_rel = yardstick(O, fs, x[s], ends)
        for i in range(len(calls)):
            ch = hit[s].get(i)
            if ch:                                                         # zl (zr), zlr and zll (zrr): 0, then + 1e-10f — as the oracle's
                idx = [0, 2, 3] if ch == "L" else [1, 2, 4]
                assert want_st[i, idx[0]] == 0 and want_st[i, idx[1]] == e10 and want_st[i, idx[2]] == e10
                assert np.array_equal(got_st[i, s, idx].view(np.uint32), want_st[i, idx].view(np.uint32)), (s, i, got_st[i, s], want_st[i])
        d = np.abs(got[:, s].astype(np.float64) - want)
        sc = scale_of(want_st)
        with np.errstate(divide="ignore", invalid="ignore"):
            ds = np.where(sc > 0, np.abs(got_st[:, s].astype(np.float64) - want_st) / sc, 0.0)
        print(f"not finite, stream {s}: D {D:.3g} seen {d.max():.3g} | D_rel {D_rel:.3g} seen {ds.max():.3g}")
        assert np.all(np.isfinite(got[:, s])) and np.all(np.isfinite(got_st[:, s]))
        assert np.all(d <= 2 * D + FLOOR), (s, D, d)
        assert np.all(ds <= 2 * D_rel + FLOOR), (s, D_rel, ds)


@pytest.mark.parametrize("cuts", ["long calls", "host blocks"])
def test_not_finite_samples_in_the_series(M, O, cuts):
    """The same with a period: the flush happens at every period end, wherever the calls cut — a NaN in a period that closes in the
    middle of a call, one in the period open at a call's end followed by short calls, an Inf just in front of a period end — and the
    period AFTER starts from zl = 0 as the reference's: every point against the oracle fed blocks of exactly P."""
    fs, P = 48000, 4800
    T = 12 * P + 700
    calls = [3 * P + 100, 2 * P + 1300, 1024, 1024, 1024, 1024, 1024, 3000, T - (5 * P + 1400 + 5 * 1024 + 3000)] if cuts == "long calls" \
        else [1024] * (T // 1024) + [T % 1024]
    assert sum(calls) == T
    x = signals(T, fs, seed=13)[[0, 3, 4, 1]]
    x[0, P + 2000, 0] = np.nan                                             # period 1 closes in the middle of call 0
    x[0, 5 * P + 1350, 1] = np.nan                                         # the period open at the end of call 1 (long calls), short calls follow
    x[1, 2 * P - 3, 1] = np.inf                                            # three frames in front of a period end
    x[1, 8 * P - 1, 0] = np.nan                                            # a period's last frame
    x[2, 4 * P, 0] = -np.inf                                               # a period's first frame
    x[3, 6 * P + 17, 0] = np.nan; x[3, 6 * P + 18, 1] = np.nan             # both channels
    n = T // P
    ends = [P * (k + 1) for k in range(n)]
    with M.Engine(4, float(fs), M.METER_STCORR) as e:
        e.stcorr_set_period(P, n)
        drive(M, e, x, calls)
        pts, n_points, _ = e.stcorr_series()
        _, st = e.stcorr_read()
    assert n_points == n and np.all(np.isfinite(pts)) and np.all(np.isfinite(st))
    for s in range(4):
        want, _, D, _ = yardstick(O, fs, x[s], ends)
        d = np.abs(pts[s].astype(np.float64) - want)
        print(f"not finite, P {P}, {cuts}, stream {s}: D {D:.3g} seen {d.max():.3g} at point {int(d.argmax())}")
        assert np.all(d <= 2 * D + FLOOR), (s, D, d)


def test_beside_the_loudness_meters(M):
    """EBU | TRUEPEAK | STCORR in one engine against two engines holding the halves: bit for bit."""
    fs, S, P = 48000, 4, 4800
    calls = [P * 3 + 7, 24000, 1000, 48000]
    x = signals(sum(calls), fs, seed=21)[:S]
    rec = {}
    for name, meters in (("all", M.METER_EBU | M.METER_TRUEPEAK | M.METER_STCORR), ("ebu", M.METER_EBU | M.METER_TRUEPEAK), ("cor", M.METER_STCORR)):
        with M.Engine(S, float(fs), meters) as e:
            if meters & M.METER_EBU:
                e.integr_start()
            if meters & M.METER_STCORR:
                e.stcorr_set_period(P, 32)
            drive(M, e, x, calls)
            r = {}
            if meters & M.METER_EBU:
                r.update(out9=e.out9(), tp=e.truepeak(), hm=e.histograms()[0], hs=e.histograms()[1])
            if meters & M.METER_STCORR:
                r.update(series=e.stcorr_series()[0], corr=e.stcorr_read()[0], st=e.stcorr_read()[1])
            rec[name] = r
    for k, v in list(rec["ebu"].items()) + list(rec["cor"].items()):
        assert np.array_equal(np.ascontiguousarray(v).view(np.uint32), np.ascontiguousarray(rec["all"][k]).view(np.uint32)), k
    assert rec["all"]["series"].shape == (S, sum(calls) // P)


def _record(e):
    pts, n, d = e.stcorr_series()
    corr, st = e.stcorr_read()
    return [pts.view(np.uint32), np.uint32(n), np.uint32(d), corr.view(np.uint32), st.view(np.uint32)]


def _same(a, b):
    for u, v in zip(a, b):
        assert np.array_equal(u, v)


@pytest.mark.parametrize("P", [0, 4807])
def test_every_way_in_is_the_device_call(M, P):
    """host memory in chunks that split the batch, integer PCM, a pair of a 5.1 frame: the same floats, the same bits"""
    fs, S = 48000, 7
    calls = [30000, 5001, 20000]
    T = sum(calls)
    x = signals(T, fs, seed=33)
    q = np.clip(np.rint(x * 32767.0), -32768, 32767).astype(np.int16)
    xq = M.pcm_decode(M.PCM_S16, q)
    wide = np.random.default_rng(4).uniform(-1, 1, (S, T, 6)).astype(np.float32)
    wide[:, :, 4], wide[:, :, 5] = x[:, :, 0], x[:, :, 1]
    assert np.array_equal(M.pick_decode(0, wide, [4, 5]), x)

    def run(feed, src, layout=None):
        with M.Engine(S, float(fs), M.METER_STCORR) as e:
            e.stcorr_set_period(P, 16)
            if layout:
                e.set_frame_layout(*layout)
            e.set_host_chunk_bytes(3 * 30000 * 8)                         # three streams of the longest call per chunk
            if feed == "device":
                drive(M, e, src, calls)
            else:
                pos = 0
                for n in calls:
                    getattr(e, feed)(np.ascontiguousarray(src[:, pos:pos + n]))
                    pos += n
            return _record(e)
    base = run("device", x)
    _same(base, run("process", x))
    _same(run("device", xq), run("process_pcm", q))
    _same(base, run("process", wide, (6, [4, 5])))
    assert base[1] == (T // P if P else 0)


def test_state_travels(M):
    """Export in the middle of a period, import into another engine at other slots: the continuation is bit for bit the
    uninterrupted run's (the pattern of tests/test_gpu_state.py).  The series is not part of the blob."""
    import torch
    fs, S, P = 48000, 5, 4800
    calls, k_stop = [5000, 7000, 9000, 4800, 1234], 2
    T = sum(calls)
    x = signals(T, fs, seed=55)[:S]
    with M.Engine(S, float(fs), M.METER_STCORR | M.METER_KMETER) as e:
        e.stcorr_set_period(P, 64)
        drive(M, e, x, calls)
        want_pts, want_n, _ = e.stcorr_series()
        want_corr, want_st = e.stcorr_read()
    done = sum(calls[:k_stop])
    assert done % P                                                        # the export lies inside a period
    with M.Engine(S, float(fs), M.METER_STCORR | M.METER_KMETER) as e:
        e.stcorr_set_period(P, 64)
        drive(M, e, x[:, :done], calls[:k_stop])
        assert e.state_bytes(S) == len(e.state_export())
        blob = e.state_export()
        # an engine that stands elsewhere refuses the blob: another cursor ...
        assert M.lib.mtr_engine_state_import(e._h, 0, blob, len(blob)) == 0
        e.process(np.zeros((S, 100, 2), np.float32))
        assert M.lib.mtr_engine_state_import(e._h, 0, blob, len(blob)) == M.engine.ERR_STATE
    with M.Engine(S, float(fs), M.METER_STCORR | M.METER_KMETER) as e:       # ... another period
        e.process(np.zeros((S, done, 2), np.float32))
        assert M.lib.mtr_engine_state_import(e._h, 0, blob, len(blob)) == M.engine.ERR_STATE
    rest = np.zeros((S + 3, T - done, 2), np.float32)
    rest[2:2 + S] = x[:, done:]
    with M.Engine(S + 3, float(fs), M.METER_STCORR | M.METER_KMETER) as e:
        e.stcorr_set_period(P, 64)
        assert e.state_import(blob, first=2) == S
        _, st0 = e.stcorr_read(2, S)
        drive(M, e, rest, calls[k_stop:])
        pts, n, _ = e.stcorr_series(2, S)
        corr, st = e.stcorr_read(2, S)
    assert n == want_n - done // P                                          # the points restart with the engine's
    assert np.array_equal(pts.view(np.uint32), want_pts[:, done // P:].view(np.uint32))
    assert np.array_equal(corr.view(np.uint32), want_corr.view(np.uint32)) and np.array_equal(st.view(np.uint32), want_st.view(np.uint32))
    # a fresh engine takes the blob's period and cursor
    with M.Engine(S, float(fs), M.METER_STCORR | M.METER_KMETER) as e:
        assert e.state_import(blob) == S
        drive(M, e, np.ascontiguousarray(x[:, done:]), calls[k_stop:])
        _, n, d = e.stcorr_series()
        corr, st = e.stcorr_read()
    assert (n, d) == (want_n - done // P, want_n - done // P)                # (it has no series to hold them)
    assert np.array_equal(corr.view(np.uint32), want_corr.view(np.uint32)) and np.array_equal(st.view(np.uint32), want_st.view(np.uint32))
    del torch


def test_blobs_without_the_bit_keep_their_size(M):
    """state_sections: mtr_stream_state 408, the two histograms 2 * 751 * 4, the FIR history 47 * 2 * 4, Kmeterdsp 2 * 24, DR-14 52 + 2 * 8000 * 4
    per stream behind a header of 64 bytes; STCORR appends 32 bytes per stream to an engine that has the bit and nothing to any other."""
    base = 408 + 2 * 751 * 4 + 47 * 2 * 4
    for meters, per in ((M.METER_EBU | M.METER_TRUEPEAK, base), (M.METER_KMETER, base + 48), (M.METER_DR14 | M.METER_KMETER, base + 52 + 64000 + 48),
                        (M.METER_STCORR, base + 32), (M.METER_KMETER | M.METER_STCORR, base + 48 + 32)):
        with M.Engine(3, 48000.0, meters) as e:
            assert e.state_bytes(3) == 64 + 3 * per, (meters, e.state_bytes(3))
            assert e.state_bytes(0) == 64


def test_refusals_and_reset(M):
    fs, S = 48000, 3
    x = signals(20000, fs, seed=5)[:S]
    with M.Engine(S, float(fs), M.METER_EBU | M.METER_STCORR) as e:
        with pytest.raises(M.EngineError) as err:
            e.process_lengths(x, [20000, 100, 5])
        assert err.value.code == M.engine.ERR_UNSUPPORTED
        import torch
        dev = torch.from_numpy(x).cuda()
        with pytest.raises(M.EngineError) as err:
            e.process_device_lengths(dev.data_ptr(), 20000, [20000, 100, 5])
        assert err.value.code == M.engine.ERR_UNSUPPORTED
        with pytest.raises(M.EngineError) as err:
            e.process_pcm(np.zeros((S, 100, 2), np.int16), frames=[100, 100, 5])
        assert err.value.code == M.engine.ERR_UNSUPPORTED
    with M.Engine(S, float(fs), M.METER_KMETER) as e:                       # an engine without the bit has no such meter
        assert M.lib.mtr_engine_stcorr_reset(e._h) == M.engine.ERR_ARG
        assert M.lib.mtr_engine_stcorr_set_period(e._h, 0, 0) == M.engine.ERR_ARG
    for whole in (False, True):
        with M.Engine(S, float(fs), M.METER_STCORR) as e:
            e.stcorr_set_period(2400, 16)
            e.process(x)
            pts0, n, _ = e.stcorr_series()
            assert n == 8 and pts0.any() and e.stcorr_read()[0].any()
            e.reset() if whole else e.stcorr_reset()
            pts, n, d = e.stcorr_series()
            corr, st = e.stcorr_read()
            assert (n, d) == (0, 0) and pts.shape == (S, 0) and not corr.any() and not st.any()
            e.process(x)                                                    # ... period kept, and the same points again
            again, n, _ = e.stcorr_series()
            assert n == 8 and np.array_equal(again.view(np.uint32), pts0.view(np.uint32))


@pytest.mark.timeout(1500)
def test_full_size(M, O):
    """8192 streams x 10 s at 48 kHz in device memory, one call: P = 0 and P = 4800; eight sampled streams against the oracle."""
    import torch
    fs, S, T, P = 48000, 8192, 480000, 4800
    buf = torch.empty((S, T, 2), dtype=torch.float32, device="cuda")
    M.synth_fill_device(buf.data_ptr(), S, T, T, 1234, float(fs), 1)
    torch.cuda.synchronize()
    pick = [0, 1, 1023, 4095, 4096, 6001, 8190, 8191]
    with M.Engine(S, float(fs), M.METER_STCORR) as e:
        e.process_device(buf.data_ptr(), T)
        corr0 = e.stcorr_read()[0]
    with M.Engine(S, float(fs), M.METER_STCORR) as e:
        e.stcorr_set_period(P, T // P)
        e.process_device(buf.data_ptr(), T)
        pts, n, d = e.stcorr_series()
        assert (n, d) == (T // P, 0)
    assert np.all(np.isfinite(corr0)) and np.all(np.abs(corr0) <= 1.0 + 1e-6) and np.all(np.isfinite(pts))
    for s in pick:
        xs = buf[s].cpu().numpy()
        want, _, D, _ = yardstick(O, fs, xs, [T])
        seen = abs(float(corr0[s]) - float(want[0]))
        wantp, _, Dp, _ = yardstick(O, fs, xs, [P * (k + 1) for k in range(T // P)])
        seenp = np.abs(pts[s].astype(np.float64) - wantp)
        print(f"full size, stream {s}: P 0 D {D:.3g} seen {seen:.3g} | P {P} D {Dp:.3g} seen {seenp.max():.3g}")
        assert seen <= 2 * D + FLOOR, (s, D, seen)
        assert np.all(seenp <= 2 * Dp + FLOOR), (s, Dp, seenp.max())
