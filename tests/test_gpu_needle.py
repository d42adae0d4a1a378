"""The needle meters for a batch (MTR_METER_NEEDLE, mtr_needle.hip) against the restatements of jmeters/vumeterdsp.cc, iec1ppmdsp.cc,
iec2ppmdsp.cc and msppmdsp.cc (oracle mo_vu_*, mo_ppm_*, mo_msppm_*, themselves bit-identical to the reference objects:
tests/test_needle_oracle_vs_ref.py, tests/test_oracle_vs_ref.py).

The kernel is a serial chain that does the reference's f32 operations in the reference's order, so every comparison here is equality
of BYTES with the oracle driven as "a host with blocks of P frames": the series, the level mtr_engine_needle_read returns, and the
state (z1 z2 as the last completed process () stored them).  The periods are the small ones (16, 18, 1023): a long period hides a
fused multiply-add, a missing + 1e-10f or P mod 4 frames that were not dropped behind the maximum over the period."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
F = C.c_float
FS = 48000
T1 = 60000
CALLS1 = [30000, 5001, 3, 1, 20000, 4995]
CALLS2 = [1024, 1023, 64, 1, 3, 4096 * 3 + 6, 96001, 512, 512]
VU, IEC1, IEC2, MS = 1, 2, 4, 8
ALL = VU | IEC1 | IEC2 | MS
KINDS = (VU, IEC1, IEC2, MS)


class Vu(C.Structure):
    _fields_ = [("z1", F), ("z2", F), ("m", F), ("res", C.c_int), ("w", F), ("g", F)]


class Ppm(C.Structure):
    _fields_ = [("z1", F), ("z2", F), ("m", F), ("res", C.c_int), ("w1", F), ("w2", F), ("w3", F), ("g", F)]


class Msppm(C.Structure):
    _fields_ = [("p", Ppm), ("db", F), ("mv", F)]


@pytest.fixture(scope="module")
def M():
    import meters.lv2_amd as m
    return m


@pytest.fixture(scope="module")
def O(oracle):
    lib = C.CDLL(oracle.lib._name)                                 # (a handle of its own: the session's keeps its argtypes)
    vp = C.c_void_p
    lib.mo_vu_init.argtypes = [C.POINTER(Vu), F]
    lib.mo_vu_process.argtypes = [C.POINTER(Vu), vp, C.c_int]
    lib.mo_vu_read.argtypes = [C.POINTER(Vu)]
    lib.mo_ppm_init_iec1.argtypes = [C.POINTER(Ppm), F]
    lib.mo_ppm_init_iec2.argtypes = [C.POINTER(Ppm), F]
    lib.mo_ppm_process.argtypes = [C.POINTER(Ppm), vp, C.c_int]
    lib.mo_ppm_read.argtypes = [C.POINTER(Ppm)]
    lib.mo_msppm_init.argtypes = [C.POINTER(Msppm), F, F]
    lib.mo_msppm_set_gain.argtypes = [C.POINTER(Msppm), F]
    lib.mo_msppm_process.argtypes = [C.POINTER(Msppm), vp, vp, C.c_int, C.c_int]
    lib.mo_msppm_read.argtypes = [C.POINTER(Msppm)]
    for f in ("mo_vu_init", "mo_vu_process", "mo_ppm_init_iec1", "mo_ppm_init_iec2", "mo_ppm_process", "mo_msppm_init", "mo_msppm_set_gain",
              "mo_msppm_process"):
        getattr(lib, f).restype = None
    for f in ("mo_vu_read", "mo_ppm_read", "mo_msppm_read"):
        getattr(lib, f).restype = F
    return lib


def stream(s, T, fs=FS):
    """stream s of the issue's signal: uniform noise under "6000 frames on, 6000 at 0.1, 8000 digital silence", R a quarter of its own
    noise, a 110 Hz tone of rising level on even s, everything at 1e-4 where s is a multiple of 3"""
    rng = np.random.default_rng(s)
    n = np.arange(T)
    ph = n % 20000
    env = np.where(ph < 6000, 1.0, np.where(ph < 12000, 0.1, 0.0)).astype(np.float32)
    x = np.zeros((T, 2), np.float32)
    x[:, 0] = rng.uniform(-1, 1, T).astype(np.float32) * env
    x[:, 1] = np.float32(0.25) * rng.uniform(-1, 1, T).astype(np.float32) * env
    if s % 2 == 0:
        tone = (0.5 * np.sin(2 * np.pi * 110.0 * n / fs) * (n / T)).astype(np.float32)
        x[:, 0] += tone
        x[:, 1] += np.float32(0.5) * tone
    return x * np.float32(1.0 if s % 3 else 1e-4)


_sig = {}


def signal(S, T):
    if (S, T) not in _sig:
        _sig[(S, T)] = np.stack([stream(s, T) for s in range(S)])
    return _sig[(S, T)]


def oracle_run(O, kind, x, ends, read_at=None, gains=(-6.0, -6.0), gain_at=None):
    """x [T, C] through the detectors of `kind`, one per channel (M/S: per side): one process () per block [ends [i - 1], ends [i]), read ()
    after block i (if read_at is None or i in it).  gain_at = (block index, side, dB): set_gain in front of that block.
    -> (levels [reads, C], states [reads, C, 2] = z1 z2 as stored)"""
    x = np.asarray(x, np.float32)
    if x.ndim == 1:
        x = x[:, None]
    chan = [np.ascontiguousarray(x[:, c]) for c in range(x.shape[1])]
    nc = 2 if kind == MS else x.shape[1]
    lev, sta = [], []
    for c in range(nc):
        if kind == VU:
            o = Vu()
            O.mo_vu_init(C.byref(o), float(FS))
            proc, read, core, p0 = O.mo_vu_process, O.mo_vu_read, o, chan[c].ctypes.data
        elif kind == MS:
            o = Msppm()
            O.mo_msppm_init(C.byref(o), float(FS), gains[c])
            read, core, p0, p1 = O.mo_msppm_read, o.p, chan[0].ctypes.data, chan[1].ctypes.data
        else:
            o = Ppm()
            (O.mo_ppm_init_iec1 if kind == IEC1 else O.mo_ppm_init_iec2)(C.byref(o), float(FS))
            proc, read, core, p0 = O.mo_ppm_process, O.mo_ppm_read, o, chan[c].ctypes.data
        ref = C.byref(o)
        lv, st, pos = [], [], 0
        for i, e in enumerate(ends):
            if kind == MS:
                if gain_at and gain_at[0] == i and gain_at[1] == c:
                    O.mo_msppm_set_gain(ref, gain_at[2])
                O.mo_msppm_process(ref, p0 + 4 * pos, p1 + 4 * pos, e - pos, c)
            else:
                proc(ref, p0 + 4 * pos, e - pos)
            pos = e
            if read_at is None or i in read_at:
                lv.append(read(ref))
                st.append((core.z1, core.z2))
        lev.append(lv)
        sta.append(st)
    return np.array(lev, np.float32).T.copy(), np.array(sta, np.float32).transpose(1, 0, 2).copy()


def periods(T, P):
    return [P * (k + 1) for k in range(T // P)]


def same(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def kinds_of(mask):
    return [k for k in KINDS if mask & k]


def record(e, kinds):
    r = {}
    for k in kinds_of(kinds):
        pts, n, d = e.needle_series(k)
        lev, st = e.needle_read(k)
        r[k] = dict(series=pts, n=n, dropped=d, level=lev, state=st)
    return r


def run_device(M, x, calls, kinds, P, cap, odd=True, reads=None, before=None):
    """x [S, T, C] (or [S, T]) in device memory — `odd`: rows T + 3 frames apart behind a base one frame into the allocation — call by
    call.  reads: the calls after which every kind is read (-> list of {kind: (level, state)}); before (i, e): a hook in front of call i.
    -> (record at the end, reads)"""
    import torch
    x = np.ascontiguousarray(x, np.float32)
    S, T = x.shape[:2]
    Cn = 1 if x.ndim == 2 else x.shape[2]
    stride = T + 3 if odd else T
    host = np.zeros(S * stride * Cn + (Cn if odd else 0), np.float32)
    host[(Cn if odd else 0):].reshape(S, stride, Cn)[:, :T] = x.reshape(S, T, Cn)
    dev = torch.from_numpy(host).cuda()
    base = dev.data_ptr() + (4 * Cn if odd else 0)
    st = torch.cuda.current_stream().cuda_stream
    got = []
    with M.Engine(S, float(FS), M.METER_NEEDLE, n_channels=Cn) as e:
        if kinds is not None:
            e.needle_configure(kinds, P, cap)
        else:
            kinds = IEC2
        pos = 0
        for i, n in enumerate(calls):
            if before:
                before(i, e)
            e.process_device(base + pos * 4 * Cn, n, stride, st)
            pos += n
            if reads is not None and i in reads:
                got.append({k: e.needle_read(k) for k in kinds_of(kinds)})
        e.sync()
        rec = record(e, kinds)
    del dev
    return rec, got


_runs = {}


def case1(M, P):
    """test 1's device run at period P (S = 37, all four kinds), once per session"""
    if P not in _runs:
        _runs[P] = run_device(M, signal(37, T1), CALLS1, ALL, P, 4000)[0]
    return _runs[P]


@pytest.mark.parametrize("P", [16, 18, 1023])
def test_series_at_the_smallest_periods(M, O, P):
    S = 37
    x = signal(S, T1)
    assert sum(CALLS1) == T1
    rec = case1(M, P)
    ends = periods(T1, P)
    for k in KINDS:
        r = rec[k]
        assert (r["n"], r["dropped"]) == (len(ends), 0) and r["series"].shape == (S, len(ends), 2)
        for s in range(S):
            want, want_st = oracle_run(O, k, x[s], ends)
            assert same(r["series"][s], want), (P, k, s, int(np.argmax((r["series"][s].view(np.uint32) != want.view(np.uint32)).any(axis=1))))
            assert same(r["level"][s], want[-1]) and same(r["state"][s], want_st[-1]), (P, k, s, r["state"][s], want_st[-1])


@pytest.mark.parametrize("channels", [2, 1])
def test_one_process_per_call(M, O, channels):
    S, reads = 5, {2, 3, 6, 8}
    x = signal(S, sum(CALLS2))
    if channels == 1:
        x = np.ascontiguousarray(x[:, :, 0])
    kinds = ALL if channels == 2 else VU | IEC1 | IEC2
    _, got = run_device(M, x, CALLS2, kinds, 0, 0, reads=reads)
    assert len(got) == len(reads)
    ends = np.cumsum(CALLS2).tolist()
    for k in kinds_of(kinds):
        for s in range(S):
            want, want_st = oracle_run(O, k, x[s], ends, read_at=reads)       # the maximum is held over the calls nobody read after
            for j in range(len(reads)):
                lev, st = got[j][k]
                assert same(lev[s], want[j]) and same(st[s], want_st[j]), (channels, k, s, j, lev[s], want[j], st[s], want_st[j])


def test_default_is_iec2_per_call(M, O):
    """an engine that was never configured: MTR_NEEDLE_IEC2, one process () per call"""
    x = signal(5, sum(CALLS2))[:, :20000]
    calls = [5000, 15000]
    rec, _ = run_device(M, x, calls, None, 0, 0)
    for s in range(5):
        want, want_st = oracle_run(O, IEC2, x[s], [5000, 20000], read_at={1})
        assert same(rec[IEC2]["level"][s], want[0]) and same(rec[IEC2]["state"][s], want_st[0])
    assert rec[IEC2]["n"] == 0


@pytest.mark.parametrize("P", [0, 2400])
def test_not_finite(M, O, P):
    """+Inf, -Inf, NaN, 1e30f and L = +Inf with R = -Inf (the M side is a NaN) in the middle of a block, in its last kept frame and —
    where the block has any (period 0: calls of 2402 frames) — in a dropped frame."""
    S, B, nb = 4, (2402 if P == 0 else 2400), 6
    calls = [2402] * nb
    T = sum(calls)
    x = signal(S, T).copy()
    inf = np.float32(np.inf)
    x[0, B + 1000, 0] = inf                                     # the middle of block 1
    x[0, 3 * B + 1200, 1] = np.nan
    x[1, 2 * B + 2399, 0] = -inf                                # a block's last kept frame
    x[1, 4 * B + 777, 1] = np.float32(1e30)
    x[2, B + 1500] = (inf, -inf)                                # M = NaN, S = Inf
    x[2, 3 * B + 2399, 0] = np.nan
    x[3, B + 2400 if P == 0 else 2 * B - 1, 0] = inf            # a dropped frame (period 0), else a block's last frame
    x[3, 3 * B + 2401 if P == 0 else 4 * B - 4, 1] = np.nan
    x[3, 4 * B + 2, 1] = -inf
    if P == 0:
        ends = np.cumsum(calls).tolist()
        _, got = run_device(M, x, calls, ALL, 0, 0, reads=set(range(nb)))
        lev = {k: np.array([g[k][0] for g in got]) for k in KINDS}          # [block, stream, C]
        sta = {k: np.array([g[k][1] for g in got]) for k in KINDS}
    else:
        ends = periods(T, P)
        rec, _ = run_device(M, x, calls, ALL, P, 16)
        lev = {k: rec[k]["series"].transpose(1, 0, 2) for k in KINDS}
        sta = None
    for k in KINDS:
        for s in range(S):
            want, want_st = oracle_run(O, k, x[s], ends)
            assert same(lev[k][:, s], want), (P, k, s, lev[k][:, s], want)
            if sta is not None:
                assert same(sta[k][:, s], want_st), (P, k, s, sta[k][:, s], want_st)
            else:
                assert same(rec[k]["state"][s], want_st[-1]) and same(rec[k]["level"][s], want[-1])
    # what the bytes above mean: the Inf of stream 0's L sticks to the end of block 1 ...
    want, want_st = oracle_run(O, IEC1, x[0], ends)
    assert want[1, 0] == inf and np.all(want_st[1, 0] == inf) and np.isfinite(want[1, 1])
    assert np.isfinite(want[2, 0]) and np.all(want_st[2, 0] <= 20.0)          # ... and block 2 starts from the clamp to 20
    want, want_st = oracle_run(O, VU, x[0], ends)
    assert want[1, 0] == inf and np.all(want_st[1, 0] == 0.0)                 # the VU's flush: z = 0, the reading INFINITY
    want, _ = oracle_run(O, MS, x[2], ends)
    assert np.isfinite(want[1, 0]) and want[1, 1] == inf                      # the NaN on the M side is ignored, the Inf on the S side is not


@pytest.mark.parametrize("kind", KINDS)
def test_kinds_are_independent(M, kind):
    """one kind alone against the same kind among all four"""
    alone, _ = run_device(M, signal(37, T1), CALLS1, kind, 18, 4000)
    every = case1(M, 18)
    for f in ("series", "level", "state"):
        assert same(alone[kind][f], every[kind][f]), (kind, f)
    assert alone[kind]["n"] == every[kind]["n"] == T1 // 18


@pytest.mark.parametrize("P,calls", [(0, [5000, 5003, 777]), (16, [4800, 4800, 1600])])
def test_ms_gain(M, O, P, calls):
    """set_gain (S, +14 dB) between two calls, as bbcm_run's switch does; the gain is a control: it survives reset ()"""
    S, T = 5, sum(calls)
    x = signal(S, T1)[:, :T]
    ends = np.cumsum(calls).tolist() if P == 0 else periods(T, P)
    at = 1 if P == 0 else calls[0] // P                                      # the block in front of which the oracle's gain moves
    import torch
    dev = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    with M.Engine(S, float(FS), M.METER_NEEDLE) as e:
        e.needle_configure(MS | IEC2, P, 1000)
        got = []
        pos = 0
        for i, n in enumerate(calls):
            if i == 1:
                e.needle_set_gain(1, 14.0)
            e.process_device(dev.data_ptr() + pos * 8, n, T)
            pos += n
            if P == 0:
                got.append(e.needle_read(MS))
        first = record(e, MS | IEC2)
        e.reset()                                                           # ... the constructors' state, the gains as they are
        e.process_device(dev.data_ptr(), T, T)
        e.sync()
        again = record(e, MS | IEC2)
    for s in range(S):
        want, want_st = oracle_run(O, MS, x[s], ends, gain_at=(at, 1, 14.0))
        if P == 0:
            for j in range(len(calls)):
                assert same(got[j][0][s], want[j]) and same(got[j][1][s], want_st[j]), (s, j)
            w2, w2_st = oracle_run(O, MS, x[s], [T], gains=(-6.0, 14.0))
            assert same(again[MS]["level"][s], w2[0]) and same(again[MS]["state"][s], w2_st[0]), s
        else:
            assert same(first[MS]["series"][s], want) and same(first[MS]["state"][s], want_st[-1]), s
            w2, w2_st = oracle_run(O, MS, x[s], ends, gains=(-6.0, 14.0))
            assert same(again[MS]["series"][s], w2) and same(again[MS]["state"][s], w2_st[-1]), s
        assert not same(want[-1], oracle_run(O, MS, x[s], ends)[0][-1])     # (the gain is heard)
    del dev


def test_every_way_in_is_the_device_call(M):
    """host memory in chunks that split the batch, integer PCM, two channels of a 4-channel frame: the same floats, the same bytes"""
    S, P = 37, 18
    x = signal(S, T1)
    q = np.clip(np.rint(x * 32767.0), -32768, 32767).astype(np.int16)
    xq = M.pcm_decode(M.PCM_S16, q)
    wide = np.random.default_rng(4).uniform(-1, 1, (S, T1, 4)).astype(np.float32)
    wide[:, :, 2], wide[:, :, 3] = x[:, :, 0], x[:, :, 1]
    assert np.array_equal(M.pick_decode(0, wide, [2, 3]), x)

    def run(feed, src, layout=None):
        with M.Engine(S, float(FS), M.METER_NEEDLE) as e:
            e.needle_configure(ALL, P, 4000)
            if layout:
                e.set_frame_layout(*layout)
            e.set_host_chunk_bytes(13 * 30000 * 8 * (2 if layout else 1))     # 13 streams of the longest call per chunk: 3 chunks
            pos = 0
            for n in CALLS1:
                getattr(e, feed)(np.ascontiguousarray(src[:, pos:pos + n]))
                pos += n
            return record(e, ALL)

    def check(a, b):
        for k in KINDS:
            assert (a[k]["n"], a[k]["dropped"]) == (b[k]["n"], b[k]["dropped"])
            for f in ("series", "level", "state"):
                assert same(a[k][f], b[k][f]), (k, f)
    base = case1(M, P)
    check(base, run("process", x))
    check(run_device(M, xq, CALLS1, ALL, P, 4000)[0], run("process_pcm", q))
    check(base, run("process", wide, (4, [2, 3])))


def test_state_travels(M):
    """Export in the middle of a period, import three of the streams into other slots of a fresh engine configured alike: the
    continuation is byte for byte the uninterrupted run's.  The series is not part of the blob."""
    S, P = 5, 18
    calls, k_stop = [5000, 7001, 9000, 4803, 1234], 2
    T, done = sum(calls), sum(calls[:2])
    x = signal(S, T1)[:, :T]
    assert done % P and (done % P) % 4                                       # inside a period, inside a group of four
    meters = M.METER_NEEDLE | M.METER_KMETER

    def feed(e, src, cs):
        pos = 0
        for n in cs:
            e.process(np.ascontiguousarray(src[:, pos:pos + n]))
            pos += n

    with M.Engine(S, float(FS), meters) as e:
        e.needle_configure(ALL, P, 4000)
        feed(e, x, calls)
        want = record(e, ALL)
    with M.Engine(S, float(FS), meters) as e:
        e.needle_configure(ALL, P, 4000)
        e.needle_set_gain(0, -3.0)
        e.needle_set_gain(0, -6.0)
        feed(e, x, calls[:k_stop])
        assert e.state_bytes(3) == len(e.state_export(2, 3))
        blob = e.state_export(2, 3)
        with M.Engine(3, float(FS), M.METER_KMETER) as plain, M.Engine(3, float(FS), M.METER_KMETER | M.METER_STCORR) as cor:
            # an engine without the bit: its blob is what it was (and NEEDLE's section comes behind STCORR's)
            assert plain.state_bytes(3) == len(plain.state_export()) and cor.state_bytes(3) == len(cor.state_export())
            per = (e.state_bytes(3) - e.state_bytes(0)) // 3 - (plain.state_bytes(3) - plain.state_bytes(0)) // 3
            assert per == 32 + 4 * 2 * 32 and e.state_bytes(0) == plain.state_bytes(0)
    with M.Engine(S, float(FS), meters) as e:                                # another period: refused
        e.needle_configure(ALL, 20, 4000)
        assert M.lib.mtr_engine_state_import(e._h, 1, blob, len(blob)) == M.engine.ERR_STATE
    with M.Engine(S, float(FS), meters) as e:                                # other kinds: refused
        e.needle_configure(VU | IEC1 | IEC2, P, 4000)
        assert M.lib.mtr_engine_state_import(e._h, 1, blob, len(blob)) == M.engine.ERR_STATE
    rest = np.zeros((S, T - done, 2), np.float32)
    rest[1:4] = x[2:5, done:]
    with M.Engine(S, float(FS), meters) as e:
        e.needle_configure(ALL, P, 4000)
        assert e.state_import(blob, first=1) == 3
        feed(e, rest, calls[k_stop:])
        for k in KINDS:
            pts, n, d = e.needle_series(k, 1, 3)
            lev, st = e.needle_read(k, 1, 3)
            assert (n, d) == (want[k]["n"] - done // P, 0)                  # the points restart with the engine's
            assert same(pts, want[k]["series"][2:5, done // P:]), k
            assert same(lev, want[k]["level"][2:5]) and same(st, want[k]["state"][2:5]), k


def test_refusals_and_reset(M):
    S = 3
    x = signal(5, T1)[:S, :20000]
    E = M.engine
    with M.Engine(S, float(FS), M.METER_EBU | M.METER_NEEDLE) as e:
        assert M.lib.mtr_engine_needle_configure(e._h, IEC2, 15, 4) == E.ERR_ARG
        assert M.lib.mtr_engine_needle_configure(e._h, IEC2, 1, 4) == E.ERR_ARG
        assert M.lib.mtr_engine_needle_configure(e._h, 0, 16, 4) == E.ERR_ARG
        assert M.lib.mtr_engine_needle_configure(e._h, 16, 16, 4) == E.ERR_ARG
        assert M.lib.mtr_engine_needle_set_gain(e._h, 2, 0.0) == E.ERR_ARG
        with pytest.raises(M.EngineError) as err:
            e.process_lengths(x, [20000, 100, 5])
        assert err.value.code == E.ERR_UNSUPPORTED
        import torch
        dev = torch.from_numpy(x).cuda()
        with pytest.raises(M.EngineError) as err:
            e.process_device_lengths(dev.data_ptr(), 20000, [20000, 100, 5])
        assert err.value.code == E.ERR_UNSUPPORTED
        e.needle_configure(VU, 16, 4)
        e.process(x)
        assert M.lib.mtr_engine_needle_configure(e._h, IEC2, 16, 4) == E.ERR_STATE     # it has processed
        lev = np.zeros((S, 2), np.float32)
        assert M.lib.mtr_engine_needle_read(e._h, IEC2, 0, S, lev.ctypes.data, None) == E.ERR_ARG   # not a selected kind
        assert M.lib.mtr_engine_needle_read(e._h, VU | IEC2, 0, S, lev.ctypes.data, None) == E.ERR_ARG
    with M.Engine(S, float(FS), M.METER_NEEDLE, n_channels=1) as e:
        assert M.lib.mtr_engine_needle_configure(e._h, MS, 0, 0) == E.ERR_UNSUPPORTED
        assert M.lib.mtr_engine_needle_configure(e._h, VU | MS, 16, 4) == E.ERR_UNSUPPORTED
    with M.Engine(S, float(FS), M.METER_KMETER) as e:                       # an engine without the bit has no such meter
        assert M.lib.mtr_engine_needle_reset(e._h) == E.ERR_ARG
        assert M.lib.mtr_engine_needle_configure(e._h, IEC2, 0, 0) == E.ERR_ARG
    P, n = 2400, 20000 // 2400
    for whole in (False, True):
        with M.Engine(S, float(FS), M.METER_NEEDLE) as e:
            e.needle_configure(ALL, P, 16)
            e.process(x)
            r0 = record(e, ALL)
            assert r0[IEC1]["n"] == n and r0[IEC1]["series"].any() and r0[IEC1]["level"].any()
            e.reset() if whole else e.needle_reset()
            r = record(e, ALL)
            for k in KINDS:
                assert (r[k]["n"], r[k]["dropped"]) == (0, 0) and r[k]["series"].shape == (S, 0, 2)
                assert not r[k]["level"].any() and not r[k]["state"].any()
            e.process(x)                                                    # ... kinds and period kept: the same points again
            r = record(e, ALL)
            for k in KINDS:
                assert r[k]["n"] == n and same(r[k]["series"], r0[k]["series"]) and same(r[k]["state"], r0[k]["state"])
    with M.Engine(S, float(FS), M.METER_NEEDLE) as e:                       # a series shorter than the run
        e.needle_configure(ALL, P, 3)
        e.process(x)
        r = record(e, ALL)
        for k in KINDS:
            assert (r[k]["n"], r[k]["dropped"]) == (n, n - 3) and same(r[k]["series"], r0[k]["series"][:, :3])
            assert same(r[k]["level"], r0[k]["level"]) and same(r[k]["state"], r0[k]["state"])


def test_deterministic(M):
    a = case1(M, 16)
    b = run_device(M, signal(37, T1), CALLS1, ALL, 16, 4000)[0]
    for k in KINDS:
        for f in ("series", "level", "state"):
            assert same(a[k][f], b[k][f]), (k, f)


def test_beside_the_other_meters(M):
    """EBU | TRUEPEAK | KMETER | STCORR | NEEDLE in one engine: the needle meters' bytes are those of an engine that holds them alone"""
    S, P = 5, 18
    x = signal(S, T1)[:, :30000]
    calls = [10001, 19999]
    rec = []
    for meters in (M.METER_NEEDLE, M.METER_NEEDLE | M.METER_EBU | M.METER_TRUEPEAK | M.METER_KMETER | M.METER_STCORR):
        with M.Engine(S, float(FS), meters) as e:
            e.needle_configure(ALL, P, 2000)
            pos = 0
            for n in calls:
                e.process(np.ascontiguousarray(x[:, pos:pos + n]))
                pos += n
            rec.append(record(e, ALL))
    for k in KINDS:
        for f in ("series", "level", "state"):
            assert same(rec[0][k][f], rec[1][k][f]), (k, f)


@pytest.mark.timeout(1500)
def test_full_size(M, O):
    """8192 streams x 10 s at 48 kHz in device memory, one call, all four kinds, P = 4800: eight sampled streams against the oracle."""
    import torch
    S, T, P = 8192, 480000, 4800
    buf = torch.empty((S, T, 2), dtype=torch.float32, device="cuda")
    M.synth_fill_device(buf.data_ptr(), S, T, T, 1234, float(FS), 1)
    torch.cuda.synchronize()
    pick = [0, 1, 1023, 4095, 4096, 6001, 8190, 8191]
    with M.Engine(S, float(FS), M.METER_NEEDLE) as e:
        e.needle_configure(ALL, P, T // P)
        e.process_device(buf.data_ptr(), T)
        rec = {k: (e.needle_series(k), e.needle_read(k)) for k in KINDS}
    ends = periods(T, P)
    for s in pick:
        xs = buf[s].cpu().numpy()
        for k in KINDS:
            (pts, n, d), (lev, st) = rec[k]
            assert (n, d) == (T // P, 0)
            want, want_st = oracle_run(O, k, xs, ends)
            assert same(pts[s], want), (s, k)
            assert same(lev[s], want[-1]) and same(st[s], want_st[-1]), (s, k)
