"""sur_run for a batch (MTR_METER_SURROUND, mtr_surround.hip) against the composition of the oracle's Kmeterdsp and Stcorrdsp
restatements (tests/_sur.py; bit-identical to the reference build: tests/test_surround_cpu.py).

The oracle is the reference's f32 recurrences; the kernel re-associates the sums in double, so levels and correlations are not
bit-exact.  The yardsticks are those of tests/test_gpu_stcorr.py: per (stream, pair) D = max over the blocks of |oracle reading - a
float64 restatement of the same recurrence|, and the kernel must lie within 2 D + 4 * 2^-23 of the oracle — as far from exact as the
reference is, on the other side, plus the floor argued there; the five pair states likewise, relative to their scale.  `level` gets the
same construction per (stream, channel), relative to the reading: the float64 restatement of Kmeterdsp's two poles with the f32
roundings at the block ends gives D_rel, the bound is 2 D_rel + 4 * 2^-23 (z2 stored as f32, one multiply, one sqrt: under 4 ulp), and
with one sur_run per call also tests/test_gpu_kmeter.py's 1e-5.  `peak` is exact.  Every case prints its D and what it saw."""
import ctypes as C

import numpy as np
import pytest

import _sur

pytestmark = pytest.mark.gpu
FLOOR = _sur.FLOOR


@pytest.fixture(scope="module")
def M():
    import meters.lv2_amd as m
    return m


@pytest.fixture(scope="module")
def O(oracle):
    return _sur.bind(oracle.lib)


def calls_of(fs):
    # below one tile, not a multiple of 4, several pieces, a repeat (fall-back factor kept), no whole group, longer than a chunk
    return [1024, 1023, 3 * 4096 + 6, 3 * 4096 + 6, 1, 3, 2 * fs + 1, 512, fs]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def drive(e, x, calls, after=None, stride=None, pad=0):
    """x [S, T, W] on the device, call by call (stride: frames between the streams' rows, T + pad by default)"""
    import torch
    S, T, W = x.shape
    if pad:
        x = np.concatenate([x, np.full((S, pad, W), np.float32(7.0))], axis=1)
    dev = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    st = torch.cuda.current_stream().cuda_stream
    pos = 0
    for i, n in enumerate(calls):
        e.process_device(dev.data_ptr() + pos * W * 4, n, T + pad, st)
        pos += n
        if after:
            after(i)
    e.sync()
    del dev


def yardstick(M, O, fs, x, ends, pairs=None, reads=None):
    """oracle (level, peak, corr, states) as [B, S, ...] and the float64 restatement's (level, corr, states)"""
    per = [_sur.run_oracle(O, fs, x[s], ends, pairs, reads) for s in range(x.shape[0])]
    want = tuple(np.stack([p[k] for p in per], axis=1) for k in range(4))
    exact = _sur.run_exact(fs, M.stcorr_coef(float(fs)), x, ends, pairs, reads)
    return want, exact


def compare(tag, got, want, exact, at=None, tight=False):
    """got = (level, peak, corr, states or None) at the blocks `at` (all by default) of want / exact"""
    B = want[0].shape[0]
    at = list(range(B)) if at is None else list(at)
    w_level, w_peak, w_corr, w_st = want
    x_level, x_corr, x_st = exact
    level, peak, corr, st = got
    assert np.array_equal(bits(peak), bits(w_peak[at])), (tag, "peak", np.argwhere(bits(peak) != bits(w_peak[at]))[:4])
    # level: relative to the reading, D_rel per (stream, channel) over all blocks
    ok = np.isfinite(w_level) & np.isfinite(x_level)
    D = np.where(ok, _sur.rel(x_level, w_level, np.abs(w_level.astype(np.float64))), 0.0).max(axis=0)
    # (a level of exactly 0 — a flushed z2 — or one that is not finite — an Inf square in a block's last frame — has no relative distance:
    # there the kernel's bits are the oracle's)
    plain = np.isfinite(w_level[at]) & (w_level[at] != 0)
    assert np.array_equal(bits(level)[~plain], bits(w_level[at])[~plain]), (tag, "level 0 / not finite", np.argwhere(~plain & (bits(level) != bits(w_level[at])))[:4])
    assert np.all(np.isfinite(level[plain])), (tag, "level finite")
    with np.errstate(invalid="ignore"):
        d = np.where(plain, _sur.rel(np.where(plain, level, 0), np.where(plain, w_level[at], 0), np.abs(w_level[at].astype(np.float64))), 0.0)
    print(f"{tag} level: D_rel {D.max():.3g} seen {d.max():.3g}")
    assert np.all(d <= 2 * D[None] + FLOOR), (tag, "level", np.argwhere(d > 2 * D[None] + FLOOR)[:4], D.max(), d.max())
    if tight:
        assert np.all(d <= 1e-5), (tag, "level 1e-5", d.max())
    # corr: absolute, D per (stream, pair)
    Dc = np.abs(w_corr.astype(np.float64) - x_corr).max(axis=0)
    dc = np.abs(corr.astype(np.float64) - w_corr[at])
    print(f"{tag} corr: D {Dc.max():.3g} seen {dc.max():.3g}")
    assert np.all(np.isfinite(corr))
    assert np.all(dc <= 2 * Dc[None] + FLOOR), (tag, "corr", np.argwhere(dc > 2 * Dc[None] + FLOOR)[:4], Dc.max(), dc.max())
    if st is not None:
        Ds = _sur.rel(w_st, x_st, _sur.scale_of(x_st)).max(axis=(0, 3), keepdims=True)[0]      # per (stream, pair): over the blocks and the five states
        ds = _sur.rel(st, w_st[at], _sur.scale_of(w_st[at]))
        print(f"{tag} states: D_rel {Ds.max():.3g} seen {ds.max():.3g}")
        assert np.all(np.isfinite(st))
        assert np.all(ds <= 2 * Ds[None] + FLOOR), (tag, "states", np.argwhere(ds > 2 * Ds[None] + FLOOR)[:4], Ds.max(), ds.max())


CASES_1 = [(c, fs) for fs in (48000, 44100) for c in (3, 4, 5, 6, 7, 8)] + [(6, 192000), (6, 8000)]


@pytest.mark.parametrize("nch,fs", CASES_1)
def test_one_sur_run_per_call(M, O, nch, fs):
    S = 5
    calls = calls_of(fs)
    ends = np.cumsum(calls).tolist()
    reads = [0, 2, 3, 4, 6, 8]                                           # the host reads the ports after only some of the calls
    x = _sur.signals(ends[-1], fs, nch, S=S)
    rec = []
    with M.Engine(S, float(fs), M.METER_SURROUND, n_channels=nch) as e:
        assert e.surround_pairs() == _sur.default_pairs(nch)
        lv, pk, co = e.surround_read()
        assert not lv.any() and not pk.any() and not co.any() and not e.surround_pair_states().any()   # the constructors' state

        def after(i):
            if i in reads:
                st = e.surround_pair_states()
                rec.append(e.surround_read() + (st,))
        drive(e, x, calls, after)
        assert e.surround_series()[3:] == (0, 0)
    got = tuple(np.array([r[k] for r in rec]) for k in range(4))
    want, exact = yardstick(M, O, fs, x, ends, reads=set(reads))
    if nch == 3:
        assert not got[2][:, :, 3].any() and not got[3][:, :, 3].any()   # three pairs on three channels
    compare(f"C {nch} fs {fs} P 0", got, want, exact, at=reads, tight=True)


CASES_2 = [(nch, fs, P) for nch in (3, 6, 8) for fs, P in ((48000, 4800), (48000, 2407), (48000, 40000), (44100, 4410))]


@pytest.mark.parametrize("nch,fs,P", CASES_2)
def test_reading_series(M, O, nch, fs, P):
    """blocks of exactly P frames wherever the calls cut the audio: P mod 4 = 0, 3 (fs / 20 + 7), 0 (longer than a chunk), 2"""
    S = 5
    calls = [P // 2 - 3, 1] + calls_of(fs)                                 # a call shorter than P, a one-frame call, none aligned with P
    T = sum(calls)
    n = T // P
    ends = [P * (k + 1) for k in range(n)]
    x = _sur.signals(T, fs, nch, seed=501, S=S)
    cap = n - 2                                                            # a series shorter than the run
    with M.Engine(S, float(fs), M.METER_SURROUND, n_channels=nch) as e:
        e.surround_set_period(P, cap)
        drive(e, x, calls)
        lv, pk, co, n_points, dropped = e.surround_series()
        last = e.surround_read()
        again = e.surround_read()
    assert (n_points, dropped) == (n, 2) and lv.shape == (S, cap, nch) and co.shape == (S, cap, 4)
    for a, b in zip(last, again):
        assert np.array_equal(bits(a), bits(b))                            # with a period a read arms nothing
    want, exact = yardstick(M, O, fs, x[:, :n * P], ends)
    got = (np.concatenate([lv.transpose(1, 0, 2), last[0][None]]), np.concatenate([pk.transpose(1, 0, 2), last[1][None]]),
           np.concatenate([co.transpose(1, 0, 2), last[2][None]]), None)
    compare(f"C {nch} fs {fs} P {P}", got, want, exact, at=list(range(cap)) + [n - 1])


@pytest.mark.parametrize("fs,P", [(48000, 2407), (44100, 4410)])
def test_calls_that_end_in_the_dropped_frames(M, O, fs, P):
    """P mod 4 = 3 and 2: Kmeterdsp drops a block's last P mod 4 frames, z1 does not run over them.  One call ends at block offset P - 1,
    one at P - 2, and one-frame calls lie wholly inside the dropped frames; the calls add up to six whole blocks, so the pair states stand
    at a block end and are held to the oracle's as well."""
    nch, S = 6, 5
    calls = [P - 1, 1, 2 * P - 2, 1, 1, 1000, 3 * P - 1000]
    assert P % 4 and (P - 2) >= (P & ~3) and sum(calls) == 6 * P
    n = 6
    ends = [P * (k + 1) for k in range(n)]
    x = _sur.signals(n * P, fs, nch, seed=511, S=S)
    with M.Engine(S, float(fs), M.METER_SURROUND, n_channels=nch) as e:
        e.surround_set_period(P, n)
        drive(e, x, calls)
        lv, pk, co, n_points, dropped = e.surround_series()
        last = e.surround_read()
        st = e.surround_pair_states()
    assert (n_points, dropped) == (n, 0)
    want, exact = yardstick(M, O, fs, x, ends)
    compare(f"dropped frames fs {fs} P {P}", (lv.transpose(1, 0, 2), pk.transpose(1, 0, 2), co.transpose(1, 0, 2), None), want, exact)
    compare(f"dropped frames fs {fs} P {P} end", (last[0][None], last[1][None], last[2][None], st[None]), want, exact, at=[n - 1])


def test_pairs(M, O):
    """a shared channel, clamped entries, a == b; a change between two calls carries the PAIR's states on"""
    fs, nch, S = 48000, 6, 5
    calls = [5000, 7001, 3000, 9000]
    ends = np.cumsum(calls).tolist()
    x = _sur.signals(ends[-1], fs, nch, seed=502, S=S)
    p0 = ((0, 0, 0, 5), (1, 2, 0, 0))                                      # (0,1) (0,2) (0,0) (5,0)
    p1 = ((4, 9, 3, 2), (7, 1, 3, 200))                                    # entries >= C: clamped to 5
    pairs = [p0, p0, p1, p1]
    rec = []
    with M.Engine(S, float(fs), M.METER_SURROUND, n_channels=nch) as e:
        e.surround_set_pairs(*p0)
        assert e.surround_pairs() == p0

        def after(i):
            st = e.surround_pair_states()
            rec.append(e.surround_read() + (st,))
            if i == 1:
                e.surround_set_pairs(*p1)
                assert e.surround_pairs() == ((4, 5, 3, 2), (5, 1, 3, 5))
        drive(e, x, calls, after)
        e.reset()
        assert e.surround_pairs() == ((4, 5, 3, 2), (5, 1, 3, 5))          # a control: it survives a reset
    got = tuple(np.array([r[k] for r in rec]) for k in range(4))
    want, exact = yardstick(M, O, fs, x, ends, pairs=pairs)
    compare("pairs P 0", got, want, exact, tight=True)
    assert np.all(np.abs(got[2][:2, :, 2] - 1) < 1e-4)                     # (0,0): a channel with itself
    # with a period: refused while a block is open, accepted on a boundary
    P = 4800
    calls = [P + 100, P - 100, 2 * P + 50, 4 * P - 50]
    T = sum(calls)
    x = _sur.signals(T, fs, nch, seed=503, S=S)
    with M.Engine(S, float(fs), M.METER_SURROUND, n_channels=nch) as e:
        e.surround_set_period(P, 16)
        e.surround_set_pairs(*p0)

        def after(i):
            if i == 0:
                a, b = np.array(p1[0], np.uint8), np.array(p1[1], np.uint8)
                assert M.lib.mtr_engine_surround_set_pairs(e._h, a.ctypes.data, b.ctypes.data) == M.engine.ERR_STATE
                assert e.surround_pairs() == p0
            if i == 1:
                e.surround_set_pairs(*p1)                                  # two blocks done, none open
        drive(e, x, calls, after)
        lv, pk, co, n, d = e.surround_series()
    assert (n, d) == (T // P, 0)
    want, exact = yardstick(M, O, fs, x, [P * (k + 1) for k in range(n)], pairs=[p0, p0] + [p1] * (n - 2))
    compare("pairs P 4800", (lv.transpose(1, 0, 2), pk.transpose(1, 0, 2), co.transpose(1, 0, 2), None), want, exact)


@pytest.mark.parametrize("P,cuts", [(0, "long calls"), (0, "host blocks"), (4800, "long calls"), (4800, "host blocks")])
def test_not_finite(M, O, P, cuts):
    """A NaN in channel 2 and an Inf in channel 4 of one stream: the affected channels and every pair touching them follow the
    reference's flush rules block by block; the other channels, pairs and streams are those of a run without them, to the bit."""
    fs, nch, S, Q = 48000, 6, 5, 4800
    T = 12 * Q + 700
    if cuts == "long calls":
        calls = [3 * Q + 100, 2 * Q + 1300, 1024, 1024, 1024, 1024, 1024, 3000, T - (5 * Q + 1400 + 5 * 1024 + 3000)]
    else:
        calls = [1024] * (T // 1024) + [T % 1024]
    assert sum(calls) == T
    clean = _sur.signals(T, fs, nch, seed=504, S=S)
    x = clean.copy()
    x[1, Q + 2000, 2] = np.nan                                             # a block that closes in the middle of call 0
    x[1, 5 * Q + 1350, 4] = np.inf                                         # the block open at the end of call 1 (long calls)
    x[1, 8 * Q - 2, 2] = np.nan                                            # a block's last group
    x[1, 9 * Q, 4] = -np.inf                                               # a block's first frame
    ends = [P * (k + 1) for k in range(T // P)] if P else np.cumsum(calls).tolist()
    # ... and an Inf in the last frame Kmeterdsp takes of the block that holds frame 6 Q + 100 (none of the others lies in it): there z1
    # and z2 end as Inf, not NaN — the level reads Inf, the next block starts from the clamp at 50
    k6 = int(np.searchsorted(ends, 6 * Q + 100, side="right"))
    b6 = ends[k6 - 1] if k6 else 0
    last_taken = b6 + ((ends[k6] - b6) & ~3) - 1
    assert np.isfinite(x[1, b6:ends[k6]]).all()
    x[1, last_taken, 4] = np.inf
    runs = []
    for src in (x, clean):
        rec = []
        with M.Engine(S, float(fs), M.METER_SURROUND, n_channels=nch) as e:
            e.surround_set_period(P, len(ends))
            drive(e, src, calls, (lambda i: rec.append(e.surround_read() + (e.surround_pair_states(),))) if not P else None)
            if P:
                lv, pk, co, n, _ = e.surround_series()
                assert n == len(ends)
                runs.append((lv.transpose(1, 0, 2), pk.transpose(1, 0, 2), co.transpose(1, 0, 2), None))
            else:
                runs.append(tuple(np.array([r[k] for r in rec]) for k in range(4)))
    got, base = runs
    pairs_hit = [1, 2]                                                     # the default pairs (2,3) and (4,5)
    for k in range(3):
        a, b = got[k].copy(), base[k].copy()
        if k < 2:
            a[:, 1, [2, 4]] = 0; b[:, 1, [2, 4]] = 0
        else:
            a[:, 1, pairs_hit] = 0; b[:, 1, pairs_hit] = 0
        assert np.array_equal(bits(a), bits(b)), ("untouched", k)
    assert not np.array_equal(bits(got[0][:, 1, 2]), bits(base[0][:, 1, 2])) and not np.array_equal(bits(got[2][:, 1, 1]), bits(base[2][:, 1, 1]))
    want, exact = yardstick(M, O, fs, x[:, :ends[-1]], ends)
    # the flushes themselves: where the oracle's level is exactly 0 (z2 flushed), so is the kernel's
    assert (want[0][:, 1, [2, 4]] == 0).any()
    assert np.array_equal(got[0] == 0, want[0] == 0)
    assert np.isinf(want[0][k6, 1, 4]) and np.isfinite(np.delete(want[0], k6, axis=0)).all()
    compare(f"not finite P {P} {cuts}", got, want, exact, tight=not P)


def test_deterministic_and_slot_independent(M):
    fs, nch, S, P = 48000, 6, 6, 4807
    calls = calls_of(fs)[:6] + [30000]
    x = _sur.signals(sum(calls), fs, nch, seed=505, S=S)
    perm = [3, 0, 5, 1, 4, 2]

    def run(src):
        with M.Engine(S, float(fs), M.METER_SURROUND, n_channels=nch) as e:
            e.surround_set_period(P, 64)
            drive(e, src, calls)
            full = e.surround_series()[:3] + e.surround_read() + (e.surround_pair_states(),)
            part = e.surround_series(2, 3)[:3] + e.surround_read(2, 3) + (e.surround_pair_states(2, 3),)
        for f, p in zip(full, part):
            assert np.array_equal(bits(f[2:5]), bits(p))                   # first / count
        return full
    a, b, c = run(x), run(x), run(np.ascontiguousarray(x[perm]))
    for u, v, w in zip(a, b, c):
        assert np.array_equal(bits(u), bits(v))
        assert np.array_equal(bits(u[perm]), bits(w))                      # a stream's results do not depend on its slot
    assert a[0].any() and a[2].any()


def _record(e):
    return list(e.surround_series()) + list(e.surround_read()) + [e.surround_pair_states()]


def _same(a, b):
    for u, v in zip(a, b):
        assert np.array_equal(bits(u) if isinstance(u, np.ndarray) else u, bits(v) if isinstance(v, np.ndarray) else v)


@pytest.mark.parametrize("P", [0, 4807])
def test_every_way_in_is_the_device_call(M, P):
    fs, nch, S = 48000, 6, 5
    calls = [30000, 5001, 20000]
    T = sum(calls)
    x = _sur.signals(T, fs, nch, seed=506, S=S)
    q16 = np.clip(np.rint(x * 32767.0), -32768, 32767).astype(np.int16)
    q32 = (q16.astype(np.int32) << 16) + 12345
    q24 = np.ascontiguousarray((q16.astype(np.int32) << 8) + 77).astype("<i4").view(np.uint8).reshape(S, T, nch, 4)[..., :3].reshape(S, T * nch * 3)
    wide = np.random.default_rng(4).uniform(-1, 1, (S, T, 8)).astype(np.float32)
    pick = [6, 1, 0, 3, 7, 4]
    wide[:, :, pick] = x
    wave = np.ascontiguousarray(x[:, :, [0, 1, 2, 5, 3, 4]])               # L R C LFE Ls Rs of x = L R C Ls Rs LFE
    assert np.array_equal(M.pick_decode(0, wide, pick), x) and np.array_equal(M.pick_decode(0, wave, [0, 1, 2, 4, 5, 3]), x)

    def run(feed, src, layout=None, **kw):
        with M.Engine(S, float(fs), M.METER_SURROUND, n_channels=nch) as e:
            e.surround_set_period(P, 16)
            if layout:
                e.set_frame_layout(*layout)
            e.set_host_chunk_bytes(2 * 30000 * nch * 4)                     # two streams of the longest call per chunk
            if feed == "device":
                drive(e, src, calls, **kw)
            else:
                pos = 0
                for n in calls:
                    w = src.shape[1] // T
                    getattr(e, feed)(np.ascontiguousarray(src[:, pos * w:(pos + n) * w]), **kw)
                    pos += n
            return _record(e)
    base = run("device", x)
    assert base[3] == (T // P if P else 0)
    _same(base, run("process", x))                                         # host memory, chunks that split the batch
    _same(base, run("device", x, pad=37))                                  # rows further apart than the call is long
    _same(base, run("device", wide, (8, pick)))                            # six of eight
    _same(base, run("process", wide, (8, pick)))
    _same(base, run("device", wave, (6, [0, 1, 2, 4, 5, 3])))              # a WAVE 5.1 file reordered
    for fmt, q in ((M.PCM_S16, q16), (M.PCM_S32, q32)):
        _same(run("device", M.pcm_decode(fmt, q)), run("process_pcm", q))
    _same(run("device", M.pcm_decode(M.PCM_S24, q24).reshape(S, T, nch)), run("process_pcm", q24, format=M.PCM_S24))
    # planar host memory: the one-stream path
    with M.Engine(1, float(fs), M.METER_SURROUND, n_channels=nch) as e:
        e.surround_set_period(P, 16)
        pos = 0
        for n in calls:
            e.process_planar([x[2, pos:pos + n, c] for c in range(nch)])
            pos += n
        one = _record(e)
    with M.Engine(1, float(fs), M.METER_SURROUND, n_channels=nch) as e:
        e.surround_set_period(P, 16)
        drive(e, x[2:3], calls)
        _same(one, _record(e))
    _same([b[2:3] if isinstance(b, np.ndarray) else b for b in base], one)


@pytest.mark.parametrize("layout", [None, (6, [0, 1, 2, 4, 5])])
def test_beside_the_loudness_meters(M, layout):
    """EBU | TRUEPEAK | SURROUND on five channels against two engines holding the halves: bit for bit.  With the WAVE 5.1 layout the
    engine that carries SURROUND stages the call (k_pick) where the other reads the wide frames itself: exactly that moves."""
    fs, nch, S, P = 48000, 5, 4, 4800
    calls = [P * 3 + 7, 24000, 1000, 48000]
    x = _sur.signals(sum(calls), fs, nch, seed=507, S=S)
    src = x
    if layout:
        src = np.random.default_rng(8).uniform(-1, 1, (S, x.shape[1], 6)).astype(np.float32)
        src[:, :, layout[1]] = x
    E, T, SUR = M.METER_EBU, M.METER_TRUEPEAK, M.METER_SURROUND
    rec = {}
    for name, meters in (("all", E | T | SUR), ("ebu", E | T), ("sur", SUR)):
        with M.Engine(S, float(fs), meters, n_channels=nch) as e:
            if meters & E:
                e.integr_start()
            if meters & SUR:
                e.surround_set_period(P, 32)
            if layout:
                e.set_frame_layout(*layout)
            drive(e, src, calls)
            r = {}
            if meters & E:
                hold, last = e.truepeak_channels()
                r.update(out9=e.out9(), hold=hold, last=last, hm=e.histograms()[0], hs=e.histograms()[1])
            if meters & SUR:
                r.update({f"s{k}": v for k, v in enumerate(_record(e))})
            stats = e.layout_stats()
        rec[name] = (r, stats)
    for k, v in list(rec["ebu"][0].items()) + list(rec["sur"][0].items()):
        w = rec["all"][0][k]
        assert np.array_equal(bits(v), bits(w)) if isinstance(v, np.ndarray) and v.dtype == np.float32 else np.array_equal(v, w), k
    assert rec["all"][0]["s3"] == sum(calls) // P
    n = len(calls)
    if layout:
        assert rec["ebu"][1] == (0, n) and rec["all"][1] == (n, 0) and rec["sur"][1] == (n, 0)
    else:
        assert rec["ebu"][1] == (0, 0) and rec["all"][1] == (0, 0)


def test_state_travels(M):
    """Export in the middle of a block, import into another engine at other slots: the continuation is bit for bit the uninterrupted
    run's.  Pairs, period and fill ride in the blob; the series does not."""
    fs, nch, S, P = 48000, 6, 4, 4800
    calls, k_stop = [5000, 7000, 9000, 4800, 1234], 2
    T = sum(calls)
    x = _sur.signals(T, fs, nch, seed=508, S=S)
    prs = ((0, 0, 5, 2), (1, 3, 4, 2))
    with M.Engine(S, float(fs), M.METER_SURROUND, n_channels=nch) as e:
        e.surround_set_period(P, 64)
        e.surround_set_pairs(*prs)
        drive(e, x, calls)
        want = _record(e)
    done = sum(calls[:k_stop])
    assert done % P
    with M.Engine(S, float(fs), M.METER_SURROUND, n_channels=nch) as e:
        e.surround_set_period(P, 64)
        e.surround_set_pairs(*prs)
        drive(e, x[:, :done], calls[:k_stop])
        blob = e.state_export()
        assert e.state_bytes(S) == len(blob)
        assert M.lib.mtr_engine_state_import(e._h, 0, blob, len(blob)) == 0                 # it stands where the blob does
        e.process(np.zeros((S, 100, nch), np.float32))
        assert M.lib.mtr_engine_state_import(e._h, 0, blob, len(blob)) == M.engine.ERR_STATE   # ... and now elsewhere in its block
    with M.Engine(S, float(fs), M.METER_SURROUND, n_channels=nch) as e:                    # another period
        e.process(np.zeros((S, done, nch), np.float32))
        assert M.lib.mtr_engine_state_import(e._h, 0, blob, len(blob)) == M.engine.ERR_STATE
    rest = np.zeros((S + 3, T - done, nch), np.float32)
    rest[2:2 + S] = x[:, done:]
    # a fresh engine takes period, fill and pairs from the blob
    with M.Engine(S + 3, float(fs), M.METER_SURROUND, n_channels=nch) as e:
        e.surround_set_period(0, 0)
        assert e.state_import(blob, first=2) == S
        assert e.surround_pairs() == prs
        drive(e, rest, calls[k_stop:])
        lv, pk, co, n, d = e.surround_series(2, S)
        got = list(e.surround_read(2, S)) + [e.surround_pair_states(2, S)]
    assert (n, d) == (want[3] - done // P, want[3] - done // P)            # (it has no series to hold them)
    _same(want[5:], got)
    with M.Engine(S + 3, float(fs), M.METER_SURROUND, n_channels=nch) as e:
        e.surround_set_period(P, 64)
        e.surround_set_pairs(*prs)
        assert e.state_import(blob, first=2) == S
        drive(e, rest, calls[k_stop:])
        lv, pk, co, n, d = e.surround_series(2, S)
        got = list(e.surround_read(2, S)) + [e.surround_pair_states(2, S)]
    assert (n, d) == (want[3] - done // P, 0)
    for k, v in enumerate((lv, pk, co)):
        assert np.array_equal(bits(v), bits(want[k][:, done // P:]))
    _same(want[5:], got)


def test_blobs_without_the_bit_keep_their_size_and_bytes(M):
    """mtr_stream_state 408, the two histograms 2 * 751 * 4, the FIR history 47 * 2 * 4 per stream behind a header of 64 bytes; layout 8
    adds C * (4 + 47 + 1 + 1) floats; SURROUND appends its 440 bytes per stream to an engine that has the bit, nothing to any other"""
    base = 408 + 2 * 751 * 4 + 47 * 2 * 4
    E, T, SUR = M.METER_EBU, M.METER_TRUEPEAK, M.METER_SURROUND
    for nch, meters, per in ((2, E | T, base), (2, M.METER_KMETER | M.METER_STCORR, base + 48 + 32), (5, E | T, base + 5 * 53 * 4),
                             (5, E | T | SUR, base + 5 * 53 * 4 + 440), (8, SUR, base + 440), (3, SUR, base + 440)):
        with M.Engine(3, 48000.0, meters, n_channels=nch) as e:
            assert e.state_bytes(3) == 64 + 3 * per, (nch, meters, e.state_bytes(3))
            assert e.state_bytes(0) == 64
    x = _sur.signals(9000, 48000, 5, seed=509, S=3)
    blobs = []
    for meters in (E | T, E | T | SUR):
        with M.Engine(3, 48000.0, meters, n_channels=5) as e:
            e.process(x)
            blobs.append(e.state_export())
    a, b = blobs
    assert len(b) == len(a) + 3 * 440 and a[64:] == b[64:len(a)]           # (the headers differ: meters mask, checksum)


def test_refusals_and_reset(M):
    fs, nch, S = 48000, 6, 3
    x = _sur.signals(20000, fs, nch, seed=510, S=S)
    E = M.engine
    with M.Engine(S, float(fs), M.METER_SURROUND | M.METER_EBU, n_channels=5) as e:
        import torch
        x5 = np.ascontiguousarray(x[:, :, :5])
        with pytest.raises(M.EngineError) as err:
            e.process_lengths(x5, [20000, 100, 5])
        assert err.value.code == E.ERR_UNSUPPORTED
        dev = torch.from_numpy(x5).cuda()
        with pytest.raises(M.EngineError) as err:
            e.process_device_lengths(dev.data_ptr(), 20000, [20000, 100, 5])
        assert err.value.code == E.ERR_UNSUPPORTED
        with pytest.raises(M.EngineError) as err:
            e.process_pcm(np.zeros((S, 100, 5), np.int16), frames=[100, 100, 5])
        assert err.value.code == E.ERR_UNSUPPORTED
    with M.Engine(S, float(fs), M.METER_EBU, n_channels=5) as e:             # an engine without the bit has no such meter
        a = np.zeros(4, np.uint8)
        assert M.lib.mtr_engine_surround_reset(e._h) == E.ERR_ARG
        assert M.lib.mtr_engine_surround_set_period(e._h, 0, 0) == E.ERR_ARG
        assert M.lib.mtr_engine_surround_set_pairs(e._h, a.ctypes.data, a.ctypes.data) == E.ERR_ARG
    with M.Engine(S, float(fs), M.METER_SURROUND, n_channels=nch) as e:
        for bad in (1, fs // 20 - 1):
            assert M.lib.mtr_engine_surround_set_period(e._h, bad, 4) == E.ERR_ARG
        e.surround_set_period(fs // 20, 4)
        e.process(x)
        assert M.lib.mtr_engine_surround_set_period(e._h, 4800, 4) == E.ERR_STATE      # it has processed
        assert M.lib.mtr_engine_surround_read(e._h, 0, S + 1, None, None, None) == E.ERR_ARG
        assert M.lib.mtr_engine_surround_read(e._h, 0, S, None, None, None) == 0        # any of the three may be NULL
    prs = ((0, 2, 4, 1), (1, 3, 5, 1))
    for whole in (False, True):
        with M.Engine(S, float(fs), M.METER_SURROUND, n_channels=nch) as e:
            e.surround_set_period(2400, 16)
            e.surround_set_pairs(*prs)
            e.process(x)
            first = _record(e)
            assert first[3] == 8 and first[0].any() and first[5].any() and first[8].any()
            e.reset() if whole else e.surround_reset()
            lv, pk, co, n, d = e.surround_series()
            assert (n, d) == (0, 0) and lv.shape == (S, 0, nch)
            assert not any(v.any() for v in e.surround_read()) and not e.surround_pair_states().any()
            assert e.surround_pairs() == prs
            e.process(x)                                                    # ... period and pairs kept: the same points again
            _same(first, _record(e))


def test_known_answer(M):
    """a full-scale 1 kHz sine in all six channels, channel 1 inverted: every K-meter reads 1.0 (sqrt (2 <x^2>)), pair (0,1) -1, (2,3) +1"""
    fs, nch, S = 48000, 6, 2
    t = np.arange(3 * fs) / fs
    x = np.repeat(np.sin(2 * np.pi * 1000.0 * t).astype(np.float32)[None, :, None], nch, axis=2).repeat(S, axis=0)
    x[:, :, 1] *= -1
    with M.Engine(S, float(fs), M.METER_SURROUND, n_channels=nch) as e:
        e.process(np.ascontiguousarray(x))
        level, peak, corr = e.surround_read()
    assert np.all(np.abs(level - 1.0) < 1e-3), level
    assert np.all(np.abs(peak - 1.0) < 1e-4), peak
    assert np.all(corr[:, 0] < -0.999) and np.all(corr[:, 1] > 0.999), corr
