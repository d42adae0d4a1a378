"""The goniometer's oversampling on the GPU (include/mtr_gonio_os.h: mtr_engine_gonio_set_oversample; k_gonio_os and k_history's 23-frame rows in front of
and behind k_gonio_points / k_gonio_image) against the restatement of tests/_gonio_os.py, which tests/test_gonio_os_cpu.py holds to the
reference's Resampler.

Every comparison is equality of BYTES, as in tests/test_gpu_gonio.py: images, the three counters, gain / lp / last point, the series and
the blocks (every NaN as one pattern, as tests/test_gpu_gonio_ends.py compares them).  Every test on the signal set first asserts, on the
restatement alone, the guard of _gonio.coverage and that for some stream the factor-f image is not the factor-1 image of the same audio:
an engine that accepts the factor and ignores it cannot pass."""
import numpy as np
import pytest

import _gonio
import _gonio_ends as GE
import _gonio_os as OS

pytestmark = pytest.mark.gpu
FS = 48000.0
U32 = np.uint32
CALLS = [1, 5, 17, 22, 23, 24, 255, 1000, 3653]      # calls shorter than, as long as and one longer than the history row
SMALL = [1, 22, 23, 24, 430, 1000]


@pytest.fixture(scope="module")
def M():
    import meters.lv2_amd as m
    return m


_sig, _ref = {}, {}


def signal(S, T, seed=1):
    if (S, T, seed) not in _sig:
        _sig[(S, T, seed)] = _gonio.signals(S, T, FS, seed)
        _sig[(S, T, seed)].setflags(write=False)
    return _sig[(S, T, seed)]


def shared(key, make):
    """a restatement, computed once, shared, never changed"""
    if key not in _ref:
        _ref[key] = make()
    return _ref[key]


def reference(S, T, f, seed=1, **kw):
    """the restatement over the whole of signal (S, T, seed) at factor f (1: tests/_gonio.py as it is)"""
    def make():
        return (_gonio.Gonio(S, FS, **kw) if f == 1 else OS.GonioOS(S, FS, f, **kw)).run(signal(S, T, seed))
    return shared(("dense", S, T, f, seed, tuple(sorted(kw.items()))), make)


def guard(S, T, f, seed=1, **kw):
    """on the restatement alone: the signal set meets every rule, and the factor shows in some stream's image"""
    ref, one = reference(S, T, f, seed, **kw), reference(S, T, 1, seed, **kw)
    _gonio.coverage(ref, T * f)
    assert (ref.img != one.img).reshape(S, -1).any(axis=1).any(), "the factor-f image is the factor-1 image in every stream"
    assert (ref.drawn + ref.clipped + ref.skipped == T * f).all()
    return ref


def engine(M, S, f, meters=None, **cfg):
    e = M.Engine(S, FS, M.METER_GONIO if meters is None else meters)
    e.gonio_configure(**cfg)
    if f is not None:
        e.gonio_set_oversample(f)
    return e


def device(x):
    import torch
    return torch.from_numpy(np.array(x, np.float32, copy=True)).cuda()


def feed(e, x, calls=None):
    dev = device(x)
    T = x.shape[1]
    pos = 0
    for n in calls or [T]:
        e.process_device(dev.data_ptr() + pos * 8, n, T)
        pos += n
    assert pos == T
    e.sync()


def bits(a):
    a = np.ascontiguousarray(a, np.float32)
    return np.where(np.isnan(a), np.float32(np.nan), a).view(U32)


def snap(e):
    img, drawn, clipped, skipped = e.gonio_image()
    gain, lp, last = e.gonio_read()
    sg, sd, sc = e.gonio_series()
    return dict(img=img, drawn=drawn, clipped=clipped, skipped=skipped, gain=bits(gain), lp=bits(lp), last=bits(last),
                s_gain=bits(sg), s_drawn=sd, s_clipped=sc, blocks=np.array(e.gonio_blocks()))


def want(g, cap=None):
    sg, sd, sc = g.series_arrays()
    n = sg.shape[1]
    k = n if cap is None else min(n, cap)
    return dict(img=g.img, drawn=g.drawn, clipped=g.clipped, skipped=g.skipped, gain=bits(g.gain),
                lp=bits(np.stack([g.lp0, g.lp1], axis=1)), last=bits(np.stack([g.last_x, g.last_y], axis=1)),
                s_gain=bits(sg[:, :k]), s_drawn=sd[:, :k], s_clipped=sc[:, :k], blocks=np.array([n, k]))


def same(a, b, rows=None, skip=()):
    for k in a:
        if k in skip or k not in b:
            continue
        x, y = (a[k], b[k]) if rows is None or k == "blocks" else (a[k][rows], b[k][rows])
        assert x.shape == y.shape, (k, x.shape, y.shape)
        bad = np.argwhere(np.asarray(x != y))[:6]
        assert not len(bad), (k, bad.tolist(), [(x[tuple(i)], y[tuple(i)]) for i in bad])


# ---- 1: fixed gain, cuts shorter than the history, every way in ------------------------------------------------------------------------
def test_fixed_gain_factor_4_bit_for_bit_however_the_audio_is_cut(M):
    S, T, f = 67, 5000, 4                                                  # a wave of 64 plus three; pieces of 1024 / 4 = 256 input frames
    ref = guard(S, T, f, P=480, gain=1.0)
    x, w = signal(S, T), want(ref)
    cfg = dict(period_frames=480, capacity=16, gain=1.0, tune_piece=1024)
    with engine(M, S, f, **cfg) as e:
        assert e.gonio_oversample() == (f, OS.hpw(FS, f)) and bits(e.gonio_config()[1].hpw) == bits(_gonio.derive(FS).hpw)
        feed(e, x, CALLS)
        cut = snap(e)
    same(cut, w)
    assert cut["blocks"].tolist() == [10, 10] and (cut["img"].reshape(S, -1).sum(axis=1, dtype=np.uint64) == cut["drawn"]).all()
    with engine(M, S, f, **cfg) as e:
        feed(e, x)
        same(snap(e), cut)
    with engine(M, S, f, **cfg) as e:
        e.process(x)
        same(snap(e), cut)
    with engine(M, S, f, **cfg) as e:                                      # the host path in views of the batch (two chunks of streams per call), two calls
        e.set_host_chunk_bytes(20 * T * 8)
        e.process(x[:, :2401])
        e.process(x[:, 2401:])
        same(snap(e), cut)


def test_fixed_gain_factor_3_pieces_of_an_odd_count_of_points(M):
    S, T, f = 67, 5000, 3                                                  # pieces of 1024 / 3 = 341 input frames = 1023 points
    ref = guard(S, T, f, P=480, gain=4.0)
    cfg = dict(period_frames=480, capacity=16, gain=4.0, tune_piece=1024)
    with engine(M, S, f, **cfg) as e:
        feed(e, signal(S, T), CALLS)
        same(snap(e), want(ref))
    with engine(M, S, f, **cfg) as e:
        e.process(signal(S, T))
        same(snap(e), want(ref))


@pytest.mark.parametrize("f", [2, 32])
def test_fixed_gain_the_smallest_and_the_largest_factor(M, f):
    S, T = 19, 1500                                                        # f = 32: 48 000 serial steps of the restatement; pieces of 32 input frames
    ref = guard(S, T, f, P=480, gain=4.0)
    cfg = dict(period_frames=480, capacity=8, gain=4.0, tune_piece=1024)
    with engine(M, S, f, **cfg) as e:
        feed(e, signal(S, T), SMALL)
        got = snap(e)
    same(got, want(ref))
    assert got["blocks"].tolist() == [3, 3]
    with engine(M, S, f, **cfg) as e:
        feed(e, signal(S, T))
        same(snap(e), got)


# ---- 2: auto gain ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [0, 100])
def test_auto_gain_series_bit_for_bit(M, P):
    S, T, f = 19, 9600, 4
    ref = guard(S, T, f, seed=2, P=P, autogain=True)
    with engine(M, S, f, period_frames=P, capacity=128 if P else 0, autogain=1) as e:
        assert e.gonio_config()[1].period_frames == (P or 1920)
        feed(e, signal(S, T, 2), [4097, 5503])
        got = snap(e)
    same(got, want(ref))
    assert got["blocks"][0] == T // (P or 1920)
    assert np.array_equal(got["s_gain"][:, -1], got["gain"])               # T is a whole number of blocks: the last point is the gain
    assert len(np.unique(got["s_gain"][0])) > 3                            # (it moved)


# ---- 3: track lengths -------------------------------------------------------------------------------------------------------------------
ES, ET, EC = 37, 5000, [2600, 2400]


def planted(P):
    """[37] ends: open; 0; inside the first 23 frames of the second call (three places); r = 63; r = 64; on a block's end, in either call;
    on either call's last frame; on the second call's first; seeded random ends for the rest"""
    C1 = EC[0]
    e = np.random.default_rng(36).integers(0, ET + 1, ES).astype(np.uint64)
    e[:16] = [ET, 0, C1 + 10, P + 63, P + 64, P, 3840, C1 - 1, ET - 1, C1, C1 + 22, C1 + 23, C1 + 24, ET, 1, 2 * P + 200]
    return e


def ref_ends(P, autogain):
    return shared(("ends", P, autogain), lambda: OS.run_ends(signal(ES, ET, 3), planted(P), FS, 4, calls=EC, P=P, autogain=bool(autogain)))


def snap_ends(e):
    up, pt = e.gonio_points()
    return dict(snap(e), updates=up, points=pt)


def want_ends(o, cap):
    k = min(o.blocks, cap)
    return dict(img=o.img, drawn=o.drawn, clipped=o.clipped, skipped=o.skipped, gain=bits(o.gain),
                lp=bits(np.stack([o.lp0, o.lp1], axis=1)), last=bits(np.stack([o.last_x, o.last_y], axis=1)),
                s_gain=bits(o.s_gain[:, :k]), s_drawn=o.s_drawn[:, :k], s_clipped=o.s_clipped[:, :k],
                blocks=np.array([o.blocks, k]), updates=o.updates, points=o.updates)


@pytest.mark.parametrize("P", [0, 480])
def test_track_lengths_each_track_is_its_own_frames_alone(M, P):
    f, ends, x = 4, planted(P or 1920), signal(ES, ET, 3)
    o = ref_ends(P or 1920, 1)
    PP = o.P
    # the guard, on the restatement alone
    _gonio.coverage(o, ET * f)
    assert (o.r >= GE.FLOOR).any() and o.painted.any(), "no closing update painted"
    assert int(o.r[4]) == 64 and int(o.r[3]) == 0 and int(o.stand[3]) == PP and int(o.stand[5]) == PP and int(o.stand[1]) == 0
    assert int(o.stand[9]) == EC[0] and int(o.r[9]) == 0 and int(o.stand[7]) == EC[0] - 1 and int(o.r[7]) >= 64 and int(o.stand[14]) == 0
    dense1 = shared(("ends1", PP), lambda: _gonio.Gonio(ES, FS, P=PP, autogain=True).run(x))
    open_ = np.nonzero(ends == ET)[0]
    assert (o.img[open_] != dense1.img[open_]).any(), "the factor-4 image is the factor-1 image"
    # a few tracks fed their own frames alone: the lock-step pass is that
    for s in (3, 4, 14):
        t = OS.track(x[s], int(o.stand[s]), int(o.r[s]), FS, f, P=PP, autogain=True)
        assert np.array_equal(t.img[0], o.img[s]) and bits(t.gain)[0] == bits(o.gain)[s] and t.drawn[0] == o.drawn[s] and t.skipped[0] == o.skipped[s], s
        assert bits(t.lp0)[0] == bits(o.lp0)[s] and bits(t.last_x)[0] == bits(o.last_x)[s] and len(t.series) == o.updates[s], s
    w = want_ends(o, 16)
    cfg = dict(period_frames=P, capacity=16 if P else 0, autogain=1, tune_piece=1024)
    if not P:
        w = want_ends(o, 4096)
    dev = device(x)

    def run(e, host):
        pos = 0
        for n in EC:
            fr = np.clip(ends.astype(np.int64) - pos, 0, n).astype(np.uint64)
            if host:
                e.process_gonio_ends(x[:, pos:pos + n], fr)
            else:
                e.process_device_gonio_ends(dev.data_ptr() + pos * 8, n, fr, ET)
            pos += n
        e.sync()
    with engine(M, ES, f, **cfg) as e:
        run(e, False)
        got = snap_ends(e)
        same(got, w)
        assert np.array_equal(e.stream_frames()[1].astype(bool), ends < ET)
    with engine(M, ES, f, **cfg) as e:
        e.set_host_chunk_bytes(10 * 2600 * 8)                              # views of the batch
        run(e, True)
        same(snap_ends(e), got)


# ---- 4: state ---------------------------------------------------------------------------------------------------------------------------
def test_state_travels_with_the_history(M):
    S, T, CUT, f = 9, 3000, 1234, 4                                        # 1234 = 2 * 480 + 274: inside a block
    ref = guard(S, T, f, seed=5, P=480, autogain=True)
    x, w = signal(S, T, 5), want(ref)
    cfg = dict(period_frames=480, capacity=8, autogain=1)
    with engine(M, S, f, **cfg) as a, engine(M, S, f, **cfg) as b:
        feed(a, x[:, :CUT])
        blob = a.state_export()
        assert len(blob) == a.state_bytes(S)
        assert b.state_import(blob) == S
        feed(b, x[:, CUT:])
        got = snap(b)
        same(got, w, skip=("s_gain", "s_drawn", "s_clipped", "blocks"))
        assert got["blocks"].tolist() == [4, 4]
        for k in ("s_gain", "s_drawn", "s_clipped"):
            assert np.array_equal(got[k], w[k][:, 2:]), k
        for other in (2, 1, None):                                         # another factor, factor 1 told, never told: not this blob's engine
            with engine(M, S, other, **cfg) as c:
                with pytest.raises(M.EngineError) as ei:
                    c.state_import(blob)
                assert ei.value.code == M.engine.ERR_STATE
    # an engine told factor 1 exports what an engine never told exports
    with engine(M, S, 1, **cfg) as a, engine(M, S, None, **cfg) as b, engine(M, S, f, **cfg) as c:
        for e in (a, b, c):
            feed(e, x[:, :CUT])
        ba, bb, bc = a.state_export(), b.state_export(), c.state_export()
        assert ba == bb
        assert len(bc) - len(bb) == S * 48 * 4                             # the history rows: 23 frames and the factor, 192 bytes a stream
        same(snap(a), snap(b))


# ---- 5: samples that are not finite -------------------------------------------------------------------------------------------------------
def test_not_finite_stays_in_its_stream_and_leaves_within_24_frames(M):
    S, T, f = 16, 2400, 4
    x = signal(S, T)
    bad = [s for s in range(S) if s % _gonio.N_SIGNALS == 6]
    clean = [s for s in range(S) if s not in bad]
    assert not np.isfinite(x[bad]).all() and np.isfinite(x[clean]).all()
    ref = guard(S, T, f, P=480)
    # the yardstick's own recovery: the points of the 24 input frames from the bad one on are not finite, every other is
    pts = OS.upsample(x[bad], f)[0]
    for t0 in (T // 3, (2 * T) // 3):
        assert not np.isfinite(pts[:, t0 * f:(t0 + 24) * f]).all(axis=(1, 2)).any() and np.isfinite(pts[:, (t0 + 24) * f:(t0 + 124) * f]).all()
    assert (ref.clipped[bad] > 0).all()
    cfg = dict(period_frames=480, capacity=16)
    with engine(M, S, f, **cfg) as e:
        feed(e, x, [1201, 1199])
        got = snap(e)
    same(got, want(ref))                                                   # the stream itself recovers as the yardstick does
    assert np.isfinite(got["lp"].view(np.float32)).all()
    y = x.copy()
    y[bad] = 0
    with engine(M, S, f, **cfg) as e:
        feed(e, y, [1201, 1199])
        same(snap(e), got, rows=clean)


# ---- 6: set-up ----------------------------------------------------------------------------------------------------------------------------
def test_set_up(M):
    S, T, f = 5, 1000, 4
    x = signal(S, T, 7)
    with engine(M, S, None, period_frames=480, capacity=8) as e:
        assert e.gonio_oversample() == (1, _gonio.derive(FS).hpw)
        for bad in (0, 33):
            assert M.lib.mtr_engine_gonio_set_oversample(e._h, bad) == M.engine.ERR_ARG
        e.gonio_set_oversample(f)
        e.gonio_configure(period_frames=100, capacity=16)                  # configure keeps the factor
        assert e.gonio_oversample()[0] == f
        feed(e, x, [333, 667])
        first = snap(e)
        assert M.lib.mtr_engine_gonio_set_oversample(e._h, 2) == M.engine.ERR_STATE
        assert M.lib.mtr_engine_gonio_set_oversample(e._h, 0) == M.engine.ERR_ARG   # a bad value is a bad value on any engine
        e.reset()                                                          # keeps the factor, zeroes the history
        assert e.gonio_oversample()[0] == f
        z = snap(e)
        assert not z["img"].any() and z["blocks"].tolist() == [0, 0]
        feed(e, x, [333, 667])
        same(snap(e), first)
        e.gonio_reset()
        feed(e, x)
        same(snap(e), first)
        same(first, want(shared(("setup", f), lambda: OS.GonioOS(S, FS, f, P=100).run(x))))
        # a call of 2^30 frames is 2^32 points: refused before anything is queued
        assert M.lib.mtr_engine_process_device(e._h, device(x).data_ptr(), 1 << 30, 1 << 30, None) == M.engine.ERR_ARG
        same(snap(e), first)
    with M.Engine(S, FS, M.METER_STCORR) as e:                             # an engine without the meter
        assert M.lib.mtr_engine_gonio_set_oversample(e._h, 2) == M.engine.ERR_ARG
        assert M.lib.mtr_engine_gonio_oversample(e._h, None, None) == M.engine.ERR_ARG
    # the reference's scratch holds `rate` frames: P > floor (rate) with a factor is refused, in whichever order the two calls come
    with engine(M, S, None, period_frames=48001, capacity=4) as e:
        assert M.lib.mtr_engine_gonio_set_oversample(e._h, 2) == M.engine.ERR_ARG
        e.gonio_set_oversample(1)
        e.gonio_configure(period_frames=48000, capacity=4)
        e.gonio_set_oversample(2)
        with pytest.raises(M.EngineError) as ei:
            e.gonio_configure(period_frames=48001, capacity=4)
        assert ei.value.code == M.engine.ERR_ARG
        assert e.gonio_config()[0].period_frames == 48000 and e.gonio_oversample()[0] == 2


def test_beside_the_other_meters(M):
    S, T, f = 19, 3000, 2
    ref = guard(S, T, f, P=480, gain=4.0)
    x = signal(S, T)
    base = M.METER_KMETER | M.METER_STCORR
    with M.Engine(S, FS, base) as a, M.Engine(S, FS, base | M.METER_GONIO) as b:
        b.gonio_configure(period_frames=480, capacity=8, gain=4.0, tune_piece=1024)
        b.gonio_set_oversample(f)
        for e in (a, b):
            e.stcorr_set_period(2400, 4)
            feed(e, x, SMALL[:-1] + [2500])
        assert bytes(a.results()) == bytes(b.results())
        sa, sb = a.stcorr_series(), b.stcorr_series()
        assert np.array_equal(sa[0].view(U32), sb[0].view(U32)) and sa[1:] == sb[1:] == (1, 0)
        same(snap(b), want(ref))
