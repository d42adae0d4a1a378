"""The goniometer for a batch (MTR_METER_GONIO, mtr_gonio.hip) against the restatement of tests/_gonio.py (draw_rb of
gui/goniometer.c:299-538 in points mode; tests/test_gonio_cpu.py holds the restatement to what follows from the formulas).

k_gonio_points is a serial chain that does the reference's f32 / double operations in the reference's order and k_gonio_image adds
integers, so every comparison here is equality of BYTES (floats as uint32 views): the images, the three counters, gain / lp / last point
and the series.  Every test on the signal set first asserts, on the restatement's counts, that some stream clipped, some stream skipped
between 10 % and 90 % of its frames and some stream painted nothing (_gonio.coverage)."""
import numpy as np
import pytest

import _gonio

pytestmark = pytest.mark.gpu
FS = 48000.0
CALLS = [1, 255, 257, 1000, 3487]
U32 = np.uint32


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


def reference(S, T, seed=1, **kw):
    """the restatement over the whole of signal (S, T, seed): computed once, shared, never changed"""
    key = (S, T, seed, tuple(sorted(kw.items())))
    if key not in _ref:
        _ref[key] = _gonio.Gonio(S, FS, **kw).run(signal(S, T, seed))
    return _ref[key]


def engine(M, S, meters=None, **cfg):
    e = M.Engine(S, FS, M.METER_GONIO if meters is None else meters)
    e.gonio_configure(**cfg)
    return e


def feed(e, x, calls=None):
    """x [S, T, W] from device memory, in calls of the given lengths (None: one call)"""
    import torch
    dev = torch.from_numpy(np.array(x, np.float32, copy=True)).cuda()
    T, W = x.shape[1], x.shape[2]
    pos = 0
    for n in calls or [T]:
        e.process_device(dev.data_ptr() + pos * 4 * W, n, T)
        pos += n
    assert pos == T
    e.sync()


def snap(e):
    img, drawn, clipped, skipped = e.gonio_image()
    gain, lp, last = e.gonio_read()
    sg, sd, sc = e.gonio_series()
    return dict(img=img, drawn=drawn, clipped=clipped, skipped=skipped, gain=gain.view(U32), lp=lp.view(U32), last=last.view(U32),
                s_gain=sg.view(U32), s_drawn=sd, s_clipped=sc, blocks=np.array(e.gonio_blocks()))


def want(g, cap=None):
    sg, sd, sc = g.series_arrays()
    n = sg.shape[1]
    k = n if cap is None else min(n, cap)
    return dict(img=g.img, drawn=g.drawn, clipped=g.clipped, skipped=g.skipped, gain=g.gain.view(U32),
                lp=np.stack([g.lp0, g.lp1], axis=1).view(U32), last=np.stack([g.last_x, g.last_y], axis=1).view(U32),
                s_gain=np.ascontiguousarray(sg[:, :k]).view(U32), s_drawn=sd[:, :k], s_clipped=sc[:, :k], blocks=np.array([n, k]))


def same(a, b, rows=None, skip=()):
    for k in a:
        if k in skip:
            continue
        x, y = (a[k], b[k]) if rows is None or k == "blocks" else (a[k][rows], b[k][rows])
        assert x.shape == y.shape and np.array_equal(x, y), (k, np.argwhere(np.asarray(x != y))[:4].tolist())


# ---- 1: fixed gain, cuts, every way in --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gain", [1.0, 4.0])
def test_fixed_gain_bit_for_bit_however_the_audio_is_cut(M, gain):
    S, T = 67, 5000                                                        # a full wave plus three lanes; pieces of 1024: five per call
    ref = reference(S, T, P=480, gain=gain)
    _gonio.coverage(ref, T)
    x, w = signal(S, T), want(ref)
    cfg = dict(period_frames=480, capacity=16, gain=gain, tune_piece=1024)
    with engine(M, S, **cfg) as e:
        feed(e, x, CALLS)
        cut = snap(e)
    same(cut, w)
    with engine(M, S, **cfg) as e:
        feed(e, x)
        same(snap(e), cut)
    with engine(M, S, **cfg) as e:
        e.process(x)
        same(snap(e), cut)
    with engine(M, S, **cfg) as e:                                         # the host path in views of the batch (two chunks of streams per call), two calls
        e.set_host_chunk_bytes(20 * T * 8)
        e.process(x[:, :2401])
        e.process(x[:, 2401:])
        same(snap(e), cut)
    assert cut["blocks"].tolist() == [10, 10] and (cut["img"].reshape(S, -1).sum(axis=1, dtype=np.uint64) == cut["drawn"]).all()


# ---- 2: auto gain ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [0, 100])
def test_auto_gain_series_bit_for_bit(M, P):
    S, T = 19, 9600
    ref = reference(S, T, seed=2, P=P, autogain=True)
    _gonio.coverage(ref, T)
    with engine(M, S, period_frames=P, capacity=128 if P else 0, autogain=1) as e:
        assert e.gonio_config()[1].period_frames == (P or 1920)
        feed(e, signal(S, T, 2), [4097, 5503])
        got = snap(e)
    same(got, want(ref))
    assert got["blocks"][0] == T // (P or 1920)
    assert np.array_equal(got["s_gain"][:, -1], got["gain"])               # T is a whole number of blocks: the last point is the gain
    assert len(np.unique(got["s_gain"][0])) > 3                            # (it moved)


# ---- 3: shifts ------------------------------------------------------------------------------------------------------------------------
def test_shifts_are_block_sums_of_one_another(M):
    S, T = 16, 3000
    imgs = {}
    for shift in (1, 2, 3):
        ref = reference(S, T, seed=3, P=480, gain=4.0, shift=shift)
        _gonio.coverage(ref, T)
        with engine(M, S, period_frames=480, capacity=8, gain=4.0, shift=shift) as e:
            assert e.gonio_config()[1].G == {1: 187, 2: 94, 3: 47}[shift]
            feed(e, signal(S, T, 3), [1500, 1500])
            got = snap(e)
        same(got, want(ref))
        imgs[shift] = got["img"]
    for k in (1, 2):
        a = imgs[k].astype(np.uint64)
        G = a.shape[1] + (a.shape[1] & 1)
        p = np.zeros((S, G, G), np.uint64)
        p[:, :a.shape[1], :a.shape[1]] = a                                 # edges padded with zeros
        assert np.array_equal(p.reshape(S, G // 2, 2, G // 2, 2).sum(axis=(2, 4)), imgs[k + 1].astype(np.uint64)), k


# ---- 4: samples that are not finite -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("autogain", [0, 1])
def test_not_finite_stays_in_its_stream(M, autogain):
    S, T = 16, 4800
    x = signal(S, T)
    bad = [s for s in range(S) if s % _gonio.N_SIGNALS == 6]
    clean = [s for s in range(S) if s not in bad]
    assert not np.isfinite(x[bad]).all() and np.isfinite(x[clean]).all()
    ref = reference(S, T, P=480, autogain=bool(autogain))
    _gonio.coverage(ref, T)
    assert (ref.clipped[bad] > 0).all()
    cfg = dict(period_frames=480, capacity=16, autogain=autogain)
    with engine(M, S, **cfg) as e:
        feed(e, x, [2401, 2399])
        got = snap(e)
    same(got, want(ref))                                                   # the stream itself: integers, gain, and lp reset at the block's end
    assert np.isfinite(got["lp"].view(np.float32)).all()
    y = x.copy()
    y[bad] = 0
    with engine(M, S, **cfg) as e:
        feed(e, y, [2401, 2399])
        same(snap(e), got, rows=clean)


# ---- 5: capacity ----------------------------------------------------------------------------------------------------------------------
def test_points_past_the_capacity_are_counted_not_written(M):
    S, T, P, CAP = 5, 1000, 100, 3
    ref = reference(S, T, seed=4, P=P, autogain=True)
    w = want(ref, CAP)
    with engine(M, S, period_frames=P, capacity=CAP, autogain=1) as e:
        feed(e, signal(S, T, 4), [333, 667])
        assert e.gonio_blocks() == (10, 3)
        same(snap(e), w)
        # the caller's buffers: a guard pattern around [S][3]
        PAD, PAT = 16, 0xA5A5A5A5
        bufs = [np.full(2 * PAD + S * CAP, PAT, U32) for _ in range(3)]
        ptr = [b.ctypes.data + 4 * PAD for b in bufs]
        assert M.lib.mtr_engine_gonio_series(e._h, 0, S, 0, CAP, *ptr) == 0
        for b, k in zip(bufs, ("s_gain", "s_drawn", "s_clipped")):
            assert (b[:PAD] == PAT).all() and (b[-PAD:] == PAT).all()
            assert np.array_equal(b[PAD:-PAD].reshape(S, CAP), w[k])
        assert M.lib.mtr_engine_gonio_series(e._h, 0, S, 0, CAP + 1, *ptr) == M.engine.ERR_ARG
        assert M.lib.mtr_engine_gonio_series(e._h, 0, S, 2, 2, *ptr) == M.engine.ERR_ARG
        assert M.lib.mtr_engine_gonio_series(e._h, 1, 2, 2, 1, *ptr) == 0
        assert np.array_equal(bufs[0][PAD:PAD + 2], w["s_gain"][1:3, 2])
        for b in bufs:
            assert (b[:PAD] == PAT).all() and (b[-PAD:] == PAT).all()


# ---- 6: state -------------------------------------------------------------------------------------------------------------------------
def test_state_travels(M):
    S, T, CUT = 9, 3000, 1234                                             # 1234 = 2 * 480 + 274: inside a block
    ref = reference(S, T, seed=5, P=480, autogain=True)
    _gonio.coverage(ref, T)
    x, w = signal(S, T, 5), want(ref)
    cfg = dict(period_frames=480, capacity=8, autogain=1)
    with engine(M, S, **cfg) as a, engine(M, S, **cfg) as b:
        feed(a, x[:, :CUT])
        blob = a.state_export()
        assert len(blob) == a.state_bytes(S)
        assert b.state_import(blob) == S
        feed(b, x[:, CUT:])
        got = snap(b)
        # (the series of the importing engine starts with the block the blob was cut in: points are not part of a blob)
        same(got, w, skip=("s_gain", "s_drawn", "s_clipped", "blocks"))
        assert got["blocks"].tolist() == [4, 4]
        for k in ("s_gain", "s_drawn", "s_clipped"):
            assert np.array_equal(got[k], w[k][:, 2:]), k
        # another P, another shift, auto gain off: not this blob's engine
        for other in (dict(cfg, period_frames=481), dict(cfg, shift=3), dict(cfg, autogain=0)):
            with engine(M, S, **other) as c:
                with pytest.raises(M.EngineError) as ei:
                    c.state_import(blob)
                assert ei.value.code == M.engine.ERR_STATE
        # an engine that stands elsewhere in its block
        with pytest.raises(M.EngineError) as ei:
            b.state_import(blob)
        assert ei.value.code == M.engine.ERR_STATE
        # image_clear keeps the filters, the last point and the gain
        before = snap(b)
        b.gonio_image_clear()
        after = snap(b)
        same(after, before, skip=("img", "drawn", "clipped", "skipped"))
        assert not after["img"].any() and not (after["drawn"] | after["clipped"] | after["skipped"]).any()
        # mtr_engine_reset: the initial values, and the same results again
        b.reset()
        z = snap(b)
        assert not z["img"].any() and not z["lp"].any() and z["blocks"].tolist() == [0, 0]
        assert (z["gain"].view(np.float32) == 1).all() and (z["last"].view(np.float32) == 186.5).all()
        feed(b, x, [CUT, T - CUT])
        same(snap(b), w)


def test_blobs_without_the_meter_are_what_they_were(M):
    S, T = 4, 2000
    x = signal(S, T, 6)
    base = M.METER_EBU | M.METER_TRUEPEAK | M.METER_STCORR | M.METER_NEEDLE
    with M.Engine(S, FS, base) as a, M.Engine(S, FS, base | M.METER_GONIO) as b:
        for e in (a, b):
            e.stcorr_set_period(2400, 4)
            feed(e, x)
        pitch = (96 + 94 * 94 * 4 + 15) & ~15
        hdr = 2 * a.state_bytes(1) - a.state_bytes(2)
        assert hdr == 2 * b.state_bytes(1) - b.state_bytes(2)
        assert b.state_bytes(S) - a.state_bytes(S) == S * pitch
        ba, bb = a.state_export(), b.state_export()
        assert bb[hdr:len(ba)] == ba[hdr:]                                 # the new section lies behind every older one
        with pytest.raises(M.EngineError) as ei:
            a.state_import(bb)
        assert ei.value.code == M.engine.ERR_STATE


# ---- 7: beside the other meters ---------------------------------------------------------------------------------------------------------
def test_beside_the_other_meters(M):
    S, T = 67, 5000
    ref = reference(S, T, P=480, gain=1.0)
    _gonio.coverage(ref, T)
    x = signal(S, T)
    base = M.METER_EBU | M.METER_TRUEPEAK | M.METER_STCORR
    with M.Engine(S, FS, base) as a, M.Engine(S, FS, base | M.METER_GONIO) as b:
        b.gonio_configure(period_frames=480, capacity=16, gain=1.0, tune_piece=1024)
        for e in (a, b):
            e.stcorr_set_period(2400, 4)
            feed(e, x, CALLS)
        assert bytes(a.results()) == bytes(b.results())
        sa, sb = a.stcorr_series(), b.stcorr_series()
        assert np.array_equal(sa[0].view(U32), sb[0].view(U32)) and sa[1:] == sb[1:] == (2, 0)
        got = snap(b)
        same(got, want(ref))
        # the six families of calls with per-stream ends refuse the meter and queue nothing
        import torch
        dev = torch.from_numpy(np.array(x, np.float32, copy=True)).cuda()
        res = bytes(b.results())
        for fam in ("lengths", "tracks", "ragged", "ends", "tpb", "any"):
            with pytest.raises(M.EngineError) as ei:
                getattr(b, "process_device_" + fam)(dev.data_ptr(), T, [T] * (S - 1) + [100])
            assert ei.value.code == M.engine.ERR_UNSUPPORTED, fam
            with pytest.raises(M.EngineError) as ei:
                getattr(b, "process_" + fam)(x, [T] * S)
            assert ei.value.code == M.engine.ERR_UNSUPPORTED, fam
        same(snap(b), got)
        assert bytes(b.results()) == res


# ---- 8: frame layout --------------------------------------------------------------------------------------------------------------------
def test_a_pair_of_wider_frames(M):
    S, T = 16, 2000
    ref = reference(S, T, P=480, gain=4.0)
    _gonio.coverage(ref, T)
    x = signal(S, T)
    wide = np.random.default_rng(9).uniform(-1, 1, (S, T, 6)).astype(np.float32)
    wide[:, :, 0], wide[:, :, 1] = x[:, :, 0], x[:, :, 1]
    cfg = dict(period_frames=480, capacity=8, gain=4.0)
    with engine(M, S, **cfg) as e:
        e.set_frame_layout(6, [0, 1])
        feed(e, wide, [999, 1001])
        same(snap(e), want(ref))
        e.reset()
        e.process(wide)
        same(snap(e), want(ref))


def test_integer_pcm_in(M):
    """16-bit PCM decoded on the GPU: the meter sees what mtr_pcm_decode_host gives"""
    S, T = 16, 2000
    q = (np.clip(np.nan_to_num(signal(S, T), nan=0.0, posinf=1.0, neginf=-1.0), -1, 1) * 32767).astype(np.int16)
    g = _gonio.Gonio(S, FS, P=480, gain=4.0).run(M.pcm_decode(M.PCM_S16, q))
    _gonio.coverage(g, T)
    with engine(M, S, period_frames=480, capacity=8, gain=4.0) as e:
        e.process_pcm(q[:, :999])
        e.process_pcm(q[:, 999:])
        same(snap(e), want(g))


# ---- 9: set_gain --------------------------------------------------------------------------------------------------------------------------
def test_set_gain_applies_from_the_next_call(M):
    S, T, CUT = 16, 3000, 1234
    x = signal(S, T)
    g = _gonio.Gonio(S, FS, P=480, gain=1.0).run(x[:, :CUT])
    g.set_gain(4.0)
    g.run(x[:, CUT:])
    _gonio.coverage(g, T)
    with engine(M, S, period_frames=480, capacity=8) as e:
        feed(e, x[:, :CUT])
        e.gonio_set_gain(4.0)
        feed(e, x[:, CUT:])
        got = snap(e)
        same(got, want(g))
        assert (got["s_gain"].view(np.float32)[:, :2] == 1).all() and (got["s_gain"].view(np.float32)[:, 2:] == 4).all()
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            assert M.lib.mtr_engine_gonio_set_gain(e._h, bad) == M.engine.ERR_ARG
        e.reset()
        assert (e.gonio_read()[0] == 1).all()                              # back to the configured gain


# ---- 10: configure after processing -------------------------------------------------------------------------------------------------------
def test_configure_only_on_a_fresh_engine(M):
    S = 3
    with engine(M, S, period_frames=480, capacity=8) as e:
        feed(e, np.zeros((S, 100, 2), np.float32))
        with pytest.raises(M.EngineError) as ei:
            e.gonio_configure(period_frames=960, capacity=8)
        assert ei.value.code == M.engine.ERR_STATE
        with pytest.raises(M.EngineError) as ei:
            e.gonio_configure(period_frames=63, capacity=8)                # a bad value is a bad value on any engine
        assert ei.value.code == M.engine.ERR_ARG
        c, d = e.gonio_config()
        assert (c.period_frames, c.capacity, c.shift, c.autogain, c.gain, c.point_width, c.tune_piece) == (480, 8, 2, 0, 1.0, 1.75, 4096)
        e.reset()
        e.gonio_configure(period_frames=960, capacity=8, autogain=1)
        c, d = e.gonio_config()
        assert (c.period_frames, c.g_attack, c.g_decay, c.g_target, c.g_rms) == (960, 54.0, 58.0, 40.0, 50.0) and d.G == 94
    with M.Engine(S, FS, M.METER_STCORR) as e:                             # an engine without the meter
        assert M.lib.mtr_engine_gonio_reset(e._h) == M.engine.ERR_ARG
        assert M.lib.mtr_engine_gonio_image(e._h, 0, 1, None, None, None, None) == M.engine.ERR_ARG
