"""Track lengths for the goniometer on the GPU (include/mtr_gonio_ends.h: mtr_engine_process_*_gonio_ends, mtr_engine_gonio_points; the ENDS
instantiations of k_gonio_points and k_gonio_image) against the restatement of tests/_gonio_ends.py, which tests/test_gonio_ends_cpu.py
holds to one-track runs of tests/_gonio.py.

Every comparison is equality of BYTES, as in tests/test_gpu_gonio.py: images, the three counters, gain / lp / last point, the series and
each stream's own count of updates.  Every test on the planted ends first asserts the guard of _gonio_ends.coverage_ends on the
restatement alone: a closing update that painted and (auto gain) moved the gain, a stream with 0 < r < 64, one with r = 0, and the
signal set's own rules."""
import numpy as np
import pytest

import _gonio
import _gonio_ends as GE

pytestmark = pytest.mark.gpu
FS = 48000.0
S, T, P = 67, 5000, 480                      # a full NS = 16 workgroup set plus three lanes; pieces of 1024: chunks of 128 frames, five pieces
CALLS = [1, 255, 257, 1000, 3487]
LEAD = 100
U32 = np.uint32
CFG = dict(period_frames=P, capacity=16, tune_piece=1024, shift=2)


@pytest.fixture(scope="module")
def M():
    import meters.lv2_amd as m
    return m


_sig, _ref = {}, {}


def signal(S_, T_, seed=1):
    if (S_, T_, seed) not in _sig:
        _sig[(S_, T_, seed)] = _gonio.signals(S_, T_, FS, seed)
        _sig[(S_, T_, seed)].setflags(write=False)
    return _sig[(S_, T_, seed)]


def ENDS():
    return GE.planted_ends(S, T, P)


def reference(key, make):
    """a restatement, computed once, shared, never changed"""
    if key not in _ref:
        _ref[key] = make()
    return _ref[key]


def ref_planted(autogain, calls=None, lead=0):
    def make():
        if lead:                                                           # a dense call of `lead` frames in front: the ends move behind it
            x = signal(S, T + lead)
            ends = ENDS() + lead                                           # (E = 0: the closing call's first frame — untouched; E = T: open)
            return GE.run(x, ends, FS, calls=[lead, T], P=P, autogain=bool(autogain))
        return GE.run(signal(S, T), ENDS(), FS, calls=calls, P=P, autogain=bool(autogain))
    return reference(("planted", autogain, tuple(calls or ()), lead), make)


def engine(M, S_, meters=None, **cfg):
    e = M.Engine(S_, FS, M.METER_GONIO if meters is None else meters)
    e.gonio_configure(**cfg)
    return e


def device(x):
    import torch
    return torch.from_numpy(np.array(x, np.float32, copy=True)).cuda()


def bits(a):
    """float32 as uint32, every NaN as ONE pattern: which NaN inf - inf gives is the machine's choice (x86: 0xFFC00000, gfx950: 0x7FC00000),
    not the reference's.  A track can end between the frame that made its last point NaN and the next painted one, which a whole
    batch of tests/test_gpu_gonio.py never shows: there every stream runs on to a finite point."""
    a = np.ascontiguousarray(a, np.float32)
    return np.where(np.isnan(a), np.float32(np.nan), a).view(U32)


def snap(e):
    img, drawn, clipped, skipped = e.gonio_image()
    gain, lp, last = e.gonio_read()
    sg, sd, sc = e.gonio_series()
    up, pt = e.gonio_points()
    return dict(img=img, drawn=drawn, clipped=clipped, skipped=skipped, gain=bits(gain), lp=bits(lp), last=bits(last),
                s_gain=bits(sg), s_drawn=sd, s_clipped=sc, blocks=np.array(e.gonio_blocks()), updates=up, points=pt)


def want(o, cap=16, blocks=None):
    n = o.blocks if blocks is None else blocks
    k = min(n, cap)
    return dict(img=o.img, drawn=o.drawn, clipped=o.clipped, skipped=o.skipped, gain=bits(o.gain),
                lp=bits(np.stack([o.lp0, o.lp1], axis=1)), last=bits(np.stack([o.last_x, o.last_y], axis=1)),
                s_gain=bits(o.s_gain[:, :k]), s_drawn=o.s_drawn[:, :k], s_clipped=o.s_clipped[:, :k],
                blocks=np.array([n, k]), updates=o.updates, points=o.updates)


def same(a, b, rows=None, skip=()):
    for k in a:
        if k in skip:
            continue
        x, y = (a[k], b[k]) if rows is None or k == "blocks" else (a[k][rows], b[k][rows])
        assert x.shape == y.shape, (k, x.shape, y.shape)
        bad = np.argwhere(np.asarray(x != y))[:6]
        assert not len(bad), (k, bad.tolist(), [(x[tuple(i)], y[tuple(i)]) for i in bad])


def feed_cut(e, dev, ends, calls, T_):
    """the audio in `calls`: a stream's end is given in the call that holds it (start <= E < start + n), closed streams ride dense calls"""
    pos = 0
    for n in calls:
        f = np.clip(ends.astype(np.int64) - pos, 0, n).astype(np.uint64)
        closed = e.stream_frames()[1].astype(bool)
        if (f[~closed] == n).all():
            e.process_device(dev.data_ptr() + pos * 8, n, T_)
        else:
            e.process_device_gonio_ends(dev.data_ptr() + pos * 8, n, f, T_)
        pos += n
    e.sync()


# ---- 1: the planted ends, four ways in ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("autogain", [0, 1])
def test_planted_ends_bit_for_bit_four_ways(M, autogain):
    ends, x = ENDS(), signal(S, T)
    one = ref_planted(autogain)
    GE.coverage_ends(one, autogain)
    cfg = dict(CFG, autogain=autogain)
    dev = device(x)
    with engine(M, S, **cfg) as e:                                         # one _device call
        e.process_device_gonio_ends(dev.data_ptr(), T, ends)
        e.sync()
        got = snap(e)
        same(got, want(one))
        assert np.array_equal(e.stream_frames()[0], ends) and np.array_equal(e.stream_frames()[1].astype(bool), ends < T)
    assert (got["img"].reshape(S, -1).sum(axis=1, dtype=np.uint64) == got["drawn"]).all()
    with engine(M, S, **cfg) as e:                                         # the same audio in calls
        cut = ref_planted(autogain, CALLS)
        GE.coverage_ends(cut, autogain)
        feed_cut(e, dev, ends, CALLS, T)
        same(snap(e), want(cut))
    with engine(M, S, **cfg) as e:                                         # the _host form, two chunks of streams per call
        e.set_host_chunk_bytes(40 * T * 8)
        e.process_gonio_ends(x, ends)
        e.sync()
        same(snap(e), got)
    lead = ref_planted(autogain, lead=LEAD)                                # fill != 0 at the closing call
    GE.coverage_ends(lead, autogain)
    xl = signal(S, T + LEAD)
    devl = device(xl)
    with engine(M, S, **cfg) as e:
        e.process_device(devl.data_ptr(), LEAD, T + LEAD)
        e.process_device_gonio_ends(devl.data_ptr() + LEAD * 8, T, ends, T + LEAD)
        e.sync()
        same(snap(e), want(lead))


# ---- 2: poison ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("autogain", [0, 1])
def test_no_frame_at_or_behind_an_end_is_read(M, autogain):
    ends = ENDS()
    one = ref_planted(autogain)
    GE.coverage_ends(one, autogain)
    x = np.array(signal(S, T), copy=True)
    z = x.copy()
    for s in range(S):
        x[s, int(ends[s]):] = np.nan
        z[s, int(ends[s]):] = 0
    cfg = dict(CFG, autogain=autogain)
    res = []
    for y in (x, z):
        with engine(M, S, **cfg) as e:
            dev = device(y)
            e.process_device_gonio_ends(dev.data_ptr(), T, ends)
            e.sync()
            res.append(snap(e))
            if y is x:
                # a closed stream's whole state is unchanged by two further calls of any entry point
                closed = np.nonzero(ends < T)[0]
                blob = e.state_export()
                poison = device(np.full((S, 300, 2), np.nan, np.float32))
                e.process_device(poison.data_ptr(), 300)
                e.process_gonio_ends(np.full((S, 300, 2), np.nan, np.float32), [300] * S)
                e.sync()
                after = snap(e)
                series = ("s_gain", "s_drawn", "s_clipped")
                same(after, res[0], rows=closed, skip=("blocks",) + series)
                for k in series:                                                   # (the lock-step count of held points moved on: 11 now)
                    assert np.array_equal(after[k][closed, :10], res[0][k][closed]), k
                # the stream's entry of the blob — state and image; the goniometer's section lies behind every older one
                pitch = (96 + 94 * 94 * 4 + 15) & ~15
                a, b = (np.frombuffer(v, np.uint8)[-S * pitch:].reshape(S, pitch) for v in (blob, e.state_export()))
                hdr = 16                                                           # (mtr_gonio_hdr: the lock-step cursor moved)
                assert np.array_equal(a[closed, hdr:], b[closed, hdr:]) and not np.array_equal(a[:, hdr:], b[:, hdr:])
    same(res[0], res[1])
    same(res[0], want(one))


# ---- 3: every stream open, every stream closed -------------------------------------------------------------------------------------------
def test_every_stream_open_is_the_dense_call_and_no_frames_change_nothing(M):
    x = signal(S, T)
    dev = device(x)
    cfg = dict(CFG, autogain=1)
    with engine(M, S, **cfg) as a, engine(M, S, **cfg) as b:
        a.process_device(dev.data_ptr(), 2000, T)
        b.process_device_gonio_ends(dev.data_ptr(), 2000, [2000] * S, T)
        a.sync(), b.sync()
        same(snap(b), snap(a))
        assert a.state_export() == b.state_export() and not b.stream_frames()[1].any()
        before = snap(b)
        b.process_device_gonio_ends(dev.data_ptr() + 2000 * 8, 3000, [0] * S, T)    # E = 0 for all: closed untouched
        b.sync()
        assert b.stream_frames()[1].all()
        got = snap(b)
        same(got, before, skip=("blocks", "s_gain", "s_drawn", "s_clipped"))
        assert got["blocks"].tolist() == [10, 10]                                  # (the lock-step cursor moved on: 5000 frames)
        for k in ("s_gain", "s_drawn", "s_clipped"):
            assert np.array_equal(got[k][:, :4], before[k]) and not got[k][:, 4:].any(), k


# ---- 4: capacity ------------------------------------------------------------------------------------------------------------------------
def test_a_closing_point_at_the_capacity_is_counted_not_written(M):
    S_, T_, P_, CAP = 5, 1000, 100, 3
    x = signal(S_, T_, 4)
    ends = np.array([370, 270, 1000, 399, 300], np.uint64)                 # closing points at index 3 == CAP, 2, -, 3, none (r = 0)
    o = reference(("cap",), lambda: GE.run(x, ends, FS, P=P_, autogain=True))
    assert o.r.tolist() == [70, 70, 0, 99, 0] and o.updates.tolist() == [4, 3, 10, 4, 3]
    with engine(M, S_, period_frames=P_, capacity=CAP, autogain=1) as e:
        dev = device(x)
        e.process_device_gonio_ends(dev.data_ptr(), T_, ends)
        e.sync()
        assert e.gonio_blocks() == (10, 3)
        same(snap(e), want(o, CAP))
        # (a point written at index CAP of stream 0 would be stream 1's first: the rows follow one another in the ring)


# ---- 5: beside the other meters -----------------------------------------------------------------------------------------------------------
def test_beside_the_other_meters(M):
    ends, x = ENDS(), signal(S, T)
    one = ref_planted(0)
    GE.coverage_ends(one, 0)
    base = M.METER_EBU | M.METER_TRUEPEAK | M.METER_STCORR
    dev = device(x)
    with M.Engine(S, FS, base) as a, M.Engine(S, FS, base | M.METER_GONIO) as b:
        b.gonio_configure(**CFG)
        for e in (a, b):
            e.stcorr_set_period(2400, 4)
        a.process_device_any(dev.data_ptr(), T, ends)
        b.process_device_gonio_ends(dev.data_ptr(), T, ends)
        a.sync(), b.sync()
        assert bytes(a.results()) == bytes(b.results())
        sa, sb = a.stcorr_series(), b.stcorr_series()
        assert np.array_equal(sa[0].view(U32), sb[0].view(U32)) and sa[1:] == sb[1:]
        assert np.array_equal(a.series_points(M.METER_STCORR), b.series_points(M.METER_STCORR))
        got = snap(b)
        same(got, want(one))
        res = bytes(b.results())
        # the six older families still refuse the engine, the new pair refuses an engine without GONIO: nothing is queued
        for fam in ("lengths", "tracks", "ragged", "ends", "tpb", "any"):
            with pytest.raises(M.EngineError) as ei:
                getattr(b, "process_device_" + fam)(dev.data_ptr(), T, [T] * (S - 1) + [100])
            assert ei.value.code == M.engine.ERR_UNSUPPORTED, fam
        ra = bytes(a.results())
        with pytest.raises(M.EngineError) as ei:
            a.process_device_gonio_ends(dev.data_ptr(), T, [T] * S)
        assert ei.value.code == M.engine.ERR_UNSUPPORTED
        with pytest.raises(M.EngineError) as ei:
            a.process_gonio_ends(x, [T] * S)
        assert ei.value.code == M.engine.ERR_UNSUPPORTED
        # frames[s] > n_frames and NULLs: MTR_ERR_ARG
        with pytest.raises(M.EngineError) as ei:
            b.process_device_gonio_ends(dev.data_ptr(), T, [T] * (S - 1) + [T + 1])
        assert ei.value.code == M.engine.ERR_ARG
        f = np.full(S, T, np.uint64)
        assert M.lib.mtr_engine_process_device_gonio_ends(b._h, None, T, T, f.ctypes.data, None) == M.engine.ERR_ARG
        assert M.lib.mtr_engine_process_device_gonio_ends(b._h, dev.data_ptr(), T, T, None, None) == M.engine.ERR_ARG
        assert M.lib.mtr_engine_process_host_gonio_ends(b._h, x.ctypes.data, T, T, None) == M.engine.ERR_ARG
        assert M.lib.mtr_engine_process_host_gonio_ends(b._h, None, T, T, f.ctypes.data) == M.engine.ERR_ARG
        same(snap(b), got)
        assert bytes(b.results()) == res and bytes(a.results()) == ra


KM_P, TPB_P = 2500, 64                      # KMETER's and TPBALLIST's periods: planted ends on a block's edge (2500; 64, 128, 1024, 2048) and inside one


def beside(e, M):
    """what the meters beside the goniometer report, floats as bits()"""
    o = dict(results=np.frombuffer(bytes(e.results()), np.uint8), km_points=e.series_points(M.METER_KMETER), tpb_points=e.tpb_points())
    groups = dict(km_read=e.kmeter_read(), km_series=e.kmeter_series(), tpb_series=e.tpb_series(), scope_points=e.scope_points(),
                  scope_read=tuple(v for _, v in sorted(e.scope_read().items())))
    for name, vals in groups.items():
        for i, v in enumerate(vals):
            v = np.asarray(v)
            o[f"{name}[{i}]"] = bits(v) if v.dtype == np.float32 else v
    return o


def test_beside_kmeter_tpb_and_scope(M):
    """Two rows of the side meters' table with words of their own in the lengths ring (KMETER, GONIO) in one engine, TPBALLIST's kernel
    queued in front of the goniometer's, SCOPE's and GONIO's per-stream counts: engine b (with GONIO) gives every other meter what engine a
    (without) gives it, byte for byte, and the goniometer what it draws alone — through the device and the host entry points, the latter
    in two views of the batch"""
    ends, x, more = ENDS(), signal(S, T), signal(S, 1000, 7)
    one = ref_planted(0)
    GE.coverage_ends(one, 0)
    closing = ends[(ends > 0) & (ends < T)].astype(np.int64)
    for p in (KM_P, TPB_P):
        assert (closing % p == 0).any() and (closing % p != 0).any(), p        # an end on a block's edge, an end inside a block
    closed = np.nonzero(ends < T)[0]
    base = M.METER_EBU | M.METER_TRUEPEAK | M.METER_KMETER | M.METER_TPBALLIST | M.METER_SCOPE
    dev, dev2 = device(x), device(more)
    for host in (False, True):
        with M.Engine(S, FS, base) as a, M.Engine(S, FS, base | M.METER_GONIO) as b:
            b.gonio_configure(**CFG)
            for e in (a, b):
                e.kmeter_set_period(KM_P, 4)
                e.tpb_set_period(TPB_P, 96)
                e.scope_configure(256, 100)
                e.scope_set_series(3, 8)
                e.integr_start()
                if host:
                    e.set_host_chunk_bytes(40 * T * 8)                             # two views of the batch: the second starts at stream 34
            if host:
                a.process_any(x, ends)
                b.process_gonio_ends(x, ends)
            else:
                a.process_device_any(dev.data_ptr(), T, ends)
                b.process_device_gonio_ends(dev.data_ptr(), T, ends)
            a.sync(), b.sync()
            same(beside(a, M), beside(b, M))
            got = snap(b)
            same(got, want(one))
            # a second call on the partly closed batch: the ends ride along without a family call
            for e in (a, b):
                if host:
                    e.process(more)
                else:
                    e.process_device(dev2.data_ptr(), 1000)
                e.sync()
            wa, wb = beside(a, M), beside(b, M)
            same(wa, wb)
            assert (wa["tpb_points"] > np.uint64(T // TPB_P)).any() and (wa["scope_points[0]"][closed] <= np.uint64(T // 100)).all()
            assert np.array_equal(a.stream_frames()[0], b.stream_frames()[0]) and np.array_equal(b.stream_frames()[1].astype(bool), ends < T)
            same(snap(b), got, rows=closed, skip=("blocks", "s_gain", "s_drawn", "s_clipped"))


# ---- 6: the state blob --------------------------------------------------------------------------------------------------------------------
def test_a_closed_stream_travels_open(M):
    """export behind a closing call, import into a fresh engine: the closed streams are open, stand at the lock-step fill and go on as the
    restatement's streams do from their snapshots — with the accumulators as the closing left them: zero"""
    ends, x = ENDS(), signal(S, T)
    one = ref_planted(1)
    GE.coverage_ends(one, 1)
    more = signal(S, 1000, 7)
    cfg = dict(CFG, autogain=1)

    def make():
        g = _gonio.Gonio(S, FS, P=P, autogain=True)
        for k in GE.STATE:
            setattr(g, k, getattr(one, k).copy())
        g.img = one.img.copy()
        g.j = T % P                                                        # the lock-step fill
        return g.run(more)
    g = reference(("travel",), make)
    with engine(M, S, **cfg) as a, engine(M, S, **cfg) as b:
        dev = device(x)
        a.process_device_gonio_ends(dev.data_ptr(), T, ends)
        blob = a.state_export()
        assert b.state_import(blob) == S
        assert a.stream_frames()[1].any() and np.array_equal(a.gonio_points()[0], one.updates)
        assert not b.stream_frames()[1].any() and (b.gonio_points()[0] == 0).all()         # open again, the importing engine's lock-step number
        d2 = device(more)
        b.process_device(d2.data_ptr(), 1000)
        b.sync()
        got = snap(b)
        w = dict(img=g.img, drawn=g.drawn, clipped=g.clipped, skipped=g.skipped, gain=bits(g.gain),
                 lp=bits(np.stack([g.lp0, g.lp1], axis=1)), last=bits(np.stack([g.last_x, g.last_y], axis=1)))
        same({k: got[k] for k in w}, w)
        sg, sd, sc = g.series_arrays()                                     # the importing engine's series starts with the block the blob was cut in
        assert got["blocks"].tolist() == [2, 2] and np.array_equal(got["s_gain"], bits(sg))
        assert np.array_equal(got["s_drawn"], sd) and np.array_equal(got["s_clipped"], sc)


# ---- 7: the NS = 64 form ------------------------------------------------------------------------------------------------------------------
def test_the_64_stream_form(M):
    S_, T_, P_ = 16384 + 3, 600, 128
    x = signal(S_, T_, 8)
    r = np.random.default_rng(5)
    ends = r.integers(0, T_ + 1, S_).astype(np.uint64)
    edge = [T_, 0, 1, 63, 64, P_, P_ + 63, P_ + 64, 2 * P_ - 1, 256, 257, 512, T_ - 1]
    for k, v in enumerate(edge):                                           # planted in the first workgroup, in the last full one and in the three lanes behind
        ends[k * 5] = ends[16384 - 64 + k] = v
    ends[16384:] = [T_, P_ + 64, 63]

    def make():
        o = GE.run(x, ends, FS, P=P_, autogain=True, shift=3)
        o.sums = o.img.reshape(S_, -1).sum(axis=1, dtype=np.uint64)
        o.img = None
        return o
    o = reference(("ns64",), make)
    assert (o.r >= 64).any() and o.moved.any() and o.painted.any() and ((o.tail > 0) & (o.tail < 64)).any()
    with engine(M, S_, period_frames=P_, capacity=8, tune_piece=256, shift=3, autogain=1) as e:
        dev = device(x)
        e.process_device_gonio_ends(dev.data_ptr(), T_, ends)
        e.sync()
        got = snap(e)
    got["img"] = got["img"].reshape(S_, -1).sum(axis=1, dtype=np.uint64)
    o.img = o.sums
    w = want(o, 8)
    o.img = None
    same(got, w)
    assert np.array_equal(got["img"], got["drawn"])


@pytest.mark.parametrize("cfg", [dict(autogain=1), dict(gain=4.0)], ids=["autogain", "fixed_gain"])
def test_the_64_stream_form_dense(M, cfg):
    """... and its dense arm (n_streams >= 16384 without ends), at the same shape: a dense call against a call whose every end is the
    call's length — the ENDS instantiations on the same frames, which the test above holds to the restatement.  Equal by bytes."""
    S_, T_, P_ = 16384 + 3, 600, 128
    dev = device(signal(S_, T_, 8))
    got = []
    for ends in (None, np.full(S_, T_, np.uint64)):
        with engine(M, S_, period_frames=P_, capacity=8, tune_piece=256, shift=3, **cfg) as e:
            if ends is None:
                e.process_device(dev.data_ptr(), T_)
            else:
                e.process_device_gonio_ends(dev.data_ptr(), T_, ends)
            e.sync()
            got.append(snap(e))
    dense, open_ = got
    assert dense["blocks"].tolist() == [T_ // P_, T_ // P_] and dense["drawn"].any() and (dense["s_drawn"] > 0).any()
    if "autogain" in cfg:
        assert (dense["s_gain"] != dense["s_gain"][:, :1]).any()           # (the gain moved)
    same(dense, open_)


# ---- 8: the image kernel's other instantiations ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [1, 3])
def test_the_other_shifts(M, shift):
    S_, T_ = 19, 3000
    x = signal(S_, T_, 3)
    ends = np.array([T_, 0, 1, 63, 64, 480, 543, 544, 959, 128, 1024, 2048, 1025, 2999, 1700, 2222, 100, T_, 1234], np.uint64)
    o = reference(("shift", shift), lambda: GE.run(x, ends, FS, P=480, shift=shift, gain=4.0))
    assert (o.r >= 64).any() and o.painted.any() and (o.clipped > 0).any()
    with engine(M, S_, period_frames=480, capacity=8, gain=4.0, shift=shift, tune_piece=1024) as e:
        dev = device(x)
        e.process_device_gonio_ends(dev.data_ptr(), T_, ends)
        e.sync()
        same(snap(e), want(o, 8))
