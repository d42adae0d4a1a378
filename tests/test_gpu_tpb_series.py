"""The true-peak bar's reading series (include/mtr_tpb.h, the SERIES instantiations of k_tpb) on the GPU.

The oracle is TruePeakdsp itself (oracle.lib.mo_tp_init / mo_tp_process / mo_tp_read2), one fresh object per (stream, channel), fed
process (P frames) + read2 block by block.  The bound is the meter's own, TPB_REL = 4e-6 of the value (tests/test_gpu_parity.py:41): the
chains re-associate two attacks into one pair map and the interpolator runs on the matrix pipe, a few ulps from the reference's sequence
at any call size, 17 frames and 1 frame included — a block end adds no arithmetic of its own to that."""
import numpy as np
import pytest

import _signals as sig

pytestmark = pytest.mark.gpu

TPB_REL = 4e-6
ERR_ARG, ERR_UNSUPPORTED, ERR_STATE = -1, -2, -7
CUTS = (0, 1, 16, 33, 700, 717)        # + T: a 1-frame call, a 15-frame call, a 17-frame call that holds a block end, ...
T0 = 5003
QUIET = {5: 1e-2, 6: 1e-3, 7: 1e-4}    # -40 / -60 / -80 dBFS


@pytest.fixture(scope="module")
def M():
    import meters.lv2_amd as m
    assert (m.engine.ERR_ARG, m.engine.ERR_UNSUPPORTED, m.engine.ERR_STATE) == (ERR_ARG, ERR_UNSUPPORTED, ERR_STATE)
    return m


@pytest.fixture(scope="module")
def oracle():
    from _oracle import Oracle
    return Oracle()


_NOISE = {}


def noise(S, T):
    """[S][T][2]: lcg noise at 2^-(s % 4), and -40 / -60 / -80 dBFS on streams 5, 6, 7 (mod 8)"""
    if (S, T) not in _NOISE:
        _NOISE[S, T] = np.stack([sig.lcg_noise(T, 700 + s, 2.0 ** -(s % 4) * QUIET.get(s % 8, 1.0)) for s in range(S)])
    return _NOISE[S, T]


_WANT = {}


def want_points(oracle, key, ch, fs, P):
    """[T // P][2] = (m, p) of every whole block of the mono signal `ch`; computed once per `key`"""
    k = (key, fs, P)
    if k not in _WANT:
        _WANT[k] = oracle.tp_process_seq(ch, fs, P)[:ch.size // P]
    return _WANT[k]


def calls_of(T, cuts=CUTS):
    c = tuple(cuts) + (T,)
    return list(zip(c[:-1], c[1:]))


def res_of(e, chn):
    r = e.results()
    return (np.array([[r[s].tpb_level[c] for c in range(chn)] for s in range(e.n_streams)], np.float32),
            np.array([[r[s].tpb_peak[c] for c in range(chn)] for s in range(e.n_streams)], np.float32))


def same(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def run(M, feed, chn, fs, P, calls, cap=2048, each_call=None):
    """feed [S][T][chn] (or [S][T]) through the host path, call by call -> (level, peak, n, dropped, results)"""
    with M.Engine(feed.shape[0], fs, M.METER_TPBALLIST, n_channels=chn) as e:
        e.tpb_set_period(P, cap)
        assert e.tpb_period() == (P, cap)
        for a, b in calls:
            e.process(np.ascontiguousarray(feed[:, a:b]))
            if each_call:
                each_call(e, b)
        return e.tpb_series() + (res_of(e, chn),)


def hold(got, want, what):
    assert abs(got - want) <= TPB_REL * want + 1e-37, (what, got, want)


# ---- 1. parity, block by block ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs,P,T", [(48000.0, 16, T0), (48000.0, 17, T0), (48000.0, 23, T0), (48000.0, 100, T0), (48000.0, 4800, T0),
                                    (48000.0, 8192, 2 * 8192 + 5), (44100.0, 100, T0)])
@pytest.mark.parametrize("chn,S", [(2, 33), (1, 65)])
def test_every_block_matches_truepeakdsp(M, oracle, chn, S, fs, P, T):
    """Two workgroups, the second with one stream; calls of 1, 15 and 17 frames, a call that completes no block at P = 4800, blocks that
    straddle calls, block ends at every position of a chunk (P = 17, 23) and in every chunk (P = 16)."""
    x = noise(65, T)[:S]
    feed = x if chn == 2 else np.ascontiguousarray(x[:, :, 0])

    def each_call(e, end):
        # results () are the last completed block's, bit for bit as the series holds them; 0.0f before the first
        lv, pk, n, d = e.tpb_series()
        assert n == end // P and d == 0
        rl, rp = res_of(e, chn)
        if n == 0:
            assert not rl.any() and not rp.any()
        else:
            assert same(rl, lv[:, -1]) and same(rp, pk[:, -1])

    lv, pk, n, d, (rl, rp) = run(M, feed, chn, fs, P, calls_of(T), each_call=each_call)
    assert n == T // P and d == 0 and lv.shape == (S, T // P, chn) == pk.shape
    for s in (0, 1, 5, 6, 7, 31, 32, S - 1):
        for c in range(chn):
            w = want_points(oracle, ("noise", s, c, T), np.ascontiguousarray(x[s, :, c]), fs, P)
            for k in range(n):
                hold(lv[s, k, c], w[k, 0], ("level", s, c, k))
                hold(pk[s, k, c], w[k, 1], ("peak", s, c, k))


# ---- 2. the arithmetic at a block's boundary shows --------------------------------------------------------------------------------------
def test_silence_and_states_past_the_clamp(M, oracle):
    """Digital silence: from the second block on the level is about 1e-20, the + 1e-20f of a block's end alone (truepeakdsp.cc:86-87) — an
    engine that adds it per call, not per block, fails the same relative bound.  Noise at amplitude 64: the oracle's states stand near
    80 and 90 at every block's end (checked below: > 20) and are clamped to 20 where the next block starts (:54-55)."""
    import ctypes as C
    from _oracle import MoTp
    fs, P = 48000.0, 4800
    T = 3 * P + 11
    loud = sig.lcg_noise(T, 900, 64.0)
    x = np.concatenate([noise(33, T), np.zeros((1, T, 2), np.float32), loud[None]])
    for c in range(2):                                               # the oracle's own states at a block's end
        t = MoTp()
        oracle.lib.mo_tp_init(C.byref(t), fs)
        oracle.lib.mo_tp_process(C.byref(t), np.ascontiguousarray(loud[:P, c]), P)
        assert t.z1 > 20 and t.z2 > 20, (t.z1, t.z2)
    lv, pk, n, d, _ = run(M, x, 2, fs, P, calls_of(T, range(0, T, 1000)))
    assert n == 3 and d == 0
    for s, key in ((33, "silence"), (34, "loud"), (0, "n0"), (7, "n7")):
        for c in range(2):
            w = want_points(oracle, (key, c, T), np.ascontiguousarray(x[s, :, c]), fs, P)
            if key == "silence":
                assert w[0, 0] == 0 and 0.5e-20 < w[1, 0] < 2e-20 and 1e-20 < w[2, 0] < 3e-20, w
            for k in range(n):
                hold(lv[s, k, c], w[k, 0], ("level", key, c, k))
                hold(pk[s, k, c], w[k, 1], ("peak", key, c, k))


# ---- 3. capacity ------------------------------------------------------------------------------------------------------------------------
def test_capacity_drops_and_counts(M):
    fs, P, S = 48000.0, 100, 33
    x = noise(65, T0)[:S]
    big = run(M, x, 2, fs, P, calls_of(T0))
    with M.Engine(S, fs, M.METER_TPBALLIST) as e:
        e.tpb_set_period(P, 5)
        for a, b in calls_of(T0):
            e.process(np.ascontiguousarray(x[:, a:b]))
        lv, pk, n, d = e.tpb_series()
        assert n == big[2] == T0 // P and d == n - 5
        assert lv.shape == (S, 5, 2) and same(lv, big[0][:, :5]) and same(pk, big[1][:, :5])
        assert same(res_of(e, 2)[0], big[0][:, -1]) and same(res_of(e, 2)[1], big[1][:, -1])   # (the last block's, kept or not)
        import ctypes as C
        n_, d_ = C.c_uint32(), C.c_uint32()
        buf = np.full((2, S * 3 * 2 + 64), -1.0, np.float32)           # output arrays of capacity 3: only three points per stream are copied
        assert M.lib.mtr_engine_tpb_series(e._h, 0, S, buf[0].ctypes.data, buf[1].ctypes.data, 3, C.byref(n_), C.byref(d_)) == 0
        lev3, pk3 = buf[0, :S * 6].reshape(S, 3, 2), buf[1, :S * 6].reshape(S, 3, 2)
        assert (n_.value, d_.value) == (n, d) and same(lev3, big[0][:, :3]) and same(pk3, big[1][:, :3])
        assert (buf[:, S * 6:] == -1.0).all()
        # ... and either pointer may be NULL
        only = np.full((S, 3, 2), -1.0, np.float32)
        assert M.lib.mtr_engine_tpb_series(e._h, 0, S, None, only.ctypes.data, 3, None, None) == 0 and same(only, pk3)


# ---- 4. every way in gives the same bits ------------------------------------------------------------------------------------------------
def test_paths_agree_bit_for_bit(M):
    import torch
    fs, P, S, T = 48000.0, 23, 37, T0
    pcm = np.round(noise(65, T)[:S] * 32767).astype(np.int16)
    x = M.engine.pcm_decode(M.PCM_S16, pcm)                            # exact in 16 bits
    calls = calls_of(T)
    st = torch.cuda.current_stream().cuda_stream

    def series(e):
        lv, pk, n, d = e.tpb_series()
        assert n == T // P and d == 0
        return lv, pk, *res_of(e, 2)

    def device(stride, off):
        flat = torch.zeros(S * stride * 2 + 8, dtype=torch.float32, device="cuda")
        flat[off:off + S * stride * 2].view(S, stride, 2)[:, :T] = torch.from_numpy(x).cuda()
        with M.Engine(S, fs, M.METER_TPBALLIST) as e:
            e.tpb_set_period(P, 512)
            for a, b in calls:
                e.process_device(flat.data_ptr() + 4 * (off + a * 2), b - a, stride, st)
            return series(e)

    want = device(T + 1, 0)                                            # streams on 16 bytes: whole chunks by LDS-DMA
    assert np.all(want[0][:5] > 0)                                     # (stream 7, -98 dBFS, is digital silence in 16 bits)
    for got in (device(T + 5, 2),):                                    # a view that starts on 8 bytes: plain loads
        assert all(same(g, w) for g, w in zip(got, want))
    with M.Engine(S, fs, M.METER_TPBALLIST) as e:                      # the host path, seven streams per chunk
        e.tpb_set_period(P, 512)
        for a, b in calls:
            e.set_host_chunk_bytes(7 * ((b - a + 1) & ~1) * 8)
            e.process(np.ascontiguousarray(x[:, a:b]))
        assert all(same(g, w) for g, w in zip(series(e), want))
    dev16 = torch.from_numpy(pcm).cuda()                               # S16 PCM in device memory
    with M.Engine(S, fs, M.METER_TPBALLIST) as e:
        e.tpb_set_period(P, 512)
        for a, b in calls:
            e.process_device_pcm(dev16.data_ptr() + a * 4, M.PCM_S16, b - a, T, stream=st)
        assert all(same(g, w) for g, w in zip(series(e), want))
    del dev16


# ---- 5. the state blob ------------------------------------------------------------------------------------------------------------------
def test_state_travels_inside_a_block(M):
    fs, P, S = 48000.0, 100, 33
    x = noise(65, T0)[:S]
    calls = calls_of(T0)
    at = [b for _, b in calls].index(717) + 1                          # export behind the call that ends at frame 717: 17 frames into a block
    with M.Engine(S, fs, M.METER_TPBALLIST) as e, M.Engine(S, fs, M.METER_TPBALLIST) as f, M.Engine(S, fs, M.METER_TPBALLIST) as g:
        e.tpb_set_period(P, 64)
        for a, b in calls[:at]:
            e.process(np.ascontiguousarray(x[:, a:b]))
        blob = e.state_export()
        assert len(blob) == e.state_bytes(S) == g.state_bytes(S) + S * 24      # one more section: period, fill, two maxima per channel
        # ... into an engine of no period, or of another: refused, engine unchanged
        for other, p in ((g, 0), (g, 101)):
            other.tpb_set_period(p, 64)
            before = (other.state_export(), other.tpb_period(), other.tpb_series()[2], *res_of(other, 2))
            with pytest.raises(M.EngineError) as err:
                other.state_import(blob)
            assert err.value.code == ERR_STATE, str(err.value)
            after = (other.state_export(), other.tpb_period(), other.tpb_series()[2], *res_of(other, 2))
            assert all(same(u, v) if isinstance(u, np.ndarray) else u == v for u, v in zip(before, after))
        f.tpb_set_period(P, 64)
        assert f.state_import(blob) == S
        n0 = e.tpb_series()[2]
        assert n0 == 7 and f.tpb_series()[2] == 0
        for a, b in calls[at:]:
            for eng in (e, f):
                eng.process(np.ascontiguousarray(x[:, a:b]))
        le, pe, ne, _ = e.tpb_series()
        lf, pf, nf, _ = f.tpb_series()
        assert ne == T0 // P and nf == ne - n0
        assert same(le[:, n0:], lf) and same(pe[:, n0:], pf)
        assert all(same(u, v) for u, v in zip(res_of(e, 2), res_of(f, 2)))
        assert e.state_export() == f.state_export()


def test_period_zero_is_the_engine_as_it_was(M):
    x = noise(65, T0)[:33]
    out = []
    for setp in (False, True):
        with M.Engine(33, 48000.0, M.METER_TPBALLIST) as e:
            if setp:
                e.tpb_set_period(0, 0)
            rec = []
            for a, b in calls_of(T0):
                e.process(np.ascontiguousarray(x[:, a:b]))
                rec.extend(res_of(e, 2))
            assert e.tpb_series()[2:] == (0, 0)
            out.append((np.stack(rec), e.state_export()))
    assert same(out[0][0], out[1][0]) and out[0][1] == out[1][1]


# ---- 6. the surface ---------------------------------------------------------------------------------------------------------------------
def test_surface(M):
    import torch
    fs, P, S = 48000.0, 4800, 5
    T = 2 * P + 77
    x = noise(65, T)[:S]
    dev = torch.from_numpy(x).cuda()

    def snap(e):
        return [e.state_export(), e.tpb_period(), *e.tpb_series(), *res_of(e, 2)]

    def unchanged(a, b):
        return all(same(u, v) if isinstance(u, np.ndarray) else u == v for u, v in zip(a, b))

    def refused(code, f, *args, **kw):
        with pytest.raises(M.EngineError) as err:
            f(*args, **kw)
        assert err.value.code == code, (err.value.code, str(err.value))

    with M.Engine(S, fs, M.METER_DR14) as e:                           # an engine without the bit
        before = e.state_export()
        refused(ERR_ARG, e.tpb_set_period, P, 64)
        refused(ERR_ARG, e.tpb_period)
        refused(ERR_ARG, e.tpb_series)
        assert e.state_export() == before
    with M.Engine(S, fs, M.METER_TPBALLIST) as e:
        e.tpb_set_period(P, 64)
        before = snap(e)
        for bad in (1, 15, 8193):
            refused(ERR_ARG, e.tpb_set_period, bad, 64)
            assert unchanged(snap(e), before)
        e.tpb_set_period(16, 4)                                        # (the edges themselves are taken)
        e.tpb_set_period(8192, 4)
        e.tpb_set_period(P, 64)
        e.process_device(dev.data_ptr(), 7001, stride=T)
        before = snap(e)
        assert before[4] == 1
        for p in (2400, 0, P):
            refused(ERR_STATE, e.tpb_set_period, p, 64)                 # after a process call
            assert unchanged(snap(e), before)
        # the calls with per-stream lengths refuse a TPBALLIST engine, with a period as without
        full = np.full(S, 1000, np.uint64)
        for name in ("lengths", "tracks", "ragged", "ends"):
            refused(ERR_UNSUPPORTED, getattr(e, "process_device_" + name), dev.data_ptr(), 1000, full, T)
            refused(ERR_UNSUPPORTED, getattr(e, "process_" + name), x[:, :1000], full)
        assert unchanged(snap(e), before)
        e.process_device(dev.data_ptr() + 7001 * 8, T - 7001, stride=T)
        first = snap(e)
        assert first[4] == 2
        e.reset()                                                      # empties the series and the open block, keeps P
        assert e.tpb_period() == (P, 64) and e.tpb_series()[2:] == (0, 0)
        assert not res_of(e, 2)[0].any() and not res_of(e, 2)[1].any()
        e.process_device(dev.data_ptr(), 7001, stride=T)
        e.process_device(dev.data_ptr() + 7001 * 8, T - 7001, stride=T)
        assert unchanged(snap(e), first)
    del dev
