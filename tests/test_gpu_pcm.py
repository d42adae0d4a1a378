"""Integer PCM in, decoded on the GPU: mtr_engine_process_host_pcm / _device_pcm (include/mtr_engine.h, k_pcm in mtr_source.hip).

The conversion is exact integer-to-float (tests/test_pcm_cpu.py pins mtr_pcm_decode_host to numpy bit for bit), and the float
chunk a PCM call hands the meters is laid out exactly as mtr_engine_process_host stages it.  So the comparison is always

    PCM call   vs   mtr_engine_process_host on pcm_decode (...) of the same integers, same set_host_chunk_bytes

with EVERY record of every meter np.array_equal, seg_stats () equal and the state blobs byte-equal after the last call — no
tolerance anywhere, the SDH's alignment-dependent double sums included.  One case goes against the oracle instead of the
engine's own float path.  No test here asserts a time.
"""
import numpy as np
import pytest

import _signals as sig

pytestmark = pytest.mark.gpu

FORMATS = ["s16", "s24", "s32"]
BITS = {"s16": 16, "s24": 24, "s32": 32}


@pytest.fixture(scope="module")
def M():
    import meters.lv2_amd as m
    return m


def _fmt(M, name):
    return {"s16": M.PCM_S16, "s24": M.PCM_S24, "s32": M.PCM_S32}[name]


def _quant(x, name):
    """float samples to the format's integers: scale, round, clip to the integer range (NaN -> 0); int16 / int32 of x's shape"""
    k = BITS[name] - 1
    with np.errstate(invalid="ignore"):                                  # (widening a signalling NaN of the bit soup)
        v = np.rint(np.nan_to_num(np.asarray(x, np.float64), nan=0.0, posinf=2.0, neginf=-2.0).clip(-2.0, 2.0) * 2.0 ** k)
    v = v.clip(-2.0 ** k, 2.0 ** k - 1).astype(np.int64)
    return v.astype(np.int16 if name == "s16" else np.int32)


def _plant_extremes(q, name):
    """the format's two extreme codes in some streams (q: [S, T, C] or [S, T])"""
    k = BITS[name] - 1
    lo, hi = -(1 << k), (1 << k) - 1
    flat = q.reshape(q.shape[0], -1)
    for s in range(0, q.shape[0], 5):
        flat[s, (7 * s + 3) % flat.shape[1]] = lo
        flat[s, (11 * s + 1) % flat.shape[1]] = hi
        flat[s, flat.shape[1] - 1 - (s % 3)] = hi if s % 2 else lo          # ... and at the very end of a row
    return q


def _raw(q, name):
    """what the entry points take: int16 / int32 as they are, S24 packed little endian as uint8 [S, samples * 3]"""
    if name != "s24":
        return np.ascontiguousarray(q)
    b = np.ascontiguousarray(q.astype("<i4")).view(np.uint8).reshape(q.shape[0], -1, 4)[:, :, :3]
    return np.ascontiguousarray(b).reshape(q.shape[0], -1)


def _cut(q, name, a, b):
    """frames [a, b) of every stream, in the entry points' form"""
    return _raw(q[:, a:b], name)


def _decoded(M, raw, name, like):
    """pcm_decode of the raw samples, shaped like the integer array they came from"""
    return M.pcm_decode(_fmt(M, name), raw).reshape(like.shape)


def _records(M, e, meters):
    """every record of every meter (the list of tests/test_gpu_hostpath.py:_records)"""
    out = {}
    if meters & (M.METER_EBU | M.METER_TRUEPEAK | M.METER_TPBALLIST):
        r = e.results()
        out["o9"] = e.out9()
        out["counts"] = np.array([[x.hist_M_count, x.hist_S_count] for x in r])
        out["tp"] = np.array([[x.truepeak[0], x.truepeak[1], x.truepeak_call[0], x.truepeak_call[1]] for x in r], np.float32)
        out["tpb"] = np.array([[x.tpb_level[0], x.tpb_level[1], x.tpb_peak[0], x.tpb_peak[1]] for x in r], np.float32)
    if meters & M.METER_TRUEPEAK:
        out["tpc_hold"], out["tpc_last"] = e.truepeak_channels()
    if meters & M.METER_EBU:
        out["hm"], out["hs"] = e.histograms()
        out["frag"] = e.fragment_powers()
    if meters & M.METER_SPECTR30:
        sp = e.spectrum()
        out["val"], out["max"] = sp["val"], sp["max"]
    if meters & M.METER_BITSTATS:
        b = e.bitstats()
        out.update({"b_" + k: v for k, v in b.items()})
    if meters & M.METER_SIGDIST:
        d = e.sigdist()
        out.update({"d_" + k: v for k, v in d.items()})
    if meters & M.METER_DR14:
        out["dr"] = np.array([[x.m_rms[0], x.m_rms[1], x.m_peak[0], x.m_peak[1], x.dr[0], x.dr[1], x.dr_total, x.block_count] for x in e.dr14()])
    if meters & M.METER_KMETER:
        out["km_rms"], out["km_peak"] = e.kmeter_read()
    return out


def _same(a, b, what=""):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


def _chunk_bytes(n, C, chunk_streams):
    """host_chunk_bytes that puts chunk_streams streams of an n-frame call into a chunk (decoded float bytes, staged stride)"""
    return chunk_streams * (((n + 3) & ~3) if C != 2 else ((n + 1) & ~1)) * C * 4


def _pcm_vs_float(M, q, name, calls, meters, fs=48000.0, chunk_streams=5, **kw):
    """the PCM host form against process_host on the decoded floats, call by call; returns the PCM engine's seg_stats"""
    S = q.shape[0]
    C = 1 if q.ndim == 2 else q.shape[2]
    got = []
    for pcm in (True, False):
        recs = []
        with M.Engine(S, fs, meters, n_channels=C, **kw) as e:
            if meters & M.METER_EBU:
                e.integr_start()
            pos, want_chunks, want_bytes = 0, 0, 0
            for n in calls:
                e.set_host_chunk_bytes(_chunk_bytes(n, C, chunk_streams))
                raw = _cut(q, name, pos, pos + n)
                if pcm:
                    e.process_pcm(raw, _fmt(M, name))
                else:
                    e.process(_decoded(M, raw, name, q[:, pos:pos + n]))
                recs.append(_records(M, e, meters))
                pos += n
                want_chunks += -(-S // chunk_streams)
                want_bytes += S * n * C * BITS[name] // 8
            assert pos == q.shape[1]
            chunks, nbytes, ms = e.pcm_stats()
            assert (chunks, nbytes, ms) == ((want_chunks, want_bytes, 0.0) if pcm else (0, 0, 0.0))
            got.append((recs, e.seg_stats(), e.state_export(), e.stream_frames()[0]))
    (a, seg_a, blob_a, fr_a), (b, seg_b, blob_b, fr_b) = got
    assert seg_a == seg_b                                                # the same kernels served both
    for i, (x, y) in enumerate(zip(a, b)):
        _same(x, y, (name, "call", i))
    assert blob_a == blob_b
    assert np.array_equal(fr_a, fr_b)
    return seg_a


T4 = 2400 * 30 + 1234
CALLS4 = [2400 * 11, 2400 * 7 + 777, 1, T4 - (2400 * 18 + 778)]          # one of 1 frame; 17577 frames: not a multiple of 16 samples in any layout


def _stereo(S, T, seed):
    return np.stack([sig.g2(T, seed + s) * np.float32(2.0 ** -(s % 4)) for s in range(S)])


CONFIGS = {
    # name: (meters, channels, fs, chunk_streams, engine knobs, k_seg calls expected or None)
    "ebu_tp_bank": ("EBU|TRUEPEAK|SPECTR30", 2, 48000.0, 5, {}, 0),
    "ebu_tp_bank_seg": ("EBU|TRUEPEAK|SPECTR30", 2, 48000.0, 5, dict(tune_segments=3), 3),
    "ebu": ("EBU", 2, 48000.0, 5, {}, None),
    "tp_441": ("TRUEPEAK", 2, 44100.0, 36, dict(tune_segments=2), None),
    "tpb_dr_km": ("TPBALLIST|DR14|KMETER", 2, 48000.0, 7, {}, None),
    "mono_int": ("BITSTATS|SIGDIST", 1, 48000.0, 3, {}, None),
    "five_ch": ("EBU|TRUEPEAK", 5, 48000.0, 5, {}, None),
}


def _mask(M, names):
    m = 0
    for n in names.split("|"):
        m |= getattr(M, "METER_" + n)
    return m


@pytest.fixture(scope="module")
def floats4():
    """the float signals of the configurations, by channel count: 37 streams each"""
    S = 37
    st = _stereo(S, T4, 300)
    mono = st[:, :, 0].copy()
    soup = sig.g5(T4, 4242)                                              # bit patterns: NaN / Inf / huge / denormal, quantised to 0 and the clip codes
    mono[4] = soup
    mono[9, ::3] = soup[::3]
    five = np.concatenate([st, _stereo(S, T4, 900), st[:, :, :1] * np.float32(0.7)], 2)
    return {2: st, 1: mono, 5: np.ascontiguousarray(five)}


@pytest.mark.timeout(900)
@pytest.mark.parametrize("cfg", list(CONFIGS))
@pytest.mark.parametrize("name", FORMATS)
def test_host_pcm_is_the_float_host_path_bit_for_bit(M, floats4, name, cfg):
    names, C, fs, chunk_streams, kw, want_seg = CONFIGS[cfg]
    q = _plant_extremes(_quant(floats4[C], name), name)
    seg = _pcm_vs_float(M, q, name, CALLS4, _mask(M, names), fs=fs, chunk_streams=chunk_streams, **kw)
    if want_seg is not None:
        assert seg[0] == want_seg, seg                                   # k_seg served every call but the 1-frame one / none


def test_pcm_stats_with_timing(M):
    """decode_ms sums the decode kernels' times while timing is on, and the decode lies inside each chunk's whole-call span"""
    S, n = 12, 48000
    q = _quant(_stereo(S, n, 40), "s16")
    with M.Engine(S, 48000.0, M.METER_EBU | M.METER_TRUEPEAK) as e:
        e.set_host_chunk_bytes(_chunk_bytes(n, 2, 5))
        e.process_pcm(q)
        assert e.pcm_stats() == (3, S * n * 2 * 2, 0.0)
        e.timing_enable(True)
        e.process_pcm(q)
        chunks, nbytes, ms = e.pcm_stats()
        assert (chunks, nbytes) == (6, 2 * S * n * 2 * 2) and ms > 0.0
        t = e.timing_calls()
        assert t.shape[0] == 3 and (t[:, 3] > 0).all()
        assert t[:, 3].sum() >= ms                                       # the spans hold the three decodes
        assert e.pcm_stats()[2] == ms                                    # nothing new since


def _device_rows(torch, raw, row_bytes, pitch, base, fill):
    """the rows of `raw` (uint8 [S, row_bytes]) in a device buffer at byte `base` + s * pitch, every other byte `fill`"""
    S = raw.shape[0]
    host = np.full(base + S * pitch + 64, fill, np.uint8)
    for s in range(S):
        host[base + s * pitch: base + s * pitch + row_bytes] = raw[s]
    return torch.from_numpy(host).cuda()


def _device_vs_host(M, q, name, meters, stride, base, fs=48000.0, chunk_streams=4, calls=1):
    import torch
    S, n = q.shape[0], q.shape[1]
    C = 1 if q.ndim == 2 else q.shape[2]
    sb = BITS[name] // 8
    raw = _raw(q, name).view(np.uint8).reshape(S, -1)
    assert raw.shape[1] == n * C * sb
    # bytes that decode to (almost) full scale at every alignment: 0x7f7f, 0x7f7f7f, 0x7f7f7f7f
    buf = _device_rows(torch, raw, n * C * sb, stride * C * sb, base, 0x7f)
    got = []
    for device in (True, False):
        with M.Engine(S, fs, meters, n_channels=C) as e:
            if meters & M.METER_EBU:
                e.integr_start()
            e.set_host_chunk_bytes(_chunk_bytes(n, C, chunk_streams))
            recs = []
            for _ in range(calls):
                if device:
                    e.process_device_pcm(buf.data_ptr() + base, _fmt(M, name), n, stride=stride, stream=torch.cuda.current_stream().cuda_stream)
                else:
                    e.process_pcm(_raw(q, name), _fmt(M, name))
                recs.append(_records(M, e, meters))
            got.append((recs, e.state_export(), e.pcm_stats()[:2]))
    for x, y in zip(got[0][0], got[1][0]):
        _same(x, y, (name, stride, base))
    assert got[0][1] == got[1][1] and got[0][2] == got[1][2]
    peak = np.abs(M.pcm_decode(_fmt(M, name), _raw(q, name))).max()
    assert peak < 0.9                                                    # (a gap byte that got in would have raised a peak)


def test_device_pcm_rows_on_every_byte_phase(M):
    """Rows in device memory that start anywhere: s16 on odd 2-byte positions (mono, odd stride), s24 on every byte phase 0 .. 15
    (mono, odd stride: 3 * stride * s mod 16 walks all of them), row lengths that are no multiple of 16 bytes, and the gaps between
    the rows filled with bytes that would decode to full scale: equal to the host PCM form on the tightly packed data."""
    n, stride, S = 20011, 20013, 17
    assert {(3 * stride * s) % 16 for s in range(S)} == set(range(16)) and (n * 3) % 16 and (n * 2) % 16
    mono = np.stack([sig.g2(n, 70 + s)[:, 0] for s in range(S)]) * np.float32(0.8)
    meters = M.METER_TPBALLIST | M.METER_BITSTATS | M.METER_SIGDIST
    _device_vs_host(M, _quant(mono, "s24"), "s24", meters, stride, 0, calls=2)
    assert {(2 * stride * s) % 16 for s in range(S)} == set(range(0, 16, 2))
    _device_vs_host(M, _quant(mono, "s16"), "s16", meters, stride, 0, calls=2)
    _device_vs_host(M, _quant(mono, "s16"), "s16", meters, stride, 6)
    _device_vs_host(M, _quant(mono, "s32"), "s32", meters, stride, 4)


@pytest.mark.parametrize("name", FORMATS)
def test_device_pcm_stereo_loudness(M, name):
    """... and the loudness / true-peak kernels behind the device form: aligned rows with a gap (the 16-byte path with its
    single-sample tail) and rows off by an odd number of samples"""
    n, S = 2400 * 5 + 1237, 9
    q = _quant(_stereo(S, n, 500) * np.float32(0.8), name)
    sb = BITS[name] // 8
    meters = M.METER_EBU | M.METER_TRUEPEAK
    assert (n * 2 * sb) % 16
    _device_vs_host(M, q, name, meters, n + 8 - n % 8 + 8, 0, calls=2)   # a stride of whole 16 bytes in every format: aligned rows
    _device_vs_host(M, q, name, meters, n + 3, sb)                       # one sample into the buffer, odd stride


def _snap(e):
    hm, hs = e.histograms()
    r = e.results()
    return dict(o9=e.out9(), hm=hm, hs=hs, tpc=np.concatenate(e.truepeak_channels(), 1),
                tp=np.array([[x.truepeak[0], x.truepeak[1], x.truepeak_call[0], x.truepeak_call[1]] for x in r], np.float32))


@pytest.mark.parametrize("name", FORMATS)
def test_lengths(M, name):
    fs, n = 48000.0, 2400 * 6 + 500
    S = 8
    q = _plant_extremes(_quant(_stereo(S, 2 * n, 40), name), name)
    frames = np.array([n, 2400 * 3 + 1001, 0, n, 1, 2400 * 2, n - 1, n], np.uint64)   # open, closed inside a fragment, closed at 0, ...
    closed = np.nonzero(frames < n)[0]
    meters = M.METER_EBU | M.METER_TRUEPEAK
    res = []
    for pcm in (True, False):
        with M.Engine(S, fs, meters) as e:
            e.integr_start()
            e.set_host_chunk_bytes(_chunk_bytes(n, 2, 3))
            raw0, raw1 = _cut(q, name, 0, n), _cut(q, name, n, 2 * n)
            if pcm:
                e.process_pcm(raw0, _fmt(M, name), frames=frames)
            else:
                e.process_lengths(_decoded(M, raw0, name, q[:, :n]), frames)
            a, fa = _snap(e), e.stream_frames()
            # a following call leaves the closed streams untouched
            if pcm:
                e.process_pcm(raw1, _fmt(M, name))
            else:
                e.process(_decoded(M, raw1, name, q[:, n:]))
            b, fb = _snap(e), e.stream_frames()
            for k in a:
                assert np.array_equal(a[k][closed], b[k][closed]), k
            assert np.array_equal(fa[0], frames) and np.array_equal(fa[1], frames < n)
            assert np.array_equal(fb[0], np.where(frames < n, frames, 2 * n)) and np.array_equal(fb[1], fa[1])
            res.append((a, b, e.state_export()))
    _same(res[0][0], res[1][0], "the call with lengths")
    _same(res[0][1], res[1][1], "the call behind it")
    assert res[0][2] == res[1][2]


def test_lengths_refused(M):
    ok = np.zeros(1, np.uint64)
    for meters, ch in [(M.METER_DR14, 2), (M.METER_KMETER, 2), (M.METER_EBU | M.METER_SPECTR30, 2)]:
        with M.Engine(1, 48000.0, meters, n_channels=ch) as e:
            y = np.zeros((1, 100, ch), np.int16)
            assert M.lib.mtr_engine_process_host_pcm(e._h, y.ctypes.data, M.PCM_S16, 100, 100, ok.ctypes.data) == -2, meters
            assert M.lib.mtr_engine_process_device_pcm(e._h, y.ctypes.data, M.PCM_S16, 100, 100, ok.ctypes.data, None) == -2, meters
            assert e.pcm_stats()[:2] == (0, 0)
    S, n = 4, 3000
    q = _quant(_stereo(S, 2 * n, 9), "s16")
    with M.Engine(S, 48000.0, M.METER_EBU | M.METER_TRUEPEAK) as e:
        e.integr_start()
        e.process_pcm(q[:, :n])
        before, fr = _snap(e), e.stream_frames()
        bad = np.array([n, n + 1, 0, 5], np.uint64)
        tail = np.ascontiguousarray(q[:, n:])
        assert M.lib.mtr_engine_process_host_pcm(e._h, tail.ctypes.data, M.PCM_S16, n, n, bad.ctypes.data) == -1
        _same(before, _snap(e), "frames[s] > n_frames")
        after = e.stream_frames()
        assert np.array_equal(fr[0], after[0]) and np.array_equal(fr[1], after[1])


def test_argument_errors_leave_the_engine_unchanged(M):
    import torch
    S, n = 4, 5000
    q = _quant(_stereo(S, n, 3), "s16")
    dev = torch.from_numpy(q).cuda()
    with M.Engine(S, 48000.0, M.METER_EBU | M.METER_TRUEPEAK) as e:
        e.integr_start()
        e.process_pcm(q[:, :2000])
        before, fr, stats = _snap(e), e.stream_frames(), e.pcm_stats()
        L = M.lib
        for fmt in (0, 4):
            assert L.mtr_engine_process_host_pcm(e._h, q.ctypes.data, fmt, 3000, n, None) == -1
            assert L.mtr_engine_process_device_pcm(e._h, dev.data_ptr(), fmt, 3000, n, None, None) == -1
        assert L.mtr_engine_process_host_pcm(e._h, q.ctypes.data, M.PCM_S16, 3000, 2999, None) == -1     # stride < n_frames
        assert L.mtr_engine_process_device_pcm(e._h, dev.data_ptr(), M.PCM_S16, 3000, 2999, None, None) == -1
        assert L.mtr_engine_process_host_pcm(e._h, None, M.PCM_S16, 3000, n, None) == -1
        assert L.mtr_engine_process_device_pcm(e._h, None, M.PCM_S16, 3000, n, None, None) == -1
        assert L.mtr_engine_process_host_pcm(e._h, q.ctypes.data, M.PCM_S16, 0, n, None) == 0           # nothing to do
        _same(before, _snap(e), "after argument errors")
        after = e.stream_frames()
        assert np.array_equal(fr[0], after[0]) and np.array_equal(fr[1], after[1]) and (after[0] == 2000).all()
        assert e.pcm_stats() == stats
    with M.Engine(S, 48000.0) as e:
        for bad in (np.zeros((S, 10, 2), np.float32), np.zeros((S, 10, 3), np.int16), np.zeros((S + 1, 10, 2), np.int16),
                    np.zeros((S, 61), np.uint8)):
            with pytest.raises(ValueError):
                e.process_pcm(bad, M.PCM_S24 if bad.dtype == np.uint8 else None)
        with pytest.raises(ValueError):
            e.process_pcm(np.zeros((S, 60), np.uint8))                   # uint8 bytes without a format


def test_s16_batch_against_oracle(M, oracle):
    """End to end against the oracle, not against the engine's own float path: the s16 quantisation of the ragged batch of
    tests/test_gpu_parity.py:test_batch_against_oracle, the oracle run on the decoded floats, that test's tolerances (DB_TOL = 1e-3 dB
    on M / maxM / S / maxS, 2e-5 relative on the fragment powers, 2e-6 relative on the true peak)."""
    S, T = 37, 48000 * 3 + 777
    x = np.stack([sig.lcg_noise(T, 1000 + s, 2.0 ** -(s % 5)) for s in range(S)])
    x[5] *= np.linspace(0, 1, T, dtype=np.float32)[:, None]
    x[6, :, 1] = 0
    q = _quant(x, "s16")
    xf = M.pcm_decode(M.PCM_S16, q)
    with M.Engine(S, 48000.0, M.METER_EBU | M.METER_TRUEPEAK) as e:
        e.integr_start()
        e.process_pcm(q)
        out9, tp, frag = e.out9(), e.truepeak(), e.fragment_powers()
    for s in range(S):
        o = oracle.ebu(xf[s], 48000.0, 2400, want_frag=True)
        assert np.allclose(out9[s, :4], o["out9"][:4], atol=1e-3), s
        assert np.allclose(frag[s], o["frag_power"], rtol=2e-5, atol=1e-30), s
        assert np.allclose(tp[s], oracle.tp(xf[s], 48000.0, 8192), rtol=2e-6), s


@pytest.mark.timeout(900)
def test_big_s16_batch_through_k_seg(M):
    """A batch big enough for the lane = segment kernel by the auto route — 4096 streams x 3.2 s of s16, 2.5 GB of host memory (the
    planner sends 4096 streams to k_seg from 64 whole fragments on: mtr_plan_query; one second of them stays with k_kwtp16) —:
    equal to the float host path, and the tail deferred for the same calls in both."""
    S, n = 4096, 2400 * 64
    assert M.plan_query(S, n)["uses_seg"] == 1
    rng = np.random.default_rng(12)
    q = rng.integers(-12000, 12000, (S, n, 2), dtype=np.int16)
    q[:, :, 1] >>= (np.arange(S) % 5).astype(np.int16)[:, None]
    q[17, 4711, 0], q[4095, n - 1, 1] = -32768, 32767
    got = []
    for pcm in (True, False):
        with M.Engine(S, 48000.0, M.METER_EBU | M.METER_TRUEPEAK) as e:
            e.integr_start()
            if pcm:
                e.process_pcm(q)
            else:
                e.process(M.pcm_decode(M.PCM_S16, q))
            got.append((_snap(e), e.seg_stats(), e.deferred_calls(), e.state_export()))
    assert got[0][1] == got[1][1] and got[0][1][0] >= 1, got[0][1]      # k_seg took the chunks
    assert got[0][2] == got[1][2]
    _same(got[0][0], got[1][0], "4096 x 3.2 s")
    assert got[0][3] == got[1][3]
