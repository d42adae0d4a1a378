"""Track lengths for the whole-track meters: mtr_engine_process_device_tracks / _host_tracks on the GPU.

The semantics are those of the _lengths pair (a stream advances by frames[s] <= n_frames frames of a call, frames[s] < n_frames closes
it until mtr_engine_reset), for engines of EBU, TRUEPEAK, DR14, KMETER, BITSTATS and SIGDIST in any combination.  Held here, at 48 and
44.1 kHz:
  * identity: lengths all n_frames give bit for bit what process_device gives (getters, state blob), each meter alone and
    EBU|TRUEPEAK|DR14|KMETER together; the open streams of a ragged batch are bit for bit the same streams of a dense batch;
  * whatever lies past a stream's end (NaN, Inf, 1e30, denormals) changes nothing of any stream, bit for bit;
  * each closed stream against the committed restatement (mo_dr14_run, mo_kmeter_*, Oracle.bitstats, Oracle.sigdist) fed exactly its
    own frames in the same call blocks, the last one truncated, at the tolerances of tests/test_gpu_dr14.py (DR_TOL),
    tests/test_gpu_kmeter.py (1e-5 relative rms, exact peak) and tests/test_gpu_intstat.py (bit-exact tables, 1e-12 on the moments);
  * closed streams stay frozen through later calls of every entry; the per-meter resets reopen nothing, mtr_engine_reset does;
  * the host form equals the device form bit for bit across three chunks;
  * beside EBU / TRUEPEAK the loudness results are bit for bit those of process_device_lengths, in both tail modes;
  * a batch of 256 streams x 10 s with uniform lengths against the restatement on sixteen sampled streams;
  * the meters that do not take track lengths, and argument errors, leave the engine unchanged.
"""
import ctypes as C

import numpy as np
import pytest

import _signals as sig
from test_gpu_dr14 import DR_TOL, programme, ref_dr14
from test_gpu_kmeter import Kmeter, signal

pytestmark = pytest.mark.gpu
FS = [48000.0, 44100.0]
F = C.c_float


@pytest.fixture(scope="module")
def M():
    import meters.lv2_amd as m
    return m


def _window(fs):
    return int(np.rint(np.float32(fs) * np.float32(3.0))) + 1           # dr14.c:155, :404


def _frames_per_call(L, calls):
    """frames of every call for a stream of total length L (0 once it has closed)"""
    out, p, done = [], 0, False
    for c in calls:
        f = 0 if done else int(min(max(L - p, 0), c))
        done = done or f < c
        out.append(f)
        p += c
    return out


def _closed_after(L, calls):
    """closure of a stream of total length L after each call"""
    out, done = [], False
    for f, c in zip(_frames_per_call(L, calls), calls):
        done = done or f < c
        out.append(done)
    return out


def _snap(M, e):
    """every getter of the engine's meters, then each stream's part of the state blob (kmeter_read arms the new-maximum flag: the blob
    is taken behind it, so that two snapshots of an untouched stream are the same bytes).  The blob's header holds the engine's
    lock-step cursors, which move on past a closed stream: _header () has it for the comparisons between two engines."""
    m, out = e.meters, {}
    if m & (M.METER_EBU | M.METER_TRUEPEAK):
        hm, hs = e.histograms()
        r = e.results()
        out.update(out9=e.out9(), hm=hm, hs=hs,
                   tp=np.array([[x.truepeak[0], x.truepeak[1], x.truepeak_call[0], x.truepeak_call[1]] for x in r], np.float32))
    if m & M.METER_DR14:
        out["dr14"] = np.frombuffer(bytes(e.dr14()), np.uint8).reshape(e.n_streams, -1).copy()
    if m & M.METER_KMETER:
        out["km_rms"], out["km_peak"] = e.kmeter_read()
    if m & M.METER_BITSTATS:
        out.update({"bim_" + k: v for k, v in e.bitstats().items()})
    if m & M.METER_SIGDIST:
        out.update({"sdh_" + k: v for k, v in e.sigdist().items()})
    hdr = 2 * e.state_bytes(1) - e.state_bytes(2)
    out["blob"] = np.stack([np.frombuffer(e.state_export(s, 1), np.uint8)[hdr:] for s in range(e.n_streams)])
    return out


def _header(e):
    return e.state_export(0, 1)[:2 * e.state_bytes(1) - e.state_bytes(2)]


def _rows(s, idx):
    return {k: np.ascontiguousarray(v[idx]) for k, v in s.items()}


def _same(a, b, what=""):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)), (what, k)


def _engine(M, S, fs, meters, chn):
    e = M.Engine(S, fs, meters, n_channels=chn)
    if meters & M.METER_EBU:
        e.integr_start()
    return e


def _run(e, dev, calls, Ls=None, entry="tracks"):
    """the calls over the device buffer dev [S, stride, C]: dense (Ls None) or with the per-call frames of total lengths Ls"""
    stride, chn = dev.shape[1], dev.shape[2]
    pos = 0
    for i, n in enumerate(calls):
        ptr = dev.data_ptr() + pos * chn * 4
        if Ls is None:
            e.process_device(ptr, n, stride=stride)
        else:
            f = np.array([_frames_per_call(L, calls)[i] for L in Ls], np.uint64)
            getattr(e, "process_device_" + entry)(ptr, n, f, stride=stride)
        pos += n


def _audio(S, T, stride, chn, seed, fs):
    """[S, stride, chn]: stereo programmes of tests/test_gpu_dr14.py (or their left channels), zero behind T"""
    x = np.zeros((S, stride, chn), np.float32)
    for s in range(S):
        x[s, :T] = programme(T, seed + s, fs)[:, :chn]
    return x


def _mono(S, T, seed):
    """mono streams for BITSTATS / SIGDIST: audio, audio beyond the SDH's 361 bins (|x| > 1.2: skipped samples, from the first
    frames on, so that the index among ALL samples matters), bit-pattern soup (NaN / Inf / denormals / every exponent)"""
    x = np.zeros((S, T), np.float32)
    for s in range(S):
        if s % 3 == 0:
            x[s] = sig.lcg_noise(T, seed + s, 0.5)[:, 0]
        elif s % 3 == 1:
            x[s] = sig.lcg_noise(T, seed + s, 1.0)[:, 0] * np.float32(1.5) + np.float32(0.125)
        else:
            x[s] = sig.g5(T, seed + s)
    return x


GARBAGE = [np.float32(np.nan), np.float32(np.inf), np.float32(1e30), np.float32(1e-40)]


def _meter_sets(M):
    return {"DR14": (M.METER_DR14, 2), "KMETER": (M.METER_KMETER, 2), "DR14_mono": (M.METER_DR14, 1), "KMETER_mono": (M.METER_KMETER, 1),
            "BITSTATS": (M.METER_BITSTATS, 1), "SIGDIST": (M.METER_SIGDIST, 1), "BITSTATS|SIGDIST": (M.METER_BITSTATS | M.METER_SIGDIST, 1),
            "EBU|TP|DR14|KMETER": (M.METER_EBU | M.METER_TRUEPEAK | M.METER_DR14 | M.METER_KMETER, 2)}


def _three_calls(fs):
    """three calls of different lengths (Kmeterdsp's fall-back factor changes) that hold more than three DR-14 windows"""
    W = _window(fs)
    return [W + 1001, W // 2 + 6, 2 * W - W // 2 + 2003]


# ---- 1. identity -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fs", FS)
@pytest.mark.parametrize("name", ["DR14", "KMETER", "DR14_mono", "KMETER_mono", "BITSTATS", "SIGDIST", "BITSTATS|SIGDIST", "EBU|TP|DR14|KMETER"])
def test_identity_full_lengths_and_open_streams(M, name, fs):
    import torch
    meters, chn = _meter_sets(M)[name]
    calls = _three_calls(fs)
    T, S = sum(calls), 6
    x = _audio(S, T, T + 1, chn, 500, fs) if name not in ("BITSTATS", "SIGDIST", "BITSTATS|SIGDIST") else _mono(S, T + 1, 500)[:, :, None]
    dev = torch.from_numpy(x).cuda()
    with _engine(M, S, fs, meters, chn) as dense, _engine(M, S, fs, meters, chn) as full, _engine(M, S, fs, meters, chn) as ragged:
        _run(dense, dev, calls)
        _run(full, dev, calls, [T] * S)
        want = _snap(M, dense)
        _same(want, _snap(M, full), "lengths all n_frames")
        assert _header(dense) == _header(full)
        f, c = full.stream_frames()
        assert (f == T).all() and not c.any()
        # streams 1, 3, 4 end somewhere in the first, second and third call; 0, 2, 5 stay open
        Ls = [T, calls[0] - 77, T, calls[0] + 1234, T - 1, T]
        _run(ragged, dev, calls, Ls)
        _same(_rows(want, [0, 2, 5]), _rows(_snap(M, ragged), [0, 2, 5]), "open streams of a ragged batch")
        assert _header(dense) == _header(ragged)
        f, c = ragged.stream_frames()
        assert f.tolist() == Ls and c.tolist() == [False, True, False, True, True, False]


# ---- 2. past the end ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fs", FS)
@pytest.mark.parametrize("name", ["DR14", "KMETER", "BITSTATS|SIGDIST", "EBU|TP|DR14|KMETER"])
def test_garbage_past_the_end_changes_nothing(M, name, fs):
    import torch
    meters, chn = _meter_sets(M)[name]
    calls = _three_calls(fs)
    T, S = sum(calls), 9
    clean = _audio(S, T, T, chn, 520, fs) if name != "BITSTATS|SIGDIST" else _mono(S, T, 520)[:, :, None]
    Ls = [0, 1, 5, calls[0] - 1030, calls[0], calls[0] + 3, calls[0] + calls[1] + 1026, T - 1, T]
    dirty = clean.copy()
    for s, L in enumerate(Ls):
        clean[s, L:] = 0
        dirty[s, L:] = GARBAGE[s % 4]
        dirty[s, L + 1::2] = GARBAGE[(s + 1) % 4]
    dc, dd = torch.from_numpy(clean).cuda(), torch.from_numpy(dirty).cuda()
    with _engine(M, S, fs, meters, chn) as a, _engine(M, S, fs, meters, chn) as b:
        _run(a, dc, calls, Ls)
        _run(b, dd, calls, Ls)
        sa, sb = _snap(M, a), _snap(M, b)
        if meters & M.METER_TRUEPEAK:
            # (the blob of a stream that CLOSES holds, by the _lengths contract, the 47 frames of the buffer in front of the call's end as
            # its interpolator history — k_history under HIST_CALL_END_IF_TOUCHED: "a stream that closes keeps whatever follows its end in
            # the buffer: nothing reads it again" — so beside EBU / TRUEPEAK the blobs of the open streams are compared, and every getter of every stream)
            opened = [s for s, L in enumerate(Ls) if L == T]
            sa["blob"], sb["blob"] = sa["blob"][opened], sb["blob"][opened]
        _same(sa, sb, "garbage behind the ends")
        assert _header(a) == _header(b)
        if meters & M.METER_BITSTATS:
            # (the sharp end: not one NaN / Inf / denormal of the padding was counted — the audio streams hold none of their own)
            audio = [s for s in range(S) if s % 3 != 2]
            assert not sb["bim_counters"][audio][:, 2:].any()


# ---- 3. closed streams against the restatement ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("fs", FS)
@pytest.mark.parametrize("chn,odd_stride", [(2, 0), (2, 1), (1, 1)])
def test_dr14_closed_streams_match_the_restatement(M, oracle, fs, chn, odd_stride):
    import torch
    W = _window(fs)
    calls = [W + 1000, W + 1001, W + 3000]                           # the streams end in the first, the second, the third, or never
    T = sum(calls)
    Ls = [0, 1, 2, W - 1, W, W + 1, calls[0], 2 * W, calls[0] + calls[1], 3 * W - 1, 3 * W, 3 * W + 1,
          W + 500, W + 501, 2 * W + 2500, 2 * W + 2501, T - 1, T]
    S = len(Ls)
    stride = T + ((T + odd_stride) & 1)                                # an even / odd stream_stride_frames (the 16-byte path's parity)
    assert stride % 2 == odd_stride
    x = _audio(S, T, stride, chn, 40, fs)
    x[:, T:] = np.float32(np.nan)
    for s, L in enumerate(Ls):
        x[s, L:T] = GARBAGE[s % 4]                                     # (never metered)
    dev = torch.from_numpy(x).cuda()
    with M.Engine(S, fs, M.METER_DR14, n_channels=chn) as e:
        _run(e, dev, calls, Ls)
        got = e.dr14()
        f, c = e.stream_frames()
    assert f.tolist() == Ls and c.tolist() == [L < T for L in Ls]
    scored = 0
    for s, L in enumerate(Ls):
        if L == 0:                                                     # untouched: as dr14_reset leaves it
            assert got[s].block_count == 0 and got[s].m_rms[0] == -81 and got[s].dr[0] == 21
            continue
        want = ref_dr14(oracle, x[s, :L], fs, chn, _frames_per_call(L, calls))
        print("dr14", fs, chn, odd_stride, L, got[s].block_count, want.block_count, [got[s].m_rms[k] - want.m_rms[k] for k in range(chn)])
        assert got[s].block_count == want.block_count, (s, L, got[s].block_count, want.block_count)
        scored += want.block_count > 3 * 2
        for k in range(chn):
            assert abs(got[s].m_rms[k] - want.m_rms[k]) <= DR_TOL, (s, L, k, got[s].m_rms[k], want.m_rms[k])
            assert abs(got[s].dr[k] - want.dr[k]) <= DR_TOL, (s, L, k, got[s].dr[k], want.dr[k])
        if chn == 2:
            assert abs(got[s].dr_total - want.dr_total) <= DR_TOL, (s, L)
    assert scored >= 3                                                 # (more than two windows: the score exists)


@pytest.mark.parametrize("fs", FS)
@pytest.mark.parametrize("chn,extra", [(2, 0), (2, 1), (1, 0), (1, 1)])
def test_kmeter_closed_streams_match_the_restatement(M, oracle, fs, chn, extra):
    import torch
    lib = oracle.lib
    lib.mo_kmeter_init.argtypes = [C.POINTER(Kmeter), F]
    lib.mo_kmeter_process.argtypes = [C.POINTER(Kmeter), C.POINTER(F), C.c_int]
    lib.mo_kmeter_read.argtypes = [C.POINTER(Kmeter), C.POINTER(F), C.POINTER(F)]
    G = 131072                                                         # a workgroup's 32768 groups of four frames
    # (the second call is shorter than the first, the third longer: the fall-back factor changes; the third starts on an odd frame)
    calls = [G + 1000, 5001, G + 1003]
    c0, c01, T = calls[0], calls[0] + calls[1], sum(calls)
    Ls = [0, 1, 3, 4, 5, 7, 8, G - 4, G - 1, G, G + 1, G + 4, c0,
          c0 + 1, c0 + 3, c0 + 4, c0 + 2501, c01,
          c01 + 1, c01 + 7, c01 + G - 4, c01 + G - 1, c01 + G, c01 + G + 1, c01 + G + 4, T - 1, T]
    S = len(Ls)
    assert T % 4 == 0
    stride = T + extra                                                 # keeps / breaks the 16-byte alignment of the streams
    x = np.zeros((S, stride, chn), np.float32)
    for s in range(S):
        x[s, :T] = signal(T, 300 + s, fs)[:, :chn]
        x[s, Ls[s]:] = GARBAGE[s % 4]
    dev = torch.from_numpy(x).cuda()
    ks = [[Kmeter() for _ in range(chn)] for _ in range(S)]
    for s in range(S):
        for c in range(chn):
            lib.mo_kmeter_init(C.byref(ks[s][c]), fs)
    with M.Engine(S, fs, M.METER_KMETER, n_channels=chn) as e:
        pos = 0
        for i, n in enumerate(calls):
            fr = [_frames_per_call(L, calls)[i] for L in Ls]
            e.process_device_tracks(dev.data_ptr() + pos * chn * 4, n, np.array(fr, np.uint64), stride=stride)
            rms, peak = e.kmeter_read()                                # read after every call
            for s in range(S):
                for c in range(chn):
                    if fr[s]:                                          # (a host that stops calling run () at the track's end)
                        ch = np.ascontiguousarray(x[s, pos:pos + fr[s], c])
                        lib.mo_kmeter_process(C.byref(ks[s][c]), ch.ctypes.data_as(C.POINTER(F)), fr[s])
                    a, b = F(), F()
                    lib.mo_kmeter_read(C.byref(ks[s][c]), C.byref(a), C.byref(b))
                    assert abs(rms[s, c] - a.value) <= 1e-5 * max(a.value, 1e-3), (i, s, Ls[s], c, rms[s, c], a.value)
                    assert peak[s, c] == np.float32(b.value), (i, s, Ls[s], c, peak[s, c], b.value)
            pos += n
            f, cl = e.stream_frames()
            assert cl.tolist() == [_closed_after(L, calls)[i] for L in Ls]
        assert f.tolist() == Ls


@pytest.mark.parametrize("fs", FS)
@pytest.mark.parametrize("extra", [0, 1])
def test_bitstats_sigdist_closed_streams_match_the_restatement(M, oracle, fs, extra):
    import torch
    ends = [1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025]
    calls = [1500, 1301, 2000]
    c0, c01, T = calls[0], calls[0] + calls[1], sum(calls)
    Ls = [0] + ends + [c0] + [c0 + v for v in ends] + [c01] + [c01 + v for v in ends] + [T - 1, T]
    S = len(Ls)
    stride = T + 3 + extra                                             # 4804 / 4805: streams on and off 16 bytes
    x = _mono(S, stride, 900)
    for s, L in enumerate(Ls):
        x[s, L:] = GARBAGE[s % 4]
    dev = torch.from_numpy(x[:, :, None]).cuda()
    with M.Engine(S, fs, M.METER_BITSTATS | M.METER_SIGDIST, n_channels=1) as e:
        _run(e, dev, calls, Ls)
        b, d = e.bitstats(), e.sigdist()
        f, c = e.stream_frames()
    assert f.tolist() == Ls and c.tolist() == [L < T for L in Ls]
    quirk = 0
    for s, L in enumerate(Ls):
        wb, wd = oracle.bitstats(x[s, :L]), oracle.sigdist(x[s, :L])
        assert np.array_equal(b["hist"][s], wb["hist"]), (s, L, np.flatnonzero(b["hist"][s] != wb["hist"])[:10])
        assert np.array_equal(b["counters"][s], wb["counters"]), (s, L, b["counters"][s], wb["counters"])
        assert b["vmin"][s] == wb["vmin"] and b["vmax"][s] == wb["vmax"], (s, L)
        assert np.array_equal(d["bins"][s], wd["bins"]), (s, L)
        assert d["peak_cnt"][s] == wd["peak_cnt"] and d["peak_bin"][s] == wd["peak_bin"], (s, L)
        assert d["count"][s] == wd["count"] == L, (s, L)
        assert abs(d["avg"][s] - wd["avg"]) <= 1e-12 * max(1.0, abs(wd["avg"])) * max(L, 1), (s, L)
        assert abs(d["var_m"][s] - wd["var_m"]) <= 1e-12 * max(1.0, abs(wd["var_m"])), (s, L, d["var_m"][s], wd["var_m"])
        assert abs(d["var_s"][s] - wd["var_s"]) <= 1e-12 * max(1.0, abs(wd["var_s"])) * 10, (s, L, d["var_s"][s], wd["var_s"])
        quirk += wd["bins"].sum() < L
    assert quirk >= S // 2                                             # (samples outside the 361 bins: the divisor is the index among all samples)


# ---- 4. frozen and reopened ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fs", FS)
@pytest.mark.parametrize("name", ["EBU|TP|DR14|KMETER", "BITSTATS|SIGDIST"])
def test_closed_streams_stay_frozen_until_reset(M, name, fs):
    import torch
    meters, chn = _meter_sets(M)[name]
    W = _window(fs)
    n0, n1 = W + 2000, 6000
    S = 6
    x = _audio(S, n0 + n1, n0 + n1, chn, 700, fs) if chn == 2 else _mono(S, n0 + n1, 700)[:, :, None]
    dev = torch.from_numpy(x).cuda()
    closing = np.array([n0, 0, 5, n0, W + 1, n0 - 1], np.uint64)
    shut = [1, 2, 4, 5]
    with _engine(M, S, fs, meters, chn) as e:
        e.process_device_tracks(dev.data_ptr(), n0, closing, stride=n0 + n1)
        frozen = _rows(_snap(M, e), shut)
        f, c = e.stream_frames()
        assert f.tolist() == closing.tolist() and c.tolist() == [False, True, True, False, True, True]
        blk = dev.data_ptr() + n0 * chn * 4
        e.process_device(blk, n1, stride=n0 + n1)
        _same(frozen, _rows(_snap(M, e), shut), "after process_device")
        e.process(np.ascontiguousarray(x[:, n0:]) if chn == 2 else np.ascontiguousarray(x[:, n0:, 0]))
        _same(frozen, _rows(_snap(M, e), shut), "after process (host)")
        e.process_device_tracks(blk, n1, np.array([n1, n1, 17, n1 - 1, 0, n1], np.uint64), stride=n0 + n1)
        _same(frozen, _rows(_snap(M, e), shut), "after _tracks")
        f, c = e.stream_frames()
        assert f.tolist() == [n0 + 3 * n1, 0, 5, n0 + 3 * n1 - 1, W + 1, n0 - 1] and c.tolist() == [False, True, True, True, True, True]
        # the per-meter resets clear the meters' states and reopen nothing
        if meters & M.METER_DR14:
            e.dr14_reset()
            e.kmeter_reset()
        else:
            e.intstat_reset()
        cleared = _rows(_snap(M, e), shut)
        e.process_device(blk, n1, stride=n0 + n1)
        _same(cleared, _rows(_snap(M, e), shut), "after a per-meter reset")
        assert e.stream_frames()[1].tolist() == [False, True, True, True, True, True]
        # mtr_engine_reset reopens every stream: the engine is a fresh one's
        e.reset()
        f, c = e.stream_frames()
        assert not f.any() and not c.any()
        if meters & M.METER_EBU:
            e.integr_start()
        e.process_device(dev.data_ptr(), n0, stride=n0 + n1)
        with _engine(M, S, fs, meters, chn) as fresh:
            fresh.process_device(dev.data_ptr(), n0, stride=n0 + n1)
            _same(_snap(M, fresh), _snap(M, e), "after mtr_engine_reset")
            assert _header(fresh) == _header(e)


# ---- 5. host form equals device form ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fs", FS)
@pytest.mark.parametrize("name", ["EBU|TP|DR14|KMETER", "BITSTATS|SIGDIST"])
def test_host_form_equals_device_form(M, name, fs):
    import torch
    meters, chn = _meter_sets(M)[name]
    W = _window(fs)
    calls = [(W + 2000) // 4 * 4, 6000]
    T, S = sum(calls), 7
    x = _audio(S, T, T, chn, 800, fs) if chn == 2 else _mono(S, T, 800)[:, :, None]
    Ls = [T, 0, 3, W + 1, calls[0], calls[0] + 2049, T - 1]
    dev = torch.from_numpy(x).cuda()
    with _engine(M, S, fs, meters, chn) as d, _engine(M, S, fs, meters, chn) as h:
        h.set_host_chunk_bytes(3 * calls[0] * chn * 4)                 # three streams per chunk: three chunks
        _run(d, dev, calls, Ls)
        pos = 0
        for i, n in enumerate(calls):
            blk = np.ascontiguousarray(x[:, pos:pos + n] if chn == 2 else x[:, pos:pos + n, 0])
            h.process_tracks(blk, np.array([_frames_per_call(L, calls)[i] for L in Ls], np.uint64))
            pos += n
        _same(_snap(M, d), _snap(M, h), "host form")
        assert _header(d) == _header(h)
        assert d.stream_frames()[0].tolist() == h.stream_frames()[0].tolist() == Ls


# ---- 6. beside EBU ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fs", FS)
@pytest.mark.parametrize("tail", [1, 2])
def test_ebu_results_beside_the_track_meters_equal_lengths(M, fs, tail):
    import torch
    fr = int(fs) // 20
    calls = [1000, 9 * fr + 300 - 1000, 2000]
    T, S = sum(calls), 8
    x = _audio(S, T, T, 2, 860, fs)
    Ls = [T, 0, 24, fr + 1, calls[0], calls[0] + 4 * fr - 24, calls[0] + calls[1] + 1500, T - 1]
    dev = torch.from_numpy(x).cuda()
    ebu = M.METER_EBU | M.METER_TRUEPEAK
    with _engine(M, S, fs, ebu | M.METER_DR14 | M.METER_KMETER, 2) as a, _engine(M, S, fs, ebu, 2) as b:
        for e in (a, b):
            e.set_deferred_tail(tail)
        _run(a, dev, calls, Ls, "tracks")
        _run(b, dev, calls, Ls, "lengths")
        sa, sb = _snap(M, a), _snap(M, b)
        _same({k: sa[k] for k in ("out9", "hm", "hs", "tp")}, {k: sb[k] for k in ("out9", "hm", "hs", "tp")}, "EBU / true peak beside DR14 | KMETER")
        # an EBU / TRUEPEAK-only engine: _tracks is _lengths
        with _engine(M, S, fs, ebu, 2) as c:
            c.set_deferred_tail(tail)
            _run(c, dev, calls, Ls, "tracks")
            _same(sb, _snap(M, c), "_tracks on an EBU / TRUEPEAK engine")


# ---- 7. one batch-sized case ----------------------------------------------------------------------------------------------------------

def test_batch_of_tracks_uniform_lengths(M, oracle):
    import torch
    lib = oracle.lib
    lib.mo_kmeter_init.argtypes = [C.POINTER(Kmeter), F]
    lib.mo_kmeter_process.argtypes = [C.POINTER(Kmeter), C.POINTER(F), C.c_int]
    lib.mo_kmeter_read.argtypes = [C.POINTER(Kmeter), C.POINTER(F), C.POINTER(F)]
    fs, S, T = 48000.0, 256, 480000
    buf = torch.empty((S, T, 2), dtype=torch.float32, device="cuda")
    M.synth_fill_device(buf.data_ptr(), S, T, T, 4711, fs, 1)
    rng = np.random.default_rng(19)
    L = rng.integers(0, T + 1, S).astype(np.uint64)
    L2 = rng.integers(0, 2 * T + 1, S).astype(np.uint64)               # the same buffer as 256 mono streams of 2 T samples
    with M.Engine(S, fs, M.METER_DR14 | M.METER_KMETER) as e:
        e.process_device_tracks(buf.data_ptr(), T, L)
        dr, (rms, peak) = e.dr14(), e.kmeter_read()
        assert e.stream_frames()[0].tolist() == L.tolist()
    with M.Engine(S, fs, M.METER_BITSTATS | M.METER_SIGDIST, n_channels=1) as e:
        e.process_device_tracks(buf.data_ptr(), 2 * T, L2)
        b, d = e.bitstats(), e.sigdist()
    for s in sorted(set(rng.integers(0, S, 24).tolist()))[:16]:
        n = int(L[s])
        x = buf[s, :n].cpu().numpy()
        if n:
            want = ref_dr14(oracle, x, fs, 2, [n])
            assert dr[s].block_count == want.block_count, (s, n)
            for c in range(2):
                assert abs(dr[s].m_rms[c] - want.m_rms[c]) <= DR_TOL and abs(dr[s].dr[c] - want.dr[c]) <= DR_TOL, (s, n, c)
            assert abs(dr[s].dr_total - want.dr_total) <= DR_TOL, (s, n)
        for c in range(2):
            k, a, p = Kmeter(), F(), F()
            lib.mo_kmeter_init(C.byref(k), fs)
            if n:
                ch = np.ascontiguousarray(x[:, c])
                lib.mo_kmeter_process(C.byref(k), ch.ctypes.data_as(C.POINTER(F)), n)
            lib.mo_kmeter_read(C.byref(k), C.byref(a), C.byref(p))
            assert abs(rms[s, c] - a.value) <= 1e-5 * max(a.value, 1e-3), (s, n, c, rms[s, c], a.value)
            assert peak[s, c] == np.float32(p.value), (s, n, c)
        m = buf[s].reshape(-1)[:int(L2[s])].cpu().numpy()
        wb, wd = oracle.bitstats(m), oracle.sigdist(m)
        assert np.array_equal(b["hist"][s], wb["hist"]) and np.array_equal(b["counters"][s], wb["counters"]), (s, m.size)
        assert np.array_equal(d["bins"][s], wd["bins"]) and d["peak_bin"][s] == wd["peak_bin"] and d["count"][s] == m.size, (s, m.size)
        assert abs(d["var_m"][s] - wd["var_m"]) <= 1e-12 * max(1.0, abs(wd["var_m"])), (s, m.size)
        assert abs(d["var_s"][s] - wd["var_s"]) <= 1e-12 * max(1.0, abs(wd["var_s"])) * 10, (s, m.size)


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_engine_unchanged(M):
    import torch
    fs, S, T = 48000.0, 2, 6000
    ok = np.array([3000, 10], np.uint64)
    for meters, ch in [(M.METER_SPECTR30, 2), (M.METER_TPBALLIST, 2), (M.METER_STCORR, 2), (M.METER_NEEDLE, 2), (M.METER_SURROUND, 5),
                       (M.METER_DR14 | M.METER_TPBALLIST, 2), (M.METER_EBU | M.METER_SPECTR30, 2), (M.METER_KMETER | M.METER_STCORR, 2)]:
        x = (np.random.default_rng(ch).standard_normal((S, T, ch)) * 0.2).astype(np.float32)
        dev = torch.from_numpy(x).cuda()
        with M.Engine(S, fs, meters, n_channels=ch) as e:
            e.process_device(dev.data_ptr(), 2000, stride=T)
            before = np.frombuffer(e.state_export(), np.uint8).copy()
            res = bytes(e.results())
            assert M.lib.mtr_engine_process_device_tracks(e._h, dev.data_ptr(), 3000, T, ok.ctypes.data, None) == M.engine.ERR_UNSUPPORTED, meters
            assert M.lib.mtr_engine_process_host_tracks(e._h, x.ctypes.data, 3000, T, ok.ctypes.data) == M.engine.ERR_UNSUPPORTED, meters
            assert np.array_equal(before, np.frombuffer(e.state_export(), np.uint8)) and res == bytes(e.results()), meters
            f, c = e.stream_frames()
            assert (f == 2000).all() and not c.any()
    x = _audio(S, T, T, 2, 990, fs)
    dev = torch.from_numpy(x).cuda()
    with M.Engine(S, fs, M.METER_DR14 | M.METER_KMETER) as e:
        e.process_device(dev.data_ptr(), 2000, stride=T)
        before = _snap(M, e)
        bad = np.array([3000, 3001], np.uint64)
        assert M.lib.mtr_engine_process_device_tracks(e._h, dev.data_ptr(), 3000, T, None, None) == M.engine.ERR_ARG
        assert M.lib.mtr_engine_process_host_tracks(e._h, x.ctypes.data, 3000, T, None) == M.engine.ERR_ARG
        assert M.lib.mtr_engine_process_device_tracks(e._h, dev.data_ptr(), 3000, T, bad.ctypes.data, None) == M.engine.ERR_ARG
        assert M.lib.mtr_engine_process_host_tracks(e._h, x.ctypes.data, 3000, T, bad.ctypes.data) == M.engine.ERR_ARG
        _same(before, _snap(M, e), "after argument errors")
        f, c = e.stream_frames()
        assert (f == 2000).all() and not c.any()
