"""Per-stream lengths: mtr_engine_process_device_lengths / _host_lengths on the GPU.

A stream advances by frames[s] <= n_frames frames of a call; frames[s] < n_frames closes it, and its results are the
reference's after exactly its own frames, frozen until reset.  Held here, on layouts 3 (k_fused2), 4 (k_kw), 6 (k_kwtp16), 7 (k_seg
forced onto a small batch with tune_segments) and 8 (k_kwmc, 5 channels), at 48 and 44.1 kHz:
  * identity: lengths all n_frames give bit for bit what process_device gives (results, histograms, peaks, state blob);
  * open streams of a ragged batch are bit for bit the same streams of a dense batch;
  * whatever lies past a stream's end (NaN, Inf, 1e30, denormals) changes nothing of any stream, bit for bit;
  * each closed stream against the oracle (tests/_mc.py: Ebu_r128_proc with C channels + one TruePeakdsp per channel) fed
    exactly its frames in the same call blocks, the last one truncated — results, histograms, the true-peak hold and the
    closing call's peak (truepeak_call) — at the tolerances of tests/test_gpu_parity.py;
  * closed streams stay frozen through later calls of every entry and both tail modes; reset reopens them;
  * the deferred tail (>= 4096 streams) and the multi-workgroup gate (> 4 x 1024 fragments) honour the lengths;
  * the full-size batch (8192 x 10 s, lengths uniform in [0, 10 s]) against the oracle on sampled streams;
  * argument errors and the meters / layouts that do not take lengths.
"""
import numpy as np
import pytest

from test_gpu_parity import CONTRACT_DB, DB_TOL, moved_allowed

pytestmark = pytest.mark.gpu

TP_RTOL = 2e-6
LAYOUTS = {   # name: (meters, engine knobs)
    "L3": ("EBU|TP", dict(tune_layout=3)),
    "L4": ("EBU", dict(tune_layout=4)),
    "L6": ("EBU|TP", dict(tune_layout=6)),
    "L7": ("EBU|TP", dict(tune_segments=2)),
    "L8": ("EBU|TP", dict(n_channels=5)),
}


def _ch(name):
    return LAYOUTS[name][1].get("n_channels", 2)
FS = [48000.0, 44100.0]


@pytest.fixture(scope="module")
def M():
    import meters.lv2_amd as m
    return m


@pytest.fixture(scope="module")
def oracle():
    from _oracle import Oracle
    return Oracle()


def _meters(M, name):
    return M.METER_EBU | (M.METER_TRUEPEAK if LAYOUTS[name][0] == "EBU|TP" else 0)


def _engine(M, name, S, fs):
    e = M.Engine(S, fs, _meters(M, name), **LAYOUTS[name][1])
    e.integr_start()
    return e


def _noise(S, T, seed, gain=0.3, C=2):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((S, T, C)) * gain).astype(np.float32)


def _snap(e, tp):
    hm, hs = e.histograms()
    r = e.results()
    out = dict(out9=e.out9(), hm=hm, hs=hs, blob=np.frombuffer(e.state_export(), np.uint8).copy(),
               tp=np.array([[x.truepeak[0], x.truepeak[1], x.truepeak_call[0], x.truepeak_call[1]] for x in r], np.float32))
    if tp:
        out["tpc"] = np.concatenate(e.truepeak_channels(), 1)
    return out


def _rows(s, idx):
    """the per-stream parts of a snapshot for the streams idx (the blob is left out)"""
    return {k: v[idx] for k, v in s.items() if k != "blob"}


def _same(a, b, what=""):
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (what, k)


def _calls(fs):
    """a call that ends inside a fragment, one that starts inside it (k_seg's head) and holds 8 whole fragments (two k_seg
    segments of four under tune_segments=2) and a tail, and one more"""
    fr = int(fs) // 20
    c0 = 1000
    head = fr - c0
    return [c0, head + 8 * fr + 300, 2000], fr


def _frames_per_call(L, calls):
    """frames of every call for a stream of total length L (0 once it has closed)"""
    out, p, done = [], 0, False
    for c in calls:
        f = 0 if done else int(min(max(L - p, 0), c))
        done = done or f < c
        out.append(f)
        p += c
    return out


def _lengths(fs):
    calls, fr = _calls(fs)
    c0, c1, c2 = calls
    head = fr - c0
    b0 = c0 + head                                  # first frame of the k_seg body (stream-absolute)
    seg1 = b0 + 4 * fr                              # its second segment
    ls = [0, 1, 23, 24, 25, 47, 48, fr - 1, fr, fr + 1, 2 * fr - 1, 2 * fr, 2 * fr + 1,
          c0, c0 + 700,                             # the whole first call; inside the head of the second
          b0 + 16, b0 + 17,                         # one step into the first k_seg segment
          seg1 - 25, seg1 - 24, seg1 - 23, seg1 - 1, seg1, seg1 + 1, seg1 + 16,
          b0 + 8 * fr - 1, c0 + c1 - 10, c0 + c1,   # the body's last frame, inside the tail, the whole second call
          c0 + c1 + 1500, c0 + c1 + c2]             # inside the third call, never closed
    return ls, calls


def _run_lengths(M, name, fs, x, ls, calls, entry="device"):
    import torch
    S = x.shape[0]
    dev = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    e = _engine(M, name, S, fs)
    per = np.array([_frames_per_call(L, calls) for L in ls], np.uint64)
    p = 0
    for k, c in enumerate(calls):
        if entry == "device":
            e.process_device_lengths(dev[:, p:].data_ptr(), c, per[:, k], stride=x.shape[1])
        else:
            e.process_lengths(x[:, p:p + c], per[:, k])
        p += c
    return e, per


@pytest.mark.parametrize("fs", FS)
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_identity_full_lengths(M, name, fs):
    import torch
    S, T = 6, 3 * 20000
    x = _noise(S, T, 11, C=_ch(name))
    dev = torch.from_numpy(x).cuda()
    tp = "TP" in LAYOUTS[name][0]
    snaps = []
    for ragged in (False, True):
        with _engine(M, name, S, fs) as e:
            for k in range(3):
                ptr = dev[:, 20000 * k:].data_ptr()
                if ragged:
                    e.process_device_lengths(ptr, 20000, np.full(S, 20000, np.uint64), stride=T)
                else:
                    e.process_device(ptr, 20000, stride=T)
            snaps.append(_snap(e, tp))
            if ragged:
                f, c = e.stream_frames()
                assert (f == T).all() and not c.any()
    _same(snaps[0], snaps[1], "identity")


@pytest.mark.parametrize("fs", FS)
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_open_streams_independent_and_garbage_past_the_end(M, name, fs):
    ls, calls = _lengths(fs)
    S, T = len(ls), sum(calls)
    x = _noise(S, T, 5, C=_ch(name))
    clean = x.copy()
    for s, L in enumerate(ls):
        clean[s, L:] = 0
    junk = clean.copy()
    fill = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 1e-42, -3e-40, 0.0], np.float32)
    for s, L in enumerate(ls):
        n = T - L
        junk[s, L:] = np.resize(fill, n * x.shape[2]).reshape(n, x.shape[2])
    tp = "TP" in LAYOUTS[name][0]
    e0, per = _run_lengths(M, name, fs, clean, ls, calls)
    a = _snap(e0, tp)
    f, c = e0.stream_frames()
    assert np.array_equal(f, np.array(ls, np.uint64)), (f, ls)
    assert np.array_equal(c, np.array([L < T for L in ls]))
    e0.close()
    e1, _ = _run_lengths(M, name, fs, junk, ls, calls)
    _same(_rows(a, slice(None)), _rows(_snap(e1, tp), slice(None)), "garbage past the end")
    e1.close()
    # the open stream (the last one) against the same stream of a dense batch
    with _engine(M, name, S, fs) as e:
        e.process(clean[:, :calls[0]]); e.process(clean[:, calls[0]:calls[0] + calls[1]]); e.process(clean[:, calls[0] + calls[1]:])
        d = _snap(e, tp)
    _same(_rows(a, [S - 1]), _rows(d, [S - 1]), "open stream vs dense batch")


def _oracle_stream(x, per, fs, tp):
    """the reference fed stream x in the engine's call blocks, each truncated to the stream's frames of that call: (out9, hist_M,
    hist_S, per-channel hold, per-channel peak of the last call that metered anything)"""
    import _mc
    m = _mc.McStream(x.shape[1], fs)
    m.start()
    p, last = 0, np.zeros(x.shape[1], np.float32)
    for f in per:
        f = int(f)
        if f:
            r = m.process(x[p:p + f], tp)
            if tp:
                last = r
        p += f
    out9, hm, hs, _ = m.get()
    return out9, hm, hs, m.hold.copy(), last


@pytest.mark.parametrize("fs", FS)
@pytest.mark.parametrize("name", list(LAYOUTS))
@pytest.mark.parametrize("entry", ["device", "host"])
def test_oracle_parity_per_stream(M, name, fs, entry):
    ls, calls = _lengths(fs)
    S, T, C = len(ls), sum(calls), _ch(name)
    x = _noise(S, T, 23, 0.5, C=C)
    tp_on = "TP" in LAYOUTS[name][0]
    e, per = _run_lengths(M, name, fs, x, ls, calls, entry)
    if name == "L7":
        assert e.seg_stats()[0] >= 1, "k_seg did not take the second call"
    out9 = e.out9()
    res = e.results()
    tp = np.array([[r.truepeak[0], r.truepeak[1]] for r in res], np.float32)
    tpc = np.array([[r.truepeak_call[0], r.truepeak_call[1]] for r in res], np.float32)
    hm, hs = e.histograms()
    if tp_on:
        ch_hold, ch_last = e.truepeak_channels()
    e.close()
    p = 0
    for s, L in enumerate(ls):
        if L == 0:                                  # closed without being touched: a fresh stream
            assert np.all(out9[s, [0, 1, 2, 3]] == -200.0) and np.all(tp[s] == 0) and np.all(tpc[s] == 0), s
            continue
        o9, ohm, ohs, hold, last = _oracle_stream(x[s], per[s], fs, tp_on)
        assert np.allclose(out9[s, :4], o9[:4], atol=DB_TOL), (s, L, out9[s], o9)
        assert hm[s].sum() == ohm.sum() and hs[s].sum() == ohs.sum(), (s, L)
        assert np.abs(hm[s] - ohm).sum() // 2 <= moved_allowed(0), (s, L)
        assert abs(out9[s, 4] - o9[4]) <= CONTRACT_DB and abs(out9[s, 5] - o9[5]) <= CONTRACT_DB, (s, L)
        assert abs(out9[s, 6] - o9[6]) <= 0.1001 and abs(out9[s, 7] - o9[7]) <= 0.1001, (s, L)
        if tp_on:
            want_hold = hold[:2] if C == 2 else np.full(2, hold.max(), np.float32)
            want_last = last[:2] if C == 2 else np.full(2, last.max(), np.float32)
            assert np.allclose(tp[s], want_hold, rtol=TP_RTOL, atol=0), (s, L, tp[s], want_hold)
            # the closing call's peak (or, closed with frames 0, the previous call's): TruePeakdsp::read () of that block
            assert np.allclose(tpc[s], want_last, rtol=TP_RTOL, atol=0), (s, L, tpc[s], want_last)
            assert np.allclose(ch_hold[s], hold, rtol=TP_RTOL, atol=0) and np.allclose(ch_last[s], last, rtol=TP_RTOL, atol=0), (s, L)


@pytest.mark.parametrize("fs", FS)
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_closed_streams_stay_frozen(M, name, fs):
    import torch
    ls, calls = _lengths(fs)
    S, T = len(ls), sum(calls)
    x = _noise(S, T, 29, C=_ch(name))
    tp = "TP" in LAYOUTS[name][0]
    e, _ = _run_lengths(M, name, fs, x, ls, calls)
    closed = [s for s, L in enumerate(ls) if L < T]
    a = _snap(e, tp)
    hdr = 2 * e.state_bytes(1) - e.state_bytes(2)               # (the blob's header holds the engine's cursors, which move on)
    blob_a = {s: e.state_export(s, 1)[hdr:] for s in closed}
    loud = _noise(S, 30000, 31, 3.0, C=_ch(name))
    dev = torch.from_numpy(loud).cuda()
    for mode in (1, 2):
        e.set_deferred_tail(mode)
        e.process_device(dev.data_ptr(), 12000, stride=30000)
        e.process(loud[:, 12000:20000])
        e.process_device_lengths(dev[:, 20000:].data_ptr(), 10000, np.full(S, 10000, np.uint64), stride=30000)
    b = _snap(e, tp)
    _same(_rows(a, closed), _rows(b, closed), "frozen")
    for s in closed:
        assert e.state_export(s, 1)[hdr:] == blob_a[s], s
    f, c = e.stream_frames()
    assert np.array_equal(c, np.array([L < T for L in ls]))
    assert f[-1] == T + 2 * 30000 and all(f[s] == ls[s] for s in closed)
    # reset reopens everything: the streams then behave as those of a fresh engine
    e.reset()
    e.integr_start()
    f, c = e.stream_frames()
    assert not f.any() and not c.any()
    e.process(x)
    r = _snap(e, tp)
    e.close()
    with _engine(M, name, S, fs) as g:
        g.process(x)
        _same(r, _snap(g, tp), "after reset")


@pytest.mark.timeout(900)
def test_deferred_tail_and_frag_path(M, oracle):
    import torch
    fs = 48000.0
    S, T = 4096, 48000
    buf = torch.empty((S, T, 2), dtype=torch.float32, device="cuda")
    M.synth_fill_device(buf.data_ptr(), S, T, T, 99, fs, 1)
    rng = np.random.default_rng(3)
    L = rng.integers(0, T + 1, S).astype(np.uint64)
    L[::7] = T
    res = []
    for mode in (1, 2):
        with M.Engine(S, fs, M.METER_EBU | M.METER_TRUEPEAK) as e:
            e.set_deferred_tail(mode)
            e.integr_start()
            for k in range(2):
                p = 24000 * k
                f = np.clip(L.astype(np.int64) - p, 0, 24000).astype(np.uint64)
                e.process_device_lengths(buf[:, p:].data_ptr(), 24000, f, stride=T)
            res.append(_snap(e, True))
            if mode == 2:
                assert e.deferred_calls() == 2
    _same(res[0], res[1], "tail modes 1 and 2")
    del buf
    # > 4 x 1024 fragments in one call: the multi-workgroup gate (k_gate_frag + k_gate_final) with per-stream limits
    fr = 2400
    T = 4200 * fr
    ls = [T, 4100 * fr + 1234, 3000 * fr + 5, 0]
    buf = torch.empty((len(ls), T, 2), dtype=torch.float32, device="cuda")
    M.synth_fill_device(buf.data_ptr(), len(ls), T, T, 7, fs, 1)
    with M.Engine(len(ls), fs, M.METER_EBU | M.METER_TRUEPEAK) as e:
        e.integr_start()
        e.process_device_lengths(buf.data_ptr(), T, np.array(ls, np.uint64))
        out9, tp = e.out9(), e.truepeak()
    for s, n in enumerate(ls[:3]):
        h = buf[s, :n].cpu().numpy()
        o = oracle.ebu(h, fs, 1 << 20)
        assert np.allclose(out9[s, :4], o["out9"][:4], atol=DB_TOL), (s, out9[s], o["out9"])
        assert abs(out9[s, 4] - o["out9"][4]) <= CONTRACT_DB
        assert np.allclose(tp[s], oracle.tp(h, fs, 1 << 20), rtol=TP_RTOL), s
    assert np.all(out9[3, :4] == -200.0)


@pytest.mark.timeout(1200)
def test_full_size_uniform_lengths(M, oracle):
    import torch
    fs = 48000.0
    S, T = 8192, 480000
    free, _ = torch.cuda.mem_get_info()
    if free < (S * T * 8) * 1.05:
        S = int(free * 0.9 / (T * 8)) // 256 * 256
    buf = torch.empty((S, T, 2), dtype=torch.float32, device="cuda")
    M.synth_fill_device(buf.data_ptr(), S, T, T, 777, fs, 1)
    rng = np.random.default_rng(8)
    L = rng.integers(0, T + 1, S).astype(np.uint64)
    with M.Engine(S, fs, M.METER_EBU | M.METER_TRUEPEAK) as e:
        assert e.layout() == 7
        e.integr_start()
        e.process_device_lengths(buf.data_ptr(), T, L)
        assert e.seg_stats()[0] == 1
        out9, tp = e.out9(), e.truepeak()
        hm, hs = e.histograms()
        dh = torch.zeros(2 * 751, dtype=torch.int32, device="cuda")
        dm = torch.zeros(4, dtype=torch.float32, device="cuda")
        e.aggregate_device(dh.data_ptr(), dm.data_ptr())
        torch.cuda.synchronize()
    h = dh.cpu().numpy().reshape(2, 751)
    assert np.array_equal(h[0], hm.sum(0)) and np.array_equal(h[1], hs.sum(0))
    for s in sorted(set(rng.integers(0, S, 64).tolist())):
        n = int(L[s])
        if n == 0:
            assert np.all(out9[s, :4] == -200.0) and np.all(tp[s] == 0)
            continue
        x = buf[s, :n].cpu().numpy()
        o = oracle.ebu(x, fs, 2400)
        assert np.allclose(out9[s, :4], o["out9"][:4], atol=DB_TOL), (s, n)
        assert abs(out9[s, 4] - o["out9"][4]) <= CONTRACT_DB, (s, n)
        assert np.allclose(tp[s], oracle.tp(x, fs, 8192), rtol=TP_RTOL), (s, n)


def test_errors_leave_the_engine_unchanged(M):
    import torch
    S, T = 4, 5000
    x = _noise(S, T, 3)
    dev = torch.from_numpy(x).cuda()
    with M.Engine(S, 48000.0, M.METER_EBU | M.METER_TRUEPEAK) as e:
        e.integr_start()
        e.process_device(dev.data_ptr(), 2000, stride=T)
        before = _snap(e, True)
        rc = M.lib.mtr_engine_process_device_lengths(e._h, dev.data_ptr(), 3000, T, None, None)
        assert rc == -1
        bad = np.array([3000, 3001, 0, 5], np.uint64)
        assert M.lib.mtr_engine_process_device_lengths(e._h, dev.data_ptr(), 3000, T, bad.ctypes.data, None) == -1
        assert M.lib.mtr_engine_process_host_lengths(e._h, x.ctypes.data, 3000, T, bad.ctypes.data) == -1
        _same(before, _snap(e, True), "after argument errors")
        f, c = e.stream_frames()
        assert (f == 2000).all() and not c.any()
    ok = np.zeros(1, np.uint64)
    for meters, ch, kw in [(M.METER_EBU | M.METER_SPECTR30, 2, {}), (M.METER_DR14, 2, {}), (M.METER_KMETER, 2, {}),
                           (M.METER_TPBALLIST, 2, {}), (M.METER_BITSTATS, 1, {}), (M.METER_SIGDIST, 1, {})]:
        with M.Engine(1, 48000.0, meters, n_channels=ch, **kw) as e:
            y = np.zeros((1, 100, ch), np.float32)
            assert M.lib.mtr_engine_process_host_lengths(e._h, y.ctypes.data, 100, 100, ok.ctypes.data) == -2, (meters, ch, kw)
