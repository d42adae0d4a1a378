"""Multichannel EBU R128 + per-channel true peak on the GPU (layout 8, mtr_kwmc.hip): n_channels 3, 4, 5 against the oracle
(mo_ebu with nchan channels, one TruePeakdsp per channel), golden_mc_v1 (the reference's own objects), the stereo engine
(identities across kernels), state round trips and the cross-stream aggregate.

Tolerances are test_gpu_parity's:
  * M, maxM, S, maxS, integrated, thresholds: 1e-3 dB;
  * histograms: counts identical, at most max (2, ceil (5e-4 x points)) points in a NEIGHBOURING 0.1 dB bin;
  * true peak: 2e-6 relative.
"""
import os

import numpy as np
import pytest

import _mc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "golden_mc_v1.npz"))

DB_TOL = 1e-3
TP_REL = 2e-6
MOVED_MAX, MOVED_RATE = 2, 5e-4


def moved_allowed(points):
    return max(MOVED_MAX, int(np.ceil(MOVED_RATE * points)))


def moved_points(got, want):
    got, want = np.asarray(got, np.int64), np.asarray(want, np.int64)
    assert got.sum() == want.sum(), (got.sum(), want.sum())
    d = got - want
    far = 0
    for row in d.reshape(-1, d.shape[-1]):
        c = 0
        for x in np.cumsum(row):
            c = c + 1 if x != 0 else 0
            far = max(far, c)
    return int(np.abs(d).sum() // 2), far


def check_hist(got, want):
    moved, far = moved_points(got, want)
    assert far <= 1 and moved <= moved_allowed(int(np.asarray(want).sum())), (moved, far)
    return moved


def check9(got9, want9):
    # the values that exist (-200 = "none yet" on both sides)
    assert np.allclose(got9[:6], want9[:6], atol=DB_TOL), (got9, want9)


@pytest.fixture(scope="module")
def M():
    import torch
    import meters.lv2_amd as m
    assert torch.cuda.is_available()
    return m


def run_engine(M, x, fs, meters, calls, integr=None, stride=None, **kw):
    """x: [S, T, C] float32 on the host -> results.  calls: frame counts of consecutive process calls (sum = T).
    integr: {call index: "start" | "pause" | "reset"}."""
    import torch
    S, T, Cn = x.shape
    dev = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    with M.Engine(S, fs, meters, n_channels=Cn, **kw) as e:
        if Cn != 2:
            assert M.lib.mtr_engine_layout(e._h) == 8
        o = 0
        for i, n in enumerate(calls):
            act = (integr or {}).get(i)
            if act:
                getattr(e, "integr_" + act)()
            e.process_device(dev.data_ptr() + o * Cn * 4, n, T)
            o += n
        torch.cuda.synchronize()
        r = dict(out9=e.out9(), hist=e.histograms())
        if meters & M.METER_TRUEPEAK:
            r["tp"] = e.truepeak()
            r["tp_hold"], r["tp_last"] = e.truepeak_channels()
        return r


def run_oracle(x, fs, calls, integr=None, with_tp=True):
    T, Cn = x.shape
    m = _mc.McStream(Cn, fs)
    o = 0
    for i, n in enumerate(calls):
        act = (integr or {}).get(i)
        if act:
            getattr(m, act)()
        m.process(x[o:o + n], with_tp)
        o += n
    out9, hm, hs, cnt = m.get()
    return dict(out9=out9, hm=hm, hs=hs, tp=m.hold)


def batch(S, T, Cn, seed):
    return np.stack([_mc.programme(T, Cn, seed + s) for s in range(S)])


def blocks(T, n):
    return [min(n, T - o) for o in range(0, T, n)]


@pytest.mark.parametrize("Cn", [3, 4, 5])
@pytest.mark.parametrize("fs", [44100.0, 48000.0])
def test_vs_oracle(M, Cn, fs):
    """64 streams x 30 s, three call shapes (1024-frame calls with integration start / pause / restart / reset, one whole-buffer
    call, a first call that ends mid-fragment); every 8th stream against the oracle, the call shapes against one another."""
    S, T = 64, int(30 * fs)
    x = batch(S, T, Cn, 100 * Cn + int(fs) % 11)
    meters = M.METER_EBU | M.METER_TRUEPEAK
    nb = len(blocks(T, 1024))
    integr = {20: "start", nb // 3: "pause", nb // 3 + 40: "start", nb // 2: "reset"}
    r = run_engine(M, x, fs, meters, blocks(T, 1024), integr)
    moved = 0
    for s in range(0, S, 8):
        o = run_oracle(x[s], fs, blocks(T, 1024), integr)
        check9(r["out9"][s], o["out9"])
        moved += check_hist(r["hist"][0][s], o["hm"]) + check_hist(r["hist"][1][s], o["hs"])
        assert np.allclose(r["tp_hold"][s], o["tp"], rtol=TP_REL, atol=0), (s, r["tp_hold"][s], o["tp"])
    # truepeak[0..1] = the max over the channels; the last call's peaks are the last block's
    assert np.array_equal(r["tp"][:, 0], r["tp_hold"].max(axis=1)) and np.array_equal(r["tp"][:, 1], r["tp_hold"].max(axis=1))
    assert np.all(r["tp_last"] <= r["tp_hold"])
    whole = run_engine(M, x, fs, meters, [T], {0: "start"})
    mid = run_engine(M, x, fs, meters, [1000, T - 1000], {0: "start"})
    for s in range(0, S, 16):
        o = run_oracle(x[s], fs, [T], {0: "start"})
        for g in (whole, mid):
            check9(g["out9"][s], o["out9"])
            check_hist(g["hist"][0][s], o["hm"]); check_hist(g["hist"][1][s], o["hs"])
            assert np.allclose(g["tp_hold"][s], o["tp"], rtol=TP_REL, atol=0)
    print(f"\nC={Cn} fs={fs}: {moved} histogram points in a neighbouring bin")


@pytest.mark.parametrize("case", [c for c in _mc.GOLDEN_CASES if c[0] >= 3], ids=lambda c: f"c{c[0]}_{int(c[1])}_{c[2]}")
def test_vs_golden_mc(M, case):
    n, fs, blk, sec, st = case
    T = int(sec * fs)
    x = _mc.programme(T, n, seed=n * 10 + int(fs) % 7 + blk % 3)[None]
    r = run_engine(M, x, fs, M.METER_EBU | M.METER_TRUEPEAK, blocks(T, blk), {st: "start"})
    k = f"c{n}_{int(fs)}_{blk}"
    check9(r["out9"][0], G[k + "_out9"])
    check_hist(r["hist"][0][0], G[k + "_hist_M"]); check_hist(r["hist"][1][0], G[k + "_hist_S"])
    assert np.allclose(r["tp_hold"][0], G[k + "_tp"], rtol=TP_REL, atol=0)


def test_identities_across_kernels(M):
    """5.0 with C / Ls / Rs silent = stereo on L / R; 3.0 with C silent = the same; Ls alone reads 10 log10 (1.41) above L alone."""
    fs, S, T = 48000.0, 8, 48000 * 12
    st = batch(S, T, 2, 7)
    meters = M.METER_EBU | M.METER_TRUEPEAK
    ref2 = run_engine(M, st, fs, meters, blocks(T, 4800), {0: "start"})
    five = np.zeros((S, T, 5), np.float32); five[..., :2] = st
    r5 = run_engine(M, five, fs, meters, blocks(T, 4800), {0: "start"})
    check9(r5["out9"][0], ref2["out9"][0])
    for s in range(S):
        check9(r5["out9"][s], ref2["out9"][s])
        check_hist(r5["hist"][0][s], ref2["hist"][0][s])
        assert np.allclose(r5["tp_hold"][s, :2], ref2["tp_hold"][s], rtol=TP_REL, atol=0)
        assert np.all(r5["tp_hold"][s, 2:] == 0)
    three = np.zeros((S, T, 3), np.float32); three[..., :2] = st
    r3 = run_engine(M, three, fs, meters, blocks(T, 4800), {0: "start"})
    for s in range(S):
        check9(r3["out9"][s], ref2["out9"][s])
        assert np.allclose(r3["tp_hold"][s, :2], ref2["tp_hold"][s], rtol=TP_REL, atol=0)
    l_only = np.zeros((S, T, 5), np.float32); l_only[..., 0] = st[..., 0]
    ls_only = np.zeros((S, T, 5), np.float32); ls_only[..., 3] = st[..., 0]
    a = run_engine(M, l_only, fs, M.METER_EBU, blocks(T, 4800), {0: "start"})
    b = run_engine(M, ls_only, fs, M.METER_EBU, blocks(T, 4800), {0: "start"})
    d = b["out9"][:, :4] - a["out9"][:, :4]
    assert np.allclose(d, 10 * np.log10(1.41), atol=2e-3), d


def test_full_size_5ch(M):
    """8192 streams x 10 s x 5 channels (the measured shape), 256 sampled streams against the oracle; the flip rate printed."""
    import torch
    S, fs = 8192, 48000.0
    T = int(10 * fs)
    dev = torch.empty((S, T, 5), dtype=torch.float32, device="cuda")
    # the device-side generator's stereo streams (T * 5 / 2 frames each) read as 5.0 frames, channels at differing levels
    M.synth_fill_device(dev.data_ptr(), S, T * 5 // 2, T * 5 // 2, 1234, fs, 1)
    dev *= torch.tensor([1.0, 0.8, 0.5, 0.3, 0.3], device="cuda")
    torch.cuda.synchronize()
    with M.Engine(S, fs, M.METER_EBU | M.METER_TRUEPEAK, n_channels=5) as e:
        e.integr_start()
        e.process_device(dev.data_ptr(), T)
        out9, (hm, hs) = e.out9(), e.histograms()
        hold, _ = e.truepeak_channels()
    moved = pts = 0
    for s in range(0, S, S // 256):
        x = dev[s].cpu().numpy()
        o = run_oracle(x, fs, [T], {0: "start"})
        check9(out9[s], o["out9"])
        moved += moved_points(hm[s], o["hm"])[0] + moved_points(hs[s], o["hs"])[0]
        pts += int(o["hm"].sum() + o["hs"].sum())
        assert np.allclose(hold[s], o["tp"], rtol=TP_REL, atol=0), s
    assert moved <= moved_allowed(pts), (moved, pts)
    print(f"\n8192 x 10 s x 5 ch: {moved} of {pts} histogram points in a neighbouring bin ({moved / max(pts, 1):.2e})")


def test_state_roundtrip_and_channel_mismatch(M):
    import ctypes as C
    import torch
    S, fs, T = 16, 48000.0, 48000 * 6
    x = batch(S, T, 5, 55)
    dev = torch.from_numpy(x).cuda()
    cuts = blocks(T, 7000)
    k = len(cuts) // 2
    meters = M.METER_EBU | M.METER_TRUEPEAK

    def feed(e, calls):
        o = sum(cuts[:calls[0]])
        for n in cuts[calls[0]:calls[1]]:
            e.process_device(dev.data_ptr() + o * 20, n, T)
            o += n

    with M.Engine(S, fs, meters, n_channels=5) as e:
        e.integr_start(); feed(e, (0, len(cuts)))
        want = (e.out9(), e.histograms(), e.truepeak_channels(), e.truepeak())
    with M.Engine(S, fs, meters, n_channels=5) as e:
        e.integr_start(); feed(e, (0, k))
        n = M.lib.mtr_engine_state_bytes(e._h, S)
        blob = (C.c_char * n)()
        assert M.lib.mtr_engine_state_export(e._h, 0, S, blob, n) == 0
    with M.Engine(S, fs, meters, n_channels=5) as f:
        assert M.lib.mtr_engine_state_import(f._h, 0, blob, n) == 0
        feed(f, (k, len(cuts)))
        got = (f.out9(), f.histograms(), f.truepeak_channels(), f.truepeak())
    assert np.array_equal(got[0], want[0])
    assert all(np.array_equal(a, b) for a, b in zip(got[1], want[1]))
    assert all(np.array_equal(a, b) for a, b in zip(got[2], want[2]))
    assert np.array_equal(got[3], want[3])
    for other in (2, 3):
        with M.Engine(S, fs, meters, n_channels=other) as g:
            assert M.lib.mtr_engine_state_import(g._h, 0, blob, n) == M.engine.ERR_STATE
    with M.Engine(S, fs, meters, n_channels=2) as g:
        n2 = M.lib.mtr_engine_state_bytes(g._h, S)
        b2 = (C.c_char * n2)()
        assert M.lib.mtr_engine_state_export(g._h, 0, S, b2, n2) == 0
    with M.Engine(S, fs, meters, n_channels=5) as h:
        assert M.lib.mtr_engine_state_import(h._h, 0, b2, n2) == M.engine.ERR_STATE


def test_aggregate_5ch(M):
    import torch
    S, fs, T = 32, 48000.0, 48000 * 8
    x = batch(S, T, 5, 77)
    dev = torch.from_numpy(x).cuda()
    with M.Engine(S, fs, M.METER_EBU | M.METER_TRUEPEAK, n_channels=5) as e:
        e.integr_start()
        e.process_device(dev.data_ptr(), T)
        hm, hs = e.histograms()
        hold, _ = e.truepeak_channels()
        dh = torch.zeros((2, 751), dtype=torch.int32, device="cuda")
        dm = torch.zeros(4, dtype=torch.float32, device="cuda")
        e.aggregate_device(dh.data_ptr(), dm.data_ptr())
        torch.cuda.synchronize()
    assert np.array_equal(dh[0].cpu().numpy(), hm.sum(axis=0)) and np.array_equal(dh[1].cpu().numpy(), hs.sum(axis=0))
    dmax = dm.cpu().numpy()
    assert dmax[0] == hold.max() and dmax[1] == hold.max(), (dmax, hold.max())


def test_nan_in_one_channel_scrubbed(M):
    """A NaN in Ls in one call: later calls stay finite (detect_process drops non-finite states, ebu_r128_proc.cc:331-334)."""
    S, fs, T = 4, 48000.0, 48000 * 6
    x = batch(S, T, 5, 91)
    x[:, 48000 + 17, 3] = np.nan
    calls = blocks(T, 4800)
    r = run_engine(M, x, fs, M.METER_EBU | M.METER_TRUEPEAK, calls, {0: "start"})
    assert np.all(np.isfinite(r["out9"][:, :6])), r["out9"]
    # the loudness after the NaN's block has left the 3 s window is the clean programme's
    clean = x.copy(); clean[:, 48000 + 17, 3] = 0.0
    c = run_engine(M, clean, fs, M.METER_EBU | M.METER_TRUEPEAK, calls, {0: "start"})
    assert np.allclose(r["out9"][:, 0], c["out9"][:, 0], atol=DB_TOL) and np.allclose(r["out9"][:, 2], c["out9"][:, 2], atol=DB_TOL)
    assert np.all(np.isfinite(r["tp_hold"][:, [0, 1, 2, 4]]))


def test_planar_and_host_paths(M):
    S, fs, T = 1, 44100.0, 44100 * 4
    x = batch(S, T, 3, 5)
    calls = blocks(T, 1024)
    want = run_engine(M, x, fs, M.METER_EBU | M.METER_TRUEPEAK, calls, {0: "start"})
    with M.Engine(1, fs, M.METER_EBU | M.METER_TRUEPEAK, n_channels=3) as e:
        e.integr_start()
        o = 0
        for n in calls:
            e.process_planar([x[0, o:o + n, c] for c in range(3)])
            o += n
        assert np.array_equal(e.out9(), want["out9"]) and np.array_equal(e.truepeak_channels()[0], want["tp_hold"])
    S = 6
    x = batch(S, T, 5, 9)
    want = run_engine(M, x, fs, M.METER_EBU | M.METER_TRUEPEAK, [T], {0: "start"})
    with M.Engine(S, fs, M.METER_EBU | M.METER_TRUEPEAK, n_channels=5) as e:
        e.integr_start()
        e.set_host_chunk_bytes(T * 5 * 4 * 2)                  # three chunks of two streams
        e.process(x)
        assert np.array_equal(e.out9(), want["out9"]) and np.array_equal(e.truepeak_channels()[0], want["tp_hold"])


def test_stereo_engine_truepeak_channels(M):
    S, fs, T = 4, 48000.0, 48000 * 2
    x = batch(S, T, 2, 3)
    r = run_engine(M, x, fs, M.METER_EBU | M.METER_TRUEPEAK, [T])
    assert np.array_equal(r["tp_hold"], r["tp"])
