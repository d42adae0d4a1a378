"""GPU parity: the HIP engine, driven through the C ABI (libmtr_engine.so), against the CPU oracle
and the committed golden vectors, on the same seeded inputs.

Tolerances (stated once, used everywhere below):
  * LUFS values (M, S, max, I, LRA edges, thresholds) and dBTP:  +-0.01 dB is the contract
    (BASELINE.json); the tests demand 1e-3 dB except where a value is quantised by the
    reference's 0.1 dB histogram (I, LRA): there a one-bin flip (a fragment loudness landing
    within float rounding of a bin edge) may move I by < 0.01 dB and an LRA edge by 0.1 dB.
  * fragment mean powers: 2e-5 relative (time-parallel summation order differs from the serial loop).
  * true peak: 2e-6 relative (FMA / accumulation order).
  * true-peak ballistics (TruePeakdsp::process: level m and raw peak p of every call): 4e-6 RELATIVE TO THE VALUE ITSELF
    (3.5e-5 dB), at any level — never "of max (1, value)".
  * band levels of the 30-band bank: 1e-3 dB above -90 dB.
  * integer histograms ("bit-exact target"): identical except for bin-edge flips — a fragment's loudness within
    ~1e-6 relative of a 0.1 dB edge: the kernels fuse the recurrence's multiply-adds and sum a fragment's power in another
    order than the serial loop, so its last bits differ and such a point lands in the neighbouring bin.  That is a RATE, and
    the bound scales with the count: at most max (2, ceil (5e-4 x points)) points of a histogram may sit
    in a NEIGHBOURING bin (never further), counts identical — moved_allowed () below; the rate actually measured is printed
    by the full-size tests (one stream x 3600 s: 36 000 + 7 200 points; 512 streams of the 8192 x 10 s batch: 51 200 +
    10 240 points) and recorded in DESIGN.md 4 — and the programme record of SUMMED histograms (mtr_hist_loudness, what
    mtr_engine_reduce feeds) must stay within 0.01 dB of the oracle's summed histograms.
"""
import os
import sys

import numpy as np
import pytest

import _signals as sig

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from make_golden import tri_noise  # noqa: E402

G = np.load(os.path.join(HERE, "golden", "golden_v1.npz"))

DB_TOL = 1e-3
CONTRACT_DB = 0.01
TPB_REL = 4e-6             # TruePeakdsp::process, level and peak of a call: relative to the value (jmeters/truepeakdsp.cc:58-84)
MOVED_MAX = 2              # histogram points in a neighbouring 0.1 dB bin for the fixture-sized checks (<= 4300 points: the rate bound's floor)
MOVED_RATE = 5e-4          # ... and per point for the big ones


def moved_allowed(points):
    return max(MOVED_MAX, int(np.ceil(MOVED_RATE * points)))


def moved_points(got, want):
    """(points that sit in another bin, the farthest any of them went in bins) between two histograms of equal count."""
    got, want = np.asarray(got, np.int64), np.asarray(want, np.int64)
    assert got.sum() == want.sum(), (got.sum(), want.sum())
    d = got - want
    moved = int(np.abs(d).sum() // 2)
    # a point that moved one bin leaves +1 / -1 in adjacent bins: the running sum of d never exceeds the moved count in
    # magnitude and returns to zero; its longest non-zero run is the farthest a point travelled
    far = 0
    for row in d.reshape(-1, d.shape[-1]):
        if not row.any():
            continue
        c = 0
        for x in np.cumsum(row):
            c = c + 1 if x != 0 else 0
            far = max(far, c)
    return moved, far


@pytest.fixture(scope="module")
def M():
    import meters.lv2_amd as m
    return m


def _db(x):
    return 20 * np.log10(np.maximum(np.asarray(x, np.float64), 1e-30))


def _check_ebu(got9, hist_got, want9, hist_want, cnt_want, frag_got=None, frag_want=None):
    # M, maxM, S, maxS: tight
    assert np.allclose(got9[:4], want9[:4], atol=DB_TOL), (got9, want9)
    # histogram: count identical, at most a couple of points moved to a neighbouring bin
    for h, w in zip(hist_got, hist_want):
        assert h.sum() == w.sum()
        moved = np.abs(h - w).sum() // 2
        assert moved <= MOVED_MAX, moved     # a fragment power within ~1e-6 of a 0.1 dB bin edge; measured over this file: 0 or 1
    # I, thresholds, LRA: the contract
    assert abs(got9[4] - want9[4]) <= CONTRACT_DB and abs(got9[5] - want9[5]) <= CONTRACT_DB
    # LRA edges are bin indices of the 0.1 dB S histogram: identical histogram -> identical edges, bit for bit;
    # a point that sits in the neighbouring bin can move an edge by that one bin
    if np.array_equal(hist_got[1], hist_want[1]):
        assert got9[6] == want9[6] and got9[7] == want9[7], (got9, want9)
    else:
        assert abs(got9[6] - want9[6]) <= 0.1001 and abs(got9[7] - want9[7]) <= 0.1001
    assert abs(got9[8] - want9[8]) <= CONTRACT_DB
    if frag_got is not None:
        assert frag_got.shape == frag_want.shape
        assert np.allclose(frag_got, frag_want, rtol=2e-5, atol=1e-30)


def _run_ebu_tp(M, x, fs=48000.0, calls=None, **kw):
    """x: [S, T, 2]. calls: list of frame counts to split the stream into process calls."""
    S, T = x.shape[0], x.shape[1]
    with M.Engine(S, fs, M.METER_EBU | M.METER_TRUEPEAK, **kw) as e:
        e.integr_start()
        pos = 0
        frags = []
        for n in (calls or [T]):
            e.process(x[:, pos:pos + n])
            frags.append(e.fragment_powers())
            pos += n
        assert pos == T
        hm, hs = e.histograms()
        return dict(out9=e.out9(), tp=e.truepeak(), hist_M=hm, hist_S=hs, frag=np.concatenate(frags, 1),
                    res=e.results())


@pytest.mark.parametrize("i", range(5))
def test_ebu_golden_cases(M, i):
    T, seed, gain, fs, block = G["ebu_cases"][i]
    x = tri_noise(int(T), int(seed), float(gain))
    r = _run_ebu_tp(M, x[None], float(fs))
    _check_ebu(r["out9"][0], (r["hist_M"][0], r["hist_S"][0]), G[f"ebu{i}_out9"],
               (G[f"ebu{i}_hist_M"], G[f"ebu{i}_hist_S"]), G[f"ebu{i}_counts"],
               r["frag"][0], G[f"ebu{i}_frag_power"])
    assert r["res"][0].hist_M_count == G[f"ebu{i}_counts"][0]
    assert r["res"][0].hist_S_count == G[f"ebu{i}_counts"][1]


def test_ebu_known_answers(M):
    r = _run_ebu_tp(M, sig.g0(48000 * 4)[None])
    assert abs(r["out9"][0, 0]) < 2e-3 and np.allclose(r["out9"][0, :4], G["ebu_g0_out9"][:4], atol=DB_TOL)
    r = _run_ebu_tp(M, sig.g1(48000 * 20)[None])
    assert np.allclose(r["out9"][0, :5], G["ebu_g1_out9"][:5], atol=CONTRACT_DB)
    assert abs(r["out9"][0, 0] + 23.0070) < 2e-3
    r = _run_ebu_tp(M, sig.g2(48000 * 30, 777)[None])
    assert np.allclose(r["out9"][0, :6], G["ebu_g2_out9"][:6], atol=CONTRACT_DB)
    assert abs(r["out9"][0, 4] + 10.5618) < CONTRACT_DB


def test_dc_offset_under_quiet_programme(M):
    """Integrator states ~1e4 x the output: a time-parallel scheme that splits zero-state and
    zero-input responses algebraically loses this one."""
    x = sig.dc_plus_quiet(48000 * 6)
    r = _run_ebu_tp(M, x[None])
    want = G["ebu_dc_frag_power"]
    # after the DC step has died out the programme sits ~-59 LUFS under a 0.25 DC offset
    assert np.allclose(r["frag"][0], want, rtol=1e-3)
    assert np.allclose(r["out9"][0, :4], G["ebu_dc_out9"][:4], atol=CONTRACT_DB)


def test_truepeak_golden(M):
    r = _run_ebu_tp(M, sig.lcg_noise(48000 * 3, 1234)[None])
    assert np.allclose(r["tp"][0], G["tp_lcg_peak"], rtol=2e-6)
    r = _run_ebu_tp(M, sig.g3(48000 * 2)[None])
    assert np.allclose(r["tp"][0], G["tp_g3_peak"], rtol=2e-6)
    assert abs(_db(r["tp"][0, 0]) - 3.1056) < 1e-3
    # identity phase alone: a lone full-scale sample shows up unchanged, the ringing stays below it
    x = np.zeros((1, 4800, 2), np.float32)
    x[0, 100, 0] = 1.0
    x[0, 4799, 1] = -0.5            # its interpolated outputs land after the end of the stream
    r = _run_ebu_tp(M, x)
    assert r["tp"][0, 0] == 1.0


def test_batch_against_oracle(M, oracle):
    """A ragged batch: every stream different, oracle run per stream."""
    S, T = 37, 48000 * 3 + 777
    x = np.stack([sig.lcg_noise(T, 1000 + s, 2.0 ** -(s % 5)) for s in range(S)])
    x[5] *= np.linspace(0, 1, T, dtype=np.float32)[:, None]
    x[6, :, 1] = 0
    r = _run_ebu_tp(M, x)
    for s in range(S):
        o = oracle.ebu(x[s], 48000.0, 2400, want_frag=True)
        assert np.allclose(r["out9"][s, :4], o["out9"][:4], atol=DB_TOL), s
        assert np.allclose(r["frag"][s], o["frag_power"], rtol=2e-5, atol=1e-30), s
        assert np.allclose(r["tp"][s], oracle.tp(x[s], 48000.0, 8192), rtol=2e-6), s


@pytest.mark.parametrize("calls", [[48000 * 4], [1, 46, 47, 48, 2400, 2353, 100000, 48000 * 4 - 104895],
                                   [1024] * 187 + [512]])
def test_streaming_calls_equal_one_call(M, oracle, calls):
    """State carried across process calls (K-filter, FIR history, open fragment, ring, counters)."""
    T = sum(calls)
    x = np.stack([tri_noise(T, 31 + s, 0.5, period=60000) for s in range(3)])
    one = _run_ebu_tp(M, x)
    many = _run_ebu_tp(M, x, calls=calls)
    assert np.allclose(one["out9"][:, :4], many["out9"][:, :4], atol=1e-4)
    assert np.allclose(one["tp"], many["tp"], rtol=1e-6)
    assert np.allclose(one["frag"], many["frag"], rtol=2e-5)
    o = oracle.ebu(x[1], 48000.0, 1024, want_frag=True)
    assert np.allclose(many["frag"][1], o["frag_power"], rtol=2e-5)
    assert np.abs(many["hist_M"][1] - o["hist_M"]).sum() // 2 <= MOVED_MAX


@pytest.mark.parametrize("run", [38, 39])
@pytest.mark.parametrize("segs", [1, 3, 7])
def test_time_segments_and_tile_shapes(M, oracle, run, segs):
    """Small batch: each stream split into warm-started time segments; 38-frame runs (layouts 6 and 7: the lane = segment kernel takes the
    whole-fragment part of the call, forced by tune_segments) and 39-frame runs (layout 3)."""
    T = 48000 * 9
    x = np.stack([tri_noise(T, 77 + s, 0.5, period=96000) + np.float32(0.01 * s) for s in range(2)])
    r = _run_ebu_tp(M, x, tune_run=run, tune_segments=segs)
    for s in range(2):
        o = oracle.ebu(x[s], 48000.0, 2400, want_frag=True)
        assert np.allclose(r["frag"][s], o["frag_power"], rtol=2e-5), (run, segs, s)
        assert np.allclose(r["out9"][s, :4], o["out9"][:4], atol=DB_TOL)
        assert np.allclose(r["tp"][s], oracle.tp(x[s], 48000.0, 8192), rtol=2e-6)


@pytest.mark.parametrize("fs", [44100.0, 96000.0, 22050.0, 192000.0, 88200.0, 8000.0])
def test_other_sample_rates(M, oracle, fs):
    T = int(fs) * 4 + 13
    x = sig.lcg_noise(T, 9, 0.5)
    r = _run_ebu_tp(M, x[None], fs)
    o = oracle.ebu(x, fs, 4096, want_frag=True)
    assert np.allclose(r["frag"][0], o["frag_power"], rtol=2e-5)
    assert np.allclose(r["out9"][0, :4], o["out9"][:4], atol=DB_TOL)
    assert np.allclose(r["tp"][0], oracle.tp(x, fs, 8192), rtol=2e-6)


def test_integration_control(M, oracle):
    """integr_start / pause / reset follow Ebu_r128_proc (ebu_r128_proc.h:77-79)."""
    x = tri_noise(48000 * 6, 3, 0.5, period=48000)
    with M.Engine(1, 48000.0, M.METER_EBU) as e:
        e.process(x[None, :48000 * 2])             # integration off: M/S run, histograms stay empty
        assert e.results()[0].hist_M_count == 0 and e.out9()[0, 4] == -200.0
        assert e.out9()[0, 0] > -100
        e.integr_start()
        e.process(x[None, 48000 * 2:48000 * 4])
        c1 = e.results()[0].hist_M_count
        assert c1 == 20                            # one point per 100 ms
        e.integr_pause()
        e.process(x[None, 48000 * 4:48000 * 5])
        assert e.results()[0].hist_M_count == c1
        e.integr_reset()
        r = e.results()[0]
        assert r.hist_M_count == 0 and r.maxloudn_M == -200.0 and r.integrated == -200.0
        e.reset()
        assert e.out9()[0, 0] == -200.0


def test_edge_cases(M):
    with M.Engine(2, 48000.0, M.METER_EBU | M.METER_TRUEPEAK) as e:
        e.integr_start()
        e.process(np.zeros((2, 0, 2), np.float32))          # empty call is a no-op
        e.process(np.zeros((2, 2400 * 3, 2), np.float32))   # digital silence
        r = e.out9()
        assert np.all(r[:, 0] == -200.0) and np.all(e.truepeak() == 0.0)
        x = np.zeros((2, 2400, 2), np.float32)
        x[0, :, 0] = np.nan                                  # NaN never wins a max, never sticks in state
        x[1, 7, 1] = np.inf
        e.process(x)
        e.process(np.full((2, 2400 * 8, 2), 0.25, np.float32))
        r = e.results()
        assert r[0].truepeak[0] < 1.0 and np.isfinite(r[0].loudness_M)
        assert r[1].truepeak[1] == np.inf
    with pytest.raises(M.EngineError):
        M.Engine(1, 48000.0, M.METER_EBU, n_channels=1)
    with pytest.raises(M.EngineError):
        M.Engine(0)
    with pytest.raises(M.EngineError):
        M.Engine(1, 48000.0, 0x100)                          # a bit that is no meter
    with pytest.raises(M.EngineError):
        M.Engine(1, 48000.0, M.METER_EBU, tune_layout=6)     # the matrix-pipe layouts need TRUEPEAK
    with pytest.raises(M.EngineError):
        M.Engine(1, 48000.0, M.METER_DR14 | M.METER_BITSTATS)   # stereo and mono-only meters do not mix


def test_filter_bank_golden(M, oracle):
    x = sig.lcg_noise(48000, 42, 0.5)
    with M.Engine(1, 48000.0, M.METER_SPECTR30) as e:
        for p in range(0, 48000, 1024):
            e.process(x[None, p:p + 1024])
        r = e.spectrum()
    assert np.allclose(r["val"][0], G["spectr_lcg_val"], rtol=1e-4)
    assert np.allclose(r["max"][0], G["spectr_lcg_max"], rtol=1e-4)
    assert np.allclose(r["val_db"][0], G["spectr_lcg_val_db"], atol=1e-3)
    assert np.allclose(r["max_db"][0], G["spectr_lcg_max_db"], atol=1e-3)
    with M.Engine(1, 48000.0, M.METER_SPECTR30) as e:
        e.process(sig.g4(48000 * 2, 16)[None])
        r = e.spectrum()
    assert abs(r["val_db"][0, 16]) < 0.01
    live = G["spectr_g4_16_val_db"] > -90
    assert np.allclose(r["val_db"][0][live], G["spectr_g4_16_val_db"][live], atol=1e-3)


def test_filter_bank_batch_and_rates(M, oracle):
    S, T = 19, 20000
    x = np.stack([sig.lcg_noise(T, 500 + s, 0.5) for s in range(S)])
    for fs in (48000.0, 44100.0):
        with M.Engine(S, fs, M.METER_SPECTR30) as e:
            e.process(x)
            r = e.spectrum()
        for s in range(S):
            o = oracle.spectr(x[s], fs, T)
            assert np.allclose(r["val"][s], o["val"], rtol=1e-4), (fs, s)
            assert np.allclose(r["val_db"][s], o["val_db"], atol=1e-3)
            assert np.allclose(r["max"][s], o["max"], rtol=1e-4), (fs, s)
            assert np.allclose(r["max_db"][s], o["max_db"], atol=1e-3)
    # mono variant (spectr30mono): input is the single channel itself
    with M.Engine(2, 48000.0, M.METER_SPECTR30, n_channels=1) as e:
        e.process(np.ascontiguousarray(x[:2, :, 0]))
        r = e.spectrum()
    stereo_same = np.repeat(x[0, :, :1], 2, axis=1)
    o = oracle.spectr(stereo_same, 48000.0, T)
    assert np.allclose(r["val"][0], o["val"], rtol=1e-4)
    assert np.allclose(r["max"][0], o["max"], rtol=1e-4) and np.allclose(r["max_db"][0], o["max_db"], atol=1e-3)


def test_all_meters_together(M, oracle):
    x = np.stack([sig.g2(48000 * 3, 777 + s) for s in range(4)])
    with M.Engine(4, 48000.0, M.METER_EBU | M.METER_TRUEPEAK | M.METER_SPECTR30) as e:
        e.integr_start()
        e.process(x)
        out9, tp, sp = e.out9(), e.truepeak(), e.spectrum()
    for s in range(4):
        assert np.allclose(out9[s, :4], oracle.ebu(x[s], 48000.0, 2400)["out9"][:4], atol=DB_TOL)
        assert np.allclose(tp[s], oracle.tp(x[s], 48000.0, 8192), rtol=2e-6)
        assert np.allclose(sp["val_db"][s], oracle.spectr(x[s], 48000.0, 48000 * 3)["val_db"], atol=1e-3)


def test_aggregate_for_multi_gpu_reduce(M, oracle):
    import torch
    S = 6
    x = np.stack([tri_noise(48000 * 8, 50 + s, 0.5, period=48000 * 2) for s in range(S)])
    with M.Engine(S, 48000.0, M.METER_EBU | M.METER_TRUEPEAK) as e:
        e.integr_start()
        e.process(x)
        dh = torch.zeros(2 * 751, dtype=torch.int32, device="cuda")
        dm = torch.zeros(4, dtype=torch.float32, device="cuda")
        e.aggregate_device(dh.data_ptr(), dm.data_ptr())
        torch.cuda.synchronize()
        hm, hs = e.histograms()
        out9, tp = e.out9(), e.truepeak()
    h = dh.cpu().numpy().reshape(2, 751)
    assert np.array_equal(h[0], hm.sum(0)) and np.array_equal(h[1], hs.sum(0))
    m = dm.cpu().numpy()
    assert m[0] == tp[:, 0].max() and m[1] == tp[:, 1].max()
    assert m[2] == out9[:, 1].max() and m[3] == out9[:, 3].max()
    prog = M.hist_loudness(h[0], h[1])
    assert -70 < prog[0] < 0 and prog[2] <= prog[3]


@pytest.mark.timeout(900)
@pytest.mark.parametrize("fs", [48000.0, 44100.0])
def test_full_size_properties(M, oracle, fs):
    """BASELINE.json's per-GPU shard (8192 streams x 10 s, 31.5 GB) through size-independent
    properties: determinism, exact x2 scaling (power-of-two gain is exact in fp32: peaks double
    exactly, fragment powers quadruple exactly, LUFS moves by 20 log10 2), position independence,
    and oracle parity on streams sampled out of the full batch."""
    import torch
    S, T = 8192, int(fs) * 10                                # (44.1 kHz: fragments of 2205 frames end inside k_seg's 16-frame steps)
    free, _ = torch.cuda.mem_get_info()
    if free < (S * T * 8) * 1.05:
        S = int(free * 0.9 / (T * 8)) // 256 * 256
    buf = torch.empty((S, T, 2), dtype=torch.float32, device="cuda")
    M.synth_fill_device(buf.data_ptr(), S, T, T, 777, fs, 1)
    torch.cuda.synchronize()
    pick = sorted({0, 1, S // 2 + 3, S - 1} | {(S * k) // 31 + (7 * k) % 13 for k in range(1, 31)})   # 34 streams: both ends, every wave position
    mid = S // 2 + 3

    def run(ptr):
        with M.Engine(S, fs, M.METER_EBU | M.METER_TRUEPEAK) as e:
            e.integr_start()
            e.process_device(ptr, T)
            hm, hs = e.histograms()
            return e.out9(), e.truepeak(), hm, hs, e.fragment_powers(mid, 1)

    a = run(buf.data_ptr())
    b = run(buf.data_ptr())
    for u, v in zip(a, b):
        assert np.array_equal(u, v)                         # deterministic
    host = {s: buf[s].cpu().numpy() for s in pick}
    for s in pick:                                           # oracle parity on sampled streams
        o = oracle.ebu(host[s], fs, int(fs) // 20)
        assert np.allclose(a[0][s, :4], o["out9"][:4], atol=DB_TOL), s
        assert abs(a[0][s, 4] - o["out9"][4]) <= CONTRACT_DB
        assert np.allclose(a[1][s], oracle.tp(host[s], fs, 8192), rtol=2e-6), s
        assert np.abs(a[2][s] - o["hist_M"]).sum() // 2 <= MOVED_MAX and np.abs(a[3][s] - o["hist_S"]).sum() // 2 <= MOVED_MAX
    assert a[2].sum() == S * 100 and a[3].sum() == S * 20    # every stream: 100 M points, 20 S points
    # The histogram flip RATE, measured: every 16th stream of the batch against the oracle — 51 200 M points
    # and 10 240 S points — and the programme record of the SUMMED histograms (what mtr_engine_reduce feeds mtr_hist_loudness)
    # against the oracle's summed histograms.
    wide = list(range(0, S, 16))
    hw = torch.stack([buf[s] for s in wide]).cpu().numpy()
    oh = [oracle.ebu(hw[i], fs, int(fs) // 20) for i in range(len(wide))]
    del hw
    om, os_ = np.stack([o["hist_M"] for o in oh]), np.stack([o["hist_S"] for o in oh])
    mv_m, far_m = moved_points(a[2][wide], om)
    mv_s, far_s = moved_points(a[3][wide], os_)
    worst = max(int(np.abs(a[2][wide[i]] - om[i]).sum() // 2) for i in range(len(wide)))
    prog_g = M.hist_loudness(a[2][wide].sum(0), a[3][wide].sum(0))
    prog_o = M.hist_loudness(om.sum(0), os_.sum(0))
    print("\nhistogram flips at %g Hz over %d streams: M %d of %d points (%.2e per point, farthest %d bin), S %d of %d (%.2e), worst stream %d; "
          "programme I %.4f vs %.4f LUFS, LRA edges %s vs %s"
          % (fs, len(wide), mv_m, om.sum(), mv_m / om.sum(), far_m, mv_s, os_.sum(), mv_s / max(os_.sum(), 1), worst,
             prog_g[0], prog_o[0], prog_g[2:4], prog_o[2:4]))
    assert mv_m <= moved_allowed(om.sum()) and mv_s <= moved_allowed(os_.sum()) and far_m <= 1 and far_s <= 1
    assert abs(prog_g[0] - prog_o[0]) <= CONTRACT_DB and abs(prog_g[1] - prog_o[1]) <= CONTRACT_DB
    assert abs(prog_g[2] - prog_o[2]) <= 0.1001 and abs(prog_g[3] - prog_o[3]) <= 0.1001 and abs(prog_g[4] - prog_o[4]) <= CONTRACT_DB
    dev_i = max(abs(float(a[0][wide[i], 4]) - float(oh[i]["out9"][4])) for i in range(len(wide)))
    assert dev_i <= CONTRACT_DB, dev_i
    buf.mul_(2.0)
    torch.cuda.synchronize()
    c = run(buf.data_ptr())
    assert np.array_equal(c[1], 2 * a[1])                   # peaks double exactly
    assert np.array_equal(c[4], 4 * a[4])                   # fragment powers quadruple exactly
    assert np.allclose(c[0][:, :4], a[0][:, :4] + 20 * np.log10(2.0), atol=1e-4)
    # position independence: the same audio at another batch index gives the same record
    small = torch.stack([buf[s] for s in pick])
    with M.Engine(len(pick), fs, M.METER_EBU | M.METER_TRUEPEAK) as e:
        e.integr_start()
        e.process_device(small.data_ptr(), T)
        o9, tp = e.out9(), e.truepeak()
    assert np.allclose(o9[:, :4], c[0][pick, :4], atol=1e-4) and np.allclose(tp, c[1][pick], rtol=1e-6)


@pytest.mark.timeout(900)
def test_config1_one_stream_one_hour_whole_record(M, oracle):
    """BASELINE configs[1] at its stated size: ONE stream x 3600 s at 48 kHz (172.8 M frames, 1.38 GB) in one call —
    k_kw with thousands of time segments, the multi-workgroup gate over 72 000 fragments, 36 000 + 7 200 histogram points
    (Ebu_r128_proc::process, ebumeter/ebu_r128_proc.cc:207-248).  The WHOLE record against the oracle: nine floats, both
    histograms, both counts, every one of the 72 000 fragment powers; then the same hour with the true peak beside it
    (k_kwtp16: one stream cannot fill k_seg's lanes) — same record within the same bounds, peak against oracle.tp over the
    whole hour.  Prints the number of histogram points that sit in a neighbouring bin."""
    import torch
    fs, T = 48000.0, 3600 * 48000
    buf = torch.empty((1, T, 2), dtype=torch.float32, device="cuda")
    M.synth_fill_device(buf.data_ptr(), 1, T, T, 4242, fs, 1)
    torch.cuda.synchronize()
    x = buf[0].cpu().numpy()
    o = oracle.ebu(x, fs, 4096, want_frag=True)
    assert o["frag_power"].shape == (72000,) and tuple(o["counts"]) == (36000, 7200)

    def check(e, tag):
        got9 = e.out9()[0]
        hm, hs = e.histograms()
        r = e.results()[0]
        frag = e.fragment_powers()[0]
        assert (r.hist_M_count, r.hist_S_count) == (36000, 7200)
        assert frag.shape == (72000,)
        rel = np.abs(frag.astype(np.float64) - o["frag_power"]) / o["frag_power"]
        assert rel.max() <= 2e-5, (tag, rel.max(), int(rel.argmax()))
        assert np.allclose(got9[:4], o["out9"][:4], atol=DB_TOL), (tag, got9, o["out9"])
        mv_m, far_m = moved_points(hm[0], o["hist_M"])
        mv_s, far_s = moved_points(hs[0], o["hist_S"])
        print("\n%s, 1 stream x 3600 s: %d of 36000 M points and %d of 7200 S points in a neighbouring bin (farthest %d); largest "
              "fragment-power deviation %.2e; I %.4f vs %.4f, LRA %.1f..%.1f vs %.1f..%.1f"
              % (tag, mv_m, mv_s, max(far_m, far_s), rel.max(), got9[4], o["out9"][4], got9[6], got9[7], o["out9"][6], o["out9"][7]))
        assert mv_m <= moved_allowed(36000) and mv_s <= moved_allowed(7200) and far_m <= 1 and far_s <= 1
        assert abs(got9[4] - o["out9"][4]) <= CONTRACT_DB and abs(got9[5] - o["out9"][5]) <= CONTRACT_DB
        assert abs(got9[6] - o["out9"][6]) <= 0.1001 and abs(got9[7] - o["out9"][7]) <= 0.1001 and abs(got9[8] - o["out9"][8]) <= CONTRACT_DB
        if mv_m == 0 and mv_s == 0:
            # identical histograms -> the identical gated record: the LRA edges (bin indices) bit for bit; I and the two
            # thresholds to the last ulp or two — they are 10 log10f (s) of identical sums, and the device's log10f is the
            # correctly rounded one ((float) log10 ((double) s)) while this image's glibc 2.35 log10f is only within ~2 ulp of
            # it (measured here: range_thr -31.482706 vs -31.482708): 4e-7 relative = 1e-5 dB
            assert got9[6] == o["out9"][6] and got9[7] == o["out9"][7]
            assert np.allclose(got9[[4, 5, 8]], o["out9"][[4, 5, 8]], rtol=4e-7, atol=0)
        return got9, hm, hs, frag

    with M.Engine(1, fs, M.METER_EBU) as e:
        e.integr_start()
        e.process_device(buf.data_ptr(), T)
        assert e.layout() == 4
        first = check(e, "EBU R128 (k_kw)")
        e.reset(); e.integr_start()
        e.process_device(buf.data_ptr(), T)                                # deterministic
        again = (e.out9()[0], *e.histograms(), e.fragment_powers()[0])
        for u, v in zip(first, again):
            assert np.array_equal(u, v)
    with M.Engine(1, fs, M.METER_EBU | M.METER_TRUEPEAK) as e:
        e.integr_start()
        e.process_device(buf.data_ptr(), T)
        check(e, "EBU R128 + true peak (k_kwtp16)")
        assert np.allclose(e.truepeak()[0], oracle.tp(x, fs, 8192), rtol=2e-6)


@pytest.mark.timeout(900)
def test_config2_truepeak_alone_full_size(M, oracle):
    """BASELINE configs[2] at its stated size: 4x true peak alone, 1024 streams x 60 s (23.6 GB) — TruePeakdsp::process_max
    (jmeters/truepeakdsp.cc:101-124) over Resampler::process: deterministic, peaks double exactly under a power-of-two gain,
    the same audio at another batch index gives the same peaks, 34 sampled streams against oracle.tp over their whole minute."""
    import torch
    fs, S, T = 48000.0, 1024, 60 * 48000
    free, _ = torch.cuda.mem_get_info()
    if free < (S * T * 8) * 1.05:
        S = int(free * 0.9 / (T * 8)) // 64 * 64
    buf = torch.empty((S, T, 2), dtype=torch.float32, device="cuda")
    M.synth_fill_device(buf.data_ptr(), S, T, T, 2024, fs, 1)
    torch.cuda.synchronize()
    pick = sorted({0, 1, S // 2 + 3, S - 1} | {(S * k) // 31 + (7 * k) % 13 for k in range(1, 31)})

    def run(ptr, n=S):
        with M.Engine(n, fs, M.METER_TRUEPEAK) as e:
            e.process_device(ptr, T)
            r = e.results()
            return e.truepeak(), np.array([[x.truepeak_call[0], x.truepeak_call[1]] for x in r], np.float32), e.seg_stats()[0]

    a = run(buf.data_ptr())
    b = run(buf.data_ptr())
    assert a[2] == 1                                          # the batch went through k_seg
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[0], a[1])
    for s in pick:
        assert np.allclose(a[0][s], oracle.tp(buf[s].cpu().numpy(), fs, 8192), rtol=2e-6), s
    small = torch.stack([buf[s] for s in pick])
    c = run(small.data_ptr(), len(pick))
    assert np.allclose(c[0], a[0][pick], rtol=1e-6)           # (34 streams plan other segments than 1024: same peaks to the last bits of the f16 split)
    buf.mul_(2.0)
    torch.cuda.synchronize()
    d = run(buf.data_ptr())
    assert np.array_equal(d[0], 2 * a[0])                    # peaks double exactly
    assert (a[0] > 0.05).all() and (a[0] < 2.0).all()


@pytest.mark.timeout(1200)
def test_config4_three_meters_in_one_engine_full_size(M):
    """BASELINE configs[4]'s per-GPU shard with everything on: EBU R128 + true peak + the 30-band bank in ONE engine at
    8192 streams x 10 s (spectrum_run's loop beside process / process_max: src/spectrumlv2.c:210-227, ebu_r128_proc.cc:207-248,
    truepeakdsp.cc:101-124) must give, bit for bit, the records of the meters in separate engines over the same buffer:
    EBU + true peak (one fused kernel either way), the bank alone, true peak alone (the same interpolator with the
    K-filter compiled out).  EBU alone runs another kernel (k_kw: the exact time-parallel scan): its record agrees within
    the stated tolerances, not bitwise."""
    import torch
    fs, S, T = 48000.0, 8192, 480000
    free, _ = torch.cuda.mem_get_info()
    if free < (S * T * 8) * 1.05:
        S = int(free * 0.9 / (T * 8)) // 256 * 256
    buf = torch.empty((S, T, 2), dtype=torch.float32, device="cuda")
    M.synth_fill_device(buf.data_ptr(), S, T, T, 99, fs, 1)
    torch.cuda.synchronize()

    def run(meters):
        with M.Engine(S, fs, meters) as e:
            if meters & M.METER_EBU:
                e.integr_start()
            e.process_device(buf.data_ptr(), T)
            out = {}
            if meters & M.METER_EBU:
                out["o9"] = e.out9()
                out["hm"], out["hs"] = e.histograms()
                out["frag"] = e.fragment_powers()
            if meters & M.METER_TRUEPEAK:
                out["tp"] = e.truepeak()
            if meters & M.METER_SPECTR30:
                sp = e.spectrum()
                out["val"], out["max"] = sp["val"], sp["max"]
            return out

    all3 = run(M.METER_EBU | M.METER_TRUEPEAK | M.METER_SPECTR30)
    two = run(M.METER_EBU | M.METER_TRUEPEAK)
    for k in ("o9", "hm", "hs", "frag", "tp"):
        assert np.array_equal(all3[k], two[k], equal_nan=True), k
    bank = run(M.METER_SPECTR30)
    for k in ("val", "max"):
        assert np.array_equal(all3[k], bank[k]), k
    tp = run(M.METER_TRUEPEAK)
    assert np.array_equal(all3["tp"], tp["tp"])
    ebu = run(M.METER_EBU)
    assert np.allclose(ebu["o9"][:, :4], all3["o9"][:, :4], atol=DB_TOL)
    assert np.abs(ebu["o9"][:, 4] - all3["o9"][:, 4]).max() <= CONTRACT_DB
    assert np.allclose(ebu["frag"], all3["frag"], rtol=2e-5)
    mv, far = moved_points(ebu["hm"], all3["hm"])
    assert mv <= moved_allowed(S * 100) and far <= 1
    assert all3["hm"].sum() == S * 100 and all3["hs"].sum() == S * 20 and (all3["val"] > 0).all() and (all3["tp"] > 0.05).all()


@pytest.mark.parametrize("meters", ["ebu", "ebu+tp"])
def test_long_call_gate_spread_over_workgroups(M, oracle, meters):
    """>= 4096 fragments in one call take the multi-workgroup gate (k_gate_frag + k_gate_final): same record,
    histograms and fragment powers as the oracle, and as the same audio fed in short calls (single-workgroup path)."""
    fs = 48000.0
    T = int(fs) * 215 + 1234                                  # 4300 fragments
    x = np.stack([sig.lcg_noise(T, 91 + s, 0.25 * (s + 1)) for s in range(2)])
    env = (0.1 + 0.9 * ((np.arange(T) // 240000) % 3 == 0)).astype(np.float32)      # loud / quiet alternation: gating matters
    x = (x * env[None, :, None]).astype(np.float32)
    mask = M.METER_EBU | (M.METER_TRUEPEAK if meters == "ebu+tp" else 0)

    def run(cuts):
        # one time segment per stream and calls cut on fragment boundaries: both runs see the same tiles and the
        # same carried K-filter state, so everything downstream must be bit-identical
        with M.Engine(2, fs, mask, tune_segments=1) as e:
            e.integr_start()
            frags = []
            for a, b in zip(cuts[:-1], cuts[1:]):
                e.process(np.ascontiguousarray(x[:, a:b]))
                frags.append(e.fragment_powers())
            hm, hs = e.histograms()
            return e.out9(), np.concatenate(frags, 1), hm, hs, e.results()

    one = run([0, T])
    many = run(list(range(0, T, 2400 * 400)) + [T])           # 11 calls of 400 fragments: the single-workgroup gate
    assert np.array_equal(one[1], many[1])                    # fragment powers do not depend on the call pattern here
    assert np.array_equal(one[2], many[2]), np.flatnonzero(one[2] != many[2])[:8]
    assert np.array_equal(one[3], many[3]), np.flatnonzero(one[3] != many[3])[:8]
    assert np.array_equal(one[0], many[0]), (one[0], many[0])
    for s in range(2):
        o = oracle.ebu(x[s], fs, 4096, want_frag=True)
        assert np.allclose(one[1][s], o["frag_power"], rtol=2e-5)
        assert np.allclose(one[0][s, :4], o["out9"][:4], atol=DB_TOL)
        assert abs(one[0][s, 4] - o["out9"][4]) <= 0.01 and abs(one[0][s, 6] - o["out9"][6]) <= 0.1001
        assert np.abs(one[2][s] - o["hist_M"]).sum() // 2 <= MOVED_MAX and np.abs(one[3][s] - o["hist_S"]).sum() // 2 <= MOVED_MAX
        assert (one[4][s].hist_M_count, one[4][s].hist_S_count) == tuple(o["counts"])


@pytest.mark.parametrize("chn,S,T", [(1, 131, 5003), (2, 131, 5003), (2, 8192 + 67, 1203)])
def test_truepeak_ballistics_many_streams(M, oracle, chn, S, T):
    """The batch layouts of k_tpb: 32 streams per workgroup (two lanes per stream in the interpolators) for
    batches up to 8192 streams, 64 beyond; the last workgroup partly filled, 12-frame chunks with a ragged
    tail, three calls of odd sizes, mono and stereo engines; sampled streams against the oracle."""
    import ctypes as C
    from _oracle import MoTp
    # levels from full scale down: 2^-(s % 4), and -40 / -60 / -80 dBFS on streams 5, 6, 7 (mod 8) — the gate below is RELATIVE
    # to the value (2e-6 of max (1, value) is 0.017 dB at a level of 1e-3, outside the +-0.01 dB contract)
    quiet = {5: 1e-2, 6: 1e-3, 7: 1e-4}
    base = np.stack([sig.lcg_noise(T, 700 + s, 2.0 ** -(s % 4) * quiet.get(s % 8, 1.0)) for s in range(131)])  # [131][T][2]
    x = base if S == 131 else base[np.arange(S) % 131] * (1.0 + (np.arange(S) // 131)[:, None, None].astype(np.float32) / 64)
    feed = x if chn == 2 else np.ascontiguousarray(x[:, :, 0])
    cuts = (0, 17, 2400 if T > 2400 else 700, T)
    with M.Engine(S, 48000.0, M.METER_TPBALLIST, n_channels=chn) as e:
        got = []
        for a, b in zip(cuts[:-1], cuts[1:]):
            e.process(np.ascontiguousarray(feed[:, a:b]))
            r = e.results()
            got.append([[(r[s].tpb_level[c], r[s].tpb_peak[c]) for c in range(chn)] for s in range(S)])
    for s in (0, 1, 5, 6, 7, 31, 32, 63, 64, 65, 127, 128, 130) + ((4095, 8191, 8192, S - 1) if S > 131 else ()):
        for c in range(chn):
            ch = np.ascontiguousarray(x[s, :, c])
            t = MoTp()
            oracle.lib.mo_tp_init(C.byref(t), 48000.0)
            m, p = C.c_float(), C.c_float()
            for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
                seg = np.ascontiguousarray(ch[a:b])
                oracle.lib.mo_tp_process(C.byref(t), seg, seg.size)
                oracle.lib.mo_tp_read2(C.byref(t), C.byref(m), C.byref(p))
                assert abs(got[i][s][c][0] - m.value) <= TPB_REL * m.value + 1e-37, (s, c, i, got[i][s][c][0], m.value)
                assert abs(got[i][s][c][1] - p.value) <= TPB_REL * p.value + 1e-37, (s, c, i, got[i][s][c][1], p.value)


def test_truepeak_ballistics_batch(M, oracle):
    """TruePeakdsp::process (PPM-style ballistics) for a batch, two calls = two process()+read() blocks."""
    S, T = 5, 6000
    x = np.stack([sig.lcg_noise(T, 40 + s, 2.0 ** -(s % 3)) for s in range(S)])
    with M.Engine(S, 48000.0, M.METER_TPBALLIST) as e:
        got = []
        for p in (0, 2500):
            e.process(x[:, p:p + (2500 if p == 0 else 3500)])
            r = e.results()
            got.append([[(r[s].tpb_level[c], r[s].tpb_peak[c]) for c in range(2)] for s in range(S)])
    import ctypes as C
    from _oracle import MoTp
    for s in range(S):
        for c in range(2):
            ch = np.ascontiguousarray(x[s, :, c])
            t = MoTp()          # a fresh oracle object per channel, fed the same two blocks
            oracle.lib.mo_tp_init(C.byref(t), 48000.0)
            m, p = C.c_float(), C.c_float()
            for i, (a, b) in enumerate(((0, 2500), (2500, 6000))):
                seg = np.ascontiguousarray(ch[a:b])
                oracle.lib.mo_tp_process(C.byref(t), seg, seg.size)
                oracle.lib.mo_tp_read2(C.byref(t), C.byref(m), C.byref(p))
                assert abs(got[i][s][c][0] - m.value) <= TPB_REL * m.value + 1e-37, (s, c, i, got[i][s][c][0], m.value)
                assert abs(got[i][s][c][1] - p.value) <= TPB_REL * p.value + 1e-37, (s, c, i, got[i][s][c][1], p.value)


def test_truepeak_ballistics_column_scale_moves(M, oracle):
    """k_tpb splits every sample once, into a ring of f16 halves under a power-of-two scale per column that follows the
    window's maximum with hysteresis and rescales the ring in place when it has to move (mtr_tpb.hip).  Signals that make
    it move: 120 dB down and up again, digital silence in between, a ramp of 6 dB per millisecond over 240 dB, lone
    full-scale samples in quiet noise (the scale shrinks for 64 frames and grows back, every time), an Inf and a NaN.
    Level and peak per call against TruePeakdsp::process / read — RELATIVE to the value itself here (4e-6; the other tests
    allow 2e-6 of max (1, value), which says nothing about a call that lies in a quiet stretch)."""
    import ctypes as C
    from _oracle import MoTp
    fs, T = 48000.0, 75000
    n = [sig.lcg_noise(T, 900 + s, 1.0) for s in range(5)]
    a = n[0] * np.float32(0.5)
    a[20000:50000] *= np.float32(2.0 ** -20); a[50000:55000] = 0.0; a[55000:65000] *= np.float32(2.0 ** -10); a[65000:] *= np.float32(1.8)
    b = n[1].copy()
    up = np.minimum(np.arange(T) - 3000, 48 * 40) / 48.0
    b *= (np.float32(2.0) ** (up - 40.0))[:, None].astype(np.float32)
    b[:3000] = 0.0
    b[40000:] *= (np.float32(2.0) ** (-(np.arange(T - 40000) / 96.0)))[:, None].astype(np.float32)        # ... and down again, 3 dB per ms, into denormals
    c = n[2] * np.float32(2.0 ** -8)
    c[777::777, 0] = 1.0; c[1000::1554, 1] = -0.75
    d = n[3] * np.float32(0.25); d[30000, 0] = np.inf; d[30000, 1] = np.nan
    e_ = n[4] * np.float32(1e-12); e_[60000:] *= np.float32(1e8)       # (far above the 1e-20f the reference adds to its states per block)
    x = np.stack([a, b, c, d, e_])
    cuts = (0, 7000, 7033, 26000, 52000, 52001, 66000, T)
    with M.Engine(5, fs, M.METER_TPBALLIST) as eng:
        got = []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            eng.process(np.ascontiguousarray(x[:, lo:hi]))
            r = eng.results()
            got.append([[(r[s].tpb_level[ch], r[s].tpb_peak[ch]) for ch in range(2)] for s in range(5)])
    for s in range(5):
        for ch in range(2):
            col = np.ascontiguousarray(x[s, :, ch])
            t = MoTp()
            oracle.lib.mo_tp_init(C.byref(t), fs)
            m, p = C.c_float(), C.c_float()
            for i, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):
                mm = pp = 0.0
                for o in range(lo, hi, 8192):
                    seg = np.ascontiguousarray(col[o:min(o + 8192, hi)])
                    oracle.lib.mo_tp_process(C.byref(t), seg, seg.size)
                    oracle.lib.mo_tp_read2(C.byref(t), C.byref(m), C.byref(p))
                    mm, pp = max(mm, m.value), max(pp, p.value)
                gm, gp = got[i][s][ch]
                if s == 3 and i >= 3:
                    # From the call with the Inf / NaN sample on.  The Inf is that call's peak and level, as in the reference (which
                    # would clamp the state at the next 8192-frame block; one engine call is one block, so the levels behind it are
                    # not comparable).  The NaN's channel comes back finite: a NaN loses every `v > z` and every maximum.
                    if ch == 0 and i == 3:
                        assert gp == np.inf and gm == np.inf and mm == np.inf, (gm, gp, mm, pp)
                    assert not np.isnan(gm) and not np.isnan(gp), (ch, i, gm, gp)
                    if ch == 1:
                        assert np.isfinite(gm) and np.isfinite(gp), (i, gm, gp)
                    continue
                assert abs(gm - mm) <= TPB_REL * mm + 1e-37, (s, ch, i, gm, mm)
                assert abs(gp - pp) <= TPB_REL * pp + 1e-37, (s, ch, i, gp, pp)


@pytest.mark.parametrize("chn", [2, 1])
def test_truepeak_ballistics_fetch_paths_agree(M, chn):
    """k_tpb brings whole chunks in by LDS-DMA (16-byte aligned streams) and everything else — a batch whose streams start
    on 4 or 8 bytes (odd stride, a view into a larger buffer), the call's ragged last chunk — by plain loads: the same
    samples either way, so level and peak must be the same bits."""
    import torch
    S, T = 37, 5003
    x = np.stack([sig.lcg_noise(T, 60 + s, 2.0 ** -(s % 5)) for s in range(S)])
    if chn == 1:
        x = np.ascontiguousarray(x[:, :, 0])
    st = torch.cuda.current_stream().cuda_stream
    got = []
    for stride, off in ((T + 3 if chn == 1 else T, 0), (T + 5, 2 if chn == 2 else 1), (T + (8 - T % 8), 0)):     # no DMA (stride); no DMA (base); DMA
        flat = torch.zeros(S * stride * chn + 8, dtype=torch.float32, device="cuda")
        view = flat[off:off + S * stride * chn].view(S, stride, chn) if chn == 2 else flat[off:off + S * stride].view(S, stride)
        view[:, :T] = torch.from_numpy(x).cuda()
        with M.Engine(S, 48000.0, M.METER_TPBALLIST, n_channels=chn) as e:
            rec = []
            for lo, hi in ((0, 1600), (1600, 1617), (1617, T)):
                e.process_device(flat.data_ptr() + 4 * (off + lo * chn), hi - lo, stride, st)
                r = e.results()
                rec.append([(r[s].tpb_level[c], r[s].tpb_peak[c]) for s in range(S) for c in range(chn)])
        got.append(np.array(rec, np.float32))
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2])
    assert np.all(got[0] > 0)


def test_truepeak_ballistics_full_size_properties(M, oracle):
    """TruePeakdsp::process at the per-GPU shard of the bench (8192 streams x 10 s) through size-independent properties:
    determinism; exact x2 scaling (a power-of-two gain is exact in fp32, in the f16 split — the column's scale moves with
    it — in the per-frame maps and on the chain: level and peak double exactly while the state stays under the clamp at 20);
    position independence; and the oracle (the reference's own object) on streams sampled out of the batch, fed in the
    8192-frame blocks TruePeakdsp::process allows."""
    import ctypes as C
    import torch
    from _oracle import MoTp
    S, T, fs = 8192, 480000, 48000.0
    free, _ = torch.cuda.mem_get_info()
    if free < (S * T * 8) * 1.05:
        S = int(free * 0.9 / (T * 8)) // 256 * 256
    buf = torch.empty((S, T, 2), dtype=torch.float32, device="cuda")
    M.synth_fill_device(buf.data_ptr(), S, T, T, 4242, fs, 1)
    torch.cuda.synchronize()

    def run(ptr, n=S):
        with M.Engine(n, fs, M.METER_TPBALLIST) as e:
            e.process_device(ptr, T)
            r = e.results()
            return np.array([[r[s].tpb_level[0], r[s].tpb_level[1], r[s].tpb_peak[0], r[s].tpb_peak[1]] for s in range(n)], np.float32)

    a = run(buf.data_ptr())
    assert np.array_equal(a, run(buf.data_ptr()))                       # deterministic
    assert np.all(a > 0) and np.all(a[:, :2] < 20.0)
    pick = sorted({0, 1, S // 2 + 3, S - 1} | {(S * k) // 31 + (7 * k) % 13 for k in range(1, 31)})   # 34 streams: both ends, every wave position
    mid = S // 2 + 3
    for s in pick:
        xs = buf[s].cpu().numpy()
        for c in range(2):
            ch = np.ascontiguousarray(xs[:, c])
            t = MoTp()
            oracle.lib.mo_tp_init(C.byref(t), fs)
            m, p = C.c_float(), C.c_float()
            mm = pp = 0.0
            for o in range(0, T, 8192):                                 # read (m, p) restarts the maxima: the call's are the maxima of the blocks'
                seg = np.ascontiguousarray(ch[o:o + 8192])
                oracle.lib.mo_tp_process(C.byref(t), seg, seg.size)
                oracle.lib.mo_tp_read2(C.byref(t), C.byref(m), C.byref(p))
                mm, pp = max(mm, m.value), max(pp, p.value)
            assert abs(a[s, c] - mm) <= TPB_REL * mm + 1e-37, (s, c, a[s, c], mm)
            assert abs(a[s, 2 + c] - pp) <= TPB_REL * pp + 1e-37, (s, c, a[s, 2 + c], pp)
    small = torch.stack([buf[s] for s in pick])
    assert np.array_equal(run(small.data_ptr(), len(pick)), a[pick])    # the same audio at another batch index: the same numbers
    buf.mul_(2.0)
    torch.cuda.synchronize()
    assert np.array_equal(run(buf.data_ptr()), 2 * a)                   # level and peak double exactly


def test_filter_bank_full_size_properties(M, oracle):
    """BASELINE config 3 (4096 streams x 10 s through the 30-band bank) through size-independent properties: determinism,
    position independence, a gain of 2 = + 6.0206 dB in every band (the +-1e-12 anti-denormal toggle is the only thing that
    does not scale: far below 1e-4 dB at these levels), and the oracle on streams sampled out of the batch."""
    import torch
    S, T, fs = 4096, 480000, 48000.0
    buf = torch.empty((S, T, 2), dtype=torch.float32, device="cuda")
    M.synth_fill_device(buf.data_ptr(), S, T, T, 99, fs, 1)
    torch.cuda.synchronize()

    def run(ptr, n=S):
        with M.Engine(n, fs, M.METER_SPECTR30) as e:
            e.process_device(ptr, T)
            r = e.spectrum()
            return r["val"].copy(), r["val_db"].copy()

    v, db = run(buf.data_ptr())
    v2, db2 = run(buf.data_ptr())
    assert np.array_equal(v, v2) and np.array_equal(db, db2)            # deterministic
    pick = sorted({0, 1, S // 2 + 3, S - 1} | {(S * k) // 31 + (7 * k) % 13 for k in range(1, 31)})   # 34 streams: both ends, every wave position
    mid = S // 2 + 3
    for s in pick:
        o = oracle.spectr(buf[s].cpu().numpy(), fs, T)
        assert np.allclose(v[s], o["val"], rtol=1e-4), s
        assert np.allclose(db[s], o["val_db"], atol=1e-3), s
    small = torch.stack([buf[s] for s in pick])
    vs, dbs = run(small.data_ptr(), len(pick))
    assert np.array_equal(vs, v[pick]) and np.array_equal(dbs, db[pick])
    buf.mul_(2.0)
    torch.cuda.synchronize()
    _, db4 = run(buf.data_ptr())
    assert np.allclose(db4, db + 20 * np.log10(2.0), atol=1e-4)
