"""k_bank, the 30-band 1/3-octave bank (MTR_METER_SPECTR30), against the oracle's call-by-call handle: call cuts at the kernel's
chunk edges, how (stream, band) lanes pack into waves, the two controls, non-finite input, levels from silence to 1e15, rates
from 8 kHz to 192 kHz (and the bands that do not exist below 35 650 Hz), the device path on padded and offset buffers, the state
blob's speed.

The contract, everywhere below and on ALL streams of a batch:
  * val, max (the linear levels):  rtol = BANK_REL, atol = 1e-30 (tests/_bank.py: the first frames of a stream leave f32 denormals
    in max, which the GPU may flush; -100 dB is 5e-11).
  * val_db, max_db:  1e-3 dB where the oracle's value is above -90 dB.
  * a band that does not exist at the engine's rate (tests/_bank.band_exists) is silent on any input: both dB values exactly
    -100.0, val and max finite and < 1e-18 — the oracle restates the reference, which asserts there, so it has no say.
All inputs are seeded LCG noise with a gain of 0.05 .. 0.8 per stream, so every band is signal-dominated and val / max need no
"live band" mask.  tests/test_bank_cpu.py holds the condition under which this comparison sees a one-frame fault at a call's tail.
The worst relative deviation of val and of max that the file met is printed at the end of its run (-s shows it)."""
import numpy as np
import pytest

import _bank as B
import _signals as sig
from test_gpu_parity import M  # noqa: F401  (M: the module fixture)

pytestmark = pytest.mark.gpu

KEYS = ("val", "max", "val_db", "max_db")
WORST = {"val": 0.0, "max": 0.0, "where": {}}
STAT_FLOOR = 1e-25         # the deviation is recorded where the oracle's level is a comfortable f32 normal


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nk_bank against the oracle, worst relative deviation met: val %.3g (%s), max %.3g (%s); BANK_REL = %g"
          % (WORST["val"], WORST["where"].get("val"), WORST["max"], WORST["where"].get("max"), B.BANK_REL))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in KEYS)


def _stack(readings):
    """oracle readings of S streams -> one dict of [S, 30] arrays"""
    return {k: np.stack([r[k] for r in readings]) for k in KEYS}


def _finite(got, what):
    for k in KEYS:
        assert np.isfinite(got[k]).all(), (what, k)


def check(got, want, what, bands=None, peak_db=True):
    """the contract above, on every stream; bands: a [30] mask of the bands to compare (all).  peak_db False: the oracle's
    max_db port is stale (its hold was reset after its last run)."""
    _finite(got, what)
    m = np.ones(B.NBANDS, bool) if bands is None else bands
    for k in ("val", "max"):
        g, w = got[k][:, m].astype(np.float64), want[k][:, m].astype(np.float64)
        big = w > STAT_FLOOR
        if big.any():
            dev = float((np.abs(g - w)[big] / w[big]).max())
            print("%-8s %-46s worst relative deviation %.3g" % (k, what, dev))
            if dev > WORST[k]:
                WORST[k], WORST["where"][k] = dev, what
        assert np.allclose(g, w, rtol=B.BANK_REL, atol=B.BANK_ATOL), (what, k, float(np.abs(g - w).max()))
    for k in ("val_db", "max_db") if peak_db else ("val_db",):
        g, w = got[k][:, m], want[k][:, m]
        live = w > B.DB_FLOOR
        assert np.allclose(g[live], w[live], atol=B.DB_TOL), (what, k, float(np.abs(g[live] - w[live]).max()))


def check_silent(got, bands, what):
    """the bands that do not exist"""
    assert (got["val_db"][:, bands] == -100.0).all() and (got["max_db"][:, bands] == -100.0).all(), (what, got["val_db"][:, bands])
    for k in ("val", "max"):
        assert np.isfinite(got[k][:, bands]).all() and (got[k][:, bands] < 1e-18).all() and (got[k][:, bands] >= 0).all(), (what, k)


def feed(mono, x):
    """[S, T, 2] -> what an engine of that width takes (mono: the left channel)"""
    return np.ascontiguousarray(x[:, :, 0]) if mono else np.ascontiguousarray(x)


def one(mono, x):
    """[T, 2] -> what the oracle handle of that width takes"""
    return np.ascontiguousarray(x[:, 0]) if mono else x


# ---- a. call cuts x lanes -------------------------------------------------------------------------------------------------------

_CUT_REF = {}


def _cut_reference(oracle, mono, s):
    """the oracle's reading after every call of the programme, stream s: computed once, the same whatever the batch's size"""
    if (mono, s) not in _CUT_REF:
        h = oracle.spectr_stream(48000.0, 1 if mono else 2)
        h.set_speed(B.SPEED)
        _CUT_REF[mono, s] = B.run_calls(h, one(mono, B.stream_input(s)), B.CALLS)
    return _CUT_REF[mono, s]


# 1: 34 dead lanes.  3: a stream split across waves.  17: wave 7's fourth row does not exist.  18: it is the last stream's bands
# 0 and 1.  32: the batch ends on a wave's end.  33: one stream past it.
@pytest.mark.parametrize("mono", [False, True], ids=["stereo", "mono"])
@pytest.mark.parametrize("S", [1, 2, 3, 17, 18, 32, 33])
def test_call_cuts_and_lanes(M, oracle, S, mono):  # noqa: F811
    x = feed(mono, np.stack([B.stream_input(s) for s in range(S)]))
    with M.Engine(S, 48000.0, M.METER_SPECTR30, n_channels=1 if mono else 2) as e:
        e.spectr_set_speed(B.SPEED)
        for i, (a, b) in enumerate(zip(B.CUTS[:-1], B.CUTS[1:])):
            e.process(np.ascontiguousarray(x[:, a:b]))
            check(e.spectrum(), _stack([_cut_reference(oracle, mono, s)[i] for s in range(S)]),
                  "cuts S=%d %s call %d (%d frames)" % (S, "mono" if mono else "stereo", i, b - a))


# ---- b. controls ----------------------------------------------------------------------------------------------------------------

PROGRAMME = [("run", 3000), ("speed", 100.0), ("run", 2001), ("reset_peak",), ("run", 777), ("speed", 0.0), ("run", 4000),
             ("speed", 1.0), ("reset_peak",), ("run", 129)]
T_PROGRAMME = sum(st[1] for st in PROGRAMME if st[0] == "run")


def _programme(e, x, handles=None, what=""):
    """PROGRAMME on an engine (and the oracle handles, compared after every step) -> the engine's reading after every step"""
    out, pos, port_fresh = [], 0, True                          # (the oracle's max_db is a port: run () alone writes it)
    for i, st in enumerate(PROGRAMME):
        before = e.spectrum()
        port_fresh = st[0] == "run" or (port_fresh and st[0] == "speed")
        if st[0] == "run":
            e.process(np.ascontiguousarray(x[:, pos:pos + st[1]]))
            if handles:
                for s, h in enumerate(handles):
                    h.run(x[s, pos:pos + st[1]])
            pos += st[1]
        elif st[0] == "speed":
            e.spectr_set_speed(st[1])
            for h in handles or []:
                h.set_speed(st[1])
        else:
            e.spectr_reset_peak()
            for h in handles or []:
                h.reset_peak()
        got = e.spectrum()
        out.append(got)
        if st[0] == "reset_peak":                                # directly after it, before any call
            assert not got["max"].any() and (got["max_db"] == -100.0).all(), (what, i)
            assert np.array_equal(_bits(got["val"]), _bits(before["val"])) and np.array_equal(_bits(got["val_db"]), _bits(before["val_db"]))
        if st[0] == "speed":                                     # a control alone moves nothing
            assert _same(got, before), (what, i)
        if handles:
            check(got, _stack([h.read() for h in handles]), "%s step %d %s" % (what, i, st), peak_db=port_fresh)
    return out


def test_controls(M, oracle):  # noqa: F811
    S = 3
    x = np.stack([B.stream_input(s, T_PROGRAMME, 7300) for s in range(S)])
    with M.Engine(S, 48000.0, M.METER_SPECTR30) as e:
        first = _programme(e, x, [oracle.spectr_stream(48000.0) for _ in range(S)], "controls")
        # speed is a control: mtr_engine_reset zeroes the bank's state and leaves the speed (here the programme's last, 1.0)
        e.reset()
        r = e.spectrum()
        assert not r["val"].any() and not r["max"].any()
        again = _programme(e, x)
    with M.Engine(S, 48000.0, M.METER_SPECTR30) as f:
        f.spectr_set_speed(1.0)
        fresh = _programme(f, x)
    for a, b, c in zip(first, again, fresh):
        assert _same(a, c) and _same(b, c)


def test_speed_survives_reset(M):  # noqa: F811
    """... seen at a speed that is not the default: reset, then audio, equals a fresh engine at that speed bit for bit — and not
    one at the default"""
    S = 3
    x = np.stack([B.stream_input(s, 1500, 7400) for s in range(S)])
    with M.Engine(S, 48000.0, M.METER_SPECTR30) as e, M.Engine(S, 48000.0, M.METER_SPECTR30) as f, \
            M.Engine(S, 48000.0, M.METER_SPECTR30) as d:
        e.spectr_set_speed(7.5)
        e.process(x[:, :700])
        e.reset()
        e.process(x)
        f.spectr_set_speed(7.5)
        f.process(x)
        d.process(x)
        assert _same(e.spectrum(), f.spectrum())
        assert not np.array_equal(e.spectrum()["val"], d.spectrum()["val"])


@pytest.mark.parametrize("outside,edge", [(100.0, 15.0), (0.0, 0.01), (-1.0, 0.01)])
def test_speed_clamps(M, oracle, outside, edge):  # noqa: F811
    S = 3
    x = np.stack([B.stream_input(s, 1300, 7500) for s in range(S)])
    with M.Engine(S, 48000.0, M.METER_SPECTR30) as e, M.Engine(S, 48000.0, M.METER_SPECTR30) as f:
        e.spectr_set_speed(outside)
        f.spectr_set_speed(edge)
        for a, b in ((0, 301), (301, 1300)):
            e.process(x[:, a:b])
            f.process(x[:, a:b])
            assert _same(e.spectrum(), f.spectrum())
        hs = [oracle.spectr_stream(48000.0) for _ in range(S)]
        for s, h in enumerate(hs):
            h.set_speed(edge)
            B.run_calls(h, x[s], [301, 999])
        check(e.spectrum(), _stack([h.read() for h in hs]), "speed %g" % outside)


# ---- c. non-finite input --------------------------------------------------------------------------------------------------------

def test_non_finite_input(M, oracle):  # noqa: F811
    S, calls = 5, [2000, 2000, 1, 3999]
    cuts = np.concatenate([[0], np.cumsum(calls)])
    x = np.stack([B.stream_input(s, int(cuts[-1]), 7600) for s in range(S)])
    c2 = int(cuts[1])
    x[0, c2 + 500, 0] = np.nan                                   # NaN in L
    x[1, c2 + 500, :] = np.inf                                   # +Inf
    x[2, int(cuts[2]) - 1, 1] = -np.inf                          # -Inf in R at the call's last frame
    x[3, c2, :] = np.nan                                         # NaN at the call's first frame
    hs = [oracle.spectr_stream(48000.0) for _ in range(S)]
    tiny = np.float32(1e-20)
    with M.Engine(S, 48000.0, M.METER_SPECTR30) as e:
        for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
            e.process(np.ascontiguousarray(x[:, a:b]))
            want = _stack([h.run(x[s, a:b]) for s, h in enumerate(hs)])
            got = e.spectrum()
            check(got, want, "non-finite call %d" % i)           # (no NaN / Inf ever leaves the getter: check () asserts it)
            if i == 0:
                held = got["max"].copy()
            if i == 1:
                # the epilogue's scrub (spectrumlv2.c:230-238): a non-finite level is 0 + 1e-20f.  A NaN loses every compare and
                # leaves the hold alone; an Inf wins one, and the scrub zeroes the hold
                assert (got["val"][:4] == tiny).all() and (want["val"][:4] == tiny).all()
                assert (got["max"][[0, 3]] > 0).all() and (got["max"][3] == held[3]).all() and (got["max"][0] >= held[0]).all()
                assert not got["max"][[1, 2]].any() and not want["max"][[1, 2]].any()
                assert (got["val_db"][:4] == -100.0).all() and (got["max_db"][[1, 2]] == -100.0).all()
                assert (got["val"][4] > 1e3 * tiny).all()                 # (the clean stream beside them was not scrubbed)
    # stream 4 as if it were alone
    alone = oracle.spectr_stream(48000.0)
    assert _same(B.run_calls(alone, x[4], calls)[-1], hs[4].read())


# ---- d. levels ------------------------------------------------------------------------------------------------------------------

SILENCE_CALLS = [64] * 10 + [1, 3, 4800]


def _through(M, x, calls, fs=48000.0, speed=None, mono=False):  # noqa: F811  (the fixture's value, handed on)
    with M.Engine(x.shape[0], fs, M.METER_SPECTR30, n_channels=1 if mono else 2) as e:
        if speed is not None:
            e.spectr_set_speed(speed)
        out, pos = [], 0
        for n in calls:
            e.process(np.ascontiguousarray(x[:, pos:pos + n]))
            out.append(e.spectrum())
            pos += n
        return out


def _oracle_through(oracle, x, calls, fs=48000.0, speed=None, mono=False):
    hs = [oracle.spectr_stream(fs, 1 if mono else 2) for _ in range(x.shape[0])]
    for h in hs:
        if speed is not None:
            h.set_speed(speed)
    per = [B.run_calls(h, x[s], calls) for s, h in enumerate(hs)]
    return [_stack([per[s][i] for s in range(x.shape[0])]) for i in range(len(calls))]


def test_silence_and_cancelling_channels(M, oracle):  # noqa: F811
    """silence: only the anti-denormal dither and the epilogue's + 1e-20f per call move the levels (7.203e-20 after these 13
    calls); L = -R: the mix is exactly 0, so the same bits"""
    T = sum(SILENCE_CALLS)
    zero = np.zeros((2, T, 2), np.float32)
    n = np.stack([B.stream_input(s, T, 7700) for s in range(2)])
    anti = np.stack([n[..., 0], -n[..., 0]], -1)
    got, want = _through(M, zero, SILENCE_CALLS), _oracle_through(oracle, zero, SILENCE_CALLS)
    for i, (g, w) in enumerate(zip(got, want)):
        check(g, w, "silence call %d" % i)
        assert (g["val_db"] == -100.0).all() and (g["max_db"] == -100.0).all()
    assert np.allclose(want[-1]["val"], 7.203e-20, rtol=1e-3)
    for g, a in zip(got, _through(M, anti, SILENCE_CALLS)):
        assert _same(g, a)


@pytest.mark.parametrize("scale", [1e-30, 1e-6, 1e15])
def test_levels(M, oracle, scale):  # noqa: F811
    x = np.stack([B.stream_input(s, 3000, 7800) for s in range(3)]) * np.float32(scale)
    calls = [3000] if scale == 1e-30 else [1001, 1999]
    got, want = _through(M, x, calls), _oracle_through(oracle, x, calls)
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.isfinite(w["val"]).all() and np.isfinite(w["max"]).all()
        check(g, w, "scale %g call %d" % (scale, i))
    if scale == 1e-30:                                          # the signal's square underflows: the level is the epilogue's constant
        assert (got[0]["val"] == np.float32(1e-20)).all() and (want[0]["val"] == np.float32(1e-20)).all()


# ---- e. rates -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("speed", [15.0, 1.0])
@pytest.mark.parametrize("fs", [44100.0, 88200.0, 96000.0, 176400.0, 192000.0])     # 44.1 kHz: band 29's upper edge is clamped to Nyquist
def test_rates(M, oracle, fs, speed):  # noqa: F811
    assert B.existing(fs).all()
    x = np.stack([B.stream_input(s, 2500, 7900) for s in range(2)])
    calls = [1501, 999]
    for i, (g, w) in enumerate(zip(_through(M, x, calls, fs, speed), _oracle_through(oracle, x, calls, fs, speed))):
        check(g, w, "rate %g speed %g call %d" % (fs, speed, i))


@pytest.mark.parametrize("fs", [32000.0, 22050.0, 16000.0, 11025.0, 8000.0])
def test_low_rates_have_no_phantom_bands(M, oracle, fs):  # noqa: F811
    """Below 35 650 Hz the top bands' lower edges lie at or above Nyquist: the reference asserts (src/spectr.c:134), and computing
    on regardless gave NaN coefficients (-100 dB only thanks to the scrub) or finite garbage: levels of -11 .. -18 dB in bands
    26, 27, 29 at 8 kHz, 27 and 28 at 11.025 kHz, 29 at 16 kHz.  Such a band is silent; the others are the oracle's.  The third
    call carries a NaN and an Inf frame: silent on ANY input."""
    ex = B.existing(fs)
    assert not ex.all() and ex[:23].all()
    x = np.stack([sig.lcg_noise(7000, 8000 + s, 0.5) for s in range(2)])
    x[0, 6200, 0] = np.nan
    x[1, 6300, :] = np.inf
    calls = [3001, 2999, 1000]
    for i, (g, w) in enumerate(zip(_through(M, x, calls, fs), _oracle_through(oracle, x, calls, fs))):
        _finite(g, fs)
        check_silent(g, ~ex, "rate %g call %d" % (fs, i))
        check(g, w, "rate %g call %d" % (fs, i), bands=ex)


# ---- f. the device path ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mono", [False, True], ids=["stereo", "mono"])
def test_device_buffers_with_padding_and_offset(M, oracle, mono):  # noqa: F811
    """process_device on [S = 18][stride = 391] frames of which 385 are audio, the padding NaN, the base one frame (stereo: 8 bytes,
    mono: 4 bytes, with an odd stride: rows on 4 bytes) past the allocation's start — two such calls and a run-out; equal to the
    oracle, and to the host path on the same frames bit for bit"""
    import torch
    S, n, stride, W = 18, 385, 391, 1 if mono else 2
    calls = [n, n, 300]
    x = feed(mono, np.stack([B.stream_input(s, sum(calls), 8100) for s in range(S)]))
    st = torch.cuda.current_stream().cuda_stream
    keep = []
    with M.Engine(S, 48000.0, M.METER_SPECTR30, n_channels=W) as e, M.Engine(S, 48000.0, M.METER_SPECTR30, n_channels=W) as h:
        e.spectr_set_speed(B.SPEED)
        h.spectr_set_speed(B.SPEED)
        want = _oracle_through(oracle, x, calls, speed=B.SPEED, mono=mono)
        pos = 0
        for i, m in enumerate(calls):
            pad = np.full((1 + S * stride) * W, np.nan, np.float32)
            rows = pad[W:].reshape(S, stride, W) if not mono else pad[W:].reshape(S, stride)
            rows[:, :m] = x[:, pos:pos + m]
            d = torch.from_numpy(pad).cuda()
            keep.append(d)
            e.process_device(d.data_ptr() + 4 * W, m, stride, st)
            h.process(np.ascontiguousarray(x[:, pos:pos + m]))
            pos += m
            got = e.spectrum()
            check(got, want[i], "device %s call %d" % ("mono" if mono else "stereo", i))
            assert _same(got, h.spectrum())
        e.sync()


# ---- g. state -------------------------------------------------------------------------------------------------------------------

def test_the_blobs_speed_wins(M):  # noqa: F811
    S = 3
    x = np.stack([B.stream_input(s, 2000, 8200) for s in range(S)])
    mk = lambda: M.Engine(S, 48000.0, M.METER_SPECTR30)          # noqa: E731
    with mk() as a, mk() as b, mk() as c, mk() as d:
        a.spectr_set_speed(7.5)
        a.process(x[:, :777])
        blob = a.state_export()
        b.spectr_set_speed(3.0)                                  # a fresh engine takes the blob's speed, whatever the setter said before
        b.state_import(blob)
        assert _same(a.spectrum(), b.spectrum())
        for p, q in ((777, 778), (778, 1291), (1291, 2000)):
            a.process(x[:, p:q])
            b.process(x[:, p:q])
            assert _same(a.spectrum(), b.spectrum())
        c.spectr_set_speed(3.0)                                  # one that has processed at another speed does not stand there
        c.process(x[:, :777])
        with pytest.raises(M.EngineError) as ei:
            c.state_import(blob)
        assert ei.value.code == M.engine.ERR_STATE
        d.spectr_set_speed(7.5)                                  # ... and at the same speed it does
        d.process(x[:, :777])
        d.state_import(blob)
