"""The 30-band bank without a GPU: the oracle's call-by-call handle (what tests/test_gpu_bank.py compares the engine with), the
speed control's arithmetic, the bands that do not exist at low rates (mtr_band_coef is host arithmetic), and the condition under
which the GPU comparison can see a one-frame fault at a call's tail at all."""
import numpy as np
import pytest

import _bank as B
import _signals as sig


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same(a, b):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in ("val", "max", "val_db", "max_db"))


GOLDEN_INPUTS = [("lcg 48k", 48000.0, lambda: sig.lcg_noise(48000, 42, 0.5)),
                 ("band 16 sine", 48000.0, lambda: sig.g4(48000 * 2, 16)),
                 ("lcg 44k1", 44100.0, lambda: sig.lcg_noise(44100, 43, 0.5))]


@pytest.mark.parametrize("name,fs,make", GOLDEN_INPUTS, ids=[g[0] for g in GOLDEN_INPUTS])
def test_handle_equals_batch_oracle(oracle, name, fs, make):
    """default speed, no reset, blocks of 1024: the handle is mo_batch_spectr (held against the reference) bit for bit"""
    x = make()
    h = oracle.spectr_stream(fs)
    r = B.run_calls(h, x, [1024] * (len(x) // 1024) + ([len(x) % 1024] if len(x) % 1024 else []))[-1]
    assert _same(r, oracle.spectr(x, fs, 1024))
    assert _same(r, h.read())


def test_mono_handle_equals_stereo_fed_twice(oracle):
    x = B.stream_input(5)
    m = np.ascontiguousarray(x[:, 0])
    a, b, c = oracle.spectr_stream(48000.0, 1), oracle.spectr_stream(48000.0, 2), oracle.spectr_stream(48000.0, 2)
    for ra, rb, rc in zip(B.run_calls(a, m, B.CALLS), B.run_calls(b, np.stack([m, m], 1), B.CALLS), B.run_calls(c, m, B.CALLS)):
        assert _same(ra, rb) and _same(ra, rc)               # (L + L) / 2 = L exactly
    with pytest.raises(ValueError):
        a.run(x)


ULP = 2.0 ** -24           # of expf's value in [0.5, 1): omega = 1.0f - expf (..) is a multiple of it, so this is ITS resolution


def _omega(v, fs):
    """spectrumlv2.c:170-177 in numpy: the clamp, the exponent in double, expf and the subtraction in float.  expf is the
    double exp of the float argument, rounded (numpy's own float32 exp is a vector routine good to 2.5 ulp only)."""
    v = min(max(float(np.float32(v)), 0.01), 15.0)
    return np.float32(1.0) - np.float32(np.exp(np.float64(np.float32(-2.0 * np.pi * v / fs))))


@pytest.mark.parametrize("fs", [8000.0, 44100.0, 48000.0, 192000.0])
def test_speed_sets_omega(oracle, fs):
    h = oracle.spectr_stream(fs)
    assert abs(float(h.omega) - float(_omega(1.0, fs))) <= ULP     # spectrumlv2.c:98: speed 1 at start
    for v in (0.01, 0.25, 1.0, 7.5, 15.0, 0.0, -3.0, 100.0, 15.0001):
        h.set_speed(v)
        want = _omega(v, fs)
        assert 0 < h.omega < 1 and abs(float(h.omega) - float(want)) <= ULP, (fs, v, h.omega, want)
        assert float(h.omega) / ULP == round(float(h.omega) / ULP)
    h.set_speed(100.0); a = h.omega
    h.set_speed(15.0); assert _bits(a) == _bits(h.omega)
    h.set_speed(0.0); a = h.omega
    h.set_speed(0.01); assert _bits(a) == _bits(h.omega)


def test_speed_and_peak_reset_act_on_the_levels(oracle):
    x = B.stream_input(3, 3000)
    a, b, c = (oracle.spectr_stream(48000.0) for _ in range(3))
    a.set_speed(100.0); b.set_speed(15.0)
    ra, rb, rc = a.run(x), b.run(x), c.run(x)
    assert _same(ra, rb) and not np.array_equal(ra["val"], rc["val"])
    b.reset_peak()
    r = b.read()
    assert not r["max"].any() and np.array_equal(_bits(r["val"]), _bits(rb["val"]))
    r = b.run(x[:1])
    assert np.array_equal(r["max"], r["val"]) and (r["val"] > 1e-12).all()           # the hold starts again from the level


# ---- bands that do not exist -----------------------------------------------------------------------------------------------------

LOW_RATES = [8000.0, 11025.0, 16000.0, 22050.0, 32000.0]


def test_which_bands_exist():
    """the lower edge f_m - bw / 2 = 0.88422 f_m below Nyquist: band 29 (f_m = 20 158.7 Hz) from 35 650 Hz on"""
    assert [int((~B.existing(fs)).sum()) for fs in LOW_RATES] == [7, 6, 4, 3, 1]
    assert not B.band_exists(35649.0, 29) and B.existing(35650.0).all() and B.existing(44100.0).all()
    for fs in LOW_RATES:                                      # (the bands that are missing are the top ones)
        ex = B.existing(fs)
        assert ex[:int(ex.sum())].all()


@pytest.mark.parametrize("fs", LOW_RATES + [35649.0, 35650.0, 44100.0, 192000.0])
def test_band_coefficients_below_the_full_rate(oracle, fs):
    """mtr_band_coef: a band that exists has the oracle's coefficients; one that does not (the reference's failed assert
    (wu > wl), src/spectr.c:134) is silent — section 0's gain 0, no poles — and MTR_OK.  Nothing is ever non-finite."""
    import meters.lv2_amd as M
    for b in range(B.NBANDS):
        w = M.band_coef(fs, b)
        assert np.isfinite(w).all(), (fs, b)
        assert (w[:, 0] == 1).all()
        if B.band_exists(fs, b):
            assert np.allclose(w, oracle.band_coef(fs, b), rtol=1e-12, atol=0), (fs, b)
            assert w[0, 3] > 0 and (np.abs(w[:, 2]) < 1).all()                   # a gain, and poles inside the unit circle
        else:
            assert not w[0, 3:].any() and not w[:, 1:3].any(), (fs, b, w)


def test_a_silent_band_stays_silent_in_the_section_arithmetic():
    """the kernel's recurrence (transposed direct form II, section 0 carrying the gain) on a silent band's coefficients: 0 out
    for any finite input, and no state ever moves"""
    import meters.lv2_amd as M
    w = M.band_coef(8000.0, 29)
    z = np.zeros((6, 2))
    for x in (0.7, -1e15, 1e-12, 3e38):
        out = x
        for i in range(6):
            y = w[i, 3] * out + z[i, 0]
            z[i, 0] = w[i, 4] * out + z[i, 1] - w[i, 1] * y
            z[i, 1] = w[i, 5] * out - w[i, 2] * y
            out = y
        assert out == 0 and not z.any()


# ---- what the GPU comparison can see ----------------------------------------------------------------------------------------------

def _readings(oracle, x, mono):
    h = oracle.spectr_stream(48000.0, 1 if mono else 2)
    h.set_speed(B.SPEED)
    return np.stack([r["val"] for r in B.run_calls(h, x, B.CALLS)]).astype(np.float64)


@pytest.mark.parametrize("mono", [False, True], ids=["stereo", "mono"])
@pytest.mark.parametrize("fault", [B.slip, B.stale], ids=["slip", "stale"])
def test_the_comparison_sees_a_one_frame_fault(oracle, fault, mono):
    """The condition tests/test_gpu_bank.py's call-cut test rests on: with its inputs, its calls and a reading after every call,
    each of these one-frame faults moves at least one band of the oracle's val by >= 10 x BANK_REL in at least one reading —
    so an engine that made the fault could not pass.  (At the default speed a frame weighs 1.3e-4 of val and the 12 poles'
    delay hides the last frames of a call: hence speed 15 and the run-out call.)  Stream 0 is in every batch, the smallest
    included; the others are held to the same."""
    for s in (0, 16, 32):
        x = B.stream_input(s)
        x = np.ascontiguousarray(x[:, 0]) if mono else x
        base = _readings(oracle, x, mono)
        for k in B.FAULT_FRAMES:
            moved = (np.abs(_readings(oracle, fault(x, k), mono) - base) / base).max()
            assert moved >= 10 * B.BANK_REL, (s, k, moved)
