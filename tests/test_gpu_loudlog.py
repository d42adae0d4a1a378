"""The loudness log (mtr_engine_loudlog_*: a (M, S) point per period of P fragments and stream) on the GPU.

The yardstick is the oracle fed fragment by fragment: Oracle.ebu_stream (fs).process on consecutive blocks of one fragment, whose
out9[0] / out9[2] after each block are that fragment's M and S.  A MTR_LOUDLOG_SAMPLE point is the value after the period's last
fragment, a MTR_LOUDLOG_MAX point the maximum over the period's fragments.  Against the oracle the bound is the project's DB_TOL = 1e-3 dB
(tests/test_gpu_parity.py), a stream of zeros must give exactly -200.0; one long call against many short ones 1e-4 dB (the bound of
test_streaming_calls_equal_one_call there); every other comparison (against the engine's own getters, between two routes of the same
call) is of bit patterns."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DB_TOL = 1e-3
CUTS = [5000, 1, 2399, 40000]                      # ... and the rest
_REF = {}


@pytest.fixture(scope="module")
def M():
    import meters.lv2_amd as m
    return m


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def noise(S, T, seed, levels=(0.3, 0.03, 0.003)):
    """Gaussian noise streams at the given levels (cycled), stereo"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((S, T, 2)).astype(np.float32)
    for s in range(S):
        x[s] *= np.float32(levels[s % len(levels)])
    return x


def short_batch(fs):
    """three noise streams and one of zeros, 37 fragments and 1000 frames"""
    key = ("short", fs)
    if key not in _REF:
        T = 37 * (int(fs) // 20) + 1000
        x = noise(4, T, 4100 + int(fs))
        x[3] = 0
        x.setflags(write=False)
        _REF[key] = x
    return _REF[key]


def frag_ms(oracle, key, x, fs):
    """(M [nf], S [nf]) of one stereo stream x [T, 2], the oracle fed fragment by fragment; computed once per key"""
    if key not in _REF:
        fr = int(fs) // 20
        nf = x.shape[0] // fr
        st = oracle.ebu_stream(fs)
        m, s = np.zeros(nf, np.float32), np.zeros(nf, np.float32)
        for k in range(nf):
            o9 = st.process(x[k * fr:(k + 1) * fr, 0], x[k * fr:(k + 1) * fr, 1], with_tp=False)[0]
            m[k], s[k] = o9[0], o9[2]
        m.setflags(write=False)
        s.setflags(write=False)
        _REF[key] = (m, s)
    return _REF[key]


def points_of(v, P, mode, n=None):
    """the points of per-fragment values v"""
    n = v.size // P if n is None else n
    return v[P - 1:n * P:P] if mode == 0 else v[:n * P].reshape(n, P).max(axis=1)


def spans(T, cuts):
    out, a = [], 0
    for c in cuts:
        out.append((a, a + c))
        a += c
    if a < T:
        out.append((a, T))
    return out


def feed(e, x, cuts, each=None):
    """x [S, T, C] through process_device call by call; each (e, frames so far) after every call"""
    keep = []
    for a, b in spans(x.shape[1], cuts):
        d = torch.from_numpy(np.array(x[:, a:b])).cuda()                # (a writable copy)
        keep.append(d)
        e.process_device(d.data_ptr(), b - a)
        if each:
            each(e, b)
    e.sync()


def check_against_oracle(oracle, name, x, fs, got, P, mode, n_want=None):
    Mg, Sg, n, d = got
    for s in range(x.shape[0]):
        m, v = frag_ms(oracle, (name, fs, s), x[s], fs)
        want = m.size // P if n_want is None else n_want[s]
        assert n[s] == want and d[s] == 0, (s, n, d)
        wm, ws = points_of(m, P, mode, want), points_of(v, P, mode, want)
        em, es = np.abs(Mg[s, :want] - wm).max(initial=0), np.abs(Sg[s, :want] - ws).max(initial=0)
        print(f"{name} fs {fs} P {P} mode {mode} stream {s}: {want} points, max |dM| {em:.2e} |dS| {es:.2e} dB")
        assert em <= DB_TOL and es <= DB_TOL, (s, em, es)
        assert np.isnan(Mg[s, want:]).all() and np.isnan(Sg[s, want:]).all()
        if not x[s].any():
            assert (Mg[s, :want] == -200.0).all() and (Sg[s, :want] == -200.0).all()


# ---- 1. the short path (k_gate) -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("fs,P", [(48000.0, 1), (48000.0, 3), (48000.0, 10), (44100.0, 2)])
def test_short_calls_against_the_oracle(M, oracle, fs, P, mode):
    x = short_batch(fs)
    with M.Engine(4, fs) as e:
        e.loudlog_set_period(P, 64, mode)
        assert e.loudlog_period() == (P, 64, mode)
        feed(e, x, CUTS)
        got = e.loudlog_series()
    assert got[0].shape == (4, 64) and got[2].dtype == np.uint32
    check_against_oracle(oracle, "short", x, fs, got, P, mode)


# ---- 2. the same bits as the getters ------------------------------------------------------------------------------------------

def test_sample_points_are_the_getters_values(M):
    x = short_batch(48000.0)
    seen = []

    def each(e, frames):
        n = frames // 2400
        if seen and seen[-1] == n:
            return                                   # (the call ended no fragment)
        seen.append(n)
        Mg, Sg, np_, _ = e.loudlog_series()
        r = e.results()
        assert (np_ == n).all()
        for s in range(4):
            assert _bits(Mg[s, n - 1]) == _bits(r[s].loudness_M) and _bits(Sg[s, n - 1]) == _bits(r[s].loudness_S), (s, n)
    with M.Engine(4, 48000.0) as e:
        e.loudlog_set_period(1, 64, M.LOUDLOG_SAMPLE)
        feed(e, x, CUTS, each)
    assert seen == [2, 3, 19, 37]


def test_max_points_hold_the_maxima_of_the_getters(M):
    x = short_batch(48000.0)
    with M.Engine(4, 48000.0) as e:
        e.loudlog_set_period(1, 64, M.LOUDLOG_MAX)
        feed(e, x, CUTS)
        Mg, Sg, n, _ = e.loudlog_series()
        r = e.results()
    assert (n == 37).all()
    for s in range(4):
        assert _bits(Mg[s, :37].max()) == _bits(r[s].maxloudn_M) and _bits(Sg[s, :37].max()) == _bits(r[s].maxloudn_S), s


# ---- 3. the long path (k_gate_frag + k_gate_final) --------------------------------------------------------------------------

def long_batch():
    if "long" not in _REF:
        x = noise(2, 4107 * 400 + 123, 8000, levels=(0.2, 0.01))
        # (levels that move: a maximum over a period is then not its last value)
        x *= (0.55 + 0.45 * np.sin(np.arange(x.shape[1]) * (2 * np.pi / 9000.0))).astype(np.float32)[None, :, None]
        x.setflags(write=False)
        _REF["long"] = x
    return _REF["long"]


# P = 7: periods straddle the 1024-fragment blocks of the workgroups (and the 256-fragment chunks of k_gate); 1500: a period holds a whole block
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("P", [1, 7, 1500])
def test_one_long_call(M, oracle, P, mode):
    fs, x = 8000.0, long_batch()
    cap = 4107 // P
    got = {}
    # (mixed: a short call, a long one that begins and ends inside a period of 7, a short one — the open period's maxima change hands twice)
    for name, cuts in (("one", []), ("100", [100 * 400] * 41), ("1000", [1000 * 400] * 4), ("mixed", [5 * 400, 4096 * 400])):
        with M.Engine(2, fs) as e:
            e.loudlog_set_period(P, cap, mode)
            feed(e, x, cuts)
            got[name] = e.loudlog_series()
    for name in got:
        check_against_oracle(oracle, "long", x, fs, got[name], P, mode)
    for name in ("100", "1000", "mixed"):
        for k in (0, 1):
            err = np.abs(got["one"][k] - got[name][k]).max()
            print(f"one call against calls of {name} fragments, P {P} mode {mode}: max |d{'MS'[k]}| {err:.2e} dB")
            assert err <= 1e-4, (name, k, err)


@pytest.mark.parametrize("mode", [0, 1])
def test_one_long_call_with_lengths(M, oracle, mode):
    """the LEN instantiations of the long path: a stream that ends inside the call, inside a block and inside a period"""
    fs, P = 8000.0, 7
    x = np.concatenate([long_batch(), np.zeros((1,) + long_batch().shape[1:], np.float32)])
    T = x.shape[1]
    frames = np.array([T, 2500 * 400 + 50, 0], np.uint64)
    with M.Engine(3, fs) as e:
        e.loudlog_set_period(P, 600, mode)
        d = torch.from_numpy(x).cuda()
        e.process_device_lengths(d.data_ptr(), T, frames)
        got = e.loudlog_series()
    assert got[2].tolist() == [4107 // 7, 2500 // 7, 0] and not got[3].any()
    check_against_oracle(oracle, "long", x[:2], fs, tuple(g[:2] for g in got), P, mode, n_want=[4107 // 7, 2500 // 7])
    assert np.isnan(got[0][2]).all() and np.isnan(got[1][2]).all()


# ---- 4. per-stream lengths ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [0, 1])
def test_lengths(M, oracle, mode):
    fs, n, P = 48000.0, 20 * 2400, 2
    frames = np.array([n, 7 * 2400 + 100, 0, 3 * 2400, 2399], np.uint64)
    key = ("lengths",)
    if key not in _REF:
        x = noise(5, 2 * n, 77)
        x.setflags(write=False)
        _REF[key] = x
    x = _REF[key]
    with M.Engine(5, fs) as e:
        e.loudlog_set_period(P, 32, mode)
        d = torch.from_numpy(np.ascontiguousarray(x[:, :n])).cuda()
        e.process_device_lengths(d.data_ptr(), n, frames)
        first = e.loudlog_series()
        d2 = torch.from_numpy(np.ascontiguousarray(x[:, n:])).cuda()
        e.process_device(d2.data_ptr(), n)
        second = e.loudlog_series()
    assert first[2].tolist() == [10, 3, 0, 1, 0] and not first[3].any()
    for s in (1, 3):                                                              # (the oracle sees a stream's own whole fragments)
        m, v = frag_ms(oracle, ("lengths", s), x[s, :int(frames[s]) // 2400 * 2400], fs)
        k = int(first[2][s])
        assert np.abs(first[0][s, :k] - points_of(m, P, mode, k)).max() <= DB_TOL
        assert np.abs(first[1][s, :k] - points_of(v, P, mode, k)).max() <= DB_TOL
    m, v = frag_ms(oracle, ("lengths", 0), x[0], fs)
    assert second[2].tolist() == [20, 3, 0, 1, 0] and not second[3].any()
    assert np.abs(second[0][0, :20] - points_of(m, P, mode, 20)).max() <= DB_TOL
    assert np.abs(second[1][0, :20] - points_of(v, P, mode, 20)).max() <= DB_TOL
    for k in (0, 1):
        assert np.array_equal(_bits(first[k][1:]), _bits(second[k][1:]))          # (NaN rows included: bit patterns)
        assert np.array_equal(_bits(first[k][0, :10]), _bits(second[k][0, :10]))


# ---- 5. the deferred tail ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [0, 1])
def test_deferred_tail_appends_the_same_bits(M, mode):
    x = short_batch(48000.0)[:3]
    got = []
    for tail in (1, 2):
        with M.Engine(3, 48000.0) as e:
            e.set_deferred_tail(tail)
            e.loudlog_set_period(3, 16, mode)
            feed(e, x, [30000, 5000])
            got.append(e.loudlog_series() + (e.deferred_calls(),))
    assert got[0][4] == 0 and got[1][4] == 3
    assert (got[0][2] == 12).all()
    for k in range(4):
        assert np.array_equal(got[0][k].view(np.uint32), got[1][k].view(np.uint32)), k


# ---- 6. host and PCM paths --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [0, 1])
def test_chunked_host_call_against_device_call(M, mode):
    T = 9 * 2400 + 700
    key = ("host",)
    if key not in _REF:
        _REF[key] = noise(5, T, 99)
    x = _REF[key]
    got = []
    for host in (False, True):
        with M.Engine(5, 48000.0) as e:
            e.loudlog_set_period(2, 8, mode)
            if host:
                for part in (x[:, :5000], x[:, 5000:]):
                    e.set_host_chunk_bytes(2 * part.shape[1] * 8)                 # two streams: the batch goes in chunks of 2, 2, 1
                    e.process(part)
            else:
                feed(e, x, [5000])
            got.append(e.loudlog_series())
    assert (got[0][2] == 4).all()
    for k in range(4):
        assert np.array_equal(got[0][k].view(np.uint32), got[1][k].view(np.uint32)), k


def test_pcm_against_decoded_floats(M):
    rng = np.random.default_rng(5)
    pcm = rng.integers(-9000, 9000, (3, 5 * 2400 + 11, 2)).astype(np.int16)
    got = []
    for as_pcm in (True, False):
        with M.Engine(3, 48000.0) as e:
            e.loudlog_set_period(1, 8, M.LOUDLOG_MAX)
            if as_pcm:
                e.process_pcm(pcm)
            else:
                e.process(M.pcm_decode(M.PCM_S16, pcm))
            got.append(e.loudlog_series())
    assert (got[0][2] == 5).all()
    for k in range(4):
        assert np.array_equal(got[0][k].view(np.uint32), got[1][k].view(np.uint32)), k


# ---- 7. five channels --------------------------------------------------------------------------------------------------------------

def test_five_channels(M):
    rng = np.random.default_rng(6)
    x = (rng.standard_normal((2, 7 * 2400 + 500, 5)) * 0.1).astype(np.float32)
    seen = []

    def each(e, frames):
        n = frames // 2400
        Mg, Sg, np_, d = e.loudlog_series()
        r = e.results()
        assert (np_ == n).all() and not d.any()
        seen.append(n)
        for s in range(2):
            assert _bits(Mg[s, n - 1]) == _bits(r[s].loudness_M) and _bits(Sg[s, n - 1]) == _bits(r[s].loudness_S), (s, n)
    with M.Engine(2, 48000.0, n_channels=5) as e:
        assert e.layout() == 8
        e.loudlog_set_period(1, 8, M.LOUDLOG_SAMPLE)
        feed(e, x, [3 * 2400 + 1000], each)
    assert seen == [3, 7]


# ---- 8. capacity and lifecycle --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [0, 1])
def test_capacity_drops_and_counts(M, oracle, mode):
    x = short_batch(48000.0)
    with M.Engine(4, 48000.0) as e:
        e.loudlog_set_period(1, 4, mode)
        feed(e, x[:, :10 * 2400 + 5], [7000])
        Mg, Sg, n, d = e.loudlog_series()
    assert Mg.shape == (4, 4) and (n == 10).all() and (d == 6).all()
    for s in range(4):
        m, v = frag_ms(oracle, ("short", 48000.0, s), x[s], 48000.0)
        assert np.abs(Mg[s] - m[:4]).max() <= DB_TOL and np.abs(Sg[s] - v[:4]).max() <= DB_TOL


def test_resets(M):
    x = short_batch(48000.0)[:, :12 * 2400 + 77]
    with M.Engine(4, 48000.0) as e:
        e.loudlog_set_period(5, 8, M.LOUDLOG_MAX)
        e.integr_start()
        feed(e, x, [3000])
        a = e.loudlog_series()
        assert (a[2] == 2).all()
        e.integr_reset()
        b = e.loudlog_series()
        for k in range(4):
            assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32))
        e.loudlog_reset()
        c = e.loudlog_series()
        assert not c[2].any() and not c[3].any() and np.isnan(c[0]).all() and e.loudlog_period() == (5, 8, M.LOUDLOG_MAX)
        e.reset()
        assert e.loudlog_period() == (5, 8, M.LOUDLOG_MAX) and not e.loudlog_series()[2].any()
        feed(e, x, [3000])                                                        # from reset: the same series again, phase and maxima emptied
        d = e.loudlog_series()
        for k in range(4):
            assert np.array_equal(a[k].view(np.uint32), d[k].view(np.uint32))


def test_set_period_rules(M):
    E = M.engine
    x = short_batch(48000.0)[:, :3 * 2400]

    def code(f, *a):
        with pytest.raises(M.EngineError) as err:
            f(*a)
        return err.value.code
    with M.Engine(4, 48000.0) as e:
        assert e.loudlog_period()[0] == 0
        assert code(e.loudlog_series) == E.ERR_ARG                                # off is the default
        assert code(e.loudlog_set_period, 1, 8, 2) == E.ERR_ARG
        assert code(e.loudlog_set_period, (1 << 20) + 1, 8, 0) == E.ERR_ARG
        e.loudlog_set_period(1 << 20, 8, 0)
        e.loudlog_set_period(2, 8, M.LOUDLOG_SAMPLE)
        e.loudlog_set_period(0, 8, 0)
        assert e.loudlog_period()[0] == 0 and code(e.loudlog_series) == E.ERR_ARG
        e.loudlog_set_period(2, 8, M.LOUDLOG_SAMPLE)
        feed(e, x, [])
        before = e.loudlog_series()
        assert code(e.loudlog_set_period, 3, 4, 1) == E.ERR_STATE
        assert code(e.loudlog_set_period, 0, 0, 0) == E.ERR_STATE
        assert e.loudlog_period() == (2, 8, M.LOUDLOG_SAMPLE)
        after = e.loudlog_series()
        assert (after[2] == 1).all()
        for k in range(4):
            assert np.array_equal(before[k].view(np.uint32), after[k].view(np.uint32))
    with M.Engine(4, 48000.0, meters=M.METER_TRUEPEAK) as e:
        assert code(e.loudlog_set_period, 1, 8, 0) == E.ERR_ARG
