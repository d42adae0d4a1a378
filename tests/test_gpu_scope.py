"""MTR_METER_SCOPE on the GPU (mtr_scope.hip) against the restatement of tests/_scope.py: numpy's float64 DFT of the f32 windowed
frames, the reference's thresholds and smoothers in its own types (gui/fft.c, gui/stereoscope.c:705-741, gui/phasewheel.c:1307-1339).

The kernel takes both channels from ONE complex f32 FFT of L + iR, so the tolerances are stated relative to the norm of both:
    N      = sqrt (W sum (fL^2 + fR^2)) over the windowed frames of an analysis — the norm of the packed spectrum, by Parseval;
    eps(W) = 8 log2 (W) 2^-24 — Higham's bound for a radix-2 f32 FFT with correctly rounded twiddles, with about 15 % headroom.
  spectrum   |sqrt power_gpu - sqrt power_64| <= eps N at every bin of both channels (the last analysis);
  level      |level - level_ref| <= 4 eps max N^2 (|delta power| <= 3 eps N^2, and the smoother is a contraction); peak and plevel alike;
  lr         |lr - lr_ref| <= 4 eps rho, rho = the largest N / sqrt (max (pL, pR)) of the bin over the case's analyses, on the bins with
             rho <= 1 / LR_FLOOR; at most 1 % of a case's bins may lie outside (tests/test_scope_cpu.py shows the seeds stay inside);
  phase      where both restated powers reach the threshold: |wrap (delta)| min (|X_L|, |X_R|) <= 4 eps N; below it phase = 0 and
             plevel = -100 exactly; bins within a relative 1e-4 of the threshold are left out (at most 0.1 %; with these seeds: none).
LR_FLOOR: the bound on lr was first stated for the bins with sqrt (max (pL, pR)) >= 1e-3 N.  With 13 analyses of white noise at
W = 16384 — where the rms bin is N / 128 — that set leaves 1.6 - 3.2 % of the bins out (test_scope_cpu prints it), more than the cap of
1 % allows.  The same bound is therefore held on the LARGER set >= 1e-4 N (it asks more: 4 eps rho is still below 0.3 there), which
leaves no bin of these signals out.
CASES: all seven windows at three hops — the default, W / 4 and 777 — so that every dense kernel, the radix-2 pass and the remapped passes
of an odd log2 W included, is held to the DFT (tests/test_scope_cpu.py: the census, and the same bound on a numpy mirror of the passes).
Every case prints its largest figure in units of its bound."""
import functools
import math

import numpy as np
import pytest

import _scope

pytestmark = pytest.mark.gpu
FS, S, NA = 48000, 5, 13
LR_FLOOR = 1e-4
CASES = [(W, hk) for W in _scope.WINDOWS for hk in ("default", "quarter", "777")]
NAMES = ("level", "lr", "phase", "plevel", "peak", "power_l", "power_r")


def hop_of(W, hk):
    return {"default": _scope.default_hop(FS), "quarter": W // 4, "777": 777}[hk]


# seeds: the first of 7000 + W + H + 100000 k whose last analysis leaves no bin within 1e-4 of the phase wheel's threshold (at W = 16384 a
# seed leaves 3 or 4 of the 81 900 powers there on average); tests/test_scope_cpu.py holds them to it without a GPU
SEED_K = {(8192, 1920): 2, (8192, 2048): 1, (8192, 777): 3, (16384, 1920): 10, (16384, 4096): 6, (16384, 777): 42}


@functools.lru_cache(maxsize=None)
def signal_of(W, H):
    x = _scope.signals(NA * H + 5, FS, W, seed=7000 + W + H + 100000 * SEED_K.get((W, H), 0), S=S)
    x.setflags(write=False)
    return x


@pytest.fixture(scope="module")
def M():
    import meters.lv2_amd as m
    return m


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return all(np.array_equal(bits(a[n]), bits(b[n])) for n in NAMES)


def run_gpu(M, x, W, H=0, calls=None, meters=None, thresh=None, fs=FS, handoff=None, extra=None, odd=False):
    """x [S, T, 2] through process_device in `calls` pieces (default: one), from a buffer whose rows are longer than T with NaN in the
    gap.  handoff = i: after call i the state moves into a fresh engine, which takes the rest.  odd: the same rows one float behind
    the start of an allocation that is one float longer — every stream then starts on 4 bytes, not on 8 (the row is an even number of
    floats).  Returns (scope_read, analyses)."""
    import torch
    meters = M.METER_SCOPE if meters is None else meters
    T = x.shape[1]
    buf = np.full((x.shape[0], T + 37, 2), np.nan, np.float32)
    buf[:, :T] = x
    if odd:
        flat = np.concatenate([np.full(1, np.nan, np.float32), buf.ravel()])
        dev = torch.from_numpy(flat).cuda()
        assert dev.data_ptr() % 8 == 0 and dev.numel() == buf.size + 1
        ptr0 = dev.data_ptr() + 4
    else:
        dev = torch.from_numpy(buf).cuda()
        ptr0 = dev.data_ptr()
    st = torch.cuda.current_stream().cuda_stream

    def engine():
        e = M.Engine(x.shape[0], float(fs), meters)
        e.scope_configure(W, H, _scope.THRESH if thresh is None else thresh)
        return e
    e = engine()
    pos = 0
    for i, n in enumerate(calls or [T]):
        e.process_device(ptr0 + pos * 8, n, buf.shape[1], st)
        pos += n
        if handoff == i:
            blob = e.state_export()
            e.close()
            e = engine()
            e.state_import(blob)
    assert pos == T
    out, n_an = e.scope_read(), e.scope_analyses()
    if extra:
        extra(e, out)
    e.close()
    del dev
    return out, n_an


@functools.lru_cache(maxsize=None)
def reference(W, H):
    """per stream: the restatement's state after the last analysis, the float64 powers and N of that analysis, the largest N and rho"""
    x, win = signal_of(W, H), _scope.window(W)
    out = []
    for s in range(S):
        rho, nmax = _scope.ratios(x[s], W, H, win=win)
        sc, n = _scope.run(x[s], W, H, win=win)
        assert n == NA
        out.append((sc, rho, nmax))
    return out


_gpu = {}


def gpu_of(M, W, H):
    if (W, H) not in _gpu:
        _gpu[W, H] = run_gpu(M, signal_of(W, H), W, H)
    return _gpu[W, H]


@pytest.mark.parametrize("W,hk", CASES)
def test_spectrum(M, W, hk):
    H, B = hop_of(W, hk), W // 2
    (g, n_an), ref = gpu_of(M, W, H), reference(W, H)
    assert n_an == NA
    worst = 0.0
    for s in range(S):
        sc = ref[s][0]
        for c, name in enumerate(("power_l", "power_r")):
            p = g[name][s].astype(np.float64)
            assert p[0] == 0 and p[B - 1] == 0
            assert (p >= 0).all()
            worst = max(worst, float(np.max(np.abs(np.sqrt(p) - np.sqrt(sc.p64[c])))) / sc.N)
    print(f"W {W} H {H}: largest |sqrt p - sqrt p64| = {worst:.3e} N = {worst / _scope.eps(W):.4f} of the bound")
    assert worst <= _scope.eps(W)


@pytest.mark.parametrize("W,hk", CASES)
def test_smoothers(M, W, hk):
    H, B = hop_of(W, hk), W // 2
    (g, _), ref = gpu_of(M, W, H), reference(W, H)
    e4 = 4 * _scope.eps(W)
    fig = dict(level=0.0, lr=0.0, peak=0.0, plevel=0.0)
    for s in range(S):
        sc, rho, nmax = ref[s]
        bound = e4 * nmax ** 2
        fig["level"] = max(fig["level"], float(np.max(np.abs(g["level"][s].astype(np.float64) - sc.level))) / bound)
        fig["peak"] = max(fig["peak"], abs(float(g["peak"][s]) - float(sc.peak)) / bound)
        near = near_threshold(sc)
        assert near.mean() <= 1e-3
        fig["plevel"] = max(fig["plevel"], float(np.max(np.abs(g["plevel"][s].astype(np.float64) - sc.plevel)[~near])) / bound)
        ok = rho * LR_FLOOR <= 1
        assert np.mean(~ok) <= 0.01
        d = np.abs(g["lr"][s].astype(np.float64) - sc.lr)
        assert d[0] == 0 and d[B - 1] == 0
        fig["lr"] = max(fig["lr"], float(np.max(d[1:B - 1][ok] / (e4 * rho[ok]))))
        assert g["level"][s][0] == -100 and g["level"][s][B - 1] == -100 and g["plevel"][s][0] == -100 and g["plevel"][s][B - 1] == -100
    print(f"W {W} H {H}: in units of the bounds: " + ", ".join(f"{k} {v:.2e}" for k, v in fig.items()))
    assert max(fig.values()) <= 1.0, fig


def near_threshold(sc):
    """bins whose restated power lies within a relative 1e-4 of the phase wheel's threshold on either channel (bins 0, B - 1: never)"""
    t = float(sc.thresh)
    near = np.any(np.abs(sc.power.astype(np.float64) - t) <= 1e-4 * t, axis=0)
    near[0] = near[-1] = False
    return near


@pytest.mark.parametrize("W,hk", CASES)
def test_phase(M, W, hk):
    H, B = hop_of(W, hk), W // 2
    (g, _), ref = gpu_of(M, W, H), reference(W, H)
    worst, n_below = 0.0, 0
    for s in range(S):
        sc = ref[s][0]
        near = near_threshold(sc)
        assert not near.any()                                          # (the seeds leave none out; the rule allows 0.1 %)
        inner = np.zeros(B, bool)
        inner[1:B - 1] = True
        below = np.any(sc.power < sc.thresh, axis=0) & inner
        above = ~below & inner
        n_below += int(below.sum())
        assert (g["phase"][s][below] == 0).all() and (g["plevel"][s][below] == -100).all()
        assert g["phase"][s][0] == 0 and g["phase"][s][B - 1] == 0
        d = g["phase"][s].astype(np.float64) - sc.phase.astype(np.float64)
        d = np.abs((d + math.pi) % (2 * math.pi) - math.pi)
        amp = np.sqrt(np.minimum(sc.p64[0], sc.p64[1]))
        worst = max(worst, float(np.max((d * amp)[above])) / (4 * _scope.eps(W) * sc.N))
    print(f"W {W} H {H}: largest |wrap (delta phase)| min |X| = {worst:.2e} of the bound; {n_below} of {S * (B - 2)} bins below the threshold")
    assert worst <= 1.0


def tone_bin(W, which):
    """low: W / 8 + 3; high: B - 3, where every high bit of the index is set — a slip in the bit-reversed read of the split shows"""
    return {"low": W // 8 + 3, "high": W // 2 - 3}[which]


@pytest.mark.parametrize("which", ["low", "high"])
@pytest.mark.parametrize("W", _scope.WINDOWS)
def test_tones(M, W, which):
    """bin-centred sines at every window: a channel swap, a bin off by one or a wrong sign of the transform shows here"""
    H, k, A = _scope.default_hop(FS), tone_bin(W, which), 0.4
    T = NA * H + 5
    tone = (A * np.sin(2 * np.pi * k * np.arange(T) / W + 0.7)).astype(np.float32)
    late = (A * np.sin(2 * np.pi * k * np.arange(T) / W + 0.7 - 1.1)).astype(np.float32)
    x = np.zeros((S, T, 2), np.float32)
    x[0, :, 0] = tone                                                 # L only
    x[1, :, 1] = tone                                                 # R only
    x[2, :, 0] = x[2, :, 1] = tone                                    # equal in both
    x[3, :, 0], x[3, :, 1] = tone, -tone                              # R inverted
    x[4, :, 0], x[4, :, 1] = tone, late                               # R 1.1 rad behind L
    g, n_an = run_gpu(M, x, W, H)
    assert n_an == NA
    e4 = 4 * _scope.eps(W)
    for s in range(S):
        sc, _ = _scope.run(x[s], W, H)
        tol = e4 * sc.N / A                                           # (rho of the tone's bin: N / A)
        assert abs(float(g["lr"][s, k]) - float(sc.lr[k])) <= tol, s
        assert abs(float(g["level"][s, k]) - float(sc.level[k])) <= e4 * sc.N ** 2, s
        assert int(np.argmax(g["power_l"][s] + g["power_r"][s])) == k
    settle = .5 * .9 ** NA                                            # what 13 steps of the one-pole leave of the initial .5
    assert abs(float(g["lr"][0, k]) - settle) <= 1e-4 and abs(float(g["lr"][1, k]) - (1 - settle)) <= 1e-4
    assert abs(float(g["power_l"][0, k]) / A ** 2 - 1) < 1e-4 and g["power_r"][0, k] < 1e-10
    assert abs(float(g["power_r"][1, k]) / A ** 2 - 1) < 1e-4 and g["power_l"][1, k] < 1e-10
    assert g["phase"][0, k] == 0 and g["plevel"][0, k] == -100         # (the silent channel is below the threshold)
    tol = e4 * math.sqrt(6.0)                                         # N / A of a tone in both channels under this window
    assert abs(float(g["lr"][2, k]) - .5) <= tol and abs(float(g["phase"][2, k])) <= tol
    assert abs(abs(float(g["phase"][3, k])) - math.pi) <= tol and abs(float(g["lr"][3, k]) - .5) <= tol
    # phaseR - phaseL of stream 4.  Two things the W = 1024, k = 73 form of this test did not meet: the reference leaves the difference of
    # two atan2f unwrapped, so it is -1.1 or 2 pi - 1.1 depending on the bin; and ft_gen_window's Hann window (W - 1 in its cosine) does
    # not vanish at whole bins, so the tone's image at bin W - k leaks r = |What (2 k)| / What (0) of its amplitude into bin k and turns
    # each channel's phase by up to asin r — the float64 DFT itself answers -1.1 + 1.9e-4 at (W 256, k = B - 3), five times `tol`.  The
    # kernel is therefore held, with `tol`, to the float64 DFT's phase of this signal, and that phase to -1.1 within tol + 2 asin r
    sc, _ = _scope.run(x[4], W, H)
    wrap = lambda d: abs((d + math.pi) % (2 * math.pi) - math.pi)
    wh = np.fft.fft(_scope.window(W).astype(np.float64))
    r = float(abs(wh[(2 * k) % W]) / abs(wh[0]))
    fig = wrap(float(g["phase"][4, k]) - float(sc.phase[k])) / tol
    print(f"W {W} bin {k}: phase of the late channel: {fig:.2e} of the bound from the DFT's, {wrap(float(g['phase'][4, k]) + 1.1):.2e} rad "
          f"from -1.1 (image leak r = {r:.2e})")
    assert fig <= 1.0
    assert wrap(float(g["phase"][4, k]) + 1.1) <= tol + 2 * math.asin(r)


def test_silence(M):
    W, H = 1024, 777
    B, T = W // 2, NA * H + 5
    x = np.array(signal_of(W, H))
    x[0] = 0
    half = 6 * H + 100
    x[1, half:] = 0
    g, n_an = run_gpu(M, x, W, H)
    assert n_an == NA
    s = slice(1, B - 1)
    assert (bits(g["lr"][0, s]) == bits(np.float32(.5))).all() and (bits(g["level"][0, s]) == 0).all()
    assert (bits(g["phase"][0]) == 0).all() and (g["plevel"][0] == -100).all() and (bits(g["power_l"][0]) == 0).all()
    assert NA * H - half >= W                                         # W zero frames have passed before the last analysis
    assert (bits(g["lr"][1, s]) == bits(np.float32(.5))).all() and (bits(g["level"][1, s]) == 0).all()
    assert (g["level"][2, s] != 0).all() and (g["lr"][2, s] != np.float32(.5)).any()      # (a stream that goes on is not touched by it)
    # a call of fewer than H frames: initial values everywhere
    g, n_an = run_gpu(M, x[:, :H - 1], W, H)
    assert n_an == 0
    assert (g["level"] == -100).all() and (g["lr"] == np.float32(.5)).all() and (g["plevel"] == -100).all()
    for n in ("phase", "peak", "power_l", "power_r"):
        assert (bits(g[n]) == 0).all(), n


def cuts_of(W, H, T):
    calls = [1, H - 1, H, H + 1, 3 * H + 17, min(W, H) // 2 + 3]
    calls.append(T - sum(calls))
    assert calls[-1] > 0 and calls[5] < W
    return calls


@pytest.mark.parametrize("W,hk", [(1024, "777"), (256, "default"), (16384, "default"), (16384, "quarter"),
                                  (512, "quarter"), (2048, "777"), (4096, "default"), (8192, "777")])
def test_call_cuts(M, W, hk):
    """(at 8192 with H = 777 every analysis reads ten hops back through the tail)"""
    H = hop_of(W, hk)
    x = signal_of(W, H)
    T = x.shape[1]
    whole = gpu_of(M, W, H)
    calls = cuts_of(W, H, T)
    cut = run_gpu(M, x, W, H, calls=calls)
    assert cut[1] == whole[1] == NA and same(cut[0], whole[0])
    for i in (0, 4):
        moved = run_gpu(M, x, W, H, calls=calls, handoff=i)
        assert moved[1] == NA and same(moved[0], whole[0]), i


@pytest.mark.parametrize("W", [512, 1024, 8192])
def test_a_buffer_that_starts_on_an_odd_float(M, W):
    """every stream starts 4 bytes off an 8-byte boundary: frame_at takes its scalar path for the call's buffer (the tail stays aligned);
    in one call and in the cuts of test_call_cuts the seven arrays are bit for bit those of the aligned buffer"""
    H = 777
    x = signal_of(W, H)
    whole = gpu_of(M, W, H)
    for calls in (None, cuts_of(W, H, x.shape[1])):
        got = run_gpu(M, x, W, H, calls=calls, odd=True)
        assert got[1] == NA and same(got[0], whole[0]), calls


def test_company(M):
    W, H = 1024, 777
    x = signal_of(W, H)
    alone = gpu_of(M, W, H)
    got = {}

    def others(e, out):
        got[len(got)] = (e.stcorr_read(), e.kmeter_read())
    both = run_gpu(M, x, W, H, meters=M.METER_SCOPE | M.METER_STCORR | M.METER_KMETER, extra=others)
    assert both[1] == NA and same(both[0], alone[0])
    import torch
    e = M.Engine(S, float(FS), M.METER_STCORR | M.METER_KMETER)
    buf = np.full((S, x.shape[1] + 37, 2), np.nan, np.float32)
    buf[:, :x.shape[1]] = x
    dev = torch.from_numpy(buf).cuda()
    e.process_device(dev.data_ptr(), x.shape[1], buf.shape[1], torch.cuda.current_stream().cuda_stream)
    e.sync()
    want = (e.stcorr_read(), e.kmeter_read())
    e.close()
    for a, b in zip(got[0], want):
        for u, v in zip(a, b):
            assert np.array_equal(bits(u), bits(v))


def test_paths(M):
    import torch
    W, H = 1024, 777
    x = signal_of(W, H)
    T = x.shape[1]
    want = gpu_of(M, W, H)
    # the pair {4, 5} of a 6-channel frame
    wide = np.random.default_rng(5).normal(0, .3, (S, T, 6)).astype(np.float32)
    wide[:, :, 4:6] = x
    for host in (False, True):
        e = M.Engine(S, float(FS), M.METER_SCOPE)
        e.scope_configure(W, H)
        e.set_frame_layout(6, (4, 5))
        if host:
            e.process(wide)
        else:
            dev = torch.from_numpy(wide).cuda()
            e.process_device(dev.data_ptr(), T, T, torch.cuda.current_stream().cuda_stream)
        e.sync()
        assert e.scope_analyses() == NA and same(e.scope_read(), want[0]), host
        e.close()
    # host memory, f32 and S16
    e = M.Engine(S, float(FS), M.METER_SCOPE)
    e.scope_configure(W, H)
    e.set_host_chunk_bytes(2 * T * 8)                                 # (several chunks of streams)
    e.process(x)
    e.sync()
    assert same(e.scope_read(), want[0])
    e.close()
    pcm = np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16)
    dec = M.pcm_decode(M.PCM_S16, pcm)
    e = M.Engine(S, float(FS), M.METER_SCOPE)
    e.scope_configure(W, H)
    e.process_pcm(pcm)
    e.sync()
    got = e.scope_read()
    e.close()
    assert same(got, run_gpu(M, dec, W, H)[0])


def test_refusals_and_isolation(M):
    import torch
    W, H = 1024, 777
    x = signal_of(W, H)
    T = x.shape[1]
    want = gpu_of(M, W, H)
    E = M.engine
    e = M.Engine(S, float(FS), M.METER_SCOPE | M.METER_KMETER)
    e.scope_configure(W, H)
    dev = torch.from_numpy(np.array(x)).cuda()
    st = torch.cuda.current_stream().cuda_stream
    frames = np.full(S, T // 2, np.uint64)
    for f in (e.process_device_lengths, e.process_device_tracks):
        with pytest.raises(M.EngineError) as err:
            f(dev.data_ptr(), T, frames, T, st)
        assert err.value.code == E.ERR_UNSUPPORTED
    for f in (e.process_lengths, e.process_tracks):
        with pytest.raises(M.EngineError) as err:
            f(x, frames)
        assert err.value.code == E.ERR_UNSUPPORTED
    assert e.scope_analyses() == 0 and (e.stream_frames()[0] == 0).all()
    e.scope_configure(W, H)                                           # (still an engine that has processed nothing)
    e.process_device(dev.data_ptr(), T, T, st)
    e.sync()
    assert same(e.scope_read(), want[0])
    with pytest.raises(M.EngineError) as err:
        e.scope_configure(W, H)
    assert err.value.code == E.ERR_STATE
    assert e.scope_config() == (W, H, _scope.THRESH)
    e.reset()                                                         # (the configuration is kept, the meter starts again)
    assert e.scope_config() == (W, H, _scope.THRESH) and e.scope_analyses() == 0 and (e.scope_read()["level"] == -100).all()
    e.process_device(dev.data_ptr(), T, T, st)
    e.sync()
    assert same(e.scope_read(), want[0])
    for bad, code in (((128, 0), E.ERR_UNSUPPORTED), ((12288, 0), E.ERR_UNSUPPORTED), ((1000, 0), E.ERR_ARG), ((32768, 0), E.ERR_ARG),
                      ((1024, 63), E.ERR_ARG), ((1024, (1 << 20) + 1), E.ERR_ARG), ((1024, 0, -1.0), E.ERR_ARG), ((1024, 0, float("nan")), E.ERR_ARG)):
        with pytest.raises(M.EngineError) as err:
            e.scope_configure(*bad)
        assert err.value.code == code, bad
    e.close()
    # a NaN in one stream
    y = np.array(x)
    y[2, 3 * H + 11, 1] = np.nan
    g, _ = run_gpu(M, y, W, H)
    for s in (0, 1, 3, 4):
        assert all(np.array_equal(bits(g[n][s]), bits(want[0][n][s])) for n in NAMES), s
    assert np.isnan(g["level"][2, 1:W // 2 - 1]).all()


def test_default_hop_at_44100(M):
    W = 1024
    x = _scope.signals(10 * 1764 + 5, 44100, W, seed=44, S=S)
    e = M.Engine(S, 44100.0, M.METER_SCOPE)
    assert e.scope_config() == (1024, 1764, _scope.THRESH)
    e.close()
    g, n_an = run_gpu(M, x, W, 0, fs=44100)
    assert n_an == 10
    sc, n = _scope.run(x[0], W, 1764)
    assert n == 10
    _, nmax = _scope.ratios(x[0], W, 1764)
    assert np.max(np.abs(g["level"][0].astype(np.float64) - sc.level)) <= 4 * _scope.eps(W) * nmax ** 2
