"""The yardstick of MTR_METER_SCOPE (tests/test_scope_cpu.py, tests/test_gpu_scope.py): a restatement of the analysis under the
reference's stereo / frequency scope and phase wheel — fftx_run and ft_analyze (gui/fft.c:163-180, 289-361), process_audio of
gui/stereoscope.c:705-741 and gui/phasewheel.c:1307-1339.

The reference's FFT is fftw3f, which the test machines do not have: the transform here is numpy's float64 DFT of the f32 windowed
frames.  Everything around it is written in the reference's types: the window as ft_gen_window makes it (double arithmetic, stored
f32), the windowed frame an f32 product, power and phase f32 from the f32-rounded spectrum, thresholds and smoothers with the
double intermediates C's promotions give them.

Behind it: the mirror of k_scope's own transform (mirror_fft, mirror_powers) — the kernel's passes on the kernel's slots in numpy.  In
complex128 it shows that the pass structure as written is the DFT; in complex64 it is the yardstick for eps (W): what f32 arithmetic in
this order costs, measured without the kernel (tests/test_scope_cpu.py)."""
import math

import numpy as np

F32 = np.float32
WINDOWS = (256, 512, 1024, 2048, 4096, 8192, 16384)
THRESH = float(F32(1e-6))                   # phasewheel.c:1212


def window(W):
    """ft_hannhamm (.5, .5) and the 2 / sum of ft_gen_window: libm's cos, a sequential double sum of the f32 values"""
    c = 2.0 * math.pi / (W - 1.0)
    w = np.array([.5 - .5 * math.cos(c * i) for i in range(W)], np.float64).astype(F32)
    total = 0.0
    for v in w.tolist():
        total += v
    return (w.astype(np.float64) * (2.0 / total)).astype(F32)


def default_hop(fs):
    return int(math.ceil(float(fs) / 25.0))  # fftx_init (.., 25): fft.c:219


def eps(W):
    """Higham's bound for a radix-2 f32 FFT with correctly rounded twiddles, with about 15 % headroom"""
    return 8.0 * math.log2(W) * 2.0 ** -24


def windowed(x, W, H, j, win):
    """the f32 windowed frames [W, 2] of analysis j (0-based) of the stream x [T, 2]: its last W frames at frame (j + 1) H, zeros in
    front of the stream's start"""
    end = (j + 1) * H
    fr = np.zeros((W, 2), F32)
    lo = max(0, end - W)
    fr[W - (end - lo):] = x[lo:end]
    return fr * win[:, None]


class Scope:
    """one stream's fa / fb, SFSUI and MF2UI state"""

    def __init__(self, W, thresh=THRESH):
        self.W, self.B, self.thresh = W, W // 2, F32(thresh)
        B = self.B
        self.level, self.lr = np.full(B, -100, F32), np.full(B, .5, F32)           # stereoscope.c:143-146
        self.phase, self.plevel, self.peak = np.zeros(B, F32), np.full(B, -100, F32), F32(0)   # phasewheel.c:202-205, :1215
        self.power = np.zeros((2, B), F32)                                         # fftx_reset
        self.p64 = np.zeros((2, B))                                                # (the float64 |X|^2 of the last analysis: case 1)
        self.N = 0.0

    def analyse(self, fw):
        """one analysis on the windowed frames fw [W, 2] f32"""
        B = self.B
        X = np.fft.fft(fw.astype(np.float64), axis=0)[:B].T                        # [2, B]
        self.N = math.sqrt(self.W * float(np.sum(fw.astype(np.float64) ** 2)))
        self.p64 = np.zeros((2, B))
        self.p64[:, 1:B - 1] = (X.real ** 2 + X.imag ** 2)[:, 1:B - 1]
        re, im = X.real.astype(F32), X.imag.astype(F32)
        with np.errstate(all="ignore"):
            pw = re * re + im * im                                                     # ft_analyze: f32
            ph = np.arctan2(im, re)
            s = slice(1, B - 1)
            self.power[:, s] = pw[:, s]
            pl, pr = pw[0, s], pw[1, s]
            # stereoscope.c:713-737
            quiet = (pl < F32(1e-20)) & (pr < F32(1e-20))
            lv = np.where(pl > pr, pl, pr)                                             # MAX (a, b): a > b ? a : b
            lt = (.5 + .5 * (np.sqrt(pr) - np.sqrt(pl)).astype(np.float64) / np.sqrt(lv).astype(np.float64)).astype(F32)
            level, lr = self.level[s], self.lr[s]
            nlevel = (level.astype(np.float64) + (.1 * (lv - level).astype(np.float64) + 1e-20)).astype(F32)
            nlr = (lr.astype(np.float64) + (.1 * (lt - lr).astype(np.float64) + 1e-10)).astype(F32)
            self.level[s] = np.where(quiet, F32(0), nlevel)
            self.lr[s] = np.where(quiet, F32(.5), nlr)
            # phasewheel.c:1315-1335
            below = (pl < self.thresh) | (pr < self.thresh)
            self.phase[s] = np.where(below, F32(0), ph[1, s] - ph[0, s])
            self.plevel[s] = np.where(below, F32(-100), lv)
            peak = F32(np.fmax.reduce(self.plevel[s][~below], initial=F32(0)))         # `if (level > peak)`: a NaN never is
            pk = F32(float(self.peak) + (.04 * float(F32(peak - self.peak)) + 1e-15))
            if math.isnan(pk):
                pk = F32(0)
            if pk > 1000:
                pk = F32(1000)
            self.peak = pk
        return self


def run(x, W, H, thresh=THRESH, win=None, each=None):
    """every analysis of the stream x [T, 2] f32 in order; each (j, scope) after every one.  Returns the Scope and the number of
    analyses"""
    win = window(W) if win is None else win
    sc = Scope(W, thresh)
    n = x.shape[0] // H
    for j in range(n):
        sc.analyse(windowed(x, W, H, j, win))
        if each:
            each(j, sc)
    return sc, n


def signals(T, fs, W, seed, S=5):
    """the GPU tests' streams [S, T, 2]: white noise (sigma .25 on L, .1 on R) plus one quiet tone per stream, off the bin centres"""
    rng = np.random.default_rng(seed)
    t = np.arange(T) / float(fs)
    x = np.zeros((S, T, 2), F32)
    for s in range(S):
        f = (37.3 + 61.7 * s) * fs / W
        x[s, :, 0] = (rng.normal(0, .25, T) + .05 * np.sin(2 * np.pi * f * t)).astype(F32)
        x[s, :, 1] = (rng.normal(0, .1, T) + .04 * np.sin(2 * np.pi * f * t + .3 * (s + 1))).astype(F32)
    return x


def ratios(x, W, H, win=None):
    """per bin of 1 .. B - 2: rho = the largest N_j / sqrt (max (pL, pR)_j) over the stream's analyses — what the bound on lr is
    stated in; and the largest N"""
    B = W // 2
    rho, nmax = np.zeros(B - 2), [0.0]

    def each(j, sc):
        m = np.sqrt(np.maximum(sc.p64[0, 1:B - 1], sc.p64[1, 1:B - 1]))
        with np.errstate(divide="ignore"):
            np.maximum(rho, np.where(m > 0, sc.N / m, np.inf), out=rho)
        nmax[0] = max(nmax[0], sc.N)
    run(x, W, H, win=win, each=each)
    return rho, nmax[0]


# ---- the mirror of k_scope's transform (mtr_scope.hip): the same passes on the same slots, in numpy ------------------------------------

def bitrev(W):
    """bitrev (k) over log2 W bits for k = 0 .. W - 1"""
    L = W.bit_length() - 1
    k, r = np.arange(W), np.zeros(W, np.int64)
    for b in range(L):
        r |= ((k >> b) & 1) << (L - 1 - b)
    return r


def twiddles(W, ctype=np.complex128):
    """exp (-2 pi i m / W), m = 0 .. W - 1, as mtr_engine_scope_configure makes them: cos and -sin in double; complex64: each rounded once"""
    ph = 2.0 * math.pi * np.arange(W).astype(np.float64) / float(W)
    tw = np.empty(W, ctype)
    tw.real, tw.imag = np.cos(ph), -np.sin(ph)                                     # (the assignment rounds to the part's type)
    return tw


def _cmul(a, w):
    """cmul of mtr_scope.hip: four products, one difference, one sum, each rounded in the part's type (no fused multiply-add)"""
    y = np.empty_like(a)
    y.real = a.real * w.real - a.imag * w.imag
    y.imag = a.real * w.imag + a.imag * w.real
    return y


def mirror_fft(z, ctype=np.complex128):
    """The forward DFT of z [..., W] by the kernel's own pass structure, every operation in ctype: in place, decimation in frequency,
    radix-4 passes for ln = LOGW, LOGW - 2, .. >= 2 — butterfly bf of a pass has jj = bf & (q - 1), base = ((bf >> (ln - 2)) << ln) + jj,
    works on base + {0, q, 2q, 3q} (q = 2^ln / 4) and multiplies y1, y2, y3 by tw [2m], tw [m], tw [3m] at m = jj << (LOGW - ln) — then one
    radix-2 pass where LOGW is odd; X [k] ends at slot bitrev (k).  The lane remap of ln = 3 .. 5 is kept: it must visit every butterfly
    of the pass once."""
    W = z.shape[-1]
    L = W.bit_length() - 1
    assert 1 << L == W and L >= 2
    z = np.array(z, ctype)
    tw = twiddles(W, ctype)
    b0 = np.arange(W // 4)
    for ln in range(L, 1, -2):
        q = 1 << (ln - 2)
        bf = ((b0 & ((1 << (L - ln)) - 1)) << (ln - 2)) + (b0 >> (L - ln)) if 3 <= ln <= 5 else b0
        assert np.array_equal(np.sort(bf), b0)
        jj = bf & (q - 1)
        base = ((bf >> (ln - 2)) << ln) + jj
        a0, a1, a2, a3 = z[..., base], z[..., base + q], z[..., base + 2 * q], z[..., base + 3 * q]
        t0, t1, u, d = a0 + a2, a1 + a3, a0 - a2, a1 - a3
        v = np.empty_like(d)
        v.real, v.imag = d.imag, -d.real                                           # -i (a1 - a3)
        y0, y1, y2, y3 = t0 + t1, t0 - t1, u + v, u - v
        if ln > 2:
            m = jj << (L - ln)
            y1, y2, y3 = _cmul(y1, tw[2 * m]), _cmul(y2, tw[m]), _cmul(y3, tw[3 * m])
        z[..., base], z[..., base + q], z[..., base + 2 * q], z[..., base + 3 * q] = y0, y1, y2, y3
    if L & 1:
        e = 2 * np.arange(W // 2)
        a0, a1 = z[..., e], z[..., e + 1]
        z[..., e], z[..., e + 1] = a0 + a1, a0 - a1
    return z[..., bitrev(W)]


def mirror_powers(fw, ctype=np.complex64):
    """the windowed frames fw [W, 2] f32 -> the two powers [2, B] as the kernel makes them: ONE transform of L + iR, the even / odd
    split and ft_analyze's power in the part's type (bin_of); bins 0 and B - 1 zero, as they are never written"""
    W = fw.shape[0]
    B = W // 2
    z = np.empty(W, ctype)
    z.real, z.imag = fw[:, 0], fw[:, 1]
    Z = mirror_fft(z, ctype)
    i = np.arange(1, B - 1)
    zi, zc = Z[i], Z[W - i]
    h = zi.real.dtype.type(.5)
    lre, lim = h * (zi.real + zc.real), h * (zi.imag - zc.imag)
    rre, rim = h * (zi.imag + zc.imag), h * (zc.real - zi.real)
    p = np.zeros((2, B), zi.real.dtype)
    p[0, 1:B - 1], p[1, 1:B - 1] = lre * lre + lim * lim, rre * rre + rim * rim
    return p
