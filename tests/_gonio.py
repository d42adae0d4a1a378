"""The yardstick of MTR_METER_GONIO (tests/test_gonio_cpu.py, tests/test_gpu_gonio.py): a restatement of the goniometer's data pump —
draw_rb of gui/goniometer.c:299-538 in points mode, without oversampling, with infinite persistence and without inflate, the set-up of
:165, :897-912 and :1086-1091, and the display period of src/goniometerlv2.c:25,81.

The reference's draw_rb paints with cairo inside a robtk UI and cannot be built on the test machines; this is its arithmetic alone,
written in the reference's C types: f32 where it holds a float, the double intermediates C's promotions give an expression, libm's
expf / log10f / logf through ctypes.  Vectorised over the streams, serial over the frames.  Integer casts come only behind the range
test: NaN coordinates occur."""
import ctypes
import math

import numpy as np

F32, F64 = np.float32, np.float64
BOUNDS = 373                                 # GM_BOUNDS
CENTER = F32(186.5)                          # GM_CENTER
RAD2 = F32(100.0)                            # GM_RAD2
DIALS = (54.0, 58.0, 40.0, 50.0)             # attack, decay, target, rms: src/goniometerlv2.c:101-104

_libm = ctypes.CDLL("libm.so.6")
for _n in ("expf", "log10f", "logf"):
    getattr(_libm, _n).restype = ctypes.c_float
    getattr(_libm, _n).argtypes = [ctypes.c_float]


def _f(name, x):
    return F32(getattr(_libm, name)(float(F32(x))))


def cells(shift):
    return (BOUNDS + (1 << shift) - 1) >> shift


class Derived:
    pass


def derive(rate, P=0, dials=DIALS, shift=2):
    """what mtr_gonio_derive answers: P, G, hpw, the two attack factors, g_target, g_rms"""
    d = Derived()
    d.P = int(P) if P else int(np.rint(rate / 25.0))                     # goniometerlv2.c:81
    d.G = cells(shift)
    d.hpw = _f("expf", -2.0 * math.pi * 20 / rate)                        # :165
    ga, gd = F32(dials[0]), F32(dials[1])                                 # :897-904
    ga = F32(0.1 * math.exp(0.06 * float(ga)) - .09)
    gd = F32(0.1 * math.exp(0.06 * float(gd)) - .09)
    if float(ga) < .01:
        ga = F32(.01)
    if float(gd) < .01:
        gd = F32(.01)
    d.g_rms = F32(.01 * float(F32(dials[3])))                             # :906
    gt = F32(math.exp(1.8 * (-.02 * float(F32(dials[2])) + 1.0)))         # :909-911
    if float(gt) < .15:
        gt = F32(.15)
    d.g_target = gt
    elapsed = F32(d.P / float(rate))                                      # :499
    d.attack = (F32(float(ga) * (.31 + .1 * float(_f("log10f", elapsed)))),      # :524, the target below the gain
                F32(float(gd) * (.03 + .007 * float(_f("logf", elapsed)))))      # ... and otherwise
    return d


class Gonio:
    """S goniometers in lock step"""

    def __init__(self, S, rate, P=0, shift=2, autogain=False, gain=1.0, width=1.75, dials=DIALS):
        self.S, self.shift, self.autogain = S, shift, bool(autogain)
        self.d = derive(rate, P, dials, shift)
        self.hw = float(F32(width)) * .5                                  # line_width * .5: a double
        self.gain0 = F32(gain)
        self.reset()

    def reset(self):
        S, G = self.S, self.d.G
        z = lambda: np.zeros(S, F32)                                      # noqa: E731
        self.lp0, self.lp1 = z(), z()                                     # :1086-1091
        self.last_x, self.last_y = np.full(S, CENTER, F32), np.full(S, CENTER, F32)
        self.gain = np.full(S, self.gain0, F32)
        self.xmax, self.xmin, self.ymax, self.ymin, self.rms0, self.rms1 = z(), z(), z(), z(), z(), z()
        self.j = 0
        self.bd, self.bc = np.zeros(S, np.uint32), np.zeros(S, np.uint32)
        self.series = []                                                  # (gain, drawn, clipped) per block, [S] each
        self.image_clear()

    def image_clear(self):
        S, G = self.S, self.d.G
        self.img = np.zeros((S, G, G), np.uint32)
        self.drawn, self.clipped, self.skipped = np.zeros(S, np.uint64), np.zeros(S, np.uint64), np.zeros(S, np.uint64)

    def set_gain(self, g):
        self.gain = np.full(self.S, F32(g), F32)

    def run(self, x):
        """x float32 [S, T, 2]"""
        x = np.asarray(x, F32)
        with np.errstate(all="ignore"):
            for t in range(x.shape[1]):
                self._frame(x[:, t, 0], x[:, t, 1])
                self.j += 1
                if self.j == self.d.P:
                    self._block_end()
                    self.j = 0
        return self

    def _frame(self, d0, d1):
        hpw = self.d.hpw
        self.lp0 = self.lp0 + hpw * (d0 - self.lp0)                       # :401-405
        self.lp1 = self.lp1 + hpw * (d1 - self.lp1)
        self.lp0 = self.lp0 + F32(1e-12)
        self.lp1 = self.lp1 + F32(1e-12)
        lp0, lp1 = self.lp0, self.lp1
        ax, ay = lp0 - lp1, lp0 + lp1
        if self.autogain:                                                 # :413-421: a NaN loses
            self.xmax = np.where(ax > self.xmax, ax, self.xmax)
            self.xmin = np.where(ax < self.xmin, ax, self.xmin)
            self.ymax = np.where(ay > self.ymax, ay, self.ymax)
            self.ymin = np.where(ay < self.ymin, ay, self.ymin)
            self.rms0 = self.rms0 + lp0 * lp0
            self.rms1 = self.rms1 + lp1 * lp1
        x = CENTER - self.gain * ax * RAD2                                # :441-442
        y = CENTER - self.gain * ay * RAD2
        l2 = (self.last_x - x) * (self.last_x - x) + (self.last_y - y) * (self.last_y - y)
        paint = ~(l2 < F32(2.0))                                          # :446
        self.last_x = np.where(paint, x, self.last_x)
        self.last_y = np.where(paint, y, self.last_y)
        px = np.rint((self.last_x.astype(F64) - self.hw).astype(F32))     # :470 rintf: half to even
        py = np.rint((self.last_y.astype(F64) - self.hw).astype(F32))
        inside = paint & (px >= 0) & (px < BOUNDS) & (py >= 0) & (py < BOUNDS)
        i = np.nonzero(inside)[0]
        if i.size:
            cx, cy = px[i].astype(np.int64) >> self.shift, py[i].astype(np.int64) >> self.shift
            self.img[i, cy, cx] += np.uint32(1)                           # (one point per stream: no index repeats; wraps at 2^32)
        out = paint & ~inside
        self.bd += inside.astype(np.uint32)
        self.bc += out.astype(np.uint32)
        self.drawn += inside.astype(np.uint64)
        self.clipped += out.astype(np.uint64)
        self.skipped += (~paint).astype(np.uint64)

    def _block_end(self):
        d = self.d
        self.lp0 = np.where(np.isfinite(self.lp0), self.lp0, F32(0))      # :494-495
        self.lp1 = np.where(np.isfinite(self.lp1), self.lp1, F32(0))
        if self.autogain:                                                 # :497-536
            xdif, ydif = self.xmax - self.xmin, self.ymax - self.ymin
            mx = np.sqrt((xdif * xdif + ydif * ydif).astype(F64)).astype(F32)
            mx = (mx.astype(F64) * .707).astype(F32)
            if float(d.g_rms) > 0 and math.isfinite(float(d.g_rms)):      # (rms_c = P > 0)
                c = F32(d.P)
                r = np.where(self.rms0 > self.rms1, np.sqrt(self.rms0 / c), np.sqrt(self.rms1 / c)).astype(F32)
                rms = (5.436 * r.astype(F64)).astype(F32)
                mx = (mx.astype(F64) * (1.0 - float(d.g_rms)) + rms.astype(F64) * float(d.g_rms)).astype(F32)
            mx = mx * d.g_target
            mx = np.where(np.isfinite(mx), mx, F32(0)).astype(F32)
            m64 = mx.astype(F64)
            tg = np.where(m64 < .01, F32(100.0), np.where(mx > F32(100.0), F32(.02), (2.0 / m64).astype(F32))).astype(F32)
            attack = np.where(tg < self.gain, d.attack[0], d.attack[1]).astype(F32)
            tg = self.gain + attack * (tg - self.gain)
            tg = np.where(tg.astype(F64) < .001, F32(.001), tg).astype(F32)
            self.gain = tg
            z = np.zeros(self.S, F32)
            self.xmax, self.xmin, self.ymax, self.ymin, self.rms0, self.rms1 = z, z.copy(), z.copy(), z.copy(), z.copy(), z.copy()
        self.series.append((self.gain.copy(), self.bd.copy(), self.bc.copy()))
        self.bd[:] = 0
        self.bc[:] = 0

    def series_arrays(self):
        """(gain float32, drawn uint32, clipped uint32), each [S, blocks]"""
        if not self.series:
            return np.zeros((self.S, 0), F32), np.zeros((self.S, 0), np.uint32), np.zeros((self.S, 0), np.uint32)
        return tuple(np.stack([p[k] for p in self.series], axis=1) for k in range(3))


# ---- the signal set of tests/test_gpu_gonio.py ---------------------------------------------------------------------------------------
N_SIGNALS = 8


def signals(S, T, rate=48000.0, seed=1):
    """float32 [S, T, 2]: stream s carries signal s mod 8, with its own seed.  0: uncorrelated noise at sigma 0.25 (nearly all painted);
    1: anti-phase noise at sigma 0.5 (clips); 2: two 100 Hz sines at 0.01 (mostly skipped); 3: silence (all skipped); 4: 997 and 1499 Hz
    at 0.9 (clips at gain 4); 5: noise at sigma 0.003 (mostly skipped at gain 1, mostly painted at gain 4); 6: signal 0 with one NaN and one
    Inf sample; 7: an in-phase 440 Hz sine."""
    x = np.zeros((S, T, 2), F32)
    t = np.arange(T, dtype=F64) / rate
    for s in range(S):
        r = np.random.default_rng(seed * 1000 + s)
        k = s % N_SIGNALS
        if k in (0, 6):
            x[s] = (0.25 * r.standard_normal((T, 2))).astype(F32)
            if k == 6:
                x[s, T // 3, 0] = np.nan
                x[s, (2 * T) // 3, 1] = np.inf
        elif k == 1:
            v = (0.5 * r.standard_normal(T)).astype(F32)
            x[s, :, 0], x[s, :, 1] = v, -v
        elif k == 2:
            ph = r.uniform(0, 2 * math.pi)
            x[s, :, 0] = (0.01 * np.sin(2 * math.pi * 100 * t + ph)).astype(F32)
            x[s, :, 1] = (0.01 * np.sin(2 * math.pi * 100 * t + ph + 1.0)).astype(F32)
        elif k == 4:
            x[s, :, 0] = (0.9 * np.sin(2 * math.pi * 997 * t + r.uniform(0, 6))).astype(F32)
            x[s, :, 1] = (0.9 * np.sin(2 * math.pi * 1499 * t + r.uniform(0, 6))).astype(F32)
        elif k == 5:
            x[s] = (0.003 * r.standard_normal((T, 2))).astype(F32)
        elif k == 7:
            v = (0.5 * np.sin(2 * math.pi * 440 * t + r.uniform(0, 6))).astype(F32)
            x[s, :, 0], x[s, :, 1] = v, v
    return x


def coverage(g, frames):
    """the guard of every test on the set: on the restatement's counts some stream clipped, some stream skipped between 10 % and 90 % of its
    frames, some stream painted nothing — a kernel that ignores a rule cannot pass"""
    assert (g.clipped > 0).any(), "no stream clipped"
    assert ((g.skipped >= frames // 10) & (g.skipped <= (9 * frames) // 10)).any(), "no stream skipped 10 .. 90 % of its frames"
    assert (g.drawn == 0).any(), "no stream painted nothing"
