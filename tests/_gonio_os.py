"""The yardstick of the goniometer's oversampling (include/mtr_gonio_os.h; tests/test_gonio_os_cpu.py, tests/test_gpu_gonio_os.py): the
reference's "Oversampling" preference (gui/goniometer.c:155-189, :359-377) puts a zita Resampler — setup (rate, rate * f, 2, 12, 1.0) — in
front of draw_rb.  This is a restatement of what that resampler computes (zita-resampler/resampler.cc:171-262 with np = f, hl = 12,
pstep = 1, fr = 1.0, behind setup_src's 8192 zero frames; the table of resampler-table.cc:52-75), in numpy f32 with every operation its
own rounding, and a GonioOS that feeds the points to the restatement of draw_rb in tests/_gonio.py.

tests/test_gonio_os_cpu.py holds it to tests/golden/gonio_os.npz, which the reference's Resampler wrote, and — where the reference-built
checker is there — to the live object."""
import copy
import math

import numpy as np

import _gonio
import _gonio_ends

F32, F64 = np.float32, np.float64
HL = 12                                      # hlen of setup_src
HALO = 2 * HL - 1                            # input frames in front of frame m that its points read
TINY = F32(1e-20)


def _sinc(x):
    x = abs(x)
    if x < 1e-6:
        return 1.0
    x *= math.pi
    return math.sin(x) / x


def _wind(x):
    x = abs(x)
    if x >= 1.0:
        return 0.0
    x *= math.pi
    return 0.384 + 0.500 * math.cos(x) + 0.116 * math.cos(2 * x)


_tables = {}


def table(f):
    """float32 [f + 1, 12]: Resampler_table's _ctab for fr = 1.0, hl = 12, np = f, in double as resampler-table.cc:65-74 builds it"""
    if f not in _tables:
        tab = np.zeros((f + 1, HL), F32)
        for j in range(f + 1):
            t = float(j) / float(f)
            for i in range(HL):
                tab[j, HL - 1 - i] = F32(1.0 * _sinc(t * 1.0) * _wind(t / HL))
                t += 1
        tab.setflags(write=False)
        _tables[f] = tab
    return _tables[f]


def hpw(rate, f):
    """:175 (:165 for f = 1): expf of the double -2.0 * M_PI * 20 / (rate * oversample), rate a double, the factor a float"""
    return _gonio._f("expf", -2.0 * math.pi * 20 / (float(rate) * float(F32(f))))


def upsample(x, f, hist=None):
    """x float32 [S, T, 2], hist float32 [S, 23, 2] (None: zeros — a reset stream) -> (points float32 [S, T * f, 2], the next hist).
    Point m f + ph: s = 1e-20f; s += x [m - 23 + i] * c1 [i] + x [m - i] * c2 [i] for i = 0 .. 11; out = s - 1e-20f (resampler.cc:215-228)"""
    x = np.asarray(x, F32)
    S, T = x.shape[0], x.shape[1]
    if hist is None:
        hist = np.zeros((S, HALO, 2), F32)
    ext = np.concatenate([np.asarray(hist, F32), x], axis=1)             # frame m of x is ext [m + 23]
    tab = table(f)
    out = np.zeros((S, T * f, 2), F32)
    with np.errstate(all="ignore"):
        for ph in range(f):
            c1, c2 = tab[ph], tab[f - ph]
            s = np.full((S, T, 2), TINY, F32)
            for i in range(HL):
                s = s + (ext[:, i:i + T] * c1[i] + ext[:, HALO - i:HALO - i + T] * c2[i])
            out[:, ph::f] = s - TINY
    return out, ext[:, ext.shape[1] - HALO:].copy()


class GonioOS:
    """S goniometers in lock step behind the interpolator: _gonio.Gonio on the points, with its hpw and its block length replaced (P f
    points, which is rms_c too) and its attack pair left (elapsed stays P / rate)"""

    def __init__(self, S, rate, f, P=0, **kw):
        self.S, self.f, self.rate = S, int(f), rate
        self.g = _gonio.Gonio(S, rate, P=P, **kw)
        self.P = self.g.d.P                                               # input frames per display update
        self.g.d.P = self.P * self.f
        self.g.d.hpw = hpw(rate, self.f)
        self.hist = np.zeros((S, HALO, 2), F32)

    def reset(self):
        self.g.reset()
        self.hist = np.zeros((self.S, HALO, 2), F32)

    def run(self, x):
        pts, self.hist = upsample(x, self.f, self.hist)
        self.g.run(pts)
        return self

    def close(self, r, dials=_gonio.DIALS):
        """the closing draw_rb of a track's r >= 64 remaining input frames (_gonio_ends): rms_c = r f, the attack pair of elapsed = r / rate"""
        assert r >= _gonio_ends.FLOOR and self.g.j == r * self.f
        d = self.g.d
        self.g.d = copy.copy(d)
        self.g.d.P, self.g.d.attack = r * self.f, _gonio_ends.attack(self.rate, r, dials)
        with np.errstate(all="ignore"):
            self.g._block_end()
        self.g.d = d
        self.g.j = 0
        return self

    def __getattr__(self, k):                                             # img, the counters, gain, lp0 .. : the inner goniometer's
        return getattr(self.__dict__["g"], k)


def run_ends(x, ends, rate, f, calls=None, **kw):
    """_gonio_ends.run behind the interpolator: x float32 [S, T, 2], ends [S] in 0 .. T (T: open), calls: the lengths the audio is cut into.
    One lock-step pass (the streams of the restatement are independent, and the interpolator is causal: a stream's state where it comes to
    stand is what its own frames alone give — track () is that, for the tests to hold a few streams to); the closing update of r input
    frames runs with rms_c = r f and the attack pair of r / rate."""
    GE = _gonio_ends
    x = np.asarray(x, F32)
    S, T = x.shape[0], x.shape[1]
    calls = list(calls) if calls else [T]
    assert sum(calls) == T and len(ends) == S
    g = GonioOS(S, rate, f, **kw)
    P = g.P
    at = [GE.stand(int(E), T, P, calls) for E in ends]
    o = GE.Ends()
    o.P, o.T, o.blocks = P, T, T // P
    o.img = np.zeros_like(g.img)
    for k in GE.STATE:
        setattr(o, k, np.zeros_like(getattr(g, k)))
    o.s_gain, o.s_drawn, o.s_clipped = np.zeros((S, o.blocks), F32), np.zeros((S, o.blocks), np.uint32), np.zeros((S, o.blocks), np.uint32)
    o.updates = np.zeros(S, np.uint64)
    o.stand = np.array([a[0] for a in at])
    o.r = np.array([a[1] for a in at])
    o.painted = np.zeros(S, bool)
    pos = 0
    for t in sorted(set(o.stand.tolist())):
        g.run(x[:, pos:t])
        pos = t
        idx = np.nonzero(o.stand == t)[0]
        whole = len(g.series)
        for k in GE.STATE:
            getattr(o, k)[idx] = getattr(g, k)[idx]
        o.img[idx] = g.img[idx]
        for b in range(min(whole, o.blocks)):
            o.s_gain[idx, b], o.s_drawn[idx, b], o.s_clipped[idx, b] = g.series[b][0][idx], g.series[b][1][idx], g.series[b][2][idx]
        o.updates[idx] = whole
        cl = idx[o.r[idx] > 0]
        if cl.size:
            r = int(o.r[cl[0]])
            assert (o.r[cl] == r).all() and r >= GE.FLOOR
            h = _gonio.Gonio(cl.size, rate, **kw)
            for k in GE.STATE:
                setattr(h, k, getattr(o, k)[cl].copy())
            h.d = copy.copy(g.g.d)
            h.d.P, h.d.attack = r * g.f, GE.attack(rate, r, kw.get("dials", _gonio.DIALS))
            with np.errstate(all="ignore"):
                h._block_end()
            pg, pd, pc = h.series[-1]
            o.painted[cl] = pd > 0
            for k in GE.STATE:
                getattr(o, k)[cl] = getattr(h, k)
            if whole < o.blocks:
                o.s_gain[cl, whole], o.s_drawn[cl, whole], o.s_clipped[cl, whole] = pg, pd, pc
            o.updates[cl] += 1
    return o


def track(x1, stand, r, rate, f, **kw):
    """one track alone: x1 float32 [T, 2], fed the `stand` frames in front of where it comes to stand and no other, then its closing update"""
    g = GonioOS(1, rate, f, **kw).run(np.asarray(x1, F32)[None, :stand])
    if r:
        g.close(r, kw.get("dials", _gonio.DIALS))
    return g
