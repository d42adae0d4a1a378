"""sur_run (src/surmeter.c:115-147) composed from the oracle's Kmeterdsp and Stcorrdsp restatements (mo_kmeter_*, mo_stcorr_*, held
bit-identical to the reference's objects by tests/test_needle_oracle_vs_ref.py), the float64 restatements of the same recurrences the
GPU tests measure the reference's own rounding with, and the signals of the surround tests.

Per block: four (three on 3 channels) mo_stcorr_process + read on the pairs' channels, then C x (mo_kmeter_process, mo_kmeter_read) —
the order of sur_run."""
import ctypes as C

import numpy as np

F = C.c_float
FLOOR = 4.0 * 2.0 ** -23
E20, E10 = np.float32(1e-20), np.float32(1e-10)


class Stcorr(C.Structure):
    _fields_ = [(n, F) for n in ("zl", "zr", "zlr", "zll", "zrr", "w1", "w2")]

    def state(self):
        return [self.zl, self.zr, self.zlr, self.zll, self.zrr]


class Kmeter(C.Structure):
    _fields_ = [("z1", F), ("z2", F), ("rms", F), ("peak", F), ("cnt", C.c_int), ("fpp", C.c_int), ("fall", F), ("flag", C.c_int),
                ("hold", C.c_int), ("fsamp", F), ("omega", F)]


def bind(lib_or_path):
    """a handle of its own on the oracle library (the session's keeps its argtypes)"""
    lib = C.CDLL(lib_or_path if isinstance(lib_or_path, str) else lib_or_path._name)
    lib.mo_stcorr_init.argtypes = [C.POINTER(Stcorr), C.c_int, F, F]
    lib.mo_stcorr_init.restype = None
    lib.mo_stcorr_process.argtypes = [C.POINTER(Stcorr), C.POINTER(F), C.POINTER(F), C.c_int]
    lib.mo_stcorr_process.restype = None
    lib.mo_stcorr_read.argtypes = [C.POINTER(Stcorr)]
    lib.mo_stcorr_read.restype = F
    lib.mo_kmeter_init.argtypes = [C.POINTER(Kmeter), F]
    lib.mo_kmeter_init.restype = None
    lib.mo_kmeter_process.argtypes = [C.POINTER(Kmeter), C.POINTER(F), C.c_int]
    lib.mo_kmeter_process.restype = None
    lib.mo_kmeter_read.argtypes = [C.POINTER(Kmeter), C.POINTER(F), C.POINTER(F)]
    lib.mo_kmeter_read.restype = None
    return lib


def n_pairs(nch):
    return 4 if nch > 3 else 3


def clamp_pairs(nch, a, b):
    """surmeter.c:124-125"""
    return tuple(min(int(v), nch - 1) for v in a), tuple(min(int(v), nch - 1) for v in b)


def default_pairs(nch):
    """the surround8 port defaults (lv2ttl/surmeter.h), clamped"""
    return clamp_pairs(nch, (0, 2, 4, 6), (1, 3, 5, 7))


def _fp(a):
    return a.ctypes.data_as(C.POINTER(F))


class SurRun:
    """one stream's plugin instance: C Kmeterdsp, four Stcorrdsp"""

    def __init__(self, lib, fs, nch, pairs=None):
        self.lib, self.nch, self.fs = lib, nch, float(fs)
        self.km = [Kmeter() for _ in range(nch)]
        self.sc = [Stcorr() for _ in range(4)]
        for k in self.km:
            lib.mo_kmeter_init(C.byref(k), float(fs))
        for c in self.sc:
            lib.mo_stcorr_init(C.byref(c), int(fs), 2e3, 0.3)
        self.pairs = clamp_pairs(nch, *pairs) if pairs else default_pairs(nch)

    def set_pairs(self, a, b):
        self.pairs = clamp_pairs(self.nch, a, b)

    def run(self, x, read=True):
        """x [n, C] float32.  (level [C], peak [C], corr [4], states [4, 5]); read False: the host does not read the K-meters' ports
        after this block (the rms maximum is not re-armed: Kmeterdsp's _flag rule) — the values are then only peeked at"""
        n = x.shape[0]
        ch = [np.ascontiguousarray(x[:, c]) for c in range(self.nch)]
        corr = np.zeros(4, np.float32)
        for p in range(n_pairs(self.nch)):
            a, b = self.pairs[0][p], self.pairs[1][p]
            self.lib.mo_stcorr_process(C.byref(self.sc[p]), _fp(ch[a]), _fp(ch[b]), n)
            corr[p] = self.lib.mo_stcorr_read(C.byref(self.sc[p]))
        level, peak = np.zeros(self.nch, np.float32), np.zeros(self.nch, np.float32)
        for c in range(self.nch):
            self.lib.mo_kmeter_process(C.byref(self.km[c]), _fp(ch[c]), n)
            if read:
                m, q = F(), F()
                self.lib.mo_kmeter_read(C.byref(self.km[c]), C.byref(m), C.byref(q))
                level[c], peak[c] = m.value, q.value
            else:
                level[c], peak[c] = self.km[c].rms, self.km[c].peak
        return level, peak, corr, np.array([c.state() for c in self.sc], np.float32)


def run_oracle(lib, fs, x, ends, pairs=None, reads=None):
    """x [T, C]: one sur_run per block [ends [i - 1], ends [i]).  pairs: None, one (a, b), or one per block.  reads: the blocks after
    which the host reads the ports (None: all).  Returns level [B, C], peak [B, C], corr [B, 4], states [B, 4, 5]."""
    o = SurRun(lib, fs, x.shape[1])
    out, pos = [], 0
    for i, e in enumerate(ends):
        if pairs is not None:
            o.set_pairs(*(pairs[i] if isinstance(pairs, list) else pairs))
        out.append(o.run(x[pos:e], reads is None or i in reads))
        pos = e
    return tuple(np.array([r[k] for r in out], np.float32) for k in range(4))


# ---- the float64 restatements ---------------------------------------------------------------------------------------------------------

def onepole(u, r, y0):
    """y [n] = r y [n - 1] + u [n] along the last axis in float64, y [-1] = y0 (shape of u without the last axis): runs of 16 by a
    prefix sum (|r|^-16 < 1e4 down to 8 kHz: twelve digits kept), the runs chained one by one"""
    u = np.asarray(u, np.float64)
    T, L = u.shape[-1], 16
    if T == 0:
        return u.copy()
    nb = (T + L - 1) // L
    pad = np.zeros(u.shape[:-1] + (nb * L,))
    pad[..., :T] = u
    pad = pad.reshape(u.shape[:-1] + (nb, L))
    k = np.arange(L)
    with np.errstate(invalid="ignore", over="ignore"):
        yb = np.cumsum(pad * r ** -k.astype(np.float64), axis=-1) * r ** k.astype(np.float64)
        carry = np.empty(u.shape[:-1] + (nb,))
        c = np.asarray(y0, np.float64).copy()
        rl = r ** L
        for b in range(nb):
            carry[..., b] = c
            c = rl * c + yb[..., b, -1]
        y = yb + carry[..., None] * r ** (k + 1.0)
    return y.reshape(u.shape[:-1] + (nb * L,))[..., :T]


class ExactPairs:
    """Stcorrdsp's five updates in float64 for any number of (stream, pair) lanes at once, the flushes and + 1e-10f at the block ends"""

    def __init__(self, w1, w2, lanes):
        self.w1, self.w2 = float(w1), float(w2)
        self.z = np.zeros((5,) + tuple(lanes))

    def run(self, l, r):
        """l, r [..., n] float32: (reading, states [5, ...]) after the block"""
        w1, w2 = self.w1, self.w2
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            zl = onepole(w1 * l.astype(np.float64) + float(E20), 1.0 - w1, self.z[0])
            zr = onepole(w1 * r.astype(np.float64) + float(E20), 1.0 - w1, self.z[1])
            z = [zl[..., -1], zr[..., -1]]
            for j, p in enumerate((zl * zr, zl * zl, zr * zr)):
                z.append(onepole(w2 * p, 1.0 - w2, self.z[2 + j])[..., -1])
            z = [np.where(np.isfinite(v), v, 0.0) for v in z]
            for j in (2, 3, 4):
                z[j] = z[j] + float(E10)
            self.z = np.array(z)
            return z[2] / np.sqrt(z[3] * z[4] + float(E10)), self.z.copy()


class ExactLevels:
    """Kmeterdsp's two poles in float64 for any number of (stream, channel) lanes, the f32 roundings (clamp, NaN rule, + 1e-20f,
    sqrtf (2 z2), the _flag rule) at the block ends.  The peak is not restated: it is exact in the oracle."""

    def __init__(self, fs, lanes):
        self.w = float(np.float32(9.72) / np.float32(fs))
        self.z1 = np.zeros(lanes, np.float32)
        self.z2 = np.zeros(lanes, np.float32)
        self.rms = np.zeros(lanes, np.float32)
        self.flag = np.zeros(lanes, bool)

    def run(self, x, read=True):
        """x [..., n] float32: the level port after the block"""
        w = self.w
        n4 = x.shape[-1] // 4 * 4
        with np.errstate(invalid="ignore", over="ignore"):
            s = (x[..., :n4] * x[..., :n4]).astype(np.float64)
            z1 = np.clip(self.z1, 0, 50).astype(np.float64)
            z2 = np.clip(self.z2, 0, 50).astype(np.float64)
            if n4:
                y1 = onepole(w * s, 1.0 - w, z1)
                y2 = onepole(4.0 * w * y1[..., 3::4], 1.0 - 4.0 * w, z2)
                z1, z2 = y1[..., -1], y2[..., -1]
                # a square that is not finite: Inf - Inf at the next frame makes the reference's z1 NaN, unless it was the last one
                bad = ~np.isfinite(s[..., :-1]).all(axis=-1)
                z1, z2 = np.where(bad, np.nan, z1), np.where(bad, np.nan, z2)
            f1, f2 = z1.astype(np.float32), z2.astype(np.float32)
            f1, f2 = np.where(np.isnan(f1), np.float32(0), f1), np.where(np.isnan(f2), np.float32(0), f2)
            self.z1, self.z2 = f1 + E20, f2 + E20
            r = np.sqrt(np.float32(2) * f2)
        self.rms = np.where(self.flag | (r > self.rms), r, self.rms).astype(np.float32)
        self.flag = np.full(self.flag.shape, bool(read))
        return self.rms.copy()


def scale_of(st):
    """what a pair state's distance is relative to: its own value, for zlr sqrt (zll zrr); st [..., 5]"""
    s = np.abs(np.asarray(st, np.float64)).copy()
    s[..., 2] = np.sqrt(s[..., 3] * s[..., 4])
    return s


def rel(got, want, scale):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(scale > 0, np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)) / scale, 0.0)


def run_exact(fs, w12, x, ends, pairs=None, reads=None):
    """x [S, T, C]: the float64 restatement of run_oracle for all streams at once: level [B, S, C], corr [B, S, 4], states [B, S, 4, 5]"""
    S, T, nch = x.shape
    npair = n_pairs(nch)
    ex_p = ExactPairs(w12[0], w12[1], (S, npair))
    ex_l = ExactLevels(fs, (S, nch))
    xt = np.ascontiguousarray(x.transpose(0, 2, 1))                   # [S, C, T]
    lv, co, st, pos = [], [], [], 0
    cur = default_pairs(nch)
    for i, e in enumerate(ends):
        if pairs is not None:
            cur = clamp_pairs(nch, *(pairs[i] if isinstance(pairs, list) else pairs))
        blk = xt[:, :, pos:e]
        c, z = ex_p.run(blk[:, list(cur[0][:npair])], blk[:, list(cur[1][:npair])])
        cc, zz = np.zeros((S, 4)), np.zeros((S, 4, 5))
        cc[:, :npair], zz[:, :npair] = c, np.moveaxis(z, 0, -1)
        co.append(cc); st.append(zz)
        lv.append(ex_l.run(blk, reads is None or i in reads))
        pos = e
    return np.array(lv), np.array(co), np.array(st)


# ---- signals --------------------------------------------------------------------------------------------------------------------------

NAMES = ["independent", "copies", "halves", "mixes", "sines", "mixes at 1e-4", "quiet"]


def signals(T, fs, nch, seed=500, S=7):
    """S <= 7 streams of nch channels on the signal of tests/test_gpu_stcorr.py (uniform noise under a 0.7 Hz envelope).  In every
    stream channel 0 is noise (stream 4: a 440 Hz sine); the others are, in turn, a copy of channel 0, -0.5 x channel 0, 0.6 x channel 0
    + 0.4 x fresh noise, silence, the mix at 1e-4, fresh noise, a 440 Hz sine one radian on — rotated by the stream's number, so that
    every kind meets every pair position.  Stream 5 is stream 3 at 1e-4; stream 6 holds silence in all but two channels."""
    rng = np.random.default_rng(seed)
    t = np.arange(T) / fs
    env = (0.05 + 0.6 * (0.5 + 0.5 * np.sin(2 * np.pi * t * 0.7 + 1.0))).astype(np.float32)

    def noise():
        return rng.uniform(-1, 1, T).astype(np.float32) * env
    x = np.zeros((7, T, nch), np.float32)
    for s in range(7):
        base = noise() if s != 4 else (0.5 * np.sin(2 * np.pi * 440.0 * t)).astype(np.float32)
        mix = np.float32(0.6) * base + np.float32(0.4) * noise()
        kinds = [base.copy(), np.float32(-0.5) * base, mix, np.zeros(T, np.float32), mix * np.float32(1e-4), noise(),
                 (0.5 * np.sin(2 * np.pi * 440.0 * t + 1.0)).astype(np.float32)]
        x[s, :, 0] = base
        for c in range(1, nch):
            x[s, :, c] = kinds[(c - 1 + s) % len(kinds)]
    x[5] = x[3] * np.float32(1e-4)
    x[6, :, 2:] = 0
    return np.ascontiguousarray(x[:S])
