"""The gate kernels' yardstick: a plain numpy restatement of the once-per-fragment part of Ebu_r128_proc::process
(ebumeter/ebu_r128_proc.cc:217-244; oracle/mtr_oracle.c:206-241 is the oracle's copy), and the programmes that drive it to its edges.

The restatement (Gate) is fed call by call, either with the fragment powers of a call (call_powers: loudness, then bookkeeping) or
with the (M, S) series of a call (call_ms: bookkeeping only — IEEE float32 arithmetic on given floats, no libm).  Every float is
computed as mtr_gate.hip computes it: sequential float32 sums oldest first, the division and the log10 in double rounded back to
float32, `10 *` and `+ (-0.6976f)` in float32, the bin `floorf (10 v + 700.5f)` with the product rounded before the sum.
tests/test_gate_model_cpu.py anchors it to the oracle; tests/test_gpu_gate_exact.py holds the kernels to it with no bin-flip allowance.

The programmes: a 997 Hz sine at 8 kHz (fragments of 400 frames), the right channel 0.7 x the left, the amplitude piecewise constant
over whole fragments.  NFRAG is 850, not 700: the call cuts of the GPU tests (0, 1, 9, 10, 11, 3, 255, 256, 257 fragments, then the
rest) need 802 fragments before the rest begins.
"""
import numpy as np

HIST_LEN = 751
FS, FRAG, NFRAG = 8000.0, 400, 850
TAIL = 177                                     # frames behind the last whole fragment: a stream never ends on a fragment boundary
# the oracle rounds glibc's log10f, the kernels and this model a double log10: at most one float32 ulp of a logarithm whose magnitude
# stays under 32, times ten
ULP_DB = float(10 * np.spacing(np.float32(32)))          # 3.8e-5 dB
CALL_FRAGS = (0, 1, 9, 10, 11, 3, 255, 256, 257)         # fragments completed per call, then the rest
CALL_ODD = (151, 233, 101, 299, 157, 263, 111, 287, 203)  # frames behind the last completed fragment where each of those calls ends


def _f32(a):
    return np.asarray(a, np.float32)


def loudness(history, powers):
    """(M, S) float32 [n] of the n fragment powers of a call behind the 64 powers of `history` (oldest first): addfrags (8) and
    addfrags (60) of ebu_r128_proc.cc:251-260 with the clamp of :226-233, vectorised over the fragments"""
    p = np.concatenate([_f32(history)[-64:], _f32(powers)])
    n = p.size - 64
    at = 64 + np.arange(n)
    out = []
    for k in (8, 60):
        s = np.zeros(n, np.float32)
        for i in range(k - 1, -1, -1):
            s = s + p[at - i]                                          # float32, oldest first
        with np.errstate(divide="ignore", invalid="ignore"):
            q = (s.astype(np.float64) / k).astype(np.float32)
            lg = np.log10(q.astype(np.float64)).astype(np.float32)
            v = np.float32(10) * lg + np.float32(-0.6976)
        v[~np.isfinite(v) | (v < np.float32(-200))] = np.float32(-200)
        out.append(v)
    return out[0], out[1]


def bins(v):
    """floorf (10 v + 700.5f) of ebu_r128_proc.cc:70 as int64; product and sum rounded to float32 one after the other"""
    return np.floor(np.float32(10) * _f32(v) + np.float32(700.5)).astype(np.int64)


class Gate:
    """One stream's Ebu_r128_proc from the fragment powers on, after reset ()."""

    def __init__(self):
        self.ring = np.zeros(64, np.float32)
        self.hist = np.zeros((2, HIST_LEN), np.int32)
        self.count = np.zeros(2, np.int64)
        self.error = np.zeros(2, np.int64)
        self.wraps = np.zeros(2, np.int64)                            # how often div1 / div2 wrapped: points offered to addpoint
        self.div1 = self.div2 = 0
        self.max_M = self.max_S = self.last_M = self.last_S = np.float32(-200)
        self.snap_hist = np.zeros((2, HIST_LEN), np.int32)             # the histograms as calc_integ / calc_range last saw them
        self.snap_count = np.zeros(2, np.int64)
        self.evaluations = 0                                           # fragments at which div2 wrapped so far

    def call_powers(self, powers, integr=True):
        M, S = loudness(self.ring, powers)
        self.ring = np.concatenate([self.ring, _f32(powers)])[-64:]
        return self.call_ms(M, S, integr)

    def _add(self, which, v):
        k = bins(v)
        k = k[k >= 0]                                                  # under -70: dropped, not counted
        self.error[which] += int((k > 750).sum())
        np.add.at(self.hist[which], np.minimum(k, 750), 1)
        self.count[which] += k.size

    def call_ms(self, M, S, integr=True):
        M, S = _f32(M), _f32(S)
        n = M.size
        evaluated = False
        if integr and n:
            f = np.arange(n)
            at_M = (self.div1 + f + 1) % 2 == 0
            at_S = (self.div2 + f + 1) % 10 == 0
            f_calc = int(f[at_S][-1]) if at_S.any() else -1
            # at a fragment the M point goes in first, then the S point, then calc_*: only the last evaluation of a call survives
            self._add(0, M[at_M & (f <= f_calc)])
            self._add(1, S[at_S & (f <= f_calc)])
            if f_calc >= 0:
                self.snap_hist, self.snap_count = self.hist.copy(), self.count.copy()
                self.evaluations += int(at_S.sum())
                evaluated = True
            self._add(0, M[at_M & (f > f_calc)])
            self._add(1, S[at_S & (f > f_calc)])
            self.wraps += (int(at_M.sum()), int(at_S.sum()))
            self.div1, self.div2 = (self.div1 + n) % 2, (self.div2 + n) % 10
        if n:                                                          # the max-holds move whether integrating or not
            self.max_M, self.max_S = max(self.max_M, M.max()), max(self.max_S, S.max())
            self.last_M, self.last_S = M[-1], S[-1]
        return dict(M=M, S=S, hist_M=self.hist[0].copy(), hist_S=self.hist[1].copy(), count=self.count.copy(), error=self.error.copy(),
                    wraps=self.wraps.copy(), max_M=self.max_M, max_S=self.max_S, last_M=self.last_M, last_S=self.last_S,
                    snap_M=self.snap_hist[0].copy(), snap_S=self.snap_hist[1].copy(), snap_count=self.snap_count.copy(),
                    evaluated=evaluated, evaluations=self.evaluations)


def expected(snap_M, snap_S):
    """dict(I, I_thr, Rmin, Rmax, R_thr, g_I, g_R) of the histograms calc_integ / calc_range last saw: meters.lv2_amd.hist_loudness
    (held bit for bit against the oracle's mo_hist_calc_* by tests/test_abi_cpu.py), -200 where a count is under 50 / 20 (a count
    never falls, so no earlier evaluation can have set them).  g_I = 10 (I_thr + 10) + 0.5 and g_R = 10 (R_thr + 20) + 0.5 are the
    arguments of the floorf that picks the gate bin (NaN where there is none)."""
    import meters.lv2_amd as m
    I, It, r0, r1, Rt = [np.float32(v) for v in m.hist_loudness(snap_M, snap_S)]
    g_I = 10 * (float(It) + 10) + 0.5 if int(np.sum(snap_M)) >= 50 else float("nan")
    g_R = 10 * (float(Rt) + 20) + 0.5 if int(np.sum(snap_S)) >= 20 else float("nan")
    return dict(I=I, I_thr=It, Rmin=r0, Rmax=r1, R_thr=Rt, g_I=g_I, g_R=g_R)


# ---- the programmes ----------------------------------------------------------------------------------------------------------------

# a sine of amplitude A, the right channel 0.7 A: -0.691 + 10 log10 (1.49 A^2 / 2) = 20 log10 A - 1.97 LUFS where the K-filter's gain
# is 0 dB; at 997 Hz of an 8 kHz stream the filter adds 0.574 dB (measured: tests/test_gate_model_cpu.py prints the steady stream's level)
LUFS_OF_UNIT_SINE = -1.3957
NAMES = ("steady", "up", "down", "gate_i", "gate_both", "floor", "over", "late", "narrow") + tuple("fuzz%d" % k for k in range(8)) + ("zeros",)


def _amp(lufs):
    return 10.0 ** ((np.asarray(lufs, np.float64) - LUFS_OF_UNIT_SINE) / 20)


def amplitudes(name, n=NFRAG):
    """the amplitude of each of n fragments, float64 [n]"""
    f = np.arange(n)
    if name == "steady":
        return np.full(n, _amp(-23.0))
    if name == "up":                                   # 0.1 dB per 5 fragments, 14 dB, repeated: from under -30 to over -20 LUFS
        return _amp(-31.0 + 0.1 * ((f // 5) % 140))
    if name == "down":
        return _amp(-17.0 - 0.1 * ((f // 5) % 140))
    if name == "gate_i":                               # quiet sections 15 dB below: cut by the -10 dB gate, kept by the -20 dB one
        return _amp(np.where((f // 100) % 2 == 0, -20.0, -35.0))
    if name == "gate_both":                            # 25 dB below: cut by both
        return _amp(np.where((f // 100) % 2 == 0, -20.0, -45.0))
    if name == "floor":                                # around -66 LUFS with stretches under -70: the gate bin k < 0 -> 0, points dropped
        return _amp(np.where(f % 100 < 60, -66.0, -75.0))
    if name == "over":                                 # stretches at amplitude 3 .. 4 (over +5 LUFS): bin 750, the error counts
        return np.where(f % 200 >= 120, 3.0 + (f % 200 - 120) / 80.0, _amp(-10.0))
    if name == "late":                                 # digital silence first: the counts pass 50 / 20 late
        return np.where(f < 200, 0.0, _amp(np.where((f // 30) % 2 == 0, -23.0, -26.0)))
    if name == "narrow":                               # the run-in of the 8- and 60-fragment windows falls under -70 and is dropped: every point in one or two bins
        return np.full(n, _amp(-69.9))
    if name.startswith("fuzz"):                        # a level per fragment, uniform in dB over [-80, +12] re full scale
        return 10.0 ** (np.random.default_rng(7000 + int(name[4:])).uniform(-80.0, 12.0, n) / 20)
    if name == "zeros":
        return np.zeros(n)
    raise KeyError(name)


def audio(amps, frag=FRAG, fs=FS, tail=TAIL):
    """float32 [n frag + tail, 2]: the sine with the amplitude of amps per fragment (the last one over the tail)"""
    amps = np.asarray(amps, np.float64)
    T = amps.size * frag + tail
    t = np.arange(T)
    a = amps[np.minimum(t // frag, amps.size - 1)]
    left = a * np.sin(2 * np.pi * 997.0 * t / fs)
    x = np.empty((T, 2), np.float32)
    x[:, 0] = left
    x[:, 1] = 0.7 * left
    return x


_BATCH = {}


def batch(names=NAMES, n=NFRAG, frag=FRAG, fs=FS, tail=TAIL):
    """float32 [len (names), n frag + tail, 2], built once and read-only"""
    key = (tuple(names), n, frag, fs, tail)
    if key not in _BATCH:
        x = np.stack([audio(amplitudes(nm, n), frag, fs, tail) for nm in names])
        x.setflags(write=False)
        _BATCH[key] = x
    return _BATCH[key]


def call_ends(total_frames, frag=FRAG, call_frags=CALL_FRAGS, odd=CALL_ODD):
    """the frame at which each call ends: the fragments completed per call run call_frags, no cut on a fragment boundary, then the rest"""
    ends, done = [], 0
    for k, o in zip(call_frags, odd):
        done += k
        ends.append(done * frag + o)
    assert ends[-1] < total_frames and all(b > a for a, b in zip(ends, ends[1:]))
    return ends + [total_frames]


# ---- coverage: the programmes provably reach the edges -------------------------------------------------------------------------------

def gate_bin(g, base):
    return max(int(np.floor(g)) + base, 0)


def assert_coverage(rec):
    """rec [name] = dict(hist_M, hist_S, count (2), wraps (2), I_thr, R_thr, Rmin, Rmax) of a stream's final record, plus
    rec ["late"]["counts_per_call"] = [(count_M, count_S)] after every call of call_ends ()."""
    r = rec["floor"]                                    # the integrated-loudness gate bin clamped at 0, points dropped under bin 0
    assert r["count"][0] >= 50 and np.floor(10 * (float(r["I_thr"]) + 10) + 0.5) + 600 < 0, r["I_thr"]
    assert 0 < r["count"][0] < r["wraps"][0] and 0 < r["count"][1] < r["wraps"][1], (r["count"], r["wraps"])
    r = rec["over"]                                     # points in bin 750
    assert r["hist_M"][750] > 0 and r["hist_S"][750] > 0
    for nm in ("up", "down"):
        r = rec[nm]
        occ = np.flatnonzero(r["hist_M"])               # more than 64 occupied M bins over two centuries
        assert occ.size > 64 and occ[-1] // 100 > occ[0] // 100, (nm, occ.size)
        occ = np.flatnonzero(r["hist_S"])
        assert occ.size > 40 and occ[-1] // 100 > occ[0] // 100, (nm, occ.size)
        # the percentile walks take a second 64-bin window: the 10 % point lies more than 64 bins above the gate bin, the 95 % point
        # more than 64 bins under bin 750
        k = gate_bin(10 * (float(r["R_thr"]) + 20) + 0.5, 500)
        i, j = int(round(float(r["Rmin"]) * 10)) + 701, int(round(float(r["Rmax"]) * 10)) + 699
        assert i - k > 64 and 750 - j > 64, (nm, k, i, j)
    r = rec["narrow"]                                   # all points in at most two bins
    assert r["count"][0] >= 50 and r["count"][1] >= 20
    assert np.count_nonzero(r["hist_M"]) <= 2 and np.count_nonzero(r["hist_S"]) <= 2
    r = rec["gate_i"]                                   # the quiet sections: under the -10 dB gate, over the -20 dB one
    q = np.flatnonzero(r["hist_S"])[0]
    assert q >= gate_bin(10 * (float(r["R_thr"]) + 20) + 0.5, 500) and np.flatnonzero(r["hist_M"])[0] < gate_bin(10 * (float(r["I_thr"]) + 10) + 0.5, 600)
    r = rec["gate_both"]
    assert np.flatnonzero(r["hist_S"])[0] < gate_bin(10 * (float(r["R_thr"]) + 20) + 0.5, 500)
    r = rec["zeros"]
    assert r["count"][0] == 0 and r["count"][1] == 0
    c = np.asarray(rec["late"]["counts_per_call"])      # the 50-point and 20-point minima crossed between two calls that both evaluate
    assert ((c[:-1, 0] > 0) & (c[:-1, 0] < 50) & (c[1:, 0] >= 50)).any(), c
    assert ((c[:-1, 1] > 0) & (c[:-1, 1] < 20) & (c[1:, 1] >= 20)).any(), c
