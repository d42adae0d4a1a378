"""DR-14 restated in plain numpy (src/dr14.c:283-352 dr14_calc_rms_score, :394-412 the per-sample loop of dr14_run, as
oracle/mtr_oracle.c restates them: dr14_window, mo_dr14_run), and the inputs of tests/test_dr14_cpu.py and tests/test_gpu_dr14_score.py.

run () takes ONE stream [T] or [T, 2], the rate and the call lengths, and returns a Reading after every call plus every closed window.
Two ways to add a window's squares (the squares themselves are f32 products, as in the reference and in the kernel):
  "f64": the sum of every piece (the part of a window inside one call) in double, added in double to the carry, the carry rounded to
         f32 — what k_dr14_sums / k_dr14_windows do;
  "f32": one f32 accumulator, sample after sample (np.cumsum with dtype float32), as the reference does.
Everything behind the sum is float32 in the reference's order.

The score is discontinuous in the histogram's bins: one window in the neighbouring 0.01 dB bin can change which bins the cut takes.
checked () therefore asserts, for given inputs, that both modes put every window into the same bin and that no window lies within
EDGE_MARGIN of a bin edge — the tests compare nothing before that holds."""
import collections
import functools

import numpy as np

F = np.float32
HISTBINS = 8000
SILENT = -2                 # "bin" of a window that the silence test dropped (a window without a bin has -1, a dropped one 0)
EDGE_MARGIN = 1e-3          # bins: about 2e-6 relative in power, ten times what a handful of f32 roundings of the carry can move

# m_rms, m_peak, dr, dr_total against this restatement, dB.  With equal bins what is left is libm: powf / log10f / sqrtf of the device
# against the host's are a few ulp on at most 16 terms and values up to 80; 1e-4 dB is 1/100 of a bin.
# Measured worst: restatement against mo_dr14_run (CPU) 7.63e-06 dB; the kernels against the restatement (MI355X) 1.53e-05 dB.
TOL_SCORE = 1e-4

Reading = collections.namedtuple("Reading", "m_rms m_peak dr dr_total block_count num_fragments m_cut n_cut chunks left hist peak_hist")
Run = collections.namedtuple("Run", "readings bins")


def window(fs):
    """frames that close a window: n_sample_cnt + 1 (dr14.c:155, :404)"""
    return int(np.rint(F(fs) * F(3.0))) + 1


def coeff_to_db(c):                                                 # dr14.c:235-238
    return F(-80) if float(c) < .0001 else F(20) * np.log10(F(c))


def db_to_coeff(db):                                                # dr14.c:240-243 (0.05 * db is a double product, powf takes its float)
    return F(0) if db <= -80 else np.power(F(10), F(0.05 * float(F(db))))


def _score(hist, nf):
    """the cut of dr14_calc_rms_score for one channel: (m_rms, m_cut, n_cut, 64-bin chunks from the top down to the last bin it took,
    occupied bins it left in that chunk)"""
    m_cut = max(1, int(np.floor(F(nf / 5.0))))
    n_cut, score, low, left = 0, F(0), HISTBINS - 1, 0
    if nf > 2:
        for b in (np.nonzero(hist[1:])[0] + 1)[::-1].tolist():      # b = 7999 ... 1, occupied bins only
            if n_cut >= m_cut:
                left += (HISTBINS - 1 - b) // 64 == (HISTBINS - 1 - low) // 64
                continue
            cd = db_to_coeff((b - HISTBINS + 1) / 100.0)
            score = F(score + F(cd * cd) * F(hist[b]))
            n_cut += int(hist[b])
            low = b
    m_rms = coeff_to_db(np.sqrt(F(score / F(n_cut)))) if n_cut > 0 else F(-81)
    return m_rms, m_cut, n_cut, (HISTBINS - 1 - low) // 64 + 1, left


def _ports(m_rms, m_peak, nf, C):
    """what dr14_run leaves on the ports (dr14.c:430-450)"""
    dr, total, valid = [], F(0), 0
    for c in range(C):
        rdb, pdb = m_rms[c], m_peak[c]
        d = (F(0) if 0 < pdb else pdb) - rdb
        ok = rdb > -80 and pdb > -80
        if ok:
            total = F(total + d)
            valid += 1
        dr.append(max(F(1), min(F(20), d)) if ok else F(21))
    dr_total = F(0)
    if C > 1:
        dr_total = max(F(1), min(F(20), F(total / F(valid)))) if valid > 0 else F(21)
    return dr, dr_total, F(3.0 * nf)


def run(x, fs, calls, mode="f64"):
    x = np.asarray(x, F)
    x = x[:, None] if x.ndim == 1 else x
    C, W = x.shape[1], window(fs)
    nsc = F(W - 1)
    rs, pk = [F(0)] * C, [F(0)] * C
    hist = np.zeros((C, HISTBINS), np.uint32)
    ph = np.zeros((C, 2), F)
    m_rms, m_peak = [F(-81)] * C, [F(-81)] * C
    stat = [[1, 0, 1, 0] for _ in range(C)]                         # (m_cut, n_cut, chunks, left) of the last score
    nf = scnt = pos = 0
    readings, bins = [], []
    for n in calls:
        end = pos + n
        while pos < end:
            p1 = min(end, pos + W - scnt)                           # the piece [pos, p1) of the open window
            for c in range(C):
                v = x[pos:p1, c]
                sq = v * v
                if mode == "f64":
                    rs[c] = F(np.float64(rs[c]) + sq.astype(np.float64).sum())
                else:
                    rs[c] = np.cumsum(np.concatenate(([rs[c]], sq)), dtype=F)[-1]
                pk[c] = max(pk[c], v.max())                         # signed, from 0 (dr14.c:401)
            scnt += p1 - pos
            pos = p1
            if scnt < W:
                break
            scnt = 0
            # ---- a window closes ----
            if not any(float(rs[c]) > 1e-9 * float(nsc) for c in range(C)):
                rs = [F(0)] * C                                     # (the peak stays)
                bins.append([SILENT] * C)
                continue
            nf += 1
            row = []
            for c in range(C):
                rms = np.sqrt(F(F(2) * rs[c]) / nsc)
                rs[c] = F(0)
                b = int(np.rint(F(100) * (F(80) + coeff_to_db(rms)))) - 1
                b = min(b, HISTBINS - 1)
                if b > 0:
                    hist[c, b] += 1
                row.append(b)
                m_rms[c], *stat[c] = _score(hist[c], nf)
                if pk[c] >= ph[c, 0]:
                    ph[c, 1], ph[c, 0] = ph[c, 0], pk[c]
                elif pk[c] > ph[c, 1]:
                    ph[c, 1] = pk[c]
                pk[c] = F(0)
                m_peak[c] = coeff_to_db(ph[c, 1]) if nf > 2 else F(-81)
            bins.append(row)
        dr, dr_total, blocks = _ports(m_rms, m_peak, nf, C)
        readings.append(Reading(list(m_rms), list(m_peak), dr, dr_total, blocks, nf, [s[0] for s in stat], [s[1] for s in stat],
                                [s[2] for s in stat], [s[3] for s in stat], hist.copy(), ph.copy()))
    return Run(readings, np.array(bins, np.int64).reshape(-1, C))


def levels(x, fs):
    """[whole windows, C] float64: 100 (80 + dB) of every whole window from its exact (double) sum, unclamped; and the window's sum
    over the silence threshold 1e-9 n_sample_cnt"""
    x = np.asarray(x, F)
    x = x[:, None] if x.ndim == 1 else x
    W = window(fs)
    n = x.shape[0] // W
    sq = (x[:n * W] * x[:n * W]).astype(np.float64).reshape(n, W, -1).sum(1)
    with np.errstate(divide="ignore"):
        d = 100.0 * (80.0 + 10.0 * np.log10(2.0 * sq / float(W - 1)))
    return d, sq / (1e-9 * float(W - 1))


def edge_distance(d):
    """distance (in bins) of 100 (80 + dB) from the nearest edge x.5 at which the window changes its bin; no edge below 0.5, none above 7999.5"""
    d = np.asarray(d, np.float64)
    with np.errstate(invalid="ignore"):
        inner = np.abs(d - np.floor(d) - 0.5)
    return np.where(d <= 0, 0.5 - d, np.where(d > HISTBINS - 0.5, d - (HISTBINS - 0.5), inner))


def checked(x, fs, calls):
    """The condition on the inputs, asserted; then (the f64 run, the f32 run)."""
    d, over = levels(x, fs)
    assert d.shape[0] == sum(calls) // window(fs)
    dist = edge_distance(d)
    loud = (over > 1).any(1)                                        # silent needs every channel under the threshold
    assert (np.abs(over.max(1) - 1) > 1e-3).all(), ("a window at the silence threshold", over.max(1))
    assert dist[loud].min(initial=1.0) > EDGE_MARGIN, ("a window within EDGE_MARGIN of a bin edge", np.argwhere(dist < EDGE_MARGIN), dist.min())
    a, b = run(x, fs, calls, "f64"), run(x, fs, calls, "f32")
    assert np.array_equal(a.bins, b.bins), ("f64 and sequential f32 sums disagree on a bin", np.argwhere(a.bins != b.bins))
    assert np.array_equal(a.bins == SILENT, np.repeat(~loud[:, None], a.bins.shape[1], 1))
    return a, b


# ---- the inputs of tests/test_dr14_cpu.py and tests/test_gpu_dr14_score.py ------------------------------------------------------------
# Uniform noise, window by window at a chosen level, at the lowest rates the engine takes: 8000 Hz (W = 24001, odd: window starts of
# both parities) and 8001 Hz (W = 24004, even).  Every stream is stereo; the mono tests take ONE channel of it (mono ()).  The seeds are
# chosen so that checked () holds for every stream (about one window in 300 lies within EDGE_MARGIN of an edge, or falls into another
# bin when summed in f32: tests/test_dr14_cpu.py::test_inputs_meet_the_condition says which, should a generator ever change).

RATES = (8000.0, 8001.0)
Case = collections.namedtuple("Case", "x calls names")             # x [S, T, 2]
MANY_SEEDS = {8000.0: (0, 1, 2, 3, 4, 5), 8001.0: (0, 1, 2, 3, 4, 5)}
SMALL_SEED = {8000.0: 0, 8001.0: 1}
EDGE_SEED = {8000.0: 0, 8001.0: 1}
MANY_WINDOWS, SMALL_WINDOWS, EDGE_WINDOWS = 46, 16, 8
NO_BIN = -270.0                                                    # 100 (80 + dB) of uniform noise of amplitude 9e-5: -82.7 dB, counted, no bin


def _calls(cuts):
    return np.diff([0] + sorted(set(cuts))).tolist()


def _level(v, W):
    return 100.0 * (80.0 + 10.0 * np.log10(2.0 * (v * v).astype(np.float64).sum() / float(W - 1)))


def _set_level(x, k, W, d):
    """scale window k of x [T, C] in place so that each channel's 100 (80 + dB) is d [C] (bisection on the f32 gain: the samples round)"""
    for c, want in enumerate(np.broadcast_to(d, x.shape[1])):
        seg = x[k * W:(k + 1) * W, c].copy()
        lo, hi = -8.0, 8.0                                          # log10 of the gain
        for _ in range(50):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if _level(seg * F(10.0 ** mid), W) < want else (lo, mid)
        x[k * W:(k + 1) * W, c] = seg * F(10.0 ** hi)
        assert abs(_level(x[k * W:(k + 1) * W, c], W) - want) < 0.05


def mono(case, channel=1):
    return Case(np.ascontiguousarray(case.x[:, :, channel:channel + 1]), case.calls, case.names)


@functools.lru_cache(maxsize=None)
def many_stream(fs, seed):
    """46 windows: levels from -50 to -6 dB (4400 bins), pairs inside one 64-bin chunk, one loudest window, the second-loudest
    segment three times over and another one twice (bins with a count of 3 and 2), three silent windows"""
    W, NW = window(fs), MANY_WINDOWS
    rng = np.random.default_rng([int(fs), seed, 14])
    x = rng.uniform(-1, 1, (NW * W + 100, 2)).astype(F)
    g = rng.uniform(-50, -6, (NW + 1, 2))
    g[6], g[21] = g[5] - 0.21, g[20] - 0.40                         # 21 and 40 bins below their neighbours
    g[3], g[8], g[14] = (-3.0, -3.5), (-5.0, -4.5), (-7.0, -6.2)
    g[4] = g[3] - 0.3                                               # in the loudest window's chunk: the walk stops above it
    for k in range(NW + 1):
        x[k * W:(k + 1) * W] *= (10.0 ** (g[k] / 20.0)).astype(F)
    for k, src in ((11, 8), (30, 8), (15, 14)):
        x[k * W:(k + 1) * W] = x[src * W:(src + 1) * W]
    for k in (2, 25, 26):
        x[k * W:(k + 1) * W] = 0
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def many_windows(fs):
    W = window(fs)
    x = np.stack([many_stream(fs, s) for s in MANY_SEEDS[fs]])
    T = x.shape[1]
    cuts = [W + 37, W + 38, 3 * W + 33, 4 * W, 5 * W - 1, 6 * W + 1, 6 * W + 2, 9 * W + 500, 12 * W + 7, 13 * W, 13 * W + 1,
            20 * W - 1, 20 * W, 31 * W + 5, 40 * W + 1, 45 * W + 3, T]
    return Case(x, _calls(cuts), ["many%d" % s for s in MANY_SEEDS[fs]])


@functools.lru_cache(maxsize=None)
def small(fs):
    """16 windows per stream: the level edges of the histogram, the loud end, the peaks"""
    W, NW = window(fs), SMALL_WINDOWS
    T = NW * W + 50
    rng = np.random.default_rng([int(fs), SMALL_SEED[fs], 15])
    out = {}

    def noise(d=None):
        x = rng.uniform(-1, 1, (T, 2)).astype(F)
        if d is not None:
            for k in range(NW + 1):
                _set_level(x, k, W, d)
        return x

    # fragments without a bin: all but two / all / bins 1 .. 63 only (the walk's last chunk) / bin 0 against bin 1
    x = noise(NO_BIN)
    _set_level(x, 4, W, (5000.3, 4800.3)); _set_level(x, 9, W, (4500.3, 4650.3))
    out["two_bins"] = x
    out["no_bin"] = noise(NO_BIN)
    x = noise(NO_BIN)
    for k in range(1, NW, 2):
        _set_level(x, k, W, rng.integers(3, 63, 2) + 0.3)
    _set_level(x, 3, W, (64.3, 2.3)); _set_level(x, 5, W, (64.3, 63.3))       # rint - 1: bins 63, 1, 63, 62
    out["last_chunk"] = x
    x = noise(NO_BIN)
    _set_level(x, 3, W, (1.0, 2.0)); _set_level(x, 6, W, (2.0, 1.0))                    # rint -> 1 / 2: bin 0 (dropped) / bin 1 (kept)
    out["bin_0_and_1"] = x
    # loud: two windows above 0 dB (amplitude 1.5: bin 7999 by the clamp, peaks above 1.0), one just under
    x = noise()
    for k in range(NW + 1):
        x[k * W:(k + 1) * W] *= (10.0 ** (rng.uniform(-20, -10, 2) / 20.0)).astype(F)
    for k, a in ((2, 1.5), (7, 1.5), (5, 1.2)):
        x[k * W:(k + 1) * W] = rng.uniform(-1, 1, (W, 2)).astype(F) * F(a)
    out["loud"] = x
    # a quiet RMS under two full-scale hits: dr clamps at 20
    x = noise() * F(0.01)
    x[W + 100], x[4 * W + 7] = (1.0, 0.9), (1.0, 1.0)
    x[6 * W + 9, 1] = 0.9
    out["dr_20"] = x
    # equal maxima in two windows (and a lower third)
    x = noise() * F(0.1)
    x[2 * W + 5], x[5 * W + 50], x[8 * W + 500] = (0.7, 0.6), (0.7, 0.6), (0.6, 0.6)
    out["tie"] = x
    # a channel that is never positive beside an ordinary one
    x = noise() * F(0.3)
    x[:, 1] = -np.abs(x[:, 1])
    out["negative"] = x
    # a silent window that holds a small positive spike: it outlives the window and tops the next window's own maximum
    x = noise() * F(0.003)
    x[6 * W:7 * W] *= F(3.0)
    x[3 * W:4 * W] = 0
    x[3 * W + 777, 1] = 0.004
    out["spike_in_silence"] = x
    for v in out.values():
        v.setflags(write=False)
    cuts = [2 * W + 11, 3 * W, 3 * W + 1, 5 * W + 3, 7 * W - 1, 10 * W + 1, 15 * W + 2, T]
    return Case(np.stack(list(out.values())), _calls(cuts), list(out))


def edge_cuts(fs, first):
    """calls whose first ends at `first` (W - 1, W or W + 1), then calls of 1 and 2 frames and cuts one frame either side of windows"""
    W = window(fs)
    return [first, first + 1, first + 3, 2 * W - 1, 2 * W + 1, 3 * W - 2, 3 * W, 3 * W + 2, 4 * W - 1, 4 * W, 4 * W + 1,
            5 * W + 1, 5 * W + 2, 6 * W - 1, 7 * W, EDGE_WINDOWS * W + 40]


@functools.lru_cache(maxsize=None)
def edge(fs):
    """noise at -60 dB under single spikes of 0.3 .. 0.6 that carry their windows' energy, on frames 0, W - 1, W, W + 1, kW - 1 and kW,
    and on the first and the last frame of every call of edge_cuts (); stream s has them in channel s >> 1"""
    W = window(fs)
    T = EDGE_WINDOWS * W + 40
    rng = np.random.default_rng([int(fs), EDGE_SEED[fs], 16])
    frames = {0, W - 1, W, W + 1} | {k * W - d for k in range(2, EDGE_WINDOWS) for d in (0, 1)}
    for first in (W - 1, W, W + 1):
        frames |= {c - d for c in edge_cuts(fs, first) for d in (0, 1) if c < T}
    frames = sorted(frames)
    x = rng.uniform(-1, 1, (4, T, 2)).astype(F) * F(1e-3)
    for s in range(4):
        x[s, frames, s >> 1] = rng.uniform(0.3, 0.6, len(frames)).astype(F)
    x.setflags(write=False)
    return x


def edge_case(fs, first):
    return Case(edge(fs), _calls(edge_cuts(fs, first)), ["edge%d" % s for s in range(4)])


def edge_mono(case):
    return Case(np.stack([case.x[s, :, s >> 1:(s >> 1) + 1] for s in range(4)]), case.calls, case.names)


def edge_lengths(fs):
    """track lengths that put a spike on the last metered frame and another on the first frame past the end"""
    W = window(fs)
    return [5 * W, 4 * W + 1, 3 * W, W + 1]


def frames_per_call(L, calls):
    """frames of every call for a stream of total length L (0 once it has ended)"""
    out, p = [], 0
    for n in calls:
        out.append(int(min(max(L - p, 0), n)))
        p += n
    return out
