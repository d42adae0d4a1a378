"""Kmeterdsp for a batch (MTR_METER_KMETER, mtr_kmeter.hip) against the restatement of jmeters/kmeterdsp.cc
(oracle mo_kmeter_*, itself bit-identical to the reference object: tests/test_needle_oracle_vs_ref.py).

One engine call = one Kmeterdsp::process () per channel.  The filter sums are re-associated (pieces of 4096
frames combined with powers of the transition matrix): 1e-5 relative on the RMS; the digital peak and its
hold / fall-back bookkeeping are exact.

Below the two tests that state this: the dense pair (k_kmeter_pieces / k_kmeter_final) at its own edges — groups of four
frames, 256 lanes, chunks of 32768 frames counted from the call's END, the 64-thread blocks of the final kernel — on
buffers of every geometry, at seven rates, through a call longer than the weights' double range, on samples that are not
finite, at the clamps and through the peak's bookkeeping.  1e-5 against the f32 restatement measures mostly that
restatement's own rounding (a stationary input stalls an f32 one-pole: 1.9e-4 on DC at 192 kHz), so wherever at most
one f32 store of the state lies inside the filter's memory — a call from a reset engine, or calls of a second and more —
the RMS is held TIGHT against the float64 yardstick mo_kmeter_process_f64 (tests/test_kmeter_cpu.py ties it to the
restatement): |rms - want| <= 4 * 2^-24 * want.  The count: the in-group weights u0 .. u2 carry at most three f32
roundings and the product with the square one more, four of 2^-24 on a term of z2, halved by the square root — two —
plus the cast of z2 to f32 and sqrtf, half an ulp of at most 2^-23 each — two more.  (Seen on an MI355X: at most 1.92,
in the 700 001-frame call; 1.74 at the edges, 1.42 over the rates.  Every test prints its figure.)  Sequences of short calls keep
1e-5 against the restatement: they are about the peak.  The peak is compared bit for bit everywhere."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
F = C.c_float


class Kmeter(C.Structure):
    _fields_ = [("z1", F), ("z2", F), ("rms", F), ("peak", F), ("cnt", C.c_int), ("fpp", C.c_int), ("fall", F),
                ("flag", C.c_int), ("hold", C.c_int), ("fsamp", F), ("omega", F)]


@pytest.fixture(scope="module")
def M():
    import meters.lv2_amd as m
    return m


def signal(n, seed, fs):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / fs
    env = (0.05 + 0.6 * (0.5 + 0.5 * np.sin(2 * np.pi * t * 0.7 + seed))).astype(np.float32)
    x = (rng.uniform(-1, 1, (n, 2)).astype(np.float32) * env[:, None])
    x[n // 3, 0] = 0.97                                         # a peak that is then held and falls back
    x[:, 1] *= np.float32(0.25)
    return x


@pytest.mark.parametrize("fs", [48000.0, 44100.0])
@pytest.mark.parametrize("chn", [2, 1])
def test_kmeter_batch_matches_the_restatement(M, oracle, fs, chn):
    lib = oracle.lib
    lib.mo_kmeter_init.argtypes = [C.POINTER(Kmeter), F]
    lib.mo_kmeter_process.argtypes = [C.POINTER(Kmeter), C.POINTER(F), C.c_int]
    lib.mo_kmeter_read.argtypes = [C.POINTER(Kmeter), C.POINTER(F), C.POINTER(F)]
    S = 5
    # call sizes: below one piece, not a multiple of four, several pieces, a repeat (fall-back multiplier
    # kept), a one-frame call (no group at all), a long one
    calls = [1024, 1023, 4096 * 3 + 6, 4096 * 3 + 6, 1, 3, int(fs * 2) + 1, 512, 512, 512]
    T = sum(calls)
    x = np.stack([signal(T, 300 + s, fs) for s in range(S)])
    read_after = {2, 3, 6, 9}                                   # the host reads now and then, not after every call
    with M.Engine(S, fs, M.METER_KMETER, n_channels=chn) as e:
        ks = [[Kmeter() for _ in range(chn)] for _ in range(S)]
        for s in range(S):
            for c in range(chn):
                lib.mo_kmeter_init(C.byref(ks[s][c]), fs)
        pos = 0
        for i, n in enumerate(calls):
            blk = x[:, pos:pos + n]
            e.process(blk if chn == 2 else np.ascontiguousarray(blk[:, :, 0]))
            for s in range(S):
                for c in range(chn):
                    ch = np.ascontiguousarray(blk[s, :, c])
                    lib.mo_kmeter_process(C.byref(ks[s][c]), ch.ctypes.data_as(C.POINTER(F)), n)
            pos += n
            if i in read_after:
                rms, peak = e.kmeter_read()
                for s in range(S):
                    for c in range(chn):
                        a, b = F(), F()
                        lib.mo_kmeter_read(C.byref(ks[s][c]), C.byref(a), C.byref(b))
                        assert abs(rms[s, c] - a.value) <= 1e-5 * max(a.value, 1e-3), (i, s, c, rms[s, c], a.value)
                        assert peak[s, c] == np.float32(b.value), (i, s, c, peak[s, c], b.value)
        e.kmeter_reset()
        rms, peak = e.kmeter_read()
        assert not rms.any() and not peak.any()


def test_kmeter_known_answer(M):
    """A full-scale sine reads 1.0 = 0 dB on a K-meter's RMS scale (the detector's sqrt (2 z2)) and peak 1.0."""
    fs, T = 48000.0, 48000 * 2
    t = np.arange(T) / fs
    x = np.sin(2 * np.pi * 1000.0 * t).astype(np.float32)
    with M.Engine(1, fs, M.METER_KMETER, n_channels=1) as e:
        e.process(x[None, :])
        rms, peak = e.kmeter_read()
    assert abs(rms[0, 0] - 1.0) < 1e-3 and abs(peak[0, 0] - 1.0) < 1e-4


# ---- the dense pair at its edges -------------------------------------------------------------------------------------------------------

TIGHT_ULPS = 4.0                      # |rms - want| <= 4 * 2^-24 * want (the module's docstring counts them)
CH = 32768                            # frames per workgroup of k_kmeter_pieces: 8192 groups of four, counted from the call's end


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def bind(lib):
    P = C.POINTER
    lib.mo_kmeter_init.argtypes = [P(Kmeter), F]
    lib.mo_kmeter_init.restype = None
    for f in (lib.mo_kmeter_process, lib.mo_kmeter_process_f64):
        f.argtypes = [P(Kmeter), P(F), C.c_int]
        f.restype = None
    lib.mo_kmeter_read.argtypes = [P(Kmeter), P(F), P(F)]
    lib.mo_kmeter_read.restype = None
    return lib


class Yard:
    """S x chn Kmeterdsp of the oracle: the f32 restatement, or the float64 yardstick"""

    def __init__(self, lib, fs, S, chn, f64):
        self.lib, self.S, self.chn = bind(lib), S, chn
        self.proc = lib.mo_kmeter_process_f64 if f64 else lib.mo_kmeter_process
        self.k = [[Kmeter() for _ in range(chn)] for _ in range(S)]
        for row in self.k:
            for k in row:
                lib.mo_kmeter_init(C.byref(k), fs)

    def process(self, blk, frames=None):
        """blk [S, n, >= chn]; frames: per-stream ends, 0 = no call at all (a host that stopped calling)"""
        for s in range(self.S):
            n = blk.shape[1] if frames is None else int(frames[s])
            if frames is not None and n == 0:
                continue
            for c in range(self.chn):
                ch = np.ascontiguousarray(blk[s, :n, c], np.float32)
                self.proc(C.byref(self.k[s][c]), ch.ctypes.data_as(C.POINTER(F)), n)

    def read(self, first=0, count=None):
        count = self.S - first if count is None else count
        rms, peak = np.zeros((count, self.chn), np.float32), np.zeros((count, self.chn), np.float32)
        for s in range(count):
            for c in range(self.chn):
                a, b = F(), F()
                self.lib.mo_kmeter_read(C.byref(self.k[first + s][c]), C.byref(a), C.byref(b))
                rms[s, c], peak[s, c] = a.value, b.value
        return rms, peak

    def field(self, name):
        return np.array([[getattr(k, name) for k in row] for row in self.k])


def run_yard(lib, fs, x, calls, f64=True):
    """(rms, peak) read after every call, x [S, T, chn]"""
    y, out, pos = Yard(lib, fs, x.shape[0], x.shape[2], f64), [], 0
    for n in calls:
        y.process(x[:, pos:pos + n])
        out.append(y.read())
        pos += n
    return out


def engine_read(e, chn, first=0, count=None):
    rms, peak = e.kmeter_read(first, count)
    return rms[:, :chn].copy(), peak[:, :chn].copy()


def run_engine(M, fs, x, calls):
    S, chn, out, pos = x.shape[0], x.shape[2], [], 0
    with M.Engine(S, fs, M.METER_KMETER, n_channels=chn) as e:
        for n in calls:
            e.process(x[:, pos:pos + n])
            out.append(engine_read(e, chn))
            pos += n
    return out


def hold_tight(tag, got, want):
    """the RMS against the float64 yardstick: its bits where that reads exactly 0 or Inf, TIGHT elsewhere.  Prints the figure first."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    edge = (want == 0) | ~np.isfinite(want)
    with np.errstate(all="ignore"):
        ulps = np.where(edge, 0.0, np.abs(got.astype(np.float64) - want.astype(np.float64)) / (2.0 ** -24 * want.astype(np.float64)))
    worst = float(ulps.max()) if ulps.size else 0.0
    print(f"{tag}: rms off the f64 yardstick by at most {worst:.3f} x 2^-24 of it (held to {TIGHT_ULPS:g})")
    assert np.array_equal(bits(got)[edge], bits(want)[edge]), (tag, got[edge], want[edge])
    assert worst <= TIGHT_ULPS, (tag, worst, np.argwhere(~(ulps <= TIGHT_ULPS)).tolist()[:8])


def same_bits(tag, got, want):
    assert np.array_equal(bits(got), bits(want)), (tag, np.argwhere(bits(got) != bits(want)).tolist()[:8], got, want)


EDGE_N = [1, 3, 4, 5, 7, 1020, 1024, 1031, 32767, 32768, 32769, 32772, 65535, 65541, 3 * 32768 + 1026]


def edge_frames(n):
    """where a call's largest sample can be mis-weighted or mis-counted: its first frame, the last frame Kmeterdsp takes, the n mod 4
    frames it drops, the first and the last frame of every workgroup's chunk (counted in groups from the call's end)"""
    Lg = n & ~3
    G = Lg // 4
    fr = {0} | set(range(Lg, n))
    if Lg:
        fr.add(Lg - 1)
    for c in range((G + CH // 4 - 1) // (CH // 4)):
        fr.add((G - min((c + 1) * (CH // 4), G)) * 4)
        fr.add((G - 1 - c * (CH // 4)) * 4 + 3)
    return sorted(fr)


@pytest.mark.parametrize("chn", [2, 1])
@pytest.mark.parametrize("n", EDGE_N)
def test_group_lane_and_chunk_edges(M, oracle, n, chn):
    """One call from a reset engine with the stream's largest sample at each edge frame in turn (three placements a run, one a stream)."""
    fs, S, lib = 48000.0, 3, bind(oracle.lib)
    base = np.stack([signal(n, 700 + s, fs)[:, :chn] for s in range(S)])
    where = edge_frames(n)
    assert where[0] == 0 and (n < 4 or (n & ~3) - 1 in where) and all(f in where for f in range(n & ~3, n))
    where += [where[-1]] * (-len(where) % S)
    with M.Engine(S, fs, M.METER_KMETER, n_channels=chn) as e:
        for r in range(0, len(where), S):
            x = base.copy()
            for s in range(S):
                x[s, where[r + s], (r + s) % chn] = np.float32(-1.5 if (r + s) & 1 else 1.5)
            if r:
                e.kmeter_reset()
            e.process(x)
            rms, peak = engine_read(e, chn)
            (wrms, wpeak), = run_yard(lib, fs, x, [n])
            tag = f"a: n {n} chn {chn} at {where[r:r + S]}"
            hold_tight(tag, rms, wrms)
            same_bits(tag + " peak", peak, wpeak)
            for s in range(S):                                  # (what the yardstick says anyway: a dropped frame is not the peak, :79)
                assert (peak[s, (r + s) % chn] == np.float32(1.5)) == (where[r + s] < (n & ~3)), (tag, s, peak)


def _padded(x, stride, shift):
    """x [S, T, chn] in a buffer of NaN: `shift` floats in front of stream 0, `stride` frames from stream to stream"""
    S, T, chn = x.shape
    flat = np.full(shift + S * stride * chn + 8, np.nan, np.float32)
    flat[shift:shift + S * stride * chn].reshape(S, stride, chn)[:, :T] = x
    return flat


@pytest.mark.parametrize("chn,S,mod4", [(2, 5, None), (1, 4, 1), (1, 4, 2), (1, 4, 3)])
def test_buffer_geometry(M, chn, S, mod4):
    """Strided buffers with NaN between the streams, the base off 16 bytes by one float, one frame, three floats: the 16-byte loads are
    taken stream by stream where they may be (stereo on an odd stride: every other stream), and never change a bit."""
    import torch
    fs, calls = 48000.0, [32768 + 1030, 4102]                     # (an even T: T + 37 is odd)
    T = sum(calls)
    stride = T + 37
    if mod4 is None:
        assert stride & 1
    else:
        stride += (mod4 - stride) % 4
        assert stride % 4 == mod4
    x = np.stack([signal(T, 720 + s, fs)[:, :chn] for s in range(S)])

    def run(flat, shift, stride):
        dev = torch.from_numpy(flat).cuda()
        out, pos = [], 0
        with M.Engine(S, fs, M.METER_KMETER, n_channels=chn) as e:
            for n in calls:
                e.process_device(dev.data_ptr() + 4 * (shift + pos * chn), n, stride)
                out.append(engine_read(e, chn))
                pos += n
        return out
    want = run(x.reshape(-1), 0, T)
    assert np.isfinite(want[1][0]).all() and (want[1][0] > 0).all()
    for shift in sorted({0, 1, chn, 3}):
        got = run(_padded(x, stride, shift), shift, stride)
        for i in range(len(calls)):
            same_bits(f"b: chn {chn} stride {stride} shift {shift} call {i} rms", got[i][0], want[i][0])
            same_bits(f"b: chn {chn} stride {stride} shift {shift} call {i} peak", got[i][1], want[i][1])


def rate_signal(kind, n, fs):
    if kind == "noise":
        return signal(n, 41, fs)
    t = np.arange(n) / fs
    v = np.full(n, 0.5) if kind == "dc" else np.sin(2 * np.pi * 1000.0 * t)
    return np.stack([v, 0.25 * v], axis=1).astype(np.float32)


@pytest.mark.parametrize("fs", [8000.0, 22050.0, 44100.0, 48000.0, 88200.0, 96000.0, 192000.0])
@pytest.mark.parametrize("kind", ["dc", "sine", "noise"])
def test_rates_and_signals(M, oracle, kind, fs):
    """Stationary inputs, on which the f32 restatement stalls, and noise, at every rate: a call of 1 s + 1 frame, then one of 1 s + 3."""
    calls = [int(fs) + 1, int(fs) + 3]
    v = rate_signal(kind, sum(calls), fs)
    x = np.stack([v, (v * np.float32(0.5))[:, ::-1]])
    got, want = run_engine(M, fs, x, calls), run_yard(bind(oracle.lib), fs, x, calls)
    for i in range(2):
        hold_tight(f"c: {kind} at {fs:g} Hz, call {i}", got[i][0], want[i][0])
        same_bits(f"c: {kind} at {fs:g} Hz, call {i} peak", got[i][1], want[i][1])


def test_call_longer_than_the_weights_range(M, oracle):
    """87.5 s at 8 kHz in one call: a^k, the weight of a group k groups before the last, underflows a double about 612 000 frames back.
    The loud head weighs nothing and is the peak; an Inf there still makes the reading 0, as a NaN state does at :101-102."""
    fs, n, head, lib = 8000.0, 700001, 10000, bind(oracle.lib)
    rng = np.random.default_rng(730)
    x = rng.uniform(-0.01, 0.01, (2, n, 1)).astype(np.float32)
    x[:, :head] = np.where(rng.uniform(size=(2, head, 1)) < 0.5, np.float32(-0.9), np.float32(0.9))
    x[1, 5000, 0] = np.inf
    (wrms, wpeak), = run_yard(lib, fs, x, [n])
    tail = x.copy()
    tail[:, :head] = 0
    assert np.array_equal(bits(run_yard(lib, fs, tail[:1], [n])[0][0]), bits(wrms[:1]))      # the head contributes nothing
    assert wrms[1, 0] == 0 and wpeak[0, 0] == np.sqrt(np.float32(0.9) * np.float32(0.9)) and wpeak[1, 0] == 0
    (rms, peak), = run_engine(M, fs, x, [n])
    hold_tight("d: 700 001 frames at 8 kHz", rms, wrms)
    same_bits("d: peak", peak, wpeak)


NF_FS = 48000.0
NF_CALLS = [32768 + 4096 + 6, 48000 + 2]


def not_finite_batch(pair):
    """(clean, x, ch): eight streams, x with what is not finite in channel ch [s] of stream s during the first call.  pair: stream 4
    holds 1.8e19, whose square is finite, and 1.9e19, whose square is not — otherwise 1e30."""
    T1, Lg = NF_CALLS[0], NF_CALLS[0] & ~3
    clean = np.stack([signal(sum(NF_CALLS), 740 + s, NF_FS) for s in range(8)])
    x, ch = clean.copy(), [s % 2 for s in range(8)]
    x[1, T1 // 2, ch[1]] = np.nan
    x[2, 20001, ch[2]] = np.inf
    x[3, 0, ch[3]] = -np.inf
    if pair:
        x[4, T1 - 3000, ch[4]] = 1.8e19
        x[4, T1 - 2000, ch[4]] = -1.9e19
        with np.errstate(over="ignore"):
            assert np.isfinite(x[4, T1 - 3000, ch[4]] ** 2) and np.isinf(x[4, T1 - 2000, ch[4]] ** 2)
    else:
        x[4, T1 - 1000, ch[4]] = 1e30                           # in the chunk that ends the call
    x[5, Lg - 1, ch[5]] = np.inf                                # the last frame the call takes: the states end as Inf
    x[6, Lg, ch[6]] = np.nan                                    # the two frames the call drops
    x[6, Lg + 1, ch[6]] = np.inf
    x[7, Lg - 2, ch[7]] = np.inf
    return clean, x, ch


@pytest.mark.parametrize("pair", [False, True], ids=["1e30", "1.8e19 and 1.9e19"])
def test_not_finite(M, oracle, pair):
    """kmeterdsp.cc:80-103: an infinite square makes z1 Inf, the next frame makes it NaN and :101-102 zero the states — the reading is 0
    and the next call starts from 0 — unless it is the last frame the call takes: then the reading is Inf and the next call starts from
    the clamp at 50.  :103 zeroes an infinite maximum.  The other channel, and a stream whose dropped frames alone are not finite, are
    those of the clean audio to the bit; the call with track lengths is the dense call to the bit."""
    import torch
    lib, fs, calls = bind(oracle.lib), NF_FS, NF_CALLS
    clean, x, ch = not_finite_batch(pair)
    f32, want = run_yard(lib, fs, x, calls, f64=False), run_yard(lib, fs, x, calls)
    for s in (2, 3, 4, 7):
        assert f32[0][0][s, ch[s]] == 0 and want[0][0][s, ch[s]] == 0
    assert np.isinf(f32[0][0][5, ch[5]]) and np.isinf(want[0][0][5, ch[5]])
    got, base = run_engine(M, fs, x, calls), run_engine(M, fs, clean, calls)
    for i in range(2):
        edge = (f32[i][0] == 0) | np.isinf(f32[i][0])
        same_bits(f"e: call {i}, where the restatement reads 0 or Inf", got[i][0][edge], f32[i][0][edge])
        hold_tight(f"e: call {i}", got[i][0], want[i][0])
        same_bits(f"e: call {i} peak", got[i][1], want[i][1])
        same_bits(f"e: call {i} peak (restatement)", got[i][1], f32[i][1])
        for k in range(2):
            for s in range(8):
                for c in range(2):
                    if c != ch[s] or s in (0, 6):
                        assert bits(got[i][k][s, c]) == bits(base[i][k][s, c]), ("untouched", i, k, s, c, got[i][k][s, c], base[i][k][s, c])
    assert np.isinf(got[0][0][5, ch[5]]) and np.isfinite(got[1][0]).all()
    # ... with track lengths: the same eight, full length, and a ninth that ends at E inside the first call, an Inf in the last frame
    # ITS process (p, E) takes
    E = 20003
    ninth = signal(sum(calls), 749, fs)
    ninth[(E & ~3) - 1, 0] = np.inf
    ninth[E:] = np.nan
    x9 = np.concatenate([x, ninth[None]])
    dev = torch.from_numpy(x9).cuda()
    y32, y64 = Yard(lib, fs, 1, 2, False), Yard(lib, fs, 1, 2, True)
    y32.process(ninth[None], [E])
    y64.process(ninth[None], [E])
    w32, w64 = y32.read(), y64.read()
    assert np.isinf(w32[0][0, 0]) and np.isinf(w64[0][0, 0]) and np.isfinite(w64[0][0, 1])
    with M.Engine(9, fs, M.METER_KMETER) as e:
        pos = 0
        for i, n in enumerate(calls):
            e.process_device_tracks(dev.data_ptr() + pos * 8, n, np.array([n] * 8 + [0 if i else E], np.uint64), stride=sum(calls))
            rms, peak = engine_read(e, 2)
            same_bits(f"e: tracks, call {i} rms", rms[:8], got[i][0])
            same_bits(f"e: tracks, call {i} peak", peak[:8], got[i][1])
            hold_tight(f"e: tracks, the stream that ends at {E}, call {i}", rms[8:], w64[0])
            same_bits("e: tracks, the ninth's peak", peak[8:], w64[1])
            same_bits("e: tracks, the ninth's peak (restatement)", peak[8:], w32[1])
            pos += n


@pytest.mark.parametrize("amp", [100.0, 1e15])
def test_clamps(M, oracle, amp):
    """States far above 50 at the end of a call: the next one starts from 50 (:74-75)."""
    fs, calls = 48000.0, [48001, 48001]
    x = np.stack([signal(sum(calls), 750 + s, fs) for s in range(2)])
    x[:, :, 1] *= np.float32(4.0)
    x[:, :calls[0]] *= np.float32(amp)
    x[:, calls[0]:] *= np.float32(0.1)
    y = Yard(bind(oracle.lib), fs, 2, 2, True)
    y.process(x[:, :calls[0]])
    assert (y.field("z1") > 50).all() and (y.field("z2") > 50).all() and np.isfinite(y.field("z2")).all()
    got, want = run_engine(M, fs, x, calls), run_yard(oracle.lib, fs, x, calls)
    for i in range(2):
        hold_tight(f"f: amplitude {amp:g}, call {i}", got[i][0], want[i][0])
        same_bits(f"f: amplitude {amp:g}, call {i} peak", got[i][1], want[i][1])


def drive(M, lib, fs, blocks, reads=None):
    """blocks [S, n, chn] one call each; reads: {call: (first, count)} (default: every stream after every call).  What is read is held
    to the restatement read the same way: rms at 1e-5, peak to the bit.  Returns [(call, rms, peak)] and the restatement."""
    S, chn = blocks[0].shape[0], blocks[0].shape[2]
    y, rec = Yard(lib, fs, S, chn, False), []
    with M.Engine(S, fs, M.METER_KMETER, n_channels=chn) as e:
        for i, b in enumerate(blocks):
            e.process(b)
            y.process(b)
            if reads is None or i in reads:
                first, count = (0, S) if reads is None else reads[i]
                rms, peak = engine_read(e, chn, first, count)
                wrms, wpeak = y.read(first, count)
                assert (np.abs(rms - wrms) <= 1e-5 * np.maximum(wrms, 1e-3)).all(), (i, rms, wrms)
                same_bits(f"g: call {i} peak", peak, wpeak)
                rec.append((i, rms, peak))
    return rec, y


def _silence(S, n, chn=2):
    return np.zeros((S, n, chn), np.float32)


def test_hold_then_fall(M, oracle):
    """A peak, then 300 calls of 256 silent frames at 8 kHz: the hold (4000 frames) is counted down in steps of fpp — 16 calls bring it
    to -96 — then the peak falls by 15 dB/s to the fixed point of peak * fall + 1e-10f."""
    fs = 8000.0
    first = _silence(2, 256)
    first[0, 100, 0], first[1, 31, 1] = 0.9, -1e-6
    rec, y = drive(M, bind(oracle.lib), fs, [first] + [_silence(2, 256)] * 300)
    p0 = rec[0][2]
    assert abs(p0[0, 0] - 0.9) < 1e-6 and abs(p0[1, 1] - 1e-6) < 1e-12
    for i, _, peak in rec[1:17]:
        assert np.array_equal(bits(peak), bits(p0)), i
    assert rec[17][2][0, 0] < p0[0, 0] and rec[17][2][1, 1] < p0[1, 1]
    assert (y.field("cnt")[[0, 1], [0, 1]] == 4000 - 16 * 256).all()
    fall = float(y.k[0][0].fall)
    assert abs(rec[-1][2][1, 1] - 1e-10 / (1 - fall)) <= 0.01 * 1e-10 / (1 - fall)


def test_equal_peak_rearms_the_hold(M, oracle):
    """:124 is >=: a later sample exactly equal to the held peak sets the counter to the hold again."""
    fs = 8000.0
    a, b = _silence(1, 256), _silence(1, 256)
    a[0, 7, 0] = 0.5
    b[0, 255, 0] = -0.5
    rec, y = drive(M, bind(oracle.lib), fs, [a] + [_silence(1, 256)] * 10 + [b] + [_silence(1, 256)] * 20)
    assert all(peak[0, 0] == np.float32(0.5) for _, _, peak in rec[:11 + 1 + 16])
    assert rec[11 + 1 + 16][2][0, 0] < np.float32(0.5)


def test_alternating_call_sizes(M, oracle):
    """256 / 1000 frames in turn: the fall-back factor is worked out anew at every call (:65-70), the counter goes down by different steps."""
    fs = 8000.0
    a = _silence(2, 256, 1)
    a[0, 3, 0], a[1, 200, 0] = 0.7, 0.01
    rec, y = drive(M, bind(oracle.lib), fs, [a] + [_silence(2, 1000 if i % 2 == 0 else 256, 1) for i in range(40)])
    assert rec[-1][2][0, 0] < 0.5 * rec[0][2][0, 0] and y.field("cnt")[0, 0] < 0


def test_calls_without_a_group(M, oracle):
    """Calls of 1, 2 and 3 frames have no group of four: the filter stands, t = 0, the + 1e-20f is applied and the hold counted each time."""
    fs = 48000.0
    x = np.stack([signal(4096, 760 + s, fs) for s in range(3)])
    calls = [1024] + [1, 2, 3] * 4 + [1024, 3, 2, 1]
    blocks, pos = [], 0
    for n in calls:
        blocks.append(x[:, pos:pos + n])
        pos += n
    rec, y = drive(M, bind(oracle.lib), fs, blocks)
    assert np.array_equal(bits(rec[0][2]), bits(rec[12][2]))               # the peak of the first call is held through them


def test_read_arms_only_what_it_reads(M, oracle):
    """kmeter_read (first = 2, count = 2) between a loud and a quiet call: streams 2 and 3 then read the quiet call's rms, the others
    still the loud one's (max-held until read)."""
    fs, S = 48000.0, 6
    v = signal(72000, 770, fs)                                             # (a second of it: z2 has caught up with z1 and only falls after)
    loud = np.stack([v[:48000]] * S)
    quiet = np.stack([v[48000:] * np.float32(0.01)] * S)
    rec, y = drive(M, bind(oracle.lib), fs, [loud, quiet], reads={0: (2, 2), 1: (0, S)})
    (_, r0, _), (_, r1, _) = rec
    others = [0, 1, 4, 5]
    assert np.array_equal(bits(r1[others]), bits(np.stack([r0[0]] * 4)))    # (every stream carries the same audio)
    assert (r1[2:4] < 0.9 * r0).all()


@pytest.mark.parametrize("S,chn", [(32, 2), (33, 2), (64, 1), (65, 1)])
def test_stream_counts_across_the_final_blocks(M, oracle, S, chn):
    """k_kmeter_final takes 64 (stream, channel) pairs a block: one block full, one pair into the next.  Every slot carries the same audio."""
    fs, T = 48000.0, 4100
    x = np.stack([signal(T, 780, fs)[:, :chn]] * S)
    (rms, peak), = run_engine(M, fs, x, [T])
    (wrms, wpeak), = run_yard(bind(oracle.lib), fs, x[:1], [T])
    same_bits(f"h: S {S} rms", rms, np.repeat(rms[:1], S, axis=0))
    same_bits(f"h: S {S} peak", peak, np.repeat(peak[:1], S, axis=0))
    hold_tight(f"h: S {S} chn {chn}, slot 0", rms[:1], wrms)
    same_bits(f"h: S {S} slot 0 peak", peak[:1], wpeak)
