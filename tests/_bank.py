"""What the 30-band bank's CPU and GPU tests share: the bound on the linear levels, the call programme with its inputs, the
faults the bound must be able to see, and which bands exist at a rate.  Test infrastructure."""
import numpy as np

import _signals as sig

NBANDS = 30

# val / max of the engine against the oracle, relative.  The arithmetic differs only in the f32 EMA's rounding order (the kernel
# may fuse omega * (q - val) + val) and in flushed f32 denormals: rounding noise, not a bias.  Measured on an MI355X over every
# comparison of tests/test_gpu_bank.py (512 comparisons, all streams): val 2.45e-7, max 2.51e-7 at worst.  The bound
# is 8 x that (noise varies with seed and length by small factors), floor 2e-6, ceiling 1e-4 — the project's older stated bound,
# which the full-size and fuzzed tests keep.  tests/test_bank_cpu.py holds the faults below against 10 x this.
BANK_REL = 2.01e-6
BANK_ATOL = 1e-30          # the first frames of a stream leave f32 denormals in max, which the GPU may flush; -100 dB is 5e-11
DB_TOL = 1e-3              # val_db / max_db where the oracle's value is above DB_FLOOR: the stated contract
DB_FLOOR = -90.0

# chunk edges +- 1 (the kernel stages 128 frames at a time), odd lengths in a row (the dither parity flips), one frame after a
# long call, and a run-out that lets a fault in the last frames of the call before it leave the filters
CALLS = [1, 2, 127, 128, 129, 255, 256, 257, 1, 383, 385, 3, 300]
CUTS = np.concatenate([[0], np.cumsum(CALLS)]).astype(int)
T_CALLS = int(CUTS[-1])
SPEED = 15.0               # the fastest the control allows: one frame weighs omega = 2e-3 of val, 15 x the default
N_STREAMS = 33
SEED0 = 7100


def gain(s):
    """0.05 .. 0.8 spread over the streams, neighbours far apart"""
    return float(np.linspace(0.05, 0.8, N_STREAMS)[(7 * s) % N_STREAMS])


def stream_input(s, T=T_CALLS, seed0=SEED0):
    """[T, 2] float32: stream s of every batch of these tests, whatever the batch's size"""
    return sig.lcg_noise(T, seed0 + s, gain(s % N_STREAMS))


def band_exists(fs, band):
    """bandpass_setup's own edges (src/spectr.c:107-134): the band exists where, after the two clamps, the upper edge is above
    the lower one — where the lower edge f_m - bw / 2 lies below Nyquist."""
    f_m = 2.0 ** ((band - 16) / 3.0) * 1000.0
    bw = f_m * 2.0 ** (1 / 6.0) - f_m * 2.0 ** (-1 / 6.0)
    wc, ww = 2 * np.pi * f_m / fs, 2 * np.pi * bw / fs
    lo, hi = max(wc - ww / 2, 1e-9), min(wc + ww / 2, np.pi - 1e-9)
    return hi > lo


def existing(fs):
    return np.array([band_exists(fs, b) for b in range(NBANDS)])


def run_calls(handle, x, calls):
    """x through an oracle handle call by call -> the reading after every call"""
    out, pos = [], 0
    for n in calls:
        out.append(handle.run(x[pos:pos + n]))
        pos += n
    return out


# ---- the faults a kernel that stages frames in chunks can make -----------------------------------------------------------------

def slip(x, k):
    """frame k delivered twice, everything behind it one frame late"""
    return np.concatenate([x[:k + 1], x[k:-1]])


def stale(x, k):
    """frame k replaced by the frame one chunk earlier (later where there is none): a buffer read before it was written"""
    y = x.copy()
    y[k] = x[k - 128] if k >= 128 else x[k + 128]
    return y


# global frame numbers: the start, both sides of the chunk-sized calls' cuts, inside the 257-frame call, the last two frames
# before the run-out, and both sides of the cut before those
FAULT_FRAMES = [0, 1, 2, 127, 128, 129, 130, 257, 258, 386, 387, 1023, 1024, 1151, 1152,
                int(CUTS[-2]) - 2, int(CUTS[-2]) - 1, int(CUTS[-3]) - 1, int(CUTS[-3])]
