#!/usr/bin/env python3
"""tools/seg_screen_model.py [streams] [signals...] — a host model of the rule by which k_seg's screen completes chunks
(mtr_seg.hip: SCREEN, the stream reference), for predicting what a change of the rule buys.  Numpy only, no GPU, no library.

What it models, on bench.py's shape (10 s at 48 kHz, 8 segments per stream, EBU R128 + true peak):
  * the three signals of k_synth (mtr_bank.hip): the LCG bit for bit (seed 777 + stream, jumped in closed form), the
    envelopes in float64 (the device's __sinf is not reproduced);
  * phases 1 - 3 of the 4x interpolator as a float64 FIR, the taps from mtr_setup_fir_table's formula;
  * the 8 segments of a stream in lock step, a step = 16 frames; per step and lane, in front of the votes: pk0 (the sample
    peak) and M (the running maximum of |x| since the segment's 48 history frames) take the step's samples; R = the maximum
    over the stream's lanes of max (pk0, pkf), taken every fourth step;
  * the vote of step j on the outputs whose windows end in the frames of step j - 1 (they lag the step's samples by 40
    frames), per lane (column, group of 4 rows): twelve values, max |Y| + eps < max (pm, R) with eps = 56 / 32768 M (the
    first product is taken for the exact output: they differ by less than eps);
  * a chunk = 2 streams x 8 segments of one channel; a chunk one lane of which fails completes, and all of its lanes fold
    their values into pm; the launch's last step completes every chunk;
  * rule 1: pkf stays zero during the launch (it receives pm only at a flush).  Rule 2: a completed chunk's pm goes into
    the owners' pkf at once (the peek), and reaches R at its next refresh.  Rule 3 (not built): ... and R is refreshed at once.
    Rule 4 (the core form, MTR_SEG_SCREEN=4): rule 2 with the vote on the core products themselves — each row's taps inside the
    32-sample stretch of its fragment (core_matrix), twelve values per lane in the core's row layout (rows 16 w + 4 kg .. + 3) —
    and eps' = 920 / 32768 M; completed chunks fold their exact outputs into pm as under every rule.

Per wave (k_seg's lazy form, MTR_SEG_SCREEN=3, pays per wave and step, not per chunk: a step of a wave with at least one completing
chunk takes the cold branch and builds lo words there): a wave = 8 streams x 8 segments = 4 pairs of streams x 2 channels = 8
chunks; wave_steps () counts the steps of the main loop in which a wave completes at least one chunk, and the chunks per such step.

It prints the share of screened chunks that complete and, for rule 2, the per-wave figures.  16 streams take about a second per signal and rule.  The model decides
no test of the kernel: tests/test_seg_screen_model_cpu.py holds rule 1 to the measured rates of
profiles/r23_kseg_trim/completion_rates.txt."""
import sys

import numpy as np

FS, T, SEGS, STEP = 48000.0, 480000, 8, 16
K_REL = 56.0 / 32768.0
K_REL_CORE = 920.0 / 32768.0                                     # CORE_K_REL (mtr_seg.hip: the core screen)


def lcg_noise(T, seed):
    """u[T, 2] of k_synth: s <- 1664525 s + 1013904223 (mod 2^32), two draws per frame, u = ((s >> 8) - 2^23) / 2^23."""
    n = 2 * T
    a = np.full(n, 1664525, np.uint32)
    a[0] = 1
    pw = np.cumprod(a, dtype=np.uint32)                          # A^0 .. A^(n-1), mod 2^32
    geo = np.cumsum(pw, dtype=np.uint32)                         # 1 + A + .. + A^(k-1), k = 1 .. n
    ak = pw * np.uint32(1664525)                                 # A^k
    s = ak * np.uint32(seed) + geo * np.uint32(1013904223)
    u = ((s >> np.uint32(8)).astype(np.int64) - (1 << 23)).astype(np.float32) / np.float32(1 << 23)
    return u.reshape(T, 2)


def synth(kind, seed, T=T, fs=FS):
    """One stream of k_synth, float32 [T, 2]."""
    u = lcg_noise(T, seed).astype(np.float64)
    f = np.arange(T, dtype=np.float64)
    if kind == 1:
        env = 0.05 + 0.45 * (0.5 + 0.5 * np.sin(2 * np.pi * 0.2 * (f / fs)))
        pl = ((f * 440) % fs) / fs
        pr = ((f * 3000) % fs) / fs
        u = np.stack([env * (0.5 * u[:, 0] + 0.5 * np.sin(2 * np.pi * pl)), env * (0.5 * u[:, 1] + 0.5 * np.sin(2 * np.pi * pr))], 1)
    elif kind == 2:
        u = u * np.exp2(-8.0 + 8.0 * f / T)[:, None]
    return u.astype(np.float32)


def taps():
    """g[3][48]: phases 1 - 3, window position 0 = the oldest sample (mtr_setup_fir_table's rows, mirrored into 48 taps)."""
    hl = 24
    tab = np.zeros((5, hl))
    for j in range(5):
        for i in range(hl):
            t = j / 4.0 + i
            x = abs(t) * np.pi
            sinc = 1.0 if abs(t) < 1e-6 else np.sin(x) / x
            w = abs(t / hl)
            win = 0.0 if w >= 1.0 else 0.384 + 0.500 * np.cos(np.pi * w) + 0.116 * np.cos(2 * np.pi * w)
            tab[j, hl - 1 - i] = sinc * win
    g = np.zeros((3, 48))
    for ph in (1, 2, 3):
        for i in range(48):
            g[ph - 1, i] = tab[ph, i] if i < 24 else tab[4 - ph, 47 - i]
    return g


def core_matrix(g):
    """[48, 64]: row n = 3 f + p of the frame-major list over the step's 64-sample window, its taps (A[f][t] = g_p[t - 1 - f]) kept
    inside the stretch [8 (w + 1), 8 (w + 1) + 32) of its fragment w = n // 16 and zero outside (mtr_mfma16_fir.h: mtr_m16_build_core)."""
    c = np.zeros((48, 64))
    for n in range(48):
        f, p, w = n // 3, n % 3, n // 16
        for t in range(8 * (w + 1), 8 * (w + 1) + 32):
            if 0 <= t - 1 - f < 48:
                c[n, t] = g[p][t - 1 - f]
    return c


def core_lanes(x, g):
    """For one stream x[T, 2]: per (channel, segment, step, kg) the max |F'| of the twelve core products lane (c, kg) votes with — rows
    16 w + 4 kg .. + 3, w = 0 .. 2, of the step whose outputs are the step's frames [2, 8, n, 4]."""
    seg = x.shape[0] // SEGS
    n = seg // STEP
    cm = core_matrix(g)
    out = np.zeros((2, SEGS, n, 4))
    for ch in range(2):
        xp = np.concatenate([np.zeros(48), x[:, ch].astype(np.float64)])
        win = np.lib.stride_tricks.sliding_window_view(xp, 64)[::STEP]          # window of step s: frames 16 s - 48 .. 16 s + 15
        f = np.abs(win @ cm.T)                                                  # [steps, 48]
        out[ch] = f.reshape(-1, 3, 4, 4).max(axis=(1, 3)).reshape(SEGS, n, 4)
    return out


def lanes(x, g):
    """For one stream x[T, 2]: per (channel, segment, step) the step's max |x| [2, 8, n] and per (channel, segment, step, row
    group) the max |Y| over 4 rows x 3 phases of the outputs whose windows end in the step's frames [2, 8, n, 4]; and the
    max |x| of each segment's 48 history frames [2, 8]."""
    seg = x.shape[0] // SEGS
    n = seg // STEP
    ml = np.zeros((2, SEGS, n))
    v = np.zeros((2, SEGS, n, 4))
    h = np.zeros((2, SEGS))
    for ch in range(2):
        xc = x[:, ch].astype(np.float64)
        xp = np.concatenate([np.zeros(47), xc])
        y = np.zeros(x.shape[0])
        for p in range(3):
            y = np.maximum(y, np.abs(np.convolve(xp, g[p][::-1], "valid")))   # y[e] = the window that ends at frame e
        ml[ch] = np.abs(xc).reshape(SEGS, n, STEP).max(2)
        v[ch] = y.reshape(SEGS, n, 4, 4).max(3)
        for q in range(1, SEGS):
            h[ch, q] = np.abs(xc[q * seg - 48:q * seg]).max()
    return ml, v, h


def run(kind, streams, rule, g=None, waves=None):
    """(chunks screened, chunks completed) of `streams` streams (an even number) of signal `kind` under `rule`.  waves: a dict that
    receives `steps` (wave-steps of the main loop), `cold` (those with at least one completing chunk) and `chunks` (completed there);
    `streams` must then be a multiple of 8."""
    g = taps() if g is None else g
    sigs = [synth(kind, 777 + s) for s in range(streams)]
    per = [lanes(x, g) for x in sigs]
    ml = np.stack([p[0] for p in per])                           # [S, 2, 8, n]
    v = np.stack([p[1] for p in per])                            # [S, 2, 8, n, 4]
    core = rule == 4
    k_rel = K_REL_CORE if core else K_REL
    vc = np.stack([core_lanes(x, g) for x in sigs]) if core else v   # what the vote sees: the truncated product itself under the core rule
    S, n = streams, ml.shape[3]
    M = np.stack([p[2] for p in per])                            # [S, 2, 8]
    pk0 = np.zeros((S, 2, SEGS))
    pkf = np.zeros((S, 2, SEGS))
    pm = np.zeros((S, 2, SEGS, 4))
    R = np.zeros((S, 2))
    pk0 = np.maximum(pk0, ml[:, :, :, 0]); M = np.maximum(M, ml[:, :, :, 0])     # step 0: no products in front of it
    R = np.maximum(pk0, pkf).max(2)
    done = 0
    w_cold = w_chunks = 0
    for j in range(1, n):
        pk0 = np.maximum(pk0, ml[:, :, :, j]); M = np.maximum(M, ml[:, :, :, j])
        if j % 4 == 0 or rule == 3:
            R = np.maximum(pk0, pkf).max(2)
        vj = v[:, :, :, j - 1, :]
        fail = vc[:, :, :, j - 1, :] + (k_rel * M)[..., None] >= np.maximum(pm, R[:, :, None, None])      # [S, 2, 8, 4]
        chunk = fail.reshape(S // 2, 2, 2, SEGS, 4).any(axis=(1, 3, 4))                    # [S / 2, 2]: pair of streams, channel
        if chunk.any():
            done += int(chunk.sum())
            if waves is not None:
                per_wave = chunk.reshape(S // 8, 8).sum(1)                                      # 4 pairs x 2 channels
                w_cold += int((per_wave > 0).sum()); w_chunks += int(per_wave.sum())
            lane = np.repeat(chunk, 2, axis=0)[:, :, None, None]                            # back to [S, 2, 1, 1]
            pm = np.where(lane, np.maximum(pm, vj), pm)
            if rule >= 2:
                pkf = np.where(lane[..., 0], np.maximum(pkf, pm.max(3)), pkf)
    done += S // 2 * 2                                           # the launch's last step runs dense
    if waves is not None:
        waves.update(steps=S // 8 * (n - 1), cold=w_cold, chunks=w_chunks)
    return S // 2 * 2 * n, done


def wave_steps(kind, streams=16, rule=2, g=None):
    """(share of a wave's steps with at least one completing chunk, chunks per such step): what the lazy form's cold path costs."""
    w = {}
    run(kind, streams, rule, g, waves=w)
    return w["cold"] / w["steps"], w["chunks"] / max(w["cold"], 1)


def main(argv):
    streams = int(argv[0]) if argv else 16
    kinds = [int(k) for k in argv[1:]] or [1, 0, 2]
    g = taps()
    for kind in kinds:
        for rule in (1, 2, 3, 4):
            scr, fin = run(kind, streams, rule, g)
            print("signal %d rule %d: streams %d chunks screened %d completed %d rate %.4f" % (kind, rule, streams, scr, fin, fin / scr))
        if streams % 8 == 0:
            for rule in (2, 4):
                share, per = wave_steps(kind, streams, rule, g)
                print("signal %d rule %d: a wave of 8 streams completes in %.4f of its steps, %.2f chunks per such step" % (kind, rule, share, per))


if __name__ == "__main__":
    main(sys.argv[1:])
