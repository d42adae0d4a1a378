"""tools/gonio_rate.py — what the goniometer (MTR_METER_GONIO, mtr_gonio.hip) costs, next to the two kernels that read the same bytes:
k_needle (mtr_needle.hip, the other serial chain per stream) and Kmeterdsp (mtr_kmeter.hip, the HBM time of these bytes).  GPU box only.

One session, one buffer (8192 streams x 10 s of stereo at 48 kHz, the bench programme: mtr_synth_fill_device kind 1), engines that take
turns on it in rotating order, each call from a reset engine, after two warm-up rounds:
    GONIO, auto gain off, shift 2 · GONIO, auto gain on, shift 2 · GONIO, auto gain on, shift 1 · NEEDLE, all four kinds · KMETER
Times are the engine's own device events around each call (mtr_engine_timing_calls, column "whole call"); for the goniometer also
k_gonio_points and k_gonio_image apart, summed over the call's pieces (mtr_engine_gonio_timing: events around each launch).  Printed:
median, min and max per form, the ratio to the K-meter's median, and the bytes a form reads and writes.
    python tools/gonio_rate.py [reps] [tune_piece]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import meters.lv2_amd as M  # noqa: E402

FS, S, T = 48000.0, 8192, 480000
WARM = 2


def buffer():
    buf = torch.empty((S, T, 2), dtype=torch.float32, device="cuda")
    M.synth_fill_device(buf.data_ptr(), S, T, T, 777, FS, 1)
    torch.cuda.synchronize()
    return buf


def line(name, v, base=None):
    v = np.asarray(v, np.float64)
    med = float(np.median(v))
    out = "%-34s median %8.3f ms  min %8.3f  max %8.3f" % (name, med, v.min(), v.max())
    if base:
        out += "  x %.3f of KMETER" % (med / base)
    print(out, flush=True)
    return med


def main(reps, piece):
    buf = buffer()
    st = torch.cuda.current_stream().cuda_stream
    every = M.NEEDLE_VU | M.NEEDLE_IEC1 | M.NEEDLE_IEC2 | M.NEEDLE_MS
    forms = [("GONIO gain fixed, shift 2", M.METER_GONIO, dict(shift=2, autogain=0)),
             ("GONIO auto gain, shift 2", M.METER_GONIO, dict(shift=2, autogain=1)),
             ("GONIO auto gain, shift 1", M.METER_GONIO, dict(shift=1, autogain=1)),
             ("NEEDLE all four kinds", M.METER_NEEDLE, None), ("KMETER", M.METER_KMETER, None)]
    engines = []
    for name, meters, cfg in forms:
        e = M.Engine(S, FS, meters)
        if cfg:
            e.gonio_configure(tune_piece=piece, **cfg)
            e.gonio_timing(True)
        elif meters == M.METER_NEEDLE:
            e.needle_configure(every, 0, 0)
        e.timing_enable(True)
        engines.append((name, e, cfg))
    t = {name: [] for name, _, _ in engines}
    tp = {name: [] for name, _, cfg in engines if cfg}
    ti = {name: [] for name, _, cfg in engines if cfg}
    for it in range(WARM + reps):
        order = engines[it % len(engines):] + engines[:it % len(engines)]     # rotating
        for name, e, cfg in order:
            e.reset()
            e.process_device(buf.data_ptr(), T, T, st)
            e.sync()
            ms = e.timing_calls()
            if cfg:
                p, i, n = e.gonio_timing(True)
            if it >= WARM:
                t[name].append(float(ms[-1, 3]))
                if cfg:
                    tp[name].append(p)
                    ti[name].append(i)
    base = line("KMETER", t["KMETER"])
    for name, e, cfg in engines[:-1]:
        line(name, t[name], base)
        if cfg:
            line("    k_gonio_points", tp[name])
            line("    k_gonio_image", ti[name])
    audio = S * T * 8
    c, d = engines[0][1].gonio_config()
    pieces = (T + c.tune_piece - 1) // c.tune_piece
    print("bytes per call: every form reads the audio once, %.2f GB" % (audio / 1e9))
    print("  GONIO: k_gonio_points also writes %.2f GB of cell codes (2 B per frame and stream; scratch %d MB: pieces of %d frames, %d per call),"
          % (S * T * 2 / 1e9, S * ((c.tune_piece + 127) // 128 * 128) * 2 >> 20, c.tune_piece, pieces))
    print("         k_gonio_image reads them back and adds the touched cells of a stream's image per piece (at most 2 x 4 B per painted point;")
    for name, e, cfg in engines[:3]:
        img, drawn, clipped, skipped = e.gonio_image(0, 64)
        G = e.gonio_config()[1].G
        print("         %s: image %d x %d = %.1f MB per engine; first 64 streams: %.1f %% of the frames painted, %.1f %% clipped, %.1f %% of the cells touched)"
              % (name, G, G, S * G * G * 4 / 1e6, 100.0 * drawn.sum() / (64 * T), 100.0 * clipped.sum() / (64 * T), 100.0 * (img != 0).mean()))
    print("  NEEDLE and KMETER write their states only")
    for _, e, _ in engines:
        e.close()


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 7, int(sys.argv[2]) if len(sys.argv) > 2 else 0)
