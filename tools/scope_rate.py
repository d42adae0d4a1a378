"""tools/scope_rate.py — what the stereo / frequency scope (MTR_METER_SCOPE, mtr_scope.hip) costs, next to a kernel that reads the same
buffer once: Kmeterdsp (mtr_kmeter.hip).  GPU box only.

One session, one buffer (8192 streams x 10 s at 48 kHz, the bench programme: mtr_synth_fill_device kind 1), four engines that take
turns on it call by call — KMETER, and SCOPE at (W 1024, H default), (W 4096, H default) and (W 16384, H 4096) — after two warm-up
rounds.  Times are the engine's own device events around each call (mtr_engine_timing_calls, column "whole call"); printed per engine:
median, min and max, the bytes the configuration must read (H > W: the W frames of every analysis; else every frame once), the
fraction of the HBM peak (8.0 TB/s) that reading them in that time is, the FFT's 5 W log2 W flop per analysis as a rate, and the
ratio to the K-meter's median.
    python tools/scope_rate.py [reps]
"""
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import meters.lv2_amd as M  # noqa: E402

FS, S, T = 48000.0, 8192, 480000
HBM_PEAK = 8.0e12
WARM = 2
FORMS = [(1024, 0), (4096, 0), (16384, 4096)]


def buffer():
    buf = torch.empty((S, T, 2), dtype=torch.float32, device="cuda")
    M.synth_fill_device(buf.data_ptr(), S, T, T, 777, FS, 1)
    torch.cuda.synchronize()
    return buf


def report(name, v, must_read, flop=0.0, base=None):
    v = np.asarray(v, np.float64)
    med = float(np.median(v))
    line = "%-24s median %8.3f ms  min %8.3f  max %8.3f  reads %6.2f GB (%5.1f %% of the batch): %5.1f %% of HBM peak" % (
        name, med, v.min(), v.max(), must_read / 1e9, 100.0 * must_read / (S * T * 8.0), 100.0 * must_read / (med * 1e-3) / HBM_PEAK)
    if flop:
        line += "  %6.3f TFLOP: %5.1f TFLOP/s" % (flop / 1e12, flop / (med * 1e-3) / 1e12)
    if base:
        line += "  x %.2f of KMETER" % (med / base)
    print(line)
    return med


def main(reps):
    buf = buffer()
    st = torch.cuda.current_stream().cuda_stream
    engines = [("KMETER", M.Engine(S, FS, M.METER_KMETER), S * T * 8.0, 0.0)]
    for W, H in FORMS:
        e = M.Engine(S, FS, M.METER_SCOPE)
        e.scope_configure(W, H)
        _, hop, _ = e.scope_config()
        n_an = T // hop
        must = S * 8.0 * (n_an * W if hop > W else T)
        engines.append(("SCOPE W %5d H %4d" % (W, hop), e, must, S * n_an * 5.0 * W * math.log2(W)))
    t = {name: [] for name, _, _, _ in engines}
    for _, e, _, _ in engines:
        e.timing_enable(True)
    for it in range(WARM + reps):
        for name, e, _, _ in engines:
            e.process_device(buf.data_ptr(), T, T, st)
            e.sync()
            ms = e.timing_calls()
            if it >= WARM:
                t[name].append(float(ms[-1, 3]))
    base = None
    for name, e, must, flop in engines:
        med = report(name, t[name], must, flop, base)
        base = base or med
        e.close()


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 9)
