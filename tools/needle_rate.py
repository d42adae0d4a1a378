"""tools/needle_rate.py — what the needle meters (MTR_METER_NEEDLE, mtr_needle.hip) cost, next to the two kernels that read the same
bytes once: Kmeterdsp (mtr_kmeter.hip, the HBM time of these bytes) and DR-14 (mtr_dr14.hip).  GPU box only.

One session, one buffer (8192 streams x 10 s at 48 kHz, the bench programme: mtr_synth_fill_device kind 1), engines that take turns
on it call by call — KMETER alone, DR14 alone, k_needle with IEC2 alone and with all four kinds, each with every call one
process () (P = 0) and with the reading series at P = 4800 — after two warm-up rounds.  Times are the engine's own device events
around each call (mtr_engine_timing_calls, column "whole call"); printed: median, min and max per engine, the ratio to the
K-meter's median and the fraction of the HBM peak (8.0 TB/s) that reading the buffer once in that time is.
    python tools/needle_rate.py [reps]

The chain's own floor is not measured here: (VALU instructions per frame on the longest wave, counted in the compiled loop) x 4
cycles x 480000 / the clock observed under the kernel.

    python tools/needle_rate.py --ebu [reps]
times the bench step instead (EBU R128 + true peak on the same buffer, integration on): run it once per library (MTR_LIB names
another build of libmtr_engine.so) to hold a build against its parent, in same-box pairs.
"""
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


def buffer():
    buf = torch.empty((S, T, 2), dtype=torch.float32, device="cuda")
    M.synth_fill_device(buf.data_ptr(), S, T, T, 777, FS, 1)
    torch.cuda.synchronize()
    return buf


def report(name, v, base=None):
    v = np.asarray(v, np.float64)
    med = float(np.median(v))
    line = "%-26s median %7.3f ms  min %7.3f  max %7.3f  %5.1f %% of HBM peak" % (name, med, v.min(), v.max(), 100.0 * S * T * 8 / (med * 1e-3) / HBM_PEAK)
    if base:
        line += "  x %.3f of KMETER" % (med / base)
    print(line, flush=True)
    return med


def meters_turn(reps):
    buf = buffer()
    st = torch.cuda.current_stream().cuda_stream
    forms = [("KMETER", M.METER_KMETER, None, None), ("DR14", M.METER_DR14, None, None)]
    if hasattr(M.lib, "mtr_engine_needle_read"):                              # (MTR_LIB may name a library from before the meter)
        every = M.NEEDLE_VU | M.NEEDLE_IEC1 | M.NEEDLE_IEC2 | M.NEEDLE_MS
        forms += [("NEEDLE IEC2 P = 0", M.METER_NEEDLE, M.NEEDLE_IEC2, 0), ("NEEDLE IEC2 P = 4800", M.METER_NEEDLE, M.NEEDLE_IEC2, 4800),
                  ("NEEDLE VU P = 4800", M.METER_NEEDLE, M.NEEDLE_VU, 4800), ("NEEDLE MS P = 4800", M.METER_NEEDLE, M.NEEDLE_MS, 4800),
                  ("NEEDLE all four P = 0", M.METER_NEEDLE, every, 0), ("NEEDLE all four P = 4800", M.METER_NEEDLE, every, 4800)]
    engines = []
    for name, meters, kinds, P in forms:
        e = M.Engine(S, FS, meters)
        if kinds:
            e.needle_configure(kinds, P, T // P if P else 0)
        e.timing_enable(True)
        engines.append((name, e))
    t = {name: [] for name, _ in engines}
    for it in range(WARM + reps):
        for name, e in engines:
            e.process_device(buf.data_ptr(), T, T, st)
            e.sync()
            ms = e.timing_calls()
            if it >= WARM:
                t[name].append(float(ms[-1, 3]))
    base = report("KMETER", t["KMETER"])
    for name, _ in engines[1:]:
        report(name, t[name], base)
    for _, e in engines:
        e.close()


def bench_step(reps):
    buf = buffer()
    st = torch.cuda.current_stream().cuda_stream
    t = []
    with M.Engine(S, FS, M.METER_EBU | M.METER_TRUEPEAK) as e:
        e.integr_start()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for it in range(WARM + reps):
            ev0.record()
            e.process_device(buf.data_ptr(), T, T, st)
            e.sync()                                                       # (the deferred tail included)
            ev1.record()
            torch.cuda.synchronize()
            if it >= WARM:
                t.append(ev0.elapsed_time(ev1))
    v = np.asarray(t)
    print("EBU | TRUEPEAK step, %s: median %.3f ms  min %.3f  max %.3f" % (os.environ.get("MTR_LIB") or "this build", np.median(v), v.min(), v.max()), flush=True)


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--ebu"]
    n = int(args[0]) if args else 9
    bench_step(n) if "--ebu" in sys.argv[1:] else meters_turn(n)
