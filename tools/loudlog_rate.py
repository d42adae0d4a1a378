"""tools/loudlog_rate.py — what the loudness log (mtr_engine_loudlog_set_period; the LOG instantiations of mtr_gate.hip) costs.
GPU box only.  The programme is the bench step's: 8192 streams x 10 s at 48 kHz (mtr_synth_fill_device kind 1), EBU R128 + true peak,
integration on.

    python tools/loudlog_rate.py --step [reps]
the step with the log off — one engine, each step from its call to the end of mtr_engine_sync (the deferred tail included) between
two events on the caller's stream.  Run it once per library (MTR_LIB names another build of libmtr_engine.so) in interleaved same-box
pairs to hold a build against its parent; parent-against-parent pairs of the same session give the margin.

    python tools/loudlog_rate.py [reps]
three engines of this build on one buffer taking turns step by step — log off, MTR_LOUDLOG_SAMPLE at P = 1, MTR_LOUDLOG_MAX at P = 1
(200 points per stream and step: the series is reset before each) — with the whole step as above and the gate's own time
(mtr_engine_timing_query: ms_gate, on whichever stream the gate ran).
Does not read the reference tree.
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


def one_step(e, buf, st, ev0, ev1):
    ev0.record()
    e.process_device(buf.data_ptr(), T, T, st)
    e.sync()                                                           # (the deferred tail included)
    ev1.record()
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1)


def step(reps):
    buf = buffer()
    st = torch.cuda.current_stream().cuda_stream
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with M.Engine(S, FS, M.METER_EBU | M.METER_TRUEPEAK) as e:
        e.integr_start()
        t = [one_step(e, buf, st, ev0, ev1) for _ in range(WARM + reps)][WARM:]
    v = np.asarray(t)
    print("EBU | TRUEPEAK step, log off, %s: median %.3f ms  min %.3f  max %.3f" % (os.environ.get("MTR_LIB") or "this build", np.median(v), v.min(), v.max()))


def forms(reps):
    buf = buffer()
    st = torch.cuda.current_stream().cuda_stream
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    engines = []
    for name, mode in (("log off", None), ("SAMPLE P = 1", M.LOUDLOG_SAMPLE), ("MAX P = 1", M.LOUDLOG_MAX)):
        e = M.Engine(S, FS, M.METER_EBU | M.METER_TRUEPEAK)
        if mode is not None:
            e.loudlog_set_period(1, T // 2400, mode)
        e.integr_start()
        e.timing_enable(True)
        engines.append((name, e))
    whole = {n: [] for n, _ in engines}
    gate = {n: [] for n, _ in engines}
    fused = {n: [] for n, _ in engines}
    for it in range(WARM + reps):
        for name, e in engines:
            if name != "log off":
                e.loudlog_reset()                                      # (every step appends its 200 points to an empty series)
                e.sync()
            ms = one_step(e, buf, st, ev0, ev1)
            q = e.timing_query()
            if it >= WARM:
                whole[name].append(ms)
                gate[name].append(q["ms_gate"])
                fused[name].append(q["ms_fused"])
    for name, e in engines:
        w, g, f = np.asarray(whole[name]), np.asarray(gate[name]), np.asarray(fused[name])
        print("%-13s step median %7.3f ms  min %7.3f  max %7.3f | ms_gate median %6.3f  min %6.3f  max %6.3f | ms_fused median %7.3f" % (
            name, np.median(w), w.min(), w.max(), np.median(g), g.min(), g.max(), np.median(f)))
        if name != "log off":
            n = e.loudlog_series()[2]
            assert (n == T // 2400).all(), n
        e.close()


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--step"]
    n = int(args[0]) if args else 9
    step(n) if "--step" in sys.argv[1:] else forms(n)
