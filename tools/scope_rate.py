"""tools/scope_rate.py — what the stereo / frequency scope (MTR_METER_SCOPE, mtr_scope.hip) costs, next to a kernel that reads the same
buffer once: Kmeterdsp (mtr_kmeter.hip).  GPU box only.

One session, one buffer (8192 streams x 10 s at 48 kHz, the bench programme: mtr_synth_fill_device kind 1), four engines that take
turns on it call by call — KMETER, and SCOPE at (W 1024, H default), (W 4096, H default) and (W 16384, H 4096) — after two warm-up
rounds.  Times are the engine's own device events around each call (mtr_engine_timing_calls, column "whole call"); printed per engine:
median, min and max, the bytes the configuration must read (H > W: the W frames of every analysis; else every frame once), the
fraction of the HBM peak (8.0 TB/s) that reading them in that time is, the FFT's 5 W log2 W flop per analysis as a rate, and the
ratio to the K-meter's median.
    python tools/scope_rate.py [reps]

--series: what the reading series (include/mtr_scope_series.h) costs.  One session, the same buffer, W 1024 at the default hop (250
analyses per stream), five forms that take turns in rotating order after two warm-up rounds:
    the dense call (no series: the kernel as it was);
    K = 1 with all seven fields (250 points of 12 KB per stream);  K = 1 with LEVEL | LR only;  K = 25 with all fields (10 points);
    the engine without a series called once per analysis — 250 calls of one hop — with scope_read after each: what a caller had to do
    for the same picture before there was a series.
The four single calls are timed by the engine's device events (column "whole call") and on the host clock around call + sync; the loop
of 250 on the host clock alone (every scope_read synchronises).  Printed per form: median, min and max of both, the bytes the points
take, and the ratio of the medians to the dense call's.
    python tools/scope_rate.py --series [reps]
"""
import math
import os
import sys
import time

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


def counts(e):
    """(n_points, dropped) of the engine's series, nothing fetched"""
    import ctypes as C
    n, d = C.c_uint32(), C.c_uint32()
    rc = M.lib.mtr_engine_scope_series(e._h, 0, 0, *([None] * 7), 0, C.byref(n), C.byref(d))
    assert rc == 0, M.lib.mtr_last_error()
    return n.value, d.value


def series(reps):
    W = 1024
    buf = buffer()
    st = torch.cuda.current_stream().cuda_stream
    hop = int(math.ceil(FS / 25.0))                                # (the default hop: fftx_init (.., 25))
    n_an = T // hop
    forms = [("dense call", 0, 0), ("K 1, all fields", 1, M.SCOPE_F_ALL), ("K 1, LEVEL | LR", 1, M.SCOPE_F_LEVEL | M.SCOPE_F_LR),
             ("K 25, all fields", 25, M.SCOPE_F_ALL)]
    engines = []
    for name, K, fields in forms:
        e = M.Engine(S, FS, M.METER_SCOPE)
        e.scope_configure(W, 0)
        if K:
            e.scope_set_series(K, n_an // K, fields)
        e.timing_enable(True)
        width = sum((1 if f == "peak" else W // 2) for k, f in enumerate(M.engine.SCOPE_FIELDS) if fields >> k & 1)
        engines.append((name, e, S * (n_an // K if K else 0) * width * 4.0))
    loop = M.Engine(S, FS, M.METER_SCOPE)
    loop.scope_configure(W, 0)
    dev_ms = {name: [] for name, _, _ in engines}
    host_ms = {name: [] for name, _, _ in engines}
    loop_ms = []

    def single(it, name, e):
        e.reset()                                                      # (the series starts again: every round appends the same points)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e.process_device(buf.data_ptr(), T, T, st)
        e.sync()
        t1 = time.perf_counter()
        if it >= WARM:
            dev_ms[name].append(float(e.timing_calls()[-1, 3]))
            host_ms[name].append((t1 - t0) * 1e3)

    def per_analysis(it, name, e):
        e.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for j in range(n_an):
            e.process_device(buf.data_ptr() + j * hop * 8, hop, T, st)
            e.scope_read()
        t1 = time.perf_counter()
        if it >= WARM:
            loop_ms.append((t1 - t0) * 1e3)

    turns = [(single, name, e) for name, e, _ in engines] + [(per_analysis, "loop", loop)]
    for it in range(WARM + reps):                                      # (in rotating order: none of them always runs behind the loop's 250 calls and copies)
        for k in range(len(turns)):
            f, name, e = turns[(k + it) % len(turns)]
            f(it, name, e)
    print("SCOPE W %d H %d, %d streams x %d frames: %d analyses per stream; %d rounds after %d warm-up rounds" % (W, hop, S, T, n_an, reps, WARM))
    base_d = base_h = None
    for name, e, pts in engines:
        d, h = np.asarray(dev_ms[name]), np.asarray(host_ms[name])
        base_d, base_h = base_d or float(np.median(d)), base_h or float(np.median(h))
        n, dr = counts(e) if pts else (0, 0)
        print("%-18s device events: median %9.3f ms  min %9.3f  max %9.3f  x %5.2f of dense | host clock, call + sync: median %9.3f ms  min %9.3f  max %9.3f  x %5.2f"
              "  | points: %6.2f GB, %d per stream, %d dropped" % (name, np.median(d), d.min(), d.max(), np.median(d) / base_d, np.median(h), h.min(), h.max(),
                                                                  np.median(h) / base_h, pts / 1e9, n, dr))
    v = np.asarray(loop_ms)
    # (what the two ways hand out is the same: the K 25 engine's last point — analysis 250 — against the loop's last reading, 64 streams)
    last, pts = loop.scope_read(0, 64), engines[3][1].scope_series(0, 64)[0]
    print("the last point at K 25 equals the loop's last scope_read bit for bit (64 streams, 7 fields):",
          all(np.array_equal(pts[f][:, -1].view(np.uint32), last[f].view(np.uint32)) for f in M.engine.SCOPE_FIELDS))
    print("%-18s host clock, %d x (call of one hop + scope_read): median %9.3f ms  min %9.3f  max %9.3f  x %5.2f of the dense call's host clock"
          % ("one call per analysis", n_an, np.median(v), v.min(), v.max(), np.median(v) / base_h))
    for _, e, _ in engines:
        e.close()
    loop.close()


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--series"]
    if "--series" in sys.argv[1:]:
        series(int(args[0]) if args else 5)
    else:
        main(int(args[0]) if args else 9)
