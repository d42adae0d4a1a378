"""tools/tpb_series_rate.py — what the true-peak bar's reading series (mtr_engine_tpb_set_period, the SERIES instantiations of k_tpb) costs.
GPU box only.

One session, one buffer (8192 streams x 10 s of stereo f32 at 48 kHz, the bench programme: mtr_synth_fill_device kind 1), three
configurations that take turns on it in rotating order after two warm-up rounds:
  (a) the dense call at P = 0: one TruePeakdsp::process () + read (m, p) per stream;
  (b) one call at P = 4800 with a series of 100 points;
  (c) what a caller had to do before the series existed: the P = 0 engine called 100 times with 4800 frames, results () after each.
Each turn is timed on the host around the call(s) and the wait for them (what the caller sees); (a) and (b) also by device events
around the call.  Prints the medians, (b) / (a) and (c) / (b) as one JSON object and writes the head of profiles/r31_tpb_series.md — the
table and the ratios; the sections that follow it there are written by hand and kept.
    python tools/tpb_series_rate.py [reps] [--out DIR]

    python tools/tpb_series_rate.py --pairs N [reps]
holds the dense call of this build against the parent's library (tools/build_ab.sh -> meters.lv2_amd/lib_ab): N pairs of child
processes, this build and the parent alternating on the same box, each timing the dense call `reps` times (--dense, with MTR_LIB naming
the library); prints a table row per child.
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

FS, S, T, P = 48000.0, 8192, 480000, 4800
WARM = 2
LIB_AB = os.path.join(ROOT, "meters.lv2_amd", "lib_ab", "libmtr_engine.so")
PROFILE = "r31_tpb_series.md"


def buffer(M, torch):
    buf = torch.empty((S, T, 2), dtype=torch.float32, device="cuda")
    M.synth_fill_device(buf.data_ptr(), S, T, T, 777, FS, 1)
    torch.cuda.synchronize()
    return buf


def turns(reps, out):
    import numpy as np
    import torch
    import meters.lv2_amd as M
    buf = buffer(M, torch)
    st = torch.cuda.current_stream().cuda_stream
    ea, eb, ec = (M.Engine(S, FS, M.METER_TPBALLIST) for _ in range(3))
    eb.tpb_set_period(P, T // P)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    host = {"a": [], "b": [], "c": []}
    dev = {"a": [], "b": []}
    last = {}

    def one(e):
        t0 = time.perf_counter()
        ev[0].record()
        e.process_device(buf.data_ptr(), T, T, st)
        ev[1].record()
        e.sync()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, ev[0].elapsed_time(ev[1])

    def trace(e):
        t0 = time.perf_counter()
        for k in range(T // P):
            e.process_device(buf.data_ptr() + k * P * 8, P, T, st)
            last["c"] = e.results()
        return (time.perf_counter() - t0) * 1e3, None

    order = ["a", "b", "c"]
    for it in range(WARM + reps):
        for key in order[it % 3:] + order[:it % 3]:                        # rotating order: nobody always runs behind the same neighbour
            if key != "a":
                (eb if key == "b" else ec).reset()                         # (every turn is the trace from a fresh engine's state)
                torch.cuda.synchronize()
            h, d = one(ea) if key == "a" else one(eb) if key == "b" else trace(ec)
            if it >= WARM:
                host[key].append(h)
                if d is not None:
                    dev[key].append(d)
    level, peak, n, dropped = eb.tpb_series()
    assert n == T // P and dropped == 0 and np.isfinite(level).all()
    # the same trace's last point: (c)'s hundredth call is (b)'s hundredth block
    lc = np.array([[r.tpb_level[c] for c in range(2)] for r in last["c"]], np.float32)
    pc = np.array([[r.tpb_peak[c] for c in range(2)] for r in last["c"]], np.float32)
    worst = float(max(np.max(np.abs(level[:, -1] - lc) / lc), np.max(np.abs(peak[:, -1] - pc) / pc)))
    for e in (ea, eb, ec):
        e.close()
    med = lambda v: float(np.median(v))
    res = {"box": f"{torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName})",
           "shape": f"{S} streams x {T // int(FS)} s stereo f32 at {int(FS)} Hz, {reps} turns after {WARM} warm ones, rotating order",
           "host_ms": host, "device_ms": dev,
           "a_ms": med(dev["a"]), "b_ms": med(dev["b"]), "a_host_ms": med(host["a"]), "b_host_ms": med(host["b"]), "c_host_ms": med(host["c"]),
           "last_point_b_vs_c_worst_relative": worst}
    res["b_over_a"] = res["b_ms"] / res["a_ms"]
    res["c_over_b"] = res["c_host_ms"] / res["b_host_ms"]
    f = lambda v: "%.3f" % v
    rng = lambda v: "—" if not v else "%.3f – %.3f" % (min(v), max(v))
    md = ["# r31: the true-peak bar's reading series — one call at P = 4800 against the dense call and against 100 calls + results\n",
          f"Made by `python tools/tpb_series_rate.py {reps}` on {res['box']}: {res['shape']}.\n",
          "| configuration | launches | device ms (median) | min – max | host ms around call(s) + wait (median) | min – max |",
          "|---|---|---|---|---|---|",
          f"| (a) dense call, P = 0 (`k_tpb<2, false>`) | 2 | {f(res['a_ms'])} | {rng(dev['a'])} | {f(res['a_host_ms'])} | {rng(host['a'])} |",
          f"| (b) one call, P = 4800, 100 points (`k_tpb<2, true>`) | 2 | {f(res['b_ms'])} | {rng(dev['b'])} | {f(res['b_host_ms'])} | {rng(host['b'])} |",
          f"| (c) P = 0 engine: 100 calls of 4800 frames, `mtr_engine_results` after each | 200 | — | — | {f(res['c_host_ms'])} | {rng(host['c'])} |",
          "",
          f"(b) / (a) = {f(res['b_over_a'])} (device time); (c) / (b) = {f(res['c_over_b'])} (host time).  The last point of (b) against the last call of (c), "
          f"worst relative difference over the {2 * S} (stream, channel)s: {worst:.2e}.\n"]
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, PROFILE)
    old = open(path).read() if os.path.exists(path) else ""
    at = old.find("\n## ")                                                 # the tool owns the file down to its first section; what was written
    md.append(old[at + 1:] if at >= 0 else "")                             # by hand behind that stays
    open(path, "w").write("\n".join(md))
    print(json.dumps(res), flush=True)


def dense(reps):
    """the dense call alone, of whichever library MTR_LIB names: one table row"""
    import numpy as np
    import torch
    import meters.lv2_amd as M
    buf = buffer(M, torch)
    st = torch.cuda.current_stream().cuda_stream
    t = []
    with M.Engine(S, FS, M.METER_TPBALLIST) as e:
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for it in range(WARM + reps):
            ev0.record()
            e.process_device(buf.data_ptr(), T, T, st)
            ev1.record()
            e.sync()
            torch.cuda.synchronize()
            if it >= WARM:
                t.append(ev0.elapsed_time(ev1))
    v = np.asarray(t)
    print("| %s | %.3f | %.3f | %.3f |" % ("parent" if os.environ.get("MTR_LIB") else "this build", np.median(v), v.min(), v.max()), flush=True)


def pairs(n, reps):
    if not os.path.exists(LIB_AB):
        sys.exit("no meters.lv2_amd/lib_ab: tools/build_ab.sh")
    print("| library (dense call, P = 0) | median ms | min | max |\n|---|---|---|---|", flush=True)
    for _ in range(n):
        for lib in (None, LIB_AB):                                          # a fresh child each: nothing of one library's session is left for the other
            env = {k: v for k, v in os.environ.items() if k != "MTR_LIB"}
            if lib:
                env["MTR_LIB"] = lib
            subprocess.run([sys.executable, os.path.abspath(__file__), "--dense", str(reps)], env=env, check=True, timeout=300)


if __name__ == "__main__":
    args = sys.argv[1:]
    out = os.path.join(ROOT, "profiles")
    if "--out" in args:
        i = args.index("--out")
        out = args[i + 1]
        del args[i:i + 2]
    if "--pairs" in args:
        i = args.index("--pairs")
        pairs(int(args[i + 1]), int(args[i + 2]) if len(args) > i + 2 else 9)
    elif "--dense" in args:
        i = args.index("--dense")
        dense(int(args[i + 1]) if len(args) > i + 1 else 9)
    else:
        turns(int(args[0]) if args else 9, out)
