"""tools/kmeter_rate.py — what the K-meter's reading series (mtr_engine_kmeter_set_period, k_kmeter_blocks) costs.  GPU box only.

One session, one buffer (8192 streams x 10 s of stereo f32 at 48 kHz, the bench programme: mtr_synth_fill_device kind 1), three
configurations that take turns on it after two warm-up rounds:
  (a) the dense call at P = 0: one Kmeterdsp::process () per stream (k_kmeter_pieces);
  (b) one call at P = 4800 with a series of 100 points (k_kmeter_blocks + k_kmeter_walk);
  (c) what a caller had to do before the series existed: the PARENT commit's library (tools/build_ab.sh -> meters.lv2_amd/lib_ab,
      loaded beside this build's through its C ABI), 100 calls of 4800 frames with mtr_engine_kmeter_read after each.
Each turn is timed on the host around the call(s) and the wait for them (what the caller sees); (a) and (b) also by device events
around the call.  Prints the bytes each must read, the medians, (b) / (a) and (c) / (b) as one JSON object and writes the head of
profiles/r22_kmeter_series.md — the table and the ratios; the sections that follow it there are written by hand and kept.
    python tools/kmeter_rate.py [reps] [--out DIR]

    python tools/kmeter_rate.py --ebu [reps]
times the bench step instead (EBU R128 + true peak on the same buffer, integration on): run it once per library (MTR_LIB names
another build of libmtr_engine.so) to hold a build against its parent, in same-box pairs.

    python tools/kmeter_rate.py --dense [reps]
times the dense call alone, (a), by device events and prints median / min / max as one JSON line: run it in child processes that
take turns, one with MTR_LIB on the parent's library (tools/build_ab.sh) and one without, to hold k_kmeter_pieces against its parent.
"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import meters.lv2_amd as M  # noqa: E402

FS, S, T, P = 48000.0, 8192, 480000, 4800
HBM_PEAK = 8.0e12
WARM = 2
LIB_AB = os.path.join(ROOT, "meters.lv2_amd", "lib_ab", "libmtr_engine.so")


def buffer():
    buf = torch.empty((S, T, 2), dtype=torch.float32, device="cuda")
    M.synth_fill_device(buf.data_ptr(), S, T, T, 777, FS, 1)
    torch.cuda.synchronize()
    return buf


class Parent:
    """a KMETER engine of the parent commit's library, through the C ABI alone"""

    def __init__(self, path):
        L = self.L = C.CDLL(path)
        vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
        L.mtr_engine_create.argtypes = [C.c_void_p, C.POINTER(vp)]
        L.mtr_engine_destroy.argtypes = [vp]
        L.mtr_engine_destroy.restype = None
        L.mtr_engine_process_device.argtypes = [vp, vp, u64, u64, vp]
        L.mtr_engine_kmeter_read.argtypes = [vp, u32, u32, vp, vp]
        L.mtr_engine_kmeter_reset.argtypes = [vp]
        L.mtr_last_error.restype = C.c_char_p
        cfg = M.engine._Config(struct_size=C.sizeof(M.engine._Config), meters=M.METER_KMETER, n_streams=S, n_channels=2, sample_rate=FS, device=0)
        self.h = vp()
        rc = L.mtr_engine_create(C.byref(cfg), C.byref(self.h))
        if rc:
            raise RuntimeError(f"{path}: mtr_engine_create failed ({rc}): {L.mtr_last_error().decode()}")
        self.rms, self.peak = np.zeros((S, 2), np.float32), np.zeros((S, 2), np.float32)

    def trace(self, ptr, st):
        """100 calls of P frames, a read after each: returns nothing — the readings land in self.rms / self.peak one after the other"""
        for k in range(T // P):
            rc = self.L.mtr_engine_process_device(self.h, ptr + k * P * 8, P, T, st) or self.L.mtr_engine_kmeter_read(self.h, 0, S, self.rms.ctypes.data, self.peak.ctypes.data)
            if rc:
                raise RuntimeError(f"parent library: call {k} failed ({rc}): {self.L.mtr_last_error().decode()}")

    def close(self):
        self.L.mtr_engine_destroy(self.h)


def turns(reps, out):
    buf = buffer()
    st = torch.cuda.current_stream().cuda_stream
    ea, eb = M.Engine(S, FS, M.METER_KMETER), M.Engine(S, FS, M.METER_KMETER)
    eb.kmeter_set_period(P, T // P)
    parent = Parent(LIB_AB) if os.path.exists(LIB_AB) else None
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    host = {"a": [], "b": [], "c": []}
    dev = {"a": [], "b": []}

    def one(e):
        ev[0].record()
        e.process_device(buf.data_ptr(), T, T, st)
        ev[1].record()
        e.sync()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1])

    for it in range(WARM + reps):
        for key, e in (("a", ea), ("b", eb)):
            if key == "b":
                eb.kmeter_reset()                                          # (every turn appends its 100 points to an empty series)
            t0 = time.perf_counter()
            d = one(e)
            h = (time.perf_counter() - t0) * 1e3
            if it >= WARM:
                host[key].append(h)
                dev[key].append(d)
        if parent:
            parent.L.mtr_engine_kmeter_reset(parent.h)                     # (as (b): every turn is the trace from the constructor's state)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            parent.trace(buf.data_ptr(), st)
            h = (time.perf_counter() - t0) * 1e3
            if it >= WARM:
                host["c"].append(h)
    rms, peak, n, dropped = eb.kmeter_series()
    assert n == T // P and dropped == 0 and np.isfinite(rms).all()
    if parent:                                                             # the same trace's last point, by the rule of tests/test_gpu_kmeter.py
        assert np.array_equal(peak[:, -1], parent.peak) and (np.abs(rms[:, -1] - parent.rms) <= 1e-5 * np.maximum(parent.rms, 1e-3)).all()
        parent.close()
    ea.close()
    eb.close()
    med = lambda v: float(np.median(v)) if v else None
    res = {"box": f"{torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName})",
           "shape": f"{S} streams x {T // int(FS)} s stereo f32 at {int(FS)} Hz, {reps} turns after {WARM} warm ones",
           "bytes_read": {"a": S * T * 8, "b": S * T * 8, "c": S * T * 8},
           "bytes_back_to_the_host": {"a": 0, "b": 0, "c": (T // P) * S * 2 * 24},   # (kmeter_read copies the [S][2] states out, and back to arm the flag)
           "launches": {"a": 2, "b": 2, "c": 2 * (T // P)},
           "host_ms": host, "device_ms": dev,
           "a_ms": med(dev["a"]), "b_ms": med(dev["b"]), "a_host_ms": med(host["a"]), "b_host_ms": med(host["b"]), "c_host_ms": med(host["c"])}
    res["b_over_a"] = res["b_ms"] / res["a_ms"]
    res["c_over_b"] = res["c_host_ms"] / res["b_host_ms"] if parent else None
    res["a_HBM_share"] = S * T * 8 / (res["a_ms"] * 1e-3) / HBM_PEAK
    res["b_HBM_share"] = S * T * 8 / (res["b_ms"] * 1e-3) / HBM_PEAK
    f = lambda v: "not run (no meters.lv2_amd/lib_ab: tools/build_ab.sh)" if v is None else "%.3f" % v
    rng = lambda v: "—" if not v else "%.3f – %.3f" % (min(v), max(v))
    md = ["# r22: the K-meter's reading series — one call at P = 4800 against the dense call and against 100 calls + reads\n",
          f"Made by `python tools/kmeter_rate.py {reps}` on {res['box']}: {res['shape']}, the configurations taking turns.\n",
          "| configuration | must read | launches | device ms (median) | min – max | host ms around call + wait (median) | min – max |",
          "|---|---|---|---|---|---|---|",
          f"| (a) dense call, P = 0 (k_kmeter_pieces) | {S * T * 8 / 1e9:.1f} GB | 2 | {f(res['a_ms'])} | {rng(dev['a'])} | {f(res['a_host_ms'])} | {rng(host['a'])} |",
          f"| (b) one call, P = 4800, 100 points (k_kmeter_blocks) | {S * T * 8 / 1e9:.1f} GB | 2 | {f(res['b_ms'])} | {rng(dev['b'])} | {f(res['b_host_ms'])} | {rng(host['b'])} |",
          f"| (c) parent library: 100 calls of 4800 frames, kmeter_read after each | {S * T * 8 / 1e9:.1f} GB + {res['bytes_back_to_the_host']['c'] / 1e6:.0f} MB over the link | 200 | — | — | {f(res['c_host_ms'])} | {rng(host['c'])} |",
          "",
          f"(b) / (a) = {f(res['b_over_a'])} (device time); (c) / (b) = {f(res['c_over_b'])} (host time).  Reading the buffer once in (a)'s time is "
          f"{100 * res['a_HBM_share']:.1f} % of the 8.0 TB/s HBM peak, in (b)'s {100 * res['b_HBM_share']:.1f} %.\n"]
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, "r22_kmeter_series.md")
    old = open(path).read() if os.path.exists(path) else ""
    at = old.find("\n## ")                                                 # the tool owns the file down to its first section; what was written
    md.append(old[at + 1:] if at >= 0 else "")                             # by hand behind that (what the numbers say, the --ebu pairs) stays
    open(path, "w").write("\n".join(md))
    print(json.dumps(res), flush=True)


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


def dense(reps):
    buf = buffer()
    st = torch.cuda.current_stream().cuda_stream
    t = []
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with M.Engine(S, FS, M.METER_KMETER) as e:
        for it in range(WARM + reps):
            ev0.record()
            e.process_device(buf.data_ptr(), T, T, st)
            ev1.record()
            e.sync()
            torch.cuda.synchronize()
            if it >= WARM:
                t.append(ev0.elapsed_time(ev1))
        rms, peak = e.kmeter_read()
    assert np.isfinite(rms).all() and (rms > 0).all()
    v = np.asarray(t)
    print(json.dumps({"dense_kmeter_ms": {"lib": os.environ.get("MTR_LIB") or "this build", "median": float(np.median(v)), "min": float(v.min()),
                                          "max": float(v.max()), "reps": reps}}), flush=True)


if __name__ == "__main__":
    if "--dense" in sys.argv[1:]:
        rest = [a for a in sys.argv[1:] if a != "--dense"]
        dense(int(rest[0]) if rest else 9)
        sys.exit(0)
    args = [a for a in sys.argv[1:] if a != "--ebu"]
    out = os.path.join(ROOT, "profiles")
    if "--out" in args:
        i = args.index("--out")
        out = args[i + 1]
        del args[i:i + 2]
    n = int(args[0]) if args else 9
    bench_step(n) if "--ebu" in sys.argv[1:] else turns(n, out)
