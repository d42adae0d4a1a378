"""tools/bank_series_rate.py — what the 30-band bank's reading series (mtr_engine_spectr_set_period, the second instantiation of k_bank)
costs.  GPU box only.

One session; per shape — config 3's 4096 streams x 10 s of stereo f32 at 48 kHz, then 8192 x 10 s — one buffer (the bench programme:
mtr_synth_fill_device kind 1) and these configurations, which take turns on it after two warm-up rounds:
  (a) the dense call at P = 0: one spectrum_run per stream (k_bank as it was);
  (b) one call at P = 4800 with a series of 100 points per stream (k_bank's series instantiation);
  (c) what a caller had to do before the series existed: the P = 0 engine called 100 times with 4800 frames and mtr_engine_spectrum after
      each — 100 host waits and 200 device-to-host copies;
  (p) where meters.lv2_amd/lib_ab exists (tools/build_ab.sh: the parent commit's library, loaded beside this build's through its C
      ABI): its dense call, in the same turns — the same-box alternating pairs that hold (a) against the parent.
Each turn is timed on the host around the call(s) and the wait for them (what the caller sees); (a), (b) and (p) also by device events
around the call.  (b)'s last point and (c)'s last reading are compared bit for bit.  Prints one JSON object per shape — the bytes each
must read, every time, the medians, (b) / (a) against (a)'s own min - max spread, (c) / (b), (a) / (p) — and writes the head of
r24_bank_series.md in --out (default profiles/): the tables; the sections that follow them there are written by hand and kept.
    python tools/bank_series_rate.py [reps] [--out DIR]
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

FS, T, P = 48000.0, 480000, 4800
SHAPES = (4096, 8192)
WARM = 2
LIB_AB = os.path.join(ROOT, "meters.lv2_amd", "lib_ab", "libmtr_engine.so")


def buffer(S):
    buf = torch.empty((S, T, 2), dtype=torch.float32, device="cuda")
    M.synth_fill_device(buf.data_ptr(), S, T, T, 777, FS, 1)
    torch.cuda.synchronize()
    return buf


class Parent:
    """a SPECTR30 engine of the parent commit's library, through the C ABI alone"""

    def __init__(self, path, S):
        L = self.L = C.CDLL(path)
        vp, u64 = C.c_void_p, C.c_uint64
        L.mtr_engine_create.argtypes = [C.c_void_p, C.POINTER(vp)]
        L.mtr_engine_destroy.argtypes = [vp]
        L.mtr_engine_destroy.restype = None
        L.mtr_engine_process_device.argtypes = [vp, vp, u64, u64, vp]
        L.mtr_engine_reset.argtypes = [vp]
        L.mtr_engine_sync.argtypes = [vp]
        L.mtr_last_error.restype = C.c_char_p
        cfg = M.engine._Config(struct_size=C.sizeof(M.engine._Config), meters=M.METER_SPECTR30, n_streams=S, n_channels=2, sample_rate=FS, device=0)
        self.h = vp()
        rc = L.mtr_engine_create(C.byref(cfg), C.byref(self.h))
        if rc:
            raise RuntimeError(f"{path}: mtr_engine_create failed ({rc}): {L.mtr_last_error().decode()}")

    def reset(self):
        self.L.mtr_engine_reset(self.h)

    def process_device(self, ptr, n, stride, st):
        rc = self.L.mtr_engine_process_device(self.h, ptr, n, stride, st)
        if rc:
            raise RuntimeError(f"parent library: the call failed ({rc}): {self.L.mtr_last_error().decode()}")

    def sync(self):
        self.L.mtr_engine_sync(self.h)

    def close(self):
        self.L.mtr_engine_destroy(self.h)


def turns(S, reps):
    buf = buffer(S)
    st = torch.cuda.current_stream().cuda_stream
    ea, eb, ec = (M.Engine(S, FS, M.METER_SPECTR30) for _ in range(3))
    eb.spectr_set_period(P, T // P)
    parent = Parent(LIB_AB, S) if os.path.exists(LIB_AB) else None
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    host = {k: [] for k in "abcp"}
    dev = {k: [] for k in "abp"}
    last = None

    def one(e):
        ev[0].record()
        e.process_device(buf.data_ptr(), T, T, st)
        ev[1].record()
        e.sync()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1])

    single = [(k, e) for k, e in (("a", ea), ("b", eb), ("p", parent)) if e is not None]
    for it in range(WARM + reps):
        # the single calls change places turn by turn: whichever comes first follows (c)'s hundred short calls and their copies, and runs
        # about 1.5 % slower at 4096 streams for it (measured with the order fixed: the same instructions, (a) behind (c) against (p) behind (b))
        for key, e in single[it % len(single):] + single[:it % len(single)]:
            e.reset()                                                      # (every turn is the call from a fresh engine's state: (b) appends its 100 points to an empty series)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            d = one(e)
            h = (time.perf_counter() - t0) * 1e3
            if it >= WARM:
                host[key].append(h)
                dev[key].append(d)
        ec.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(T // P):
            ec.process_device(buf.data_ptr() + k * P * 8, P, T, st)
            last = ec.spectrum()
        h = (time.perf_counter() - t0) * 1e3
        if it >= WARM:
            host["c"].append(h)
    ser, n, dropped = eb.spectr_series()
    assert n == T // P and dropped == 0 and np.isfinite(ser["val"]).all()
    same = all(np.array_equal(ser[k][:, -1].view(np.uint32), last[k].view(np.uint32)) for k in ("val", "max", "val_db", "max_db"))
    for e in (ea, eb, ec) + ((parent,) if parent else ()):
        e.close()
    del buf
    torch.cuda.empty_cache()
    med = lambda v: float(np.median(v)) if v else None                     # noqa: E731
    res = {"box": f"{torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName})",
           "shape": f"{S} streams x {T // int(FS)} s stereo f32 at {int(FS)} Hz, {reps} turns after {WARM} warm ones", "streams": S,
           "bytes_read": {k: S * T * 8 for k in "abcp"},
           "bytes_back_to_the_host": {"a": 0, "b": 0, "c": (T // P) * S * 2 * M.engine.NBANDS * 4, "p": 0},
           "launches": {"a": 1, "b": 1, "c": T // P, "p": 1}, "host_waits": {"a": 1, "b": 1, "c": T // P, "p": 1},
           "series_last_point_equals_loop_last_reading": bool(same),
           "host_ms": host, "device_ms": dev,
           "a_ms": med(dev["a"]), "b_ms": med(dev["b"]), "p_ms": med(dev["p"]),
           "a_host_ms": med(host["a"]), "b_host_ms": med(host["b"]), "c_host_ms": med(host["c"])}
    res["a_spread_ms"] = [min(dev["a"]), max(dev["a"])]
    res["b_over_a"] = res["b_ms"] / res["a_ms"]
    res["b_inside_a_spread"] = bool(min(dev["a"]) <= res["b_ms"] <= max(dev["a"]))
    res["c_over_b"] = res["c_host_ms"] / res["b_host_ms"]
    res["a_over_p"] = res["a_ms"] / res["p_ms"] if parent else None
    assert same, "the series' last point is not the loop's last reading"
    return res


def table(res, reps):
    S = res["streams"]
    f = lambda v: "not run (no meters.lv2_amd/lib_ab: tools/build_ab.sh)" if v is None else "%.3f" % v   # noqa: E731
    rng = lambda v: "—" if not v else "%.3f – %.3f" % (min(v), max(v))                                     # noqa: E731
    gb, dev, host = S * T * 8 / 1e9, res["device_ms"], res["host_ms"]
    return [f"### {res['shape']}\n",
            "| configuration | must read | launches / host waits | device ms (median) | min – max | host ms around call(s) + wait (median) | min – max |",
            "|---|---|---|---|---|---|---|",
            f"| (a) dense call, P = 0 | {gb:.1f} GB | 1 / 1 | {f(res['a_ms'])} | {rng(dev['a'])} | {f(res['a_host_ms'])} | {rng(host['a'])} |",
            f"| (b) one call, P = 4800, 100 points per stream | {gb:.1f} GB | 1 / 1 | {f(res['b_ms'])} | {rng(dev['b'])} | {f(res['b_host_ms'])} | {rng(host['b'])} |",
            f"| (c) P = 0, 100 calls of 4800 frames, mtr_engine_spectrum after each | {gb:.1f} GB + {res['bytes_back_to_the_host']['c'] / 1e6:.0f} MB over the link in 200 copies | 100 / 100 | — | — | {f(res['c_host_ms'])} | {rng(host['c'])} |",
            f"| (p) parent library's dense call | {gb:.1f} GB | 1 / 1 | {f(res['p_ms'])} | {rng(dev['p'])} | {f(float(np.median(host['p'])) if host['p'] else None)} | {rng(host['p'])} |",
            "",
            f"(b) / (a) = {f(res['b_over_a'])} (device time, medians); (a)'s own spread is {rng(dev['a'])} ms and (b)'s median lies "
            f"{'inside' if res['b_inside_a_spread'] else 'OUTSIDE'} it.  (c) / (b) = {f(res['c_over_b'])} (host time).  (a) / (p) = {f(res['a_over_p'])} (device time).  "
            f"(b)'s last point equals (c)'s last reading bit for bit: {res['series_last_point_equals_loop_last_reading']}.\n"]


if __name__ == "__main__":
    args = sys.argv[1:]
    out = os.path.join(ROOT, "profiles")
    if "--out" in args:
        i = args.index("--out")
        out = args[i + 1]
        del args[i:i + 2]
    reps = int(args[0]) if args else 12
    md = ["# r24: the bank's reading series — one call at P = 4800 against the dense call and against 100 calls + readings\n"]
    for S in SHAPES:
        res = turns(S, reps)
        print(json.dumps(res), flush=True)
        if len(md) == 1:
            md.append(f"Made by `python tools/bank_series_rate.py {reps}` on {res['box']}, the configurations taking turns, the single calls in rotating order.\n")
        md += table(res, reps)
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, "r24_bank_series.md")
    old = open(path).read() if os.path.exists(path) else ""
    at = old.find("\n## ")                                                 # the tool owns the file down to its first section; what was written
    md.append(old[at + 1:] if at >= 0 else "")                             # by hand behind that stays
    open(path, "w").write("\n".join(md))
