"""tools/bank_ends_rate.py — what track lengths cost and save in the 30-band bank (mtr_engine_process_device_ends, the two ENDS
instantiations of k_bank).  GPU box only.

One session; per shape — config 3's 4096 streams x 10 s of stereo f32 at 48 kHz, then 8192 x 10 s — one buffer (the bench programme:
mtr_synth_fill_device kind 1), and for P = 0 and P = 4800 (a series of 100 points per stream) these calls, which take turns on it after
two warm-up rounds, in rotating order, each from a freshly reset engine:
  (d)  the dense call of n frames (mtr_engine_process_device: k_bank as it was);
  (o)  _ends with every stream open, frames[s] = n;
  (q)  _ends with every end at n / 4;
  (dq) the dense call of n / 4 frames on the same buffer: what (q) should cost;
  (u)  _ends with lengths uniform in [0, n] (seeded).
Every call is timed by device events around it.  Prints one JSON object per shape and period — the frames each call must compute, every
time, the medians, (o) / (d) with both spreads, (q) against (dq) within twice (dq)'s own min - max spread, (u) / (d) beside the share of
the frames — and writes the head of r26_bank_ends.md in --out (default profiles/): the tables; the sections that follow them there are
written by hand and kept.
    python tools/bank_ends_rate.py [reps] [--out DIR]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import meters.lv2_amd as M  # noqa: E402

FS, T = 48000.0, 480000
PERIODS = (0, 4800)
SHAPES = (4096, 8192)
WARM = 2
KEYS = ("d", "o", "q", "dq", "u")
NAMES = {"d": "(d) dense call, n frames", "o": "(o) _ends, every stream open", "q": "(q) _ends, every end at n / 4",
         "dq": "(dq) dense call of n / 4 frames", "u": "(u) _ends, lengths uniform in [0, n]"}


def buffer(S):
    buf = torch.empty((S, T, 2), dtype=torch.float32, device="cuda")
    M.synth_fill_device(buf.data_ptr(), S, T, T, 777, FS, 1)
    torch.cuda.synchronize()
    return buf


def turns(buf, S, period, reps):
    st = torch.cuda.current_stream().cuda_stream
    frames = {"o": np.full(S, T, np.uint64), "q": np.full(S, T // 4, np.uint64),
              "u": np.random.default_rng(2600 + S).integers(0, T + 1, S).astype(np.uint64)}
    eng = {k: M.Engine(S, FS, M.METER_SPECTR30) for k in KEYS}
    for e in eng.values():
        e.spectr_set_period(period, T // period if period else 0)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    dev = {k: [] for k in KEYS}
    order = list(KEYS)
    for it in range(WARM + reps):
        for k in order[it % len(order):] + order[:it % len(order)]:
            e = eng[k]
            e.reset()                                            # (a closing call closes its streams until the reset)
            torch.cuda.synchronize()
            ev[0].record()
            if k == "d":
                e.process_device(buf.data_ptr(), T, T, st)
            elif k == "dq":
                e.process_device(buf.data_ptr(), T // 4, T, st)
            else:
                e.process_device_ends(buf.data_ptr(), T, frames[k], T, st)
            ev[1].record()
            e.sync()
            torch.cuda.synchronize()
            if it >= WARM:
                dev[k].append(ev[0].elapsed_time(ev[1]))
    # the answers behind the last turn: (o) is (d), (q) is (dq), bit for bit
    sp = {k: eng[k].spectrum() for k in KEYS}
    same = lambda a, b: all(np.array_equal(sp[a][x].view(np.uint32), sp[b][x].view(np.uint32)) for x in ("val", "max"))   # noqa: E731
    checks = {"open_equals_dense": bool(same("o", "d")), "quarter_equals_dense_quarter": bool(same("q", "dq")),
              "uniform_finite": bool(np.isfinite(sp["u"]["val"]).all())}
    if period:
        pts = eng["u"].spectr_points()
        want = np.array([sum(M.series_cut(0, period, T, int(f))) for f in frames["u"]], np.uint64)
        checks["uniform_points_are_series_cut"] = bool(np.array_equal(pts, want))
    for e in eng.values():
        e.close()
    med = lambda v: float(np.median(v))                                    # noqa: E731
    res = {"box": f"{torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName})",
           "shape": f"{S} streams x {T // int(FS)} s stereo f32 at {int(FS)} Hz, P = {period}, {reps} turns after {WARM} warm ones", "streams": S, "period": period,
           "frames_computed": {"d": S * T, "o": S * T, "q": S * (T // 4), "dq": S * (T // 4), "u": int(frames["u"].sum())},
           "device_ms": dev, "median_ms": {k: med(dev[k]) for k in KEYS}, "spread_ms": {k: [min(dev[k]), max(dev[k])] for k in KEYS}, "checks": checks}
    m = res["median_ms"]
    res["o_over_d"] = m["o"] / m["d"]
    res["q_minus_dq_ms"] = m["q"] - m["dq"]
    res["twice_dq_spread_ms"] = 2 * (max(dev["dq"]) - min(dev["dq"]))
    res["q_within_twice_dq_spread"] = bool(abs(res["q_minus_dq_ms"]) <= res["twice_dq_spread_ms"])
    res["u_over_d"] = m["u"] / m["d"]
    res["u_frames_share"] = res["frames_computed"]["u"] / (S * T)
    assert all(checks.values()), checks
    return res


def table(res):
    dev, m, fr = res["device_ms"], res["median_ms"], res["frames_computed"]
    out = [f"### {res['shape']}\n", "| call | frames it must compute | device ms (median) | min – max |", "|---|---|---|---|"]
    out += [f"| {NAMES[k]} | {fr[k] / 1e6:.1f} M | {m[k]:.3f} | {min(dev[k]):.3f} – {max(dev[k]):.3f} |" for k in KEYS]
    out += ["",
            f"(o) / (d) = {res['o_over_d']:.4f} (medians; spreads above).  (q) − (dq) = {res['q_minus_dq_ms']:+.3f} ms against twice (dq)'s own spread, "
            f"{res['twice_dq_spread_ms']:.3f} ms: {'inside' if res['q_within_twice_dq_spread'] else 'OUTSIDE'}.  (u) / (d) = {res['u_over_d']:.3f} at "
            f"{res['u_frames_share']:.3f} of the frames.  Checks: {json.dumps(res['checks'])}.\n"]
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    out = os.path.join(ROOT, "profiles")
    if "--out" in args:
        i = args.index("--out")
        out = args[i + 1]
        del args[i:i + 2]
    reps = int(args[0]) if args else 10
    md = ["# r26: track lengths in the 30-band bank — _ends against the dense call, every end at n / 4, uniform lengths\n"]
    for S in SHAPES:
        buf = buffer(S)
        for period in PERIODS:
            res = turns(buf, S, period, reps)
            print(json.dumps(res), flush=True)
            if len(md) == 1:
                md.append(f"Made by `python tools/bank_ends_rate.py {reps}` on {res['box']}, the calls taking turns in rotating order, each from a reset engine.\n")
            md += table(res)
        del buf
        torch.cuda.empty_cache()
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, "r26_bank_ends.md")
    old = open(path).read() if os.path.exists(path) else ""
    at = old.find("\n## ")                                                 # the tool owns the file down to its first section; what was written
    md.append(old[at + 1:] if at >= 0 else "")                             # by hand behind that stays
    open(path, "w").write("\n".join(md))
