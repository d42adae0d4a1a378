"""tools/tpb_ends_rate.py — what track lengths cost the true-peak bar (mtr_engine_process_*_tpb, the ENDS instantiations of k_tpb), and what
they save.  GPU box only.

One session, one buffer (8192 streams x 10 s of stereo f32 at 48 kHz, the bench programme: mtr_synth_fill_device kind 1).  At P = 0 and at
P = 4800 five forms take turns on it in rotating order after two warm-up rounds, each from a reset engine, timed by device events around
the call:
  (a) the dense call;
  (b) _tpb with every stream open (frames[s] == n_frames): the ENDS kernel walking what the dense one walks;
  (c) _tpb with every end at a quarter of the call, next to
  (d) the dense call of that quarter;
  (e) _tpb with lengths uniform in [0, 10 s].
A workgroup runs to the last end among its 32 streams, so (e) walks more than half of the chunks: the tool prints the chunks each form
must walk.  Prints everything as one JSON object and writes the head of profiles/r32_tpb_ends.md — the tables and the ratios; the sections
that follow it there are written by hand and kept.
    python tools/tpb_ends_rate.py [reps] [--out DIR]

    python tools/tpb_ends_rate.py --pairs N [reps]
holds the dense call of this build against the parent's library (tools/build_ab.sh -> meters.lv2_amd/lib_ab): N pairs of child
processes, this build and the parent alternating on the same box, each timing the dense call `reps` times (--dense, with MTR_LIB naming
the library); prints a table row per child.
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

FS, S, T = 48000.0, 8192, 480000
PERIODS = (0, 4800)
WARM = 2
WG = 32                                   # stereo streams per workgroup of k_tpb
LIB_AB = os.path.join(ROOT, "meters.lv2_amd", "lib_ab", "libmtr_engine.so")
PROFILE = "r32_tpb_ends.md"
FORMS = ["a", "b", "c", "d", "e"]
NAMES = {"a": "(a) dense call", "b": "(b) `_tpb`, every stream open", "c": "(c) `_tpb`, every end at T / 4", "d": "(d) dense call of T / 4 frames",
         "e": "(e) `_tpb`, lengths uniform in [0, T]"}


def buffer(M, torch):
    buf = torch.empty((S, T, 2), dtype=torch.float32, device="cuda")
    M.synth_fill_device(buf.data_ptr(), S, T, T, 777, FS, 1)
    torch.cuda.synchronize()
    return buf


def chunks(frames):
    """16-frame chunks the workgroups walk: each runs to the last end among its streams"""
    import numpy as np
    last = np.asarray(frames, np.int64).reshape(-1, WG).max(axis=1)
    return int(((last + 15) // 16).sum())


def turns(reps, out):
    import numpy as np
    import torch
    import meters.lv2_amd as M
    buf = buffer(M, torch)
    st = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(32)
    frames = {"b": np.full(S, T, np.uint64), "c": np.full(S, T // 4, np.uint64), "e": rng.integers(0, T + 1, S).astype(np.uint64)}
    walked = {"a": chunks(np.full(S, T)), "b": chunks(frames["b"]), "c": chunks(frames["c"]), "d": chunks(np.full(S, T // 4)), "e": chunks(frames["e"])}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    dev = {P: {k: [] for k in FORMS} for P in PERIODS}
    eng = {}
    for P in PERIODS:
        eng[P] = M.Engine(S, FS, M.METER_TPBALLIST)
        if P:
            eng[P].tpb_set_period(P, T // P)

    def one(e, key):
        e.reset()
        torch.cuda.synchronize()
        ev[0].record()
        if key == "a":
            e.process_device(buf.data_ptr(), T, T, st)
        elif key == "d":
            e.process_device(buf.data_ptr(), T // 4, T, st)
        else:
            e.process_device_tpb(buf.data_ptr(), T, frames[key], T, st)
        ev[1].record()
        e.sync()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1])

    jobs = [(P, k) for P in PERIODS for k in FORMS]
    for it in range(WARM + reps):
        r = it % len(jobs)
        for P, key in jobs[r:] + jobs[:r]:                                  # rotating order: nobody always runs behind the same neighbour
            d = one(eng[P], key)
            if it >= WARM:
                dev[P][key].append(d)
    pts = eng[4800].tpb_points()
    assert int(pts.sum()) == int(sum(int(f) // 4800 + (1 if int(f) % 4800 and int(f) < T else 0) for f in frames["e"]))
    for e in eng.values():
        e.close()
    med = lambda v: float(np.median(v))
    res = {"box": f"{torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName})",
           "shape": f"{S} streams x {T // int(FS)} s stereo f32 at {int(FS)} Hz, {reps} turns after {WARM} warm ones, rotating order",
           "chunks": walked, "share_of_dense_chunks": {k: walked[k] / walked["a"] for k in FORMS},
           "device_ms": {str(P): dev[P] for P in PERIODS},
           "median_ms": {str(P): {k: med(dev[P][k]) for k in FORMS} for P in PERIODS}}
    res["ratios"] = {str(P): {"b_over_a": med(dev[P]["b"]) / med(dev[P]["a"]), "c_over_d": med(dev[P]["c"]) / med(dev[P]["d"]),
                              "e_over_a": med(dev[P]["e"]) / med(dev[P]["a"])} for P in PERIODS}
    f = lambda v: "%.3f" % v
    span = lambda v: "—" if not v else "%.3f – %.3f" % (min(v), max(v))
    md = ["# r32: track lengths for the true-peak bar — the ENDS instantiations of `k_tpb` against the dense call of the same session\n",
          f"Made by `python tools/tpb_ends_rate.py {reps}` on {res['box']}: {res['shape']}.\n"]
    for P in PERIODS:
        md += [f"P = {P}:\n", "| form | chunks walked | share of the dense call's | device ms (median) | min – max |", "|---|---|---|---|---|"]
        md += [f"| {NAMES[k]} | {walked[k]} | {f(walked[k] / walked['a'])} | {f(med(dev[P][k]))} | {span(dev[P][k])} |" for k in FORMS]
        q = res["ratios"][str(P)]
        md += ["", f"(b) / (a) = {f(q['b_over_a'])}; (c) / (d) = {f(q['c_over_d'])}; (e) / (a) = {f(q['e_over_a'])} at {f(walked['e'] / walked['a'])} of the chunks.\n"]
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
