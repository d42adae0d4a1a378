"""tools/any_ends_rate.py — what track lengths cost the scope and the surround meter (mtr_engine_process_*_any: the ENDS instantiations of
k_scope, the LEN instantiations of k_sur_pieces / k_sur_final), and what they save.  GPU box only.

One session, one buffer per meter: SCOPE at W 1024 and H 1920 on 8192 streams x 10 s of stereo f32 at 48 kHz (the bench programme:
mtr_synth_fill_device kind 1), then SURROUND without a period and at P = 4800 on 8192 streams x 10 s of 6-channel f32 (uniform noise, a
gain per channel: the buffer of tools/surround_rate.py).  Five forms take turns on the buffer in rotating order after two warm-up rounds, each from a reset
engine, timed by device events around the call:
  (a) the dense call;
  (b) _any with every stream open (frames[s] == n_frames): the ENDS kernel running the analyses the dense one runs;
  (c) _any with every end at a quarter of the call, next to
  (d) the dense call of that quarter;
  (e) _any with lengths uniform in [0, 10 s].
A workgroup of k_scope is one stream and runs the stream's own analyses, W frames each (H > W: the frames between two windows are never
read), then stores its tail; one of k_sur_pieces is one (stream, piece) and reads the piece's frames up to the stream's end, once.  The tool
prints the analyses (frames, for the surround meter) and the bytes each form must read.  Prints everything as one JSON object and writes
the head of profiles/r33_any_ends.md — the tables and the ratios; the sections that follow it there are written by hand and kept.
    python tools/any_ends_rate.py [reps] [--out DIR]

    python tools/any_ends_rate.py --pairs N [reps]
holds the dense call of this build against the parent's library (tools/build_ab.sh -> meters.lv2_amd/lib_ab): N pairs of child
processes, this build and the parent alternating on the same box, each timing the dense call `reps` times (--dense, with MTR_LIB naming
the library) for the scope, then for the surround meter; prints a table row per child.
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

FS, S, T = 48000.0, 8192, 480000
W, H = 1024, 1920
WARM = 2
LIB_AB = os.path.join(ROOT, "meters.lv2_amd", "lib_ab", "libmtr_engine.so")
PROFILE = "r33_any_ends.md"
FORMS = ["a", "b", "c", "d", "e"]
NAMES = {"a": "(a) dense call", "b": "(b) `_any`, every stream open", "c": "(c) `_any`, every end at T / 4", "d": "(d) dense call of T / 4 frames",
         "e": "(e) `_any`, lengths uniform in [0, T]"}


NCH = 6                                   # channels of the surround form
PERIOD = 4800                             # ... and the period of its second form: a point every 0.1 s
METERS = ("scope", "surround", "surround_p")
PAIRED = ("scope", "surround")            # the dense calls held against the parent's library
TITLE = {"scope": f"SCOPE W {W} H {H}, stereo", "surround": f"SURROUND, {NCH} channels, no period",
         "surround_p": f"SURROUND, {NCH} channels, P = {PERIOD} ({T // PERIOD} points per stream kept)"}
UNIT = {"scope": "analyses", "surround": "frames", "surround_p": "frames"}


def buffer(M, torch, meter):
    if meter == "scope":
        buf = torch.empty((S, T, 2), dtype=torch.float32, device="cuda")
        M.synth_fill_device(buf.data_ptr(), S, T, T, 777, FS, 1)
    else:
        buf = torch.empty((S, T, NCH), dtype=torch.float32, device="cuda")
        g = torch.Generator(device="cuda").manual_seed(777)
        gains = torch.tensor([0.5, 0.4, 0.3, 0.2, 0.2, 0.1][:NCH], device="cuda")
        for s0 in range(0, S, 256):                                        # (in slabs: no second buffer of that size)
            sl = buf[s0:s0 + 256]
            sl.uniform_(-1.0, 1.0, generator=g)
            sl.mul_(gains)
    torch.cuda.synchronize()
    return buf


def engine(M, meter):
    if meter == "scope":
        e = M.Engine(S, FS, M.METER_SCOPE)
        e.scope_configure(W, H)
    else:
        e = M.Engine(S, FS, M.METER_SURROUND, n_channels=NCH)
        if meter == "surround_p":
            e.surround_set_period(PERIOD, T // PERIOD)
    return e


def work(meter, frames):
    """(units, bytes read).  scope: from a reset engine a stream of f frames runs f // H analyses, each reads min (W, H) new frames of the
    buffer (the rest of a window overlaps the one before where H < W), and its tail reads the W frames in front of its end.  surround:
    the stream's frames, once (the warm-up frames in front of a piece come on top: 112 per 14224)"""
    import numpy as np
    f = np.asarray(frames, np.int64)
    if meter != "scope":
        return int(f.sum()), int(f.sum()) * NCH * 4
    an = f // H
    return int(an.sum()), int((an * min(W, H) + np.minimum(f, W)).sum()) * 8


def turns_of(meter, reps):
    """the five forms of one meter -> (what each must do, device ms per form)"""
    import numpy as np
    import torch
    import meters.lv2_amd as M
    buf = buffer(M, torch, meter)
    st = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(33)
    frames = {"b": np.full(S, T, np.uint64), "c": np.full(S, T // 4, np.uint64), "e": rng.integers(0, T + 1, S).astype(np.uint64)}
    must = {"a": work(meter, np.full(S, T)), "b": work(meter, frames["b"]), "c": work(meter, frames["c"]), "d": work(meter, np.full(S, T // 4)),
            "e": work(meter, frames["e"])}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    dev = {k: [] for k in FORMS}
    e = engine(M, meter)

    def one(key):
        e.reset()
        torch.cuda.synchronize()
        ev[0].record()
        if key == "a":
            e.process_device(buf.data_ptr(), T, T, st)
        elif key == "d":
            e.process_device(buf.data_ptr(), T // 4, T, st)
        else:
            e.process_device_any(buf.data_ptr(), T, frames[key], T, st)
        ev[1].record()
        e.sync()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1])

    for it in range(WARM + reps):
        r = it % len(FORMS)
        for key in FORMS[r:] + FORMS[:r]:                                   # rotating order: nobody always runs behind the same neighbour
            d = one(key)
            if it >= WARM:
                dev[key].append(d)
    one("e")
    if meter == "scope":
        assert int(e.scope_points()[0].sum()) == must["e"][0]
    else:
        assert int(e.stream_frames()[0].sum()) == must["e"][0]
    e.close()
    del buf
    torch.cuda.empty_cache()
    return must, dev


def turns(reps, out):
    import numpy as np
    import torch
    med = lambda v: float(np.median(v))
    f = lambda v: "%.3f" % v
    span = lambda v: "—" if not v else "%.3f – %.3f" % (min(v), max(v))
    res = {"box": f"{torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName})",
           "shape": f"{S} streams x {T // int(FS)} s f32 at {int(FS)} Hz, {reps} turns after {WARM} warm ones, rotating order"}
    md = ["# r33: track lengths for the scope and the surround meter — `_any` against the dense call of the same session\n",
          f"Made by `python tools/any_ends_rate.py {reps}` on {res['box']}: {res['shape']}.\n"]
    for meter in METERS:
        must, dev = turns_of(meter, reps)
        q = {"b_over_a": med(dev["b"]) / med(dev["a"]), "c_over_d": med(dev["c"]) / med(dev["d"]), "e_over_a": med(dev["e"]) / med(dev["a"])}
        res[meter] = {UNIT[meter]: {k: must[k][0] for k in FORMS}, "bytes": {k: must[k][1] for k in FORMS}, "device_ms": dev,
                      "median_ms": {k: med(dev[k]) for k in FORMS}, "ratios": q}
        md += [f"{TITLE[meter]}:\n", f"| form | {UNIT[meter]} | share of the dense call's | MB to read | device ms (median) | min – max |", "|---|---|---|---|---|---|"]
        md += [f"| {NAMES[k]} | {must[k][0]} | {f(must[k][0] / must['a'][0])} | {must[k][1] / 1e6:.1f} | {f(med(dev[k]))} | {span(dev[k])} |" for k in FORMS]
        md += ["", f"(b) / (a) = {f(q['b_over_a'])}; (c) / (d) = {f(q['c_over_d'])}; (e) / (a) = {f(q['e_over_a'])} at {f(must['e'][0] / must['a'][0])} of the {UNIT[meter]}.\n"]
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, PROFILE)
    old = open(path).read() if os.path.exists(path) else ""
    at = old.find("\n## ")                                                 # the tool owns the file down to its first section; what was written
    md.append(old[at + 1:] if at >= 0 else "")                             # by hand behind that stays
    open(path, "w").write("\n".join(md))
    print(json.dumps(res), flush=True)


def dense(meter, reps):
    """the dense call alone, of whichever library MTR_LIB names: one table row"""
    import numpy as np
    import torch
    import meters.lv2_amd as M
    buf = buffer(M, torch, meter)
    st = torch.cuda.current_stream().cuda_stream
    t = []
    with engine(M, meter) as e:
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
    for meter in PAIRED:
        print("\n| library (dense call, %s) | median ms | min | max |\n|---|---|---|---|" % TITLE[meter], flush=True)
        for _ in range(n):
            for lib in (None, LIB_AB):                                      # a fresh child each: nothing of one library's session is left for the other
                env = {k: v for k, v in os.environ.items() if k != "MTR_LIB"}
                if lib:
                    env["MTR_LIB"] = lib
                subprocess.run([sys.executable, os.path.abspath(__file__), "--dense", meter, str(reps)], env=env, check=True, timeout=300)


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
        dense(args[i + 1], int(args[i + 2]) if len(args) > i + 2 else 9)
    else:
        turns(int(args[0]) if args else 9, out)
