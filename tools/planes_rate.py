"""tools/planes_rate.py [--out DIR] [--sections a,b,c] — what a plane layout (mtr_engine_set_plane_layout, include/mtr_planes.h) costs.  One
process, one GPU, one session; the forms of a section take turns in ROTATING order, each from a reset engine, >= 5 repeats after a warm one.
Prints one JSON object and writes DIR/r40_planes.md + the raw lines under DIR/r40_planes/ (DIR = profiles).
  (a) k_plane alone on resident planes (the device entry with a plane layout, the chunk = the batch): stereo f32 / S16 / S24 / S32 and
      5- and 8-channel f32, bytes read + written over kernel time; next to it k_pick with a map of the same width on the interleaved
      form of the same samples (the same source bytes), and a device-to-device copy of the same traffic.
  (b) the bench step (8192 x 10 s, EBU + true peak, chunk = the decoded batch) from a planar (S, 2, T) device tensor through
      Engine.process_tensor, against transpose (1, 2).contiguous () + the default call, and against the default call alone on the
      interleaved batch.  The last difference is what reading the planes inside the meters' kernels could save at most.
  (c) 1024 x 10 s of planar f32 / S16 in pageable host memory through Engine.process_tensor, against a plain copy of the same bytes and
      against the interleaved host pass of the same samples.

    python tools/planes_rate.py --ebu [reps]          the bench step of ONE library (MTR_LIB names another build of it)
    python tools/planes_rate.py --pairs [pairs [reps]]  ... of the parent's library (tools/build_ab.sh -> meters.lv2_amd/lib_ab) and of this
                                                      build in alternating child processes: the call without a plane layout costs what it cost
    python tools/planes_rate.py --probe [ROWS]        a few k_plane and k_pick calls of rows of (a) and nothing else — ROWS like
                                                      f32:2,s32:2,f32:8, by default f32:2 —: what a counter run of its own wraps
                                                      (rocprofv3 --pmc <one set that fits a pass> -- python tools/planes_rate.py --probe ...)
It never runs by itself in a test."""
import argparse
import json
import os
import platform
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import meters.lv2_amd as M  # noqa: E402

FS = 48000.0
SB = {"f32": 4, "s16": 2, "s24": 3, "s32": 4}
FMT = {"f32": 0, "s16": M.PCM_S16, "s24": M.PCM_S24, "s32": M.PCM_S32}
TORCH_T = {"f32": "float32", "s16": "int16", "s32": "int32"}
WARM = 1


def rotations(forms, reps):
    """the forms `reps` times, each round starting one form later (a warm round in front: its index is < 0)"""
    for it in range(-WARM, reps):
        k = it % len(forms)
        yield it, forms[k:] + forms[:k]


def spread(v):
    v = np.asarray(v, np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "all": [float(x) for x in v]}


# ---- (a) ----------------------------------------------------------------------------------------------------------------------------
def decode_ms(e, name, before):
    """the time of the call's first step (k_plane / k_pick) alone: the decode timer for integer samples, the call's span less the meters'
    parts for f32 (tools/frames_rate.py)"""
    if name != "f32":
        return e.pcm_stats()[2] - before
    tw = e.timing_calls()
    return float(tw[-1, 3] - tw[-1, :3].sum())


def a_row(torch, name, C, S, T, reps, probe=False):
    sb = SB[name]
    meters, kw = (M.METER_SURROUND, dict(n_channels=C)) if C > 5 else (M.METER_EBU, dict(n_channels=C))
    perm = (1, 0) + tuple(range(2, C))                                   # the same width, not the identity: k_pick runs
    src = torch.randint(0, 64, (S * C * T * sb,), dtype=torch.uint8, device="cuda")   # small samples in every format, planar or interleaved
    st = torch.cuda.current_stream().cuda_stream
    traffic = S * T * C * (sb + 4)
    a = torch.empty(traffic // 2, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    t = {"k_plane": [], "k_pick": [], "d2d": []}
    with M.Engine(S, FS, meters, **kw) as ep, M.Engine(S, FS, meters, **kw) as ek:
        ep.set_plane_layout(C, perm)
        ek.set_frame_layout(C, perm)
        for e in (ep, ek):
            e.set_host_chunk_bytes(S * T * C * 4 + (1 << 20))
            e.timing_enable(not probe)

        def call(e):
            e.reset()
            before = 0.0 if name == "f32" or probe else e.pcm_stats()[2]
            e.process_raw(src.data_ptr(), T, T, FMT[name], stream=st)
            e.sync()
            return None if probe else decode_ms(e, name, before)

        def d2d(_):
            ev[0].record(); b.copy_(a); ev[1].record(); torch.cuda.synchronize()
            return ev[0].elapsed_time(ev[1])
        forms = [("k_plane", call, ep), ("k_pick", call, ek)] + ([] if probe else [("d2d", d2d, None)])
        for it, order in rotations(forms, reps):
            for key, fn, e in order:
                ms = fn(e)
                if it >= 0 and ms is not None:
                    t[key].append(ms)
        assert ep.plane_stats() == WARM + reps and ek.layout_stats()[0] == WARM + reps
    del src, a, b
    torch.cuda.empty_cache()
    if probe:
        return None
    row = {"format": name, "channels": C, "traffic_bytes": traffic, "ms": {k: spread(v) for k, v in t.items()}}
    row["TB_per_s"] = {k: traffic / row["ms"][k]["median"] / 1e9 for k in t}
    row["TB_per_s_range"] = {k: [traffic / row["ms"][k]["max"] / 1e9, traffic / row["ms"][k]["min"] / 1e9] for k in t}
    row["k_plane_inside_k_pick_range"] = bool(row["ms"]["k_plane"]["median"] <= row["ms"]["k_pick"]["max"])
    return row


def section_a(torch, S, T, reps, res, lines):
    rows = []
    for name, C in (("f32", 2), ("s16", 2), ("s24", 2), ("s32", 2), ("f32", 5), ("f32", 8)):
        row = a_row(torch, name, C, S, T, reps)
        rows.append(row)
        lines.append(json.dumps({"a": row}))
        print("a", json.dumps(row), file=sys.stderr)
    res["a"] = rows


# ---- (b) ----------------------------------------------------------------------------------------------------------------------------
def section_b(torch, S, T, reps, res, lines):
    il = torch.empty((S, T, 2), dtype=torch.float32, device="cuda")
    M.synth_fill_device(il.data_ptr(), S, T, T, 777, FS, 1)
    planar = il.transpose(1, 2).contiguous()                             # (S, 2, T): what a PyTorch batch is
    torch.cuda.synchronize()
    st = torch.cuda.current_stream().cuda_stream
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    t = {"planar": [], "transpose_default": [], "default": []}
    with M.Engine(S, FS, M.METER_EBU | M.METER_TRUEPEAK) as ep, M.Engine(S, FS, M.METER_EBU | M.METER_TRUEPEAK) as ed:
        ep.set_host_chunk_bytes(S * T * 2 * 4 + (1 << 20))

        def run_planar():
            ep.reset(); ep.integr_start()
            ev[0].record(); ep.process_tensor(planar); ep.sync(); ev[1].record()

        def run_transpose():
            ed.reset(); ed.integr_start()
            ev[0].record()
            x = planar.transpose(1, 2).contiguous()
            ed.process_device(x.data_ptr(), T, T, st); ed.sync()
            ev[1].record()
            torch.cuda.synchronize()
            del x

        def run_default():
            ed.reset(); ed.integr_start()
            ev[0].record(); ed.process_device(il.data_ptr(), T, T, st); ed.sync(); ev[1].record()
        forms = [("planar", run_planar), ("transpose_default", run_transpose), ("default", run_default)]
        for it, order in rotations(forms, reps):
            for key, fn in order:
                fn()
                torch.cuda.synchronize()
                if it >= 0:
                    t[key].append(ev[0].elapsed_time(ev[1]))
        same = ep.state_export() == ed.state_export()                    # (both engines' last call took the same samples)
        chunks = ep.plane_stats()
    row = {"ms": {k: spread(v) for k, v in t.items()}, "plane_chunks": chunks, "same_state_blob": bool(same)}
    m = {k: row["ms"][k]["median"] for k in t}
    row["planar_over_default_ms"] = m["planar"] - m["default"]
    row["transpose_over_planar_ms"] = m["transpose_default"] - m["planar"]
    res["b"] = row
    lines.append(json.dumps({"b": row}))
    print("b", json.dumps(row), file=sys.stderr)
    del il, planar
    torch.cuda.empty_cache()


# ---- (c) ----------------------------------------------------------------------------------------------------------------------------
def section_c(torch, S, T, reps, res, lines):
    rows = {}
    rng = np.random.default_rng(3)
    for name in ("f32", "s16"):
        block = rng.integers(-8000, 8000, (32, 2, T), dtype=np.int16)
        block = block.astype(np.float32) * np.float32(2.0 ** -15) if name == "f32" else block
        planar = np.tile(block, (S // 32, 1, 1))                         # (S, 2, T) in pageable memory
        il = np.ascontiguousarray(planar.transpose(0, 2, 1))             # (S, T, 2): the same samples interleaved
        src = torch.from_numpy(planar.reshape(S, -1))
        dst = torch.empty(src.shape, dtype=src.dtype, device="cuda")
        t = {"plain_copy": [], "planar": [], "interleaved": []}
        with M.Engine(S, FS, M.METER_EBU | M.METER_TRUEPEAK) as ep, M.Engine(S, FS, M.METER_EBU | M.METER_TRUEPEAK) as ei:
            def plain():
                t0 = time.perf_counter(); dst.copy_(src); torch.cuda.synchronize()
                return time.perf_counter() - t0

            def run_planar():
                ep.reset(); ep.integr_start()
                t0 = time.perf_counter(); ep.process_tensor(planar); ep.sync()
                return time.perf_counter() - t0

            def run_il():
                ei.reset(); ei.integr_start()
                t0 = time.perf_counter()
                ei.process(il) if name == "f32" else ei.process_pcm(il)
                ei.sync()
                return time.perf_counter() - t0
            forms = [("plain_copy", plain), ("planar", run_planar), ("interleaved", run_il)]
            for it, order in rotations(forms, reps):
                for key, fn in order:
                    s = fn()
                    if it >= 0:
                        t[key].append(planar.nbytes / s / 1e9)
            same = ep.state_export() == ei.state_export()
            chunks = ep.plane_stats() // (WARM + reps)
        row = {"bytes": int(planar.nbytes), "GB_per_s": {k: spread(v) for k, v in t.items()}, "chunks_per_pass": chunks, "same_state_blob": bool(same)}
        plain_med = row["GB_per_s"]["plain_copy"]["median"]
        row["share_of_plain_copy"] = {k: row["GB_per_s"][k]["median"] / plain_med for k in ("planar", "interleaved")}
        rows[name] = row
        lines.append(json.dumps({"c": name, **row}))
        print("c", name, json.dumps(row), file=sys.stderr)
        del planar, il, src, dst
        torch.cuda.empty_cache()
    res["c"] = rows


def report(res):
    o = ["# r40: plane layouts — k_plane alone, the bench step from a planar tensor, planar host audio\n",
         f"Made by `python tools/planes_rate.py` on {res['box']}; raw lines in `r40_planes/`.  Forms in rotating order, each from a reset engine, "
         f"{res['reps']} repeats after a warm one.\n"]
    f = lambda r: f"{r['median']:.3f} ({r['min']:.3f} – {r['max']:.3f})"
    if "a" in res:
        o.append(f"## (a) k_plane alone: {res['a_shape']}\n")
        o.append("| samples | read + written | k_plane ms: median (min – max) | TB/s | k_pick, same width, interleaved form ms | TB/s | D2D copy of the same traffic ms | TB/s | k_plane's median inside k_pick's min – max |")
        o.append("|---|---|---|---|---|---|---|---|---|")
        for r in res["a"]:
            o.append(f"| {r['channels']} x {r['format']} | {r['traffic_bytes'] / 1e9:.1f} GB | {f(r['ms']['k_plane'])} | {r['TB_per_s']['k_plane']:.2f} | {f(r['ms']['k_pick'])} | "
                     f"{r['TB_per_s']['k_pick']:.2f} | {f(r['ms']['d2d'])} | {r['TB_per_s']['d2d']:.2f} | {'yes' if r['k_plane_inside_k_pick_range'] else 'NO: below'} |")
    if "b" in res:
        r = res["b"]
        o.append(f"\n## (b) the bench step: {res['b_shape']}\n")
        o.append("| form | ms: median (min – max) |")
        o.append("|---|---|")
        o.append(f"| planar (S, 2, T) tensor, `process_tensor`: k_plane + the meters | {f(r['ms']['planar'])} |")
        o.append(f"| `transpose (1, 2).contiguous ()` + the default call | {f(r['ms']['transpose_default'])} |")
        o.append(f"| the default call alone on the interleaved batch | {f(r['ms']['default'])} |")
        o.append(f"\nplanar − default = {r['planar_over_default_ms']:.3f} ms: what a route that reads the planes inside the meters' kernels could save at most.  "
                 f"transpose − planar = {r['transpose_over_planar_ms']:.3f} ms, and the transposed copy's second buffer of the batch's size is not allocated.  "
                 f"State blobs of the planar and the default engine byte-equal: {'yes' if r['same_state_blob'] else 'NO'}.")
    if "c" in res:
        o.append(f"\n## (c) planar host audio: {res['c_shape']}\n")
        o.append("| samples | bytes | plain copy GB/s: median (min – max) | planar pass | share of the copy | interleaved pass of the same samples | share | chunks per pass |")
        o.append("|---|---|---|---|---|---|---|---|")
        g = lambda r: f"{r['median']:.1f} ({r['min']:.1f} – {r['max']:.1f})"
        for n, r in res["c"].items():
            o.append(f"| {n} | {r['bytes'] / 1e9:.2f} GB | {g(r['GB_per_s']['plain_copy'])} | {g(r['GB_per_s']['planar'])} | {r['share_of_plain_copy']['planar']:.3f} | "
                     f"{g(r['GB_per_s']['interleaved'])} | {r['share_of_plain_copy']['interleaved']:.3f} | {r['chunks_per_pass']} |")
    return "\n".join(o) + "\n"


# ---- the bench step of one library, and pairs of child processes -----------------------------------------------------------------------
def bench_step(reps):
    import torch
    S, T = 8192, 480000
    buf = torch.empty((S, T, 2), dtype=torch.float32, device="cuda")
    M.synth_fill_device(buf.data_ptr(), S, T, T, 777, FS, 1)
    torch.cuda.synchronize()
    st = torch.cuda.current_stream().cuda_stream
    t = []
    with M.Engine(S, FS, M.METER_EBU | M.METER_TRUEPEAK) as e:
        e.integr_start()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for it in range(2 + reps):
            ev0.record()
            e.process_device(buf.data_ptr(), T, T, st)
            e.sync()                                                       # (the deferred tail included)
            ev1.record()
            torch.cuda.synchronize()
            if it >= 2:
                t.append(ev0.elapsed_time(ev1))
    v = np.asarray(t)
    print("EBU | TRUEPEAK step, %s: median %.3f ms  min %.3f  max %.3f" % (os.environ.get("MTR_LIB") or "this build", np.median(v), v.min(), v.max()), flush=True)


def pairs(n_pairs, reps):
    lib_ab = os.path.join(ROOT, "meters.lv2_amd", "lib_ab", "libmtr_engine.so")
    if not os.path.exists(lib_ab):
        sys.exit(lib_ab + " is missing: tools/build_ab.sh <parent revision> builds it")
    for p in range(n_pairs):
        for lib in (lib_ab, None):
            env = dict(os.environ)
            env.pop("MTR_LIB", None)
            if lib:
                env["MTR_LIB"] = lib
            print("pair %d, %s" % (p, "parent (lib_ab)" if lib else "this build"), flush=True)
            subprocess.run([sys.executable, os.path.abspath(__file__), "--ebu", str(reps)], env=env, check=True, timeout=300)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--kernel-streams", type=int, default=2048)    # (two engines' staging buffers of the whole batch each beside the source)
    ap.add_argument("--device-streams", type=int, default=8192)
    ap.add_argument("--host-streams", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sections", default="a,b,c")
    ap.add_argument("--ebu", action="store_true")
    ap.add_argument("--pairs", action="store_true")
    ap.add_argument("--probe", nargs="?", const="f32:2", default=None)
    ap.add_argument("nums", nargs="*", type=int)
    a = ap.parse_args()
    if a.pairs:
        return pairs(a.nums[0] if a.nums else 3, a.nums[1] if len(a.nums) > 1 else 7)
    if a.ebu:
        return bench_step(a.nums[0] if a.nums else 9)
    import torch
    torch.cuda.set_device(0)
    T = int(a.seconds * FS)
    if a.probe:
        for row in a.probe.split(","):
            name, C = row.split(":")
            a_row(torch, name, int(C), a.kernel_streams, T, 3, probe=True)
        return
    res = {"box": f"{platform.node()} ({torch.cuda.get_device_name(0)}, {torch.cuda.get_device_properties(0).gcnArchName})", "library": M.lib.mtr_version().decode(),
           "reps": a.reps,
           "a_shape": f"{a.kernel_streams} streams x {a.seconds:.0f} s resident in HBM, the map (1, 0, 2, ...) of the samples' own width, one chunk",
           "b_shape": f"{a.device_streams} streams x {a.seconds:.0f} s of stereo f32 resident in HBM, EBU + true peak, integration on, one chunk; whole calls by events, the deferred tail included",
           "c_shape": f"{a.host_streams} streams x {a.seconds:.0f} s of stereo planes in pageable numpy memory, EBU + true peak, the default chunk size"}
    lines = []
    want = a.sections.split(",")
    if "a" in want:
        section_a(torch, a.kernel_streams, T, a.reps, res, lines)
    if "b" in want:
        section_b(torch, a.device_streams, T, a.reps, res, lines)
    if "c" in want:
        section_c(torch, a.host_streams, T, a.reps, res, lines)
    os.makedirs(os.path.join(a.out, "r40_planes"), exist_ok=True)
    open(os.path.join(a.out, "r40_planes", "lines.jsonl"), "w").write("\n".join(lines) + "\n")
    open(os.path.join(a.out, "r40_planes", "result.json"), "w").write(json.dumps(res, indent=1) + "\n")
    open(os.path.join(a.out, "r40_planes.md"), "w").write(report(res))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
