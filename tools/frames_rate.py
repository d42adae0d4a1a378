"""tools/frames_rate.py [--out DIR] — what a frame layout (mtr_engine_set_frame_layout) costs.  One process, one GPU, alternating,
>= 5 repeats each.  Prints one JSON object and writes DIR/r13_frames.md + the raw lines under DIR/r13_frames/ (DIR = profiles).
  1. Host path, 1024 streams x 10 s of 6-channel S16, S24 and f32 with the WAVE 5.1 layout on a 5-channel engine, against (a) a plain
     hipMemcpy2DAsync-like copy (torch H2D) of the same source bytes and (b) the default-layout pass of a 5-channel batch of the SAME
     SOURCE BYTES per pass.  Gate: the layout pass's share of the plain copy is no lower than (b)'s by more than (b)'s max - min.
  2. k_pick alone on resident rows (device PCM / f32 entry with a permuted 5-of-6 map, the chunk = the batch): bytes read + written
     over kernel time, beside k_pcm of the same format on the same source bytes and a device-to-device copy of the same traffic.
  3. k_kwmc51 (direct) on 8192 x 10 s of 6-channel f32 against the dense k_kwmc on the compact 5-channel batch, EBU only and EBU + TP,
     and against the staged route (k_pick + dense) on the same input.  Gate: direct <= 6/5 x dense + the spread of the dense repeats.
"""
import argparse
import json
import os
import platform
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import meters.lv2_amd as M  # noqa: E402

FS = 48000.0
WAVE51 = (0, 1, 2, 4, 5)
PERM = (5, 0, 4, 1, 2)
SB = {"f32": 4, "s16": 2, "s24": 3, "s32": 4}
FMT = {"f32": 0, "s16": M.PCM_S16, "s24": M.PCM_S24, "s32": M.PCM_S32}


def host_array(name, S, frames, width, seed):
    """[S, frames * width (* 3)] of the format's samples in pageable memory: small-amplitude noise"""
    rng = np.random.default_rng(seed)
    if name == "f32":
        return (rng.integers(-8000, 8000, (S, frames, width), dtype=np.int16).astype(np.float32) * np.float32(2.0 ** -15))
    if name == "s16":
        return rng.integers(-8000, 8000, (S, frames, width), dtype=np.int16)
    if name == "s32":
        return rng.integers(-8000 << 16, 8000 << 16, (S, frames, width), dtype=np.int32)
    b = rng.integers(0, 256, (S, frames * width, 3), dtype=np.uint8)
    b[:, :, 2] = (b[:, :, 2] % 32).astype(np.uint8) - 16                   # sign-extended top byte: |x| < 2^-3
    return b.reshape(S, -1)


def plain_h2d(torch, arr):
    src = torch.from_numpy(arr.reshape(arr.shape[0], -1))
    dst = torch.empty(src.shape, dtype=src.dtype, device="cuda")
    dst.copy_(src); torch.cuda.synchronize()
    t0 = time.perf_counter()
    dst.copy_(src)
    torch.cuda.synchronize()
    return arr.nbytes / (time.perf_counter() - t0) / 1e9


def one_pass(e, name, arr):
    t0 = time.perf_counter()
    if name == "f32":
        e.process(arr)
    else:
        e.process_pcm(arr, FMT[name])
    e.sync()
    return arr.nbytes / (time.perf_counter() - t0) / 1e9


def host_section(torch, S, T, reps, res, lines):
    rows = {}
    for name in ("s16", "s24", "f32"):
        wide = host_array(name, S, T, 6, 1)
        T5 = T * 6 // 5                                                  # the same source bytes per pass as a 5-channel batch
        comp = host_array(name, S, T5, 5, 2)
        assert wide.nbytes == comp.nbytes
        with M.Engine(S, FS, M.METER_EBU | M.METER_TRUEPEAK, n_channels=5) as ew, M.Engine(S, FS, M.METER_EBU | M.METER_TRUEPEAK, n_channels=5) as ec:
            ew.set_frame_layout(6, WAVE51)
            ew.integr_start(); ec.integr_start()
            one_pass(ew, name, wide); one_pass(ec, name, comp)          # warm
            r = {"layout": [], "default": [], "plain": []}
            for _ in range(reps):
                r["plain"].append(plain_h2d(torch, wide))
                r["layout"].append(one_pass(ew, name, wide))
                r["default"].append(one_pass(ec, name, comp))
            staged = ew.layout_stats()[0]
        plain = float(np.median(r["plain"]))
        share = {k: [g / plain for g in r[k]] for k in ("layout", "default")}
        spread = max(share["default"]) - min(share["default"])
        row = {"bytes": int(wide.nbytes), "GB_per_s": r, "plain_median_GB_per_s": plain, "share_layout_median": float(np.median(share["layout"])),
               "share_default_median": float(np.median(share["default"])), "default_spread": spread, "staged_chunks": staged,
               "link_bound": bool(np.median(share["layout"]) >= np.median(share["default"]) - spread)}
        rows[name] = row
        lines.append(json.dumps({"host": name, **row}))
        print("host", name, json.dumps(row), file=sys.stderr)
        del wide, comp
    res["host"] = rows


def pick_section(torch, S, T, reps, res, lines):
    rows = {}
    for name in ("s16", "s24", "s32", "f32"):
        sb = SB[name]
        src = torch.randint(0, 64, (S, T * 6 * sb), dtype=torch.uint8, device="cuda")
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        r = {"k_pick_call_ms": [], "k_pcm_call_ms": [], "d2d_ms": []}
        st = torch.cuda.current_stream().cuda_stream
        with M.Engine(S, FS, M.METER_EBU, n_channels=5) as ew, M.Engine(S, FS, M.METER_EBU, n_channels=5) as ec:
            ew.set_frame_layout(6, PERM)
            for e in (ew, ec):
                e.set_host_chunk_bytes(S * T * 6 * 4 + (1 << 20))
            T5 = T * 6 // 5

            def wide():
                if name == "f32":
                    ew.process_device(src.data_ptr(), T, T, st)
                else:
                    ew.process_device_pcm(src.data_ptr(), FMT[name], T, stream=st)

            def comp():
                if name == "f32":
                    ec.process_device(src.data_ptr(), T5, T5, st)
                else:
                    ec.process_device_pcm(src.data_ptr(), FMT[name], T5, stream=st)
            traffic = S * T * (6 * sb + 5 * 4)
            a = torch.empty(traffic // 2, dtype=torch.uint8, device="cuda")
            b = torch.empty_like(a)
            wide(); comp(); b.copy_(a); torch.cuda.synchronize()
            # the decode step alone = the whole call minus the meters: the default-layout f32 call on the same batch has no decode
            for _ in range(reps):
                for key, fn in (("k_pick_call_ms", wide), ("k_pcm_call_ms", comp)):
                    ev[0].record(); fn(); ev[1].record(); torch.cuda.synchronize()
                    r[key].append(ev[0].elapsed_time(ev[1]))
                ev[0].record(); b.copy_(a); ev[1].record(); torch.cuda.synchronize()
                r["d2d_ms"].append(ev[0].elapsed_time(ev[1]))
            ew.timing_enable(True); ec.timing_enable(True)
            wide(); comp()
            pick_ms = ew.pcm_stats()[2] if name != "f32" else None
            pcm_ms = ec.pcm_stats()[2] if name != "f32" else None
            tw, tc = ew.timing_calls(), ec.timing_calls()
            if name == "f32":                                            # whole span minus the meters' parts
                pick_ms = float(tw[0, 3] - tw[0, :3].sum())
        row = {"traffic_bytes": traffic, "k_pick_ms": pick_ms, "k_pcm_ms": pcm_ms, "d2d_ms_median": float(np.median(r["d2d_ms"])),
               "k_pick_TB_per_s": traffic / pick_ms / 1e9 if pick_ms else None,
               "k_pcm_TB_per_s": S * T5 * 5 * (sb + 4) / pcm_ms / 1e9 if pcm_ms else None,
               "d2d_TB_per_s": traffic / float(np.median(r["d2d_ms"])) / 1e9, "calls_ms": r}
        rows[name] = row
        lines.append(json.dumps({"pick": name, **row}))
        print("pick", name, json.dumps(row), file=sys.stderr)
        del src, a, b
        torch.cuda.empty_cache()
    res["pick"] = rows


def direct_section(torch, S, T, reps, res, lines):
    wide = torch.empty((S, T, 6), dtype=torch.float32, device="cuda")
    M.synth_fill_device(wide.data_ptr(), S, T * 3, T * 3, 99, FS, 1)
    comp = wide[:, :, list(WAVE51)].contiguous()
    torch.cuda.synchronize()
    st = torch.cuda.current_stream().cuda_stream
    rows = {}
    for label, meters in (("ebu", M.METER_EBU), ("ebu_tp", M.METER_EBU | M.METER_TRUEPEAK)):
        r = {"dense": [], "direct": [], "staged": []}
        with M.Engine(S, FS, meters, n_channels=5) as ed, M.Engine(S, FS, meters, n_channels=5) as ex, M.Engine(S, FS, meters, n_channels=5) as es:
            ex.set_frame_layout(6, WAVE51)
            es.set_frame_layout(6, (0, 1, 2, 5, 4))                      # a map that stages: the same bytes through k_pick + dense k_kwmc
            es.set_host_chunk_bytes(S * T * 5 * 4 + (1 << 20))
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            runs = (("dense", lambda: ed.process_device(comp.data_ptr(), T, T, st)),
                    ("direct", lambda: ex.process_device(wide.data_ptr(), T, T, st)),
                    ("staged", lambda: es.process_device(wide.data_ptr(), T, T, st)))
            for _, fn in runs:
                fn()
            torch.cuda.synchronize()
            for e in (ed, ex, es):
                e.timing_enable(True)
            for _ in range(reps):
                for key, fn in runs:
                    ev[0].record(); fn(); ev[1].record(); torch.cuda.synchronize()
                    r[key].append(ev[0].elapsed_time(ev[1]))
            k = {"dense": ed.timing_calls()[:, 0].tolist(), "direct": ex.timing_calls()[:, 0].tolist(), "staged": es.timing_calls()[:, 0].tolist()}
            assert ex.layout_stats() == (0, reps + 1) and es.layout_stats()[1] == 0
        dense, spread = float(np.median(k["dense"])), max(k["dense"]) - min(k["dense"])
        row = {"kernel_ms": k, "call_ms": r, "dense_kernel_median": dense, "direct_kernel_median": float(np.median(k["direct"])),
               "dense_spread": spread, "bound_ms": 1.2 * dense + spread, "direct_within_bound": bool(np.median(k["direct"]) <= 1.2 * dense + spread),
               "direct_call_median": float(np.median(r["direct"])), "staged_call_median": float(np.median(r["staged"])),
               "dense_call_median": float(np.median(r["dense"])), "direct_beats_staged": bool(np.median(r["direct"]) < np.median(r["staged"]))}
        rows[label] = row
        lines.append(json.dumps({"direct": label, **row}))
        print("direct", label, json.dumps(row), file=sys.stderr)
    res["direct"] = rows


def report(res):
    o = ["# r13: frame layouts — host link rates, k_pick alone, k_kwmc51 against dense k_kwmc and the staged route\n",
         f"Made by `python tools/frames_rate.py` on {res['box']}; raw lines in `r13_frames/`.\n"]
    if "host" in res:
        o.append(f"## Host path: {res['host_shape']}\n")
        o.append("| source | bytes | plain copy GB/s (median) | layout pass: share of the copy (median) | default 5-channel pass of the same bytes | its max − min | layout ≥ default − spread |")
        o.append("|---|---|---|---|---|---|---|")
        for n, r in res["host"].items():
            o.append(f"| {n} | {r['bytes'] / 1e9:.2f} GB | {r['plain_median_GB_per_s']:.1f} | {r['share_layout_median']:.4f} | {r['share_default_median']:.4f} | "
                     f"{r['default_spread']:.4f} | {'yes' if r['link_bound'] else 'NO'} |")
    if "pick" in res:
        o.append(f"\n## k_pick alone: {res['pick_shape']}\n")
        o.append("| format | read + written | k_pick ms | TB/s | k_pcm (5-channel batch of the same bytes) ms | TB/s | D2D copy of the same traffic ms | TB/s |")
        o.append("|---|---|---|---|---|---|---|---|")
        f = lambda v, p="%.2f": "—" if v is None else p % v
        for n, r in res["pick"].items():
            o.append(f"| {n} | {r['traffic_bytes'] / 1e9:.1f} GB | {f(r['k_pick_ms'])} | {f(r['k_pick_TB_per_s'])} | {f(r['k_pcm_ms'])} | {f(r['k_pcm_TB_per_s'])} | "
                     f"{r['d2d_ms_median']:.2f} | {r['d2d_TB_per_s']:.2f} |")
    if "direct" in res:
        o.append(f"\n## k_kwmc51 (reads 5.1 frames itself): {res['direct_shape']}\n")
        o.append("| meters | dense k_kwmc kernel ms (median) | spread | bound 6/5 × dense + spread | k_kwmc51 kernel ms | within | whole call: dense | direct | staged (k_pick + dense) | direct beats staged |")
        o.append("|---|---|---|---|---|---|---|---|---|---|")
        for n, r in res["direct"].items():
            o.append(f"| {n} | {r['dense_kernel_median']:.2f} | {r['dense_spread']:.2f} | {r['bound_ms']:.2f} | {r['direct_kernel_median']:.2f} | "
                     f"{'yes' if r['direct_within_bound'] else 'NO'} | {r['dense_call_median']:.2f} | {r['direct_call_median']:.2f} | {r['staged_call_median']:.2f} | "
                     f"{'yes' if r['direct_beats_staged'] else 'NO'} |")
    return "\n".join(o) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--host-streams", type=int, default=1024)
    ap.add_argument("--device-streams", type=int, default=8192)
    ap.add_argument("--pick-streams", type=int, default=2048)      # (two engines' staging buffers of the whole batch each beside the source)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sections", default="host,pick,direct")
    a = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    T = int(a.seconds * FS)
    res = {"box": f"{platform.node()} ({torch.cuda.get_device_name(0)}, {torch.cuda.get_device_properties(0).gcnArchName})", "library": M.lib.mtr_version().decode(),
           "host_shape": f"{a.host_streams} streams x {a.seconds:.0f} s of 6-channel frames, 48 kHz, pageable numpy memory, WAVE 5.1 on a 5-channel EBU + true peak engine, {a.reps} alternating passes after a warm one",
           "pick_shape": f"{a.pick_streams} streams x {a.seconds:.0f} s of 6-channel frames resident in HBM, permuted 5-of-6 map, one chunk",
           "direct_shape": f"{a.device_streams} streams x {a.seconds:.0f} s of 6-channel f32 resident in HBM, {a.reps} alternating calls"}
    lines = []
    want = a.sections.split(",")
    if "host" in want:
        host_section(torch, a.host_streams, T, a.reps, res, lines)
    if "pick" in want:
        pick_section(torch, a.pick_streams, T, a.reps, res, lines)
        torch.cuda.empty_cache()
    if "direct" in want:
        direct_section(torch, a.device_streams, T, a.reps, res, lines)
    os.makedirs(os.path.join(a.out, "r13_frames"), exist_ok=True)
    open(os.path.join(a.out, "r13_frames", "lines.jsonl"), "w").write("\n".join(lines) + "\n")
    open(os.path.join(a.out, "r13_frames", "result.json"), "w").write(json.dumps(res, indent=1) + "\n")
    open(os.path.join(a.out, "r13_frames.md"), "w").write(report(res))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
