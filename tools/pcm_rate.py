"""tools/pcm_rate.py [--out DIR] [--parent-lib PATH] — what integer PCM in (mtr_engine_process_host_pcm / _device_pcm) buys.

One process, one GPU.  Prints one JSON object and writes DIR/r12_pcm.md + the raw lines under DIR/r12_pcm/ (DIR = profiles).
  1. the shape of bench.py's end_to_end_host (1024 streams x 10 s stereo, 48 kHz, pageable numpy memory, EBU + true peak, one
     warm pass, three timed passes) for float, s16, s24 and s32 in the same run, each next to a plain torch H2D copy of THE SAME
     BYTES FROM THE SAME MEMORY: GB/s over the link, frac_of_link, frames/s, chunks, decode ms, kernel ms;
  2. the float path of the PARENT commit's library (tools/build_ab.sh <rev> builds it into meters.lv2_amd/lib_ab) in the same
     process, interleaved with the head's, three runs each;
  3. the decode kernel alone on device-resident PCM at 8192 streams x 10 s stereo: ms and bytes read + written per second, next to
     a device-to-device copy of the same total traffic in the same run and to the meters' kernel time for that batch.
"""
import argparse
import importlib.util
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
BITS = {"s16": 16, "s24": 24, "s32": 32}
FMT = {"s16": M.PCM_S16, "s24": M.PCM_S24, "s32": M.PCM_S32}


def parent_binding(path):
    """the head's binding over another build of the library (MTR_LIB is read when the module is executed)"""
    old = os.environ.get("MTR_LIB")
    os.environ["MTR_LIB"] = path
    try:
        spec = importlib.util.spec_from_file_location("mtr_parent_binding", os.path.join(ROOT, "meters.lv2_amd", "engine.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        if old is None:
            del os.environ["MTR_LIB"]
        else:
            os.environ["MTR_LIB"] = old
    return mod


def quantise(x, name, slab=32):
    """float [S, T, 2] to the format's integers (scale, round, clip), slab by slab; s24 packed as uint8 [S, T * 6]"""
    k = BITS[name] - 1
    S = x.shape[0]
    out = np.empty((S, x.shape[1] * 6), np.uint8) if name == "s24" else np.empty(x.shape, np.int16 if name == "s16" else np.int32)
    for a in range(0, S, slab):
        v = np.rint(x[a:a + slab].astype(np.float64) * 2.0 ** k).clip(-2.0 ** k, 2.0 ** k - 1)
        if name == "s24":
            b = v.astype("<i4").view(np.uint8).reshape(v.shape[0], -1, 4)[:, :, :3]
            out[a:a + slab] = b.reshape(v.shape[0], -1)
        else:
            out[a:a + slab] = v.astype(out.dtype)
    return out


def plain_h2d(torch, arr, reps=3):
    src = torch.from_numpy(arr)
    dst = torch.empty(src.shape, dtype=src.dtype, device="cuda")
    dst.copy_(src); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        dst.copy_(src)
    torch.cuda.synchronize()
    return arr.nbytes * reps / (time.perf_counter() - t0)


def host_passes(mod, arr, name, S, T, reps=3):
    """one warm pass, `reps` timed passes one by one, one pass with timing on"""
    with mod.Engine(S, FS, mod.METER_EBU | mod.METER_TRUEPEAK) as e:
        e.integr_start()
        run = (lambda: e.process(arr)) if name == "f32" else (lambda: e.process_pcm(arr, FMT[name]))
        run(); e.sync()
        dts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            run(); e.sync()
            dts.append(time.perf_counter() - t0)
        e.timing_enable(True)
        c0 = e.pcm_stats()[0] if name != "f32" else 0
        run()
        q = e.timing_query()
        st = e.pcm_stats() if name != "f32" else (0, 0, 0.0)
        out9 = e.out9()
    gbs = [arr.nbytes / dt / 1e9 for dt in dts]
    return {"GB_per_s": arr.nbytes * reps / sum(dts) / 1e9, "GB_per_s_passes": gbs, "frames_per_s": S * T * reps / sum(dts),
            "wall_ms": 1e3 * sum(dts) / reps, "bytes": int(arr.nbytes), "chunks": q["calls"], "pcm_chunks": st[0] - c0,
            "decode_ms": st[2], "kernel_ms": q["ms_fused"] + q["ms_gate"]}, out9


def host_section(torch, buf, S, parent, res, lines):
    T = buf.shape[1]
    x = buf[:S].cpu().numpy()
    rows, ref9 = {}, None
    for name in ("f32", "s16", "s24", "s32"):
        arr = x if name == "f32" else quantise(x, name)
        link = plain_h2d(torch, arr)
        r, out9 = host_passes(M, arr, name, S, T)
        r["plain_h2d_GB_per_s"] = link / 1e9
        r["frac_of_link"] = r["GB_per_s"] / r["plain_h2d_GB_per_s"]
        r["frac_of_link_passes"] = [g / r["plain_h2d_GB_per_s"] for g in r["GB_per_s_passes"]]
        if name == "f32":
            ref9 = out9
        else:
            r["max_abs_dLUFS_vs_f32"] = float(np.abs(out9[:, :4] - ref9[:, :4]).max())   # (the quantised signal is another signal: a sanity figure)
        rows[name] = r
        lines.append(json.dumps({"host": name, **r}))
        print("host", name, json.dumps(r), file=sys.stderr)
        if name != "f32":
            del arr
    f = rows["f32"]
    margin = max(f["frac_of_link_passes"]) - min(f["frac_of_link_passes"])
    for name in ("s16", "s24", "s32"):
        rows[name]["frames_ratio_to_f32"] = rows[name]["frames_per_s"] / f["frames_per_s"]
        rows[name]["link_bound"] = bool(rows[name]["frac_of_link"] >= f["frac_of_link"] - margin)
    res["host"] = rows
    res["host_margin_frac"] = margin
    # the refactored float loop against the loop it replaces: the parent's library, interleaved, three runs each
    if parent is not None:
        ab = {"head": [], "parent": []}
        for _ in range(3):
            for who, mod in (("head", M), ("parent", parent)):
                r, _ = host_passes(mod, x, "f32", S, T)
                ab[who].append(r["GB_per_s"])
                lines.append(json.dumps({"float_ab": who, **r}))
        spread = max(ab["parent"]) - min(ab["parent"])
        res["float_ab"] = {"head_GB_per_s": ab["head"], "parent_GB_per_s": ab["parent"], "parent_spread": spread,
                           "head_mean": float(np.mean(ab["head"])), "parent_mean": float(np.mean(ab["parent"])),
                           "head_not_slower": bool(np.mean(ab["head"]) >= np.mean(ab["parent"]) - spread)}


def device_section(torch, buf, res, lines):
    S, T = buf.shape[0], buf.shape[1]
    n = S * T * 2
    with M.Engine(S, FS, M.METER_EBU | M.METER_TRUEPEAK) as e:     # the meters on the resident floats: what the device form's decode comes on top of
        e.integr_start()
        e.process_device(buf.data_ptr(), T); e.sync()
        e.timing_enable(True)
        e.process_device(buf.data_ptr(), T)
        q = e.timing_query()
    meters_ms = q["ms_fused"] + q["ms_gate"]
    rows = {}
    for name in ("s16", "s24", "s32"):
        k, sb = BITS[name] - 1, BITS[name] // 8
        pcm = torch.empty((S, T * 2 * sb), dtype=torch.uint8, device="cuda")
        for a in range(0, S, 256):
            v = (buf[a:a + 256].double() * 2.0 ** k).round().clamp(-2.0 ** k, 2.0 ** k - 1)
            if name == "s16":
                pcm[a:a + 256] = v.to(torch.int16).view(torch.uint8).reshape(v.shape[0], -1)
            else:
                b = v.to(torch.int32).view(torch.uint8).reshape(v.shape[0], -1, 4)
                pcm[a:a + 256] = (b[:, :, :3] if name == "s24" else b).reshape(v.shape[0], -1)
            del v
        traffic = n * (sb + 4)
        runs = {}
        for chunk in ("default", "batch"):                          # chunks of 256 MiB of decoded floats; the whole batch as one chunk
            with M.Engine(S, FS, M.METER_EBU | M.METER_TRUEPEAK) as e:
                e.integr_start()
                if chunk == "batch":
                    e.set_host_chunk_bytes(n * 4 + (1 << 20))
                e.process_device_pcm(pcm.data_ptr(), FMT[name], T); e.sync()
                e.timing_enable(True)
                e.process_device_pcm(pcm.data_ptr(), FMT[name], T)
                q = e.timing_query()
                chunks, _, ms = e.pcm_stats()
                runs[chunk] = (ms, chunks // 2, q["ms_fused"] + q["ms_gate"])
        dec_ms, chunks = runs["default"][0], runs["default"][1]
        del pcm
        # a device-to-device copy that moves the same bytes (read + written)
        src = torch.empty(traffic // 2, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        dst.copy_(src); torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(3):
            dst.copy_(src)
        ev[1].record(); torch.cuda.synchronize()
        d2d_ms = ev[0].elapsed_time(ev[1]) / 3
        del src, dst
        rows[name] = {"decode_ms": dec_ms, "decode_chunks": chunks, "decode_ms_one_chunk": runs["batch"][0],
                      "meters_kernel_ms_on_pcm_one_chunk": runs["batch"][2], "traffic_bytes": traffic, "decode_TB_per_s": traffic / dec_ms / 1e9,
                      "d2d_copy_ms": d2d_ms, "d2d_TB_per_s": traffic / d2d_ms / 1e9, "frac_of_d2d": d2d_ms / dec_ms,
                      "meters_kernel_ms_on_pcm": runs["default"][2], "meters_kernel_ms_on_resident_f32": meters_ms,
                      "decode_over_meters": dec_ms / meters_ms}
        lines.append(json.dumps({"device": name, **rows[name]}))
        print("device", name, json.dumps(rows[name]), file=sys.stderr)
    res["device"] = rows


def report(res):
    h, o = res["host"], []
    o.append("# r12: integer PCM in — host link rates, the float loop against its parent, the decode kernel alone\n")
    o.append(f"Made by `python tools/pcm_rate.py` on {res['box']}; raw lines in `r12_pcm/`.\n")
    o.append(f"## Host path: {res['host_shape']}\n")
    o.append("| source | bytes | GB/s (3 passes) | passes | plain H2D of the same bytes | frac_of_link | frames/s | : f32 | chunks | decode ms | kernel ms |")
    o.append("|---|---|---|---|---|---|---|---|---|---|---|")
    for name, r in h.items():
        o.append(f"| {name} | {r['bytes'] / 1e9:.2f} GB | {r['GB_per_s']:.1f} | {', '.join('%.1f' % g for g in r['GB_per_s_passes'])} | "
                 f"{r['plain_h2d_GB_per_s']:.1f} | {r['frac_of_link']:.3f} | {r['frames_per_s'] / 1e9:.2f} G | "
                 f"{r.get('frames_ratio_to_f32', 1.0):.2f} | {r['chunks']} | {r['decode_ms']:.2f} | {r['kernel_ms']:.1f} |")
    o.append(f"\nMargin = the spread of the float path's three passes = {res['host_margin_frac']:.4f} of the link; link-bound by that yardstick: "
             + ", ".join(f"{n} {'yes' if h[n]['link_bound'] else 'NO'}" for n in ("s16", "s24", "s32")) + ".\n")
    if "float_ab" in res:
        a = res["float_ab"]
        o.append("## The float host path, head against the parent commit's library (same process, interleaved)\n")
        o.append("| | run 1 | run 2 | run 3 | mean GB/s |\n|---|---|---|---|---|")
        o.append("| head | " + " | ".join("%.2f" % g for g in a["head_GB_per_s"]) + f" | {a['head_mean']:.2f} |")
        o.append("| parent | " + " | ".join("%.2f" % g for g in a["parent_GB_per_s"]) + f" | {a['parent_mean']:.2f} |")
        o.append(f"\nSpread of the parent's three runs: {a['parent_spread']:.2f} GB/s; head not slower by more than that: {'yes' if a['head_not_slower'] else 'NO'}.\n")
    if "device" in res:
        o.append(f"## The decode kernel alone: {res['device_shape']}\n")
        o.append("| format | k_pcm ms (sum over the chunks) | as one chunk | read + written | TB/s | D2D copy of the same traffic, ms | TB/s | copy : k_pcm | meters' kernels on resident f32, ms | decode : meters |")
        o.append("|---|---|---|---|---|---|---|---|---|---|")
        for name, r in res["device"].items():
            o.append(f"| {name} | {r['decode_ms']:.2f} ({r['decode_chunks']} chunks) | {r['decode_ms_one_chunk']:.2f} | {r['traffic_bytes'] / 1e9:.1f} GB | {r['decode_TB_per_s']:.2f} | {r['d2d_copy_ms']:.2f} | "
                     f"{r['d2d_TB_per_s']:.2f} | {r['frac_of_d2d']:.2f} | {r['meters_kernel_ms_on_resident_f32']:.2f} | {r['decode_over_meters']:.2f} |")
        d = res["device"]
        o.append("\nThe meters' kernels of the device form itself: " + ", ".join(f"{n} {d[n]['meters_kernel_ms_on_pcm']:.1f} ms in {d[n]['decode_chunks']} chunks, "
                 f"{d[n]['meters_kernel_ms_on_pcm_one_chunk']:.2f} ms as one chunk" for n in d) + ". The kernels are planned for the whole batch (lane = time segment: a chunk "
                 "of few streams takes about as long as all of them), which the host forms hide under the link; a caller with device-resident PCM and HBM to spare sets "
                 "mtr_engine_set_host_chunk_bytes to the decoded batch.")
        o.append("\nThe last column is what mtr_engine_process_device_pcm costs on top of the meters, and what reading the integers inside the "
                 "metering kernels would save for device-resident PCM.\n")
    return "\n".join(o) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--parent-lib", default=os.path.join(ROOT, "meters.lv2_amd", "lib_ab", "libmtr_engine.so"))
    ap.add_argument("--host-streams", type=int, default=1024)
    ap.add_argument("--device-streams", type=int, default=8192)
    ap.add_argument("--seconds", type=float, default=10.0)
    a = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    T = int(a.seconds * FS)
    S = max(a.host_streams, a.device_streams)
    buf = torch.empty((S, T, 2), dtype=torch.float32, device="cuda")
    M.synth_fill_device(buf.data_ptr(), S, T, T, 12, FS, 1)
    torch.cuda.synchronize()
    res = {"box": f"{platform.node()} ({torch.cuda.get_device_name(0)}, {torch.cuda.get_device_properties(0).gcnArchName})", "library": M.lib.mtr_version().decode(),
           "host_shape": f"{a.host_streams} streams x {a.seconds:.0f} s stereo, 48 kHz, pageable numpy memory, EBU + true peak, 3 timed passes after a warm one",
           "device_shape": f"{a.device_streams} streams x {a.seconds:.0f} s stereo, PCM resident in HBM"}
    lines = []
    parent = parent_binding(a.parent_lib) if os.path.exists(a.parent_lib) else None
    if parent is None:
        print(f"no parent library at {a.parent_lib}: the float A/B is left out (tools/build_ab.sh HEAD~1)", file=sys.stderr)
    host_section(torch, buf, a.host_streams, parent, res, lines)
    if a.device_streams:
        device_section(torch, buf[:a.device_streams], res, lines)
    os.makedirs(os.path.join(a.out, "r12_pcm"), exist_ok=True)
    open(os.path.join(a.out, "r12_pcm", "lines.jsonl"), "w").write("\n".join(lines) + "\n")
    open(os.path.join(a.out, "r12_pcm", "result.json"), "w").write(json.dumps(res, indent=1) + "\n")
    open(os.path.join(a.out, "r12_pcm.md"), "w").write(report(res))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
