"""tools/gonio_rate.py — what the goniometer (MTR_METER_GONIO, mtr_gonio.hip) costs, next to the two kernels that read the same bytes:
k_needle (mtr_needle.hip, the other serial chain per stream) and Kmeterdsp (mtr_kmeter.hip, the HBM time of these bytes).  GPU box only.

One session, one buffer (8192 streams x 10 s of stereo at 48 kHz, the bench programme: mtr_synth_fill_device kind 1), engines that take
turns on it in rotating order, each call from a reset engine, after two warm-up rounds:
    GONIO, auto gain off, shift 2 · GONIO, auto gain on, shift 2 · GONIO, auto gain on, shift 1 · NEEDLE, all four kinds · KMETER
Times are the engine's own device events around each call (mtr_engine_timing_calls, column "whole call"); for the goniometer also
k_gonio_points and k_gonio_image apart, summed over the call's pieces (mtr_engine_gonio_timing: events around each launch).  Printed:
median, min and max per form, the ratio to the K-meter's median, and the bytes a form reads and writes.
    python tools/gonio_rate.py [reps] [tune_piece]

    python tools/gonio_rate.py --ends [reps] [tune_piece]
what track lengths (mtr_engine_process_device_gonio_ends: the ENDS instantiations of the two kernels) cost and save, auto gain on, shift 2:
five forms on the same buffer in rotating order, each from a reset engine, device events around the call — (a) the dense call; (b) the new
call with every stream open; (c) every end at a quarter of the call, next to (d) the dense call of that quarter; (e) lengths uniform in
[0, 10 s] — with the chunks of 128 frames each form must walk (16 lanes share a wave's loop: a workgroup walks up to its last cut).

    python tools/gonio_rate.py --oversample [F] [reps] [tune_piece]
what the oversampling (mtr_engine_gonio_set_oversample: k_gonio_os in front of the two kernels, which then walk F points per frame) costs,
auto gain on, shift 2: the call at factor 1, 2 and F (4) on the same buffer in rotating order, each from a reset engine — device events
around the call, and around every launch for the three kernels apart (mtr_engine_gonio_timing, mtr_engine_gonio_os_timing) — with the
bytes each kernel moves and the rate that implies.

    python tools/gonio_rate.py --pairs [N] [reps] [tune_piece]
the dense call of this build against the parent's library (tools/build_ab.sh -> meters.lv2_amd/lib_ab): N pairs of child processes
alternating on the same box (--dense, with MTR_LIB naming the library), a table row per child.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import meters.lv2_amd as M  # noqa: E402

FS, S, T = 48000.0, 8192, 480000
WARM = 2


def buffer():
    buf = torch.empty((S, T, 2), dtype=torch.float32, device="cuda")
    M.synth_fill_device(buf.data_ptr(), S, T, T, 777, FS, 1)
    torch.cuda.synchronize()
    return buf


def line(name, v, base=None):
    v = np.asarray(v, np.float64)
    med = float(np.median(v))
    out = "%-34s median %8.3f ms  min %8.3f  max %8.3f" % (name, med, v.min(), v.max())
    if base:
        out += "  x %.3f of KMETER" % (med / base)
    print(out, flush=True)
    return med


def main(reps, piece):
    buf = buffer()
    st = torch.cuda.current_stream().cuda_stream
    every = M.NEEDLE_VU | M.NEEDLE_IEC1 | M.NEEDLE_IEC2 | M.NEEDLE_MS
    forms = [("GONIO gain fixed, shift 2", M.METER_GONIO, dict(shift=2, autogain=0)),
             ("GONIO auto gain, shift 2", M.METER_GONIO, dict(shift=2, autogain=1)),
             ("GONIO auto gain, shift 1", M.METER_GONIO, dict(shift=1, autogain=1)),
             ("NEEDLE all four kinds", M.METER_NEEDLE, None), ("KMETER", M.METER_KMETER, None)]
    engines = []
    for name, meters, cfg in forms:
        e = M.Engine(S, FS, meters)
        if cfg:
            e.gonio_configure(tune_piece=piece, **cfg)
            e.gonio_timing(True)
        elif meters == M.METER_NEEDLE:
            e.needle_configure(every, 0, 0)
        e.timing_enable(True)
        engines.append((name, e, cfg))
    t = {name: [] for name, _, _ in engines}
    tp = {name: [] for name, _, cfg in engines if cfg}
    ti = {name: [] for name, _, cfg in engines if cfg}
    for it in range(WARM + reps):
        order = engines[it % len(engines):] + engines[:it % len(engines)]     # rotating
        for name, e, cfg in order:
            e.reset()
            e.process_device(buf.data_ptr(), T, T, st)
            e.sync()
            ms = e.timing_calls()
            if cfg:
                p, i, n = e.gonio_timing(True)
            if it >= WARM:
                t[name].append(float(ms[-1, 3]))
                if cfg:
                    tp[name].append(p)
                    ti[name].append(i)
    base = line("KMETER", t["KMETER"])
    for name, e, cfg in engines[:-1]:
        line(name, t[name], base)
        if cfg:
            line("    k_gonio_points", tp[name])
            line("    k_gonio_image", ti[name])
    audio = S * T * 8
    c, d = engines[0][1].gonio_config()
    pieces = (T + c.tune_piece - 1) // c.tune_piece
    print("bytes per call: every form reads the audio once, %.2f GB" % (audio / 1e9))
    print("  GONIO: k_gonio_points also writes %.2f GB of cell codes (2 B per frame and stream; scratch %d MB: pieces of %d frames, %d per call),"
          % (S * T * 2 / 1e9, S * ((c.tune_piece + 127) // 128 * 128) * 2 >> 20, c.tune_piece, pieces))
    print("         k_gonio_image reads them back and adds the touched cells of a stream's image per piece (at most 2 x 4 B per painted point;")
    for name, e, cfg in engines[:3]:
        img, drawn, clipped, skipped = e.gonio_image(0, 64)
        G = e.gonio_config()[1].G
        print("         %s: image %d x %d = %.1f MB per engine; first 64 streams: %.1f %% of the frames painted, %.1f %% clipped, %.1f %% of the cells touched)"
              % (name, G, G, S * G * G * 4 / 1e6, 100.0 * drawn.sum() / (64 * T), 100.0 * clipped.sum() / (64 * T), 100.0 * (img != 0).mean()))
    print("  NEEDLE and KMETER write their states only")
    for _, e, _ in engines:
        e.close()


# ---- track lengths (mtr_gonio_ends.h): --ends, --pairs -----------------------------------------------------------------------------------
FORMS = ["a", "b", "c", "d", "e"]
NAMES = {"a": "(a) dense call", "b": "(b) `_gonio_ends`, every stream open", "c": "(c) `_gonio_ends`, every end at T / 4",
         "d": "(d) dense call of T / 4 frames", "e": "(e) `_gonio_ends`, lengths uniform in [0, T]"}
LIB_AB = os.path.join(ROOT, "meters.lv2_amd", "lib_ab", "libmtr_engine.so")
ENDS_CFG = dict(shift=2, autogain=1)


def chunks(frames, piece, P=1920):
    """chunks of 128 frames that k_gonio_points must walk (NS = 16: a workgroup is 16 streams in lock step and walks a piece up to the last
    cut among them), and the frames its lanes draw there"""
    cut = np.array([M.gonio_cut(0, P, FS, T + 1, int(f), **ENDS_CFG)[2] for f in frames], np.int64)
    last = cut.reshape(-1, 16).max(axis=1)
    n = 0
    for f0 in range(0, T, piece):
        n += int(((np.clip(last - f0, 0, min(piece, T - f0)) + 127) // 128).sum())
    return n, int(cut.sum())


def ends(reps, piece):
    """five forms on one buffer in rotating order, each from a reset engine (auto gain on, shift 2); device events around the call"""
    buf = buffer()
    st = torch.cuda.current_stream().cuda_stream
    piece = piece or 4096
    rng = np.random.default_rng(35)
    frames = {"a": np.full(S, T, np.uint64), "b": np.full(S, T, np.uint64), "c": np.full(S, T // 4, np.uint64), "d": np.full(S, T // 4, np.uint64),
              "e": rng.integers(0, T + 1, S).astype(np.uint64)}
    must = {k: chunks(frames[k], piece) for k in FORMS}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    dev = {k: [] for k in FORMS}
    e = M.Engine(S, FS, M.METER_GONIO)
    e.gonio_configure(tune_piece=piece, **ENDS_CFG)

    def one(key):
        e.reset()
        torch.cuda.synchronize()
        ev[0].record()
        if key == "a":
            e.process_device(buf.data_ptr(), T, T, st)
        elif key == "d":
            e.process_device(buf.data_ptr(), T // 4, T, st)
        else:
            e.process_device_gonio_ends(buf.data_ptr(), T, frames[key], T, st)
        ev[1].record()
        e.sync()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1])

    for it in range(WARM + reps):
        r = it % len(FORMS)
        for key in FORMS[r:] + FORMS[:r]:
            d = one(key)
            if it >= WARM:
                dev[key].append(d)
    one("e")
    assert int(e.stream_frames()[0].sum()) == int(frames["e"].sum())
    # the two kernels apart for (a) and (b), in three more turns with events around every launch
    split = {"a": [], "b": []}
    e.gonio_timing(True)
    for it in range(3):
        for key in ("a", "b") if it % 2 == 0 else ("b", "a"):
            one(key)
            split[key].append(e.gonio_timing(True)[:2])
    e.gonio_timing(False)
    e.close()
    med = {k: float(np.median(dev[k])) for k in FORMS}
    print("GONIO auto gain, shift 2, pieces of %d: %d streams x %d s, %d turns after %d warm ones, rotating order" % (piece, S, T // int(FS), reps, WARM))
    print("| form | chunks to walk | share of the dense call's | frames drawn, share | device ms (median) | min – max |\n|---|---|---|---|---|---|")
    for k in FORMS:
        print("| %s | %d | %.3f | %.3f | %.3f | %.3f – %.3f |" % (NAMES[k], must[k][0], must[k][0] / must["a"][0], must[k][1] / must["a"][1], med[k],
                                                                  min(dev[k]), max(dev[k])), flush=True)
    print("(b) / (a) = %.3f; (c) / (d) = %.3f; (e) / (a) = %.3f at %.3f of the chunks and %.3f of the frames; (a) max / min = %.3f"
          % (med["b"] / med["a"], med["c"] / med["d"], med["e"] / med["a"], must["e"][0] / must["a"][0], must["e"][1] / must["a"][1],
             max(dev["a"]) / min(dev["a"])), flush=True)
    for k in ("a", "b"):
        v = np.median(np.asarray(split[k]), axis=0)
        print("%s: k_gonio_points %.3f ms, k_gonio_image %.3f ms (medians of 3, summed over the call's pieces)" % (NAMES[k], v[0], v[1]), flush=True)


def oversample(top, reps, piece):
    """the auto-gain 94 x 94 call at factor 1, 2 and `top`, taking turns on one buffer in rotating order, each from a reset engine"""
    buf = buffer()
    st = torch.cuda.current_stream().cuda_stream
    piece = piece or 4096
    factors = sorted({1, 2, top})
    engines = {}
    for f in factors:
        e = M.Engine(S, FS, M.METER_GONIO)
        e.gonio_configure(tune_piece=piece, **ENDS_CFG)
        e.gonio_set_oversample(f)
        e.gonio_timing(True)
        e.timing_enable(True)
        engines[f] = e
    whole, parts = {f: [] for f in factors}, {f: [] for f in factors}
    for it in range(WARM + reps):
        r = it % len(factors)
        for f in factors[r:] + factors[:r]:
            e = engines[f]
            e.reset()
            e.process_device(buf.data_ptr(), T, T, st)
            e.sync()
            ms = e.timing_calls()
            p, i, n = e.gonio_timing(True)
            o = e.gonio_os_timing()[0]
            if it >= WARM:
                whole[f].append(float(ms[-1, 3]))
                parts[f].append((o, p, i))
    print("GONIO auto gain, shift 2, tune_piece %d: %d streams x %d s, %d turns after %d warm ones, rotating order; ms: median (min - max)"
          % (piece, S, T // int(FS), reps, WARM))
    print("| factor | input frames per piece | whole call | k_gonio_os | k_gonio_points | k_gonio_image | k_gonio_os / k_gonio_points |\n|---|---|---|---|---|---|---|")
    med = {}
    for f in factors:
        v = np.asarray(parts[f])
        m = np.median(v, axis=0)
        med[f] = (float(np.median(whole[f])), *[float(t) for t in m])
        cell = lambda a: "%.2f (%.2f - %.2f)" % (np.median(a), np.min(a), np.max(a))   # noqa: E731
        print("| %d | %d | %s | %s | %s | %s | %.3f |" % (f, piece // f, cell(whole[f]), cell(v[:, 0]), cell(v[:, 1]), cell(v[:, 2]), m[0] / m[1]), flush=True)
    audio = S * T * 8
    for f in factors:
        w, o, p, i = med[f]
        pts = audio * f
        print("factor %d: k_gonio_points %.2f x its factor-1 time (%.1f ns per point and stream-lane)" % (f, p / med[1][2], p * 1e6 / (T * f)), flush=True)
        if f > 1:
            print("  k_gonio_os reads %.2f GB of audio (+ %.0f %% halo) and writes %.2f GB of points: %.2f TB/s; k_gonio_points reads them back (%.2f TB/s) and"
                  " writes %.2f GB of cell codes; k_gonio_image reads those" % (audio / 1e9, 100.0 * 23 / 128, pts / 1e9, (audio * (1 + 23 / 128) + pts) / o / 1e9,
                                                                               pts / p / 1e9, S * T * f * 2 / 1e9), flush=True)
    for e in engines.values():
        e.close()


def dense(reps, piece):
    """the dense call alone, of whichever library MTR_LIB names: one table row"""
    buf = buffer()
    st = torch.cuda.current_stream().cuda_stream
    t = []
    with M.Engine(S, FS, M.METER_GONIO) as e:
        e.gonio_configure(tune_piece=piece, **ENDS_CFG)
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for it in range(WARM + reps):
            e.reset()
            torch.cuda.synchronize()
            ev0.record()
            e.process_device(buf.data_ptr(), T, T, st)
            ev1.record()
            e.sync()
            torch.cuda.synchronize()
            if it >= WARM:
                t.append(ev0.elapsed_time(ev1))
    v = np.asarray(t)
    print("| %s | %.3f | %.3f | %.3f |" % ("parent" if os.environ.get("MTR_LIB") else "this build", np.median(v), v.min(), v.max()), flush=True)


def pairs(n, reps, piece):
    """the dense call of this build against the parent's library (tools/build_ab.sh -> meters.lv2_amd/lib_ab) in alternating child processes"""
    import subprocess
    if not os.path.exists(LIB_AB):
        sys.exit("no meters.lv2_amd/lib_ab: tools/build_ab.sh")
    print("| library (dense call, GONIO auto gain, shift 2) | median ms | min | max |\n|---|---|---|---|", flush=True)
    for _ in range(n):
        for lib in (None, LIB_AB):                                          # a fresh child each: nothing of one library's session is left for the other
            env = {k: v for k, v in os.environ.items() if k != "MTR_LIB"}
            if lib:
                env["MTR_LIB"] = lib
            subprocess.run([sys.executable, os.path.abspath(__file__), "--dense", str(reps), str(piece)], env=env, check=True, timeout=300)


if __name__ == "__main__":
    args = sys.argv[1:]
    mode = args.pop(0) if args and args[0] in ("--ends", "--pairs", "--dense", "--oversample") else None
    num = [int(v) for v in args]
    if mode == "--ends":
        ends(num[0] if num else 7, num[1] if len(num) > 1 else 0)
    elif mode == "--pairs":
        pairs(num[0] if num else 3, num[1] if len(num) > 1 else 7, num[2] if len(num) > 2 else 0)
    elif mode == "--oversample":
        oversample(num[0] if num else 4, num[1] if len(num) > 1 else 7, num[2] if len(num) > 2 else 0)
    elif mode == "--dense":
        dense(num[0] if num else 7, num[1] if len(num) > 1 else 0)
    else:
        main(num[0] if num else 7, num[1] if len(num) > 1 else 0)
