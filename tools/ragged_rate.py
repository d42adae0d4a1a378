"""tools/ragged_rate.py — what a ragged call (mtr_engine_process_device_ragged) costs the phase correlation and the needle meters.  GPU box only.

One session, one device-resident buffer (8192 streams x 10 s at 48 kHz, the bench programme: mtr_synth_fill_device kind 1), and for
each of STCORR and NEEDLE (IEC II, the engine's default kind) at P = 0 and P = 4800 three forms that take turns call by call, after
two warm-up rounds:
    (a) the dense call (mtr_engine_process_device),
    (b) _ragged with every length equal to n_frames (the LEN kernels on the same bytes),
    (c) _ragged with lengths uniform in [0, n_frames] (about half the bytes).
Every call is followed by mtr_engine_reset, so that each form meters a fresh engine (a closed stream would stay closed).  Times are
the engine's own device events around each call (mtr_engine_timing_calls, column "whole call"); printed: median, min and max per
form, the ratio to (a), the bytes the form must read and their rate as a fraction of the HBM peak (8.0 TB/s).
Expected: (c) approaches half of (a) for STCORR, whose empty pieces return before they load anything; for NEEDLE it lies between half
and the whole, since a workgroup of 16 streams runs to the longest of them.
    python tools/ragged_rate.py [reps]

    python tools/ragged_rate.py --pairs [pairs [reps]]
holds the dense call against the parent commit's: `pairs` alternating same-box pairs of child processes, each timing (a) alone —
one with MTR_LIB=meters.lv2_amd/lib_ab/libmtr_engine.so (tools/build_ab.sh builds the parent there), one with this build.
    python tools/ragged_rate.py --dense [reps]
is what each child runs.
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

FS, S, T = 48000.0, 8192, 480000
HBM_PEAK = 8.0e12
WARM = 2
CASES = [("STCORR", 0), ("STCORR", 4800), ("NEEDLE", 0), ("NEEDLE", 4800)]


def report(name, v, nbytes, base=None):
    import numpy as np
    v = np.asarray(v, np.float64)
    med = float(np.median(v))
    line = "%-46s median %7.3f ms  min %7.3f  max %7.3f  %7.2f GB  %5.1f %% of HBM peak" % (
        name, med, v.min(), v.max(), nbytes / 1e9, 100.0 * nbytes / (med * 1e-3) / HBM_PEAK)
    if base:
        line += "  x %.3f of (a)" % (med / base)
    print(line, flush=True)
    return med


def session(reps, dense_only):
    import numpy as np
    import torch
    import meters.lv2_amd as M
    buf = torch.empty((S, T, 2), dtype=torch.float32, device="cuda")
    M.synth_fill_device(buf.data_ptr(), S, T, T, 777, FS, 1)
    torch.cuda.synchronize()
    st = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(8)
    which = os.environ.get("MTR_LIB") or "this build"
    full = np.full(S, T, np.uint64)
    half = rng.integers(0, T + 1, S).astype(np.uint64)
    for meter, P in CASES:
        forms = [("(a) dense", None)]
        if not dense_only:
            forms += [("(b) _ragged, lengths = n_frames", full), ("(c) _ragged, lengths uniform in [0, n]", half)]
        t = {f: [] for f, _ in forms}
        with M.Engine(S, FS, getattr(M, "METER_" + meter)) as e:
            if meter == "STCORR":
                e.stcorr_set_period(P, T // P + 1 if P else 0)
            else:
                e.needle_configure(M.NEEDLE_IEC2, P, T // P + 1 if P else 0)
            e.timing_enable(True)
            for it in range(WARM + reps):
                for f, L in forms:
                    if L is None:
                        e.process_device(buf.data_ptr(), T, T, st)
                    else:
                        e.process_device_ragged(buf.data_ptr(), T, L, T, st)
                    e.sync()
                    ms = e.timing_calls()
                    if it >= WARM:
                        t[f].append(float(ms[-1, 3]))
                    e.reset()
        base = None
        for f, L in forms:
            nbytes = S * T * 8 if L is None else int(L.sum()) * 8
            name = "%s P %d %s" % (meter, P, f)
            med = report(name + " [%s]" % which if dense_only else name, t[f], nbytes, base)
            base = base or med


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
            subprocess.run([sys.executable, os.path.abspath(__file__), "--dense", str(reps)], env=env, check=True, timeout=300)


if __name__ == "__main__":
    flags = [a for a in sys.argv[1:] if a.startswith("--")]
    nums = [int(a) for a in sys.argv[1:] if not a.startswith("--")]
    if "--pairs" in flags:
        pairs(nums[0] if nums else 3, nums[1] if len(nums) > 1 else 7)
    else:
        session(nums[0] if nums else 9, "--dense" in flags)
