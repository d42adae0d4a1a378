"""tools/surround_rate.py — what the surround meter (MTR_METER_SURROUND, mtr_surround.hip) costs, and what the same readings cost
with the parent commit's library.  GPU box only.

One session, one device-resident buffer: 8192 streams x 10 s at 48 kHz of 6-channel f32 (94.4 GB; --eight: 4096 streams of 8
channels, 62.9 GB), filled with uniform noise under per-channel gains.
  * this build: one SURROUND engine, every call one sur_run (P = 0) and with the reading series at P = 4800;
  * the parent (tools/build_ab.sh builds it into meters.lv2_amd/lib_ab; run as a child process with MTR_LIB naming it): what a user
    of that library needs for the same readings of a 6-channel frame — three KMETER | STCORR stereo engines with the frame layouts
    6,{0,1}, 6,{2,3}, 6,{4,5} and one STCORR engine for the fourth pair (6,{5,5}: the default pair (6,7) clamped), all over the same
    buffer, one after the other.  (Its K-meters have no reading series: the P = 4800 row sets the period on the STCORR halves alone.)
Times are HIP events around the calls (torch.cuda.Event), median of `reps` >= 10 after two warm-up rounds; printed: both medians,
their ratio, and the new pass as a fraction of the HBM peak (8.0 TB/s) for one read of the buffer.
    tools/build_ab.sh HEAD~1 && python tools/surround_rate.py [reps] [--eight]
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import meters.lv2_amd as M  # noqa: E402

FS, T = 48000.0, 480000
HBM_PEAK = 8.0e12
WARM = 2
LIB_AB = os.path.join(ROOT, "meters.lv2_amd", "lib_ab", "libmtr_engine.so")


def buffer(S, nch):
    buf = torch.empty((S, T, nch), dtype=torch.float32, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(777)
    gains = torch.tensor([0.5, 0.4, 0.3, 0.2, 0.2, 0.1, 0.05, 0.01][:nch], device="cuda")
    for s0 in range(0, S, 256):                                          # (in slabs: no second buffer of that size)
        sl = buf[s0:s0 + 256]
        sl.uniform_(-1.0, 1.0, generator=g)
        sl.mul_(gains)
    torch.cuda.synchronize()
    return buf


def timed(fn, reps):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t = []
    for it in range(WARM + reps):
        ev0.record()
        fn()
        ev1.record()
        torch.cuda.synchronize()
        if it >= WARM:
            t.append(ev0.elapsed_time(ev1))
    return [float(v) for v in t]


def this_build(S, nch, reps):
    buf = buffer(S, nch)
    st = torch.cuda.current_stream().cuda_stream
    out = {}
    for P in (0, 4800):
        with M.Engine(S, FS, M.METER_SURROUND, n_channels=nch) as e:
            e.surround_set_period(P, T // P if P else 0)
            out[P] = timed(lambda: e.process_device(buf.data_ptr(), T, T, st), reps)
            level, peak, corr = e.surround_read(0, 4)
            assert np.all(np.isfinite(level)) and np.all(level > 0) and np.all(np.abs(corr) <= 1.0 + 1e-6)
    return out


def parent_composition(S, nch, reps):
    """with whatever library MTR_LIB names: the stereo engines a 6-channel (or wider) frame takes there"""
    buf = buffer(S, nch)
    st = torch.cuda.current_stream().cuda_stream
    pairs = [(0, 1), (2, 3), (4, 5), (min(6, nch - 1), min(7, nch - 1))]
    out = {}
    for P in (0, 4800):
        engines = []
        for k, pr in enumerate(pairs):
            kmeter = k < (nch + 1) // 2 and pr[0] != pr[1]               # (every channel's K-meter once)
            e = M.Engine(S, FS, (M.METER_KMETER if kmeter else 0) | M.METER_STCORR)
            e.set_frame_layout(nch, list(pr))
            e.set_host_chunk_bytes(1 << 30)
            if P:
                e.stcorr_set_period(P, T // P)
            engines.append(e)

        def step():
            for e in engines:
                e.process_device(buf.data_ptr(), T, T, st)
        out[P] = timed(step, reps)
        for e in engines:
            e.close()
    return out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = max(10, int(args[0])) if args else 11
    S, nch = (4096, 8) if "--eight" in sys.argv else (8192, 6)
    if "--parent" in sys.argv:
        print("PARENT " + json.dumps({str(k): v for k, v in parent_composition(S, nch, reps).items()}))
        return
    new = this_build(S, nch, reps)
    torch.cuda.empty_cache()
    old = None
    if os.path.exists(LIB_AB):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), str(reps), "--parent"] + (["--eight"] if nch == 8 else []),
                           env=dict(os.environ, MTR_LIB=LIB_AB), capture_output=True, text=True, timeout=1100)
        for line in r.stdout.splitlines():
            if line.startswith("PARENT "):
                old = {int(k): v for k, v in json.loads(line[7:]).items()}
        if old is None:
            print("the parent's run failed:", r.stdout[-2000:], r.stderr[-2000:])
    else:
        print("no meters.lv2_amd/lib_ab: tools/build_ab.sh <parent revision> builds it")
    nbytes = S * T * nch * 4
    print("%d streams x %d frames x %d channels f32 = %.1f GB, %d repetitions" % (S, T, nch, nbytes / 1e9, reps))
    for P in (0, 4800):
        v = np.asarray(new[P])
        med = float(np.median(v))
        line = "P = %-5d SURROUND median %8.3f ms (min %8.3f max %8.3f)  %5.1f %% of HBM peak" % (P, med, v.min(), v.max(), 100.0 * nbytes / (med * 1e-3) / HBM_PEAK)
        if old:
            w = np.asarray(old[P])
            line += " | parent's four stereo engines median %8.3f ms (min %8.3f max %8.3f)  x %.2f" % (np.median(w), w.min(), w.max(), np.median(w) / med)
        print(line)


if __name__ == "__main__":
    main()
