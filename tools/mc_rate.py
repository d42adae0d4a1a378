"""tools/mc_rate.py — the multichannel kernel's rate (layout 8, mtr_kwmc.hip) next to the stereo kernels, one engine per case
in one process: 8192 streams x 10 s at 48 kHz, HIP events around 20 process calls after two of warm-up.  C in {3, 5} x
{EBU, EBU + TRUEPEAK}, and the stereo k_kw (layout 4) and k_kwtp16 (layout 6) at the same shape.  Prints per case the ms
per call, the kernel's own ms per call (the engine's fused-kernel events), and the fraction of 8 TB/s for 4 C bytes per frame.

    python tools/mc_rate.py [--streams 8192] [--seconds 10] [--calls 20] [--json out.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import meters.lv2_amd as M  # noqa: E402

HBM = 8.0e12


def case(name, C, meters, S, T, calls, **kw):
    fs = 48000.0
    dev = torch.empty((S, T, C), dtype=torch.float32, device="cuda")
    M.synth_fill_device(dev.data_ptr(), S, T * C // 2, T * C // 2, 99, fs, 1)
    torch.cuda.synchronize()
    with M.Engine(S, fs, meters, n_channels=C, **kw) as e:
        layout = M.lib.mtr_engine_layout(e._h)
        e.integr_start()
        for _ in range(2):
            e.process_device(dev.data_ptr(), T)
        e.sync()
        e.timing_enable(True)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            e.process_device(dev.data_ptr(), T)
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b) / calls
        fused = float(e.timing_calls()[:, 0].mean())
    del dev
    torch.cuda.empty_cache()
    byts = 4.0 * C * S * T
    r = dict(case=name, channels=C, layout=layout, ms=round(ms, 3), kernel_ms=round(fused, 3), gbytes=round(byts / 1e9, 2),
             hbm_frac=round(byts / (fused * 1e-3) / HBM, 3), hbm_frac_call=round(byts / (ms * 1e-3) / HBM, 3))
    print(json.dumps(r))
    sys.stdout.flush()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=8192)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--json")
    a = ap.parse_args()
    S, T = a.streams, int(a.seconds * 48000)
    E, TP = M.METER_EBU, M.METER_TRUEPEAK
    out = [case("stereo k_kw (layout 4)", 2, E, S, T, a.calls, tune_layout=4),
           case("stereo k_kwtp16 (layout 6)", 2, E | TP, S, T, a.calls, tune_layout=6)]
    for C in (3, 5):
        out.append(case(f"{C} ch EBU (layout 8)", C, E, S, T, a.calls))
        out.append(case(f"{C} ch EBU+TP (layout 8)", C, E | TP, S, T, a.calls))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
