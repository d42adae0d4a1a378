"""tools/lengths_rate.py — one process call with per-stream lengths against the dense call of the same n_frames, on the bench
shape (8192 streams x 10 s at 48 kHz, EBU R128 + true peak, layout 7).  GPU box only.

Each timed call starts from a reset engine (a call with lengths closes its streams: the next one would meter nothing), by HIP
events around the call; dense and ragged alternate, after one warm-up of each.  Printed: median and spread of each, their
ratio, and the same for lengths all equal to n_frames (the LEN kernels on open streams).
    python tools/lengths_rate.py [reps]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import meters.lv2_amd as M  # noqa: E402


def main(reps=7):
    fs, S, T = 48000.0, 8192, 480000
    buf = torch.empty((S, T, 2), dtype=torch.float32, device="cuda")
    M.synth_fill_device(buf.data_ptr(), S, T, T, 777, fs, 1)
    torch.cuda.synchronize()
    rng = np.random.default_rng(8)
    forms = {
        "dense": None,
        "uniform [0, 10 s]": rng.integers(0, T + 1, S).astype(np.uint64),
        "all n_frames": np.full(S, T, np.uint64),
    }
    t = {k: [] for k in forms}
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with M.Engine(S, fs, M.METER_EBU | M.METER_TRUEPEAK) as e:
        assert e.layout() == 7
        for it in range(reps + 1):
            for k, L in forms.items():
                e.reset()
                e.integr_start()
                e.sync()
                ev0.record()
                if L is None:
                    e.process_device(buf.data_ptr(), T)
                else:
                    e.process_device_lengths(buf.data_ptr(), T, L)
                ev1.record()
                e.sync()
                torch.cuda.synchronize()
                if it:
                    t[k].append(ev0.elapsed_time(ev1))
    base = np.median(t["dense"])
    for k, v in t.items():
        v = np.array(v)
        print("%-18s median %8.3f ms  min %8.3f  max %8.3f  ratio to dense %.3f" % (k, np.median(v), v.min(), v.max(), np.median(v) / base))


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 7)
