"""Writes golden_mc_v1.npz: multichannel EBU R128 + per-channel true peak from the REFERENCE's own objects
(Ebu_r128_proc::init (nchan, fs) + Ebu_r128_proc::process, one TruePeakdsp per channel with process_max + read),
oracle/_ref/libmeters_ref.so — for nchan 1, 3, 4, 5 at 44.1 and 48 kHz, 1024- and 4800-frame blocks, integration from
the fourth block on.  The signals are the oracle's LCG noise (tests/_mc.py: programme), regenerated from their seeds.

    python tests/golden/make_golden_mc.py        (needs `make -C oracle ref`)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _mc  # noqa: E402


def main():
    out = {}
    for (n, fs, blk, sec, st) in _mc.GOLDEN_CASES:
        r, _ = _mc.run_case(_mc.RefMcStream, n, fs, blk, sec, st)
        key = f"c{n}_{int(fs)}_{blk}"
        for k, v in r.items():
            out[f"{key}_{k}"] = v
    np.savez_compressed(os.path.join(HERE, "golden_mc_v1.npz"), **out)
    print("wrote", len(_mc.GOLDEN_CASES), "cases")


if __name__ == "__main__":
    main()
