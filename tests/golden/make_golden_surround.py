#!/usr/bin/env python3
"""tests/golden/make_golden_surround.py — golden vectors for the surround meter, FROM THE REFERENCE BUILD
(oracle/_ref/libmeters_ref.so: jmeters/{stcorr,kmeter}dsp.cc compiled where they lie), composed as sur_run composes
them (src/surmeter.c:115-147): per 1024-frame block the pairs' Stcorrdsp::process + read (), then every channel's
Kmeterdsp::process + read (m, p).

Run in the authoring container only (needs the reference build); writes tests/golden/golden_surround_v1.npz: level, peak
and corr after every block of a reproducible noise signal (integer LCG and power-of-two gains only, so any machine
regenerates the same input bits), 8 channels with the default pairs and the first 5 with (1,4),(2,3),(0,4),(0,1), at
48 kHz and 44.1 kHz.  Data only — no reference text."""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _signals as sig  # noqa: E402
from _oracle import Reference  # noqa: E402

F = C.c_float
B = 1024
GAINS = (1.0, 0.5, 0.25, 1.0, 0.125, 0.0625, 0.5, 2.0 ** -10)
CASES = {8: ((0, 2, 4, 6), (1, 3, 5, 7)), 5: ((1, 2, 0, 0), (4, 3, 4, 1))}


def signal(fs, seed=2718):
    """one second of 8 channels: four LCG stereo pairs, each channel under a power-of-two gain"""
    n = int(fs)
    x = np.concatenate([sig.lcg_noise(n, seed + 11 * k, 1.0) for k in range(4)], axis=1)
    return np.ascontiguousarray(x * np.array(GAINS, np.float32))


def fp(a):
    return a.ctypes.data_as(C.POINTER(F))


def main():
    r = Reference().lib
    for f in ("ref_stcorr_new", "ref_kmeter_new"):
        getattr(r, f).restype = C.c_void_p
    r.ref_stcorr_new.argtypes = [C.c_int, F, F]
    r.ref_kmeter_new.argtypes = [F]
    r.ref_stcorr_read.restype = F
    r.ref_stcorr_read.argtypes = [C.c_void_p]
    r.ref_stcorr_process.argtypes = [C.c_void_p, C.POINTER(F), C.POINTER(F), C.c_int]
    r.ref_kmeter_process.argtypes = [C.c_void_p, C.POINTER(F), C.c_int]
    r.ref_kmeter_read.argtypes = [C.c_void_p, C.POINTER(F), C.POINTER(F)]
    out = {}
    for fs in (48000.0, 44100.0):
        x = signal(fs)
        for nch, (pa, pb) in CASES.items():
            cor = [r.ref_stcorr_new(int(fs), 2e3, 0.3) for _ in range(4)]
            km = [r.ref_kmeter_new(fs) for _ in range(nch)]
            level, peak, corr = [], [], []
            for q in range(0, x.shape[0] - B + 1, B):
                ch = [np.ascontiguousarray(x[q:q + B, c]) for c in range(nch)]
                cc = []
                for p in range(4):
                    r.ref_stcorr_process(cor[p], fp(ch[pa[p]]), fp(ch[pb[p]]), B)
                    cc.append(r.ref_stcorr_read(cor[p]))
                m, pk = F(), F()
                lv, pv = [], []
                for c in range(nch):
                    r.ref_kmeter_process(km[c], fp(ch[c]), B)
                    r.ref_kmeter_read(km[c], C.byref(m), C.byref(pk))
                    lv.append(m.value); pv.append(pk.value)
                level.append(lv); peak.append(pv); corr.append(cc)
            tag = f"{nch}_{int(fs)}"
            out[f"level_{tag}"] = np.array(level, np.float32)
            out[f"peak_{tag}"] = np.array(peak, np.float32)
            out[f"corr_{tag}"] = np.array(corr, np.float32)
    np.savez_compressed(os.path.join(HERE, "golden_surround_v1.npz"), **out)
    print("wrote golden_surround_v1.npz:", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
