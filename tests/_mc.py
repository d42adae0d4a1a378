"""Multichannel checkers (1 .. 5 channels): the CPU oracle's mo_ebu with nchan channels plus one TruePeakdsp per channel —
what Ebu_r128_proc::init (nchan, fs) and the LV2 glue's per-channel TruePeakdsp hold (ebumeter/ebu_r128_proc.h:26, 104;
src/ebulv2.cc:344-347, 361-365) — and the same driven through the reference's own objects where oracle/_ref is built."""
import ctypes as C
import os

import numpy as np

from _oracle import MoEbu, MoTp, build_oracle

HIST_LEN = 751
GAINS = (1.0, 1.0, 1.0, 1.41, 1.41)           # _chan_gain, ebu_r128_proc.cc:29 (L R C Ls Rs)
TP_MAX_FRAMES = 8192                          # TruePeakdsp::process_max takes at most this many frames per call

_f32p = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
REF_SO = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", "libmeters_ref.so")
REF_PROCESS = "_ZN4LV2M13Ebu_r128_proc7processEiPPf"     # Ebu_r128_proc::process (int, float**), exported by the reference build


def lcg(n, seed, gain):
    """n samples of the oracle's LCG noise (mo_fill_lcg: deterministic on every machine)."""
    lib = oracle_lib()
    buf = np.zeros(2 * n, np.float32)
    lib.mo_fill_lcg(buf, n, seed, gain)
    return buf[:n].copy()


def programme(T, C_, seed, fs=48000.0):
    """[T, C] float32: one level per channel (LCG noise), the second half 12 dB quieter than the first (a range to measure)."""
    x = np.zeros((T, C_), np.float32)
    for c in range(C_):
        lev = np.float32(0.5 * 10 ** (-(3 * c + (seed % 5)) / 20.0))
        x[:, c] = lcg(T, seed * 7 + c + 1, lev)
    x[T // 2:] *= np.float32(0.25)
    return x


_LIB = None


def oracle_lib():
    global _LIB
    if _LIB is None:
        lib = C.CDLL(build_oracle())
        lib.mo_fill_lcg.argtypes = [_f32p, C.c_uint32, C.c_uint32, C.c_float]
        lib.mo_fill_lcg.restype = None
        lib.mo_ebu_init.argtypes = [C.POINTER(MoEbu), C.c_int, C.c_float]
        lib.mo_ebu_process.argtypes = [C.POINTER(MoEbu), C.c_int, C.POINTER(C.c_void_p)]
        for f in ("mo_ebu_integr_start", "mo_ebu_integr_pause", "mo_ebu_integr_reset"):
            getattr(lib, f).argtypes = [C.POINTER(MoEbu)]
        lib.mo_tp_init.argtypes = [C.POINTER(MoTp), C.c_float]
        lib.mo_tp_process_max.argtypes = [C.POINTER(MoTp), _f32p, C.c_int]
        lib.mo_tp_read.argtypes = [C.POINTER(MoTp)]
        lib.mo_tp_read.restype = C.c_float
        _LIB = lib
    return _LIB


class McStream:
    """mo_ebu (nchan) + nchan TruePeakdsp, block by block, with the integration controls."""

    def __init__(self, nchan, fs):
        self.lib, self.n = oracle_lib(), nchan
        self.e = MoEbu()
        self.t = [MoTp() for _ in range(nchan)]
        self.lib.mo_ebu_init(C.byref(self.e), nchan, fs)
        for t in self.t:
            self.lib.mo_tp_init(C.byref(t), fs)
        self.hold = np.zeros(nchan, np.float32)

    def start(self):
        self.lib.mo_ebu_integr_start(C.byref(self.e))

    def pause(self):
        self.lib.mo_ebu_integr_pause(C.byref(self.e))

    def reset(self):
        self.lib.mo_ebu_integr_reset(C.byref(self.e))

    def process(self, x, with_tp=True):
        """x: [n, C] -> the per-channel peaks of this block (or None)"""
        ch = [np.ascontiguousarray(x[:, c], np.float32) for c in range(self.n)]
        ptrs = (C.c_void_p * self.n)(*[a.ctypes.data for a in ch])
        self.lib.mo_ebu_process(C.byref(self.e), x.shape[0], ptrs)
        if not with_tp:
            return None
        last = np.zeros(self.n, np.float32)
        for c in range(self.n):
            for o in range(0, ch[c].size, TP_MAX_FRAMES):          # (read () restarts the maximum: the call's peak is the max)
                seg = np.ascontiguousarray(ch[c][o:o + TP_MAX_FRAMES])
                self.lib.mo_tp_process_max(C.byref(self.t[c]), seg, seg.size)
                last[c] = max(last[c], self.lib.mo_tp_read(C.byref(self.t[c])))
        self.hold = np.maximum(self.hold, last)
        return last

    def get(self):
        e = self.e
        out9 = np.array([e.loudness_M, e.maxloudn_M, e.loudness_S, e.maxloudn_S, e.integrated, e.integ_thr,
                         e.range_min, e.range_max, e.range_thr], np.float32)
        return out9, np.array(e.hist_M.histc, np.int32), np.array(e.hist_S.histc, np.int32), (e.hist_M.count, e.hist_S.count)


class RefMcStream:
    """The same through the reference's Ebu_r128_proc (nchan) and TruePeakdsp objects (oracle/_ref/libmeters_ref.so)."""

    def __init__(self, nchan, fs):
        lib = C.CDLL(REF_SO)
        self.lib, self.n = lib, nchan
        lib.ref_ebu_new.argtypes = [C.c_int, C.c_float]
        lib.ref_ebu_new.restype = C.c_void_p
        lib.ref_ebu_free.argtypes = [C.c_void_p]
        for f in ("ref_ebu_integr_start", "ref_ebu_integr_pause", "ref_ebu_integr_reset"):
            getattr(lib, f).argtypes = [C.c_void_p]
        self.proc = getattr(lib, REF_PROCESS)
        self.proc.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
        self.proc.restype = None
        lib.ref_ebu_get.argtypes = [C.c_void_p, _f32p, np.ctypeslib.ndpointer(np.int32), np.ctypeslib.ndpointer(np.int32),
                                    np.ctypeslib.ndpointer(np.int32)]
        lib.ref_tp_new.argtypes = [C.c_float]
        lib.ref_tp_new.restype = C.c_void_p
        lib.ref_tp_free.argtypes = [C.c_void_p]
        lib.ref_tp_process_max.argtypes = [C.c_void_p, _f32p, C.c_int]
        lib.ref_tp_read.argtypes = [C.c_void_p]
        lib.ref_tp_read.restype = C.c_float
        self.h = lib.ref_ebu_new(nchan, fs)
        self.t = [lib.ref_tp_new(fs) for _ in range(nchan)]
        self.hold = np.zeros(nchan, np.float32)

    def close(self):
        self.lib.ref_ebu_free(self.h)
        for t in self.t:
            self.lib.ref_tp_free(t)

    def start(self):
        self.lib.ref_ebu_integr_start(self.h)

    def pause(self):
        self.lib.ref_ebu_integr_pause(self.h)

    def reset(self):
        self.lib.ref_ebu_integr_reset(self.h)

    def process(self, x, with_tp=True):
        ch = [np.ascontiguousarray(x[:, c], np.float32) for c in range(self.n)]
        ptrs = (C.c_void_p * self.n)(*[a.ctypes.data for a in ch])
        self.proc(self.h, x.shape[0], ptrs)
        if not with_tp:
            return None
        last = np.zeros(self.n, np.float32)
        for c in range(self.n):
            for o in range(0, ch[c].size, TP_MAX_FRAMES):
                seg = np.ascontiguousarray(ch[c][o:o + TP_MAX_FRAMES])
                self.lib.ref_tp_process_max(self.t[c], seg, seg.size)
                last[c] = max(last[c], self.lib.ref_tp_read(self.t[c]))
        self.hold = np.maximum(self.hold, last)
        return last

    def get(self):
        out9 = np.zeros(9, np.float32)
        hm = np.zeros(HIST_LEN, np.int32)
        hs = np.zeros(HIST_LEN, np.int32)
        cnt = np.zeros(2, np.int32)
        self.lib.ref_ebu_get(self.h, out9, hm, hs, cnt)
        return out9, hm, hs, (int(cnt[0]), int(cnt[1]))


# the golden cases: (nchan, fs, block, seconds, integration starts at this block)
GOLDEN_CASES = [(n, fs, blk, 8.0, 3) for n in (1, 3, 4, 5) for fs in (44100.0, 48000.0) for blk in (1024, 4800)]


def run_case(make, nchan, fs, block, seconds, start_at):
    """Feed programme () through a checker in `block`-frame calls, integration from block `start_at` on."""
    T = int(seconds * fs)
    x = programme(T, nchan, seed=nchan * 10 + int(fs) % 7 + block % 3)
    m = make(nchan, fs)
    for i, o in enumerate(range(0, T, block)):
        if i == start_at:
            m.start()
        m.process(x[o:o + block])
    out9, hm, hs, cnt = m.get()
    return dict(out9=out9, hist_M=hm, hist_S=hs, counts=np.array(cnt, np.int32), tp=m.hold.copy()), x
