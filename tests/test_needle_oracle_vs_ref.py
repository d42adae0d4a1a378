"""The needle-meter restatements (oracle/mtr_oracle.c: IEC 268-10 type I / II PPM, M/S PPM, stereo correlation,
K-meter) against the reference's own objects (oracle/_ref, built from jmeters/*.cc where they lie): every
value read after every block must be BIT-IDENTICAL, at several block sizes and sample rates.  Where oracle/_ref cannot be built,
the reference's reads come from their recording (tests/golden/golden_ref_calls_v1.npz)."""
import ctypes as C

import numpy as np
import pytest

import _signals as sig

pytestmark = pytest.mark.ref
F = C.c_float


class Ppm(C.Structure):
    _fields_ = [("z1", F), ("z2", F), ("m", F), ("res", C.c_int), ("w1", F), ("w2", F), ("w3", F), ("g", F)]


class MsPpm(C.Structure):
    _fields_ = [("p", Ppm), ("db", F), ("mv", F)]


class Stcorr(C.Structure):
    _fields_ = [("zl", F), ("zr", F), ("zlr", F), ("zll", F), ("zrr", F), ("w1", F), ("w2", F)]


class Kmeter(C.Structure):
    _fields_ = [("z1", F), ("z2", F), ("rms", F), ("peak", F), ("cnt", C.c_int), ("fpp", C.c_int), ("fall", F),
                ("flag", C.c_int), ("hold", C.c_int), ("fsamp", F), ("omega", F)]


def fp(a):
    return a.ctypes.data_as(C.POINTER(F))


def noise(n, seed, gain=1.0):
    x = sig.lcg_noise(n, seed, gain)
    env = (np.arange(n) % 20000 < 6000).astype(np.float32) * np.float32(0.9) + np.float32(0.1)   # bursts: attack and decay
    return (x[:, 0] * env).copy(), (x[:, 1] * env[::-1]).copy()


def _bind_ref(r):
    """argtypes of the reference shim's needle entry points (r: the live Reference)."""
    r = r.lib
    for f in ("ref_ppm_new", "ref_msppm_new", "ref_stcorr_new", "ref_kmeter_new"):
        getattr(r, f).restype = C.c_void_p
    r.ref_ppm_new.argtypes = [C.c_int, F]
    r.ref_msppm_new.argtypes = [F, F]
    r.ref_stcorr_new.argtypes = [C.c_int, F, F]
    r.ref_kmeter_new.argtypes = [F]
    for f in ("ref_ppm_read", "ref_msppm_read", "ref_stcorr_read"):
        getattr(r, f).restype = F
        getattr(r, f).argtypes = [C.c_void_p]
    r.ref_ppm_process.argtypes = [C.c_void_p, C.POINTER(F), C.c_int]
    r.ref_msppm_process.argtypes = [C.c_void_p, C.POINTER(F), C.POINTER(F), C.c_int, C.c_int]
    r.ref_msppm_set_gain.argtypes = [C.c_void_p, F]
    r.ref_stcorr_process.argtypes = [C.c_void_p, C.POINTER(F), C.POINTER(F), C.c_int]
    r.ref_kmeter_process.argtypes = [C.c_void_p, C.POINTER(F), C.c_int]
    r.ref_kmeter_read.argtypes = [C.c_void_p, C.POINTER(F), C.POINTER(F)]
    for f in ("ref_ppm_free", "ref_msppm_free", "ref_stcorr_free", "ref_kmeter_free", "ref_kmeter_reset"):
        getattr(r, f).argtypes = [C.c_void_p]
    return r


@pytest.fixture(scope="module")
def olib(oracle):
    o = oracle.lib
    for f in ("mo_ppm_read", "mo_msppm_read", "mo_stcorr_read"):
        getattr(o, f).restype = F
    o.mo_ppm_init_iec1.argtypes = o.mo_ppm_init_iec2.argtypes = [C.POINTER(Ppm), F]
    o.mo_ppm_process.argtypes = [C.POINTER(Ppm), C.POINTER(F), C.c_int]
    o.mo_ppm_read.argtypes = [C.POINTER(Ppm)]
    o.mo_msppm_init.argtypes = [C.POINTER(MsPpm), F, F]
    o.mo_msppm_set_gain.argtypes = [C.POINTER(MsPpm), F]
    o.mo_msppm_process.argtypes = [C.POINTER(MsPpm), C.POINTER(F), C.POINTER(F), C.c_int, C.c_int]
    o.mo_msppm_read.argtypes = [C.POINTER(MsPpm)]
    o.mo_stcorr_init.argtypes = [C.POINTER(Stcorr), C.c_int, F, F]
    o.mo_stcorr_process.argtypes = [C.POINTER(Stcorr), C.POINTER(F), C.POINTER(F), C.c_int]
    o.mo_stcorr_read.argtypes = [C.POINTER(Stcorr)]
    o.mo_kmeter_init.argtypes = [C.POINTER(Kmeter), F]
    o.mo_kmeter_process.argtypes = [C.POINTER(Kmeter), C.POINTER(F), C.c_int]
    o.mo_kmeter_read.argtypes = [C.POINTER(Kmeter), C.POINTER(F), C.POINTER(F)]
    o.mo_kmeter_reset.argtypes = [C.POINTER(Kmeter)]
    return o


BLOCKS = (64, 1000, 1024, 4099)


# The reference's side of each test: every value it reads, in order (reference.run: live, or its recording)

def _ref_ppm(R, kind, fs, x, B):
    r, out = _bind_ref(R), []
    h = r.ref_ppm_new(kind, fs)
    for i, q in enumerate(range(0, x.size - B + 1, B)):
        blk = x[q:q + B].copy()
        r.ref_ppm_process(h, fp(blk), B)
        if i % 3 != 2:                                           # the maximum is held over unread blocks
            out.append(r.ref_ppm_read(h))
    r.ref_ppm_free(h)
    return np.array(out, np.float32)


def _ref_msppm(R, fs, xl, xr, B, side, db):
    r, out = _bind_ref(R), []
    h = r.ref_msppm_new(fs, -6.0)
    for i, q in enumerate(range(0, xl.size - B + 1, B)):
        if i == 5:                                               # the "+20 dB" switch of the S needle (bbcm_run)
            r.ref_msppm_set_gain(h, db)
        bl, br = xl[q:q + B].copy(), xr[q:q + B].copy()
        r.ref_msppm_process(h, fp(bl), fp(br), B, side)
        out.append(r.ref_msppm_read(h))
    r.ref_msppm_free(h)
    return np.array(out, np.float32)


def _ref_stcorr(R, fs, xl, xr, B):
    r, out = _bind_ref(R), []
    h = r.ref_stcorr_new(fs, 2e3, 0.3)
    for i, q in enumerate(range(0, xl.size - B + 1, B)):
        bl, br = xl[q:q + B].copy(), xr[q:q + B].copy()
        r.ref_stcorr_process(h, fp(bl), fp(br), B)
        out.append(r.ref_stcorr_read(h))
    r.ref_stcorr_free(h)
    return np.array(out, np.float32)


def _ref_kmeter(R, fs, x, B):
    r, out = _bind_ref(R), []
    h = r.ref_kmeter_new(fs)
    ra, rp = F(), F()
    for i, q in enumerate(range(0, x.size - B + 1, B)):
        n = B if i % 7 else B - 3                                # a change of period size recomputes the fallback factor
        blk = x[q:q + n].copy()
        r.ref_kmeter_process(h, fp(blk), n)
        if i % 2 == 0:
            r.ref_kmeter_read(h, C.byref(ra), C.byref(rp))
            out.append((ra.value, rp.value))
        if i == 40:
            r.ref_kmeter_reset(h)
    r.ref_kmeter_free(h)
    return np.array(out, np.float32).reshape(-1, 2)


def _same(a, b):
    return np.float32(a).tobytes() == np.float32(b).tobytes()


@pytest.mark.parametrize("kind", [1, 2])
@pytest.mark.parametrize("fs", [44100.0, 48000.0, 96000.0])
def test_iec_ppm(olib, reference, kind, fs):
    o = olib
    x, _ = noise(60000, 5 + kind)
    for B in BLOCKS:
        want = reference.run("ppm", _ref_ppm, kind, fs, x, B)
        p = Ppm()
        (o.mo_ppm_init_iec1 if kind == 1 else o.mo_ppm_init_iec2)(C.byref(p), fs)
        j = 0
        for i, q in enumerate(range(0, x.size - B + 1, B)):
            blk = x[q:q + B].copy()
            o.mo_ppm_process(C.byref(p), fp(blk), B)
            if i % 3 != 2:                                       # the maximum is held over unread blocks
                a, b = want[j], o.mo_ppm_read(C.byref(p))
                j += 1
                assert _same(a, b), (kind, fs, B, i, a, b)
        assert j == want.size, (kind, fs, B)


def test_ms_ppm(olib, reference):
    o = olib
    fs = 48000.0
    xl, xr = noise(60000, 9)
    for B in BLOCKS:
        for side, db in ((0, -6.0), (1, -6.0), (1, 14.0)):
            want = reference.run("msppm", _ref_msppm, fs, xl, xr, B, side, db)
            p = MsPpm()
            o.mo_msppm_init(C.byref(p), fs, -6.0)
            n = 0
            for i, q in enumerate(range(0, xl.size - B + 1, B)):
                if i == 5:                                       # the "+20 dB" switch of the S needle (bbcm_run)
                    o.mo_msppm_set_gain(C.byref(p), db)
                bl, br = xl[q:q + B].copy(), xr[q:q + B].copy()
                o.mo_msppm_process(C.byref(p), fp(bl), fp(br), B, side)
                a, b = want[i], o.mo_msppm_read(C.byref(p))
                n += 1
                assert _same(a, b), (B, side, db, i, a, b)
            assert n == want.size, (B, side, db)


@pytest.mark.parametrize("fs", [44100, 48000, 96000])
def test_stereo_correlation(olib, reference, fs):
    o = olib
    xl, xr = noise(50000, 13)
    xr[:20000] = xl[:20000]                                      # +1, then decorrelated, then inverted
    xr[35000:] = -xl[35000:]
    xl[40000], xr[40001] = np.inf, np.nan                        # the non-finite scrub at block ends
    for B in BLOCKS:
        want = reference.run("stcorr", _ref_stcorr, fs, xl, xr, B)
        c = Stcorr()
        o.mo_stcorr_init(C.byref(c), fs, 2e3, 0.3)
        n = 0
        for i, q in enumerate(range(0, xl.size - B + 1, B)):
            bl, br = xl[q:q + B].copy(), xr[q:q + B].copy()
            o.mo_stcorr_process(C.byref(c), fp(bl), fp(br), B)
            a, b = want[i], o.mo_stcorr_read(C.byref(c))
            n += 1
            assert _same(a, b), (fs, B, i, a, b)
        assert n == want.size, (fs, B)


@pytest.mark.parametrize("fs", [44100.0, 48000.0, 96000.0])
def test_kmeter(olib, reference, fs):
    o = olib
    x, _ = noise(120000, 17, 0.8)
    x[70000:] *= np.float32(0.05)                                # quiet tail: peak hold (0.5 s) then fallback
    for B in BLOCKS:
        want = reference.run("kmeter", _ref_kmeter, fs, x, B)
        k = Kmeter()
        o.mo_kmeter_init(C.byref(k), fs)
        oa, op = F(), F()
        j = 0
        for i, q in enumerate(range(0, x.size - B + 1, B)):
            n = B if i % 7 else B - 3                            # a change of period size recomputes the fallback factor
            blk = x[q:q + n].copy()
            o.mo_kmeter_process(C.byref(k), fp(blk), n)
            if i % 2 == 0:
                o.mo_kmeter_read(C.byref(k), C.byref(oa), C.byref(op))
                (ra, rp), j = want[j], j + 1
                assert _same(ra, oa.value), (fs, B, i, ra, oa.value)
                assert _same(rp, op.value), (fs, B, i, rp, op.value)
            if i == 40:
                o.mo_kmeter_reset(C.byref(k))
        assert j == len(want), (fs, B)
