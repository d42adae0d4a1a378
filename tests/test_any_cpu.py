"""Track lengths for the scope and the surround meter (include/mtr_any.h): the surface, and the one-stream arithmetic tests/test_gpu_scope_any.py and
tests/test_gpu_surround_any.py lean on, without a GPU.  What the entry points compute is held on the GPU there."""
import ctypes as C
import os
import re

import numpy as np

import meters.lv2_amd as M
import _scope

HERE = os.path.dirname(os.path.abspath(__file__))
NEW = ["mtr_engine_process_device_any", "mtr_engine_process_host_any", "mtr_engine_scope_points"]
ERR_ARG = -1


def test_the_header_declares_the_three_entry_points_and_the_library_exports_them():
    assert M.exported_symbols("mtr_any.h") == NEW
    assert not set(NEW) & set(M.exported_symbols()) and not set(NEW) & set(M.exported_symbols("mtr_tpb_ends.h"))
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "mtr_engine.h")).read()
    assert re.search(r'^#include "mtr_any\.h"$', hdr, re.M)
    assert hdr.index('#include "mtr_tpb_ends.h"') < hdr.index('#include "mtr_any.h"') < hdr.index("mtr_engine_stream_frames (")
    assert re.search(r"#define\s+MTR_ABI_VERSION\s+2\b", hdr) and M.lib.mtr_abi_version() == 2   # (an addition inside version 2)
    for n in NEW:
        assert hasattr(M.lib, n), f"{n} is declared but libmtr_engine.so does not export it"


def test_the_ctypes_mirror_has_the_headers_signatures():
    """every parameter of the header's declarations, in order, against the argtypes of the binding"""
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(os.path.dirname(HERE), "include", "mtr_any.h")).read(), flags=re.S)
    kind = {"uint64_t": C.c_uint64, "uint32_t": C.c_uint32}
    for n in NEW:
        m = re.search(r"\bint\s+" + n + r"\s*\(([^)]*)\)\s*;", txt)
        assert m, n
        want = []
        for p in m.group(1).split(","):
            p = p.strip()
            want.append(C.c_void_p if "*" in p else kind[p.split()[0]])
        assert list(getattr(M.lib, n).argtypes) == want, (n, m.group(1))
    # the pair has the parameters of the _tpb pair, name for name
    tpb = re.sub(r"/\*.*?\*/", "", open(os.path.join(os.path.dirname(HERE), "include", "mtr_tpb_ends.h")).read(), flags=re.S)
    for form in ("device", "host"):
        a = re.search(r"mtr_engine_process_%s_any\s*\(([^)]*)\)" % form, txt).group(1)
        b = re.search(r"mtr_engine_process_%s_tpb\s*\(([^)]*)\)" % form, tpb).group(1)
        assert re.sub(r"\s+", " ", a) == re.sub(r"\s+", " ", b), form


def test_the_binding_has_the_methods():
    for n in ("process_device_any", "process_any", "scope_points"):
        assert callable(getattr(M.Engine, n))
    assert M.Engine._FAMILY["any"][0] == "mtr_engine_process_device_any"


def test_null_arguments_are_argument_errors_under_the_pairs_own_name():
    """without a device: the checks come before anything is queued"""
    f = np.zeros(1, np.uint64)
    x = np.zeros(8, np.float32)
    for args in ((None, x.ctypes.data, 4, 4, f.ctypes.data, None), (None, None, 0, 0, f.ctypes.data, None), (None, x.ctypes.data, 4, 4, None, None)):
        assert M.lib.mtr_engine_process_device_any(*args) == ERR_ARG
        assert M.lib.mtr_last_error() == b"mtr_engine_process_device_any: null argument"
        assert M.lib.mtr_engine_process_host_any(*args[:5]) == ERR_ARG
        assert M.lib.mtr_last_error() == b"mtr_engine_process_host_any: null argument"
    assert M.lib.mtr_engine_scope_points(None, 0, 0, f.ctypes.data, f.ctypes.data) == ERR_ARG
    assert M.lib.mtr_last_error()


def test_the_cut_with_a_streams_own_frames_counts_what_the_restatement_performs():
    """mtr_scope_series_cut with frames[s] in place of n_frames, for the ends of tests/test_gpu_scope_any.py: the analyses _scope.run
    performs on the stream's own frames — a hop that is not full runs none (gui/fft.c:308-311)"""
    fs = 48000
    for W, H in ((256, 777), (1024, 1920), (8192, 4096)):
        n1, n2 = 3 * H + 5, 4 * H + 1
        first = H - 5
        ends = [n2, 0, first - 1, first, first + 2 * H + 7, n2 - 1]
        x = _scope.signals(n1 + n2, fs, W, seed=5, S=1)[0]
        a1, _ = M.scope_series_cut(0, H, 0, 0, n1)
        assert a1 == 3 and n1 % H == 5
        got = []
        for E in ends:
            a2, p2 = M.scope_series_cut(5, H, a1 % 2, 2, E)
            assert a2 == (0 if E < first else (E - first) // H + 1)
            assert p2 == (a1 % 2 + a2) // 2
            got.append(a2)
            if W == 256:                                               # (the count does not depend on the window: one shape runs the transform)
                _, n_an = _scope.run(x[:n1 + E], W, H)
                assert n_an == a1 + a2, (H, E)
            assert (n1 + E) // H == a1 + a2
        assert got == [4, 0, 0, 1, 3, 4]


def test_a_truncated_last_block_of_the_oracle_is_the_reference_builds(oracle):
    """what tests/test_gpu_surround_any.py leans on: _sur.run_oracle on a stream's own frames — the last block cut to 0 < f frames, with
    f < 4, f mod 4 != 0 and f inside and behind the first tile — is bit for bit the reference's Kmeterdsp / Stcorrdsp objects fed the same
    blocks (ref_kmeter_*, ref_stcorr_* of oracle/_ref).  Held where oracle/_ref is present; elsewhere tests/test_surround_cpu.py holds the
    composition against the reference's recorded answers for whole blocks."""
    import _sur
    from _oracle import REF_SO, have_reference
    if not have_reference():
        return
    F = C.c_float
    R = C.CDLL(REF_SO)
    R.ref_stcorr_new.restype = R.ref_kmeter_new.restype = C.c_void_p
    R.ref_stcorr_new.argtypes = [C.c_int, F, F]
    R.ref_kmeter_new.argtypes = [F]
    R.ref_stcorr_read.restype = F
    R.ref_stcorr_read.argtypes = R.ref_stcorr_free.argtypes = R.ref_kmeter_free.argtypes = [C.c_void_p]
    R.ref_stcorr_process.argtypes = [C.c_void_p, C.POINTER(F), C.POINTER(F), C.c_int]
    R.ref_kmeter_process.argtypes = [C.c_void_p, C.POINTER(F), C.c_int]
    R.ref_kmeter_read.argtypes = [C.c_void_p, C.POINTER(F), C.POINTER(F)]
    O = _sur.bind(oracle.lib)
    fs, nch = 48000, 6
    x = _sur.signals(1023 + 12294, fs, nch, seed=526, S=2)[1]
    pa, pb = _sur.default_pairs(nch)
    fp = lambda a: a.ctypes.data_as(C.POINTER(F))
    for f in (1, 3, 1022, 7001, 12293, 12294):
        ends = [1023, 1023 + f]
        level, peak, corr, _ = _sur.run_oracle(O, fs, x[:ends[-1]], ends)
        km = [R.ref_kmeter_new(float(fs)) for _ in range(nch)]
        sc = [R.ref_stcorr_new(fs, 2e3, 0.3) for _ in range(4)]
        pos = 0
        for b, e in enumerate(ends):
            ch = [np.ascontiguousarray(x[pos:e, c]) for c in range(nch)]
            for p in range(4):
                R.ref_stcorr_process(sc[p], fp(ch[pa[p]]), fp(ch[pb[p]]), e - pos)
                got = np.float32(R.ref_stcorr_read(sc[p]))
                assert got.view(np.uint32) == corr[b, p].view(np.uint32), (f, b, p)
            for c in range(nch):
                m, q = F(), F()
                R.ref_kmeter_process(km[c], fp(ch[c]), e - pos)
                R.ref_kmeter_read(km[c], C.byref(m), C.byref(q))
                assert np.float32(m.value).view(np.uint32) == level[b, c].view(np.uint32), (f, b, c)
                assert np.float32(q.value).view(np.uint32) == peak[b, c].view(np.uint32), (f, b, c)
            pos = e
        for h in km:
            R.ref_kmeter_free(h)
        for h in sc:
            R.ref_stcorr_free(h)


def test_the_cut_against_a_count_frame_by_frame():
    """mtr_scope_series_cut, which the engine's per-stream counts and the GPU tests' expectations both use, against a count that shares
    nothing with it: the frames fed one by one, an analysis at every full hop, a point at every K-th analysis"""
    rng = np.random.default_rng(91)
    cases = [(0, 64, 0, 0, 0), (63, 64, 0, 1, 1), (5, 777, 1, 2, 4 * 777 + 1), (0, 1920, 2, 3, 1919), (1919, 1920, 0, 1, 1)]
    for _ in range(200):
        H = int(rng.integers(64, 3000))
        K = int(rng.integers(0, 5))
        cases.append((int(rng.integers(0, H)), H, int(rng.integers(0, K)) if K else 0, K, int(rng.integers(0, 6 * H))))
    for fill, H, since, K, n in cases:
        an = pt = 0
        f, g = fill, since
        for _ in range(n):
            f += 1
            if f == H:
                f, an = 0, an + 1
                if K:
                    g += 1
                    if g == K:
                        g, pt = 0, pt + 1
        assert M.scope_series_cut(fill, H, since, K, n) == (an, pt), (fill, H, since, K, n)
