"""Track lengths for the goniometer (include/mtr_gonio_ends.h) without a GPU: the surface, mtr_gonio_cut against the arithmetic of the
restatement (tests/_gonio_ends.py), its argument errors, the restatement itself against one-track runs of tests/_gonio.py, and the guard
of tests/test_gpu_gonio_ends.py on that test's own inputs."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _gonio
import _gonio_ends as GE

HERE = os.path.dirname(os.path.abspath(__file__))
INC = os.path.join(os.path.dirname(HERE), "include")
NEW = ["mtr_engine_gonio_points", "mtr_engine_process_device_gonio_ends", "mtr_engine_process_host_gonio_ends", "mtr_gonio_cut"]
U32 = np.uint32
FS = 48000.0


@pytest.fixture(scope="module")
def M():
    import meters.lv2_amd as m
    return m


def test_the_header_declares_the_entry_points_and_the_library_exports_them(M):
    assert M.exported_symbols("mtr_gonio_ends.h") == NEW
    assert not set(NEW) & set(M.exported_symbols()) and not set(NEW) & set(M.exported_symbols("mtr_gonio.h"))
    hdr = open(os.path.join(INC, "mtr_engine.h")).read()
    assert re.search(r'^#include "mtr_gonio_ends\.h"$', hdr, re.M)
    assert hdr.index('#include "mtr_gonio.h"') < hdr.index('#include "mtr_gonio_ends.h"')       # (it names mtr_gonio_config)
    assert re.search(r"#define\s+MTR_ABI_VERSION\s+2\b", hdr) and M.lib.mtr_abi_version() == 2  # (an addition inside version 2)
    for n in NEW:
        assert hasattr(M.lib, n), f"{n} is declared but libmtr_engine.so does not export it"
    for n in ("process_device_gonio_ends", "process_gonio_ends", "gonio_points"):
        assert callable(getattr(M.Engine, n))
    assert callable(M.gonio_cut)
    # the pair has the parameters of the _any pair, name for name
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(INC, "mtr_gonio_ends.h")).read(), flags=re.S)
    old = re.sub(r"/\*.*?\*/", "", open(os.path.join(INC, "mtr_any.h")).read(), flags=re.S)
    for form in ("device", "host"):
        a = re.search(r"mtr_engine_process_%s_gonio_ends\s*\(([^)]*)\)" % form, txt).group(1)
        b = re.search(r"mtr_engine_process_%s_any\s*\(([^)]*)\)" % form, old).group(1)
        assert re.sub(r"\s+", " ", a) == re.sub(r"\s+", " ", b), form
    # the documents no longer say that the meter is refused track lengths
    gonio = open(os.path.join(INC, "mtr_gonio.h")).read()
    assert "mtr_gonio_ends.h" in gonio and "its track lengths are a later change" not in gonio


@pytest.mark.parametrize("rate", [44100.0, 48000.0, 192000.0])
@pytest.mark.parametrize("P", [64, 480, 1920])
def test_cut_is_the_restatements_arithmetic(M, P, rate):
    n = 2 * P + 200
    seen = set()
    for fill in (0, 1, P - 1):
        for E in (0, 1, 63, 64, P - fill - 1, P - fill, P - fill + 63, P - fill + 64, n):
            whole, closing, drawn, att = M.gonio_cut(fill, P, rate, n, E, autogain=1)
            assert (whole, closing, drawn) == GE.cut(fill, P, n, E), (fill, E)
            r = (fill + E) % P
            if 0 < E < n and r >= 64:
                assert closing == r and drawn == E
                want = GE.attack(rate, r)
                assert [a.view(U32) for a in att] == [w.view(U32) for w in want], (fill, E, att, want)
                seen.add(r)
            else:
                assert closing == 0 and att == (0.0, 0.0)
                if 0 < E < n and r:
                    assert drawn == E - min(E, r)                  # stands behind its last whole update, not in front of the call
    assert seen or P == 64, "no closing update among the cases"    # (P = 64: r < 64 always — no stream ever gets one)
    if rate == 192000.0 and 64 in seen:
        assert GE.attack(rate, 64)[0] < 0                          # (elapsed = 1 / 3000 s: .31 + .1 log10f is negative, as the formula gives it)
    if P == 64:
        return
    # the dials are the configuration's
    a = M.gonio_cut(0, P, rate, n, 100, dials=(10.0, 90.0, 40.0, 50.0))[3]
    w = GE.attack(rate, 100, (10.0, 90.0, 40.0, 50.0))
    assert [v.view(U32) for v in a] == [v.view(U32) for v in w] and a != M.gonio_cut(0, P, rate, n, 100, autogain=1)[3]


def test_cut_refuses(M):
    E, lib = M.engine, M.lib
    cfg = M.gonio_config()
    w, c, d, a = C.c_uint64(), C.c_uint32(), C.c_uint64(), (C.c_float * 2)()
    ok = [0, 480, 48000.0, 1000, 500, C.byref(cfg), C.byref(w), C.byref(c), C.byref(d), a]
    assert lib.mtr_gonio_cut(*ok) == 0
    for i in (5, 6, 7, 8, 9):                                      # a NULL
        bad = list(ok)
        bad[i] = None
        assert lib.mtr_gonio_cut(*bad) == E.ERR_ARG, i
    for i, v in ((0, 480), (1, 0), (1, 63), (2, 7999.0), (4, 1001)):   # fill >= period, no period, one below the floor, the rate, frames > n_frames
        bad = list(ok)
        bad[i] = v
        assert lib.mtr_gonio_cut(*bad) == E.ERR_ARG, (i, v)
    bad_cfg = M.gonio_config(shift=7)
    assert lib.mtr_gonio_cut(*(ok[:5] + [C.byref(bad_cfg)] + ok[6:])) == E.ERR_ARG
    assert lib.mtr_engine_gonio_points(None, 0, 0, None, None) == E.ERR_ARG
    assert lib.mtr_engine_process_device_gonio_ends(None, None, 0, 0, None, None) == E.ERR_ARG
    assert lib.mtr_engine_process_host_gonio_ends(None, None, 0, 0, None) == E.ERR_ARG


def _same_track(o, g, s=0):
    for k in GE.STATE:
        a, b = getattr(o, k)[s:s + 1], getattr(g, k)
        assert a.tobytes() == b.tobytes(), k
    assert np.array_equal(o.img[s], g.img[0])


@pytest.mark.parametrize("autogain", [False, True])
def test_the_restatement_is_a_one_track_run_where_no_closing_update_runs(autogain):
    T, P = 1500, 480
    x = _gonio.signals(8, T, FS, 3)
    kw = dict(P=P, autogain=autogain)
    for E, upto in ((960, 960), (480, 480), (960 + 63, 960), (63, 0), (0, 0)):       # r = 0; 0 < r < 64: behind the last whole update
        o = GE.run(x, [E] * 8, FS, **kw)
        for s in range(8):
            g = _gonio.Gonio(1, FS, **kw).run(x[s:s + 1, :upto])
            _same_track(o, g, s)
            sg = g.series_arrays()
            assert o.updates[s] == upto // P and np.array_equal(o.s_gain[s, :upto // P].view(U32), sg[0][0].view(U32))
            assert not o.s_gain[s, upto // P:].any() and not o.s_drawn[s, upto // P:].any()
    # an open stream is the lock-step run
    o = GE.run(x, [T] * 8, FS, calls=[700, 800], **kw)
    g = _gonio.Gonio(8, FS, **kw).run(x)
    for k in GE.STATE:
        assert getattr(o, k).tobytes() == getattr(g, k).tobytes(), k
    assert np.array_equal(o.img, g.img) and (o.updates == T // P).all()


def test_a_closing_update_is_a_block_end_of_r_frames():
    """r >= 64: the state behind the closing draw_rb is that of a goniometer whose display update has r frames, run to its end"""
    T, P, r = 1500, 480, 200
    x = _gonio.signals(8, T, FS, 3)
    o = GE.run(x, [P + r] * 8, FS, P=P, autogain=True)
    g = _gonio.Gonio(8, FS, P=P, autogain=True).run(x[:, :P])
    g.d.P, g.d.attack, g.j = r, GE.attack(FS, r), 0                 # the second update has r frames, and r's attack pair
    g.run(x[:, P:P + r])
    for k in GE.STATE:
        assert getattr(o, k).tobytes() == getattr(g, k).tobytes(), k
    assert np.array_equal(o.img, g.img) and (o.updates == 2).all() and (o.r == r).all()
    assert np.array_equal(o.s_gain[:, 1].view(U32), g.series[1][0].view(U32)) and o.moved.any() and o.painted.any()
    assert not (o.xmax.any() or o.rms0.any() or o.bd.any())         # the accumulators are zero behind it
    # the cut into calls matters where a stream would have to be un-drawn: it stands at the closing call's start
    a = GE.run(x, [P + 30] * 8, FS, calls=[P + 10, T - P - 10], P=P)
    assert (a.stand == P + 10).all() and (a.updates == 1).all()
    b = GE.run(x, [P + 30] * 8, FS, P=P)
    assert (b.stand == P).all()


@pytest.mark.parametrize("autogain", [False, True])
def test_the_gpu_tests_inputs_meet_the_guard(autogain):
    S, T, P = 67, 5000, 480
    x = _gonio.signals(S, T, FS, 1)
    o = GE.run(x, GE.planted_ends(S, T, P), FS, P=P, autogain=autogain)
    GE.coverage_ends(o, autogain)
