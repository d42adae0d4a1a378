"""Multichannel EBU R128 / true peak (n_channels 3, 4, 5) without a GPU: the oracle against golden_mc_v1 (recorded from
the reference's own Ebu_r128_proc (nchan) and TruePeakdsp objects) and the live reference where oracle/_ref is built; what
mtr_engine_create and mtr_plan_query accept and route."""
import ctypes as C
import os

import numpy as np
import pytest

import _mc

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "golden_mc_v1.npz"))


@pytest.fixture(scope="module")
def M():
    import meters.lv2_amd as m
    return m


def _key(n, fs, blk):
    return f"c{n}_{int(fs)}_{blk}"


@pytest.mark.parametrize("case", _mc.GOLDEN_CASES, ids=lambda c: _key(*c[:3]))
def test_oracle_reproduces_golden_mc(case):
    r, _ = _mc.run_case(_mc.McStream, *case)
    k = _key(*case[:3])
    for f in ("out9", "hist_M", "hist_S", "counts", "tp"):
        assert np.array_equal(r[f], G[f"{k}_{f}"]), (k, f, r[f], G[f"{k}_{f}"])
    assert r["counts"][0] > 0 and r["out9"][4] > -200.0      # integration ran: the case exercises the gate


@pytest.mark.skipif(not os.path.exists(_mc.REF_SO), reason="oracle/_ref not built here: golden_mc_v1 is its recording")
@pytest.mark.parametrize("case", [c for c in _mc.GOLDEN_CASES if c[2] == 1024], ids=lambda c: _key(*c[:3]))
def test_oracle_matches_live_reference_mc(case):
    got, _ = _mc.run_case(_mc.McStream, *case)
    want, _ = _mc.run_case(_mc.RefMcStream, *case)
    for f in ("out9", "hist_M", "hist_S", "counts", "tp"):
        assert np.array_equal(got[f], want[f]), (case, f)


def _create(M, n_channels, meters, **kw):
    cfg = M.engine._Config(struct_size=C.sizeof(M.engine._Config), meters=meters, n_streams=4, n_channels=n_channels,
                           sample_rate=48000.0, device=0, **kw)
    h = C.c_void_p()
    rc = M.lib.mtr_engine_create(C.byref(cfg), C.byref(h))
    if h.value:
        M.lib.mtr_engine_destroy(h)
    return rc


@pytest.mark.parametrize("n", [3, 4, 5])
@pytest.mark.parametrize("meters", ["EBU", "TP", "EBU|TP"])
def test_create_accepts_multichannel_loudness(M, n, meters):
    m = {"EBU": M.METER_EBU, "TP": M.METER_TRUEPEAK, "EBU|TP": M.METER_EBU | M.METER_TRUEPEAK}[meters]
    rc = _create(M, n, m)
    assert rc in (0, M.engine.ERR_NODEVICE), (rc, M.lib.mtr_last_error())


@pytest.mark.parametrize("n", [0, 6, 8])
def test_create_rejects_channel_counts(M, n):
    assert _create(M, n, M.METER_EBU | M.METER_TRUEPEAK) == M.engine.ERR_ARG


def test_create_mono_loudness_still_unsupported(M):
    # mono EBU / TRUEPEAK stays outside the engine's contract (the stereo suite's edge cases hold it there)
    assert _create(M, 1, M.METER_EBU) == M.engine.ERR_UNSUPPORTED
    assert _create(M, 1, M.METER_TRUEPEAK) == M.engine.ERR_UNSUPPORTED


@pytest.mark.parametrize("other", ["METER_SPECTR30", "METER_TPBALLIST", "METER_DR14", "METER_KMETER", "METER_BITSTATS", "METER_SIGDIST"])
def test_create_surround_other_meters_unsupported(M, other):
    assert _create(M, 5, M.METER_EBU | getattr(M, other)) == M.engine.ERR_UNSUPPORTED
    assert _create(M, 3, getattr(M, other)) == M.engine.ERR_UNSUPPORTED


def test_create_multichannel_tuning_knobs(M):
    E = M.engine
    assert _create(M, 5, M.METER_EBU, tune_layout=8) in (0, E.ERR_NODEVICE)
    for kw in (dict(tune_layout=6), dict(tune_layout=4), dict(tune_run=38), dict(tune_prune=1), dict(tune_fir=1)):
        assert _create(M, 5, M.METER_EBU | M.METER_TRUEPEAK, **kw) == E.ERR_ARG, kw
    # layout 8 is not a stereo layout
    assert _create(M, 2, M.METER_EBU | M.METER_TRUEPEAK, tune_layout=8) == E.ERR_ARG


@pytest.mark.parametrize("n", [3, 4, 5])
@pytest.mark.parametrize("fs", [44100.0, 48000.0])
def test_plan_query_routes_multichannel_to_layout8(M, n, fs):
    for meters in (M.METER_EBU | M.METER_TRUEPEAK, M.METER_EBU, M.METER_TRUEPEAK):
        p = M.plan_query(8192, int(10 * fs), sample_rate=fs, meters=meters, n_channels=n)
        assert p["layout"] == 8 and p["uses_seg"] == 0 and p["body_fragments"] == 0, p
        assert p["kw_segments"] >= 1 and p["n_tiles"] >= int(10 * fs) // 1280, p
        assert p["n_fragments_ended"] == 200, p


def test_plan_query_stereo_unchanged(M):
    # what the stereo planner answered before multichannel engines existed (layout 7 = k_kwtp16 + k_seg for a big batch)
    p = M.plan_query(8192, 480000, n_channels=2)
    assert p["layout"] == 7 and p["uses_seg"] == 1 and p["body_fragments"] == 200, p
    q = M.plan_query(8192, 480000, meters=M.METER_EBU, n_channels=2)
    assert q["layout"] == 4 and q["uses_seg"] == 0, q


def test_python_binding_has_truepeak_channels(M):
    assert hasattr(M.lib, "mtr_engine_truepeak_channels")
    assert hasattr(M.Engine, "truepeak_channels")
