"""Track lengths for the 30-band bank (mtr_engine_process_device_ends / _host_ends, mtr_engine_spectr_points, include/mtr_ends.h; the two
ENDS instantiations of k_bank) on the GPU.  Every stream of the engine under test is held two ways (tests/_bank_ends.py):
  * bit for bit against the existing path: an engine without a period that is fed stream s alone, in calls of P frames plus a last call
    of r frames (P = 0: the same calls with the last one cut at frames[s]), mtr_engine_spectrum read after each;
  * against the oracle's handle fed the same blocks, with tests/_bank.py's contract: val, max rtol = BANK_REL, atol = BANK_ATOL; val_db,
    max_db DB_TOL where the oracle is above DB_FLOOR.
Shapes: 5 streams (waves {0, 1, 2}, {2, 3, 4}, {4}), calls of 600 frames (four chunks and a partial fifth), P = 100."""
import numpy as np
import pytest

import _bank as B
import _bank_ends as E
import _bank_series as BS
from test_gpu_parity import M  # noqa: F401  (M: the module fixture)

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_UNSUPPORTED = -1, -2
MODES = [BS.HOLD, BS.BLOCK]
MODE_IDS = ["hold", "block"]
TINY = np.float32(1e-20)
S, N, P = E.S, E.N, E.P


def close(got, want, what):
    """the contract of tests/_bank.py on two dicts of equally shaped arrays"""
    for k in BS.KEYS:
        assert got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        assert np.isfinite(got[k]).all(), (what, k)
    for k in ("val", "max"):
        g, w = got[k].astype(np.float64), want[k].astype(np.float64)
        assert np.allclose(g, w, rtol=B.BANK_REL, atol=B.BANK_ATOL), (what, k, float(np.abs(g - w).max()) if g.size else 0.0)
    for k in ("val_db", "max_db"):
        live = want[k] > B.DB_FLOOR
        assert np.allclose(got[k][live], want[k][live], atol=B.DB_TOL), (what, k)


def row(d, s, a=None, b=None):
    return {k: v[s, a:b] for k, v in d.items()}


def held(M, oracle, x, got, totals, period, mode, mono, what, calls=None, speed=B.SPEED, tag="noise", cap=16, skip=()):
    """Every stream s of `got` (tests/_bank_ends.through) against its two yardsticks after totals[s] frames of its own; skip: streams
    the caller holds otherwise."""
    for s in range(x.shape[0]):
        if s in skip:
            continue
        who = "%s stream %d (%d frames)" % (what, s, totals[s])
        cuts = E.cuts_of(totals[s], period, calls)
        y_ser, y_fin = E.yard(M, x[s], cuts, mode, mono, speed, key=(tag, s))
        o_ser, o_fin = E.oracle_cuts(oracle, x[s], cuts, mode, mono, speed, key=(tag, s))
        assert BS.same(row(got["spectrum"], s), y_fin), who + ": mtr_engine_spectrum is not the existing path's"
        if cuts:                                                 # (the handle's dB ports are those of its last run; BLOCK: max_f was reset behind it)
            keys = ("val", "val_db") if mode == BS.BLOCK else BS.KEYS
            close({k: row(got["spectrum"], s)[k] if k in keys else o_fin[k] for k in BS.KEYS}, o_fin, who + " spectrum")
        if not period:
            assert got["points"][s] == 0, who
            continue
        own = len(cuts)
        assert got["points"][s] == own, (who, got["points"].tolist())
        kept = min(own, cap)
        ser = row(got["series"], s)
        assert BS.same({k: v[:kept] for k, v in ser.items()}, {k: v[:kept] for k, v in y_ser.items()}), who + ": the series is not the existing path's"
        close({k: v[:kept] for k, v in ser.items()}, {k: v[:kept] for k, v in o_ser.items()}, who + " series")
        # behind its own points a closed stream's row holds 0.0f, the dB outputs -100
        assert not ser["val"][kept:].any() and not ser["max"][kept:].any(), who
        assert (ser["val_db"][kept:] == -100.0).all() and (ser["max_db"][kept:] == -100.0).all(), who


# ---- a. one closing call: the ends x width x peak mode x period, an even and an odd stride ------------------------------------------------

@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("mono", [False, True], ids=["stereo", "mono"])
@pytest.mark.parametrize("name", list(E.ENDS))
def test_one_closing_call(M, oracle, name, mono, mode):  # noqa: F811
    x = E.batch()
    ends = E.ENDS[name]
    f = np.array(ends, np.uint64)
    for period, pad in ((P, 0), (P, 7), (0, 7)):
        if period == 0 and mode == BS.BLOCK:
            continue                                             # (the peak mode belongs to the series)
        what = "%s P=%d stride %d %s %s" % (name, period, N + pad, "mono" if mono else "stereo", MODE_IDS[mode])
        got = E.through(M, x, [(N, f)], period, mode=mode, mono=mono, pad=pad)
        assert got["frames"].tolist() == ends and got["closed"].tolist() == [v < N for v in ends], what
        if period:
            assert (got["n_points"], got["dropped"]) == (N // period, 0) and got["series"]["val"].shape == (S, N // period, B.NBANDS), what
            assert got["points"].tolist() == [sum(E.expected_points(0, period, N, v)) for v in ends], what
        held(M, oracle, x, got, ends, period, mode, mono, what, calls=[N])


def test_every_stream_open_is_the_dense_call(M):  # noqa: F811
    """frames[s] == n_frames for all: bit for bit mtr_engine_process_device, blob included, with and without a period"""
    x = E.batch()
    for period in (0, P):
        a = E.through(M, x, [(N, np.full(S, N, np.uint64))], period, mode=BS.BLOCK, pad=7)
        b = E.through(M, x, [(N, None)], period, mode=BS.BLOCK, pad=7)
        assert E.same_result(a, b) and not a["closed"].any(), period


# ---- b. two calls: the ends fall in the second, which starts mid-block ------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("second", [[129, 350, 0, 257, 99], [1, 2, 50, 51, 350]], ids=["mixed", "around-a-block-end"])
def test_the_ends_fall_in_a_second_call_that_starts_mid_block(M, oracle, second, mode):  # noqa: F811
    """calls of 250 and 350 frames: the second one starts 50 frames into block 2 (e0 = 50, not P).  frames 0 in it closes a stream where
    the first call left it — mid-block, no epilogue, no point: that stream is held against the engine after the first call alone."""
    n1, n2 = 250, 350
    x = E.batch()
    f = np.array(second, np.uint64)
    totals = [n1 + v for v in second]
    for period in (P, 0):
        if period == 0 and mode == BS.BLOCK:
            continue
        what = "two calls P=%d %s" % (period, MODE_IDS[mode])
        got = E.through(M, x, [(n1, None), (n2, f)], period, mode=mode, pad=3)
        first = E.through(M, x, [(n1, None)], period, mode=mode, pad=3)
        assert got["frames"].tolist() == totals and got["closed"].tolist() == [v < n2 for v in second], what
        untouched = [s for s in range(S) if second[s] == 0]
        held(M, oracle, x, got, totals, period, mode, False, what, calls=[n1, n2], skip=untouched if period else ())
        if period:
            assert (got["n_points"], got["dropped"]) == ((n1 + n2) // P, 0), what
            want = [n1 // P + sum(E.expected_points(n1 % P, P, n2, v)) for v in second]
            assert got["points"].tolist() == want, (what, got["points"].tolist(), want)
            for s in untouched:
                assert BS.same(row(got["spectrum"], s), row(first["spectrum"], s)), what
                assert BS.same(row(got["series"], s, 0, n1 // P), row(first["series"], s)), what
                assert not got["series"]["val"][s, n1 // P:].any() and not got["series"]["max"][s, n1 // P:].any(), what


def test_a_truncated_point_past_the_capacity_is_dropped(M):  # noqa: F811
    """capacity 2: stream 0 (129 frames) keeps its whole block and its truncated point, stream 3 (257) its two whole blocks only — and
    nothing is written past a stream's row"""
    x = E.batch()
    f = np.array(E.ENDS["mixed"], np.uint64)
    full = E.through(M, x, [(N, f)], P, cap=16, mode=BS.BLOCK)
    short = E.through(M, x, [(N, f)], P, cap=2, mode=BS.BLOCK)
    assert (short["n_points"], short["dropped"]) == (6, 4) and short["points"].tolist() == full["points"].tolist() == [2, 6, 0, 3, 1]
    assert BS.same(short["series"], {k: v[:, :2] for k, v in full["series"].items()}) and BS.same(short["spectrum"], full["spectrum"])


# ---- c. nothing behind a stream's end counts ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mono", [False, True], ids=["stereo", "mono"])
@pytest.mark.parametrize("name", list(E.ENDS))
def test_poison_behind_the_ends_changes_nothing(M, name, mono):  # noqa: F811
    x = E.batch()
    f = np.array(E.ENDS[name], np.uint64)
    for period in (0, P):
        clean = E.through(M, x, [(N, f)], period, mode=BS.BLOCK, mono=mono, pad=7)
        nan = E.through(M, x, [(N, f)], period, mode=BS.BLOCK, mono=mono, pad=7, poison=True)
        assert E.same_result(clean, nan), (name, period)
        assert np.isfinite(nan["spectrum"]["val"]).all() and np.isfinite(nan["spectrum"]["max"]).all()


# ---- d. silence: the dither's and the epilogues' levels alone -----------------------------------------------------------------------------

@pytest.mark.parametrize("period", [P, 0])
def test_silence(M, oracle, period):  # noqa: F811
    """Levels of about 7e-20: one epilogue (+ 1e-20f) too many or too few — at r = 0 (stream 2 ends with block 0) or r = 1 (stream 3) —
    or a dither parity that is off is a deviation of the order of the value itself."""
    zero = np.zeros((S, N, 2), np.float32)
    ends = E.ENDS["early"]
    assert ends[2] % P == 0 and ends[3] % P == 1
    got = E.through(M, zero, [(N, np.array(ends, np.uint64))], period, speed=None)
    held(M, oracle, zero, got, ends, period, BS.HOLD, False, "silence P=%d" % period, calls=[N], speed=None, tag="silence")
    v = got["spectrum"]["val"]
    assert (v >= TINY).all() and (v < 2e-19).all() and (got["spectrum"]["val_db"] == -100.0).all()
    if period:                                                   # r = 0: ONE epilogue at frame 100, whose point is the stream's level
        assert np.array_equal(BS.bits(got["series"]["val"][2, 0]), BS.bits(v[2])) and got["points"][2] == 1 and got["points"][3] == 2


# ---- e. later calls -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("period", [P, 0])
def test_later_dense_calls_leave_closed_streams_alone(M, oracle, period):  # noqa: F811
    """mtr_engine_process_device twice behind the closing call: the closed streams stay bit for bit, series rows and counts included; the
    open one advances as an engine that never heard of ends"""
    T = N + 300
    x = E.batch(T)
    ends = E.ENDS["mixed"]
    f = np.array(ends, np.uint64)
    mode = BS.BLOCK if period else BS.HOLD
    closing = E.through(M, x, [(N, f)], period, mode=mode, pad=7)
    later = E.through(M, x, [(N, f), (100, None), (200, None)], period, mode=mode, pad=7)
    assert later["closed"].tolist() == closing["closed"].tolist() and later["frames"].tolist() == [v if v < N else T for v in ends]
    totals = [v if v < N else T for v in ends]
    held(M, oracle, x, later, totals, period, mode, False, "later calls P=%d" % period, calls=[N, 100, 200], tag="noise of %d frames" % T)
    for s in range(S):
        if ends[s] < N:
            assert BS.same(row(later["spectrum"], s), row(closing["spectrum"], s)) and later["points"][s] == closing["points"][s], s
            if period:
                assert BS.same(row(later["series"], s, 0, N // P), row(closing["series"], s)), s
    if period:
        assert later["n_points"] == T // P


@pytest.mark.parametrize("tag", ["noise", "silence"])
def test_blob_continuation(M, tag):  # noqa: F811
    """P = 0.  The closing call, three dense calls (an odd number of swaps of the parity's two buffers), export; a fresh engine imports and
    gets 300 frames: every stream comes out bit for bit as an engine fed its own frames and then those 300 — the levels and, in the
    state blob, the filters' states in double and the parity itself, which a parity that is lost, not carried across the swaps, or computed
    from n_frames does not survive (ends 129, 257, 99: odd; n_frames 600: even).  (The levels alone would not show it: the dither is
    1e-12 of full scale.)"""
    later, more = [64, 1, 63], 300
    T = N + sum(later)
    x = E.batch(T) if tag == "noise" else np.zeros((S, T, 2), np.float32)
    y = E.batch(more, first=S) if tag == "noise" else np.zeros((S, more, 2), np.float32)
    speed = B.SPEED if tag == "noise" else None
    ends = E.ENDS["mixed"]
    a = E.through(M, x, [(N, np.array(ends, np.uint64))] + [(n, None) for n in later], 0, speed=speed, pad=1)
    with M.Engine(S, E.FS, M.METER_SPECTR30) as e:
        if speed is not None:
            e.spectr_set_speed(speed)
        e.state_import(a["blob"])
        assert BS.same(e.spectrum(), a["spectrum"]) and not e.stream_frames()[1].any()
        e.process(y)
        got = e.spectrum()
        blobs = [e.state_export(s, 1) for s in range(S)]
    for s in range(S):
        own = ends[s] if ends[s] < N else T
        cuts = E.cuts_of(own, 0, [N] + later) + [more]
        _, fin, blob = E.yard(M, np.concatenate([x[s, :own], y[s]]), cuts, speed=speed, blob=True)
        assert BS.same(row(got, s), fin), (tag, s, own)
        assert len(blobs[s]) == len(blob) and blobs[s][-E.BANK_BLOB_BYTES:] == blob[-E.BANK_BLOB_BYTES:], (tag, s, own, "z, val, max or the parity in the blob")


# ---- f. the routes ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mono", [False, True], ids=["stereo", "mono"])
def test_host_path_in_three_views_equals_the_device_path(M, mono):  # noqa: F811
    """mtr_engine_set_host_chunk_bytes for two streams per view: views {0, 1}, {2, 3}, {4} — each view's kernel reads its own streams' ends"""
    x = E.batch()
    for name, ends in E.ENDS.items():
        f = np.array(ends, np.uint64)
        for period in (0, P):
            dev = E.through(M, x, [(250, None), (350, np.minimum(f, 350))], period, mode=BS.BLOCK, mono=mono)
            host = E.through(M, x, [(250, None), (350, np.minimum(f, 350))], period, mode=BS.BLOCK, mono=mono, host=True, chunk_streams=2)
            assert E.same_result(dev, host), (name, period)


def test_combined_engine(M):  # noqa: F811
    """EBU | TRUEPEAK | SPECTR30 through _ends: the loudness and true-peak results of an EBU | TRUEPEAK engine through _lengths, the
    bank's of a SPECTR30 engine through _ends"""
    import torch
    n = 6000                                                     # two and a half fragments
    x = E.batch(n)
    f = np.array([n, 2500, 0, 4801, 99], np.uint64)
    d = torch.from_numpy(x).cuda()
    res = {}
    for key, meters in (("all", M.METER_EBU | M.METER_TRUEPEAK | M.METER_SPECTR30), ("fused", M.METER_EBU | M.METER_TRUEPEAK), ("bank", M.METER_SPECTR30)):
        with M.Engine(S, E.FS, meters) as e:
            if meters & M.METER_SPECTR30:
                e.spectr_set_speed(B.SPEED)
                e.spectr_set_period(1000, 8, BS.BLOCK)
            if meters & M.METER_EBU:
                e.integr_start()
            (e.process_device_lengths if key == "fused" else e.process_device_ends)(d.data_ptr(), n, f)
            res[key] = dict(frames=e.stream_frames()[0].tolist())
            if meters & M.METER_EBU:
                res[key].update(out9=e.out9(), tp=e.truepeak(), hist=e.histograms())
            if meters & M.METER_SPECTR30:
                res[key].update(spectrum=e.spectrum(), series=e.spectr_series(), points=e.spectr_points().tolist())
    del d
    a, fu, bk = res["all"], res["fused"], res["bank"]
    assert a["frames"] == fu["frames"] == bk["frames"] == f.tolist()
    assert np.array_equal(BS.bits(a["out9"]), BS.bits(fu["out9"])) and np.array_equal(BS.bits(a["tp"]), BS.bits(fu["tp"]))
    assert np.array_equal(a["hist"][0], fu["hist"][0]) and np.array_equal(a["hist"][1], fu["hist"][1])
    assert BS.same(a["spectrum"], bk["spectrum"]) and BS.same(a["series"][0], bk["series"][0]) and a["series"][1:] == bk["series"][1:]
    assert a["points"] == bk["points"] == [6, 3, 0, 5, 1]


def test_a_mask_that_ragged_accepts_gives_raggeds_snapshot(M):  # noqa: F811
    import torch
    n = 6000
    x = E.batch(n)
    f = np.array([n, 2500, 0, 4801, 99], np.uint64)
    d = torch.from_numpy(x).cuda()
    snaps = []
    for name in ("ragged", "ends"):
        with M.Engine(S, E.FS, M.METER_EBU | M.METER_KMETER | M.METER_STCORR | M.METER_DR14) as e:
            e.stcorr_set_period(2400, 4)
            getattr(e, "process_device_" + name)(d.data_ptr(), n, f)
            e.process_device(d.data_ptr(), 1000, n)
            snaps.append((e.state_export(), e.stream_frames()[0].tolist(), e.stream_frames()[1].tolist(), e.series_points(M.METER_STCORR).tolist(),
                          e.stcorr_series()[0].tobytes()))
    del d
    assert snaps[0] == snaps[1]


# ---- g. refusals ---------------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_engine_unchanged(M):  # noqa: F811
    import torch
    n = N
    st = np.ascontiguousarray(E.batch()[:4])
    f = np.array([n, 100, 0, n], np.uint64)
    for meters, chn in ((M.METER_TPBALLIST, 2), (M.METER_SURROUND, 5), (M.METER_SCOPE, 2), (M.METER_SPECTR30 | M.METER_TPBALLIST, 2), (M.METER_EBU, 5)):
        x = st if chn == 2 else np.ascontiguousarray(np.concatenate([st, st, st[:, :, :1]], axis=2))
        dev = torch.from_numpy(x).cuda()
        with M.Engine(4, E.FS, meters, n_channels=chn) as e:
            e.process_device(dev.data_ptr(), n)
            before = e.state_export()
            assert M.lib.mtr_engine_process_device_ends(e._h, dev.data_ptr(), n, n, f.ctypes.data, 0) == ERR_UNSUPPORTED, (meters, chn)
            assert M.lib.mtr_engine_process_host_ends(e._h, x.ctypes.data, n, n, f.ctypes.data) == ERR_UNSUPPORTED, (meters, chn)
            assert e.state_export() == before and not e.stream_frames()[1].any() and e.stream_frames()[0].tolist() == [n] * 4
        del dev
    dev = torch.from_numpy(st).cuda()
    out = np.zeros(4, np.uint64)
    for period in (0, P):
        with M.Engine(4, E.FS, M.METER_SPECTR30) as e:
            e.spectr_set_period(period, 8)
            e.process_device(dev.data_ptr(), n)
            before = e.state_export()
            big = np.array([n, 100, n + 1, n], np.uint64)
            assert M.lib.mtr_engine_process_device_ends(e._h, dev.data_ptr(), n, n, None, 0) == ERR_ARG
            assert M.lib.mtr_engine_process_device_ends(e._h, dev.data_ptr(), n, n, big.ctypes.data, 0) == ERR_ARG
            assert M.lib.mtr_engine_process_host_ends(e._h, st.ctypes.data, n, n, None) == ERR_ARG
            assert M.lib.mtr_engine_process_host_ends(e._h, st.ctypes.data, n, n, big.ctypes.data) == ERR_ARG
            # the ends on the device are 32 bits: refused before anything is read or queued
            huge = 0xFFFFFFFF
            assert M.lib.mtr_engine_process_device_ends(e._h, dev.data_ptr(), huge, huge, f.ctypes.data, 0) == ERR_ARG
            assert M.lib.mtr_engine_process_host_ends(e._h, st.ctypes.data, huge, huge, f.ctypes.data) == ERR_ARG
            assert M.lib.mtr_engine_spectr_points(e._h, 0, 4, None) == ERR_ARG
            assert M.lib.mtr_engine_spectr_points(e._h, 2, 3, out.ctypes.data) == ERR_ARG
            assert M.lib.mtr_engine_spectr_points(e._h, 0, 4, out.ctypes.data) == 0 and out.tolist() == [n // period if period else 0] * 4
            assert e.state_export() == before and not e.stream_frames()[1].any() and e.stream_frames()[0].tolist() == [n] * 4
            e.reset()
            assert M.lib.mtr_engine_spectr_points(e._h, 0, 4, out.ctypes.data) == 0 and not out.any()
            # ... and once a stream is closed every call runs the kernels that read them: the same bound for the plain calls
            e.process_device_ends(dev.data_ptr(), n, f)
            before, frames = e.state_export(), e.stream_frames()
            assert frames[1].tolist() == [False, True, True, False]
            assert M.lib.mtr_engine_process_device(e._h, dev.data_ptr(), huge, huge, 0) == ERR_ARG
            assert M.lib.mtr_engine_process_host(e._h, st.ctypes.data, huge, huge) == ERR_ARG
            assert e.state_export() == before and e.stream_frames()[0].tolist() == frames[0].tolist()
    del dev
    with M.Engine(4, E.FS, M.METER_KMETER) as e:                 # no SPECTR30 in the engine
        assert M.lib.mtr_engine_spectr_points(e._h, 0, 4, out.ctypes.data) == ERR_ARG
    assert M.lib.mtr_engine_spectr_points(None, 0, 0, out.ctypes.data) == ERR_ARG
