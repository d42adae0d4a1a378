"""The gate kernels (mtr_gate.hip: k_gate, k_gate_frag, k_gate_final, each x LEN x LOG) held to the engine's own inputs, with no bin-flip
allowance.

The gate is written to be exact given its inputs, so it is checked against tests/_gate.py (anchored to the oracle by
tests/test_gate_model_cpu.py) on what the engine's own getters say those inputs were: mtr_engine_fragment_powers gives a call's fragment
powers, the loudness log at P = 1, MTR_LOUDLOG_SAMPLE, the gate's own (M, S) of every fragment.  check (), for every stream after every
call:
  1. the (M, S) series equals the model driven by that call's fragment powers: every deviation <= ULP_DB = 3.8e-5 dB, values that are
     not bit-equal fewer than 1 in 1000 (kernel and model both round a double log10);
  2. the bookkeeping model driven by the GPU's own (M, S) series: both histograms bin for bin, both counts, max M / max S and M / S bit
     for bit the series' maximum so far and its last value;
  3. I, I_thr, Rmin, Rmax, R_thr against hist_loudness of the model's histograms as they stood at the last fragment at which div2 wrapped:
     Rmin and Rmax bit for bit, the others within ULP_DB.  Where the floorf argument g of a gate bin lies within 1e-3 of an integer the
     two log10 routes may pick neighbouring bins: that evaluation is skipped and counted, at most 2 % of the file's evaluations (the
     width gives an expected share of 0.2 %);
  4. integr off: counts, histograms and dividers stand still — the next insert lands where the model puts it.
The programmes (tests/_gate.py) reach the gate's edges; assert_coverage holds that on the GPU's own histograms.

Measured on an MI355X over the whole file (every check prints its own counts and the file's so far): 0 of 130 302 (M, S) values not
bit-equal to the model, largest deviation 0 dB; 1 of 574 evaluations skipped (in test_lengths).

The tests were themselves tested against three wrong-on-purpose builds of mtr_gate.hip: `i = base + l` for `base + l + 1` in
hist_calc_range's percentile walk (test_short_calls, test_long_call, test_lengths and test_deferred_walk fail), hist_integrate without
its `divf_cr (s, 10.0f)` (the same four), and `f_abs < f_calc` for `<=` on k_gate's M insert (the same four).
"""
import numpy as np
import pytest
import torch

import _gate as G

pytestmark = pytest.mark.gpu
STATS = dict(values=0, not_bit_equal=0, worst=0.0, evaluations=0, skipped=0)      # over every check () of the file
CHECKED = set()                                                                    # the tags of the checks that ran
N_CHECKS = 8
_RUNS = {}
FIELDS = ("out9", "counts", "hist_M", "hist_S", "frag")


@pytest.fixture(scope="module")
def M():
    import meters.lv2_amd as m
    return m


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def run(M, x, ends, fs=G.FS, meters=None, log=True, integr=None, frames=None, tail=None, every_call=True):
    """x [S, T, 2] through one engine in calls that end at the frames `ends`; integr [call]: whether the integration runs during the call
    (default: always); frames [call][S]: per-stream lengths (process_device_lengths).  -> ([record per call], state blob, deferred calls)"""
    S, T = x.shape[:2]
    frag = int(fs) // 20
    dev = torch.from_numpy(np.array(x)).cuda()
    recs, on, a = [], False, 0
    with M.Engine(S, fs, M.METER_EBU if meters is None else meters) as e:
        if tail is not None:
            e.set_deferred_tail(tail)
        if log:
            e.loudlog_set_period(1, T // frag + 1, M.LOUDLOG_SAMPLE)
        for c, b in enumerate(ends):
            want = True if integr is None else integr[c]
            if want != on:
                (e.integr_start if want else e.integr_pause)()
                on = want
            if frames is None:
                e.process_device(dev.data_ptr() + a * 8, b - a, T)
            else:
                e.process_device_lengths(dev.data_ptr() + a * 8, b - a, frames[c], T)
            a = b
            if every_call or c == len(ends) - 1:
                res = e.results()
                r = dict(out9=e.out9(), counts=np.array([[v.hist_M_count, v.hist_S_count] for v in res]), frag=e.fragment_powers().copy())
                r["hist_M"], r["hist_S"] = e.histograms()
                if log:
                    r["M"], r["S"], r["n"], r["d"] = e.loudlog_series()
                recs.append(r)
        blob, nd = e.state_export(), e.deferred_calls()
    del dev
    return recs, blob, nd


def near_edge(g):
    """the floorf argument of a gate bin within 1e-3 of an integer (NaN: there is no gate bin)"""
    return g == g and abs(g - np.round(g)) < 1e-3


def check(recs, integr=None, lengths=False, tag=""):
    """the common check; -> [final model record per stream]"""
    S = recs[0]["out9"].shape[0]
    st = dict(values=0, not_bit_equal=0, worst=0.0, evaluations=0, skipped=0)
    finals = []
    for s in range(S):
        by_power, by_series, done, last = G.Gate(), G.Gate(), 0, None
        for c, r in enumerate(recs):
            on = True if integr is None else integr[c]
            now = int(r["n"][s])
            nf = now - done
            assert r["d"][s] == 0 and nf >= 0
            if not lengths:
                assert nf == r["frag"].shape[1], (s, c, nf, r["frag"].shape)
            Mg, Sg = r["M"][s, done:now], r["S"][s, done:now]
            assert np.isnan(r["M"][s, now:]).all()
            done = now
            # 1. the series against the model driven by the call's fragment powers
            a = by_power.call_powers(r["frag"][s, :nf], on)
            dev = max(np.abs(a["M"].astype(np.float64) - Mg).max(initial=0), np.abs(a["S"].astype(np.float64) - Sg).max(initial=0))
            st["worst"] = max(st["worst"], float(dev))
            assert dev <= G.ULP_DB, (tag, s, c, dev)
            st["values"] += 2 * nf
            st["not_bit_equal"] += int((_bits(a["M"]) != _bits(Mg)).sum() + (_bits(a["S"]) != _bits(Sg)).sum())
            # 2. the bookkeeping on the GPU's own series
            b = last = by_series.call_ms(Mg, Sg, on)
            assert np.array_equal(r["hist_M"][s], b["hist_M"]), (tag, s, c, np.flatnonzero(r["hist_M"][s] != b["hist_M"]))
            assert np.array_equal(r["hist_S"][s], b["hist_S"]), (tag, s, c, np.flatnonzero(r["hist_S"][s] != b["hist_S"]))
            assert tuple(r["counts"][s]) == tuple(b["count"]), (tag, s, c, r["counts"][s], b["count"])
            o = r["out9"][s]
            assert _same(o[:4], [b["last_M"], b["max_M"], b["last_S"], b["max_S"]]), (tag, s, c, o[:4], b["last_M"], b["max_M"], b["last_S"], b["max_S"])
            # 3. what calc_integ / calc_range made of the histograms at the last wrap
            e = G.expected(b["snap_M"], b["snap_S"])
            st["evaluations"] += 2 * b["evaluated"]
            assert abs(float(o[5]) - float(e["I_thr"])) <= G.ULP_DB and abs(float(o[8]) - float(e["R_thr"])) <= G.ULP_DB, (tag, s, c, o, e)
            if near_edge(e["g_I"]):
                st["skipped"] += b["evaluated"]
            else:
                assert abs(float(o[4]) - float(e["I"])) <= G.ULP_DB, (tag, s, c, o, e)
            if near_edge(e["g_R"]):
                st["skipped"] += b["evaluated"]
            else:
                assert _same(o[6:8], [e["Rmin"], e["Rmax"]]), (tag, s, c, o, e)
        finals.append(last)
    print(f"\n{tag}: {st['not_bit_equal']} of {st['values']} (M, S) values not bit-equal to the model, largest deviation {st['worst']:.2e} dB; "
          f"{st['skipped']} of {st['evaluations']} evaluations skipped (gate bin within 1e-3 of an edge)")
    assert st["not_bit_equal"] * 1000 < max(st["values"], 1000), st
    for k in st:
        STATS[k] = max(STATS[k], st[k]) if k == "worst" else STATS[k] + st[k]
    CHECKED.add(tag)
    print(f"the file so far: {STATS['not_bit_equal']} of {STATS['values']} values not bit-equal, largest deviation {STATS['worst']:.2e} dB; "
          f"{STATS['skipped']} of {STATS['evaluations']} evaluations skipped")
    return finals


def same_records(a, b, fields=FIELDS, what=""):
    for k in fields:
        assert a[k].shape == b[k].shape and (_same(a[k], b[k]) if a[k].dtype == np.float32 else np.array_equal(a[k], b[k])), (what, k)


def short_run(M, log=True):
    if ("short", log) not in _RUNS:
        x = G.batch()
        _RUNS["short", log] = run(M, x, G.call_ends(x.shape[1]), log=log)[0]
    return _RUNS["short", log]


# ---- the dense k_gate <*, LOG> -----------------------------------------------------------------------------------------------------

def test_short_calls(M):
    recs = short_run(M)
    finals = check(recs, tag="short calls")
    rec = {}
    for s, nm in enumerate(G.NAMES):
        o = recs[-1]["out9"][s]
        rec[nm] = dict(hist_M=recs[-1]["hist_M"][s], hist_S=recs[-1]["hist_S"][s], count=recs[-1]["counts"][s], wraps=finals[s]["wraps"],
                       I_thr=o[5], R_thr=o[8], Rmin=o[6], Rmax=o[7])
        assert tuple(finals[s]["wraps"]) == (G.NFRAG // 2, G.NFRAG // 10)
    rec["late"]["counts_per_call"] = [tuple(r["counts"][G.NAMES.index("late")]) for r in recs]
    G.assert_coverage(rec)
    # the same audio with the integration paused over calls 4 - 5, every other stream
    x = G.batch()[::2]
    ends = G.call_ends(x.shape[1])
    integr = [c not in (4, 5) for c in range(len(ends))]
    paused = run(M, x, ends, integr=integr)[0]
    finals = check(paused, integr=integr, tag="short calls, integration paused over calls 4 - 5")
    assert all(tuple(f["wraps"]) == ((G.NFRAG - 14) // 2, (G.NFRAG - 14) // 10) for f in finals)
    for c in (4, 5):                                   # (and directly: nothing of the record but M, S and their maxima moved)
        assert np.array_equal(paused[c]["hist_M"], paused[3]["hist_M"]) and np.array_equal(paused[c]["hist_S"], paused[3]["hist_S"])
        assert np.array_equal(paused[c]["counts"], paused[3]["counts"]) and _same(paused[c]["out9"][:, 4:], paused[3]["out9"][:, 4:])


def test_log_off_is_the_same_record(M):
    on, off = short_run(M), short_run(M, log=False)
    assert len(on) == len(off)
    for c, (a, b) in enumerate(zip(on, off)):
        same_records(a, b, what=c)


# ---- k_gate_frag + k_gate_final -----------------------------------------------------------------------------------------------------

LONG = ("fuzz0", "up", "over")
LONG_FRAGS = 7 + 4107 + 13


def test_long_call(M):
    x = G.batch(LONG, LONG_FRAGS)
    T = x.shape[1]
    small = run(M, x, [k * 100 * G.FRAG for k in range(1, LONG_FRAGS // 100 + 1)] + [T], every_call=False)[0][-1]
    for cuts in ([7 * G.FRAG + 211, (7 + 4107) * G.FRAG + 133, T], [4096 * G.FRAG + 189, T]):
        recs = run(M, x, cuts)[0]
        assert recs[-2]["frag"].shape[1] >= 4096                                  # (the call went the long way)
        check(recs, tag="long call %s" % [b // G.FRAG for b in cuts])
        off = run(M, x, cuts, log=False)[0]
        for c, (a, b) in enumerate(zip(recs, off)):
            same_records(a, b, what=("log off", cuts, c))
        # (the record, not the series: the K-weighting kernels sum a fragment's power in the order the call's cuts give them, so single
        # fragment powers — the gate's inputs, point 1 above — may differ in their last bit between two cuttings)
        same_records(recs[-1], small, ("out9", "counts", "hist_M", "hist_S", "n"), what=("calls of 100 fragments", cuts))


# ---- the LEN kernels ------------------------------------------------------------------------------------------------------------------

def test_lengths(M):
    names = ("up", "fuzz0", "over", "steady", "fuzz1", "floor", "fuzz2", "gate_i")
    x = G.batch(names, 220)
    n = 40 * G.FRAG + 150                                # the first two calls: 40 fragments and 150 frames each
    T = x.shape[1]
    # ends: with the call (open) / inside fragment 17 / on a fragment boundary / at 0 frames (untouched) / in the second call / before
    # ten fragments (no wrap ever) / one frame before the call's end / open
    first = np.array([n, 17 * G.FRAG + 123, 20 * G.FRAG, 0, n, 7 * G.FRAG + 50, n - 1, n], np.uint64)
    second = np.array([n, 0, 0, 0, 5 * G.FRAG + 77, 0, 0, n], np.uint64)
    # 80 fragments hold 40 M points and 8 S points: under the 50 / 20 minima, calc_* would never get past its first line.  So a third
    # call of 140 fragments, which stream 7 leaves after 100: stream 0 ends with 110 M points and 22 S points, I and the range valid
    third = np.array([T - 2 * n, 0, 0, 0, 0, 0, 0, 100 * G.FRAG + 31], np.uint64)
    frames = [first, second, third]
    recs = run(M, x, [n, 2 * n, T], frames=frames)[0]
    assert [int(v) for v in recs[0]["n"]] == [40, 17, 20, 0, 40, 7, 40, 40]
    assert [int(v) for v in recs[1]["n"]] == [80, 17, 20, 0, 45, 7, 40, 80]
    assert [int(v) for v in recs[2]["n"]] == [220, 17, 20, 0, 45, 7, 40, 180]
    check(recs, lengths=True, tag="lengths")
    assert (recs[2]["out9"][0, 4:] > -200.0).all() and recs[2]["out9"][7, 4] > -200.0
    for s, c0 in ((1, 0), (2, 0), (3, 0), (5, 0), (6, 0), (4, 1)):      # a closed stream's record does not move in later calls
        for c in range(c0 + 1, 3):
            for k in ("out9", "counts", "hist_M", "hist_S"):
                assert _same(recs[c0][k][s], recs[c][k][s]) if k == "out9" else np.array_equal(recs[c0][k][s], recs[c][k][s]), (s, c, k)
    assert (recs[2]["out9"][3] == -200.0).all() and not recs[2]["hist_M"][3].any() and not recs[2]["hist_S"][3].any()
    assert (recs[2]["out9"][5, 4:] == -200.0).all() and recs[2]["counts"][5, 1] == 0
    off = run(M, x, [n, 2 * n, T], frames=frames, log=False)[0]
    for c in range(3):
        same_records(recs[c], off[c], ("out9", "counts", "hist_M", "hist_S"), what=("log off", c))
    # the long path: ends at the call's end / inside fragment 3000 / at 0 frames
    x = G.batch(LONG, 4200, tail=0)
    T = x.shape[1]
    frames = [np.array([T, 3000 * G.FRAG + 5, 0], np.uint64)]
    recs = run(M, x, [T], frames=frames)[0]
    assert [int(v) for v in recs[0]["n"]] == [4200, 3000, 0]
    check(recs, lengths=True, tag="lengths, long path")
    off = run(M, x, [T], frames=frames, log=False)[0]
    same_records(recs[0], off[0], ("out9", "counts", "hist_M", "hist_S"), what="long path, log off")


# ---- the deferred gate: a workgroup walks several streams ------------------------------------------------------------------------------

def test_deferred_walk(M, monkeypatch):
    monkeypatch.setenv("MTR_TAIL_GATE_GRID", "3")        # read by mtr_engine_create (include/mtr_engine.h): 11 streams over 3 workgroups
    x = G.batch()[:11]
    ends = G.call_ends(x.shape[1])
    serial, blob1, nd1 = run(M, x, ends, tail=1)
    check(serial, tag="the serial run of the deferred walk's batch")
    walked, blob2, nd2 = run(M, x, ends, tail=2, every_call=False)     # (no getter between the calls: the gates queue up)
    assert nd1 == 0 and nd2 == len(ends)
    same_records(walked[-1], serial[-1], ("out9", "counts", "hist_M", "hist_S", "M", "S", "n", "d"), what="deferred")
    assert blob1 == blob2


# ---- the route the batch kernels feed -----------------------------------------------------------------------------------------------

def test_48k_with_truepeak(M):
    names = ("fuzz0", "fuzz1", "fuzz2", "floor", "steady", "zeros")
    x = G.batch(names, 60, frag=2400, fs=48000.0)
    recs = run(M, x, [5000, 5001, 7400, x.shape[1]], fs=48000.0, meters=M.METER_EBU | M.METER_TRUEPEAK)[0]
    check(recs, tag="48 kHz with true peak")


def test_skipped_share_of_the_file():
    """(last) skipped evaluations are at most 2 % of all evaluations in the file; a run of single tests only prints its own"""
    print(f"\n{len(CHECKED)} of {N_CHECKS} checks ran: {STATS['skipped']} of {STATS['evaluations']} evaluations skipped, "
          f"{STATS['not_bit_equal']} of {STATS['values']} (M, S) values not bit-equal")
    if len(CHECKED) == N_CHECKS:
        assert STATS["skipped"] * 50 <= STATS["evaluations"], STATS
        assert STATS["not_bit_equal"] * 1000 < STATS["values"], STATS
