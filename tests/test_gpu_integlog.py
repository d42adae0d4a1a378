"""The integration log (mtr_engine_integlog_*: integrated, integ_thr, range_min, range_max, range_thr per K evaluations and stream; the
EVAL instantiations of k_gate, mtr_gate.hip) on the GPU, every point held to tests/_gate.py.

The yardstick for a point: the loudness log runs beside the new log at P = 1, MTR_LOUDLOG_SAMPLE (so the LOG x EVAL instantiations are
under test), which gives the gate's own (M, S) of every fragment.  Per stream, _gate.Gate.call_ms is fed that series in slices that end at
each evaluation — the fragments at which its div2 wraps while the integration runs — and _gate.expected (snap_M, snap_S) of the
histograms as they stand there is what the point must be.  The bounds are those of tests/test_gpu_gate_exact.py item 3: Rmin and Rmax bit
for bit, I, I_thr and R_thr within _gate.ULP_DB (the oracle rounds glibc's log10f, kernel and model a double log10); an evaluation whose
gate-bin argument lies within 1e-3 of an integer is skipped and counted, at most 2 % of the file's evaluations (test_skipped_share_of_the_file;
the reference fed ten fragments at a time gives 8 of 3060 for _gate.batch () and 1 of 352 for the batch of test_lengths).

The programmes are _gate's 997 Hz sines at 8 kHz, fragments of 400 frames.  Every check prints its own counts and the file's so far.
"""
import numpy as np
import pytest
import torch

import _gate as G

pytestmark = pytest.mark.gpu
STATS = dict(evaluations=0, skipped=0)                # over every hold () of the file
CHECKED = set()
N_CHECKS = 10
FIELDS = ("I", "I_thr", "Rmin", "Rmax", "R_thr")
LONG = ("fuzz0", "up", "over")
GUARD, SENTINEL = 4, np.float32(12345.0)
_RUNS = {}


@pytest.fixture(scope="module")
def M():
    import meters.lv2_amd as m
    return m


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and (np.array_equal(_bits(a), _bits(b)) if a.dtype == np.float32 else np.array_equal(a, b))


def run(M, x, ends, fs=G.FS, meters=None, K=1, cap=None, integr=None, reset_before=None, frames=None, tail=None, every_call=True,
        host=False, guard=False):
    """x [S, T, 2] through one engine in calls that end at the frames `ends`, the loudness log at P = 1 and the integration log at K
    (0: off) with `cap` points; integr [call]: whether the integration runs during the call (default: always); reset_before: the call in
    front of which integr_reset is called; frames [call][S]: per-stream lengths; host: through Engine.process in chunks of three streams.
    -> ([record per call], state blob, deferred calls)"""
    S, T = x.shape[:2]
    frag = int(fs) // 20
    cap = T // frag // 10 + 1 if cap is None else cap
    dev = None if host else torch.from_numpy(np.array(x)).cuda()
    recs, on, a = [], False, 0
    with M.Engine(S, fs, M.METER_EBU if meters is None else meters) as e:
        if tail is not None:
            e.set_deferred_tail(tail)
        e.loudlog_set_period(1, T // frag + 1, M.LOUDLOG_SAMPLE)
        if K:
            e.integlog_set_every(K, cap)
            assert e.integlog_every() == (K, cap)
        for c, b in enumerate(ends):
            want = True if integr is None else integr[c]
            if want != on:
                (e.integr_start if want else e.integr_pause)()
                on = want
            if c == reset_before:
                e.integr_reset()
            if host:
                e.set_host_chunk_bytes(3 * (b - a) * 8)
                e.process(x[:, a:b])
            elif frames is None:
                e.process_device(dev.data_ptr() + a * 8, b - a, T)
            else:
                e.process_device_lengths(dev.data_ptr() + a * 8, b - a, frames[c], T)
            a = b
            if every_call or c == len(ends) - 1:
                res = e.results()
                r = dict(out9=e.out9(), counts=np.array([[v.hist_M_count, v.hist_S_count] for v in res]), frag=e.fragment_powers().copy())
                r["hist_M"], r["hist_S"] = e.histograms()
                r["M"], r["S"], r["n"], r["d"] = e.loudlog_series()
                if K:
                    r["il"] = e.integlog_series()
                recs.append(r)
        if guard:                                       # rows wider than the capacity, straight through the C entry point
            wide = [np.full((S, cap + GUARD), SENTINEL, np.float32) for _ in FIELDS]
            assert M.lib.mtr_engine_integlog_series(e._h, 0, S, *[w.ctypes.data for w in wide], cap + GUARD, None, None) == 0
            recs[-1]["wide"] = dict(zip(FIELDS, wide))
        blob, nd = e.state_export(), e.deferred_calls()
    del dev
    return recs, blob, nd


def yardstick(recs, integr=None, reset_before=None):
    """[stream][evaluation] = _gate.expected of the model's histograms at that evaluation, the model fed the GPU's own (M, S) series in
    slices that end at each evaluation"""
    out = []
    for s in range(recs[0]["out9"].shape[0]):
        g, done, exp = G.Gate(), 0, []
        for c, r in enumerate(recs):
            if c == reset_before:
                g = G.Gate()                            # integr_reset: histograms, counts and dividers to zero (ebu_r128_proc.cc:192-204)
            now = int(r["n"][s])
            assert r["d"][s] == 0 and now >= done
            Mg, Sg = r["M"][s, done:now], r["S"][s, done:now]
            done = now
            if integr is not None and not integr[c]:
                g.call_ms(Mg, Sg, False)
                continue
            a = 0
            while a < Mg.size:
                need = 10 - g.div2
                b = min(a + need, Mg.size)
                m = g.call_ms(Mg[a:b], Sg[a:b], True)
                if b - a == need:
                    assert m["evaluated"] and g.div2 == 0
                    exp.append(G.expected(m["snap_M"], m["snap_S"]))
                a = b
        out.append(exp)
    return out


def near_edge(g):
    """the floorf argument of a gate bin within 1e-3 of an integer (NaN: there is no gate bin)"""
    return g == g and abs(g - np.round(g)) < 1e-3


def hold(il, exps, K=1, tag=""):
    """every point the series holds against the yardstick's evaluation (j + 1) K"""
    st = dict(evaluations=0, skipped=0)
    cap = il["I"].shape[1]
    for s, exp in enumerate(exps):
        n = int(il["n_points"][s])
        assert n == len(exp) // K and int(il["dropped"][s]) == max(n - cap, 0), (tag, s, n, len(exp))
        kept = min(n, cap)
        for j in range(kept):
            e = exp[(j + 1) * K - 1]
            got = {f: il[f][s, j] for f in FIELDS}
            st["evaluations"] += 2
            assert abs(float(got["I_thr"]) - float(e["I_thr"])) <= G.ULP_DB and abs(float(got["R_thr"]) - float(e["R_thr"])) <= G.ULP_DB, (tag, s, j, got, e)
            if near_edge(e["g_I"]):
                st["skipped"] += 1
            else:
                assert abs(float(got["I"]) - float(e["I"])) <= G.ULP_DB, (tag, s, j, got, e)
            if near_edge(e["g_R"]):
                st["skipped"] += 1
            else:
                assert _same([got["Rmin"], got["Rmax"]], [e["Rmin"], e["Rmax"]]), (tag, s, j, got, e)
        for f in FIELDS:                                # rows behind a stream's points are NaN
            assert np.isnan(il[f][s, kept:]).all() and not np.isnan(il[f][s, :kept]).any(), (tag, s, f)
    print(f"\n{tag}: {st['skipped']} of {st['evaluations']} evaluations skipped (gate bin within 1e-3 of an edge)")
    for k in st:
        STATS[k] += st[k]
    CHECKED.add(tag)
    print(f"the file so far: {STATS['skipped']} of {STATS['evaluations']} evaluations skipped")


def same_series(a, b, what=""):
    for f in FIELDS + ("n_points", "dropped"):
        assert _same(a[f], b[f]), (what, f)


def short_run(M, K=1):
    if ("short", K) not in _RUNS:
        x = G.batch()
        _RUNS["short", K] = run(M, x, G.call_ends(x.shape[1]), K=K, cap=20 if K == 3 else None, guard=K == 3)[0]
    return _RUNS["short", K]


# ---- 1. short calls ---------------------------------------------------------------------------------------------------------------------

def test_short_calls(M):
    recs = short_run(M)
    il = recs[-1]["il"]
    assert il["I"].shape == (len(G.NAMES), G.NFRAG // 10 + 1)
    assert (il["n_points"] == G.NFRAG // 10).all() and not il["dropped"].any()
    hold(il, yardstick(recs), tag="short calls")
    z = G.NAMES.index("zeros")
    for f in FIELDS:
        assert (il[f][z, :G.NFRAG // 10] == np.float32(-200)).all(), f
    s = G.NAMES.index("steady")                         # (and something was measured: -23 LUFS, a range of nothing)
    assert abs(il["I"][s, 84] + 23.0) < 0.1 and il["Rmax"][s, 84] - il["Rmin"][s, 84] < 0.5 and il["I"][s, 8] == -200.0 and il["I"][s, 9] > -30.0


# ---- 2. the call's last evaluation is the getters'; the log off is the same record ---------------------------------------------------

def test_last_point_is_the_getters_and_log_off_is_the_same_record(M):
    on, off = short_run(M), short_run(M, K=0)
    assert len(on) == len(off)
    before = np.zeros(len(G.NAMES), np.uint32)
    evaluated = 0
    for c, (a, b) in enumerate(zip(on, off)):
        il = a["il"]
        for s in np.flatnonzero(il["n_points"] > before):
            assert _same([il[f][s, il["n_points"][s] - 1] for f in FIELDS], a["out9"][s, 4:9]), (c, s)
            evaluated += 1
        before = il["n_points"].copy()
        for k in ("out9", "counts", "hist_M", "hist_S", "frag", "M", "S", "n", "d"):
            assert _same(a[k], b[k]), (c, k)
    assert evaluated == 7 * len(G.NAMES)                # (the calls of 0, 1 and 3 fragments wrap nothing: div2 stands at 0, 1, .., 1 there)


# ---- 3. K and capacity --------------------------------------------------------------------------------------------------------------------

def test_every_third_and_capacity(M):
    one, three = short_run(M)[-1]["il"], short_run(M, K=3)
    il = three[-1]["il"]
    assert il["I"].shape[1] == 20 and (il["n_points"] == 28).all() and (il["dropped"] == 8).all()
    for f in FIELDS:
        assert _same(il[f], one[f][:, 2::3][:, :20]), f
        w = three[-1]["wide"][f]
        assert _same(w[:, :20], il[f]) and (w[:, 20:] == SENTINEL).all(), f      # the guard band beyond the capacity is untouched
    div2 = ev = pts = 0
    for c, r in enumerate(three):                       # integlog_cut predicts every stream's counts after every call
        nf = r["frag"].shape[1]
        e, p = M.integlog_cut(div2, ev, 3, nf)
        div2, ev, pts = (div2 + nf) % 10, ev + e, pts + p
        assert (r["il"]["n_points"] == pts).all() and (r["il"]["dropped"] == max(pts - 20, 0)).all(), (c, pts, r["il"]["n_points"])
    assert (ev, pts) == (85, 28)
    CHECKED.add("K = 3")


# ---- 4. controls ---------------------------------------------------------------------------------------------------------------------------

def test_pause_and_integr_reset(M):
    x = G.batch()[::2]
    ends = G.call_ends(x.shape[1])
    integr = [c not in (4, 5) for c in range(len(ends))]
    recs = run(M, x, ends, integr=integr)[0]
    for c in (4, 5):                                    # a paused integration makes no evaluations: no points
        same_series(recs[c]["il"], recs[3]["il"], what=("paused", c))
    assert (recs[3]["il"]["n_points"] == 2).all() and (recs[-1]["il"]["n_points"] == (G.NFRAG - 14) // 10).all()
    hold(recs[-1]["il"], yardstick(recs, integr=integr), tag="integration paused over calls 4 - 5")
    # integr_reset in front of call 7: 289 fragments lie behind it (28 evaluations, div2 = 9), 256 + 257 + 48 follow from div2 = 0
    recs = run(M, x, ends, reset_before=7)[0]
    assert (recs[6]["il"]["n_points"] == 28).all() and (recs[7]["il"]["n_points"] == 28 + 25).all()      # the count goes on
    assert (recs[-1]["il"]["n_points"] == 28 + (256 + 257 + 48) // 10).all()
    il = recs[-1]["il"]
    hold(il, yardstick(recs, reset_before=7), tag="integr_reset in front of call 7")
    s = G.NAMES[::2].index("steady")
    # ... and the points return to -200 until the minima are passed again: 50 M points after 100 fragments, 20 S points after 200
    assert il["I"][s, 27] > -30.0 and il["Rmin"][s, 27] > -30.0
    assert (il["I"][s, 28:37] == -200.0).all() and (il["I_thr"][s, 28:37] == -200.0).all() and il["I"][s, 37] > -30.0
    assert (il["Rmin"][s, 28:47] == -200.0).all() and (il["Rmax"][s, 28:47] == -200.0).all() and il["Rmin"][s, 47] > -30.0


def test_reset_and_errors(M):
    E = M.engine

    def code(f, *a):
        with pytest.raises(M.EngineError) as err:
            f(*a)
        return err.value.code
    x = G.batch(("steady", "up"), 60)
    T = x.shape[1]
    dev = torch.from_numpy(np.array(x)).cuda()
    with M.Engine(2, G.FS, M.METER_EBU) as e:
        assert e.integlog_every() == (0, 0) and code(e.integlog_series) == E.ERR_ARG          # off is the default
        assert code(e.integlog_set_every, (1 << 20) + 1, 8) == E.ERR_ARG
        e.integlog_set_every(1 << 20, 8)
        e.integlog_set_every(0, 8)
        assert e.integlog_every() == (0, 0) and code(e.integlog_series) == E.ERR_ARG
        e.integlog_set_every(2, 8)
        e.integr_start()
        e.process_device(dev.data_ptr(), T)
        a = e.integlog_series()
        assert (a["n_points"] == 3).all() and (a["I"][:, :3] == -200.0).all() and np.isnan(a["I"][:, 3:]).all()
        assert code(e.integlog_set_every, 1, 8) == E.ERR_STATE and code(e.integlog_set_every, 0, 0) == E.ERR_STATE
        assert e.integlog_every() == (2, 8)
        same_series(e.integlog_series(), a, what="a refused set_every")
        e.integlog_reset()                                                                     # empties the series, keeps K and the capacity
        b = e.integlog_series()
        assert not b["n_points"].any() and not b["dropped"].any() and all(np.isnan(b[f]).all() for f in FIELDS) and e.integlog_every() == (2, 8)
        e.process_device(dev.data_ptr(), T)                                                    # 120 fragments: 60 M points, I is there
        c = e.integlog_series()
        assert (c["n_points"] == 3).all() and (c["I"][:, 2] > -40.0).all() and _same(c["I"][:, 2], e.out9()[:, 4])
        e.integr_reset()                                                                       # ... does not touch the log
        same_series(e.integlog_series(), c, what="integr_reset")
        e.reset()                                                                              # ... which mtr_engine_reset empties
        assert not e.integlog_series()["n_points"].any() and e.integlog_every() == (2, 8)
        e.integlog_set_every(1, 4)                                                             # (nothing processed since reset)
    with M.Engine(2, G.FS, M.METER_TRUEPEAK) as e:
        assert code(e.integlog_set_every, 1, 8) == E.ERR_ARG


# ---- 5. per-stream lengths ---------------------------------------------------------------------------------------------------------------

def test_lengths(M):
    names = ("up", "fuzz0", "over", "steady", "fuzz1", "floor", "fuzz2", "gate_i")
    x = G.batch(names, 220)
    n = 40 * G.FRAG + 150                                # the first two calls: 40 fragments and 150 frames each
    T = x.shape[1]
    # ends: with the call (open) / inside fragment 17 / on a fragment boundary / at 0 frames (untouched) / in the second call / before
    # ten fragments (no wrap ever) / one frame before the call's end / open; the third call: stream 7 leaves after 100 fragments
    first = np.array([n, 17 * G.FRAG + 123, 20 * G.FRAG, 0, n, 7 * G.FRAG + 50, n - 1, n], np.uint64)
    second = np.array([n, 0, 0, 0, 5 * G.FRAG + 77, 0, 0, n], np.uint64)
    third = np.array([T - 2 * n, 0, 0, 0, 0, 0, 0, 100 * G.FRAG + 31], np.uint64)
    recs = run(M, x, [n, 2 * n, T], frames=[first, second, third])[0]
    assert [int(v) for v in recs[0]["il"]["n_points"]] == [4, 1, 2, 0, 4, 0, 4, 4]
    assert [int(v) for v in recs[1]["il"]["n_points"]] == [8, 1, 2, 0, 4, 0, 4, 8]
    assert [int(v) for v in recs[2]["il"]["n_points"]] == [22, 1, 2, 0, 4, 0, 4, 18]
    hold(recs[2]["il"], yardstick(recs), tag="lengths")
    assert recs[2]["il"]["I"][0, 21] > -200.0 and recs[2]["il"]["Rmin"][0, 21] > -200.0
    for s, c0 in ((1, 0), (2, 0), (3, 0), (5, 0), (6, 0), (4, 1)):      # a closed stream's row and count do not move in later calls
        for c in range(c0 + 1, 3):
            for f in FIELDS + ("n_points", "dropped"):
                assert _same(recs[c0]["il"][f][s], recs[c]["il"][f][s]), (s, c, f)


# ---- 6. a long call: the one-workgroup walk where the log-off call takes k_gate_frag / k_gate_final ----------------------------------

def test_long_call(M):
    x = G.batch(LONG, 4200)
    T = x.shape[1]
    for cuts in ([T], [4096 * G.FRAG + 189, T]):
        recs = run(M, x, cuts)[0]
        assert (recs[-1]["il"]["n_points"] == 420).all() and not recs[-1]["il"]["dropped"].any()
        hold(recs[-1]["il"], yardstick(recs), tag="long call %s" % [b // G.FRAG for b in cuts])
        off = run(M, x, cuts, K=0)[0]
        assert off[0]["frag"].shape[1] >= 4096           # (the call went the long way)
        for k in ("out9", "counts", "hist_M", "hist_S", "M", "S", "n"):
            assert _same(recs[-1][k], off[-1][k]), (cuts, k)


# ---- 7. the deferred gate: a workgroup walks several streams ------------------------------------------------------------------------------

def test_deferred_walk(M, monkeypatch):
    monkeypatch.setenv("MTR_TAIL_GATE_GRID", "3")        # read by mtr_engine_create (include/mtr_engine.h): 11 streams over 3 workgroups
    x = G.batch()[:11]
    ends = G.call_ends(x.shape[1])
    serial, blob1, nd1 = run(M, x, ends, tail=1, every_call=False)
    walked, blob2, nd2 = run(M, x, ends, tail=2, every_call=False)     # (no getter between the calls: the gates queue up)
    assert nd1 == 0 and nd2 == len(ends)
    assert (serial[-1]["il"]["n_points"] == 85).all()
    same_series(walked[-1]["il"], serial[-1]["il"], what="deferred")
    for k in ("out9", "counts", "hist_M", "hist_S", "M", "S", "n", "d"):
        assert _same(walked[-1][k], serial[-1][k]), k
    assert blob1 == blob2
    CHECKED.add("deferred")


# ---- 8. 48 kHz beside the true-peak meter, and the host route ---------------------------------------------------------------------------

def test_48k_with_truepeak_and_host_chunks(M):
    # (60 fragments would never pass the 50-point minimum: 240)
    x = G.batch(("fuzz0", "fuzz1", "steady", "zeros"), 240, frag=2400, fs=48000.0)
    ends = [5000, 5001, 7400, x.shape[1]]
    recs = run(M, x, ends, fs=48000.0, meters=M.METER_EBU | M.METER_TRUEPEAK)[0]
    il = recs[-1]["il"]
    assert (il["n_points"] == 24).all() and (il["I"][:3, 23] > -200.0).all() and (il["Rmin"][:3, 23] > -200.0).all()
    hold(il, yardstick(recs), tag="48 kHz with true peak")
    host = run(M, x, ends, fs=48000.0, meters=M.METER_EBU | M.METER_TRUEPEAK, host=True)[0]      # three streams per chunk: two chunks
    same_series(host[-1]["il"], il, what="host chunks")


# ---- 9. against the reference's own Ebu_r128_proc, polled every ten fragments ----------------------------------------------------------

def test_against_the_reference(M):
    from _oracle import Oracle
    from test_gpu_parity import CONTRACT_DB
    fs, frag, nfrag = 48000.0, 2400, 120
    rng = np.random.default_rng(4321)
    x = np.zeros((3, nfrag * frag, 2), np.float32)
    x[0] = 0.1 * rng.standard_normal((nfrag * frag, 2))
    x[1] = (0.02 + 0.2 * (np.arange(nfrag * frag) // (7 * frag) % 3))[:, None] * rng.standard_normal((nfrag * frag, 2))
    orc = Oracle()
    want = np.zeros((3, nfrag // 10, 5), np.float32)
    for s in range(3):
        o = orc.ebu_stream(fs)
        o.start()
        for j in range(nfrag // 10):
            seg = x[s, j * 10 * frag:(j + 1) * 10 * frag]
            want[s, j] = o.process(seg[:, 0], seg[:, 1], with_tp=False)[0][4:9]
    il = run(M, x, [x.shape[1]], fs=fs)[0][-1]["il"]
    assert (il["n_points"] == nfrag // 10).all()
    got = np.stack([il[f][:, :nfrag // 10] for f in FIELDS], axis=2)
    dev = np.abs(got.astype(np.float64) - want)
    print("\nagainst the reference: largest deviations I %.2e  I_thr %.2e  Rmin %.2e  Rmax %.2e  R_thr %.2e dB" % tuple(dev.max(axis=(0, 1))))
    assert (want[:2, -1, 0] > -60.0).all() and (want[2, :, 0] == -200.0).all()
    assert (dev[:, :, [0, 1, 4]] <= CONTRACT_DB).all() and (dev[:, :, [2, 3]] <= 0.1001).all(), dev.max(axis=(0, 1))
    CHECKED.add("reference")


def test_skipped_share_of_the_file():
    """(last) skipped evaluations are at most 2 % of all evaluations in the file; a run of single tests only prints its own"""
    print(f"\n{len(CHECKED)} of {N_CHECKS} checks ran: {STATS['skipped']} of {STATS['evaluations']} evaluations skipped")
    if len(CHECKED) == N_CHECKS:
        assert STATS["skipped"] * 50 <= STATS["evaluations"], STATS
