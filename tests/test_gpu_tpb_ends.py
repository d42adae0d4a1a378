"""Track lengths for the true-peak bar (include/mtr_tpb_ends.h: mtr_engine_process_*_tpb, the ENDS instantiations of k_tpb) on the GPU.

The shapes are those of tests/test_gpu_tpb_series.py: stereo S = 33 (two workgroups, the second with one stream), mono S = 65, T = 5003,
calls cut at CUTS + T.  A stream's track length L is a frame of the whole feed: call [a, b) gets frames[s] = clamp (L - a, 0, b - a).
Bit-for-bit references are engines of this library fed the dense call (truncated at the stream's end where the stream closes); the
numerical reference is TruePeakdsp itself (the oracle's object) within the meter's own bound, TPB_REL = 4e-6 of the value
(tests/test_gpu_parity.py:41) — a column's end adds no arithmetic of its own to what a block's end or a call's end does."""
import ctypes as C

import numpy as np
import pytest

import _signals as sig

pytestmark = pytest.mark.gpu

TPB_REL = 4e-6
ERR_ARG, ERR_UNSUPPORTED = -1, -2
CUTS = (0, 1, 16, 33, 700, 717)
T = 5003
QUIET = {5: 1e-2, 6: 1e-3, 7: 1e-4}
PERIODS = (0, 16, 23, 100, 4800)


@pytest.fixture(scope="module")
def M():
    import meters.lv2_amd as m
    assert (m.engine.ERR_ARG, m.engine.ERR_UNSUPPORTED) == (ERR_ARG, ERR_UNSUPPORTED)
    return m


@pytest.fixture(scope="module")
def oracle():
    from _oracle import Oracle
    return Oracle()


_NOISE = {}


def noise(S=65):
    if "x" not in _NOISE:
        _NOISE["x"] = np.stack([sig.lcg_noise(T, 700 + s, 2.0 ** -(s % 4) * QUIET.get(s % 8, 1.0)) for s in range(65)])
    return _NOISE["x"][:S]


def feed_of(chn, S):
    x = noise(S)
    return x if chn == 2 else np.ascontiguousarray(x[:, :, 0])


CALLS = list(zip(CUTS, CUTS[1:] + (T,)))


def lengths(S, P, variant):
    """Track lengths of S streams.  Variant 0: every kind of end among the first workgroup's streams (which runs to the call's end: some
    stay open), the lone stream of the second workgroup closed.  Variant 1: every stream of the first workgroup ends early — inside the
    call [33, 700), so that its loop stops long before the call does and every later call finds all its ends 0 — and the lone stream open."""
    Q = P or 23
    k = max(1, 2300 // Q) * Q                  # a block end: ends on it (r = 0), next to it, and in its 16-frame chunk in front of it and behind it
    kinds = [0, 1, 15, 16, 17, 47, 48, T - 1, T, 20, 705, k, k - 1, k + 1, k - 5, k + 3, Q, Q + 1, 2 * Q - 1, 33, 700, 716, 3000, T]
    early = [0, 1, 15, 16, 17, 47, 48, 20, 33, 34, 49, 64, 65, 100, Q, Q + 1, 2 * Q - 1, 600]
    n0 = S - 1
    if variant == 0:
        ls = [kinds[s % len(kinds)] for s in range(n0)] + [k + 1]
    else:
        ls = [early[s % len(early)] for s in range(n0)] + [T]
    return np.minimum(np.array(ls, np.int64), T)                 # (P = 4800: two blocks are more than the feed)


def frames_of(ls, a, b):
    return np.clip(ls - a, 0, b - a).astype(np.uint64)


def res_of(e):
    r = e.results()
    chn = e.n_channels
    return (np.array([[r[s].tpb_level[c] for c in range(chn)] for s in range(e.n_streams)], np.float32),
            np.array([[r[s].tpb_peak[c] for c in range(chn)] for s in range(e.n_streams)], np.float32))


def same(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def snap(e):
    lv, pk, n, d = e.tpb_series()
    return dict(level=res_of(e)[0], peak=res_of(e)[1], s_level=lv, s_peak=pk, n=n, d=d, points=e.tpb_points(), blob=e.state_export())


def snaps_equal(a, b):
    return all(same(a[k], b[k]) if isinstance(a[k], np.ndarray) and a[k].dtype == np.float32 else np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray)
               else a[k] == b[k] for k in a)


def engine(M, S, chn, fs, P, cap=512, meters=None):
    e = M.Engine(S, fs, M.METER_TPBALLIST if meters is None else meters, n_channels=chn)
    if P:
        e.tpb_set_period(P, cap)
    return e


_RUNS = {}


def run_tpb(M, chn, S, fs, P, variant, cap=512):
    """the _tpb engine's snapshot behind the whole feed (host form), computed once per case"""
    key = (chn, S, fs, P, variant, cap)
    if key not in _RUNS:
        feed, ls = feed_of(chn, S), lengths(S, P, variant)
        with engine(M, S, chn, fs, P, cap) as e:
            for a, b in CALLS:
                e.process_tpb(np.ascontiguousarray(feed[:, a:b]), frames_of(ls, a, b))
            _RUNS[key] = (snap(e), e.stream_frames())
    return _RUNS[key]


def want_points(M, ls, P):
    """the arithmetic of mtr_series_cut over the calls: points per stream"""
    out = np.zeros(len(ls), np.uint64)
    if not P:
        return out
    for s, L in enumerate(ls):
        for a, b in CALLS:
            w, p = C.c_uint64(), C.c_uint32()
            f = int(min(max(L - a, 0), b - a))
            assert M.lib.mtr_series_cut(a % P, P, b - a, f, C.byref(w), C.byref(p)) == 0
            out[s] += w.value + p.value
            if f < b - a:
                break
    return out


def hold(got, want, what):
    assert abs(got - want) <= TPB_REL * want + 1e-37, (what, got, want)


# ---- 1. identity with the dense call ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [0, 23, 4800])
@pytest.mark.parametrize("chn,S", [(2, 33), (1, 65)])
def test_all_open_is_the_dense_call(M, chn, S, P):
    feed = feed_of(chn, S)
    with engine(M, S, chn, 48000.0, P) as d, engine(M, S, chn, 48000.0, P) as e:
        for a, b in CALLS:
            d.process(np.ascontiguousarray(feed[:, a:b]))
            e.process_tpb(np.ascontiguousarray(feed[:, a:b]), np.full(S, b - a, np.uint64))
            sd, se = snap(d), snap(e)
            if P:
                sd["points"] = np.full(S, b // P, np.uint64)       # (the dense call counts them as well: the hook is the call path's)
            assert snaps_equal(sd, se), (a, b)
        assert not e.stream_frames()[1].any()


@pytest.mark.parametrize("P", [0, 23])
def test_dense_call_on_an_engine_with_closed_streams(M, P):
    """process() once streams are closed: the closed ones untouched, the open ones bit for bit those of an engine that never closed any"""
    chn, S = 2, 33
    feed, ls = feed_of(chn, S), lengths(S, P, 0)
    at = 4
    with engine(M, S, chn, 48000.0, P) as d, engine(M, S, chn, 48000.0, P) as e:
        for a, b in CALLS[:at]:
            d.process(np.ascontiguousarray(feed[:, a:b]))
            e.process_tpb(np.ascontiguousarray(feed[:, a:b]), frames_of(ls, a, b))
        closed = e.stream_frames()[1]
        assert closed.any() and not closed.all() and closed[:32].any() and not closed[:32].all()
        frozen = snap(e)
        hdr = 2 * e.state_bytes(1) - e.state_bytes(2)
        blobs = [e.state_export(s, 1)[hdr:] for s in range(S)]
        for a, b in CALLS[at:]:
            d.process(np.ascontiguousarray(feed[:, a:b]))
            e.process(np.ascontiguousarray(feed[:, a:b]))
        sd, se = snap(d), snap(e)
        op = ~closed
        for k in ("level", "peak", "s_level", "s_peak"):
            assert same(sd[k][op], se[k][op]), k
            n = frozen[k].shape[1] if k.startswith("s_") else None
            assert same(se[k][closed][:, :n], frozen[k][closed]), k
            if k.startswith("s_"):
                assert not se[k][closed][:, n:].any()                  # 0.0f behind a closed stream's own points
        assert np.array_equal(se["points"][closed], frozen["points"][closed])
        for s in range(S):
            if closed[s] and not P:
                assert e.state_export(s, 1)[hdr:] == blobs[s], s
            if not closed[s]:
                assert e.state_export(s, 1)[hdr:] == d.state_export(s, 1)[hdr:], s


# ---- 2. closed streams, bit for bit the truncated dense call -------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [0, 23])
@pytest.mark.parametrize("chn,S", [(2, 33), (1, 65)])
def test_closed_streams_equal_the_truncated_call(M, chn, S, P):
    """One engine per distinct end L (ten of them), fed the same calls with the closing call truncated to n_frames = L: a column's samples
    behind its end are the zeros that call's last chunk holds, and columns are independent."""
    feed, ls = feed_of(chn, S), lengths(S, P, 0)
    got, _ = run_tpb(M, chn, S, 48000.0, P, 0)
    k = max(1, 2300 // (P or 23)) * (P or 23)
    ends = [1, 16, 17, 47, 20, 705, k - 5, k, k + 3, T - 1]
    assert all((ls == L).any() for L in ends)
    for L in ends:
        with engine(M, S, chn, 48000.0, P) as d:
            for a, b in CALLS:
                if a < L:
                    d.process(np.ascontiguousarray(feed[:, a:min(b, L)]))
            w = snap(d)
        for s in np.flatnonzero(ls == L):
            if P:
                n = L // P
                assert w["n"] == n
                assert same(got["s_level"][s, :n], w["s_level"][s, :n]) and same(got["s_peak"][s, :n], w["s_peak"][s, :n]), (L, s)
            else:
                assert same(got["level"][s], w["level"][s]) and same(got["peak"][s], w["peak"][s]), (L, s)


# ---- 3. closed streams against TruePeakdsp -------------------------------------------------------------------------------------------------
CASES = [(2, 33, 48000.0, P, v) for P in PERIODS for v in (0, 1)] + [(1, 65, 48000.0, P, 0) for P in (0, 23, 100)] + [(1, 65, 48000.0, 16, 1), (2, 33, 44100.0, 100, 0)]


@pytest.mark.parametrize("chn,S,fs,P,variant", CASES)
def test_every_stream_matches_truepeakdsp(M, oracle, chn, S, fs, P, variant):
    ls = lengths(S, P, variant)
    x = noise(S)
    got, (metered, closed) = run_tpb(M, chn, S, fs, P, variant)
    assert np.array_equal(metered, ls.astype(np.uint64)) and np.array_equal(closed, ls < T)
    pts = want_points(M, ls, P)
    assert np.array_equal(got["points"], pts)
    assert got["n"] == (T // P if P else 0) and got["d"] == 0
    if P:
        for s in range(S):
            assert not got["s_level"][s, int(pts[s]):].any() and not got["s_peak"][s, int(pts[s]):].any(), s
    # every kind of end once (the kinds repeat with the streams), the quiet streams, both workgroups
    pick = sorted(set(list(range(min(S - 1, 24))) + [S - 1]))
    for s in pick:
        L = int(ls[s])
        for c in range(chn):
            ch = np.ascontiguousarray(x[s, :L, c])
            if P:
                # every whole block and, where a call closes the stream inside one, the truncated block (a stream whose end is a call's
                # end is closed by the next call's frames [s] = 0, untouched: no reading is taken there — the _tracks rule)
                exp = L // P + (1 if L % P and L < T and L not in CUTS else 0)
                assert pts[s] == exp, (s, L)
                w = oracle.tp_process_seq(ch, fs, P)[:exp] if L else np.zeros((0, 2), np.float32)
                assert len(w) == exp, (s, L)
                # (the getter hands out the lock-step count of points: a truncated point behind the engine's last whole block — L = T - 1 at
                # P = 16 — is in the series' memory and is what results () reports, and comes out of the getter once the engine has moved on)
                shown = got["s_level"].shape[1]
                assert exp <= shown + 1
                for k in range(min(len(w), shown)):
                    hold(got["s_level"][s, k, c], w[k, 0], ("level", s, L, c, k))
                    hold(got["s_peak"][s, k, c], w[k, 1], ("peak", s, L, c, k))
                if len(w):                                               # results (): the stream's last point, as the series holds it
                    hold(got["level"][s, c], w[-1, 0], ("last level", s, L, c))
                    hold(got["peak"][s, c], w[-1, 1], ("last peak", s, L, c))
                    if len(w) <= shown:
                        assert same(got["level"][s, c], got["s_level"][s, len(w) - 1, c]) and same(got["peak"][s, c], got["s_peak"][s, len(w) - 1, c])
                else:
                    assert got["level"][s, c] == 0 and got["peak"][s, c] == 0
            else:
                # one process () of the stream's frames of each call, read (m, p) behind it: the last call that gave it any
                from _oracle import MoTp
                t = MoTp()
                oracle.lib.mo_tp_init(C.byref(t), fs)
                m, p = C.c_float(), C.c_float()
                for a, b in CALLS:
                    seg = np.ascontiguousarray(ch[a:b])
                    if seg.size:
                        oracle.lib.mo_tp_process(C.byref(t), seg, seg.size)
                        oracle.lib.mo_tp_read2(C.byref(t), C.byref(m), C.byref(p))
                hold(got["level"][s, c], m.value, ("level", s, L, c))
                hold(got["peak"][s, c], p.value, ("peak", s, L, c))


def test_capacity_drops_and_counts_per_stream(M):
    chn, S, P = 2, 33, 100
    ls = lengths(S, P, 0)
    big, _ = run_tpb(M, chn, S, 48000.0, P, 0)
    got, _ = run_tpb(M, chn, S, 48000.0, P, 0, cap=5)
    assert got["n"] == T // P and got["d"] == T // P - 5
    assert np.array_equal(got["points"], big["points"]) and np.array_equal(got["points"], want_points(M, ls, P))
    assert got["s_level"].shape == (S, 5, chn) and same(got["s_level"], big["s_level"][:, :5]) and same(got["s_peak"], big["s_peak"][:, :5])
    assert same(got["level"], big["level"]) and same(got["peak"], big["peak"])        # (the last point's, kept or dropped)
    assert (got["points"] > 5).any() and (got["points"] < 5).any()


# ---- 4. poison behind the ends -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chn,S,P,variant", [(2, 33, 0, 0), (2, 33, 23, 0), (1, 65, 23, 1), (1, 65, 0, 0)])
def test_nothing_behind_an_end_is_looked_at(M, chn, S, P, variant):
    import torch
    feed, ls = feed_of(chn, S), lengths(S, P, variant)
    garbage = np.array([np.nan, np.inf, 1e30, 1e-40, -np.inf, -1e30], np.float32)
    st = torch.cuda.current_stream().cuda_stream
    out = []
    for off, stride in ((0, T + 5), (2, T + 7)):       # rows on 16 bytes (whole chunks by LDS-DMA where the call starts on 16 bytes), a view on 8
        assert (stride * chn * 4) % 16 == 0 or off
        for dirty in (False, True):
            host = np.zeros((S, stride, chn), np.float32)
            host[:, :T] = feed.reshape(S, T, chn)
            for s, L in enumerate(ls):
                host[s, L:] = 0
                if dirty:
                    host[s, L:] = garbage[(np.arange(stride - L)[:, None] + np.arange(chn)[None, :] + s) % garbage.size]
            flat = torch.zeros(S * stride * chn + 8, dtype=torch.float32, device="cuda")
            flat[off:off + S * stride * chn] = torch.from_numpy(host.reshape(-1)).cuda()
            with engine(M, S, chn, 48000.0, P) as e:
                for a, b in CALLS:
                    e.process_device_tpb(flat.data_ptr() + 4 * (off + a * chn), b - a, frames_of(ls, a, b), stride, st)
                out.append(snap(e))
            del flat
    want, _ = run_tpb(M, chn, S, 48000.0, P, variant)
    for i, o in enumerate(out):
        assert snaps_equal(o, want), i


# ---- 5. every way in gives the same bits ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [0, 23])
def test_host_chunks_and_the_state_blob(M, P):
    chn, S = 2, 33
    feed, ls = feed_of(chn, S), lengths(S, P, 0)
    want, _ = run_tpb(M, chn, S, 48000.0, P, 0)
    at = 4
    with engine(M, S, chn, 48000.0, P) as e, engine(M, S, chn, 48000.0, P) as f:
        for a, b in CALLS[:at]:
            e.set_host_chunk_bytes(7 * ((b - a + 1) & ~1) * 8)             # seven streams per chunk
            e.process_tpb(np.ascontiguousarray(feed[:, a:b]), frames_of(ls, a, b))
        closed = e.stream_frames()[1]
        n0 = e.tpb_series()[2]
        assert f.state_import(e.state_export()) == S                   # (the blob carries no closure: the frames [s] = 0 of the calls behind it close them again)
        for a, b in CALLS[at:]:
            for eng in (e, f):
                eng.set_host_chunk_bytes(7 * ((b - a + 1) & ~1) * 8)
                eng.process_tpb(np.ascontiguousarray(feed[:, a:b]), frames_of(ls, a, b))
        se, sf = snap(e), snap(f)
        assert snaps_equal(se, want)
        op = ~closed
        assert same(se["level"][op], sf["level"][op]) and same(se["peak"][op], sf["peak"][op])
        assert same(se["s_level"][op][:, n0:], sf["s_level"][op]) and same(se["s_peak"][op][:, n0:], sf["s_peak"][op])
        hdr = 2 * e.state_bytes(1) - e.state_bytes(2)
        for s in np.flatnonzero(op):
            assert e.state_export(s, 1)[hdr:] == f.state_export(s, 1)[hdr:], s
        # a closed stream's part of the blob — states, readings, the open block's entry, the interpolator's history row — stays as it is over
        # two further calls (of a whole block together: the entry's header is the engine's lock-step cursor)
        now = e.stream_frames()[1]
        before = [e.state_export(s, 1)[hdr:] for s in range(S)]
        loud = sig.lcg_noise(T, 77, 3.0)
        n1, n2 = ((P - 7, 7) if P else (50, 17))
        e.process(np.ascontiguousarray(np.broadcast_to(loud[None, :n1], (S, n1, 2))))
        e.process_tpb(np.ascontiguousarray(np.broadcast_to(loud[None, n1:n1 + n2], (S, n2, 2))), np.full(S, n2, np.uint64))
        for s in range(S):
            assert (e.state_export(s, 1)[hdr:] == before[s]) == bool(now[s]), s


# ---- 6. beside the other meters ------------------------------------------------------------------------------------------------------------
def test_the_dr14_plugins_meter_set(M):
    chn, S, P = 2, 33, 0
    feed, ls = feed_of(chn, S), lengths(S, P, 0)
    want, _ = run_tpb(M, chn, S, 48000.0, P, 0)
    both = M.METER_DR14 | M.METER_KMETER
    with engine(M, S, chn, 48000.0, 0, meters=M.METER_TPBALLIST | both) as e, engine(M, S, chn, 48000.0, 0, meters=both) as d:
        for a, b in CALLS:
            e.process_tpb(np.ascontiguousarray(feed[:, a:b]), frames_of(ls, a, b))
            d.process_tracks(np.ascontiguousarray(feed[:, a:b]), frames_of(ls, a, b))
        assert bytes(e.dr14()) == bytes(d.dr14())
        assert all(same(u, v) for u, v in zip(e.kmeter_read(), d.kmeter_read()))
        assert same(res_of(e)[0], want["level"]) and same(res_of(e)[1], want["peak"])
    fused = M.METER_EBU | M.METER_TRUEPEAK
    with engine(M, S, chn, 48000.0, 0, meters=fused) as e, engine(M, S, chn, 48000.0, 0, meters=fused) as d:
        for a, b in CALLS:
            e.process_tpb(np.ascontiguousarray(feed[:, a:b]), frames_of(ls, a, b))
            d.process_lengths(np.ascontiguousarray(feed[:, a:b]), frames_of(ls, a, b))
        assert bytes(e.results()) == bytes(d.results()) and e.state_export() == d.state_export()


# ---- 7. the surface ------------------------------------------------------------------------------------------------------------------------
def test_surface(M):
    fs, S, n = 48000.0, 4, 1000
    x = noise(S)[:, :n]

    def refused(code, f, *args):
        with pytest.raises(M.EngineError) as err:
            f(*args)
        assert err.value.code == code, (err.value.code, str(err.value))

    full = np.full(S, n, np.uint64)
    for meters, chn in ((M.METER_SURROUND, 5), (M.METER_SCOPE | M.METER_TPBALLIST, 2), (M.METER_EBU, 5)):
        with M.Engine(S, fs, meters, n_channels=chn) as e:
            before = (e.state_export(), bytes(e.results()))
            refused(ERR_UNSUPPORTED, e.process_tpb, np.zeros((S, n, chn), np.float32), full)
            assert (e.state_export(), bytes(e.results())) == before and not e.stream_frames()[0].any()
    with M.Engine(S, fs, M.METER_DR14) as e:
        refused(ERR_ARG, e.tpb_points)
    with engine(M, S, 2, fs, 100, cap=64) as e:
        e.process_tpb(x[:, :250], np.array([250, 250, 30, 0], np.uint64))
        before = snap(e)
        assert before["points"].tolist() == [2, 2, 1, 0]
        long = full.copy()
        long[1] = n + 1
        refused(ERR_ARG, e.process_tpb, x, long)
        assert snaps_equal(snap(e), before)
        refused(ERR_ARG, e.tpb_points, 2, S)
        e.reset()                                                        # zeroes the points, reopens the streams, keeps P
        assert e.tpb_period() == (100, 64) and not e.tpb_points().any() and not e.stream_frames()[1].any()
        assert e.tpb_series()[2:] == (0, 0) and not res_of(e)[0].any()
        e.process_tpb(x[:, :250], np.array([250, 250, 30, 0], np.uint64))
        assert snaps_equal(snap(e), before)
