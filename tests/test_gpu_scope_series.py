"""The scope's reading series on the GPU (mtr_engine_scope_set_series / _series_config / _series, include/mtr_scope_series.h; the SERIES
instantiation of k_scope, mtr_scope.hip).

The yardstick is the engine WITHOUT a series, whose kernel is the one tests/test_gpu_scope.py holds against the restatement of
tests/_scope.py: point n of a series of one point per K analyses is, bit for bit and in all seven fields — bins 0 and B - 1 included —
what scope_read of a series-off engine answers after exactly (n + 1) K H frames, however the calls cut the audio.  Two cases (an even and an odd log2 W) hold
the points against the restatement itself, to the tolerances tests/test_gpu_scope.py states.  S = 5 streams, its signals and seeds
(13 analyses and 5 frames), buffer rows longer than T with NaN in the gap."""
import ctypes as C
import functools

import numpy as np
import pytest

import _scope
import test_gpu_scope as tg

pytestmark = pytest.mark.gpu
FS, S, NA, NAMES = tg.FS, tg.S, tg.NA, tg.NAMES
SENT = np.float32(-7.25)                                              # what a getter's row holds before the call
DEFAULT = _scope.default_hop(FS)


@pytest.fixture(scope="module")
def M():
    import meters.lv2_amd as m
    return m


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def equal(a, b, names=NAMES):
    return all(a[n].shape == b[n].shape and np.array_equal(bits(a[n]), bits(b[n])) for n in names)


_dev = {}


def device_rows(x, key=None):
    """x [S, T, 2] in device memory, rows of T + 37 frames with NaN behind the stream's own; kept per key"""
    import torch
    if key is not None and key in _dev:
        return _dev[key]
    buf = np.full((x.shape[0], x.shape[1] + 37, 2), np.nan, np.float32)
    buf[:, :x.shape[1]] = x
    dev = torch.from_numpy(buf).cuda()
    if key is not None:
        _dev[key] = dev
    return dev


def feed(e, dev, calls, pos=0):
    import torch
    st = torch.cuda.current_stream().cuda_stream
    for n in calls:
        e.process_device(dev.data_ptr() + pos * 8, n, dev.shape[1], st)
        pos += n
    return pos


@functools.lru_cache(maxsize=None)
def snapshots(W, H):
    """the series-off engine on tg.signal_of (W, H): scope_read after exactly (j + 1) H frames for j = 0 .. 12, and after all T frames"""
    import meters.lv2_amd as m
    x = tg.signal_of(W, H)
    dev = device_rows(x, (W, H))
    e = m.Engine(S, float(FS), m.METER_SCOPE)
    e.scope_configure(W, H, _scope.THRESH)
    assert e.scope_series_config() == (0, 0, 0)
    snaps = []
    for j in range(NA):
        feed(e, dev, [H], j * H)
        snaps.append(e.scope_read())
    feed(e, dev, [x.shape[1] - NA * H], NA * H)
    final = e.scope_read()
    assert e.scope_analyses() == NA
    e.close()
    return snaps, final


def expected(snaps, K, n_pts, first=0):
    """points first .. first + n_pts - 1 of a series of one point per K analyses, from the snapshots: {name: [S, n_pts, B]} and peak [S, n_pts]"""
    return {n: np.stack([snaps[(first + p + 1) * K - 1][n] for p in range(n_pts)], axis=1) for n in NAMES}


def series_engine(M, W, H, K, cap, fields=None, meters=None, thresh=_scope.THRESH):
    e = M.Engine(S, float(FS), M.METER_SCOPE if meters is None else meters)
    e.scope_configure(W, H, thresh)
    e.scope_set_series(K, cap, M.SCOPE_F_ALL if fields is None else fields)
    return e


def run_series(M, W, H, K, cap=NA, calls=None, x=None, **kw):
    """-> (series dict, n_points, dropped, scope_read behind the last call)"""
    key = (W, H) if x is None else None
    x = tg.signal_of(W, H) if x is None else x
    dev = device_rows(x, key)
    e = series_engine(M, W, H, K, cap, **kw)
    assert feed(e, dev, calls or [x.shape[1]]) == x.shape[1]
    out = e.scope_series() + (e.scope_read(),)
    assert e.scope_analyses() == x.shape[1] // H
    e.close()
    return out


def raw(M, e, capacity, names, first=0, count=S):
    """mtr_engine_scope_series into rows of `capacity` points pre-filled with SENT -> (rc, arrays, n_points, dropped)"""
    B = e.scope_config()[0] // 2
    out = {n: np.full((count, capacity) + (() if n == "peak" else (B,)), SENT, np.float32) for n in names}
    n_, d_ = C.c_uint32(), C.c_uint32()
    ptrs = [out[n].ctypes.data if n in out else None for n in NAMES]
    rc = M.lib.mtr_engine_scope_series(e._h, first, count, *ptrs, capacity, C.byref(n_), C.byref(d_))
    return rc, out, n_.value, d_.value


# ---- against the engine without a series, bit for bit -----------------------------------------------------------------------------

# every window: 256, 1024 and 16384 at both hops and K = 1, 3, 5; the others — an odd log2 W, or the r loops at 1 and 4 trips — at H 777, K 3
POINT_CASES = [(W, hk, K) for W in (256, 1024, 16384) for hk in ("777", "default") for K in (1, 3, 5)] + [(W, "777", 3) for W in (512, 2048, 4096, 8192)]


@pytest.mark.parametrize("W,hk,K", POINT_CASES)
def test_points_are_what_scope_read_would_answer(M, W, hk, K):
    H, B = tg.hop_of(W, hk), W // 2
    snaps, final = snapshots(W, H)
    T = NA * H + 5
    want = expected(snaps, K, NA // K)
    assert want["level"].shape == (S, NA // K, B) and want["peak"].shape == (S, NA // K)
    cuts = [1, H - 1, H + 1, 3 * H + 7]                                # (calls that complete no analysis, and analyses but no point)
    for calls in (None, cuts + [T - sum(cuts)]):
        got, n, d, last = run_series(M, W, H, K, calls=calls)
        assert (n, d) == (NA // K, 0), calls
        for name in NAMES:
            assert np.array_equal(bits(got[name]), bits(want[name])), (name, calls)
        assert (got["level"][:, :, 0] == -100).all() and (got["level"][:, :, B - 1] == -100).all()
        assert (got["lr"][:, :, 0] == np.float32(.5)).all() and (got["plevel"][:, :, B - 1] == -100).all()
        assert (bits(got["phase"][:, :, 0]) == 0).all() and (bits(got["power_l"][:, :, 0]) == 0).all() and (bits(got["power_r"][:, :, B - 1]) == 0).all()
        assert equal(last, final), calls


# ---- against the restatement ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W,H,K", [(1024, DEFAULT, 3), (2048, DEFAULT, 3)])
def test_points_against_the_restatement(M, W, H, K):
    """W 1024 and W 2048 — a series kernel with an odd log2 W — at the default hop, K = 3: every point to the tolerances of
    tests/test_gpu_scope.py — sqrt power to eps N; level, plevel and peak to 4 eps max N^2; lr to 4 eps rho on the bins with rho <= 1 / LR_FLOOR (at most 1 % of a stream's bins outside); phase to
    |wrap (delta)| min |X| <= 4 eps N above the threshold, 0 / -100 exactly below it, bins within 1e-4 of it left out (at most 0.1 %) —
    with N, max N and rho taken over the analyses up to the point's own."""
    B, x = W // 2, tg.signal_of(W, H)
    got, n, d, _ = run_series(M, W, H, K)
    assert (n, d) == (NA // K, 0)
    eps, win = _scope.eps(W), _scope.window(W)
    fig = dict(power=0.0, level=0.0, plevel=0.0, peak=0.0, lr=0.0, phase=0.0)
    inner = np.zeros(B, bool)
    inner[1:B - 1] = True
    for s in range(S):
        rho, nmax = np.zeros(B - 2), [0.0]

        def each(j, sc):
            m = np.sqrt(np.maximum(sc.p64[0, 1:B - 1], sc.p64[1, 1:B - 1]))
            with np.errstate(divide="ignore"):
                np.maximum(rho, np.where(m > 0, sc.N / m, np.inf), out=rho)
            nmax[0] = max(nmax[0], sc.N)
            if (j + 1) % K:
                return
            p = (j + 1) // K - 1
            g = {name: got[name][s, p] for name in NAMES}
            for c, name in enumerate(("power_l", "power_r")):
                q = g[name].astype(np.float64)
                assert q[0] == 0 and q[B - 1] == 0 and (q >= 0).all()
                fig["power"] = max(fig["power"], float(np.max(np.abs(np.sqrt(q) - np.sqrt(sc.p64[c])))) / (eps * sc.N))
            bound = 4 * eps * nmax[0] ** 2
            fig["level"] = max(fig["level"], float(np.max(np.abs(g["level"].astype(np.float64) - sc.level))) / bound)
            fig["peak"] = max(fig["peak"], abs(float(g["peak"]) - float(sc.peak)) / bound)
            near = tg.near_threshold(sc)
            assert near.mean() <= 1e-3, (s, p)
            fig["plevel"] = max(fig["plevel"], float(np.max(np.abs(g["plevel"].astype(np.float64) - sc.plevel)[~near])) / bound)
            ok = rho * tg.LR_FLOOR <= 1
            assert np.mean(~ok) <= 0.01, (s, p)
            dl = np.abs(g["lr"].astype(np.float64) - sc.lr)
            assert dl[0] == 0 and dl[B - 1] == 0
            fig["lr"] = max(fig["lr"], float(np.max(dl[1:B - 1][ok] / (4 * eps * rho[ok]))))
            below = np.any(sc.power < sc.thresh, axis=0) & inner & ~near
            above = ~np.any(sc.power < sc.thresh, axis=0) & inner & ~near
            assert (g["phase"][below] == 0).all() and (g["plevel"][below] == -100).all(), (s, p)
            assert g["phase"][0] == 0 and g["phase"][B - 1] == 0 and g["plevel"][0] == -100 and g["level"][B - 1] == -100
            dp = g["phase"].astype(np.float64) - sc.phase.astype(np.float64)
            dp = np.abs((dp + np.pi) % (2 * np.pi) - np.pi)
            amp = np.sqrt(np.minimum(sc.p64[0], sc.p64[1]))
            fig["phase"] = max(fig["phase"], float(np.max((dp * amp)[above])) / (4 * eps * sc.N))
        _, n_an = _scope.run(x[s], W, H, win=win, each=each)
        assert n_an == NA
    print("W %d H %d K %d, %d points: in units of the bounds: " % (W, H, K, n) + ", ".join("%s %.2e" % kv for kv in fig.items()))
    assert max(fig.values()) <= 1.0, fig


# ---- capacity --------------------------------------------------------------------------------------------------------------------------

def test_capacity(M):
    W, H, B = 1024, 777, 512
    snaps, _ = snapshots(W, H)
    got, n, d, _ = run_series(M, W, H, 1, cap=4)
    assert (n, d) == (13, 9) and equal(got, expected(snaps, 1, 4))
    # the getter's own capacity: 2 and 6 points per row of a ring of 4
    dev = device_rows(tg.signal_of(W, H), (W, H))
    e = series_engine(M, W, H, 1, 4)
    feed(e, dev, [NA * H + 5])
    want = expected(snaps, 1, 4)
    for capacity in (2, 6):
        rc, out, n, d = raw(M, e, capacity, NAMES)
        k = min(capacity, 4)
        assert rc == 0 and (n, d) == (13, 9)
        for name in NAMES:
            assert np.array_equal(bits(out[name][:, :k]), bits(want[name][:, :k])), (name, capacity)
            assert (bits(out[name][:, k:]) == bits(SENT)).all(), (name, capacity)
    e.close()
    # a ring of no points: the counts alone
    e = series_engine(M, W, H, 1, 0)
    assert e.scope_series_config() == (1, 0, M.SCOPE_F_ALL)
    feed(e, dev, [NA * H + 5])
    rc, out, n, d = raw(M, e, 3, NAMES)
    assert rc == 0 and (n, d) == (13, 13)
    for name in NAMES:
        assert (bits(out[name]) == bits(SENT)).all(), name
    series, n, d = e.scope_series()
    assert (n, d) == (13, 13) and series["level"].shape == (S, 0, B) and series["peak"].shape == (S, 0)
    e.close()


# ---- fields ----------------------------------------------------------------------------------------------------------------------------

def test_fields(M):
    W, H = 1024, 777
    snaps, final = snapshots(W, H)
    want = expected(snaps, 3, 4)
    F = M.SCOPE_F_LEVEL | M.SCOPE_F_PEAK
    dev = device_rows(tg.signal_of(W, H), (W, H))
    e = series_engine(M, W, H, 3, 8, fields=F)
    assert e.scope_series_config() == (3, 8, F)
    feed(e, dev, [2 * H + 9, NA * H + 5 - (2 * H + 9)])
    got, n, d = e.scope_series()
    assert (n, d) == (4, 0) and sorted(got) == ["level", "peak"] and equal(got, want, ("level", "peak"))
    assert equal(e.scope_read(), final)
    rc, out, _, _ = raw(M, e, 8, ("level", "phase"))
    assert rc == M.engine.ERR_ARG and (bits(out["level"]) == bits(SENT)).all()
    for name in ("lr", "plevel", "power_l", "power_r"):
        assert raw(M, e, 8, (name,))[0] == M.engine.ERR_ARG, name
    # sub-ranges of the streams
    for first, count in ((0, 2), (2, 3), (4, 1), (1, 0)):
        sub, n, d = e.scope_series(first, count)
        assert (n, d) == (4, 0)
        assert equal(sub, {k: v[first:first + count] for k, v in want.items()}, ("level", "peak")), (first, count)
    with pytest.raises(M.EngineError) as err:
        e.scope_series(3, 3)
    assert err.value.code == M.engine.ERR_ARG
    e.close()
    # every field alone
    for k, name in enumerate(NAMES):
        got, n, d, last = run_series(M, W, H, 3, cap=8, fields=1 << k)
        assert (n, d) == (4, 0) and list(got) == [name] and equal(got, want, (name,)) and equal(last, final), name


# ---- controls --------------------------------------------------------------------------------------------------------------------------

def test_controls(M):
    E = M.engine
    W, H = 1024, 777
    snaps, final = snapshots(W, H)
    want = expected(snaps, 3, 4)
    dev = device_rows(tg.signal_of(W, H), (W, H))
    T = NA * H + 5
    e = M.Engine(S, float(FS), M.METER_SCOPE)
    e.scope_configure(W, H)
    assert e.scope_series_config() == (0, 0, 0)
    with pytest.raises(M.EngineError) as err:                          # the getter with the series off
        e.scope_series()
    assert err.value.code == E.ERR_ARG
    for bad in ((3, 8, 0), (3, 8, 128), (3, 8, 0x80000001), ((1 << 20) + 1, 8, 127)):
        with pytest.raises(M.EngineError) as err:
            e.scope_set_series(*bad)
        assert err.value.code == E.ERR_ARG, bad
    assert e.scope_series_config() == (0, 0, 0)
    e.scope_set_series(1 << 20, 2, M.SCOPE_F_PEAK)                     # (the largest K)
    assert e.scope_series_config() == (1 << 20, 2, M.SCOPE_F_PEAK)
    e.scope_set_series(0)
    assert e.scope_series_config() == (0, 0, 0)
    e.scope_set_series(3, 8)
    feed(e, dev, [T])
    first = e.scope_series()
    assert first[1:] == (4, 0) and equal(first[0], want)
    for args in ((3, 8, 127), (0, 0, 0)):
        with pytest.raises(M.EngineError) as err:                      # after a process call
            e.scope_set_series(*args)
        assert err.value.code == E.ERR_STATE
    # the two resets empty the series and the open group (13 = 4 * 3 + 1) and keep the settings
    for reset in (e.reset, e.scope_reset):
        reset()
        assert e.scope_series_config() == (3, 8, 127)
        got, n, d = e.scope_series()
        assert (n, d) == (0, 0) and got["level"].shape == (S, 0, W // 2)
        feed(e, dev, [5 * H + 1, T - (5 * H + 1)])
        got, n, d = e.scope_series()
        assert (n, d) == (4, 0) and equal(got, want) and equal(e.scope_read(), final)
    e.close()
    e = M.Engine(S, float(FS), M.METER_STCORR)                         # an engine without SCOPE
    with pytest.raises(M.EngineError) as err:
        e.scope_set_series(3, 8)
    assert err.value.code == E.ERR_ARG
    with pytest.raises(M.EngineError) as err:
        e.scope_series_config()
    assert err.value.code == E.ERR_ARG
    e.close()
    # scope_configure to another window keeps K, the capacity and the fields; the rings are the new window's
    e = M.Engine(S, float(FS), M.METER_SCOPE)
    e.scope_set_series(3, 8)
    e.scope_configure(256, 777)
    assert e.scope_series_config() == (3, 8, 127)
    feed(e, device_rows(tg.signal_of(256, 777), (256, 777)), [T])
    got, n, d = e.scope_series()
    assert (n, d) == (4, 0) and equal(got, expected(snapshots(256, 777)[0], 3, 4))
    e.close()


# ---- state -----------------------------------------------------------------------------------------------------------------------------

def test_state(M):
    W, H, K = 1024, 777, 3
    snaps, final = snapshots(W, H)
    dev = device_rows(tg.signal_of(W, H), (W, H))
    T = NA * H + 5
    head = 5 * H + 3                                                   # five analyses: one point, two analyses into the next group
    e = series_engine(M, W, H, K, 8)
    feed(e, dev, [head])
    assert e.scope_series()[1:] == (1, 0)
    blob = e.state_export()
    e.close()
    e = series_engine(M, W, H, 5, 8)
    with pytest.raises(M.EngineError) as err:
        e.state_import(blob)
    assert err.value.code == M.engine.ERR_STATE
    e.close()
    e = series_engine(M, W, H, K, 5, fields=M.SCOPE_F_ALL & ~M.SCOPE_F_LR)   # (fields and capacity need not match)
    e.state_import(blob)
    feed(e, dev, [T - head], head)
    got, n, d = e.scope_series()
    names = [n_ for n_ in NAMES if n_ != "lr"]
    assert (n, d) == (3, 0) and equal(got, expected(snaps, K, 3, first=1), names) and equal(e.scope_read(), final)
    # an engine that has processed must stand at the same analyses since its last point
    two = series_engine(M, W, H, K, 8)
    feed(two, dev, [4 * H + 3])                                        # (one analysis into the group, not two)
    with pytest.raises(M.EngineError) as err:
        two.state_import(blob)
    assert err.value.code == M.engine.ERR_STATE
    two.close()
    e.close()
    # with the series off the blob is what an engine that never heard of the series exports
    blobs = []
    for touch in (False, True):
        e = M.Engine(S, float(FS), M.METER_SCOPE)
        e.scope_configure(W, H)
        if touch:
            e.scope_set_series(K, 8)
            e.scope_set_series(0)
        feed(e, dev, [head])
        blobs.append(bytes(e.state_export()))
        e.close()
    assert len(blobs[0]) == len(blobs[1]) and blobs[0] == blobs[1]
    assert len(blob) == len(blobs[0]) + S * 8                          # (the series' section: K and the analyses since the last point)


# ---- beside other meters and routes ----------------------------------------------------------------------------------------------------

def test_company(M):
    W, H, K = 1024, 777, 3
    snaps, final = snapshots(W, H)
    dev = device_rows(tg.signal_of(W, H), (W, H))
    T = NA * H + 5
    meters = M.METER_SCOPE | M.METER_STCORR | M.METER_KMETER
    others = []
    for with_series in (True, False):
        e = M.Engine(S, float(FS), meters)
        e.scope_configure(W, H)
        if with_series:
            e.scope_set_series(K, 8)
        feed(e, dev, [2 * H + 1, T - (2 * H + 1)])
        e.sync()
        if with_series:
            got, n, d = e.scope_series()
            assert (n, d) == (4, 0) and equal(got, expected(snaps, K, 4))
        assert equal(e.scope_read(), final)
        others.append((e.stcorr_read(), e.kmeter_read()))
        e.close()
    for a, b in zip(*others):
        for u, v in zip(a, b):
            assert np.array_equal(bits(u), bits(v))


def test_host_path_in_several_views(M):
    W, H, K = 1024, 777, 3
    snaps, final = snapshots(W, H)
    x = tg.signal_of(W, H)
    T = x.shape[1]
    e = series_engine(M, W, H, K, 8)
    e.set_host_chunk_bytes(2 * T * 8)                                  # (two streams per view: three views)
    head = 4 * H + 11
    e.process(np.ascontiguousarray(x[:, :head]))
    e.process(np.ascontiguousarray(x[:, head:]))
    e.sync()
    got, n, d = e.scope_series()
    assert (n, d) == (4, 0) and equal(got, expected(snaps, K, 4)) and equal(e.scope_read(), final)
    e.close()


def test_non_finite_samples_stay_in_their_stream(M):
    W, H = 1024, 777
    snaps, _ = snapshots(W, H)
    y = np.array(tg.signal_of(W, H))
    y[2, 3 * H + 11, 1] = np.nan
    y[2, 7 * H + 5, 0] = np.inf
    got, n, d, _ = run_series(M, W, H, 1, x=y)
    want = expected(snaps, 1, NA)
    assert (n, d) == (NA, 0)
    for s in (0, 1, 3, 4):
        assert all(np.array_equal(bits(got[name][s]), bits(want[name][s])) for name in NAMES), s
    assert all(np.array_equal(bits(got[name][2, :3]), bits(want[name][2, :3])) for name in NAMES)   # (before the first of them)
    assert np.isnan(got["level"][2, 4:, 1:W // 2 - 1]).all()
