"""Track lengths for the scope on the GPU (include/mtr_any.h: mtr_engine_process_*_any, mtr_engine_scope_points; the ENDS instantiations
of k_scope, mtr_scope.hip).

The yardstick is exact.  Every analysis is a function of its W frames and the carried state alone, so stream s of a batch whose streams
end at their own frames must be — bit for bit, in all seven arrays of scope_read and in every point of the series — what an engine of ONE
stream gives that was fed exactly that stream's own frames through plain process_device in the same cuts: the dense kernel, which
tests/test_gpu_scope.py holds against the restatement of tests/_scope.py — the float64 DFT — at every one of the seven windows, so an
ENDS kernel (SHAPES: every window) and a series + ends kernel (test_series_rows_are_the_streams_own_points_then_zeros: every window) that
equal it bit for bit are held to the DFT with it.

S = 6 streams, three calls: 3 H + 5 frames whole; n2 = 4 H + 1 frames through _any with the ends below; H + 9 frames through plain
process_device.  With first = H - 5 — the call-2 frame at which its first analysis ends — the ends are
    [n2, 0, first - 1, first, first + 2 H + 7, n2 - 1]
open; untouched; one frame short of an analysis; exactly on one; mid-hop after three; one frame short of the call (and of nothing else:
four analyses, as the open stream).  Rows are longer than the audio, and NaN stands at and behind every stream's end, inside the call's
buffer too."""
import functools

import numpy as np
import pytest

import _scope

pytestmark = pytest.mark.gpu
FS, S = 48000, 6
# H > W, H > W by less than 2 (H ~ W), H < W with the LDS attribute path; then the other four windows: every ENDS kernel is launched
SHAPES = [(256, 777), (1024, 1920), (8192, 4096), (512, 777), (2048, 1920), (4096, 777), (16384, 4096)]
NAMES = ("level", "lr", "phase", "plevel", "peak", "power_l", "power_r")
ERR_ARG, ERR_UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def M():
    import meters.lv2_amd as m
    return m


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def calls_of(H):
    n1, n2, n3 = 3 * H + 5, 4 * H + 1, H + 9
    first = H - 5
    ends = [n2, 0, first - 1, first, first + 2 * H + 7, n2 - 1]
    return (n1, n2, n3), ends


@functools.lru_cache(maxsize=None)
def signal_of(W, H):
    (n1, n2, n3), _ = calls_of(H)
    x = _scope.signals(n1 + n2 + n3, FS, W, seed=9100 + W + H, S=S)
    x.setflags(write=False)
    return x


def own_frames(H, s):
    """the calls stream s sees: (frames of call 1, of call 2, of call 3)"""
    (n1, n2, n3), ends = calls_of(H)
    return (n1, ends[s], n3 if ends[s] == n2 else 0)


def want_counts(M, H, K, s, upto=3):
    """(analyses, points) of stream s behind its first `upto` calls, by mtr_scope_series_cut on its own frames"""
    fill = since = an = pt = 0
    (n1, n2, n3), _ = calls_of(H)
    for n_call, f in list(zip((n1, n2, n3), own_frames(H, s)))[:upto]:
        a, p = M.scope_series_cut(fill, H, since, K, f)
        an, pt = an + a, pt + p
        if f < n_call:
            break                                                       # closed
        fill, since = (fill + f) % H, (since + a) % K if K else 0
    return an, pt


def poisoned(x, H):
    """[S, T + 37, 2]: the streams' own frames, NaN at and behind every end"""
    (n1, n2, n3), ends = calls_of(H)
    T = n1 + n2 + n3
    buf = np.full((S, T + 37, 2), np.nan, np.float32)
    for s in range(S):
        n = sum(own_frames(H, s))
        buf[s, :n] = x[s, :n]
    return buf


def engine(M, W, H, K=0, cap=0, fields=None, n=S, meters=None):
    e = M.Engine(n, float(FS), M.METER_SCOPE if meters is None else meters)
    e.scope_configure(W, H, _scope.THRESH)
    if K:
        e.scope_set_series(K, cap, M.SCOPE_F_ALL if fields is None else fields)
    return e


def payload(e, s):
    """what stream s carries from call to call, without the blob's own header"""
    hdr = 2 * e.state_bytes(1) - e.state_bytes(2)
    return e.state_export(s, 1)[hdr:]


@functools.lru_cache(maxsize=None)
def alone(W, H, K=0, cap=0):
    """per stream: an engine of that one stream, fed its own frames through process_device in the batch's cuts -> scope_read behind call 2
    and behind call 3, the series, the stream's part of the blob behind call 2"""
    import torch
    import meters.lv2_amd as m
    x = signal_of(W, H)
    st = torch.cuda.current_stream().cuda_stream
    out = []
    for s in range(S):
        fr = own_frames(H, s)
        n = sum(fr)
        row = np.full((1, n + 37, 2), np.nan, np.float32)
        row[0, :n] = x[s, :n]
        dev = torch.from_numpy(row).cuda()
        e = engine(m, W, H, K, cap, n=1)
        pos, reads = 0, []
        for i, f in enumerate(fr):
            if f:
                e.process_device(dev.data_ptr() + pos * 8, f, row.shape[1], st)
            pos += f
            if i == 1:
                reads.append(e.scope_read())
                blob = payload(e, 0)
        reads.append(e.scope_read())
        out.append(dict(after2=reads[0], after3=reads[1], series=e.scope_series()[0] if K else None, blob=blob, analyses=e.scope_analyses()))
        e.close()
        del dev
    return out


def run_batch(M, W, H, K=0, cap=0, host=False, chunk=None, reset_first=False):
    """the three calls on the batch -> (engine, scope_read behind call 2, scope_points behind call 2, blob parts behind call 2)"""
    import torch
    (n1, n2, n3), ends = calls_of(H)
    buf = poisoned(signal_of(W, H), H)
    stride = buf.shape[1]
    fr = np.array(ends, np.uint64)
    e = engine(M, W, H, K, cap)
    if chunk:
        e.set_host_chunk_bytes(chunk)
    if host:
        if reset_first:
            e.process(np.ascontiguousarray(buf[:, :n1 + n2]))
            e.reset()
        e.process(np.ascontiguousarray(buf[:, :n1]))
        e.process_any(np.ascontiguousarray(buf[:, n1:n1 + n2]), fr)
        mid = (e.scope_read(), e.scope_points(), [payload(e, s) for s in range(S)])
        e.process(np.ascontiguousarray(buf[:, n1 + n2:n1 + n2 + n3]))
    else:
        dev = torch.from_numpy(buf).cuda()
        st = torch.cuda.current_stream().cuda_stream
        if reset_first:                                                 # (the rings then hold older points behind every stream's own)
            e.process_device(dev.data_ptr(), n1 + n2, stride, st)
            e.reset()
        e.process_device(dev.data_ptr(), n1, stride, st)
        e.process_device_any(dev.data_ptr() + n1 * 8, n2, fr, stride, st)
        mid = (e.scope_read(), e.scope_points(), [payload(e, s) for s in range(S)])
        e.process_device(dev.data_ptr() + (n1 + n2) * 8, n3, stride, st)
        e.sync()
        del dev
    return (e,) + mid


# ---- every stream is its own engine ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W,H", SHAPES)
def test_every_stream_is_what_an_engine_of_its_own_gives(M, W, H):
    (n1, n2, n3), ends = calls_of(H)
    ref = alone(W, H)
    e, mid, (an2, pt2), blobs = run_batch(M, W, H)
    B = W // 2
    scope_bytes = W * 8 + 6 * B * 4 + 4                                 # tail, six arrays of B, peak: the stream's entry behind the scope's header
    for s in range(S):
        for name in NAMES:
            assert same(mid[name][s], ref[s]["after2"][name][0]), (s, name, "behind call 2")
        assert an2[s] == want_counts(M, H, 0, s, upto=2)[0] == ref[s]["analyses"] - (1 if s == 0 else 0), s
        # the stream's part of the blob: the tail — the W frames in front of its own end — and the arrays (the header in front of them
        # holds the engine's lock-step cursors), and nothing in it is NaN: no frame at or behind the end was read
        assert blobs[s][-scope_bytes:] == ref[s]["blob"][-scope_bytes:], s
        assert blobs[s][:-scope_bytes - 24] == ref[s]["blob"][:-scope_bytes - 24], s
        assert not np.isnan(np.frombuffer(blobs[s][-scope_bytes:], np.float32)).any(), s
    assert not pt2.any()
    assert an2.tolist() == [7, 3, 3, 4, 6, 7]
    frames, closed = e.stream_frames()
    assert closed.tolist() == [False, True, True, True, True, True]
    assert frames.tolist() == [n1 + n2 + n3] + [n1 + f for f in ends[1:]]
    # call 3, dense, has moved stream 0 alone
    end = e.scope_read()
    an3, _ = e.scope_points()
    for name in NAMES:
        assert same(end[name][0], ref[0]["after3"][name][0]), name
        assert not same(end[name][0], mid[name][0]), name
        assert same(end[name][1:], mid[name][1:]), name
    assert an3.tolist() == [8] + an2.tolist()[1:] and e.scope_analyses() == 8
    for s in range(1, S):
        assert payload(e, s)[-scope_bytes:] == blobs[s][-scope_bytes:], s
    # reset: the counts are zeroed, the streams open
    e.reset()
    assert not e.scope_points()[0].any() and not e.stream_frames()[1].any() and e.scope_analyses() == 0
    e.close()


def test_whole_streams_are_the_dense_call(M):
    """frames[s] == n_frames on every stream: bit for bit mtr_engine_process_device, the blob included"""
    import torch
    W, H = 1024, 1920
    (n1, n2, n3), _ = calls_of(H)
    buf = poisoned(signal_of(W, H), H)
    buf[:, :n1 + n2] = signal_of(W, H)[:, :n1 + n2]
    dev = torch.from_numpy(buf).cuda()
    st = torch.cuda.current_stream().cuda_stream
    a, b = engine(M, W, H, 2, 8), engine(M, W, H, 2, 8)
    for e in (a, b):
        e.process_device(dev.data_ptr(), n1, buf.shape[1], st)
    a.process_device(dev.data_ptr() + n1 * 8, n2, buf.shape[1], st)
    b.process_device_any(dev.data_ptr() + n1 * 8, n2, np.full(S, n2, np.uint64), buf.shape[1], st)
    assert a.state_export() == b.state_export() and not b.stream_frames()[1].any()
    ra, rb = a.scope_read(), b.scope_read()
    sa, sb = a.scope_series(), b.scope_series()
    assert all(same(ra[n], rb[n]) and same(sa[0][n], sb[0][n]) for n in NAMES) and sa[1:] == sb[1:] == (3, 0)
    assert all(np.array_equal(u, v) for u, v in zip(a.scope_points(), b.scope_points())) and b.scope_points()[1].tolist() == [3] * S
    a.close()
    b.close()


# ---- the series ----------------------------------------------------------------------------------------------------------------------------

# (1, 16) at every window — the series + ends kernel of each; the two cases at W = 1024 keep the names they had
@pytest.mark.parametrize("W,H,K,cap", [pytest.param(1024, 1920, 1, 16, id="1-16"), pytest.param(1024, 1920, 2, 2, id="2-2")]
                         + [(W, H, 1, 16) for W, H in SHAPES if W != 1024])
def test_series_rows_are_the_streams_own_points_then_zeros(M, W, H, K, cap):
    ref, dense = alone(W, H, K, cap), alone(W, H)                      # (one-stream engines: the series kernel, the dense kernel)
    e, mid, (an2, pt2), _ = run_batch(M, W, H, K, cap, reset_first=True)
    got, n, d = e.scope_series()
    total = 8 // K                                                      # the open stream's: lock-step
    assert (n, d) == (total, max(0, total - cap))
    an, pt = e.scope_points()
    for s in range(S):
        assert (an[s], pt[s]) == want_counts(M, H, K, s), s
        own = min(int(pt[s]), cap)
        for name in NAMES:
            assert got[name].shape[:2] == (S, min(total, cap))
            assert same(got[name][s, :own], ref[s]["series"][name][0, :own]), (s, name)
            assert (bits(got[name][s, own:]) == 0).all(), (s, name)     # 0.0f behind a closed stream's own points
            assert same(mid[name][s], ref[s]["after2"][name][0]), (s, name)
            assert same(mid[name][s], dense[s]["after2"][name][0]), (s, name)
    assert an.tolist() == [8, 3, 3, 4, 6, 7] and pt.tolist() == [v // K for v in (8, 3, 3, 4, 6, 7)]
    if K == 2:
        assert d == 2 and (pt > cap).any() and (pt < cap).any()
    e.close()


# ---- paths and state -----------------------------------------------------------------------------------------------------------------------

def test_the_host_form_is_the_device_form(M):
    W, H = 1024, 1920
    (n1, n2, n3), _ = calls_of(H)
    d, dmid, dpts, dblobs = run_batch(M, W, H, 1, 16)
    h, hmid, hpts, hblobs = run_batch(M, W, H, 1, 16, host=True, chunk=2 * ((n2 + 1) & ~1) * 8)     # two streams per view: three views
    assert dblobs == hblobs and d.state_export() == h.state_export()
    assert all(np.array_equal(u, v) for u, v in zip(d.scope_points(), h.scope_points()))
    rd, rh, sd, sh = d.scope_read(), h.scope_read(), d.scope_series(), h.scope_series()
    assert all(same(rd[n], rh[n]) and same(sd[0][n], sh[0][n]) and same(dmid[n], hmid[n]) for n in NAMES) and sd[1:] == sh[1:]
    assert np.array_equal(d.stream_frames()[1], h.stream_frames()[1])
    d.close()
    h.close()


def test_beside_the_other_meters_each_gets_what_tpb_gives(M):
    """a SCOPE | STCORR | KMETER | TPBALLIST engine through _any against the engine without SCOPE through _tpb; the scope beside them is
    the scope alone"""
    import torch
    W, H = 1024, 1920
    (n1, n2, n3), ends = calls_of(H)
    buf = poisoned(signal_of(W, H), H)
    dev = torch.from_numpy(buf).cuda()
    st = torch.cuda.current_stream().cuda_stream
    others = M.METER_STCORR | M.METER_KMETER | M.METER_TPBALLIST
    fr = np.array(ends, np.uint64)
    a = engine(M, W, H, meters=M.METER_SCOPE | others)
    b = M.Engine(S, float(FS), others)
    for e, call in ((a, a.process_device_any), (b, b.process_device_tpb)):
        e.process_device(dev.data_ptr(), n1, buf.shape[1], st)
        call(dev.data_ptr() + n1 * 8, n2, fr, buf.shape[1], st)
        e.process_device(dev.data_ptr() + (n1 + n2) * 8, n3, buf.shape[1], st)
    b_blob = b.state_export()                                           # (before kmeter_read arms the flags in it)
    assert bytes(a.results()) == bytes(b.results())
    for u, v in zip(a.stcorr_read() + a.kmeter_read(), b.stcorr_read() + b.kmeter_read()):
        assert same(u, v) and not np.isnan(u).any()
    ref, got = alone(W, H), a.scope_read()
    for s in range(S):
        assert all(same(got[n][s], ref[s]["after3"][n][0]) for n in NAMES), s
    # an engine whose mask _tpb takes: _any is _tpb, the blob included
    c = M.Engine(S, float(FS), others)
    c.process_device(dev.data_ptr(), n1, buf.shape[1], st)
    c.process_device_any(dev.data_ptr() + n1 * 8, n2, fr, buf.shape[1], st)
    c.process_device(dev.data_ptr() + (n1 + n2) * 8, n3, buf.shape[1], st)
    assert c.state_export() == b_blob and bytes(c.results()) == bytes(b.results())
    for e in (a, b, c):
        e.close()


def test_an_imported_stream_is_open_again(M):
    import torch
    W, H, K = 1024, 1920, 2
    (n1, n2, n3), ends = calls_of(H)
    e, mid, _, _ = run_batch(M, W, H, K, 8)
    assert e.stream_frames()[1].tolist() == [False] + [True] * (S - 1)
    an0, pt0 = e.scope_points()
    blob = e.state_export(2, 2)
    assert e.state_import(blob, 2) == 2
    assert e.stream_frames()[1].tolist() == [False, True, False, False, True, True]
    an, pt = e.scope_points()
    assert an.tolist() == [8, 3, 8, 8, 6, 7] and pt.tolist() == [4, 1, 4, 4, 3, 3]      # (the lock-step numbers)
    before = e.scope_read()
    x = signal_of(W, H)
    dev = torch.from_numpy(np.ascontiguousarray(x[:, :2 * H])).cuda()
    e.process_device(dev.data_ptr(), 2 * H, 2 * H, torch.cuda.current_stream().cuda_stream)
    after = e.scope_read()
    moved = [not same(after["level"][s], before["level"][s]) for s in range(S)]
    assert moved == [True, False, True, True, False, False]
    assert e.scope_points()[0].tolist() == [10, 3, 10, 10, 6, 7]
    e.close()


def test_the_older_pairs_refuse_and_any_checks_its_arguments(M):
    W, H = 256, 777
    n = 2 * H
    x = np.ascontiguousarray(signal_of(W, H)[:, :n])
    full = np.full(S, n, np.uint64)

    def refused(code, f, *args):
        with pytest.raises(M.EngineError) as err:
            f(*args)
        assert err.value.code == code, (err.value.code, str(err.value))

    e = engine(M, W, H, 1, 4)
    e.process(x[:, :H + 3])
    before = (e.state_export(), e.scope_points()[0].tolist(), e.stream_frames()[0].tolist())
    for f in (e.process_lengths, e.process_tracks, e.process_ragged, e.process_ends, e.process_tpb):
        refused(ERR_UNSUPPORTED, f, x, full)
    long = full.copy()
    long[3] = n + 1
    refused(ERR_ARG, e.process_any, x, long)
    assert M.lib.mtr_engine_process_host_any(e._h, x.ctypes.data, n, n, None) == ERR_ARG
    assert M.lib.mtr_last_error() == b"mtr_engine_process_host_any: null argument"
    assert M.lib.mtr_engine_process_device_any(e._h, None, n, n, full.ctypes.data, None) == ERR_ARG
    assert M.lib.mtr_last_error() == b"mtr_engine_process_device_any: null argument"
    refused(ERR_ARG, e.scope_points, 2, S)
    assert (e.state_export(), e.scope_points()[0].tolist(), e.stream_frames()[0].tolist()) == before
    e.close()
    with M.Engine(S, float(FS), M.METER_STCORR) as o:
        refused(ERR_ARG, o.scope_points)


def test_a_five_channel_loudness_engine_gets_what_lengths_gives(M):
    rng = np.random.default_rng(77)
    n = 7000
    x = (rng.standard_normal((S, n, 5)) * 0.2).astype(np.float32)
    fr = np.array([n, 0, 1, 2400, 4801, n - 1], np.uint64)
    y = x.copy()
    for s in range(S):
        y[s, int(fr[s]):] = np.nan
    meters = M.METER_EBU | M.METER_TRUEPEAK
    with M.Engine(S, float(FS), meters, n_channels=5) as a, M.Engine(S, float(FS), meters, n_channels=5) as b:
        for e, call in ((a, a.process_any), (b, b.process_lengths)):
            e.integr_start()
            e.process(x[:, :3000])
            call(y, fr)
            e.process(x[:, :1000])
        assert a.state_export() == b.state_export() and bytes(a.results()) == bytes(b.results())
        assert np.array_equal(a.stream_frames()[0], b.stream_frames()[0]) and a.stream_frames()[1].tolist() == [False] + [True] * (S - 1)
        assert not np.isnan(a.out9()).any()
