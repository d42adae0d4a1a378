"""The 30-band bank's reading series (mtr_engine_spectr_set_period / _period / _series, include/mtr_spectr.h; the second instantiation
of k_bank) on the GPU.  The engine's points are held three ways:
  * against the oracle's call-by-call handle fed in blocks of P (MTR_SPECTR_PEAK_BLOCK: reset_peak () after every read), on ALL streams,
    with tests/test_gpu_bank.py's contract: val, max rtol = BANK_REL, atol = BANK_ATOL; val_db, max_db DB_TOL where the oracle is above
    DB_FLOOR.  tests/test_bank_series_cpu.py holds the condition under which this sees a block end that is one frame off.
  * bit for bit against the engine WITHOUT a period, fed calls of exactly P frames with mtr_engine_spectrum (and, PEAK_BLOCK,
    mtr_engine_spectr_reset_peak) after each: the existing path, not the code under test.
  * bit for bit against itself however the calls cut the audio — one call, the programme of tests/_bank.py, calls of one frame around a
    block end — the final mtr_engine_spectrum included.
Shapes are tiny: 2227 frames (tests/_bank.CALLS), 1 .. 33 streams."""
import ctypes as C

import numpy as np
import pytest

import _bank as B
import _bank_series as BS
from test_gpu_parity import M  # noqa: F401  (M: the module fixture)

pytestmark = pytest.mark.gpu

T = B.T_CALLS
ERR_ARG, ERR_UNSUPPORTED, ERR_STATE = -1, -2, -7
MODES = [BS.HOLD, BS.BLOCK]
MODE_IDS = ["hold", "block"]
TINY = np.float32(1e-20)


def batch(S, T=T):
    return np.stack([B.stream_input(s, T) for s in range(S)])


def check(got, want, what):
    """the contract above on [S, points, 30] arrays"""
    for k in BS.KEYS:
        assert got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        assert np.isfinite(got[k]).all(), (what, k)
    for k in ("val", "max"):
        g, w = got[k].astype(np.float64), want[k].astype(np.float64)
        if g.size:
            big = w > 1e-25
            print("%-4s %-52s worst relative deviation %.3g" % (k, what, float((np.abs(g - w)[big] / w[big]).max()) if big.any() else 0.0))
        assert np.allclose(g, w, rtol=B.BANK_REL, atol=B.BANK_ATOL), (what, k, float(np.abs(g - w).max()))
    for k in ("val_db", "max_db"):
        live = want[k] > B.DB_FLOOR
        assert np.allclose(got[k][live], want[k][live], atol=B.DB_TOL), (what, k)


def around(P, T=T):
    """calls of one frame on both sides of a block end (the first, or where P > T the call's own end), the rest in two calls"""
    k = min(P, T)
    head = [k - 2] if k > 2 else []
    ones = [1] * min(4, T - sum(head))
    rest = T - sum(head) - len(ones)
    return head + ones + ([rest // 2, rest - rest // 2] if rest > 1 else [rest] if rest else [])


# ---- a. P x lanes x width x mode: oracle, the dense engine, the cuts ------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("mono", [False, True], ids=["stereo", "mono"])
@pytest.mark.parametrize("S", [1, 3, 33])
@pytest.mark.parametrize("P", [100, 128, 129, 300, 2227, 5000])
def test_series_oracle_dense_and_cuts(M, oracle, P, S, mono, mode):  # noqa: F811
    x = batch(S)
    what = "P=%d S=%d %s %s" % (P, S, "mono" if mono else "stereo", MODE_IDS[mode])
    n = T // P
    one = BS.through(M, x, P, [T], mode=mode, mono=mono)
    assert (one[1], one[2]) == (n, 0) and one[0]["val"].shape == (S, n, B.NBANDS)
    check(one[0], BS.stack([BS.reference(oracle, s, T, P, mode, mono) for s in range(S)]), what)
    assert BS.same(one[0], BS.dense(M, x, P, mode, mono=mono)), what + ": not the dense engine fed calls of P frames"
    for calls in (B.CALLS, around(P)):
        assert sum(calls) == T
        got = BS.through(M, x, P, calls, mode=mode, mono=mono)
        assert got[1:3] == one[1:3] and BS.same(got[0], one[0]), (what, calls)
        assert BS.same(got[3], one[3]), (what, calls, "the final mtr_engine_spectrum")
    if n == 0:                                                   # no point, the block still open: the levels as they stand (no epilogue yet)
        check({k: v[:, None] for k, v in one[3].items()}, BS.stack([BS.reference(oracle, s, T, T, BS.HOLD, mono) for s in range(S)]), what + " open block")


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_a_period_of_one_frame(M, oracle, mode):  # noqa: F811
    """P = 1 on the first 40 frames: every frame ends a block"""
    S, n = 3, 40
    x = batch(S)[:, :n]
    one = BS.through(M, x, 1, [n], mode=mode)
    assert (one[1], one[2]) == (n, 0)
    check(one[0], BS.stack([BS.oracle_series(oracle, x[s], 1, mode) for s in range(S)]), "P=1 %s" % MODE_IDS[mode])
    assert BS.same(one[0], BS.dense(M, x, 1, mode))
    got = BS.through(M, x, 1, [1, 2, 37], mode=mode)
    assert BS.same(got[0], one[0]) and BS.same(got[3], one[3])
    if mode == BS.BLOCK:                                         # the hold starts again with every frame: max is the level
        assert np.allclose(one[0]["max"], one[0]["val"], rtol=1e-6, atol=2e-20)      # (val carries the + 1e-20f, max does not)


# ---- b. overflow ----------------------------------------------------------------------------------------------------------------------

def test_points_past_the_capacity_are_dropped_and_counted(M):  # noqa: F811
    S, P = 3, 100
    x = batch(S)
    full = BS.through(M, x, P, B.CALLS, cap=64)
    assert (full[1], full[2]) == (22, 0)
    short = BS.through(M, x, P, B.CALLS, cap=16)
    assert (short[1], short[2]) == (22, 6) and short[0]["val"].shape == (S, 16, B.NBANDS)
    # the kept points are the first 16 — of EVERY stream: a point written past a stream's row would have landed in the next stream's first points
    assert BS.same(short[0], {k: v[:, :16] for k, v in full[0].items()}) and BS.same(short[3], full[3])
    none = BS.through(M, x, P, B.CALLS, cap=0)
    assert (none[1], none[2]) == (22, 22) and none[0]["val"].shape == (S, 0, B.NBANDS) and BS.same(none[3], full[3])
    # the caller's rows: the first min (n_points, capacity, capacity_points) points are copied, the rest is left as it was
    with M.Engine(S, 48000.0, M.METER_SPECTR30) as e:
        e.spectr_set_speed(B.SPEED)
        e.spectr_set_period(P, 16)
        e.process(x)
        for capacity, kept in ((20, 16), (10, 10)):
            rows = [np.full((S, capacity, B.NBANDS), 7.0, np.float32) for _ in range(4)]
            n, d = C.c_uint32(), C.c_uint32()
            assert M.lib.mtr_engine_spectr_series(e._h, 0, S, *[r.ctypes.data for r in rows], capacity, C.byref(n), C.byref(d)) == 0
            assert (n.value, d.value) == (22, 6)
            for r, k in zip(rows, BS.KEYS):
                assert np.array_equal(BS.bits(r[:, :kept]), BS.bits(full[0][k][:, :kept])) and (r[:, kept:] == 7.0).all(), (capacity, k)
        only = np.full((1, 16, B.NBANDS), 7.0, np.float32)       # one array of the four, a window of the streams
        assert M.lib.mtr_engine_spectr_series(e._h, 2, 1, None, None, only.ctypes.data, None, 16, None, None) == 0
        assert np.array_equal(BS.bits(only[0]), BS.bits(full[0]["val_db"][2, :16]))


# ---- c. levels: silence, non-finite input -----------------------------------------------------------------------------------------------

def test_silence_with_cuts_inside_the_blocks(M, oracle):  # noqa: F811
    """The levels are the dither's and the epilogues' + 1e-20f alone (about 7e-20): one epilogue too many, too few or at a call's end
    instead of a block's is a deviation of the order of the value itself."""
    calls = [64] * 10 + [1, 3, 300]
    n, P = sum(calls), 100
    zero = np.zeros((2, n, 2), np.float32)
    got = BS.through(M, zero, P, calls, speed=None)
    assert got[1] == n // P
    want = BS.stack([BS.oracle_series(oracle, zero[s], P, speed=None) for s in range(2)])
    assert (want["val"] >= TINY).all() and (want["val"] < 2e-19).all() and (want["val"][:, -1] > 5 * TINY).all()
    check(got[0], want, "silence")
    assert (got[0]["val_db"] == -100.0).all() and (got[0]["max_db"] == -100.0).all()
    assert BS.same(got[0], BS.dense(M, zero, P, speed=None)) and BS.same(got[0], BS.through(M, zero, P, [n], speed=None)[0])


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_non_finite_input_inside_a_block(M, oracle, mode):  # noqa: F811
    """P = 300: a NaN and an Inf inside block 2 (frames 600 .. 899), an Inf at its last frame, a NaN at its first — that block's point
    and the following ones against the oracle's block-wise scrub (spectrumlv2.c:230-238), in the manner of test_non_finite_input"""
    S, P = 5, 300
    x = batch(S)
    x[0, 700, 0] = np.nan
    x[1, 700, :] = np.inf
    x[2, 899, 1] = -np.inf
    x[3, 600, :] = np.nan
    got = BS.through(M, x, P, B.CALLS, mode=mode)
    want = BS.stack([BS.oracle_series(oracle, x[s], P, mode) for s in range(S)])
    check(got[0], want, "non-finite %s" % MODE_IDS[mode])        # (no NaN / Inf ever leaves the getter: check () asserts it)
    v, m = got[0]["val"], got[0]["max"]
    assert (v[:4, 2] == TINY).all() and (want["val"][:4, 2] == TINY).all() and (got[0]["val_db"][:4, 2] == -100.0).all()
    assert not m[[1, 2], 2].any() and not want["max"][[1, 2], 2].any()          # an Inf wins the compare, the scrub zeroes the hold
    if mode == BS.HOLD:
        assert (m[[0, 3], 2] >= m[[0, 3], 1]).all() and (m[[0, 3], 2] > 0).all()   # a NaN loses it: the hold stands
    # the clean stream beside them, and the blocks behind the scrub (the bands from 1 kHz up: they answer within a block of 300 frames)
    assert (v[4, :, 15:] > 1e3 * TINY).all() and (v[:4, 3:, 15:] > 1e3 * TINY).all()
    assert BS.same(got[0], BS.dense(M, x, P, mode)) and BS.same(got[0], BS.through(M, x, P, [T], mode=mode)[0])


# ---- d. the routes ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mono", [False, True], ids=["stereo", "mono"])
def test_device_buffers_with_padding_and_offset(M, oracle, mono):  # noqa: F811
    """process_device on [S = 18][stride] frames, the padding NaN, the base one frame past the allocation's start, in two calls; equal to
    the oracle, and to the host path bit for bit"""
    import torch
    S, P, W = 18, 129, 1 if mono else 2
    x = batch(S)
    xs = BS.feed(mono, x)
    stride = T + 7
    pad = np.full((1 + S * stride) * W, np.nan, np.float32)
    rows = pad[W:].reshape(S, stride, W) if not mono else pad[W:].reshape(S, stride)
    rows[:, :T] = xs
    d = torch.from_numpy(pad).cuda()
    st = torch.cuda.current_stream().cuda_stream

    def device(e, a, b):
        e.process_device(d.data_ptr() + 4 * W * (1 + a), b - a, stride, st)

    for mode in MODES:
        got = BS.through(M, x, P, [385, T - 385], mode=mode, mono=mono, process=device)
        assert got[1] == T // P
        check(got[0], BS.stack([BS.reference(oracle, s, T, P, mode, mono) for s in range(S)]), "device %s %s" % ("mono" if mono else "stereo", MODE_IDS[mode]))
        host = BS.through(M, x, P, [385, T - 385], mode=mode, mono=mono)
        assert BS.same(got[0], host[0]) and BS.same(got[3], host[3])
    del d


def test_host_path_in_several_views(M):  # noqa: F811
    """mtr_engine_set_host_chunk_bytes small enough for three streams per view: every view cuts its blocks where the CALL started and
    appends at the same points; the series' overflow included"""
    S, P = 33, 100
    x = batch(S)

    def small(e, a, b):
        e.set_host_chunk_bytes(3 * (b - a) * 8)
        e.process(np.ascontiguousarray(x[:, a:b]))

    for cap in (64, 16):
        whole = BS.through(M, x, P, B.CALLS, cap=cap, mode=BS.BLOCK)
        views = BS.through(M, x, P, B.CALLS, cap=cap, mode=BS.BLOCK, process=small)
        assert views[1:3] == whole[1:3] == (22, max(0, 22 - cap)) and BS.same(views[0], whole[0]) and BS.same(views[3], whole[3])


def test_integer_pcm_and_a_frame_layout(M):  # noqa: F811
    """16-bit PCM in 4-channel frames of which the engine meters channels (2, 0): the series of the float path on the decoded pick"""
    S, P = 3, 129
    rng = np.random.default_rng(8300)
    raw = rng.integers(-20000, 20000, (S, T, 4)).astype(np.int16)
    x = M.pick_decode(M.PCM_S16, raw, [2, 0])

    def pcm(e, a, b):
        if a == 0:
            e.set_frame_layout(4, [2, 0])
        e.process_pcm(np.ascontiguousarray(raw[:, a:b]))

    got = BS.through(M, x, P, B.CALLS, process=pcm)
    want = BS.through(M, x, P, B.CALLS)
    assert got[1] == T // P and BS.same(got[0], want[0]) and BS.same(got[3], want[3])


# ---- e. controls ------------------------------------------------------------------------------------------------------------------------

def test_controls_between_calls_inside_a_block(M, oracle):  # noqa: F811
    """set_speed and reset_peak between calls that end mid-block, against handles that are fed the same pieces and read at the blocks'
    ends.  A handle's run () that ends mid-block adds its epilogue's 1e-20f to val there, which the engine does not (in the first block's
    low bands that is the level itself): it is taken off the handle's val_f again, exact to an ulp."""
    S, P = 3, 300
    x = batch(S)
    calls = [250, 100, 475, 2, 1400]                             # the calls end at 250, 350, 825, 827, 2227: inside blocks 0, 1, 2, 2, 7
    ctl = {0: ("speed", 2.0), 1: ("reset_peak",), 2: ("speed", 100.0), 3: ("reset_peak",)}   # behind call i

    def after(e, i):
        if i in ctl:
            e.spectr_set_speed(ctl[i][1]) if ctl[i][0] == "speed" else e.spectr_reset_peak()

    ends = np.cumsum(calls)
    cuts = sorted(set(ends.tolist()) | set(range(P, T + 1, P)))
    for mode in MODES:
        got = BS.through(M, x, P, calls, mode=mode, after=after)
        want = []
        for s in range(S):
            h = oracle.spectr_stream(48000.0)
            h.set_speed(B.SPEED)
            pts, pos = [], 0
            for c in cuts:
                r = h.run(x[s, pos:c])
                pos = c
                if c % P == 0:
                    pts.append(r)
                    if mode == BS.BLOCK:
                        h.reset_peak()
                else:
                    for b in range(B.NBANDS):
                        h.s.val_f[b] = float(np.float32(h.s.val_f[b]) - TINY)
                if c in ends and int(np.searchsorted(ends, c)) in ctl:
                    k = ctl[int(np.searchsorted(ends, c))]
                    h.set_speed(k[1]) if k[0] == "speed" else h.reset_peak()
            want.append({k: np.stack([r[k] for r in pts]) for k in BS.KEYS})
        check(got[0], BS.stack(want), "controls %s" % MODE_IDS[mode])
        plain = BS.through(M, x, P, calls, mode=mode)
        assert not np.array_equal(plain[0]["val"][:, 1:], got[0]["val"][:, 1:]) and not np.array_equal(plain[0]["max"][:, 1], got[0]["max"][:, 1])


def test_reset_empties_the_series_and_keeps_the_period(M):  # noqa: F811
    S, P = 3, 129
    x = batch(S)
    fresh = BS.through(M, x, P, B.CALLS, cap=32, mode=BS.BLOCK)
    with M.Engine(S, 48000.0, M.METER_SPECTR30) as e:
        assert e.spectr_period() == (0, 0, BS.HOLD)
        e.spectr_set_speed(B.SPEED)
        e.spectr_set_period(P, 32, BS.BLOCK)
        assert e.spectr_period() == (P, 32, BS.BLOCK)
        e.process(x[:, :700])
        assert e.spectr_series()[1] == 700 // P
        e.reset()
        ser, n, d = e.spectr_series()
        assert (n, d) == (0, 0) and ser["val"].shape == (S, 0, B.NBANDS) and e.spectr_period() == (P, 32, BS.BLOCK)
        assert not e.spectrum()["val"].any()
        pos = 0
        for c in B.CALLS:
            e.process(np.ascontiguousarray(x[:, pos:pos + c]))
            pos += c
        ser, n, d = e.spectr_series()
        assert (n, d) == fresh[1:3] and BS.same(ser, fresh[0]) and BS.same(e.spectrum(), fresh[3])
        # a period is set before the first call only; after a reset it can be, and 0 switches the series off
        with pytest.raises(M.EngineError) as ei:
            e.spectr_set_period(P, 32, BS.HOLD)
        assert ei.value.code == ERR_STATE and e.spectr_period() == (P, 32, BS.BLOCK)
        e.reset()
        e.spectr_set_period(0)
        assert e.spectr_period() == (0, 0, BS.HOLD)
        assert M.lib.mtr_engine_spectr_series(e._h, 0, S, None, None, None, None, 0, None, None) == ERR_ARG


def test_refusals(M):  # noqa: F811
    with M.Engine(2, 48000.0, M.METER_SPECTR30) as e:
        for args in ((100, 4, 2), (100, 4, -1), (0x7fffffff, 4, 0), (0xffffffff, 0, 0)):
            assert M.lib.mtr_engine_spectr_set_period(e._h, *args) == ERR_ARG, args
        assert e.spectr_period() == (0, 0, BS.HOLD)
        assert M.lib.mtr_engine_spectr_series(e._h, 0, 2, None, None, None, None, 0, None, None) == ERR_ARG      # the series is off
        assert M.lib.mtr_engine_spectr_set_period(e._h, 0x7ffffffe, 0, 1) == 0 and e.spectr_period() == (0x7ffffffe, 0, 1)
        assert M.lib.mtr_engine_spectr_series(e._h, 1, 2, None, None, None, None, 0, None, None) == ERR_ARG      # the stream range
    with M.Engine(2, 48000.0, M.METER_KMETER) as e:              # no SPECTR30 in the engine
        assert M.lib.mtr_engine_spectr_set_period(e._h, 100, 4, 0) == ERR_ARG
        assert M.lib.mtr_engine_spectr_period(e._h, None, None, None) == ERR_ARG
        assert M.lib.mtr_engine_spectr_series(e._h, 0, 2, None, None, None, None, 0, None, None) == ERR_ARG


def test_lengths_tracks_and_ragged_still_refuse_the_engine(M):  # noqa: F811
    import torch
    S, n = 4, 600
    x = np.ascontiguousarray(batch(S)[:, :n])
    dev = torch.from_numpy(x).cuda()
    f = np.array([n, 100, 0, n], np.uint64)
    for P in (0, 100):
        with M.Engine(S, 48000.0, M.METER_SPECTR30) as e:
            e.spectr_set_period(P, 8)
            e.process_device(dev.data_ptr(), n)
            before = e.state_export()
            for name in ("lengths", "tracks", "ragged"):
                assert getattr(M.lib, "mtr_engine_process_device_" + name)(e._h, dev.data_ptr(), n, n, f.ctypes.data, 0) == ERR_UNSUPPORTED, (P, name)
                assert getattr(M.lib, "mtr_engine_process_host_" + name)(e._h, x.ctypes.data, n, n, f.ctypes.data) == ERR_UNSUPPORTED, (P, name)
            assert e.state_export() == before and not e.stream_frames()[1].any()
            if P:
                assert e.spectr_series()[1] == n // P
                out = np.zeros(S, np.uint64)                     # (mtr_engine_series_points keeps its three meters)
                assert M.lib.mtr_engine_series_points(e._h, M.METER_SPECTR30, 0, S, out.ctypes.data) == ERR_ARG
    del dev


# ---- f. the state blob ------------------------------------------------------------------------------------------------------------------

def test_without_a_period_the_blob_is_what_it_was(M):  # noqa: F811
    """an engine that never heard of the series, one whose series was switched on and off again: the same bytes; with a period, twelve
    more per stream"""
    S = 3
    x = batch(S)
    with M.Engine(S, 48000.0, M.METER_SPECTR30) as a, M.Engine(S, 48000.0, M.METER_SPECTR30) as b, M.Engine(S, 48000.0, M.METER_SPECTR30) as c:
        b.spectr_set_period(100, 8, BS.BLOCK)
        b.spectr_set_period(0)
        c.spectr_set_period(100, 8, BS.BLOCK)
        for e in (a, b, c):
            e.process(x[:, :777])
        assert [a.state_bytes(k) for k in (0, 1, S)] == [b.state_bytes(k) for k in (0, 1, S)]
        assert a.state_export() == b.state_export()
        per = a.state_bytes(1) - a.state_bytes(0)
        assert c.state_bytes(S) == a.state_bytes(S) + 12 * S
        assert per >= B.NBANDS * (12 * 8 + 4 + 4) + 4             # (the bank's sections: z, val, max, the dither parity)
        with pytest.raises(M.EngineError) as ei:                 # ... and neither takes the other's
            a.state_import(c.state_export())
        assert ei.value.code == ERR_STATE


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_export_inside_a_block_and_continue(M, mode):  # noqa: F811
    S, P, cut = 3, 300, 777                                      # 177 frames into block 2
    x = batch(S)
    whole = BS.through(M, x, P, [cut, T - cut], mode=mode)
    mk = lambda: M.Engine(S, 48000.0, M.METER_SPECTR30)          # noqa: E731
    with mk() as a, mk() as b, mk() as other_p, mk() as other_m, mk() as elsewhere, mk() as there:
        for e, (p, m) in ((a, (P, mode)), (b, (P, mode)), (other_p, (299, mode)), (other_m, (P, 1 - mode)), (elsewhere, (P, mode)), (there, (P, mode))):
            e.spectr_set_speed(B.SPEED)
            e.spectr_set_period(p, 16, m)
        a.process(x[:, :cut])
        blob = a.state_export()
        b.state_import(blob)
        assert BS.same(a.spectrum(), b.spectrum()) and b.spectr_series()[1] == 0      # (the series itself is not part of the blob)
        b.process(x[:, cut:])
        ser, n, d = b.spectr_series()
        assert (n, d) == (whole[1] - cut // P, 0)
        assert BS.same(ser, {k: v[:, cut // P:] for k, v in whole[0].items()}) and BS.same(b.spectrum(), whole[3])
        for e in (other_p, other_m):                             # another period, another mode
            with pytest.raises(M.EngineError) as ei:
                e.state_import(blob)
            assert ei.value.code == ERR_STATE
        elsewhere.process(x[:, :cut - 1])                        # not fresh, and one frame short of where the blob stands
        with pytest.raises(M.EngineError) as ei:
            elsewhere.state_import(blob)
        assert ei.value.code == ERR_STATE
        there.process(x[:, :cut])                                # ... and where it stands
        there.state_import(blob)
