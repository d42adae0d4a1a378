"""The interpolator history itself (k_history, mtr_history.hip): the row a call leaves in the state blob, bit for bit.

Every call of an engine with TRUEPEAK or TPBALLIST ends by keeping the last 47 frames of (old history ++ this call's audio) per stream.
The other tests see that row only through the next call's peaks; here it is read out of mtr_engine_state_export and held against the
numpy restatement: the last 47 frames of concatenate (zeros (47), everything fed so far) under the call's cut rule (HistCut,
mtr_internal.h) —
  call end (dense calls; _lengths calls for every stream with frames [s] != 0, a closing one included: its row holds what FOLLOWS its
            end in the buffer, so those frames carry a pattern of their own here; frames [s] == 0: the row stays),
  own end  (_tpb calls of a TPBALLIST engine: the frames in front of frames [s]; 0: the row stays).
S = 6 streams of distinct noise per stream and channel; dense calls of 1, 45, 1, 47, 48, 130 frames (a row of old history moved on by
one frame, mixed rows, a row that is exactly the call, rows wholly from the call); calls with lengths [0, 1, 46, 47, n - 1, n] of
n = 130 behind a full call of 45, then 48 more for the one stream still open.  Host path (stride = n) and device path (an odd stride
> n, the padding filled with a third pattern).  Nothing here is new behaviour: the test passes on the library before mtr_history.hip
as well (MTR_LIB), 1-frame calls included — no meter set here refuses them."""
import numpy as np
import pytest

import _signals as sig

pytestmark = pytest.mark.gpu

S, H, FS = 6, 47, 48000.0
DENSE = (1, 45, 1, 47, 48, 130)
N = 130
RAGGED = ((45, None), (N, (0, 1, 46, 47, N - 1, N)), (48, (0, 0, 0, 0, 0, 48)))     # (n_frames, frames per stream or None: all n_frames)
STATE, HISTS = 408, 2 * 751 * 4             # sizeof (mtr_stream_state), the two loudness histograms: state_sections, mtr_state.hip
LFE = 7000.0                                # the LFE column of the 5.1 frames: LFE + frame, found nowhere else


@pytest.fixture(scope="module")
def M():
    import meters.lv2_amd as m
    return m


_X = {}


def audio(C):
    """[S, 400, C] float32: noise, distinct per stream and channel"""
    if C not in _X:
        _X[C] = np.stack([np.concatenate([sig.lcg_noise(400, 9000 + 10 * s + k) for k in range((C + 1) // 2)], 1)[:, :C] for s in range(S)])
    return _X[C]


def rows(e, C):
    """[S, 47, HC] float32: the history rows as the blob holds them; the blob's layout is asserted, not trusted"""
    hdr = 2 * e.state_bytes(1) - e.state_bytes(2)
    HC = 2 if C <= 2 else C
    per = STATE + HISTS + H * 2 * 4 + (0 if C <= 2 else C * 16 + H * C * 4 + 2 * C * 4)      # layout 8: + K-filter states, its row, tp_last, tp_hold
    assert e.state_bytes(1) == hdr + per, "the state blob's sections changed: see state_sections (mtr_state.hip)"
    at = hdr + STATE + HISTS + (0 if C <= 2 else H * 2 * 4 + C * 16)
    return np.stack([np.frombuffer(e.state_export(s, 1), np.float32, H * HC, at).reshape(H, HC) for s in range(S)])


def same(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def buffers(C, plan, stride_of, wide=False):
    """per call of `plan` the buffer [S, stride, W]: the next n frames of audio (C), a pattern of its own behind a stream's end inside
    the call (100 + frame + c / 8), another in the padding of the stride (-(100 + frame + c / 8)); wide: 5.1 frames around C = 5"""
    x, out, a = audio(C), [], 0
    for n, frames in plan:
        st = stride_of(n)
        pat = (100.0 + np.arange(st, dtype=np.float32)[None, :, None] + np.arange(C, dtype=np.float32)[None, None, :] / 8) * np.ones((S, 1, 1), np.float32)
        buf = -pat
        buf[:, :n] = pat[:, :n]
        for s in range(S):
            k = n if frames is None else frames[s]
            buf[s, :k] = x[s, a:a + k]
        if wide:
            buf, compact = np.empty((S, st, 6), np.float32), buf
            buf[:, :, [0, 1, 2, 4, 5]] = compact
            buf[:, :, 3] = LFE + np.arange(st, dtype=np.float32)[None, :]
        out.append(np.ascontiguousarray(buf.reshape(S, st) if C == 1 else buf))
        a += n
    return out


def restate(bufs, plan, own_end, C, wide=False):
    """after each call, [S, 47, HC]: the last 47 frames of zeros (47) ++ what each stream has been fed under the rule"""
    HC = 2 if C <= 2 else C
    fed = [[np.zeros((H, HC), np.float32)] for _ in range(S)]
    out = []
    for buf, (n, frames) in zip(bufs, plan):
        buf = buf.reshape(S, buf.shape[1], -1)
        if wide:
            buf = buf[:, :, [0, 1, 2, 4, 5]]
        for s in range(S):
            k = n if frames is None else frames[s]
            if k:
                piece = np.zeros((k if own_end else n, HC), np.float32)          # (mono: the right channel is zero)
                piece[:, :C] = buf[s, :piece.shape[0]]
                fed[s].append(piece)
        out.append(np.stack([np.concatenate(fed[s])[-H:] for s in range(S)]))
    return out


def feed(e, path, family, buf, n, frames):
    """one call: host path (the buffer's first n frames, stride n) or device path (the buffer as it is)"""
    import torch
    f = None if frames is None else np.array(frames, np.uint64)
    if family is not None and f is None:
        f = np.full(S, n, np.uint64)
    if path == "host":
        x = np.ascontiguousarray(buf[:, :n])
        if family is None:
            e.process(x)
        else:
            getattr(e, "process_" + family)(x, f)
        return
    dev = torch.from_numpy(buf).cuda()
    if family is None:
        e.process_device(dev.data_ptr(), n, buf.shape[1])
    else:
        getattr(e, "process_device_" + family)(dev.data_ptr(), n, f, buf.shape[1])
    e.sync()                                                         # (before the buffer goes)


def run(M, meters, C, plan, path, family, own_end=False, wide=False, tail=None, each=None):
    """the rows after every call of `plan`, each held against the restatement; each (e): what else to read after a call"""
    stride_of = (lambda n: n) if path == "host" else (lambda n: (n + 3) | 1)
    bufs = buffers(C, plan, stride_of, wide)
    want = restate(bufs, plan, own_end, C, wide)
    got, extra = [], []
    with M.Engine(S, FS, meters, n_channels=C) as e:
        if tail is not None:
            e.set_deferred_tail(tail)
        if wide:
            e.set_frame_layout(6, [0, 1, 2, 4, 5])
        for k, (buf, (n, frames)) in enumerate(zip(bufs, plan)):
            feed(e, path, family, buf, n, frames)
            got.append(rows(e, C))
            assert same(got[-1], want[k]), (k, n, frames, np.argwhere(got[-1].view(np.uint32) != want[k].view(np.uint32))[:4])
            if each:
                extra.append(each(e))
        if tail is not None:
            assert (e.deferred_calls() > 0) == (tail == 2)
    return got, extra


def dense_plan():
    return [(n, None) for n in DENSE]


PATHS = ["host", "device"]


@pytest.mark.parametrize("path", PATHS)
def test_stereo_truepeak_dense_fold_in_gate_or_in_history(M, path):
    """1. the serial order (k_gate folds the call's peaks) and the deferred tail (k_history does): the same rows, the same peaks after every call"""
    peaks = lambda e: (e.truepeak(),) + e.truepeak_channels()
    a, pa = run(M, M.METER_TRUEPEAK, 2, dense_plan(), path, None, tail=1, each=peaks)
    b, pb = run(M, M.METER_TRUEPEAK, 2, dense_plan(), path, None, tail=2, each=peaks)
    for k in range(len(DENSE)):
        assert same(a[k], b[k]), k
        assert all(same(u, v) for u, v in zip(pa[k], pb[k])), k
        assert pa[k][2].max() > 0                                    # (the call's own peak: a fold that never ran would leave zeros)


@pytest.mark.parametrize("path", PATHS)
def test_stereo_lengths_leave_the_frames_in_front_of_the_calls_end(M, path):
    """2. open or closing: what lies in front of the CALL's end, the buffer's frames behind the stream's own end included; 0 frames: unchanged"""
    got, _ = run(M, M.METER_EBU | M.METER_TRUEPEAK, 2, list(RAGGED), path, "lengths")
    assert same(got[1][0], got[0][0]) and got[0][0].any()            # frames 0: the row of the call before, and that is not empty
    assert (got[1][1:5, -1, 0] == 100.0 + N - 1).all()               # closing streams: the pattern behind their ends is what they keep
    assert same(got[2][:5], got[1][:5])                              # closed: the third call leaves them alone


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("with_ebu", [False, True])
def test_stereo_tpb_leaves_the_frames_in_front_of_each_streams_own_end(M, path, with_ebu):
    """3. beside the true-peak bar nothing behind a stream's end reaches its row"""
    meters = M.METER_TPBALLIST | (M.METER_EBU | M.METER_TRUEPEAK if with_ebu else 0)
    got, _ = run(M, meters, 2, list(RAGGED), path, "tpb", own_end=True)
    assert same(got[1][0], got[0][0]) and got[0][0].any()
    assert (np.abs(np.stack(got)) < 2).all()                         # (neither pattern anywhere)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("family", [None, "tpb"])
def test_mono_tpb_rows_are_47_by_2_with_a_zero_right_channel(M, path, family):
    """4. mono TPBALLIST, dense and with ends"""
    got, _ = run(M, M.METER_TPBALLIST, 1, dense_plan() if family is None else list(RAGGED), path, family, own_end=family is not None)
    g = np.stack(got)
    assert not g[..., 1].view(np.uint32).any() and g[..., 0].any()   # exactly + 0.0


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("family", [None, "lengths"])
@pytest.mark.parametrize("C", [3, 5])
def test_multichannel_rows_are_47_by_C(M, C, family, path):
    """5. layout 8: the row of its own behind the stereo one"""
    run(M, M.METER_EBU | M.METER_TRUEPEAK, C, dense_plan() if family is None else list(RAGGED), path, family)


@pytest.mark.parametrize("family", [None, "lengths"])
def test_wave51_frames_leave_the_row_of_the_picked_channels(M, family):
    """6. five channels read from 5.1 frames on the device: the compact call's row, and nothing of the LFE column in it"""
    plan = dense_plan() if family is None else list(RAGGED)
    meters = M.METER_EBU | M.METER_TRUEPEAK
    wide, _ = run(M, meters, 5, plan, "device", family, wide=True)
    compact, _ = run(M, meters, 5, plan, "device", family)
    for k in range(len(plan)):
        assert same(wide[k], compact[k]), k
        assert not (wide[k] >= LFE).any(), k
