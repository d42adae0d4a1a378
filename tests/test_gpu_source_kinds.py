"""The source kinds following each other on ONE engine: every form a call takes its samples in goes through one launcher
(mtr_launch_decode, mtr_source.hip) and one layout state, so what a kind leaves behind — the layout, the staging and landing buffers of
both chunks, the counters — meets the next kind.  Engine `a` (5 stereo streams, EBU | TRUEPEAK, 48 kHz) takes six calls of 4099 frames
— one whole k_plane tile of 4096 frames and a 3-frame tail that goes float by float, a multiple of no piece size — with
set_host_chunk_bytes (100000), so that every call is two chunks of 3 + 2 streams and uses both staging buffers:

    1. host f32 in the default layout               4. host S24 under plane layout 3, map (2, 0)
    2. host S16 PCM                                 5. device f32 under plane layout 2, the identity, planes 4099 + 5 samples apart
    3. device f32 under frame layout 4, map (3, 1)  6. device S32 PCM in the default layout

Engine `b` takes process () of pcm_decode / pick_decode / plane_decode of the same buffers (the host definitions, pinned to numpy by the
*_cpu tests).  After every call the state blobs of the two are equal by bytes, and the counters of `a` are the literals below."""
import numpy as np
import pytest

import _signals as sig
import test_gpu_frames as F

pytestmark = pytest.mark.gpu

S, T, FS = 5, 4099, 48000.0
CHUNK_BYTES = 100000
# (pcm_stats ()[:2], layout_stats (), plane_stats ()) of `a` after each call.  Taken from the PARENT commit's library on this very sequence
# (the build before the three decode files became one), not from the code under test: two chunks a call, PCM bytes at the source's width
# (5 x 4099 x 2 x 2, + 5 x 4099 x 3 x 3, + 5 x 4099 x 2 x 4).
COUNTERS = [
    ((0, 0), (0, 0), 0),
    ((2, 81980), (0, 0), 0),
    ((2, 81980), (2, 0), 0),
    ((4, 266435), (2, 0), 2),
    ((4, 266435), (2, 0), 4),
    ((6, 430395), (2, 0), 4),
]


@pytest.fixture(scope="module")
def M():
    import meters.lv2_amd as m
    return m


def programme(n_streams, n_frames):
    """[n_streams, 4, n_frames] float32: four channels' worth of programme per stream, stream s scaled by 2^-(s mod 4)"""
    a = np.concatenate([sig.g2(n_frames + 11 * n_streams, 4100 + k).T * np.float32(0.9 ** k) for k in range(2)]).astype(np.float32)
    return np.stack([a[:, 11 * s: 11 * s + n_frames] * np.float32(2.0 ** -(s % 4)) for s in range(n_streams)])


def sequence(M, torch, x):
    """The six calls on the programme x [S, 4, T]: (what engine `a` does, what engine `b` processes) each.  Device buffers are made here and
    kept alive by the closures."""
    n = x.shape[2]
    dev = lambda h: torch.from_numpy(np.ascontiguousarray(h)).cuda()
    frames = lambda *ch: np.ascontiguousarray(x[:, list(ch), :].transpose(0, 2, 1))   # [S, T, len (ch)]
    out = []
    h1 = frames(0, 1)
    out.append((lambda a: a.process(h1), h1))
    q2 = F._quant(frames(1, 2), "s16")
    out.append((lambda a: a.process_pcm(q2), M.pcm_decode(M.PCM_S16, q2)))
    h3 = frames(0, 1, 2, 3)
    d3 = dev(h3)
    out.append((lambda a: (a.set_frame_layout(4, (3, 1)), a.process_device(d3.data_ptr(), n)), M.pick_decode(0, h3, (3, 1))))
    q4 = F._quant(x[:, 1:4, :], "s24")                                        # [S, 3, T] planes
    b4 = np.ascontiguousarray(np.ascontiguousarray(q4.astype("<i4")).view(np.uint8).reshape(q4.shape + (4,))[..., :3]).reshape(q4.shape[0], 3, -1)
    out.append((lambda a: (a.set_plane_layout(3, (2, 0)), a.process_raw(b4.ctypes.data, n, n, M.PCM_S24, host=True)),
                M.plane_decode(M.PCM_S24, b4, (2, 0))))
    h5 = np.full((x.shape[0], 2, n + 5), np.nan, np.float32)                  # (behind a plane's n frames: NaN up to the stride)
    h5[:, :, :n] = x[:, 2:4, :]
    d5 = dev(h5)
    out.append((lambda a: (a.set_plane_layout(2), a.process_device(d5.data_ptr(), n, n + 5)), M.plane_decode(0, h5[:, :, :n], None)))
    q6 = F._quant(frames(3, 0), "s32")
    d6 = dev(q6)
    out.append((lambda a: (a.set_plane_layout(0), a.process_device_pcm(d6.data_ptr(), M.PCM_S32, n)), M.pcm_decode(M.PCM_S32, q6)))
    return out


def counters(e):
    return e.pcm_stats()[:2], e.layout_stats(), e.plane_stats()


def test_the_kinds_follow_each_other(M):
    import torch
    torch.cuda.set_device(0)
    x = programme(S, T)
    with M.Engine(S, FS, M.METER_EBU | M.METER_TRUEPEAK) as a, M.Engine(S, FS, M.METER_EBU | M.METER_TRUEPEAK) as b:
        for e in (a, b):
            e.set_host_chunk_bytes(CHUNK_BYTES)
            e.integr_start()
        for i, (call, ref) in enumerate(sequence(M, torch, x)):
            call(a)
            b.process(ref)
            got = counters(a)
            print("call", i + 1, got)
            assert a.state_export() == b.state_export(), f"call {i + 1}: the state blobs differ"
            assert got == COUNTERS[i], f"call {i + 1}: counters {got}, the parent's {COUNTERS[i]}"
        assert counters(b) == ((0, 0), (0, 0), 0)
