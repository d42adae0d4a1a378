"""tensor_source (meters.lv2_amd/engine.py) without a GPU, without torch and without a tensor: how Engine.process_tensor reads a tensor's
shape and strides — channels first (planes) or channels last (frames), contiguous or a window in time of a longer tensor — and what it
refuses.  Strides are in elements, as torch counts them; the numpy cases divide by the item size."""
import numpy as np
import pytest

import meters.lv2_amd as M

TS = M.tensor_source


def _np(x):
    return x.shape, tuple(s // x.itemsize for s in x.strides), x.dtype


def test_contiguous_channels_first():
    r = TS((5, 2, 1000), (2000, 1000, 1), "float32", 2, channels_first=True)
    assert r == M.TensorSource(0, "planes", 2, (0, 1), 1000, 1000)
    # the shape decides where only one reading has the engine's width
    assert TS((5, 2, 1000), (2000, 1000, 1), "float32", 2) == r
    assert TS((5, 6, 1000), (6000, 1000, 1), "torch.int16", 5, map=(0, 1, 2, 4, 5)) == M.TensorSource(M.PCM_S16, "planes", 6, (0, 1, 2, 4, 5), 1000, 1000)
    assert TS((5, 1, 1000), (1000, 1000, 1), np.dtype(np.int32), 2, map=(0, 0)) == M.TensorSource(M.PCM_S32, "planes", 1, (0, 0), 1000, 1000)
    assert TS(*_np(np.zeros((3, 8, 64), np.float32)), 8).kind == "planes"


def test_contiguous_channels_last():
    r = TS((5, 1000, 2), (2000, 2, 1), "float32", 2)
    assert r == M.TensorSource(0, "frames", 2, (0, 1), 1000, 1000)
    assert TS((5, 1000, 2), (2000, 2, 1), "float32", 2, channels_first=False) == r
    assert TS((5, 1000, 8), (8000, 8, 1), "int16", 2, map=(6, 7)) == M.TensorSource(M.PCM_S16, "frames", 8, (6, 7), 1000, 1000)
    assert TS(*_np(np.zeros((3, 64, 5), np.int32)), 5) == M.TensorSource(M.PCM_S32, "frames", 5, (0, 1, 2, 3, 4), 64, 64)


def test_time_sliced_windows_keep_the_long_stride():
    long_first = np.zeros((4, 2, 9000), np.float32)
    w = long_first[:, :, 1234:1234 + 4801]
    assert TS(*_np(w), 2) == M.TensorSource(0, "planes", 2, (0, 1), 4801, 9000)
    long_last = np.zeros((4, 9000, 2), np.int16)
    w = long_last[:, 77:77 + 2400]
    assert TS(*_np(w), 2) == M.TensorSource(M.PCM_S16, "frames", 2, (0, 1), 2400, 9000)
    # a window of ONE frame: the time axis may have any stride
    assert TS((4, 2, 1), (18000, 9000, 1), "float32", 2, channels_first=True).stride == 9000
    assert TS((4, 1, 2), (18000, 2, 1), "float32", 2, channels_first=False) == M.TensorSource(0, "frames", 2, (0, 1), 1, 9000)
    # a square window is what its strides say: 2 planes 9000 apart are no frames of 2 channels, frames of 2 are no planes 2 apart ...
    assert TS((4, 2, 2), (18000, 9000, 1), "float32", 2).kind == "planes"
    assert TS((4, 2, 2), (18000, 2, 1), "float32", 2) == M.TensorSource(0, "frames", 2, (0, 1), 2, 9000)
    # one stream: the batch axis may have any stride
    assert TS((1, 2, 100), (0, 100, 1), "float32", 2) == M.TensorSource(0, "planes", 2, (0, 1), 100, 100)
    assert TS((1, 100, 2), (12345, 2, 1), "float32", 2) == M.TensorSource(0, "frames", 2, (0, 1), 100, 100)


def test_the_ambiguous_cases_need_the_caller():
    # a mono engine, C == 1: (B, T, 1) is T frames of one channel, and with T == 1 also one plane of one sample — the same thing
    assert TS((5, 1, 1), (1, 1, 1), "float32", 1) == M.TensorSource(0, "frames", 1, (0,), 1, 1)
    assert TS((5, 1000, 1), (1000, 1, 1), "float32", 1) == M.TensorSource(0, "frames", 1, (0,), 1000, 1000)      # (1000 planes are not 1 channel)
    assert TS((5, 1, 1000), (1000, 1000, 1), "float32", 1) == M.TensorSource(0, "planes", 1, (0,), 1000, 1000)
    # a mono file on a stereo engine, W == 1: 4 frames of one channel or 4 planes of one sample, both go with the map
    with pytest.raises(ValueError, match="channels_first"):
        TS((5, 4, 1), (4, 1, 1), "float32", 2, map=(0, 0))
    assert TS((5, 4, 1), (4, 1, 1), "float32", 2, map=(0, 0), channels_first=False) == M.TensorSource(0, "frames", 1, (0, 0), 4, 4)
    assert TS((5, 4, 1), (4, 1, 1), "float32", 2, map=(0, 0), channels_first=True) == M.TensorSource(0, "planes", 4, (0, 0), 1, 1)
    # a contiguous square: 2 planes of 2 samples or 2 frames of 2 channels
    with pytest.raises(ValueError, match="channels_first"):
        TS((5, 2, 2), (4, 2, 1), "float32", 2)
    assert TS((5, 2, 2), (4, 2, 1), "float32", 2, channels_first=True).kind == "planes"
    # T == 1 with a map that fits both widths
    with pytest.raises(ValueError, match="channels_first"):
        TS((5, 1, 8), (8, 8, 1), "float32", 1, map=(0,))
    assert TS((5, 1, 8), (8, 8, 1), "float32", 1, map=(0,), channels_first=True) == M.TensorSource(0, "planes", 1, (0,), 8, 8)
    assert TS((5, 1, 8), (8, 8, 1), "float32", 1, map=(0,), channels_first=False) == M.TensorSource(0, "frames", 8, (0,), 1, 1)


def test_refused():
    t = np.zeros((4, 100, 2), np.float32)
    with pytest.raises(ValueError, match=r"innermost stride.*\(200, 1, 2\)"):
        TS(*_np(t.transpose(0, 2, 1)), 2)                                # a transposed view: (4, 2, 100) with strides (200, 1, 2)
    with pytest.raises(ValueError, match="negative strides"):
        TS(*_np(np.zeros((4, 2, 100), np.float32)[:, :, ::-1]), 2)
    with pytest.raises(ValueError, match="negative strides"):
        TS((4, 2, 100), (-200, 100, 1), "float32", 2)
    for bad in ("float64", "float16", "uint8", "int64", "torch.bfloat16"):
        with pytest.raises(ValueError, match="dtype"):
            TS((4, 2, 100), (200, 100, 1), bad, 2)
    with pytest.raises(ValueError, match=r"shorter than n_frames.*\(100, 50, 1\)"):
        TS((4, 2, 100), (100, 50, 1), "float32", 2)                      # st < n_frames: overlapping planes
    with pytest.raises(ValueError, match="shorter than n_frames"):
        TS((4, 100, 2), (100, 2, 1), "float32", 2)                       # ... overlapping streams
    with pytest.raises(ValueError, match=r"\(0, 100, 1\)"):
        TS((4, 2, 100), (0, 100, 1), "float32", 2, channels_first=True)  # an expanded batch
    with pytest.raises(ValueError, match="shorter than n_frames"):
        TS((4, 2, 100), (200, 0, 1), "float32", 2)                       # an expanded channel
    with pytest.raises(ValueError, match=r"\(400, 4, 1\)"):
        TS((4, 100, 2), (400, 4, 1), "float32", 2)                       # every other frame
    with pytest.raises(ValueError, match=r"\(300, 100, 1\)"):
        TS((4, 2, 100), (300, 100, 1), "float32", 2)                     # two of three planes: the streams are not P * st apart
    with pytest.raises(ValueError, match="three axes"):
        TS((4, 100), (100, 1), "float32", 1)
    with pytest.raises(ValueError, match="three axes"):
        TS((4, 2, 100, 1), (200, 100, 1, 1), "float32", 2)
    with pytest.raises(ValueError, match="empty"):
        TS((4, 2, 0), (0, 0, 1), "float32", 2)
    with pytest.raises(ValueError, match="n_channels"):
        TS((4, 3, 100), (300, 100, 1), "float32", 2)                     # neither axis is the engine's width, and no map
    with pytest.raises(ValueError, match="map"):
        TS((4, 3, 100), (300, 100, 1), "float32", 2, map=(0, 3), channels_first=True)
    with pytest.raises(ValueError, match="map"):
        TS((4, 9, 100), (900, 100, 1), "float32", 2, map=(0, 1), channels_first=True)   # more than 8 planes
    with pytest.raises(ValueError, match="map"):
        TS((4, 3, 100), (300, 100, 1), "float32", 2, map=(0, 1, 2), channels_first=True)


def test_it_never_copies_and_needs_no_torch():
    import sys
    had = "torch" in sys.modules
    r = TS((2, 2, 10), (20, 10, 1), "float32", 2)
    assert isinstance(r, tuple) and r._fields == ("format", "kind", "width", "map", "n_frames", "stride")
    assert ("torch" in sys.modules) == had
