"""Frame layouts (mtr_engine_set_frame_layout): the surface and the pick / decode contract, without a GPU.

mtr_pick_decode_host is what k_pick (mtr_source.hip) is held against (tests/test_gpu_frames.py), so it is pinned here to numpy
BIT FOR BIT: `decode (x)[:, map]`, compared as uint32 views — a NaN keeps its payload, -0.0 stays -0.0.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import meters.lv2_amd as M

HERE = os.path.dirname(os.path.abspath(__file__))
NEW = ("mtr_engine_set_frame_layout", "mtr_engine_frame_layout", "mtr_pick_decode_host", "mtr_engine_layout_stats")
FORMATS = (0, 1, 2, 3)                                                   # f32, MTR_PCM_S16, _S24, _S32
BYTES = {0: 4, 1: 2, 2: 3, 3: 4}
MAPS = {1: [(0,), (0, 0), (0, 0, 0, 0, 0)], 2: [(1,), (1, 0), (0, 0), (1, 1, 0)], 3: [(2, 0), (0, 1, 2), (2, 2, 1, 0)],
        4: [(3, 1), (0, 1, 2, 3), (3, 2, 1, 0, 0)], 5: [(4,), (4, 3, 2, 1, 0)], 6: [(0, 1, 2, 4, 5), (5, 3)], 7: [(6, 0, 6)],
        8: [(6, 7), (7, 5, 3, 1), (0, 2, 4, 6, 7)]}


def test_header_declares_and_library_exports_the_frame_layout_entry_points():
    names = M.exported_symbols()
    for n in NEW:
        assert n in names, f"{n} is not declared in include/mtr_engine.h"
        assert hasattr(M.lib, n), f"{n} is declared but libmtr_engine.so does not export it"
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "mtr_engine.h")).read()
    assert re.search(r"#define\s+MTR_ABI_VERSION\s+2\b", hdr)          # (an addition inside version 2)
    assert M.lib.mtr_abi_version() == 2
    assert re.search(r"#define\s+MTR_MAX_FRAME_CHANNELS\s+8\b", hdr)
    # the header gains exactly these four: everything else it declares is what test_pcm_cpu.py and its predecessors pin
    before = set(PARENT_SYMBOLS.split())
    assert set(names) - before == set(NEW) and before <= set(names)


PARENT_SYMBOLS = """
mtr_abi_version mtr_band_coef mtr_comm_destroy mtr_comm_device mtr_comm_init mtr_comm_init_timeout mtr_comm_nranks mtr_comm_probe
mtr_comm_set_timeout mtr_comm_unique_id mtr_engine_aggregate_device mtr_engine_bitstats mtr_engine_create mtr_engine_deferred_stats
mtr_engine_destroy mtr_engine_dr14_reset mtr_engine_dr14_results mtr_engine_fragment_powers mtr_engine_histograms
mtr_engine_integr_pause mtr_engine_integr_reset mtr_engine_integr_start mtr_engine_intstat_reset mtr_engine_join
mtr_engine_kmeter_read mtr_engine_kmeter_reset mtr_engine_layout mtr_engine_pcm_stats mtr_engine_prepare_host
mtr_engine_process_device mtr_engine_process_device_lengths mtr_engine_process_device_pcm mtr_engine_process_host
mtr_engine_process_host_lengths mtr_engine_process_host_pcm mtr_engine_process_planar_host mtr_engine_prune_stats mtr_engine_reduce
mtr_engine_refine_stats mtr_engine_reset mtr_engine_results mtr_engine_seg_stats mtr_engine_set_deferred_tail
mtr_engine_set_host_chunk_bytes mtr_engine_sigdist mtr_engine_spectr_reset_peak mtr_engine_spectr_set_speed mtr_engine_spectrum
mtr_engine_state_bytes mtr_engine_state_export mtr_engine_state_import mtr_engine_stream_frames mtr_engine_sync
mtr_engine_timing_calls mtr_engine_timing_enable mtr_engine_timing_query mtr_engine_truepeak_channels mtr_engine_truepeak_reset
mtr_fir_table mtr_hist_loudness mtr_kweight_coef mtr_last_error mtr_pcm_decode_host mtr_pcm_sample_bytes mtr_plan_query
mtr_rccl_version mtr_state_blob_count mtr_synth_fill_device mtr_version
"""


def test_binding_has_the_frame_layout_methods():
    for m in ("set_frame_layout", "frame_layout", "layout_stats"):
        assert callable(getattr(M.Engine, m, None)), m
    assert callable(getattr(M, "pick_decode", None))


def _source(fmt, n, fc, seed):
    """(raw bytes of n frames of fc samples, their float32 values [n, fc] by numpy's own conversion)"""
    rng = np.random.default_rng(seed)
    if fmt == 0:
        w = rng.integers(0, 1 << 32, (n, fc), dtype=np.uint64).astype(np.uint32)     # bit soup: NaNs with payloads, Inf, denormals
        if n:
            w[0, 0] = 0x80000000                                         # -0.0
            w[-1, -1] = 0x7fc12345                                       # a quiet NaN with a payload
            w[n // 2, 0] = 0x7f812345                                    # a signalling one
        return w.view(np.uint8).reshape(-1).copy(), w.view(np.float32)
    k = {1: 15, 2: 23, 3: 31}[fmt]
    v = rng.integers(-(1 << k), 1 << k, (n, fc))
    if n:
        v[0, 0], v[-1, -1] = -(1 << k), (1 << k) - 1
    want = v.astype(np.int32).astype(np.float32) * np.float32(2.0 ** -k)
    if fmt == 1:
        raw = v.astype("<i2").view(np.uint8)
    elif fmt == 3:
        raw = v.astype("<i4").view(np.uint8)
    else:
        raw = np.ascontiguousarray(v.astype("<i4")).view(np.uint8).reshape(-1, 4)[:, :3]
    return np.ascontiguousarray(raw).reshape(-1).copy(), want


def _pick_at(fmt, raw, n, fc, m, shift):
    """mtr_pick_decode_host on n frames whose bytes start `shift` bytes into a fresh buffer; nothing behind n * C floats is written"""
    buf = np.zeros(raw.size + shift + 16, np.uint8)
    buf[shift:shift + raw.size] = raw
    mp = np.array(m, np.uint8)
    out = np.full(n * len(m) + 4, np.float32(123.0))
    assert M.lib.mtr_pick_decode_host(fmt, buf.ctypes.data + shift, n, fc, mp.ctypes.data, len(m), out.ctypes.data) == 0
    assert (out[n * len(m):] == 123.0).all()
    return out[:n * len(m)].reshape(n, len(m))


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("fc", range(1, 9))
def test_pick_decode_host_is_numpy_bit_for_bit(fmt, fc):
    for n in (0, 1, 7, 1001):
        raw, want = _source(fmt, n, fc, 100 * fmt + fc)
        assert raw.size == n * fc * BYTES[fmt]
        for m in MAPS[fc]:
            for shift in (0, 1, 3) if fmt != 0 else (0, 4):
                got = _pick_at(fmt, raw, n, fc, m, shift)
                ref = np.ascontiguousarray(want[:, list(m)])
                assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (fmt, fc, m, n, shift)


def test_pick_decode_binding():
    x = np.arange(2 * 5 * 6, dtype=np.float32).reshape(2, 5, 6)
    assert np.array_equal(M.pick_decode(0, x, [0, 1, 2, 4, 5]), x[..., [0, 1, 2, 4, 5]])
    q = (np.arange(2 * 5 * 8).reshape(2, 5, 8) * 37 - 900).astype(np.int16)
    assert np.array_equal(M.pick_decode(M.PCM_S16, q, [6, 7], 2), M.pcm_decode(M.PCM_S16, q)[..., 6:])
    b = np.ascontiguousarray(q.astype("<i4")).view(np.uint8).reshape(2, 5, 8, 4)[..., :3].reshape(2, 5, 24)
    assert np.array_equal(M.pick_decode(M.PCM_S24, np.ascontiguousarray(b), [0, 0]), (q[..., [0, 0]].astype(np.float32) * np.float32(2.0 ** -23)))
    with pytest.raises(ValueError):
        M.pick_decode(0, x, [0, 1], 3)


def test_argument_errors():
    src = np.zeros(256, np.uint8)
    dst = np.zeros(64, np.float32)
    ok = np.array([0, 1], np.uint8)
    L = M.lib
    assert L.mtr_pick_decode_host(0, src.ctypes.data, 4, 2, ok.ctypes.data, 2, dst.ctypes.data) == 0
    for fmt in (4, -1, 17):
        assert L.mtr_pick_decode_host(fmt, src.ctypes.data, 4, 2, ok.ctypes.data, 2, dst.ctypes.data) == -1, fmt
    for fmt in FORMATS:
        assert L.mtr_pick_decode_host(fmt, None, 4, 2, ok.ctypes.data, 2, dst.ctypes.data) == -1
        assert L.mtr_pick_decode_host(fmt, src.ctypes.data, 4, 2, ok.ctypes.data, 2, None) == -1
        assert L.mtr_pick_decode_host(fmt, src.ctypes.data, 4, 2, None, 2, dst.ctypes.data) == -1
        assert L.mtr_pick_decode_host(fmt, src.ctypes.data, 4, 1, ok.ctypes.data, 2, dst.ctypes.data) == -1     # entry 1 >= frame_channels 1
        assert L.mtr_pick_decode_host(fmt, src.ctypes.data, 4, 9, ok.ctypes.data, 2, dst.ctypes.data) == -1     # > MTR_MAX_FRAME_CHANNELS
        assert L.mtr_pick_decode_host(fmt, src.ctypes.data, 4, 0, ok.ctypes.data, 2, dst.ctypes.data) == -1
    assert (dst == 0).all()
    # a NULL engine is refused before anything else
    assert L.mtr_engine_set_frame_layout(None, 6, ok.ctypes.data) == -1
    fc = C.c_uint32()
    assert L.mtr_engine_frame_layout(None, C.byref(fc), None) == -1
    a, b = C.c_uint64(), C.c_uint64()
    assert L.mtr_engine_layout_stats(None, C.byref(a), C.byref(b)) == -1
