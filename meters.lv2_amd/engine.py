"""ctypes binding of include/mtr_engine.h (libmtr_engine.so).

Names follow the reference's classes: Engine.integr_start/.integr_pause/.integr_reset mirror
Ebu_r128_proc (ebumeter/ebu_r128_proc.h:77-79), Engine.results() returns the getters of
ebu_r128_proc.h:81-94 per stream, Engine.process() is the batched process()/process_max()/
spectrum_run inner loop.  Device buffers are passed as raw pointers (torch tensors' data_ptr());
Engine.process_tensor() takes a torch tensor or a numpy array as it lies, channels first or last.
"""
import collections
import ctypes as C
import os
import re

import numpy as np

METER_EBU, METER_TRUEPEAK, METER_SPECTR30, METER_TPBALLIST = 0x01, 0x02, 0x04, 0x08
METER_BITSTATS, METER_SIGDIST, METER_DR14, METER_KMETER = 0x10, 0x20, 0x40, 0x80
METER_STCORR = 0x200                       # (0x100 is no meter)
METER_NEEDLE = 0x800                       # VU, IEC I / II PPM, M/S PPM: include/mtr_needle.h (0x400 is no meter either)
METER_SURROUND = 0x2000                    # sur_run: C K-meters + four pair correlations, 3 .. 8 channels: include/mtr_surround.h (0x1000 is no meter)
METER_SCOPE = 0x8000                       # the stereoscope's / phase wheel's FFT analysis, stereo: include/mtr_scope.h (0x4000 is no meter)
METER_GONIO = 0x20000                      # the goniometer's M/S point image, auto gain and series, stereo: include/mtr_gonio.h (0x10000 is no meter)
NEEDLE_VU, NEEDLE_IEC1, NEEDLE_IEC2, NEEDLE_MS = 1, 2, 4, 8
BIM_LAST, DIST_BIN = 584, 361
HIST_LEN, NBANDS = 751, 30
PCM_S16, PCM_S24, PCM_S32 = 1, 2, 3        # MTR_PCM_*: little-endian int16 / packed 3-byte / int32 samples
# MTR_SCOPE_F_*: the fields of a point of the scope's reading series (include/mtr_scope_series.h), in the order of mtr_engine_scope_series' outputs
SCOPE_F_LEVEL, SCOPE_F_LR, SCOPE_F_PHASE, SCOPE_F_PLEVEL, SCOPE_F_PEAK, SCOPE_F_POWER_L, SCOPE_F_POWER_R, SCOPE_F_ALL = 1, 2, 4, 8, 16, 32, 64, 127
SCOPE_FIELDS = ("level", "lr", "phase", "plevel", "peak", "power_l", "power_r")
SPECTR_PEAK_HOLD, SPECTR_PEAK_BLOCK = 0, 1   # MTR_SPECTR_PEAK_*: max as held since reset / reset_peak, or zeroed behind every point
LOUDLOG_SAMPLE, LOUDLOG_MAX = 0, 1         # MTR_LOUDLOG_*: a point is the period's last (M, S) / the maxima over the period
INTEGLOG_FIELDS = ("I", "I_thr", "Rmin", "Rmax", "R_thr")   # a point of the integration log (mtr_integlog.h), in the getters' order

_HERE = os.path.dirname(os.path.abspath(__file__))
# MTR_LIB: an alternative build of the same library (instrumented kernels, tools/f4_prof.py); never a different backend
lib_path = os.environ.get("MTR_LIB") or os.path.join(_HERE, "lib", "libmtr_engine.so")


class EngineError(RuntimeError):
    """A C-ABI call returned a status other than MTR_OK; `.code` is that status (ERR_TIMEOUT, ERR_STATE, ...)."""
    code = 0


ABI_VERSION = 2            # MTR_ABI_VERSION of include/mtr_engine.h this file binds

ERR_ARG, ERR_UNSUPPORTED, ERR_NODEVICE, ERR_HIP, ERR_NOMEM, ERR_TIMEOUT, ERR_STATE = -1, -2, -3, -4, -5, -6, -7


class _Config(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("meters", C.c_uint32), ("n_streams", C.c_uint32),
                ("n_channels", C.c_uint32), ("sample_rate", C.c_float), ("device", C.c_int32),
                ("max_frames", C.c_uint32), ("tune_run", C.c_uint32), ("tune_segments", C.c_uint32),
                ("tune_layout", C.c_uint32), ("tune_fir", C.c_uint32), ("tune_prune", C.c_uint32)]


class GonioConfig(C.Structure):
    """mtr_gonio_config (include/mtr_gonio.h); zeros select the defaults"""
    _fields_ = [("struct_size", C.c_uint32), ("period_frames", C.c_uint32), ("capacity", C.c_uint32), ("shift", C.c_uint32),
                ("autogain", C.c_uint32), ("gain", C.c_float), ("point_width", C.c_float), ("g_attack", C.c_float), ("g_decay", C.c_float),
                ("g_target", C.c_float), ("g_rms", C.c_float), ("tune_piece", C.c_uint32)]


class GonioDerived(C.Structure):
    """mtr_gonio_derived (include/mtr_gonio.h)"""
    _fields_ = [("period_frames", C.c_uint32), ("G", C.c_uint32), ("hpw", C.c_float), ("attack", C.c_float * 2), ("g_target", C.c_float),
                ("g_rms", C.c_float)]


class PlanInfo(C.Structure):
    """mtr_plan_info: how an engine would tile and route a call (mtr_plan_query: host arithmetic, no device)."""
    _fields_ = [(n, C.c_uint32) for n in ("layout", "uses_seg", "head_frames", "body_fragments", "segments", "fragments_per_lane",
                                          "warm_steps", "n_tiles", "head_tiles", "n_fragments_ended", "kw_segments", "frames_left_after")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class Dr14Result(C.Structure):
    """mtr_dr14_result: what dr14_run leaves on the dr14 plugins' ports in dr_operation_mode."""
    _fields_ = [("m_rms", C.c_float * 2), ("m_peak", C.c_float * 2), ("dr", C.c_float * 2),
                ("dr_total", C.c_float), ("block_count", C.c_float)]


class StreamResult(C.Structure):
    """mtr_stream_result: Ebu_r128_proc's getters in declaration order, then true peak."""
    _fields_ = [("loudness_M", C.c_float), ("maxloudn_M", C.c_float), ("loudness_S", C.c_float),
                ("maxloudn_S", C.c_float), ("integrated", C.c_float), ("integ_thr", C.c_float),
                ("range_min", C.c_float), ("range_max", C.c_float), ("range_thr", C.c_float),
                ("hist_M_count", C.c_int32), ("hist_S_count", C.c_int32),
                ("truepeak", C.c_float * 2), ("truepeak_call", C.c_float * 2),
                ("tpb_level", C.c_float * 2), ("tpb_peak", C.c_float * 2)]


def _preload_hip_runtime():
    """One HIP runtime and one RCCL per process.  PyTorch-ROCm wheels bundle their own libamdhip64.so and librccl.so
    (same SONAMEs as /opt/rocm's); if our library pulled in the system copies first and torch then loaded
    its own, the second runtime finds no GPU.  When torch is installed (it is only plumbing here:
    device buffers, torch.distributed) load ITS copies first so both sides share them; without torch
    the library's rpath (/opt/rocm/lib) applies."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec and spec.submodule_search_locations:
        for name in ("libamdhip64.so", "librccl.so"):
            cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", name)
            if os.path.exists(cand):
                try:
                    C.CDLL(cand, mode=C.RTLD_GLOBAL if name == "libamdhip64.so" else C.RTLD_LOCAL)
                except OSError:
                    pass                      # the system copy (rpath) serves


def _load():
    if not os.path.exists(lib_path):
        raise ImportError(
            f"{lib_path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). meters.lv2_amd has no CPU or pure-Python fallback.")
    _preload_hip_runtime()
    L = C.CDLL(lib_path)
    vp, u32, u64, i32, f32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int32, C.c_float
    L.mtr_last_error.restype = C.c_char_p
    L.mtr_version.restype = C.c_char_p
    # the entry points bound below are those of ABI version ABI_VERSION: an older library (MTR_LIB pointing at a stale
    # build) is named as such here instead of failing somewhere below with an AttributeError
    have = L.mtr_abi_version() if hasattr(L, "mtr_abi_version") else 0
    if have < ABI_VERSION:
        raise ImportError(f"{lib_path} speaks ABI version {have}, this binding needs {ABI_VERSION} (include/mtr_engine.h): rebuild it "
                          "with `python -c 'import __graft_entry__ as g; g.build()'`")
    L.mtr_engine_create.argtypes = [C.POINTER(_Config), C.POINTER(vp)]
    L.mtr_engine_destroy.argtypes = [vp]
    L.mtr_engine_destroy.restype = None
    for n in ("reset", "integr_start", "integr_pause", "integr_reset", "truepeak_reset",
              "spectr_reset_peak", "sync"):
        getattr(L, "mtr_engine_" + n).argtypes = [vp]
    L.mtr_engine_spectr_set_speed.argtypes = [vp, f32]
    L.mtr_engine_process_device.argtypes = [vp, vp, u64, u64, vp]
    L.mtr_engine_process_host.argtypes = [vp, vp, u64, u64]
    if hasattr(L, "mtr_engine_stream_frames"):                 # (an addition inside ABI version 2: per-stream lengths)
        L.mtr_engine_process_device_lengths.argtypes = [vp, vp, u64, u64, vp, vp]
        L.mtr_engine_process_host_lengths.argtypes = [vp, vp, u64, u64, vp]
        L.mtr_engine_stream_frames.argtypes = [vp, u32, u32, vp, vp]
    if hasattr(L, "mtr_engine_process_device_tracks"):         # (an addition inside ABI version 2: track lengths for the whole-track meters)
        L.mtr_engine_process_device_tracks.argtypes = [vp, vp, u64, u64, vp, vp]
        L.mtr_engine_process_host_tracks.argtypes = [vp, vp, u64, u64, vp]
    if hasattr(L, "mtr_engine_process_device_ragged"):         # (an addition inside ABI version 2: ragged batches for STCORR and NEEDLE)
        L.mtr_engine_process_device_ragged.argtypes = [vp, vp, u64, u64, vp, vp]
        L.mtr_engine_process_host_ragged.argtypes = [vp, vp, u64, u64, vp]
        L.mtr_engine_series_points.argtypes = [vp, u32, u32, u32, vp]
        L.mtr_series_cut.argtypes = [u64, u64, u64, u64, C.POINTER(u64), C.POINTER(u32)]
    if hasattr(L, "mtr_engine_process_device_ends"):           # (an addition inside ABI version 2: track lengths for the 30-band bank)
        L.mtr_engine_process_device_ends.argtypes = [vp, vp, u64, u64, vp, vp]
        L.mtr_engine_process_host_ends.argtypes = [vp, vp, u64, u64, vp]
        L.mtr_engine_spectr_points.argtypes = [vp, u32, u32, vp]
    if hasattr(L, "mtr_engine_process_device_tpb"):            # (an addition inside ABI version 2: track lengths for the true-peak bar)
        L.mtr_engine_process_device_tpb.argtypes = [vp, vp, u64, u64, vp, vp]
        L.mtr_engine_process_host_tpb.argtypes = [vp, vp, u64, u64, vp]
        L.mtr_engine_tpb_points.argtypes = [vp, u32, u32, vp]
    if hasattr(L, "mtr_engine_process_device_any"):            # (an addition inside ABI version 2: track lengths for the scope and the surround meter)
        L.mtr_engine_process_device_any.argtypes = [vp, vp, u64, u64, vp, vp]
        L.mtr_engine_process_host_any.argtypes = [vp, vp, u64, u64, vp]
        L.mtr_engine_scope_points.argtypes = [vp, u32, u32, vp, vp]
    if hasattr(L, "mtr_engine_pcm_stats"):                     # (an addition inside ABI version 2: integer PCM in)
        L.mtr_engine_process_host_pcm.argtypes = [vp, vp, C.c_int, u64, u64, vp]
        L.mtr_engine_process_device_pcm.argtypes = [vp, vp, C.c_int, u64, u64, vp, vp]
        L.mtr_engine_pcm_stats.argtypes = [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(f32)]
        L.mtr_pcm_sample_bytes.argtypes = [C.c_int]
        L.mtr_pcm_sample_bytes.restype = C.c_size_t
        L.mtr_pcm_decode_host.argtypes = [C.c_int, vp, C.c_size_t, vp]
    if hasattr(L, "mtr_engine_set_frame_layout"):              # (an addition inside ABI version 2: frame layouts)
        L.mtr_engine_set_frame_layout.argtypes = [vp, u32, vp]
        L.mtr_engine_frame_layout.argtypes = [vp, C.POINTER(u32), vp]
        L.mtr_engine_layout_stats.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
        L.mtr_pick_decode_host.argtypes = [C.c_int, vp, C.c_size_t, u32, vp, u32, vp]
    L.mtr_engine_set_host_chunk_bytes.argtypes = [vp, u64]
    L.mtr_engine_process_planar_host.argtypes = [vp, C.POINTER(vp), u32]
    L.mtr_engine_results.argtypes = [vp, u32, u32, C.POINTER(StreamResult)]
    L.mtr_engine_histograms.argtypes = [vp, u32, u32, vp, vp]
    if hasattr(L, "mtr_engine_truepeak_channels"):             # (an addition inside ABI version 2: multichannel engines)
        L.mtr_engine_truepeak_channels.argtypes = [vp, u32, u32, vp, vp]
    L.mtr_engine_fragment_powers.argtypes = [vp, u32, u32, vp, u32, C.POINTER(u32)]
    L.mtr_engine_spectrum.argtypes = [vp, u32, u32, vp, vp, vp, vp]
    L.mtr_engine_aggregate_device.argtypes = [vp, vp, vp, vp]
    L.mtr_engine_bitstats.argtypes = [vp, u32, u32, vp, vp, vp]
    L.mtr_engine_sigdist.argtypes = [vp, u32, u32, vp, vp, vp, vp]
    L.mtr_engine_intstat_reset.argtypes = [vp]
    L.mtr_engine_dr14_results.argtypes = [vp, u32, u32, vp]
    L.mtr_engine_dr14_reset.argtypes = [vp]
    L.mtr_engine_kmeter_read.argtypes = [vp, u32, u32, vp, vp]
    L.mtr_engine_kmeter_reset.argtypes = [vp]
    if hasattr(L, "mtr_engine_kmeter_series"):                 # (an addition inside ABI version 2: the K-meter's reading series)
        L.mtr_engine_kmeter_set_period.argtypes = [vp, u32, u32]
        L.mtr_engine_kmeter_period.argtypes = [vp, C.POINTER(u32), C.POINTER(u32)]
        L.mtr_engine_kmeter_series.argtypes = [vp, u32, u32, vp, vp, u32, C.POINTER(u32), C.POINTER(u32)]
    if hasattr(L, "mtr_engine_tpb_series"):                    # (an addition inside ABI version 2: the true-peak bar's reading series)
        L.mtr_engine_tpb_set_period.argtypes = [vp, u32, u32]
        L.mtr_engine_tpb_period.argtypes = [vp, C.POINTER(u32), C.POINTER(u32)]
        L.mtr_engine_tpb_series.argtypes = [vp, u32, u32, vp, vp, u32, C.POINTER(u32), C.POINTER(u32)]
    if hasattr(L, "mtr_engine_spectr_series"):                 # (an addition inside ABI version 2: the 30-band bank's reading series)
        L.mtr_engine_spectr_set_period.argtypes = [vp, u32, u32, C.c_int]
        L.mtr_engine_spectr_period.argtypes = [vp, C.POINTER(u32), C.POINTER(u32), C.POINTER(C.c_int)]
        L.mtr_engine_spectr_series.argtypes = [vp, u32, u32, vp, vp, vp, vp, u32, C.POINTER(u32), C.POINTER(u32)]
    if hasattr(L, "mtr_engine_stcorr_read"):                   # (an addition inside ABI version 2: stereo phase correlation)
        L.mtr_stcorr_coef.argtypes = [f32, vp]
        L.mtr_engine_stcorr_set_period.argtypes = [vp, u32, u32]
        L.mtr_engine_stcorr_read.argtypes = [vp, u32, u32, vp, vp]
        L.mtr_engine_stcorr_series.argtypes = [vp, u32, u32, vp, u32, C.POINTER(u32), C.POINTER(u32)]
        L.mtr_engine_stcorr_reset.argtypes = [vp]
    if hasattr(L, "mtr_engine_needle_read"):                   # (an addition inside ABI version 2: the needle meters)
        L.mtr_needle_coef.argtypes = [u32, f32, vp]
        L.mtr_engine_needle_configure.argtypes = [vp, u32, u32, u32]
        L.mtr_engine_needle_set_gain.argtypes = [vp, C.c_int, f32]
        L.mtr_engine_needle_read.argtypes = [vp, u32, u32, u32, vp, vp]
        L.mtr_engine_needle_series.argtypes = [vp, u32, u32, u32, vp, u32, C.POINTER(u32), C.POINTER(u32)]
        L.mtr_engine_needle_reset.argtypes = [vp]
    if hasattr(L, "mtr_engine_surround_read"):                 # (an addition inside ABI version 2: the surround meter)
        L.mtr_engine_surround_set_pairs.argtypes = [vp, vp, vp]
        L.mtr_engine_surround_pairs.argtypes = [vp, vp, vp]
        L.mtr_engine_surround_set_period.argtypes = [vp, u32, u32]
        L.mtr_engine_surround_read.argtypes = [vp, u32, u32, vp, vp, vp]
        L.mtr_engine_surround_pair_states.argtypes = [vp, u32, u32, vp]
        L.mtr_engine_surround_series.argtypes = [vp, u32, u32, vp, vp, vp, u32, C.POINTER(u32), C.POINTER(u32)]
        L.mtr_engine_surround_reset.argtypes = [vp]
    if hasattr(L, "mtr_engine_scope_read"):                    # (an addition inside ABI version 2: the stereo / frequency scope)
        L.mtr_scope_window.argtypes = [u32, vp]
        L.mtr_engine_scope_configure.argtypes = [vp, u32, u32, f32]
        L.mtr_engine_scope_config.argtypes = [vp, C.POINTER(u32), C.POINTER(u32), C.POINTER(f32)]
        L.mtr_engine_scope_read.argtypes = [vp, u32, u32, vp, vp, vp, vp, vp, vp, vp]
        L.mtr_engine_scope_analyses.argtypes = [vp, C.POINTER(u64)]
        L.mtr_engine_scope_reset.argtypes = [vp]
    if hasattr(L, "mtr_engine_scope_series"):                  # (an addition inside ABI version 2: the scope's reading series)
        L.mtr_engine_scope_set_series.argtypes = [vp, u32, u32, u32]
        L.mtr_engine_scope_series_config.argtypes = [vp, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32)]
        L.mtr_engine_scope_series.argtypes = [vp, u32, u32, vp, vp, vp, vp, vp, vp, vp, u32, C.POINTER(u32), C.POINTER(u32)]
        L.mtr_scope_series_cut.argtypes = [u32, u32, u32, u32, u64, C.POINTER(u64), C.POINTER(u64)]
    if hasattr(L, "mtr_engine_gonio_image"):                   # (an addition inside ABI version 2: the goniometer)
        L.mtr_gonio_derive.argtypes = [C.POINTER(GonioConfig), C.c_double, C.POINTER(GonioDerived)]
        L.mtr_engine_gonio_configure.argtypes = [vp, C.POINTER(GonioConfig)]
        L.mtr_engine_gonio_config.argtypes = [vp, C.POINTER(GonioConfig), C.POINTER(GonioDerived)]
        L.mtr_engine_gonio_set_gain.argtypes = [vp, f32]
        L.mtr_engine_gonio_image.argtypes = [vp, u32, u32, vp, vp, vp, vp]
        L.mtr_engine_gonio_read.argtypes = [vp, u32, u32, vp, vp, vp]
        L.mtr_engine_gonio_blocks.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
        L.mtr_engine_gonio_series.argtypes = [vp, u32, u32, u64, u32, vp, vp, vp]
        L.mtr_engine_gonio_image_clear.argtypes = [vp]
        L.mtr_engine_gonio_reset.argtypes = [vp]
        L.mtr_engine_gonio_timing.argtypes = [vp, C.c_int, C.POINTER(f32), C.POINTER(f32), C.POINTER(u32)]
    if hasattr(L, "mtr_engine_process_device_gonio_ends"):     # (an addition inside ABI version 2: track lengths for the goniometer)
        L.mtr_engine_process_device_gonio_ends.argtypes = [vp, vp, u64, u64, vp, vp]
        L.mtr_engine_process_host_gonio_ends.argtypes = [vp, vp, u64, u64, vp]
        L.mtr_gonio_cut.argtypes = [u64, u32, C.c_double, u64, u64, C.POINTER(GonioConfig), C.POINTER(u64), C.POINTER(u32), C.POINTER(u64),
                                    C.POINTER(f32)]
        L.mtr_engine_gonio_points.argtypes = [vp, u32, u32, vp, vp]
    if hasattr(L, "mtr_engine_gonio_set_oversample"):          # (an addition inside ABI version 2: the goniometer's oversampling)
        L.mtr_gonio_os_table.argtypes = [u32, vp]
        L.mtr_gonio_os_hpw.argtypes = [C.c_double, u32, C.POINTER(f32)]
        L.mtr_engine_gonio_set_oversample.argtypes = [vp, u32]
        L.mtr_engine_gonio_oversample.argtypes = [vp, C.POINTER(u32), C.POINTER(f32)]
        L.mtr_engine_gonio_os_timing.argtypes = [vp, C.POINTER(f32), C.POINTER(u32)]
    if hasattr(L, "mtr_engine_set_plane_layout"):              # (an addition inside ABI version 2: plane layouts)
        L.mtr_engine_set_plane_layout.argtypes = [vp, u32, vp]
        L.mtr_engine_plane_layout.argtypes = [vp, C.POINTER(u32), vp]
        L.mtr_plane_decode_host.argtypes = [C.c_int, vp, C.c_size_t, u64, u32, vp, u32, vp]
        L.mtr_engine_plane_stats.argtypes = [vp, C.POINTER(u64)]
    if hasattr(L, "mtr_engine_loudlog_series"):                # (an addition inside ABI version 2: the loudness log)
        L.mtr_engine_loudlog_set_period.argtypes = [vp, u32, u32, C.c_int]
        L.mtr_engine_loudlog_period.argtypes = [vp, C.POINTER(u32), C.POINTER(u32), C.POINTER(C.c_int)]
        L.mtr_engine_loudlog_series.argtypes = [vp, u32, u32, vp, vp, u32, vp, vp]
        L.mtr_engine_loudlog_reset.argtypes = [vp]
    if hasattr(L, "mtr_engine_integlog_series"):               # (an addition inside ABI version 2: the integration log)
        L.mtr_engine_integlog_set_every.argtypes = [vp, u32, u32]
        L.mtr_engine_integlog_every.argtypes = [vp, C.POINTER(u32), C.POINTER(u32)]
        L.mtr_engine_integlog_series.argtypes = [vp, u32, u32, vp, vp, vp, vp, vp, u32, vp, vp]
        L.mtr_engine_integlog_reset.argtypes = [vp]
        L.mtr_integlog_cut.argtypes = [u32, u64, u32, u64, C.POINTER(u64), C.POINTER(u64)]
    L.mtr_engine_prune_stats.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
    L.mtr_engine_refine_stats.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
    L.mtr_engine_layout.argtypes = [vp]
    L.mtr_engine_seg_stats.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
    L.mtr_plan_query.argtypes = [vp, u32, u64, u32, vp]
    L.mtr_comm_unique_id.argtypes = [vp]
    L.mtr_comm_init.argtypes = [C.POINTER(vp), i32, i32, vp, i32]
    L.mtr_comm_init_timeout.argtypes = [C.POINTER(vp), i32, i32, vp, i32, u32, C.POINTER(f32)]
    L.mtr_comm_probe.argtypes = [vp, u32, C.POINTER(f32)]
    L.mtr_comm_set_timeout.argtypes = [vp, u32]
    L.mtr_comm_nranks.argtypes = [vp]
    L.mtr_comm_device.argtypes = [vp]
    L.mtr_engine_set_deferred_tail.argtypes = [vp, C.c_int]
    L.mtr_engine_join.argtypes = [vp, vp]
    L.mtr_engine_deferred_stats.argtypes = [vp, C.POINTER(u64)]
    L.mtr_rccl_version.argtypes = []
    L.mtr_engine_state_bytes.argtypes = [vp, u32]
    L.mtr_engine_state_bytes.restype = C.c_size_t
    L.mtr_engine_state_export.argtypes = [vp, u32, u32, vp, C.c_size_t]
    L.mtr_engine_state_import.argtypes = [vp, u32, vp, C.c_size_t]
    L.mtr_state_blob_count.argtypes = [vp, C.c_size_t]
    L.mtr_state_blob_count.restype = u32
    L.mtr_comm_destroy.argtypes = [vp]
    L.mtr_comm_destroy.restype = None
    L.mtr_engine_reduce.argtypes = [vp, vp, vp, vp, vp]
    L.mtr_hist_loudness.argtypes = [vp, vp] + [C.POINTER(f32)] * 5
    L.mtr_hist_loudness.restype = None
    L.mtr_engine_timing_enable.argtypes = [vp, C.c_int]
    L.mtr_engine_timing_query.argtypes = [vp, C.POINTER(f32), C.POINTER(f32), C.POINTER(f32), C.POINTER(u32)]
    L.mtr_engine_timing_calls.argtypes = [vp, vp, u32, C.POINTER(u32)]
    L.mtr_kweight_coef.argtypes = [f32, vp]
    L.mtr_fir_table.argtypes = [vp]
    L.mtr_band_coef.argtypes = [C.c_double, u32, vp]
    L.mtr_synth_fill_device.argtypes = [vp, u32, u64, u64, u32, f32, C.c_int, vp]
    return L


lib = _load()
if b"TIMING-ONLY" in lib.mtr_version() and os.environ.get("MTR_ALLOW_TIMING_ONLY_BUILD") != "1":
    # a library built with -DMTR_TIMING_ONLY_BUILD may carry kernels with a role switched off (tools/: elimination runs): its
    # results are wrong by construction, and only the timing tools — which set the variable — may load it
    raise ImportError(f"{lib_path} is a TIMING-ONLY build ({lib.mtr_version().decode()}): it computes wrong results and is only "
                      "for the elimination runs under tools/ (MTR_ALLOW_TIMING_ONLY_BUILD=1)")


def _check(rc, what):
    if rc != 0:
        err = EngineError(f"{what} failed ({rc}): {lib.mtr_last_error().decode()}")
        err.code = rc
        raise err


def exported_symbols(header="mtr_engine.h"):
    """Every function include/mtr_engine.h — or one of the headers it includes, e.g. "mtr_needle.h" — declares itself, parsed from the
    header."""
    hdr = os.path.join(os.path.dirname(_HERE), "include", header)
    txt = re.sub(r"/\*.*?\*/", "", open(hdr).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(mtr_[a-z0-9_]+)\s*\(", txt)))


def kweight_coef(fs):
    out = np.zeros(7, np.float32)
    _check(lib.mtr_kweight_coef(fs, out.ctypes.data), "mtr_kweight_coef")
    return out


def fir_table():
    out = np.zeros(120, np.float32)
    _check(lib.mtr_fir_table(out.ctypes.data), "mtr_fir_table")
    return out


def band_coef(rate, band):
    out = np.zeros(36, np.float64)
    _check(lib.mtr_band_coef(float(rate), band, out.ctypes.data), "mtr_band_coef")
    return out.reshape(6, 6)


def stcorr_coef(fs):
    """(w1, w2) of Stcorrdsp::init ((int) fs, 2e3f, 0.3f) as float32."""
    out = np.zeros(2, np.float32)
    _check(lib.mtr_stcorr_coef(fs, out.ctypes.data), "mtr_stcorr_coef")
    return out


def scope_window(window_frames):
    """The Hann window of ft_gen_window (gui/fft.c) as float32 [window_frames], as MTR_METER_SCOPE applies it."""
    out = np.zeros(int(window_frames), np.float32)
    _check(lib.mtr_scope_window(int(window_frames), out.ctypes.data), "mtr_scope_window")
    return out


def scope_series_cut(fill, hop, since, every, n_frames):
    """(analyses, points): a call of n_frames to a SCOPE stream that stands `fill` frames behind its last analysis and `since` analyses
    behind its last series point completes `analyses` analyses of `hop` frames and appends `points` points, one per `every` analyses
    (every 0: the series is off, 0 points) (mtr_scope_series_cut; no device)."""
    if not hasattr(lib, "mtr_scope_series_cut"):
        raise EngineError(f"{lib_path} has no SCOPE reading series: rebuild it")
    an, pt = C.c_uint64(), C.c_uint64()
    _check(lib.mtr_scope_series_cut(int(fill), int(hop), int(since), int(every), int(n_frames), C.byref(an), C.byref(pt)), "mtr_scope_series_cut")
    return an.value, pt.value


def integlog_cut(div2, evaluations, every, n_fragments):
    """(evaluations, points) a stream gains from `n_fragments` integrating fragments when its _div2 stands at `div2` (0 .. 9) and it has
    made `evaluations` evaluations so far, a point per `every` evaluations (every 0: the log is off, 0 points) (mtr_integlog_cut; no
    device)."""
    if not hasattr(lib, "mtr_integlog_cut"):
        raise EngineError(f"{lib_path} has no integration log: rebuild it")
    ev, pt = C.c_uint64(), C.c_uint64()
    _check(lib.mtr_integlog_cut(int(div2), int(evaluations), int(every), int(n_fragments), C.byref(ev), C.byref(pt)), "mtr_integlog_cut")
    return ev.value, pt.value


def series_cut(fill, period, n_frames, frames):
    """(whole, partial): of a call of n_frames that starts `fill` frames into a block of `period`, a stream that takes `frames` completes
    `whole` blocks, and a truncated one follows them if partial == 1 (mtr_series_cut; no device)."""
    if not hasattr(lib, "mtr_series_cut"):
        raise EngineError(f"{lib_path} has no ragged batches: rebuild it")
    whole, partial = C.c_uint64(), C.c_uint32()
    _check(lib.mtr_series_cut(int(fill), int(period), int(n_frames), int(frames), C.byref(whole), C.byref(partial)), "mtr_series_cut")
    return whole.value, partial.value


def _need_gonio():
    if not hasattr(lib, "mtr_engine_gonio_image"):
        raise EngineError(f"{lib_path} has no goniometer (MTR_METER_GONIO): rebuild it")


def gonio_config(period_frames=0, capacity=0, shift=0, autogain=0, gain=0.0, point_width=0.0, dials=None, tune_piece=0):
    """A GonioConfig; zeros select the defaults.  autogain: False / 0 off, True / 1 on with the reference's dials; dials = (attack, decay,
    target, rms), 0 .. 100 each, selects autogain 2."""
    c = GonioConfig(struct_size=C.sizeof(GonioConfig), period_frames=int(period_frames), capacity=int(capacity), shift=int(shift),
                    autogain=int(autogain), gain=float(gain), point_width=float(point_width), tune_piece=int(tune_piece))
    if dials is not None:
        c.autogain = 2
        c.g_attack, c.g_decay, c.g_target, c.g_rms = [float(v) for v in dials]
    return c


def gonio_derive(rate, config=None, **kw):
    """GonioDerived for `config` (or gonio_config (**kw)) at `rate`: P, G, hpw, the two attack factors, g_target, g_rms
    (mtr_gonio_derive; no engine, no device)."""
    _need_gonio()
    c = config if config is not None else gonio_config(**kw)
    d = GonioDerived()
    _check(lib.mtr_gonio_derive(C.byref(c), float(rate), C.byref(d)), "mtr_gonio_derive")
    return d


def _need_gonio_os():
    if not hasattr(lib, "mtr_engine_gonio_set_oversample"):
        raise EngineError(f"{lib_path} has no oversampling for the goniometer: rebuild it")


def gonio_os_table(factor):
    """float32 [factor + 1, 12]: the interpolator's table for a factor of 2 .. 32, Resampler_table's _ctab (mtr_gonio_os_table; no engine,
    no device)."""
    _need_gonio_os()
    tab = np.zeros((max(int(factor), 0) + 1, 12), np.float32)
    _check(lib.mtr_gonio_os_table(int(factor), tab.ctypes.data), "mtr_gonio_os_table")
    return tab


def gonio_os_hpw(rate, factor):
    """the hpw the chain runs on at `rate` with `factor` (1 .. 32), a float32 (mtr_gonio_os_hpw; no engine, no device)."""
    _need_gonio_os()
    h = C.c_float()
    _check(lib.mtr_gonio_os_hpw(float(rate), int(factor), C.byref(h)), "mtr_gonio_os_hpw")
    return np.float32(h.value)


def _need_gonio_ends():
    if not hasattr(lib, "mtr_engine_process_device_gonio_ends"):
        raise EngineError(f"{lib_path} has no track lengths for the goniometer: rebuild it")


def gonio_cut(fill, period, rate, n_frames, frames, config=None, **kw):
    """(whole, closing_frames, drawn_frames, (attack0, attack1)) of a stream that takes `frames` of a call of n_frames which starts `fill`
    frames into a display update of `period` frames: the updates it completes, the frames of its closing update (0: none), the call frame
    at which its drawing ends, and the closing update's attack pair as float32 (mtr_gonio_cut; no engine, no device)."""
    _need_gonio_ends()
    c = config if config is not None else gonio_config(**kw)
    whole, closing, drawn, att = C.c_uint64(), C.c_uint32(), C.c_uint64(), (C.c_float * 2)()
    _check(lib.mtr_gonio_cut(int(fill), int(period), float(rate), int(n_frames), int(frames), C.byref(c), C.byref(whole), C.byref(closing),
                             C.byref(drawn), att), "mtr_gonio_cut")
    return whole.value, closing.value, drawn.value, (np.float32(att[0]), np.float32(att[1]))


def needle_coef(kind, fs):
    """(w1, w2, w3, g) of the needle meter `kind` (one NEEDLE_* bit) as float32; NEEDLE_VU: (w, 4 w, 0, g)."""
    out = np.zeros(4, np.float32)
    _check(lib.mtr_needle_coef(int(kind), fs, out.ctypes.data), "mtr_needle_coef")
    return out


def hist_loudness(hist_M, hist_S):
    """(integrated, integ_thr, range_min, range_max, range_thr) of (summed) histograms."""
    hm = np.ascontiguousarray(hist_M, np.int32)
    hs = np.ascontiguousarray(hist_S, np.int32)
    o = [C.c_float() for _ in range(5)]
    lib.mtr_hist_loudness(hm.ctypes.data, hs.ctypes.data, *[C.byref(x) for x in o])
    return tuple(x.value for x in o)


def plan_query(n_streams, n_frames, sample_rate=48000.0, meters=METER_EBU | METER_TRUEPEAK, frames_left_in_fragment=0, n_slots=0,
               n_channels=2, tune_run=0, tune_segments=0, tune_layout=0, tune_fir=0, tune_prune=0):
    """How an engine of this configuration would tile and route a call (no GPU needed)."""
    cfg = _Config(struct_size=C.sizeof(_Config), meters=meters, n_streams=n_streams, n_channels=n_channels, sample_rate=sample_rate,
                  device=0, max_frames=0, tune_run=tune_run, tune_segments=tune_segments, tune_layout=tune_layout, tune_fir=tune_fir,
                  tune_prune=tune_prune)
    info = PlanInfo()
    _check(lib.mtr_plan_query(C.byref(cfg), frames_left_in_fragment, n_frames, n_slots, C.byref(info)), "mtr_plan_query")
    return info.as_dict()


def _need_pcm():
    if not hasattr(lib, "mtr_engine_pcm_stats"):
        raise EngineError(f"{lib_path} has no integer PCM entry points: rebuild it")


def _pcm_format(x, format):
    """The MTR_PCM_* format of an array of integer samples: inferred from int16 / int32, PCM_S24 must be named (packed uint8)."""
    want = {np.dtype(np.int16): PCM_S16, np.dtype(np.int32): PCM_S32, np.dtype(np.uint8): PCM_S24}.get(x.dtype)
    if want is None:
        raise ValueError(f"integer PCM is int16 (PCM_S16), int32 (PCM_S32) or packed uint8 (PCM_S24), not {x.dtype}")
    if format is None and want == PCM_S24:
        raise ValueError("uint8 bytes: name the format (format=PCM_S24)")
    if format is not None and format != want:
        raise ValueError(f"format {format} does not go with dtype {x.dtype}")
    return want


def _samples(x, format, what, f32=True):
    """Array `x` as a source of samples: (format, bytes per sample, samples on the last axis).  Format 0 takes float32 (f32=False: the
    caller takes integers only); an integer format is checked against the dtype — None: inferred from it — by _pcm_format, and the last
    axis of PCM_S24's packed bytes holds whole samples: `what`."""
    if format == 0 and f32:
        if x.dtype != np.float32:
            raise ValueError(f"format 0 takes float32, not {x.dtype}")
        return 0, 4, x.shape[-1]
    fmt = _pcm_format(x, format)
    sb = {PCM_S16: 2, PCM_S24: 3, PCM_S32: 4}[fmt]
    if x.shape[-1] * x.itemsize % sb:
        raise ValueError(f"PCM_S24: the last axis holds {what}, not {x.shape}")
    return fmt, sb, x.shape[-1] * x.itemsize // sb


def pcm_decode(format, array):
    """mtr_pcm_decode_host: the integer samples of `array` (int16 for PCM_S16, int32 for PCM_S32, packed little-endian uint8 bytes
    for PCM_S24) as float32 — the same shape, PCM_S24 a third of the last axis.  The definition the GPU decode is held against."""
    _need_pcm()
    x = np.ascontiguousarray(array)
    format, _, n = _samples(x, format, "3 bytes per sample", f32=False)
    out = np.empty(x.shape[:-1] + (n,), np.float32)
    _check(lib.mtr_pcm_decode_host(format, x.ctypes.data, out.size, out.ctypes.data), "mtr_pcm_decode_host")
    return out


def _need_frames():
    if not hasattr(lib, "mtr_engine_set_frame_layout"):
        raise EngineError(f"{lib_path} has no frame layouts: rebuild it")


def pick_decode(format, array, map, n_channels=None):
    """mtr_pick_decode_host: frames of frame_channels samples to frames of n_channels (= len(map)) float32, channel c = source
    channel map[c].  The last axis of `array` is one frame: float32 [..., frame_channels] for format 0, int16 / int32
    [..., frame_channels] for PCM_S16 / PCM_S32, packed uint8 [..., frame_channels * 3] for PCM_S24.  Returns [..., n_channels].
    The definition the GPU pick is held against."""
    _need_frames()
    m = np.ascontiguousarray(map, np.uint8)
    n_channels = m.size if n_channels is None else n_channels
    if m.ndim != 1 or m.size != n_channels:
        raise ValueError(f"map: {n_channels} entries, not {m.shape}")
    x = np.ascontiguousarray(array)
    format, _, fc = _samples(x, format, "frame_channels * 3 bytes")
    out = np.empty(x.shape[:-1] + (n_channels,), np.float32)
    n_frames = out.size // n_channels
    _check(lib.mtr_pick_decode_host(int(format), x.ctypes.data, n_frames, fc, m.ctypes.data, n_channels, out.ctypes.data), "mtr_pick_decode_host")
    return out


def _need_planes():
    if not hasattr(lib, "mtr_engine_set_plane_layout"):
        raise EngineError(f"{lib_path} has no plane layouts: rebuild it")


def _plane_map(map, n_planes, n_channels):
    """the map of a plane (or frame) layout as uint8 [n_channels]; None: the identity, which needs n_planes == n_channels"""
    if map is None:
        if n_planes != n_channels:
            raise ValueError(f"map=None is the identity and needs {n_channels} planes, not {n_planes}")
        return np.arange(n_channels, dtype=np.uint8)
    m = np.ascontiguousarray(map, np.uint8)
    if m.shape != (n_channels,):
        raise ValueError(f"map: one entry per engine channel, shape ({n_channels},), not {m.shape}")
    return m


def plane_decode(format, array, map, n_channels=None, stride=None):
    """mtr_plane_decode_host on every stream of `array`: [..., P, n_frames] planes of one channel each — float32 for format 0, int16 /
    int32 for PCM_S16 / PCM_S32, packed uint8 [..., P, n_frames * 3] for PCM_S24 — to [..., n_frames, n_channels] float32, channel c =
    plane map[c] (map=None: the identity).  `array` is read where it lies: a view whose last axis is contiguous and whose planes lie
    `stride` samples apart (by default: what the view's strides say) is not copied, so the planes may be windows of longer ones, with
    anything behind their ends, and start on any byte.  The definition the GPU's k_plane is held against."""
    _need_planes()
    x = np.asarray(array)
    if x.ndim < 2:
        raise ValueError(f"planes: [..., P, n_frames], not {x.shape}")
    format, sb, n_frames = _samples(x, format, "n_frames * 3 bytes")
    P = x.shape[-2]
    if n_frames > 1 and x.strides[-1] != x.itemsize:
        raise ValueError(f"planes: the last axis must be contiguous, strides {x.strides}")
    if stride is None:
        stride = n_frames if P == 1 or n_frames == 0 else x.strides[-2] // sb
    if P > 1 and n_frames and x.strides[-2] != stride * sb:
        raise ValueError(f"planes {x.strides[-2]} bytes apart are not {stride} samples of {sb} bytes apart")
    n_channels = (P if map is None else len(map)) if n_channels is None else n_channels
    m = _plane_map(map, P, n_channels)
    out = np.empty(x.shape[:-2] + (n_frames, n_channels), np.float32)
    for idx in np.ndindex(*x.shape[:-2]):
        _check(lib.mtr_plane_decode_host(int(format), x[idx].ctypes.data, n_frames, int(stride), P, m.ctypes.data, n_channels,
                                         out[idx].ctypes.data), "mtr_plane_decode_host")
    return out


TensorSource = collections.namedtuple("TensorSource", "format kind width map n_frames stride")
_TENSOR_FORMATS = {"float32": 0, "int16": PCM_S16, "int32": PCM_S32}


def tensor_source(shape, strides, dtype, n_channels, channels_first=None, map=None):
    """How a process call takes a 3-D tensor as it lies, never a copy: a TensorSource (format: 0 / PCM_S16 / PCM_S32; kind: "frames" — a
    frame layout of `width` interleaved channels — or "planes" — a plane layout of `width` planes —; map: a tuple of n_channels entries;
    n_frames; stride: the call's stream_stride_frames), or ValueError.  shape and strides (in ELEMENTS) are the tensor's: (batch, time,
    channel) — channels last — with strides (st * W, W, 1), or (batch, channel, time) — channels first — with strides (P * st, st, 1), st >=
    n_frames either way (a window of a longer tensor has st = its length); an axis of one element may have any stride.  The width must be
    n_channels (map=None: the identity) or go with `map`.  channels_first=None decides from shape and strides, and refuses a tensor that
    fits both ways with different meanings.  No device and no torch are needed."""
    name = str(dtype).split(".")[-1]
    if name not in _TENSOR_FORMATS:
        raise ValueError(f"tensor dtype {dtype}: float32, int16 or int32 (24-bit PCM has no tensor dtype: process_pcm)")
    shape, strides = tuple(int(v) for v in shape), tuple(int(v) for v in strides)
    if len(shape) != 3 or len(strides) != 3:
        raise ValueError(f"a tensor of three axes, (batch, channel, time) or (batch, time, channel), not shape {shape} strides {strides}")
    if min(shape) < 1:
        raise ValueError(f"an empty tensor: shape {shape}")
    if min(strides) < 0:
        raise ValueError(f"negative strides {strides}: a flipped view is not taken (and never copied)")
    B, a, b = shape
    s0, s1, s2 = strides
    if b > 1 and s2 != 1:
        raise ValueError(f"the innermost stride must be 1: strides {strides} of shape {shape} (a transposed view is not taken, and never copied)")

    def width_ok(w):
        if map is None:
            return None if w == n_channels else f"width {w} is not n_channels = {n_channels} and there is no map"
        m = tuple(int(v) for v in map)
        if len(m) != n_channels or not 1 <= w <= 8 or max(m) >= w or min(m) < 0:
            return f"map {m} does not go with width {w} and n_channels = {n_channels}"
        return None

    def first():                                              # (B, P, T) with strides (P * st, st, 1)
        P, T = a, b
        st = s1 if P > 1 else s0 if B > 1 else T
        if st < T:
            return f"channels first: planes {st} apart are shorter than n_frames = {T} (strides {strides})"
        if B > 1 and s0 != P * st:
            return f"channels first: strides {strides} are not ({P} * st, st, 1)"
        return width_ok(P) or TensorSource(_TENSOR_FORMATS[name], "planes", P, tuple(range(P)) if map is None else tuple(int(v) for v in map), T, st)

    def last():                                               # (B, T, W) with strides (st * W, W, 1)
        T, W = a, b
        if T > 1 and s1 != W:
            return f"channels last: strides {strides} are not (st * {W}, {W}, 1)"
        if B > 1 and s0 % W:
            return f"channels last: strides {strides} are not (st * {W}, {W}, 1)"
        st = s0 // W if B > 1 else T
        if st < T:
            return f"channels last: streams {st} frames apart are shorter than n_frames = {T} (strides {strides})"
        return width_ok(W) or TensorSource(_TENSOR_FORMATS[name], "frames", W, tuple(range(W)) if map is None else tuple(int(v) for v in map), T, st)

    if channels_first is not None:
        r = first() if channels_first else last()
        if isinstance(r, str):
            raise ValueError(r)
        return r
    f, l = first(), last()
    if isinstance(f, str) and isinstance(l, str):
        raise ValueError(f"shape {shape} with strides {strides} is neither: {f}; {l}")
    if isinstance(f, str) or isinstance(l, str):
        return l if isinstance(f, str) else f
    if a == 1 and b == 1:
        return l                                              # (one sample per stream: the same either way)
    raise ValueError(f"shape {shape} with strides {strides} is {a} planes of {b} samples as well as {a} frames of {b} channels: say channels_first")


def synth_fill_device(ptr, n_streams, n_frames, stride, seed, fs=48000.0, kind=1, stream=0):
    _check(lib.mtr_synth_fill_device(ptr, n_streams, n_frames, stride, seed, fs, kind, stream),
           "mtr_synth_fill_device")


COMM_ID_BYTES = 128


def comm_unique_id():
    """Rank 0: the 128-byte RCCL id every rank needs for Comm(...)."""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    _check(lib.mtr_comm_unique_id(buf), "comm_unique_id")
    return bytes(buf.raw)


def rccl_version():
    """ncclGetVersion of the RCCL this process runs, e.g. 22606."""
    v = lib.mtr_rccl_version()
    if v < 0:
        _check(v, "rccl_version")
    return v


class Comm:
    """mtr_comm: one RCCL communicator per rank (ncclCommInitRank is collective: every rank constructs its own).
    timeout_ms > 0: mtr_comm_init_timeout — the creation (and every later call on the communicator) is polled to that
    deadline and raises EngineError with code ERR_TIMEOUT instead of hanging; `.init_ms` is how long the creation took."""

    def __init__(self, rank, world, unique_id, device=0, timeout_ms=0):
        self._h = C.c_void_p()
        self.world = world
        buf = C.create_string_buffer(bytes(unique_id), COMM_ID_BYTES)
        ms = C.c_float()
        _check(lib.mtr_comm_init_timeout(C.byref(self._h), rank, world, buf, device, int(timeout_ms), C.byref(ms)), "comm_init")
        self.init_ms = ms.value

    def probe(self, timeout_ms=0):
        """The job's first collective (one 4-byte all-reduce on the communicator's own stream), bounded; returns its ms."""
        ms = C.c_float()
        _check(lib.mtr_comm_probe(self._h, int(timeout_ms), C.byref(ms)), "comm_probe")
        return ms.value

    def set_timeout(self, timeout_ms):
        _check(lib.mtr_comm_set_timeout(self._h, int(timeout_ms)), "comm_set_timeout")

    def nranks(self):
        """ncclCommCount: the ranks RCCL itself sees in this communicator."""
        n = lib.mtr_comm_nranks(self._h)
        if n < 0:
            _check(n, "comm_nranks")
        return n

    def device(self):
        """ncclCommCuDevice: the device RCCL bound this rank to."""
        d = lib.mtr_comm_device(self._h)
        if d < 0:
            _check(d, "comm_device")
        return d

    def close(self):
        if self._h:
            lib.mtr_comm_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class Engine:
    def __init__(self, n_streams, sample_rate=48000.0, meters=METER_EBU | METER_TRUEPEAK,
                 n_channels=2, device=0, tune_run=0, tune_segments=0, tune_layout=0, tune_fir=0, tune_prune=0):
        cfg = _Config(struct_size=C.sizeof(_Config), meters=meters, n_streams=n_streams,
                      n_channels=n_channels, sample_rate=sample_rate, device=device,
                      max_frames=0, tune_run=tune_run, tune_segments=tune_segments,
                      tune_layout=tune_layout, tune_fir=tune_fir, tune_prune=tune_prune)
        self._h = C.c_void_p()
        self.n_streams, self.meters, self.sample_rate, self.n_channels = n_streams, meters, sample_rate, n_channels
        self._device = device
        _check(lib.mtr_engine_create(C.byref(cfg), C.byref(self._h)), "mtr_engine_create")

    def close(self):
        if getattr(self, "_h", None):
            lib.mtr_engine_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def reset(self):
        _check(lib.mtr_engine_reset(self._h), "reset")

    def integr_start(self):
        _check(lib.mtr_engine_integr_start(self._h), "integr_start")

    def integr_pause(self):
        _check(lib.mtr_engine_integr_pause(self._h), "integr_pause")

    def integr_reset(self):
        _check(lib.mtr_engine_integr_reset(self._h), "integr_reset")

    def truepeak_reset(self):
        _check(lib.mtr_engine_truepeak_reset(self._h), "truepeak_reset")

    def spectr_set_speed(self, v):
        _check(lib.mtr_engine_spectr_set_speed(self._h, v), "spectr_set_speed")

    def spectr_reset_peak(self):
        _check(lib.mtr_engine_spectr_reset_peak(self._h), "spectr_reset_peak")

    def process_device(self, ptr, n_frames, stride=None, stream=0):
        _check(lib.mtr_engine_process_device(self._h, ptr, n_frames, stride or n_frames, stream), "process_device")

    def _frames_f32(self, x):
        """x as contiguous float32 [S, T, W] (or [S, T] where W == 1), W = the frame width the process calls take: n_channels, or
        frame_channels once a layout is set — a narrower array would be read past its end, a wider one mis-metered"""
        x = np.ascontiguousarray(x, np.float32)
        W = self._width()
        if x.shape[:1] != (self.n_streams,) or not (x.ndim == 3 and x.shape[2] == W or (W == 1 and x.ndim == 2)):
            raise ValueError(f"float32 [{self.n_streams}, T, {W}]" + (" or [S, T]" if W == 1 else "") + f", not {x.shape}")
        return x

    def process(self, x):
        """x: host float32 [S, T, W] (or [S, T] where W == 1), W = n_channels, or frame_channels once set_frame_layout() set one."""
        x = self._frames_f32(x)
        _check(lib.mtr_engine_process_host(self._h, x.ctypes.data, x.shape[1], x.shape[1]), "process_host")

    # the families of calls with per-stream ends: the symbol whose absence means "rebuild the library", and what the library then lacks
    _FAMILY = {"lengths": ("mtr_engine_stream_frames", "per-stream lengths"), "tracks": ("mtr_engine_process_device_tracks", "track lengths"),
               "ragged": ("mtr_engine_process_device_ragged", "ragged batches"),
               "ends": ("mtr_engine_process_device_ends", "track lengths for the 30-band bank"),
               "tpb": ("mtr_engine_process_device_tpb", "track lengths for the true-peak bar"),
               "any": ("mtr_engine_process_device_any", "track lengths for the scope and the surround meter"),
               "gonio_ends": ("mtr_engine_process_device_gonio_ends", "track lengths for the goniometer")}

    def _frames(self, frames, family):
        """frames as contiguous uint64 [S], for a call of `family`"""
        symbol, what = self._FAMILY[family]
        if not hasattr(lib, symbol):
            raise EngineError(f"{lib_path} has no {what}: rebuild it")
        f = np.ascontiguousarray(frames, np.uint64)
        if f.shape != (self.n_streams,):
            raise ValueError(f"frames: one length per stream, shape ({self.n_streams},), not {f.shape}")
        return f

    def _device_frames(self, family, ptr, n_frames, frames, stride, stream):
        f = self._frames(frames, family)
        _check(getattr(lib, "mtr_engine_process_device_" + family)(self._h, ptr, n_frames, stride or n_frames, f.ctypes.data, stream),
               "process_device_" + family)

    def _host_frames(self, family, x, frames):
        x = self._frames_f32(x)
        f = self._frames(frames, family)
        _check(getattr(lib, "mtr_engine_process_host_" + family)(self._h, x.ctypes.data, x.shape[1], x.shape[1], f.ctypes.data),
               "process_host_" + family)

    def process_device_lengths(self, ptr, n_frames, frames, stride=None, stream=0):
        """Advance stream s by frames[s] <= n_frames frames of the device buffer at `ptr`; a stream with frames[s] < n_frames
        is closed by the call (its results are final until reset()), frames[s] == n_frames leaves it open."""
        self._device_frames("lengths", ptr, n_frames, frames, stride, stream)

    def process_lengths(self, x, frames):
        """process() with per-stream lengths: x host float32 [S, T, W] as process() takes it, frames [S] <= T."""
        self._host_frames("lengths", x, frames)

    def process_device_tracks(self, ptr, n_frames, frames, stride=None, stream=0):
        """process_device_lengths() for engines of EBU, TRUEPEAK, DR14, KMETER, BITSTATS and SIGDIST in any combination: stream s is
        metered up to frames[s] <= n_frames, as by a host that stops calling run() at the track's end; frames[s] < n_frames closes it."""
        self._device_frames("tracks", ptr, n_frames, frames, stride, stream)

    def process_tracks(self, x, frames):
        """process() with track lengths: x host float32 [S, T, W] as process() takes it, frames [S] <= T."""
        self._host_frames("tracks", x, frames)

    def process_device_ragged(self, ptr, n_frames, frames, stride=None, stream=0):
        """process_device_tracks() for engines that also hold STCORR or NEEDLE: stream s is metered up to frames[s] <= n_frames, the
        block it ends in truncated there (one last process () and read (), the stream's last point); frames[s] < n_frames closes it."""
        self._device_frames("ragged", ptr, n_frames, frames, stride, stream)

    def process_ragged(self, x, frames):
        """process() as a ragged batch: x host float32 [S, T, W] as process() takes it, frames [S] <= T."""
        self._host_frames("ragged", x, frames)

    def series_points(self, meter, first=0, count=None):
        """[count] uint64: the points each stream's own STCORR, NEEDLE, KMETER or SURROUND series (meter: METER_STCORR / METER_NEEDLE / METER_KMETER /
        METER_SURROUND) has got since reset, dropped ones included — of a stream that a call with track lengths closed, its whole blocks and
        the truncated one."""
        self._frames(np.zeros(self.n_streams, np.uint64), "ragged")
        count = self.n_streams - first if count is None else count
        out = np.zeros(count, np.uint64)
        _check(lib.mtr_engine_series_points(self._h, int(meter), first, count, out.ctypes.data), "series_points")
        return out

    def process_device_ends(self, ptr, n_frames, frames, stride=None, stream=0):
        """process_device_ragged() for engines that also hold SPECTR30: stream s is metered up to frames[s] <= n_frames — the bank's
        spectrum_run ends there with its epilogue and, with a period, a truncated last point; frames[s] < n_frames closes it."""
        self._device_frames("ends", ptr, n_frames, frames, stride, stream)

    def process_ends(self, x, frames):
        """process() with track lengths for the bank: x host float32 [S, T, W] as process() takes it, frames [S] <= T."""
        self._host_frames("ends", x, frames)

    def spectr_points(self, first=0, count=None):
        """[count] uint64: the points each stream's own SPECTR30 series has got since reset, dropped ones included — of a stream that
        process_*_ends closed, its whole blocks and the truncated one."""
        self._frames(np.zeros(self.n_streams, np.uint64), "ends")
        count = self.n_streams - first if count is None else count
        out = np.zeros(count, np.uint64)
        _check(lib.mtr_engine_spectr_points(self._h, first, count, out.ctypes.data), "spectr_points")
        return out

    def process_device_tpb(self, ptr, n_frames, frames, stride=None, stream=0):
        """process_device_ends() for engines that also hold TPBALLIST: stream s is metered up to frames[s] <= n_frames — the true-peak
        bar's process () ends there with its read () and, with a period, a truncated last point; frames[s] < n_frames closes it."""
        self._device_frames("tpb", ptr, n_frames, frames, stride, stream)

    def process_tpb(self, x, frames):
        """process() with track lengths for the true-peak bar: x host float32 [S, T, W] as process() takes it, frames [S] <= T."""
        self._host_frames("tpb", x, frames)

    def tpb_points(self, first=0, count=None):
        """[count] uint64: the points each stream's own TPBALLIST series has got since reset, dropped ones included — of a stream that
        process_*_tpb closed, its whole blocks and the truncated one."""
        self._frames(np.zeros(self.n_streams, np.uint64), "tpb")
        count = self.n_streams - first if count is None else count
        out = np.zeros(count, np.uint64)
        _check(lib.mtr_engine_tpb_points(self._h, first, count, out.ctypes.data), "tpb_points")
        return out

    def process_device_any(self, ptr, n_frames, frames, stride=None, stream=0):
        """process_device_tpb() for engines that also hold SCOPE, and for SURROUND engines (3 .. 8 channels, beside EBU / TRUEPEAK up to
        5): stream s is metered up to frames[s] <= n_frames — the scope runs the analyses that end at or before its last frame, the
        surround meter one last sur_run of the frames the stream has of its block — as under a host that stops feeding it there;
        frames[s] < n_frames closes it.  (One call is refused: SURROUND with a period, the open block inside a group of four frames, and
        a stream that ends before that group completes.)"""
        self._device_frames("any", ptr, n_frames, frames, stride, stream)

    def process_any(self, x, frames):
        """process() with track lengths for the scope and the surround meter: x host float32 [S, T, W] as process() takes it, frames [S] <= T."""
        self._host_frames("any", x, frames)

    def scope_points(self, first=0, count=None):
        """(analyses, points), [count] uint64 each: the analyses each stream's own SCOPE has run since reset and the points its own
        series has got (dropped ones included; 0 without a series) — of a stream that process_*_any closed, those that end at or
        before its last frame."""
        if not hasattr(lib, "mtr_engine_scope_points"):
            raise EngineError(f"{lib_path} has no {self._FAMILY['any'][1]}: rebuild it")
        count = self.n_streams - first if count is None else count
        an, pt = np.zeros(count, np.uint64), np.zeros(count, np.uint64)
        _check(lib.mtr_engine_scope_points(self._h, first, count, an.ctypes.data, pt.ctypes.data), "scope_points")
        return an, pt

    def process_pcm(self, x, format=None, frames=None):
        """process() for host integer PCM, decoded on the GPU: x int16 or int32 [S, T, C] (or [S, T] mono; the format is inferred),
        or packed 24-bit samples as uint8 [S, T * C * 3] with format=PCM_S24.  frames: per-stream lengths as process_lengths()."""
        _need_pcm()
        x = np.ascontiguousarray(x)
        C_ = self._width()                                       # (frames of frame_channels samples once a layout is set)
        fmt = _samples(x, format, f"T * {C_} * 3 bytes", f32=False)[0]
        if fmt == PCM_S24:
            if x.ndim != 2 or x.shape[0] != self.n_streams or x.shape[1] % (3 * C_):
                raise ValueError(f"PCM_S24: uint8 [{self.n_streams}, T * {C_} * 3], not {x.shape}")
            n = x.shape[1] // (3 * C_)
        else:
            if x.shape[:1] != (self.n_streams,) or not (x.shape[2:] == (C_,) and x.ndim == 3 or (C_ == 1 and x.ndim == 2)):
                raise ValueError(f"integer PCM: [{self.n_streams}, T, {C_}]" + (" or [S, T]" if C_ == 1 else "") + f", not {x.shape}")
            n = x.shape[1]
        self.process_raw(x.ctypes.data, n, n, fmt, frames, host=True)

    def process_device_pcm(self, ptr, format, n_frames, stride=None, frames=None, stream=0):
        """process_device() for integer PCM in device memory at `ptr` (stream s at ptr + s * stride * n_channels * sample bytes): one
        decode pass on top of the meters.  frames: per-stream lengths as process_device_lengths()."""
        _need_pcm()
        f = None if frames is None else self._frames(frames, "lengths")
        _check(lib.mtr_engine_process_device_pcm(self._h, ptr, int(format), n_frames, stride or n_frames,
                                                 None if f is None else f.ctypes.data, stream), "process_device_pcm")

    def pcm_stats(self):
        """(PCM chunks decoded, bytes of PCM taken, ms of the decode kernels while timing was on) since the engine was created."""
        _need_pcm()
        a, b, ms = C.c_uint64(), C.c_uint64(), C.c_float()
        _check(lib.mtr_engine_pcm_stats(self._h, C.byref(a), C.byref(b), C.byref(ms)), "pcm_stats")
        return a.value, b.value, ms.value

    def set_frame_layout(self, frame_channels, map=None):
        """The buffers of every later process call hold frames of `frame_channels` samples, engine channel c = source channel map[c]
        (mtr_engine_set_frame_layout); frame_channels 0: back to frames of n_channels.  process / process_lengths / process_pcm then take
        [S, T, frame_channels] arrays (PCM_S24: uint8 [S, T * frame_channels * 3])."""
        _need_frames()
        m = None if map is None else np.ascontiguousarray(map, np.uint8)
        if m is not None and m.shape != (self.n_channels,):
            raise ValueError(f"map: one source channel per engine channel, shape ({self.n_channels},), not {m.shape}")
        _check(lib.mtr_engine_set_frame_layout(self._h, int(frame_channels), None if m is None else m.ctypes.data), "set_frame_layout")

    def frame_layout(self):
        """(frame_channels, map) as mtr_engine_frame_layout reads them back: map a tuple of n_channels source channels."""
        _need_frames()
        fc, m = C.c_uint32(), np.zeros(self.n_channels, np.uint8)
        _check(lib.mtr_engine_frame_layout(self._h, C.byref(fc), m.ctypes.data), "frame_layout")
        return fc.value, tuple(int(v) for v in m)

    def layout_stats(self):
        """(chunks that went through the pick kernel, process calls whose kernel read the wide frames itself) since create"""
        _need_frames()
        a, b = C.c_uint64(), C.c_uint64()
        _check(lib.mtr_engine_layout_stats(self._h, C.byref(a), C.byref(b)), "layout_stats")
        return a.value, b.value

    def set_plane_layout(self, n_planes, map=None):
        """The buffers of every later process call hold, per stream, `n_planes` planes of one channel each, the call's stride counting
        from plane to plane; engine channel c = plane map[c] (mtr_engine_set_plane_layout, include/mtr_planes.h).  map=None: the identity,
        which needs n_planes == n_channels; n_planes 0: back to the default.  It takes a frame layout away, as set_frame_layout takes this
        one.  The host wrappers that check an array's shape (process, process_pcm, ...) go on expecting frames: planar buffers go through
        process_tensor or process_raw."""
        _need_planes()
        m = None if not n_planes else _plane_map(map, int(n_planes), self.n_channels)
        _check(lib.mtr_engine_set_plane_layout(self._h, int(n_planes), None if m is None else m.ctypes.data), "set_plane_layout")

    def plane_layout(self):
        """(n_planes, map) as mtr_engine_plane_layout reads them back: n_planes 0 without a plane layout."""
        _need_planes()
        p, m = C.c_uint32(), np.zeros(self.n_channels, np.uint8)
        _check(lib.mtr_engine_plane_layout(self._h, C.byref(p), m.ctypes.data), "plane_layout")
        return p.value, tuple(int(v) for v in m)

    def plane_stats(self):
        """chunks that went through the plane kernel since create"""
        _need_planes()
        a = C.c_uint64()
        _check(lib.mtr_engine_plane_stats(self._h, C.byref(a)), "plane_stats")
        return a.value

    def process_raw(self, ptr, n_frames, stride=None, format=0, frames=None, family=None, host=False, stream=0):
        """One process call on the buffer at address `ptr` as the layout in force describes it — host memory (host=True) or device memory
        on `stream` —, nothing about it checked here: format 0 = float32, else PCM_*; frames: per-stream lengths; family: the pair of
        entry points, by the names _device_frames / _host_frames use ("lengths", "tracks", "ragged", "ends", "tpb", "any", "gonio_ends"),
        None: the plain call, the _lengths call with frames, the _pcm call for integer samples."""
        stride = stride or n_frames
        if format and family not in (None, "lengths"):
            raise ValueError(f"integer PCM goes through the _pcm entry points, with per-stream lengths or without: no family {family!r}")
        if frames is None and family is not None:
            raise ValueError(f"family {family!r} takes per-stream lengths: frames")
        if not host:                                             # the device forms: the wrappers above, which check nothing about a buffer
            if format:
                self.process_device_pcm(ptr, format, n_frames, stride, frames, stream)
            elif frames is None:
                self.process_device(ptr, n_frames, stride, stream)
            else:
                self._device_frames(family or "lengths", ptr, n_frames, frames, stride, stream)
            return
        # the host forms: the wrappers above take arrays and check their shape against a frame layout, so the entry points themselves
        if format:
            _need_pcm()
            f = None if frames is None else self._frames(frames, "lengths")
            _check(lib.mtr_engine_process_host_pcm(self._h, ptr, int(format), n_frames, stride, None if f is None else f.ctypes.data), "process_host_pcm")
        elif frames is None:
            _check(lib.mtr_engine_process_host(self._h, ptr, n_frames, stride), "process_host")
        else:
            family = family or "lengths"
            f = self._frames(frames, family)
            _check(getattr(lib, "mtr_engine_process_host_" + family)(self._h, ptr, n_frames, stride, f.ctypes.data), "process_host_" + family)

    def process_tensor(self, t, channels_first=None, map=None, frames=None, family=None):
        """One process call on a tensor as it lies: a torch tensor — on the engine's device: the device entry point on
        torch.cuda.current_stream (); on the CPU: the host entry point — or a numpy array (host), float32 / int16 / int32, (batch, channel,
        time) or (batch, time, channel), contiguous or a window in time of a longer one: what tensor_source () accepts, which also says how
        channels_first and map are read.  Nothing is copied or transposed on the way: the call runs under the frame or plane layout the
        tensor needs, and the layout that stood before stands again afterwards, also after an error.  frames / family as process_raw."""
        _need_planes()
        if hasattr(t, "data_ptr") and hasattr(t, "stride"):                  # a torch tensor
            shape, strides, dev = tuple(t.shape), tuple(t.stride()), t.device
            host = dev.type == "cpu"
            if not host and (dev.type != "cuda" or dev.index != self._device):
                raise ValueError(f"a tensor on {dev}: the engine is on device {self._device}")
            ptr = t.data_ptr()
        elif isinstance(t, np.ndarray):
            if any(v % t.itemsize for v in t.strides):
                raise ValueError(f"strides {t.strides} of {t.dtype} are no whole elements")
            shape, strides, host, ptr = t.shape, tuple(v // t.itemsize for v in t.strides), True, t.ctypes.data
        else:
            raise ValueError(f"a torch tensor or a numpy array, not {type(t).__name__}")
        src = tensor_source(shape, strides, t.dtype, self.n_channels, channels_first, map)
        if shape[0] != self.n_streams:
            raise ValueError(f"{shape[0]} streams in a tensor of shape {tuple(shape)}: the engine has {self.n_streams}")
        stream = 0
        if not host:
            import torch
            stream = torch.cuda.current_stream(t.device).cuda_stream
        before_p, before_f = self.plane_layout(), self.frame_layout()
        try:
            if src.kind == "planes":
                self.set_plane_layout(src.width, src.map)
            else:
                self.set_frame_layout(src.width, src.map)
            self.process_raw(ptr, src.n_frames, src.stride, src.format, frames, family, host, stream)
        finally:
            if before_p[0]:
                self.set_plane_layout(*before_p)
            else:
                self.set_frame_layout(*before_f)

    def _width(self):
        """samples per frame of the buffers a process call takes"""
        return self.frame_layout()[0] if hasattr(lib, "mtr_engine_set_frame_layout") else self.n_channels

    def stream_frames(self, first=0, count=None):
        """(frames, closed): [count] uint64 frames metered per stream since create / reset, [count] bool closed."""
        if not hasattr(lib, "mtr_engine_stream_frames"):
            raise EngineError(f"{lib_path} has no per-stream lengths: rebuild it")
        count = self.n_streams - first if count is None else count
        frames = np.zeros(count, np.uint64)
        closed = np.zeros(count, np.uint8)
        _check(lib.mtr_engine_stream_frames(self._h, first, count, frames.ctypes.data, closed.ctypes.data), "stream_frames")
        return frames, closed.astype(bool)

    def set_host_chunk_bytes(self, n):
        """Bytes of audio per chunk of process() (host memory crosses the link chunk by chunk under the kernels)."""
        _check(lib.mtr_engine_set_host_chunk_bytes(self._h, n), "set_host_chunk_bytes")

    def process_planar(self, chans):
        arrs = [np.ascontiguousarray(c, np.float32) for c in chans]
        ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
        _check(lib.mtr_engine_process_planar_host(self._h, ptrs, arrs[0].size), "process_planar_host")

    def sync(self):
        _check(lib.mtr_engine_sync(self._h), "sync")

    def set_deferred_tail(self, mode):
        """0 auto / 1 never / 2 always: k_gate (and the reduction) of a call on the engine's side stream, beside the next call."""
        _check(lib.mtr_engine_set_deferred_tail(self._h, int(mode)), "set_deferred_tail")

    def join(self, stream=0):
        """`stream` waits for what the engine's side stream holds (before reading reduce()'s buffers in stream order)."""
        _check(lib.mtr_engine_join(self._h, stream), "join")

    def deferred_calls(self):
        n = C.c_uint64()
        _check(lib.mtr_engine_deferred_stats(self._h, C.byref(n)), "deferred_stats")
        return n.value

    def results(self, first=0, count=None):
        count = self.n_streams - first if count is None else count
        out = (StreamResult * count)()
        _check(lib.mtr_engine_results(self._h, first, count, out), "results")
        return out

    def out9(self, first=0, count=None):
        """[count, 9] float32: M, maxM, S, maxS, I, I_thr, Rmin, Rmax, R_thr."""
        r = self.results(first, count)
        return np.array([[getattr(x, f[0]) for f in StreamResult._fields_[:9]] for x in r], np.float32)

    def truepeak(self, first=0, count=None):
        r = self.results(first, count)
        return np.array([[x.truepeak[0], x.truepeak[1]] for x in r], np.float32)

    def truepeak_channels(self, first=0, count=None):
        """(hold, last): [count, n_channels] float32 — per channel, the max-hold since reset and the most recent call's peak."""
        if not hasattr(lib, "mtr_engine_truepeak_channels"):
            raise EngineError(f"{lib_path} has no mtr_engine_truepeak_channels: rebuild it")
        count = self.n_streams - first if count is None else count
        hold = np.zeros((count, self.n_channels), np.float32)
        last = np.zeros((count, self.n_channels), np.float32)
        _check(lib.mtr_engine_truepeak_channels(self._h, first, count, hold.ctypes.data, last.ctypes.data), "truepeak_channels")
        return hold, last

    def histograms(self, first=0, count=None):
        count = self.n_streams - first if count is None else count
        hm = np.zeros((count, HIST_LEN), np.int32)
        hs = np.zeros((count, HIST_LEN), np.int32)
        _check(lib.mtr_engine_histograms(self._h, first, count, hm.ctypes.data, hs.ctypes.data), "histograms")
        return hm, hs

    def fragment_powers(self, first=0, count=None):
        count = self.n_streams - first if count is None else count
        n = C.c_uint32()
        _check(lib.mtr_engine_fragment_powers(self._h, first, count, None, 0, C.byref(n)), "fragment_powers")
        out = np.zeros((count, max(n.value, 1)), np.float32)
        _check(lib.mtr_engine_fragment_powers(self._h, first, count, out.ctypes.data, out.shape[1], C.byref(n)),
               "fragment_powers")
        return out[:, :n.value]

    def spectrum(self, first=0, count=None):
        count = self.n_streams - first if count is None else count
        a = [np.zeros((count, NBANDS), np.float32) for _ in range(4)]
        _check(lib.mtr_engine_spectrum(self._h, first, count, *[x.ctypes.data for x in a]), "spectrum")
        return dict(val=a[0], max=a[1], val_db=a[2], max_db=a[3])

    def spectr_set_period(self, period_frames, capacity_points=0, peak_mode=SPECTR_PEAK_HOLD):
        """0: every call is one spectrum_run; P > 0: blocks of exactly P frames wherever the calls cut the audio, (val, max) of the 30
        bands after each appended to a series of `capacity_points` per stream; SPECTR_PEAK_BLOCK zeroes max behind every point.  Only
        before the first process call since create / reset."""
        if not hasattr(lib, "mtr_engine_spectr_series"):
            raise EngineError(f"{lib_path} has no SPECTR30 reading series: rebuild it")
        _check(lib.mtr_engine_spectr_set_period(self._h, int(period_frames), int(capacity_points), int(peak_mode)), "spectr_set_period")

    def spectr_period(self):
        """(period_frames, capacity_points, peak_mode) as spectr_set_period set them."""
        if not hasattr(lib, "mtr_engine_spectr_series"):
            raise EngineError(f"{lib_path} has no SPECTR30 reading series: rebuild it")
        p, c, m = C.c_uint32(), C.c_uint32(), C.c_int()
        _check(lib.mtr_engine_spectr_period(self._h, C.byref(p), C.byref(c), C.byref(m)), "spectr_period")
        return p.value, c.value, m.value

    def spectr_series(self, first=0, count=None):
        """(dict(val, max, val_db, max_db) of [count, kept, 30] arrays, n_points, dropped): the readings after every completed block
        since reset that the series holds."""
        if not hasattr(lib, "mtr_engine_spectr_series"):
            raise EngineError(f"{lib_path} has no SPECTR30 reading series: rebuild it")
        a, n, d = self._series("spectr_series", first, count, [(NBANDS,)] * 4,
                               lambda count, ptrs, *tail: lib.mtr_engine_spectr_series(self._h, first, count, *ptrs, *tail))
        return dict(val=a[0], max=a[1], val_db=a[2], max_db=a[3]), n, d

    def bitstats(self, first=0, count=None):
        count = self.n_streams - first if count is None else count
        hist = np.zeros((count, BIM_LAST), np.int32)
        cnt = np.zeros((count, 5), np.int32)
        mm = np.zeros((count, 2), np.float32)
        _check(lib.mtr_engine_bitstats(self._h, first, count, hist.ctypes.data, cnt.ctypes.data, mm.ctypes.data), "bitstats")
        return dict(hist=hist, counters=cnt, vmin=mm[:, 0], vmax=mm[:, 1])

    def dr14(self, first=0, count=None):
        count = self.n_streams - first if count is None else count
        out = (Dr14Result * count)()
        _check(lib.mtr_engine_dr14_results(self._h, first, count, out), "dr14_results")
        return out

    def kmeter_read(self, first=0, count=None):
        """Kmeterdsp::read for every stream: (rms, peak) as [count, 2] arrays; arms the new-maximum flag."""
        count = self.n_streams - first if count is None else count
        rms = np.zeros((count, 2), np.float32)
        peak = np.zeros((count, 2), np.float32)
        _check(lib.mtr_engine_kmeter_read(self._h, first, count, rms.ctypes.data, peak.ctypes.data), "kmeter_read")
        return rms, peak

    def kmeter_reset(self):
        _check(lib.mtr_engine_kmeter_reset(self._h), "kmeter_reset")

    def kmeter_set_period(self, period_frames, capacity_points=0):
        """0: every call is one Kmeterdsp::process (); P > 0: blocks of exactly P frames wherever the calls cut the audio, read (rms, peak)
        after each appended to a series of `capacity_points` per stream; kmeter_read() then returns the last completed block's and arms
        nothing.  Only before the first process call since create / reset."""
        if not hasattr(lib, "mtr_engine_kmeter_series"):
            raise EngineError(f"{lib_path} has no K-meter reading series: rebuild it")
        _check(lib.mtr_engine_kmeter_set_period(self._h, int(period_frames), int(capacity_points)), "kmeter_set_period")

    def kmeter_period(self):
        """(period_frames, capacity_points) as kmeter_set_period set them."""
        if not hasattr(lib, "mtr_engine_kmeter_series"):
            raise EngineError(f"{lib_path} has no K-meter reading series: rebuild it")
        p, c = C.c_uint32(), C.c_uint32()
        _check(lib.mtr_engine_kmeter_period(self._h, C.byref(p), C.byref(c)), "kmeter_period")
        return p.value, c.value

    def kmeter_series(self, first=0, count=None):
        """(rms [count, kept, C], peak [count, kept, C], n_points, dropped): (rms, peak) after every completed block since reset that
        the series holds."""
        if not hasattr(lib, "mtr_engine_kmeter_series"):
            raise EngineError(f"{lib_path} has no K-meter reading series: rebuild it")
        (rms, peak), n, d = self._series("kmeter_series", first, count, [(self.n_channels,)] * 2,
                                         lambda count, ptrs, *tail: lib.mtr_engine_kmeter_series(self._h, first, count, *ptrs, *tail))
        return rms, peak, n, d

    def tpb_set_period(self, period_frames, capacity_points=0):
        """0: every call is one TruePeakdsp::process () + read (m, p); P in 16 .. 8192: blocks of exactly P frames wherever the calls cut
        the audio, read (m, p) after each appended to a series of `capacity_points` per stream; results() then reports the last completed
        block's tpb_level / tpb_peak.  Only before the first process call since create / reset."""
        if not hasattr(lib, "mtr_engine_tpb_series"):
            raise EngineError(f"{lib_path} has no true-peak reading series: rebuild it")
        _check(lib.mtr_engine_tpb_set_period(self._h, int(period_frames), int(capacity_points)), "tpb_set_period")

    def tpb_period(self):
        """(period_frames, capacity_points) as tpb_set_period set them."""
        if not hasattr(lib, "mtr_engine_tpb_series"):
            raise EngineError(f"{lib_path} has no true-peak reading series: rebuild it")
        p, c = C.c_uint32(), C.c_uint32()
        _check(lib.mtr_engine_tpb_period(self._h, C.byref(p), C.byref(c)), "tpb_period")
        return p.value, c.value

    def tpb_series(self, first=0, count=None):
        """(level [count, kept, C], peak [count, kept, C], n_points, dropped): read (m, p) after every completed block since reset that
        the series holds."""
        if not hasattr(lib, "mtr_engine_tpb_series"):
            raise EngineError(f"{lib_path} has no true-peak reading series: rebuild it")
        (level, peak), n, d = self._series("tpb_series", first, count, [(self.n_channels,)] * 2,
                                           lambda count, ptrs, *tail: lib.mtr_engine_tpb_series(self._h, first, count, *ptrs, *tail))
        return level, peak, n, d

    def stcorr_set_period(self, period_frames, capacity_points=0):
        """0: every call is one Stcorrdsp::process (); P > 0: blocks of exactly P frames wherever the calls cut the audio, read () after
        each appended to a series of `capacity_points` per stream.  Only before the first process call since create / reset."""
        _check(lib.mtr_engine_stcorr_set_period(self._h, int(period_frames), int(capacity_points)), "stcorr_set_period")

    def stcorr_read(self, first=0, count=None):
        """(corr [count], state5 [count, 5] = zl zr zlr zll zrr): Stcorrdsp::read () after the most recent call / completed period."""
        count = self.n_streams - first if count is None else count
        corr = np.zeros(count, np.float32)
        st = np.zeros((count, 5), np.float32)
        _check(lib.mtr_engine_stcorr_read(self._h, first, count, corr.ctypes.data, st.ctypes.data), "stcorr_read")
        return corr, st

    def stcorr_series(self, first=0, count=None):
        """(points [count, kept], n_points, dropped): the readings after every completed period since reset that the series holds."""
        (out,), n, d = self._series("stcorr_series", first, count, [()], lambda count, ptrs, *tail: lib.mtr_engine_stcorr_series(self._h, first, count, *ptrs, *tail))
        return out, n, d

    def _series(self, what, first, count, shapes, call):
        """The two calls of a reading series' getter: ask for the counts, allocate one [count, kept] + shape array per entry of `shapes`,
        fetch.  call (count, pointers, capacity, n_points, dropped) -> rc.  Returns ([arrays], n_points, dropped)."""
        count = self.n_streams - first if count is None else count
        n, d = C.c_uint32(), C.c_uint32()
        _check(call(count, [None] * len(shapes), 0, C.byref(n), C.byref(d)), what)
        kept = n.value - d.value
        cap = max(kept, 1)
        outs = [np.zeros((count, cap) + tuple(s), np.float32) for s in shapes]
        _check(call(count, [o.ctypes.data for o in outs], cap, C.byref(n), C.byref(d)), what)
        return [o[:, :kept] for o in outs], n.value, d.value

    def stcorr_reset(self):
        _check(lib.mtr_engine_stcorr_reset(self._h), "stcorr_reset")

    def needle_configure(self, kinds, period_frames=0, capacity_points=0):
        """kinds: NEEDLE_* bits.  period 0: every call is one process () per (stream, channel, kind); P >= 16: blocks of exactly P frames
        wherever the calls cut the audio, read () after each appended to a series of `capacity_points` per stream and kind.  Only
        before the first process call since create / reset."""
        _check(lib.mtr_engine_needle_configure(self._h, int(kinds), int(period_frames), int(capacity_points)), "needle_configure")

    def needle_set_gain(self, side, db):
        """Msppmdsp::set_gain of the M (side 0) or S (side 1) detectors; applies from the next process call."""
        _check(lib.mtr_engine_needle_set_gain(self._h, int(side), float(db)), "needle_set_gain")

    def needle_read(self, kind, first=0, count=None):
        """(level [count, C], state [count, C, 2] = z1 z2 as stored): read () now (period 0; arms a new maximum) or of the last
        completed period."""
        count = self.n_streams - first if count is None else count
        level = np.zeros((count, self.n_channels), np.float32)
        st = np.zeros((count, self.n_channels, 2), np.float32)
        _check(lib.mtr_engine_needle_read(self._h, int(kind), first, count, level.ctypes.data, st.ctypes.data), "needle_read")
        return level, st

    def needle_series(self, kind, first=0, count=None):
        """(points [count, kept, C], n_points, dropped): the readings of `kind` after every completed period since reset that the series holds."""
        (out,), n, d = self._series("needle_series", first, count, [(self.n_channels,)],
                                    lambda count, ptrs, *tail: lib.mtr_engine_needle_series(self._h, int(kind), first, count, *ptrs, *tail))
        return out, n, d

    def needle_reset(self):
        _check(lib.mtr_engine_needle_reset(self._h), "needle_reset")

    def surround_set_pairs(self, a, b):
        """The four correlation pairs' channels (the plugin's cor?A / cor?B ports): entries >= n_channels are clamped; from the next
        process call on.  With a period only where no block is open."""
        a, b = np.ascontiguousarray(a, np.uint8), np.ascontiguousarray(b, np.uint8)
        if a.shape != (4,) or b.shape != (4,):
            raise ValueError(f"pairs: four channels each, not {a.shape} / {b.shape}")
        _check(lib.mtr_engine_surround_set_pairs(self._h, a.ctypes.data, b.ctypes.data), "surround_set_pairs")

    def surround_pairs(self):
        """(a, b): two tuples of four channels, as clamped."""
        a, b = np.zeros(4, np.uint8), np.zeros(4, np.uint8)
        _check(lib.mtr_engine_surround_pairs(self._h, a.ctypes.data, b.ctypes.data), "surround_pairs")
        return tuple(int(v) for v in a), tuple(int(v) for v in b)

    def surround_set_period(self, period_frames, capacity_points=0):
        """0: every call is one sur_run; P > 0: blocks of exactly P frames wherever the calls cut the audio, every port read after each and
        appended to a series of `capacity_points` per stream.  Only before the first process call since create / reset."""
        _check(lib.mtr_engine_surround_set_period(self._h, int(period_frames), int(capacity_points)), "surround_set_period")

    def surround_read(self, first=0, count=None):
        """(level [count, C], peak [count, C], corr [count, 4]): the ports after the most recent call (period 0; arms a new rms
        maximum) or the last completed block."""
        count = self.n_streams - first if count is None else count
        level = np.zeros((count, self.n_channels), np.float32)
        peak = np.zeros((count, self.n_channels), np.float32)
        corr = np.zeros((count, 4), np.float32)
        _check(lib.mtr_engine_surround_read(self._h, first, count, level.ctypes.data, peak.ctypes.data, corr.ctypes.data), "surround_read")
        return level, peak, corr

    def surround_pair_states(self, first=0, count=None):
        """[count, 4, 5]: zl zr zlr zll zrr of every pair as they stand."""
        count = self.n_streams - first if count is None else count
        st = np.zeros((count, 4, 5), np.float32)
        _check(lib.mtr_engine_surround_pair_states(self._h, first, count, st.ctypes.data), "surround_pair_states")
        return st

    def surround_series(self, first=0, count=None):
        """(level [count, kept, C], peak [count, kept, C], corr [count, kept, 4], n_points, dropped): the ports after every completed
        block since reset that the series holds."""
        (level, peak, corr), n, d = self._series("surround_series", first, count, [(self.n_channels,), (self.n_channels,), (4,)],
                                                 lambda count, ptrs, *tail: lib.mtr_engine_surround_series(self._h, first, count, *ptrs, *tail))
        return level, peak, corr, n, d

    def surround_reset(self):
        _check(lib.mtr_engine_surround_reset(self._h), "surround_reset")

    def scope_configure(self, window_frames=1024, hop_frames=0, phase_thresh_power=1e-6):
        """window: a power of two, 256 .. 16384; hop 0: ceil (sample_rate / 25), else 64 .. 2^20; the phase wheel's threshold on the
        powers.  Only before the first process call since create / reset."""
        _check(lib.mtr_engine_scope_configure(self._h, int(window_frames), int(hop_frames), float(phase_thresh_power)), "scope_configure")

    def scope_config(self):
        """(window_frames, hop_frames, phase_thresh_power) as configured, the hop resolved."""
        w, h, t = C.c_uint32(), C.c_uint32(), C.c_float()
        _check(lib.mtr_engine_scope_config(self._h, C.byref(w), C.byref(h), C.byref(t)), "scope_config")
        return w.value, h.value, t.value

    def scope_read(self, first=0, count=None):
        """dict of float32 arrays after the most recent analysis: level, lr (the stereoscope's), phase, plevel (the phase wheel's),
        power_l, power_r (the last |X|^2), each [count, W / 2], and peak [count]."""
        count = self.n_streams - first if count is None else count
        B = self.scope_config()[0] // 2
        names = ("level", "lr", "phase", "plevel", "peak", "power_l", "power_r")
        out = {n: np.zeros(count if n == "peak" else (count, B), np.float32) for n in names}
        _check(lib.mtr_engine_scope_read(self._h, first, count, *[out[n].ctypes.data for n in names]), "scope_read")
        return out

    def scope_analyses(self):
        """analyses completed since reset (the streams advance in lock step)."""
        n = C.c_uint64()
        _check(lib.mtr_engine_scope_analyses(self._h, C.byref(n)), "scope_analyses")
        return n.value

    def scope_reset(self):
        _check(lib.mtr_engine_scope_reset(self._h), "scope_reset")

    def _need_scope_series(self):
        if not hasattr(lib, "mtr_engine_scope_series"):
            raise EngineError(f"{lib_path} has no SCOPE reading series: rebuild it")

    def scope_set_series(self, every_analyses, capacity_points=0, fields=SCOPE_F_ALL):
        """0: off.  K = 1 .. 2^20: after every K-th analysis since reset, wherever the calls cut the audio, what scope_read would answer
        at that moment — the fields of `fields`, SCOPE_F_* bits — is appended to a series of `capacity_points` per stream.  Only before
        the first process call since create / reset."""
        self._need_scope_series()
        _check(lib.mtr_engine_scope_set_series(self._h, int(every_analyses), int(capacity_points), int(fields)), "scope_set_series")

    def scope_series_config(self):
        """(every_analyses, capacity_points, fields) as scope_set_series set them; every_analyses 0: the series is off."""
        self._need_scope_series()
        k, c, f = C.c_uint32(), C.c_uint32(), C.c_uint32()
        _check(lib.mtr_engine_scope_series_config(self._h, C.byref(k), C.byref(c), C.byref(f)), "scope_series_config")
        return k.value, c.value, f.value

    def scope_series(self, first=0, count=None):
        """(dict of the selected fields: [count, kept, W / 2] float32 arrays and peak [count, kept], n_points, dropped): the points since
        reset that the series holds."""
        self._need_scope_series()
        fields = self.scope_series_config()[2]
        B = self.scope_config()[0] // 2
        sel = [k for k in range(7) if fields >> k & 1]

        def call(count, ptrs, *tail):
            slots = [None] * 7
            for k, p in zip(sel, ptrs):
                slots[k] = p
            return lib.mtr_engine_scope_series(self._h, first, count, *slots, *tail)
        a, n, d = self._series("scope_series", first, count, [() if SCOPE_FIELDS[k] == "peak" else (B,) for k in sel], call)
        return {SCOPE_FIELDS[k]: v for k, v in zip(sel, a)}, n, d

    def _need_loudlog(self):
        if not hasattr(lib, "mtr_engine_loudlog_series"):
            raise EngineError(f"{lib_path} has no loudness log: rebuild it")

    def loudlog_set_period(self, period_fragments, capacity_points, mode=LOUDLOG_SAMPLE):
        """The loudness log of an EBU engine: a (M, S) point per stream every `period_fragments` 50 ms fragments, wherever the calls cut
        the audio, `capacity_points` of them kept per stream; 0 turns it off.  Only before the first process call since create / reset."""
        self._need_loudlog()
        _check(lib.mtr_engine_loudlog_set_period(self._h, int(period_fragments), int(capacity_points), int(mode)), "loudlog_set_period")

    def loudlog_period(self):
        """(period_fragments, capacity_points, mode) as set; period 0: the log is off."""
        self._need_loudlog()
        p, c, m = C.c_uint32(), C.c_uint32(), C.c_int()
        _check(lib.mtr_engine_loudlog_period(self._h, C.byref(p), C.byref(c), C.byref(m)), "loudlog_period")
        return p.value, c.value, m.value

    def loudlog_series(self, first=0, count=None):
        """(M [count, cap] float32, S, n_points [count] uint32, dropped): the points each stream holds, rows filled with NaN past the
        stream's own min(n_points, cap)."""
        self._need_loudlog()
        count = self.n_streams - first if count is None else count
        cap = self.loudlog_period()[1]
        M = np.full((count, cap), np.nan, np.float32)
        S = np.full((count, cap), np.nan, np.float32)
        n, d = np.zeros(count, np.uint32), np.zeros(count, np.uint32)
        _check(lib.mtr_engine_loudlog_series(self._h, first, count, M.ctypes.data, S.ctypes.data, cap, n.ctypes.data, d.ctypes.data), "loudlog_series")
        return M, S, n, d

    def loudlog_reset(self):
        self._need_loudlog()
        _check(lib.mtr_engine_loudlog_reset(self._h), "loudlog_reset")

    def _need_integlog(self):
        if not hasattr(lib, "mtr_engine_integlog_series"):
            raise EngineError(f"{lib_path} has no integration log: rebuild it")

    def integlog_set_every(self, every_evaluations, capacity_points):
        """The integration log of an EBU engine: the five values (integrated, integ_thr, range_min, range_max, range_thr) per stream after
        every `every_evaluations`-th evaluation — an evaluation falls every ten integrating fragments, 0.5 s —, `capacity_points` of them
        kept per stream; 0 turns it off.  Only before the first process call since create / reset."""
        self._need_integlog()
        _check(lib.mtr_engine_integlog_set_every(self._h, int(every_evaluations), int(capacity_points)), "integlog_set_every")

    def integlog_every(self):
        """(every_evaluations, capacity_points) as set; every 0: the log is off."""
        self._need_integlog()
        k, c = C.c_uint32(), C.c_uint32()
        _check(lib.mtr_engine_integlog_every(self._h, C.byref(k), C.byref(c)), "integlog_every")
        return k.value, c.value

    def integlog_series(self, first=0, count=None):
        """dict(I, I_thr, Rmin, Rmax, R_thr: [count, cap] float32, rows filled with NaN past the stream's own min(n_points, cap);
        n_points, dropped: [count] uint32)."""
        self._need_integlog()
        count = self.n_streams - first if count is None else count
        cap = self.integlog_every()[1]
        out = {k: np.full((count, cap), np.nan, np.float32) for k in INTEGLOG_FIELDS}
        n, d = np.zeros(count, np.uint32), np.zeros(count, np.uint32)
        _check(lib.mtr_engine_integlog_series(self._h, first, count, *[out[k].ctypes.data for k in INTEGLOG_FIELDS], cap, n.ctypes.data, d.ctypes.data),
               "integlog_series")
        out["n_points"], out["dropped"] = n, d
        return out

    def integlog_reset(self):
        self._need_integlog()
        _check(lib.mtr_engine_integlog_reset(self._h), "integlog_reset")

    def dr14_reset(self):
        _check(lib.mtr_engine_dr14_reset(self._h), "dr14_reset")

    def sigdist(self, first=0, count=None):
        count = self.n_streams - first if count is None else count
        bins = np.zeros((count, DIST_BIN), np.int32)
        peak = np.zeros((count, 2), np.int32)
        mom = np.zeros((count, 3), np.float64)
        n = np.zeros(count, np.int64)
        _check(lib.mtr_engine_sigdist(self._h, first, count, bins.ctypes.data, peak.ctypes.data, mom.ctypes.data,
                                      n.ctypes.data), "sigdist")
        return dict(bins=bins, peak_cnt=peak[:, 0], peak_bin=peak[:, 1], avg=mom[:, 0], var_m=mom[:, 1],
                    var_s=mom[:, 2], count=n)

    def intstat_reset(self):
        _check(lib.mtr_engine_intstat_reset(self._h), "intstat_reset")

    def state_bytes(self, count):
        return int(lib.mtr_engine_state_bytes(self._h, count))

    # ---- the goniometer (METER_GONIO, include/mtr_gonio.h) ----
    def gonio_configure(self, config=None, **kw):
        """config: a GonioConfig, or the keywords of gonio_config ().  Only before the first process call; resets the meter."""
        _need_gonio()
        c = config if config is not None else gonio_config(**kw)
        _check(lib.mtr_engine_gonio_configure(self._h, C.byref(c)), "gonio_configure")

    def gonio_config(self):
        """(GonioConfig with every zero resolved, GonioDerived)"""
        _need_gonio()
        c, d = GonioConfig(), GonioDerived()
        _check(lib.mtr_engine_gonio_config(self._h, C.byref(c), C.byref(d)), "gonio_config")
        return c, d

    def gonio_set_gain(self, gain):
        _need_gonio()
        _check(lib.mtr_engine_gonio_set_gain(self._h, float(gain)), "gonio_set_gain")

    def gonio_image(self, first=0, count=None):
        """(img uint32 [count, G, G], drawn, clipped, skipped uint64 [count])"""
        count = self.n_streams - first if count is None else count
        G = self.gonio_config()[1].G
        img = np.zeros((count, G, G), np.uint32)
        cnt = [np.zeros(count, np.uint64) for _ in range(3)]
        _check(lib.mtr_engine_gonio_image(self._h, first, count, img.ctypes.data, *[c.ctypes.data for c in cnt]), "gonio_image")
        return (img, *cnt)

    def gonio_read(self, first=0, count=None):
        """(gain [count], lp [count, 2], last [count, 2] = last_x, last_y), float32"""
        _need_gonio()
        count = self.n_streams - first if count is None else count
        g, lp, last = np.zeros(count, np.float32), np.zeros((count, 2), np.float32), np.zeros((count, 2), np.float32)
        _check(lib.mtr_engine_gonio_read(self._h, first, count, g.ctypes.data, lp.ctypes.data, last.ctypes.data), "gonio_read")
        return g, lp, last

    def gonio_blocks(self):
        """(display updates completed since reset, those of them the series holds)"""
        _need_gonio()
        b, h = C.c_uint64(), C.c_uint64()
        _check(lib.mtr_engine_gonio_blocks(self._h, C.byref(b), C.byref(h)), "gonio_blocks")
        return b.value, h.value

    def gonio_series(self, first=0, count=None, start=0, n=None):
        """(gain float32, drawn uint32, clipped uint32), each [count, n]: points [start, start + n) of the series (n None: all it holds
        from `start` on)"""
        count = self.n_streams - first if count is None else count
        n = self.gonio_blocks()[1] - start if n is None else n
        g, d, c = np.zeros((count, n), np.float32), np.zeros((count, n), np.uint32), np.zeros((count, n), np.uint32)
        _check(lib.mtr_engine_gonio_series(self._h, first, count, int(start), int(n), g.ctypes.data, d.ctypes.data, c.ctypes.data), "gonio_series")
        return g, d, c

    def process_device_gonio_ends(self, ptr, n_frames, frames, stride=None, stream=0):
        """process_device_any() for stereo engines that hold GONIO: stream s is metered up to frames[s] <= n_frames — the goniometer
        draws the whole display updates that end at or before its last frame and one closing update of the r frames it has of the
        open one if r >= 64 (draw_rb's floor); frames[s] < n_frames closes it."""
        self._device_frames("gonio_ends", ptr, n_frames, frames, stride, stream)

    def process_gonio_ends(self, x, frames):
        """process() with track lengths for the goniometer: x host float32 [S, T, W] as process() takes it, frames [S] <= T."""
        self._host_frames("gonio_ends", x, frames)

    def gonio_points(self, first=0, count=None):
        """(updates, points), [count] uint64 each: each stream's own display updates since reset, closing ones included, and the points
        its series has got, dropped ones included."""
        _need_gonio_ends()
        count = self.n_streams - first if count is None else count
        up, pt = np.zeros(count, np.uint64), np.zeros(count, np.uint64)
        _check(lib.mtr_engine_gonio_points(self._h, first, count, up.ctypes.data, pt.ctypes.data), "gonio_points")
        return up, pt

    def gonio_set_oversample(self, factor):
        """factor 1 (off) or 2 .. 32: the reference's "Oversampling" preference.  Only before the first process call; resets the meter."""
        _need_gonio_os()
        _check(lib.mtr_engine_gonio_set_oversample(self._h, int(factor)), "gonio_set_oversample")

    def gonio_oversample(self):
        """(factor, hpw float32): what is set, and the hpw the chain runs on"""
        _need_gonio_os()
        f, h = C.c_uint32(), C.c_float()
        _check(lib.mtr_engine_gonio_oversample(self._h, C.byref(f), C.byref(h)), "gonio_oversample")
        return f.value, np.float32(h.value)

    def gonio_os_timing(self):
        """(k_gonio_os ms, pieces) summed since the last query of this getter, while gonio_timing is on"""
        _need_gonio_os()
        t, n = C.c_float(), C.c_uint32()
        _check(lib.mtr_engine_gonio_os_timing(self._h, C.byref(t), C.byref(n)), "gonio_os_timing")
        return t.value, n.value

    def gonio_image_clear(self):
        _need_gonio()
        _check(lib.mtr_engine_gonio_image_clear(self._h), "gonio_image_clear")

    def gonio_reset(self):
        _need_gonio()
        _check(lib.mtr_engine_gonio_reset(self._h), "gonio_reset")

    def gonio_timing(self, enable):
        """(k_gonio_points ms, k_gonio_image ms, pieces) summed since the last query; enable: go on timing or stop"""
        _need_gonio()
        p, i, n = C.c_float(), C.c_float(), C.c_uint32()
        _check(lib.mtr_engine_gonio_timing(self._h, int(bool(enable)), C.byref(p), C.byref(i), C.byref(n)), "gonio_timing")
        return p.value, i.value, n.value

    def state_export(self, first=0, count=None):
        """Everything streams [first, first + count) carry from call to call, as one opaque blob (bytes)."""
        count = self.n_streams - first if count is None else count
        buf = C.create_string_buffer(self.state_bytes(count))
        _check(lib.mtr_engine_state_export(self._h, first, count, buf, len(buf)), "state_export")
        return bytes(buf.raw)

    def state_import(self, blob, first=0):
        """Put a blob's streams into slots [first, first + its count) of this engine (same meters / channels / rate)."""
        blob = bytes(blob)
        _check(lib.mtr_engine_state_import(self._h, first, blob, len(blob)), "state_import")
        return int(lib.mtr_state_blob_count(blob, len(blob)))

    def aggregate_device(self, hist_ptr, max_ptr, stream=0):
        _check(lib.mtr_engine_aggregate_device(self._h, hist_ptr, max_ptr, stream), "aggregate_device")

    def layout(self):
        return lib.mtr_engine_layout(self._h)

    def seg_stats(self):
        """layout 7: (calls whose whole fragments ran k_seg, frames per stream it covered)"""
        a, b = C.c_uint64(), C.c_uint64()
        _check(lib.mtr_engine_seg_stats(self._h, C.byref(a), C.byref(b)), "seg_stats")
        return a.value, b.value

    def reduce(self, comm, hist_ptr, max_ptr, stream=0):
        """aggregate_device + the RCCL all-reduce across the ranks of `comm` (a Comm), in place, on `stream`."""
        _check(lib.mtr_engine_reduce(self._h, comm._h, hist_ptr, max_ptr, stream), "reduce")

    def prune_stats(self):
        a, b = C.c_uint64(), C.c_uint64()
        _check(lib.mtr_engine_prune_stats(self._h, C.byref(a), C.byref(b)), "prune_stats")
        return a.value, b.value

    def refine_stats(self):
        """(products screened with the first f16 product, completed with the other two): k_kwtp16's channel-blocks with
        tune_prune = 2, k_seg's 16-column chunks (layout 7, unless MTR_SEG_SCREEN=0; MTR_SEG_SCREEN=1 is the screen whose stream
        reference takes completed interpolated peaks only at a flush, 2 the one that takes them as they
        are found: the same chunks screened, fewer completed, the same peaks; 3 is rule 2 with the lo halves
        of the f16 split built only where a chunk completes: the counts of 2; 4 — the default — is form 3 with each chunk screened by
        the taps' 32-sample core, three MFMAs in place of six: the same chunks screened, more completed, the same peaks)"""
        a, b = C.c_uint64(), C.c_uint64()
        _check(lib.mtr_engine_refine_stats(self._h, C.byref(a), C.byref(b)), "refine_stats")
        return a.value, b.value

    def timing_enable(self, on=True):
        _check(lib.mtr_engine_timing_enable(self._h, int(on)), "timing_enable")

    def timing_calls(self, cap=4096):
        """[calls, 4] float32 ms per timed call since the last query: fused, gate, behind the gate, whole call."""
        n = C.c_uint32()
        out = np.zeros((cap, 4), np.float32)
        _check(lib.mtr_engine_timing_calls(self._h, out.ctypes.data, cap, C.byref(n)), "timing_calls")
        return out[:min(n.value, cap)]

    def timing_query(self):
        f, g, b, n = C.c_float(), C.c_float(), C.c_float(), C.c_uint32()
        _check(lib.mtr_engine_timing_query(self._h, C.byref(f), C.byref(g), C.byref(b), C.byref(n)), "timing_query")
        return dict(ms_fused=f.value, ms_gate=g.value, ms_bank=b.value, calls=n.value)
