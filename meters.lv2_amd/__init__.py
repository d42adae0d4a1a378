"""meters.lv2_amd — MI355X-native batch engine for the meters.lv2 DSP hot path.

The product is the C-ABI shared library ``lib/libmtr_engine.so`` (HIP kernels for gfx950 + host
code, built from ``csrc/`` by ``__graft_entry__.build()``) and the LV2 plugin ``lib/meters_amd.so``
on top of it.  This Python package is only the thin ctypes binding the tests and bench.py drive
the library through; there is no Python or CPU compute path here, and importing it fails loudly
when the library has not been built.
"""
from .engine import (  # noqa: F401
    Engine, EngineError, StreamResult, lib, lib_path, Comm, comm_unique_id,
    METER_EBU, METER_TRUEPEAK, METER_SPECTR30, METER_TPBALLIST, METER_BITSTATS, METER_SIGDIST, METER_DR14, METER_KMETER, METER_STCORR,
    METER_SURROUND, METER_SCOPE, scope_window, METER_NEEDLE, NEEDLE_VU, NEEDLE_IEC1, NEEDLE_IEC2, NEEDLE_MS, needle_coef,
    fir_table, kweight_coef, band_coef, hist_loudness, stcorr_coef, synth_fill_device, exported_symbols, plan_query, series_cut,
    PCM_S16, PCM_S24, PCM_S32, pcm_decode, pick_decode, LOUDLOG_SAMPLE, LOUDLOG_MAX, SPECTR_PEAK_HOLD, SPECTR_PEAK_BLOCK,
    scope_series_cut, SCOPE_F_LEVEL, SCOPE_F_LR, SCOPE_F_PHASE, SCOPE_F_PLEVEL, SCOPE_F_PEAK, SCOPE_F_POWER_L, SCOPE_F_POWER_R, SCOPE_F_ALL,
    METER_GONIO, GonioConfig, GonioDerived, gonio_config, gonio_derive, gonio_cut, gonio_os_table, gonio_os_hpw,
    plane_decode, tensor_source, TensorSource, integlog_cut, INTEGLOG_FIELDS,
)
