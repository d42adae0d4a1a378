/* mtr_scope.h — the stereo / frequency scope part of the engine's C ABI (MTR_METER_SCOPE).  Included by mtr_engine.h; additions inside
 * MTR_ABI_VERSION 2, looked up by name. */
#ifndef MTR_SCOPE_H
#define MTR_SCOPE_H

#ifndef MTR_ENGINE_H
#error "include mtr_engine.h: it defines mtr_engine and includes this header"
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* The analysis under the reference's two FFT views of a stereo programme, for a batch (MTR_METER_SCOPE; stereo engines only — a pair of
 * a wider frame: mtr_engine_set_frame_layout, as for STCORR).  Combines with every other stereo meter.  Of the per-stream-lengths
 * and track-lengths entry points mtr_engine_process_device_any / _host_any take it (mtr_any.h); the five older pairs refuse it
 * (MTR_ERR_UNSUPPORTED, nothing queued).  n_frames per call < 2^31 - 1.
 *
 * W = window frames, B = W / 2 bins, H = hop.  After every H frames of a stream, counted across the process calls wherever they cut the
 * audio (a lock-step cursor like STCORR's period), one analysis runs on the stream's last W frames, zeros in front of its start: what
 * fftx_run fed with blocks of H frames does (gui/fft.c:289-361).  Per channel the frames are multiplied by mtr_scope_window and
 * transformed (forward DFT, FFTW's sign); power [i] = Re^2 + Im^2 and phase [i] = atan2f (Im, Re) for 1 <= i <= B - 2 (ft_analyze,
 * gui/fft.c:163-180).  Bins 0 and B - 1 are never written: they keep their initial values in every output.  Then, per bin:
 *   the stereoscope (process_audio, gui/stereoscope.c:705-741): both powers < 1e-20: lr = .5f, level = 0; else lv = max (pL, pR),
 *     lr_t = .5 + .5 (sqrtf pR - sqrtf pL) / sqrtf lv, level += .1 (lv - level) + 1e-20, lr += .1 (lr_t - lr) + 1e-10, in its C types;
 *     initially level = -100, lr = .5;
 *   the phase wheel (process_audio, gui/phasewheel.c:1307-1339): either power < phase_thresh_power: phase = 0, plevel = -100; else
 *     phase = phaseR - phaseL (not wrapped, as there), plevel = max (pL, pR); per analysis peak += .04 (max plevel - peak) + 1e-15 with
 *     its NaN guard and its clamp at 1000; initially phase = 0, plevel = -100, peak = 0.
 * Samples that are not finite: the stream's outputs are what the arithmetic gives (the reference's levels go NaN and stay there); no
 * other stream and no other meter is affected.
 *
 * The Hann window of ft_gen_window (gui/fft.c:69-79, 122-161: ft_hannhamm (.5, .5) times 2 / sum, computed in double and stored as
 * f32 as written there): out [window_frames].  window_frames as mtr_engine_scope_configure takes it, with its answers. */
int  mtr_scope_window (uint32_t window_frames, float* out);
/* window_frames: a power of two, 256 .. 16384; default 1024, the plugins' 512 bins (stereoscope.c:641, phasewheel.c:1219).  Any other
 * size in 128 .. 16384 the reference would round to itself (reinitialize_fft, stereoscope.c:123-131: 128, 12288, ...):
 * MTR_ERR_UNSUPPORTED; anything else MTR_ERR_ARG.  hop_frames: 0 = ceil (sample_rate / 25), fftx_init (.., 25) (gui/fft.c:219;
 * stereoscope.c:136) — 1920 at 48 kHz, 1764 at 44.1 kHz — else 64 .. 2^20.  phase_thresh_power >= 0, default 1e-6f
 * (phasewheel.c:1212; set_phase_thresh :836 squares an amplitude).
 * Only on an engine that has processed nothing since create / reset (else MTR_ERR_STATE).  Resets the meter. */
int  mtr_engine_scope_configure (mtr_engine* e, uint32_t window_frames, uint32_t hop_frames, float phase_thresh_power);
/* what is configured (the hop resolved: never 0); any pointer may be NULL */
int  mtr_engine_scope_config (const mtr_engine* e, uint32_t* window_frames, uint32_t* hop_frames, float* phase_thresh_power);
/* What the two process_audio leave after the most recent analysis (initial values before the first): the stereoscope's level, lr
 * [count][B]; the phase wheel's phase, plevel [count][B] and peak [count]; power_l, power_r [count][B]: the last analysis' |X|^2 per
 * channel (fa->power, fb->power; 0 before the first).  Any pointer may be NULL.  Synchronises. */
int  mtr_engine_scope_read (mtr_engine* e, uint32_t first, uint32_t count, float* level, float* lr, float* phase, float* plevel, float* peak,
                            float* power_l, float* power_r);
/* *n = analyses completed since reset (the streams advance in lock step: one number) */
int  mtr_engine_scope_analyses (mtr_engine* e, uint64_t* n);
/* reinitialize_fft's initial values (stereoscope.c:143-146, phasewheel.c:202-205) and fftx_reset (gui/fft.c:191-205); the configuration
 * is kept.  Part of mtr_engine_reset. */
int  mtr_engine_scope_reset (mtr_engine* e);

#ifdef __cplusplus
}
#endif

/* The reading series — a point per stream after every K-th analysis, what the two GUIs paint over time — has a header of its own */
#include "mtr_scope_series.h"

#endif
