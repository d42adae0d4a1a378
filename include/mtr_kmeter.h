/* mtr_kmeter.h — the K-meter's reading series, part of the engine's C ABI (MTR_METER_KMETER).  Included by mtr_engine.h, which
 * declares mtr_engine_kmeter_read / _reset itself; additions inside MTR_ABI_VERSION 2, looked up by name. */
#ifndef MTR_KMETER_H
#define MTR_KMETER_H

#ifndef MTR_ENGINE_H
#error "include mtr_engine.h: it defines mtr_engine and includes this header"
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* period_frames 0 (default): every engine call is ONE Kmeterdsp::process () per (stream, channel), read when the caller asks
 * (mtr_engine_kmeter_read).
 * period_frames P > 0: the streams are metered as by a host that calls Kmeterdsp::process (p, P) and then read (rms, peak) on
 * consecutive blocks of exactly P frames, wherever the process calls cut the audio (jmeters/kmeterdsp.cc:56-155, as kmeter_run does it,
 * src/meters.cc:333-412): _fpp = P with the fall-back factor of P (:65-70); the P mod 4 trailing frames of every block enter neither
 * filter nor peak (:79) and the groups of four restart at each block's start; at every block's end the clamp to [0, 50] (:74-75), the
 * NaN rules (:101-103) and + 1e-20f (:106-107); rms = sqrtf (2 z2) of the block (:109; a read follows every block, so nothing is
 * max-held, :112-121); the hold / fall-back bookkeeping with cnt -= P (:124-139).  Every (rms, peak) is appended to two per-stream
 * series of `capacity_points` points of n_channels floats (engine-owned device memory; points past the capacity are dropped and
 * counted).  P must be 0 or >= (uint32_t) sample_rate / 20, else MTR_ERR_ARG.  Only on an engine that has processed nothing since
 * create / reset (else MTR_ERR_STATE).  Resets the meter.
 * With P > 0 mtr_engine_kmeter_read returns the last completed block's (rms, peak) — 0.0f before the first — and arms nothing;
 * mtr_engine_kmeter_reset empties the series and the open block and keeps P; mtr_engine_process_*_ragged closes a stream that ends r
 * frames into a block, 0 < r < P, with one last process (p, r) + read, its last point (mtr_ragged.h), and mtr_engine_process_*_tracks
 * refuses the engine (MTR_ERR_UNSUPPORTED).  A state blob of such an engine carries the open block: it goes into an engine of the same
 * period only. */
int  mtr_engine_kmeter_set_period (mtr_engine* e, uint32_t period_frames, uint32_t capacity_points);
/* what set_period set; either pointer may be NULL */
int  mtr_engine_kmeter_period (const mtr_engine* e, uint32_t* period_frames, uint32_t* capacity_points);
/* rms, peak [count][capacity][n_channels] (either may be NULL): the first min (*n_points, capacity, capacity_points) readings of each
 * stream; *n_points = blocks completed since reset, *dropped = points that did not fit the series (the streams advance in lock step:
 * one number each; a stream that a ragged call closed has its own count, mtr_engine_series_points, and 0.0f behind its own points). */
int  mtr_engine_kmeter_series (mtr_engine* e, uint32_t first, uint32_t count, float* rms, float* peak, uint32_t capacity,
                               uint32_t* n_points, uint32_t* dropped);

#ifdef __cplusplus
}
#endif

#endif
