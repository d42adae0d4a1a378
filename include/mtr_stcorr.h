/* mtr_stcorr.h — the stereo phase correlation part of the engine's C ABI (MTR_METER_STCORR).  Included by mtr_engine.h; additions
 * inside MTR_ABI_VERSION 2, looked up by name. */
#ifndef MTR_STCORR_H
#define MTR_STCORR_H

#ifndef MTR_ENGINE_H
#error "include mtr_engine.h: it defines mtr_engine and includes this header"
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* Stcorrdsp for a batch (MTR_METER_STCORR; stereo engines only — a pair of a wider frame: mtr_engine_set_frame_layout, e.g. 6, {4, 5}
 * for Ls / Rs of a 5.1 file; all four selectable pairs of the surround plugins, src/surmeter.c, with their K-meters from one read of
 * the wide frames: MTR_METER_SURROUND, mtr_surround.h).  Combines with every other stereo meter.  A batch of tracks that end where
 * their audio ends: mtr_engine_process_device_ragged / _host_ragged (mtr_ragged.h; the _lengths and _tracks pairs refuse the meter).
 * n_frames per call < 2^31 - 1.
 * w1, w2 of Stcorrdsp::init ((int) sample_rate, 2e3f, 0.3f) (stcorrdsp.cc:85-93; src/meters.cc:202-207) */
int  mtr_stcorr_coef (float sample_rate, float* out2);
/* period_frames 0 (default): every engine call is ONE Stcorrdsp::process () per stream (as MTR_METER_KMETER).
 * period_frames P > 0: the streams are processed as by a host that calls process () on consecutive blocks of exactly P
 * frames, wherever the process calls cut the audio (a lock-step cursor like DR-14's window), and read () after each
 * block is appended to a per-stream series of `capacity_points` floats (engine-owned device memory; points past the
 * capacity are dropped and counted).  P must be 0 or >= (uint32_t) sample_rate / 20, else MTR_ERR_ARG.
 * Only on an engine that has processed nothing since create / reset (else MTR_ERR_STATE).  Resets the meter.
 * Samples that are not finite: the flushes of stcorrdsp.cc:65-69 happen at every block's end, as there.  (One departure: a finite
 * sample beyond 1e19, which overflows the reference's f32 sums inside a block, need not flush the block here.) */
int  mtr_engine_stcorr_set_period (mtr_engine* e, uint32_t period_frames, uint32_t capacity_points);
/* corr [count]: Stcorrdsp::read () (:79-82) — after the most recent call (P = 0) or after the last completed period
 * (P > 0; 0.0f before the first).  state5 [count][5] = zl zr zlr zll zrr as they stand now, may be NULL.  Synchronises. */
int  mtr_engine_stcorr_read (mtr_engine* e, uint32_t first, uint32_t count, float* corr, float* state5);
/* out [count][capacity] (may be NULL): the first min (*n_points, capacity, capacity_points) readings of each stream; *n_points =
 * periods completed since reset, *dropped = points that did not fit the series (the streams advance in lock step: one number each;
 * a stream that a ragged call closed has its own count, mtr_engine_series_points, and 0.0f behind its own points). */
int  mtr_engine_stcorr_series (mtr_engine* e, uint32_t first, uint32_t count, float* out, uint32_t capacity,
                               uint32_t* n_points, uint32_t* dropped);
/* Stcorrdsp's constructor state (:33-36); series emptied, period kept.  Part of mtr_engine_reset. */
int  mtr_engine_stcorr_reset (mtr_engine* e);

#ifdef __cplusplus
}
#endif

#endif
