/* mtr_needle.h — the needle meters' part of the engine's C ABI (MTR_METER_NEEDLE): Vumeterdsp, Iec1ppmdsp, Iec2ppmdsp and Msppmdsp
 * (jmeters/) for a batch, with a reading series.  Included by mtr_engine.h; additions inside MTR_ABI_VERSION 2, looked up by name. */
#ifndef MTR_NEEDLE_H
#define MTR_NEEDLE_H

#ifndef MTR_ENGINE_H
#error "include mtr_engine.h: it defines mtr_engine and includes this header"
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define MTR_NEEDLE_VU     1u       /* vumeterdsp.cc:45-73 */
#define MTR_NEEDLE_IEC1   2u       /* iec1ppmdsp.cc:47-80  (DIN, NOR) */
#define MTR_NEEDLE_IEC2   4u       /* iec2ppmdsp.cc:47-80  (BBC, EBU) */
#define MTR_NEEDLE_MS     8u       /* msppmdsp.cc:50-118: "channel" 0 = processM, 1 = processS; stereo engines only */

/* The needle meters for a batch (MTR_METER_NEEDLE; engines of 1 or 2 channels, C = n_channels; MTR_NEEDLE_MS needs 2).  Combines with
 * every other meter of such an engine.  A batch of tracks that end where their audio ends: mtr_engine_process_device_ragged /
 * _host_ragged (mtr_ragged.h; the _lengths and _tracks pairs refuse the meter).  n_frames per call < 2^31 - 1.  The arithmetic is
 * the reference's, operation for operation in f32: readings and states are bit for bit those of the reference's objects.
 * w1 w2 w3 g of Iec1ppmdsp::init / Iec2ppmdsp::init (= Msppmdsp::init) (iec1ppmdsp.cc:89-95, iec2ppmdsp.cc:89-95, msppmdsp.cc:131-137);
 * of Vumeterdsp::init (vumeterdsp.cc:82-86): w, 4 w, 0, g.  `kind` is ONE of the four bits, else MTR_ERR_ARG.  Host only, no device. */
int  mtr_needle_coef (uint32_t kind, float sample_rate, float* out4);
/* kinds: a non-empty subset of the four bits (else MTR_ERR_ARG; MTR_NEEDLE_MS on a mono engine: MTR_ERR_UNSUPPORTED).  An engine that
 * was never configured runs MTR_NEEDLE_IEC2 with period 0.  The results of a kind do not depend on which other kinds are selected.
 * period_frames 0: every engine call is ONE process () per (stream, channel, kind) — the clamp at its start, the + 1e-10f (PPM) or the
 * isfinite flushes (VU) at its end, the n mod 4 trailing frames of the call dropped as by `n /= 4`; the maximum is held over the calls
 * until it is read.
 * period_frames P >= 16 (1 .. 15: MTR_ERR_ARG): the streams are processed as by a host that calls process () on consecutive blocks of
 * exactly P frames and read () after each, wherever the process calls cut the audio (a lock-step cursor); the P mod 4 trailing frames
 * of every block are dropped.  Every reading is appended to a per-stream series of `capacity_points` points per selected kind
 * (engine-owned device memory; points past the capacity are dropped and counted).
 * Only on an engine that has processed nothing since create / reset (else MTR_ERR_STATE).  Resets the meter; the gains stay. */
int  mtr_engine_needle_configure (mtr_engine* e, uint32_t kinds, uint32_t period_frames, uint32_t capacity_points);
/* Msppmdsp::set_gain (msppmdsp.cc:140-148) of the M (side 0) or S (side 1) detectors: mv = powf (10, .05 * db).  -6 / -6 after create
 * (src/meters.cc:211-212).  A control: it applies from the next process call, survives mtr_engine_reset and travels in the state blob. */
int  mtr_engine_needle_set_gain (mtr_engine* e, int side, float db);
/* `kind`: one selected kind.  level [count][C]: period 0: read () = g * m now, and the maximum starts again with the next call (the
 * reference's _res); P > 0: the reading of the last completed period (0.0f before the first), nothing is armed.  state [count][C][2]
 * (may be NULL) = z1 z2 as the most recent completed process () stored them.  Synchronises. */
int  mtr_engine_needle_read (mtr_engine* e, uint32_t kind, uint32_t first, uint32_t count, float* level, float* state);
/* out [count][capacity][C] (may be NULL): the first min (*n_points, capacity, capacity_points) readings of `kind` of each stream;
 * *n_points = periods completed since reset, *dropped = points that did not fit the series (lock step: one number each; a stream that
 * a ragged call closed has its own count, mtr_engine_series_points, and 0.0f behind its own points). */
int  mtr_engine_needle_series (mtr_engine* e, uint32_t kind, uint32_t first, uint32_t count, float* out, uint32_t capacity,
                               uint32_t* n_points, uint32_t* dropped);
/* The constructors' state; series emptied; kinds, period and gains kept.  Part of mtr_engine_reset. */
int  mtr_engine_needle_reset (mtr_engine* e);

#ifdef __cplusplus
}
#endif

#endif
