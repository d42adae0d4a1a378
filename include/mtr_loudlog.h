/* mtr_loudlog.h — the loudness log of the engine's C ABI: momentary / short-term loudness over time for every stream of an
 * MTR_METER_EBU engine (the curve a loudness report draws; the reference plugin's radar ring, src/ebulv2.cc:390-420).  Included by
 * mtr_engine.h; additions inside MTR_ABI_VERSION 2, looked up by name.  A setting of the engine, not a meter bit. */
#ifndef MTR_LOUDLOG_H
#define MTR_LOUDLOG_H

#ifndef MTR_ENGINE_H
#error "include mtr_engine.h: it defines mtr_engine and includes this header"
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* A point is a pair (M, S) of the values the gate computes for a 50 ms fragment — addfrags (8) and addfrags (60) of
 * ebumeter/ebu_r128_proc.cc:251-260 with the clamp `!isfinite || < -200 -> -200` of :226-233 — whether or not the integration runs.
 * One fragment is (int) sample_rate / 20 frames (Ebu_r128_proc::init); a period is P fragments. */
#define MTR_LOUDLOG_SAMPLE 0   /* point k = (loudness_M (), loudness_S ()) as a host reads them after fragment (k + 1) P - 1 */
#define MTR_LOUDLOG_MAX    1   /* point k = (max M, max S) over fragments [k P, (k + 1) P): the radar's max-hold per step, without the
                                  reference's `if (lm > radarSC)` slip (ebulv2.cc:392) */

/* period_fragments P = 0 (the default): the log is off, its memory freed, every kernel the one it is without the log.
 * 1 <= P <= 2^20: the log is on — every stream keeps `capacity_points` points in engine-owned device memory; points past the
 * capacity are dropped and counted, never written.  Fragments are counted from this call or the last mtr_engine_reset: a lock-step
 * cursor of the open streams that advances by the fragments that END inside a process call, wherever the calls cut the audio (a call
 * that ends no fragment appends nothing).  Per-stream lengths: a stream a call closes gets the points whose period ends at or before
 * its own last whole fragment and nothing afterwards (its open period is dropped); a stream with frames[s] == 0 is untouched.
 * Every route of a process call appends (device / host / lengths / PCM / frame layouts, 2 .. 5 channels, the deferred tail).
 * P > 2^20, an unknown mode, an engine without MTR_METER_EBU: MTR_ERR_ARG.  Only on an engine that has processed nothing since create /
 * reset, else MTR_ERR_STATE (the rule of mtr_engine_stcorr_set_period).  Memory that cannot be had: MTR_ERR_NOMEM, and the log is off.
 * The log is NOT part of the state blob: mtr_engine_state_export does not carry it, mtr_engine_state_import leaves series, counts and
 * phase as they are. */
int  mtr_engine_loudlog_set_period (mtr_engine* e, uint32_t period_fragments, uint32_t capacity_points, int mode);
/* what was set (any pointer may be NULL); period 0: the log is off */
int  mtr_engine_loudlog_period (const mtr_engine* e, uint32_t* period_fragments, uint32_t* capacity_points, int* mode);
/* M, S [count][capacity] (either may be NULL): the first min (n_points [s], capacity, capacity_points) points of each stream, the rest
 * of a row is left as it was.  n_points [count] = periods the stream completed since reset, dropped [count] = those that did not fit
 * the series (either may be NULL; per stream, because streams end at their own lengths).  Waits for the caller's stream and the
 * engine's side stream (a deferred gate writes its points there).  The log is off: MTR_ERR_ARG. */
int  mtr_engine_loudlog_series (mtr_engine* e, uint32_t first, uint32_t count, float* M, float* S, uint32_t capacity,
                                uint32_t* n_points /* [count] */, uint32_t* dropped /* [count] */);
/* Empties the series, the counts, the phase and the running maxima of MTR_LOUDLOG_MAX; keeps period, capacity and mode (MTR_OK and
 * nothing to do while the log is off).  Part of mtr_engine_reset; mtr_engine_integr_reset does not touch the log. */
int  mtr_engine_loudlog_reset (mtr_engine* e);

#ifdef __cplusplus
}
#endif

#endif
