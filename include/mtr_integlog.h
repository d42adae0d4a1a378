/* mtr_integlog.h — the integration log of the engine's C ABI: integrated loudness and loudness range over time for every stream of an
 * MTR_METER_EBU engine (the I (t) and LRA (t) curves of a loudness report; what the reference's GUI shows moving while it integrates).
 * Included by mtr_engine.h; additions inside MTR_ABI_VERSION 2, looked up by name.  A setting of the engine, not a meter bit. */
#ifndef MTR_INTEGLOG_H
#define MTR_INTEGLOG_H

#ifndef MTR_ENGINE_H
#error "include mtr_engine.h: it defines mtr_engine and includes this header"
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* An EVALUATION is a 50 ms fragment at which the stream's _div2 wraps while the integration runs: there Ebu_r128_proc::process
 * re-evaluates _integrated / _integ_thr (calc_integ) and _range_min / _range_max / _range_thr (calc_range), every tenth integrating
 * fragment, 0.5 s of audio (ebumeter/ebu_r128_proc.cc:236-242).  Without the log the gate makes only the last evaluation of a call —
 * the one a getter can see.  Evaluations are counted per stream, in device memory, from the moment the log is set or from
 * mtr_engine_reset.  mtr_engine_integr_reset does not restart the count: it zeroes _div2 and the histograms (:192-204), and the points
 * that follow show -200 until the 50 / 20 point minima of calc_integ / calc_range are passed again.  A paused integration makes no
 * evaluations and so adds no points.
 *
 * A POINT is the five values integrated (), integ_thr (), range_min (), range_max (), range_thr () as the reference's getters return them
 * right after an evaluation, with the early returns and the clamp of calc_integ (:110-114) and calc_range (:133-138): with fewer than 50
 * M points `integrated` is -200 and `integ_thr` keeps what it held; with fewer than 20 S points the range edges are -200 and `range_thr`
 * keeps what it held. */

/* every_evaluations K = 0 (the default): the log is off, its memory freed, every kernel launched the one launched without the log.
 * 1 <= K <= 2^20: the log is on — point j of a stream is taken right after the stream's evaluation (j + 1) K, and every stream keeps
 * `capacity_points` points in engine-owned device memory; points at or past the capacity are counted, never written.
 * Every route of a process call appends (device / host chunks / PCM / frame and plane layouts, every per-stream-lengths family, 1 .. 5
 * channels, the LV2 block path, the serial and the deferred tail).  Per-stream lengths: a stream evaluates at the wraps among the
 * fragments that end at or before its own end; a stream with frames[s] == 0 is untouched.  With the log on a call of any length goes
 * through the one-workgroup-per-stream gate (the multi-workgroup gate of long calls keeps no state in between).  The deferred tail stays
 * in use: the gate's instantiations with the log fit beside the batch kernel as those without it do.
 * K > 2^20, an engine without MTR_METER_EBU: MTR_ERR_ARG.  Only on an engine that has processed nothing since create / reset, else
 * MTR_ERR_STATE (the rule of mtr_engine_loudlog_set_period).  Memory that cannot be had: MTR_ERR_NOMEM, and the log is off.
 * The log is NOT part of the state blob: mtr_engine_state_export does not carry it, mtr_engine_state_import leaves series and counts as
 * they are (the imported _div2 decides when the next evaluation falls). */
int  mtr_engine_integlog_set_every (mtr_engine* e, uint32_t every_evaluations, uint32_t capacity_points);
/* what was set (either pointer may be NULL); K = 0: the log is off */
int  mtr_engine_integlog_every (const mtr_engine* e, uint32_t* every_evaluations, uint32_t* capacity_points);
/* integrated, integ_thr, range_min, range_max, range_thr [count][capacity] (any may be NULL): the first min (n_points [s], capacity, capacity_points) points of
 * each stream — what a host would have read from the five getters (ebu_r128_proc.h: integrated (), integ_thr (), range_min (),
 * range_max (), range_thr ()) after process () calls that end on those evaluations; the rest of a row is left as it was.
 * n_points [count] = points the stream has reached since reset (its evaluations / K), dropped [count] = those that did not fit the series
 * (either may be NULL).  Waits for the caller's stream and the engine's side stream (a deferred gate writes its points there).
 * The log is off: MTR_ERR_ARG. */
int  mtr_engine_integlog_series (mtr_engine* e, uint32_t first, uint32_t count, float* integrated, float* integ_thr, float* range_min, float* range_max, float* range_thr,
                                 uint32_t capacity, uint32_t* n_points /* [count] */, uint32_t* dropped /* [count] */);
/* Empties the series and the evaluation counts; keeps K and the capacity (MTR_OK and nothing to do while the log is off).  Part of
 * mtr_engine_reset (Ebu_r128_proc::reset, :176-189); mtr_engine_integr_reset (:192-204) does not touch the log. */
int  mtr_engine_integlog_reset (mtr_engine* e);
/* Pure host arithmetic, the rule of mtr_series_cut for this log: a stream whose _div2 stands at `div2` (0 .. 9) and which has made
 * `evaluations_so_far` evaluations gains *evaluations_out = (div2 + n_fragments) / 10 evaluations (the `if (++_div2 == 10)` of :236) and
 * *points_out points from `n_fragments` integrating fragments; K = 0: no points.  A host sizes its capacity with it.
 * A NULL result, div2 > 9, K > 2^20 or counts that do not fit 64 bits: MTR_ERR_ARG. */
int  mtr_integlog_cut (uint32_t div2, uint64_t evaluations_so_far, uint32_t every_evaluations, uint64_t n_fragments,
                       uint64_t* evaluations_out, uint64_t* points_out);

#ifdef __cplusplus
}
#endif

#endif
