/* mtr_surround.h — the surround meter part of the engine's C ABI (MTR_METER_SURROUND).  Included by mtr_engine.h; additions inside
 * MTR_ABI_VERSION 2, looked up by name. */
#ifndef MTR_SURROUND_H
#define MTR_SURROUND_H

#ifndef MTR_ENGINE_H
#error "include mtr_engine.h: it defines mtr_engine and includes this header"
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* sur_run (src/surmeter.c:115-147, the surround3 .. surround8 plugins) for a batch: engines of C = 3 .. 8 channels.  Per stream C x
 * Kmeterdsp::process + read (m, p) (jmeters/kmeterdsp.cc:56-153) and n_pairs = C > 3 ? 4 : 3 x Stcorrdsp::process + read ()
 * (jmeters/stcorrdsp.cc:47-93, init (rate, 2e3f, 0.3f)), pair p on the channels (a [p], b [p]).  One kernel reads the frames once for
 * all of them.  3 .. 5 channels combine it with MTR_METER_EBU / MTR_METER_TRUEPEAK; 6 .. 8 channels take it alone (anything else:
 * MTR_ERR_ARG, as every engine of more than 5 channels without it); 1 or 2 channels: MTR_ERR_UNSUPPORTED.  Of the
 * per-stream-lengths and track-lengths entry points mtr_engine_process_device_any / _host_any take it (mtr_any.h); the
 * five older pairs refuse it.  n_frames per call < 2^31 - 1.
 *
 * The pairs: a control, like the plugin's cor?A / cor?B ports.  a4, b4: four entries each; an entry >= C is clamped to C - 1
 * (surmeter.c:124-125), a == b is legal.  After create: pair p = (2 p, 2 p + 1), clamped (the surround8 port defaults).  Applies from
 * the next process call, survives mtr_engine_reset, travels in the state blob.  The five states of a pair belong to the PAIR: after a
 * change zl / zr go on from what the old channels left, as the plugin's four Stcorrdsp objects do.  With a period P > 0 only where no
 * period is open (else MTR_ERR_STATE): no host changes a port inside a run (). */
int  mtr_engine_surround_set_pairs (mtr_engine* e, const uint8_t* a4, const uint8_t* b4);
/* the pairs as they stand (clamped); either may be NULL */
int  mtr_engine_surround_pairs (const mtr_engine* e, uint8_t* a4, uint8_t* b4);
/* period_frames 0 (default): every engine call is ONE sur_run per stream — level is Kmeterdsp's rms, max-held until read, peak carries
 * the hold / fall-back of kmeterdsp.cc:121-138 with fpp = the call's length (what MTR_METER_KMETER does).
 * period_frames P > 0: the streams are processed as by a host that runs the plugin on consecutive blocks of exactly P frames and reads
 * every port after each block, wherever the process calls cut the audio (a lock-step cursor): level = sqrtf (2 z2) of that block, fpp = P,
 * the P mod 4 trailing frames of every block are dropped by the K-meters (kmeterdsp.cc:71) but not by the correlation meters, Stcorrdsp's
 * flushes and + 1e-10f happen at every block's end; every block appends one point to a per-stream series of `capacity_points` points
 * (engine-owned device memory; points past the capacity are dropped and counted).  P must be 0 or >= (uint32_t) sample_rate / 20, else
 * MTR_ERR_ARG.  Only on an engine that has processed nothing since create / reset (else MTR_ERR_STATE).  Resets the meter.
 * (One departure, as MTR_METER_STCORR's: a finite sample beyond 1e19 overflows the reference's f32 sums inside a block and need not
 * flush the block here.) */
int  mtr_engine_surround_set_period (mtr_engine* e, uint32_t period_frames, uint32_t capacity_points);
/* level [count][C], peak [count][C], corr [count][4] (any may be NULL; corr [3] stays 0.0f on a 3-channel engine).  P = 0: the
 * readings now, and the rms maximum is armed as mtr_engine_kmeter_read does; P > 0: those of the last completed block (0.0f before the
 * first), nothing is armed.  Synchronises. */
int  mtr_engine_surround_read (mtr_engine* e, uint32_t first, uint32_t count, float* level, float* peak, float* corr);
/* zl zr zlr zll zrr of every pair as they stand now: state5 [count][4][5] (what mtr_engine_stcorr_read's state5 is for the stereo
 * meter).  No plugin port carries them: the entry point exists for verification — the tests hold the states to the oracle's.
 * Synchronises. */
int  mtr_engine_surround_pair_states (mtr_engine* e, uint32_t first, uint32_t count, float* state5);
/* level [count][capacity][C], peak [count][capacity][C], corr [count][capacity][4] (any may be NULL): the first min (*n_points,
 * capacity, capacity_points) points of each stream; *n_points = blocks completed since reset, *dropped = points that did not fit the
 * series (the streams advance in lock step: one number each). */
int  mtr_engine_surround_series (mtr_engine* e, uint32_t first, uint32_t count, float* level, float* peak, float* corr,
                                 uint32_t capacity, uint32_t* n_points, uint32_t* dropped);
/* The constructors' state (kmeterdsp.cc:33-40, stcorrdsp.cc:33-36); series emptied, period and pairs kept.  Part of mtr_engine_reset. */
int  mtr_engine_surround_reset (mtr_engine* e);

#ifdef __cplusplus
}
#endif

#endif
