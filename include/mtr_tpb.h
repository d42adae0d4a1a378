/* mtr_tpb.h — the reading series of the true-peak bar, part of the engine's C ABI (MTR_METER_TPBALLIST).  Included by mtr_engine.h;
 * additions inside MTR_ABI_VERSION 2, looked up by name. */
#ifndef MTR_TPB_H
#define MTR_TPB_H

#ifndef MTR_ENGINE_H
#error "include mtr_engine.h: it defines mtr_engine and includes this header"
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* period_frames 0 (default): every engine call is ONE TruePeakdsp::process () per (stream, channel) followed by read (m, p)
 * (jmeters/truepeakdsp.cc:41-99, 133-138): mtr_stream_result.tpb_level / tpb_peak.
 * period_frames P > 0: every (stream, channel) is metered as by a host that calls TruePeakdsp::process (p, P) and then read (m, p) on
 * consecutive blocks of exactly P frames, wherever the process calls cut the audio (the dBTP plugins' bar, src/meters.cc:465-507, and
 * the true-peak bar of the DR-14 plugin, src/dr14.c:388, 421, at a fixed block size): at a block's start the two states are clamped to
 * [0, 20] (:54-55) and m and p start from 0, a read having preceded the block (:52-53, :133-138); at its end the states get + 1e-20f
 * (:86-87) and m *= g (:89).  A call boundary inside a block does none of that: the open block's running maxima and the raw states are
 * carried to the next call.  The interpolator's 47 frames of history run on across blocks and calls.  Every (m, p) is appended to two
 * per-stream series of `capacity_points` points of n_channels floats (engine-owned device memory; points past the capacity are dropped
 * and counted).
 * P must be 0 or 16 .. 8192, else MTR_ERR_ARG: 8192 is the reference's own limit for one process () (:44), 16 frames are what the
 * kernel walks at a time.  Only in an engine with MTR_METER_TPBALLIST (else MTR_ERR_ARG), mono or stereo, beside any other meter it
 * may hold, and only on an engine that has processed nothing since create / reset (else MTR_ERR_STATE).
 * With P > 0 mtr_engine_results' tpb_level / tpb_peak are the last completed block's — 0.0f before the first; mtr_engine_reset
 * empties the series and the open block and keeps P; the calls with per-stream lengths (mtr_engine_process_*_lengths / _tracks /
 * _ragged / _ends) refuse a TPBALLIST engine as they do without a period (MTR_ERR_UNSUPPORTED; mtr_engine_process_*_tpb takes it).
 * A state blob of such an engine carries the open block in one more section behind every older one: it goes into an engine of the
 * same period only (else MTR_ERR_STATE); the blob of an engine with P = 0 is what it always was. */
int  mtr_engine_tpb_set_period (mtr_engine* e, uint32_t period_frames, uint32_t capacity_points);
/* what set_period set; either pointer may be NULL */
int  mtr_engine_tpb_period (const mtr_engine* e, uint32_t* period_frames, uint32_t* capacity_points);
/* level, peak [count][capacity][n_channels] (either may be NULL): the first min (*n_points, capacity, capacity_points) readings of each
 * stream; *n_points = blocks completed since reset, *dropped = points that did not fit the series (the streams advance in lock step:
 * one number each). */
int  mtr_engine_tpb_series (mtr_engine* e, uint32_t first, uint32_t count, float* level, float* peak, uint32_t capacity,
                            uint32_t* n_points, uint32_t* dropped);

/* Track lengths for the true-peak bar — tracks that end where their audio ends, exactly and at the cost of their own frames, with a period as
 * without: mtr_engine_process_device_tpb / _host_tpb and mtr_engine_tpb_points, declared in mtr_tpb_ends.h (included by mtr_engine.h next
 * to mtr_ends.h).  Per (stream, channel) the reference's TruePeakdsp after exactly the stream's own frames (jmeters/truepeakdsp.cc:41-99,
 * 133-138): a stream that ends r frames into a block, 0 < r < P, gets one last process (p, r) and read (); the series getter above keeps
 * its lock-step counts, and the rows of a closed stream hold 0.0f behind its own points. */

#ifdef __cplusplus
}
#endif

#endif
