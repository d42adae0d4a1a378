/* mtr_spectr.h — the 30-band bank's reading series, part of the engine's C ABI (MTR_METER_SPECTR30).  Included by mtr_engine.h, which
 * declares mtr_engine_spectr_set_speed / _reset_peak and mtr_engine_spectrum itself; additions inside MTR_ABI_VERSION 2, looked up by
 * name. */
#ifndef MTR_SPECTR_H
#define MTR_SPECTR_H

#ifndef MTR_ENGINE_H
#error "include mtr_engine.h: it defines mtr_engine and includes this header"
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define MTR_SPECTR_PEAK_HOLD  0   /* max_f as the ports show it: held since reset / mtr_engine_spectr_reset_peak */
#define MTR_SPECTR_PEAK_BLOCK 1   /* max_f = 0 at the start of every block: the host that answers every reading with
                                     the peak-reset handshake (src/spectrumlv2.c:191-198) */

/* period_frames 0 (the default): every process call is ONE spectrum_run per stream (src/spectrumlv2.c:160-249), read when the caller asks
 * (mtr_engine_spectrum).  Nothing changes, no memory is held, the kernel is the one it is without the series.
 * 1 <= period_frames P <= 2^31 - 2: the streams are metered as by a host that calls spectrum_run on consecutive blocks of exactly P frames,
 * counted from create / mtr_engine_reset, and reads val_f / max_f after each; the process calls only deliver audio, wherever they cut it.
 * At a block's last frame the engine does what spectrum_run's epilogue does (:230-238): val, max and the twelve z of every band that are
 * not finite become 0, val += 1e-20f; then (val, max) of the 30 bands is appended to two per-stream series of `capacity_points` points
 * (engine-owned device memory); with MTR_SPECTR_PEAK_BLOCK max is zeroed behind the point (:191-198).  A call that ends inside a block
 * does none of that: it stores the states as they stand — no scrub, no + 1e-20f — and mtr_engine_spectrum then reads that mid-block state.
 * The dither parity of bandpass_process (src/spectr.c:81-82) runs on across blocks and calls as it does without a period.  The series
 * therefore does not depend on where the calls cut the audio, bit for bit; and it is, bit for bit, what an engine without a period gives
 * that is fed calls of exactly P frames and read (and, for MTR_SPECTR_PEAK_BLOCK, sent mtr_engine_spectr_reset_peak) after each.
 * Points past `capacity_points` are dropped and counted, never written; capacity_points 0 is allowed: every point is then dropped.
 * Every route of a process call appends: device and host memory (every view of a chunked host call cuts its blocks where the call
 * started), integer PCM, frame layouts, mono and stereo engines.  mtr_engine_process_*_lengths / _tracks / _ragged refuse a SPECTR30
 * engine as before.  That costs little: the bank is causal and the streams run in lock step, so of a zero-padded track every point that
 * ends at or before the track's own last frame is already exact — the first frames / P points of its row; the host knows that number.
 * mtr_engine_series_points does not know this series (the points are lock-step: *n_points below).  Tracks that end where their audio
 * ends, exactly and at the cost of their own frames: mtr_engine_process_device_ends / _host_ends and mtr_engine_spectr_points, mtr_ends.h.
 * mtr_engine_spectr_set_speed works as before (the omega of the next call); mtr_engine_spectr_reset_peak zeroes max wherever the open
 * block stands; mtr_engine_reset empties the series, the counts and the open block and keeps P, the capacity and the mode.
 * MTR_ERR_ARG: an unknown peak_mode, P > 2^31 - 2, no SPECTR30 in the engine.  Only on an engine that has processed nothing since create /
 * reset, else MTR_ERR_STATE (the rule of mtr_engine_stcorr_set_period).  Memory that cannot be had: MTR_ERR_NOMEM, and the series is off.
 * State blob: without a period it is byte for byte what it was; with one it carries one more section behind every older one — period,
 * peak mode and the frames into the open block — and goes into an engine of the same period and mode only (a fresh one continues the
 * open block; one that has processed must stand at the same frame of it), else MTR_ERR_STATE.  The series itself is not part of the
 * blob: an importing engine's series and counts stay as they are. */
int  mtr_engine_spectr_set_period (mtr_engine* e, uint32_t period_frames, uint32_t capacity_points, int peak_mode);
/* what set_period set; any pointer may be NULL */
int  mtr_engine_spectr_period (const mtr_engine* e, uint32_t* period_frames, uint32_t* capacity_points, int* peak_mode);
/* val, max, val_db, max_db [count][capacity][30] (any may be NULL): the first min (*n_points, capacity, capacity_points) points of each
 * stream, the rest of each row is left as it was.  val / max are val_f / max_f as stored at the block's end (val carries the + 1e-20f of
 * :237, invisible above the -100 dB floor), val_db / max_db the port values of :240-247, the arithmetic of mtr_engine_spectrum.
 * *n_points = blocks completed since reset, *dropped = points that did not fit the series (the streams advance in lock step: one number
 * each; either may be NULL).  Waits for the caller's stream.  The series is off: MTR_ERR_ARG. */
int  mtr_engine_spectr_series (mtr_engine* e, uint32_t first, uint32_t count,
                               float* val, float* max, float* val_db, float* max_db,
                               uint32_t capacity, uint32_t* n_points, uint32_t* dropped);

#ifdef __cplusplus
}
#endif

#endif
