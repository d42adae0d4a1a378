/* mtr_ragged.h — ragged batches for the meters that report a reading OVER TIME: the phase correlation (MTR_METER_STCORR) and the needle
 * meters (MTR_METER_NEEDLE), beside the meters that mtr_engine_process_*_tracks takes.  Included by mtr_engine.h, next to mtr_tracks.h;
 * additions inside MTR_ABI_VERSION 2, looked up by name. */
#ifndef MTR_RAGGED_H
#define MTR_RAGGED_H

#ifndef MTR_ENGINE_H
#error "include mtr_engine.h: it defines mtr_engine and includes this header"
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* The call of mtr_engine_process_device_tracks / _host_tracks for engines that also hold STCORR or NEEDLE.  The semantics are those of
 * that pair, word for word (frames[s] <= n_frames; < n_frames closes stream s; 0 closes it untouched; a closed stream is changed by no
 * later call of any entry point until mtr_engine_reset; closure is not part of the state blob; frames == NULL or frames[s] > n_frames:
 * MTR_ERR_ARG before anything is queued), for engines whose mask is any non-empty combination of EBU, TRUEPEAK, DR14, KMETER, BITSTATS,
 * SIGDIST, STCORR and NEEDLE (channel rules as the meters state them).  An engine whose mask _tracks accepts gives bit for bit what
 * _tracks gives; a stream with frames[s] == n_frames comes out bit for bit as mtr_engine_process_device leaves it.
 * Per stream, the result is the reference's after exactly the stream's own frames, fed in the same blocks with the last one truncated:
 *   period 0   the closing call is one process (p, frames[s]) per detector — for the needle meters frames[s] & ~3 frames between the
 *              clamp at its start and the + 1e-10f (PPM) or the flushes (VU) at its end;
 *   period P   the blocks are the engine's lock-step blocks.  A stream that ends r frames into one, 0 < r < P, gets one last
 *              process (p, r) and one last read (): that reading is the stream's last point, at the index of the whole blocks it
 *              completed.  r = 0 adds nothing.  STCORR's lower bound on P does not apply to r; the needle meters drop the r mod 4
 *              trailing frames, and r < 4 is a process () of no group.  KMETER with a period (mtr_kmeter.h) likewise: _fpp = r with the
 *              fall-back factor of r, r / 4 groups; a group of four that an earlier call left open and the stream's end leaves
 *              incomplete drops out whole.
 * mtr_engine_stcorr_read / _needle_read report where a closed stream stood at its end: the reading of its last block, truncated or not,
 * and its states there.  mtr_engine_stcorr_series / _needle_series keep their lock-step *n_points / *dropped — the counts of a stream
 * that was never closed — and the rows of a closed stream hold 0.0f behind its own points (mtr_engine_series_points); a truncated last
 * point at index *n_points or beyond comes into their reach once the open streams have completed that block.
 * Once a stream is closed, every later call on the streams that hold it (mtr_engine_process_device / _host, an LV2 block) runs the
 * length-masking kernels, end 0 for the closed ones.  The per-meter resets (mtr_engine_stcorr_reset, _needle_reset, ...) reopen nothing.
 * Engines that hold SPECTR30, TPBALLIST, SURROUND or SCOPE: MTR_ERR_UNSUPPORTED, nothing queued, engine unchanged (SPECTR30 has a pair of
 * its own that takes these meters beside it: mtr_engine_process_device_ends / _host_ends, mtr_ends.h; SCOPE is taken by
 * mtr_engine_process_device_any / _host_any, mtr_any.h).  (SURROUND is taken by that pair too, but for one call with a period: a stream that ends before the
 * group of four frames completes which the call before left open needs its K-meters' state in front of that group, as KMETER's series
 * carries it, and the surround meter's kernel and state do not make it.)
 * replaces: a host that stops calling run() at the track's end. */
int  mtr_engine_process_device_ragged (mtr_engine* e, const float* d_audio, uint64_t n_frames,
                                       uint64_t stream_stride_frames, const uint64_t* frames, void* hip_stream);
int  mtr_engine_process_host_ragged (mtr_engine* e, const float* h_audio, uint64_t n_frames,
                                     uint64_t stream_stride_frames, const uint64_t* frames);
/* points [count]: the points each stream's own series of `meter` (MTR_METER_STCORR, MTR_METER_NEEDLE, MTR_METER_KMETER or MTR_METER_SURROUND; anything else, or a meter the
 * engine lacks: MTR_ERR_ARG) has got since reset, dropped ones included: the whole blocks it completed and, if it was closed inside
 * one, the truncated block.  Period 0: no series, 0.  Counted on the host: no device work, no synchronisation.  Zeroed by the meter's
 * reset and by mtr_engine_reset. */
int  mtr_engine_series_points (mtr_engine* e, uint32_t meter, uint32_t first, uint32_t count, uint64_t* points);
/* The arithmetic behind that count; host only, no device.  A series stands `fill` frames into a block of `period`; of a call of
 * n_frames a stream takes `frames`.  *whole: the blocks it completes; *partial: 1 if a truncated block follows them (the stream ends
 * inside the call, 0 < frames < n_frames, and inside a block), else 0.  period 0: *whole = 0, *partial = 1 exactly when
 * 0 < frames < n_frames (the closing call is the truncated block; an open stream's call is no series point).
 * fill >= period > 0, frames > n_frames or a NULL pointer: MTR_ERR_ARG. */
int  mtr_series_cut (uint64_t fill, uint64_t period, uint64_t n_frames, uint64_t frames, uint64_t* whole, uint32_t* partial);

#ifdef __cplusplus
}
#endif

#endif
