/* mtr_ends.h — track lengths for the 30-band bank (MTR_METER_SPECTR30): the call of mtr_engine_process_device_ragged / _host_ragged for
 * engines that also hold the bank, and each stream's own count of the bank's reading series.  Included by mtr_engine.h, next to
 * mtr_ragged.h; additions inside MTR_ABI_VERSION 2, looked up by name. */
#ifndef MTR_ENDS_H
#define MTR_ENDS_H

#ifndef MTR_ENGINE_H
#error "include mtr_engine.h: it defines mtr_engine and includes this header"
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* The semantics of the _tracks pair, word for word (frames[s] <= n_frames; < n_frames closes stream s; 0 closes it untouched; a closed
 * stream is changed by no later call of any entry point until mtr_engine_reset; closure is not part of the state blob; frames == NULL or
 * frames[s] > n_frames: MTR_ERR_ARG before anything is queued), for engines whose mask is any non-empty combination of the meters _ragged
 * takes (EBU, TRUEPEAK, DR14, KMETER, BITSTATS, SIGDIST, STCORR, NEEDLE) and SPECTR30, mono or stereo.  An engine whose mask _ragged
 * accepts gives bit for bit what _ragged gives; a stream with frames[s] == n_frames comes out bit for bit as mtr_engine_process_device
 * leaves it.  The ends on the device are 32 bits: with SPECTR30 in the engine, n_frames > 2^32 - 2 is MTR_ERR_ARG — for this pair, and for
 * every process call of any entry point while one of the engine's streams is closed (such a call runs the same kernels); before anything
 * is queued, engine unchanged.
 * SPECTR30, per stream: the reference's spectrum_run (src/spectrumlv2.c:160-249) after exactly the stream's own frames.  No frame at or
 * behind frames[s] has any influence on any result, whatever the buffer holds there.
 *   period 0   the closing call is one spectrum_run of frames[s] frames: the epilogue (:230-238 — val, max and the z that are not finite
 *              become 0, val += 1e-20f) runs once, at the stream's end, and the dither parity of bandpass_process (src/spectr.c:81-82)
 *              advances by frames[s], not by n_frames;
 *   period P   (mtr_engine_spectr_set_period) the blocks are the engine's lock-step blocks.  A stream that ends r frames into one,
 *              0 < r < P, gets the epilogue and one truncated point (val, max) there, at the index of the whole blocks it completed; with
 *              MTR_SPECTR_PEAK_BLOCK max is zeroed behind it as behind any other; a truncated point at or beyond the capacity is dropped
 *              like any other.  r = 0 adds nothing: the block's end was the stream's, and there is no second epilogue.
 *   frames[s] == 0, or a stream that is already closed: nothing of it changes — states, levels, parity, series.
 * mtr_engine_spectrum reports where a closed stream stood at its end.  mtr_engine_spectr_series keeps its lock-step *n_points / *dropped —
 * the counts of a stream that was never closed — and the rows of a closed stream hold 0.0f (the dB outputs: -100) behind its own points,
 * whose number mtr_engine_spectr_points gives.
 * Once a stream is closed, every later call on the streams that hold it (mtr_engine_process_device / _host, an LV2 block) runs the
 * length-masking kernels, end 0 for the closed ones; mtr_engine_spectr_reset_peak reopens nothing.
 * Engines that hold TPBALLIST, SURROUND or SCOPE, or meter 3 .. 5 channels: MTR_ERR_UNSUPPORTED, nothing queued, engine unchanged.
 * mtr_engine_process_*_lengths / _tracks / _ragged refuse a SPECTR30 engine as before.
 * The _host form indexes `frames` by stream as mtr_engine_process_host's chunks do (bit for bit the _device form).
 * replaces: a host that stops calling spectrum_run (src/spectrumlv2.c:160) at the track's end, its last call cut to the frames left. */
int  mtr_engine_process_device_ends (mtr_engine* e, const float* d_audio, uint64_t n_frames,
                                     uint64_t stream_stride_frames, const uint64_t* frames, void* hip_stream);
int  mtr_engine_process_host_ends (mtr_engine* e, const float* h_audio, uint64_t n_frames,
                                   uint64_t stream_stride_frames, const uint64_t* frames);
/* points [count]: the points each stream's own SPECTR30 series has got since reset, dropped ones included: the whole blocks it completed
 * and, if it was closed inside one, the truncated block (the arithmetic of mtr_series_cut).  Period 0: no series, 0.  Counted on the host:
 * no device work, no synchronisation.  Zeroed by mtr_engine_reset; a stream that mtr_engine_state_import writes stands where the open
 * streams do.  No SPECTR30 in the engine, a stream range out of bounds or a NULL pointer: MTR_ERR_ARG.
 * replaces: the host's own count of the spectrum_runs it made for a track (src/spectrumlv2.c:160). */
int  mtr_engine_spectr_points (mtr_engine* e, uint32_t first, uint32_t count, uint64_t* points);

#ifdef __cplusplus
}
#endif

#endif
