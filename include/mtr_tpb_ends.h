/* mtr_tpb_ends.h — track lengths for the true-peak bar (MTR_METER_TPBALLIST): the call of mtr_engine_process_device_ends / _host_ends for
 * engines that also hold the bar, and each stream's own count of the bar's reading series (mtr_tpb.h).  Included by mtr_engine.h, next to
 * mtr_ends.h; additions inside MTR_ABI_VERSION 2, looked up by name. */
#ifndef MTR_TPB_ENDS_H
#define MTR_TPB_ENDS_H

#ifndef MTR_ENGINE_H
#error "include mtr_engine.h: it defines mtr_engine and includes this header"
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* Track lengths for the true-peak bar: a fifth pair of calls with per-stream ends, beside _lengths / _tracks / _ragged / _ends (which keep
 * their meter sets and go on refusing a TPBALLIST engine).  The semantics of the _tracks pair, word for word (frames[s] <= n_frames;
 * < n_frames closes stream s; 0 closes it untouched; a closed stream is changed by no later call of any entry point until
 * mtr_engine_reset; closure is not part of the state blob; a NULL argument or frames[s] > n_frames: MTR_ERR_ARG before anything is
 * queued), for engines whose mask is any non-empty combination of the meters _ends takes (EBU, TRUEPEAK, DR14, KMETER, BITSTATS, SIGDIST,
 * STCORR, NEEDLE, SPECTR30) and TPBALLIST, mono or stereo.  An engine whose mask _ends accepts gives bit for bit what _ends gives, under
 * _ends' own limits; a stream with frames[s] == n_frames comes out bit for bit as mtr_engine_process_device leaves it.
 * TPBALLIST, per (stream, channel): the reference's TruePeakdsp after exactly the stream's own frames (jmeters/truepeakdsp.cc:41-99,
 * 133-138).  No frame at or behind frames[s] has any influence on any result, whatever the buffer holds there: the interpolator's output
 * behind a track's last frame is never looked at, the states do not decay over padding.
 *   period 0   the closing call is one process (p, frames[s]) followed by read (m, p): tpb_level / tpb_peak are that reading, the states
 *              are stored + 1e-20f (:86-87);
 *   period P   (mtr_engine_tpb_set_period) the blocks are the engine's lock-step blocks.  Whole blocks that end at or before the stream's
 *              end give their points as ever.  A stream that ends r frames into a block, 0 < r < P, gets one last process (p, r) and
 *              read (): that block takes up the open maxima of earlier calls as any block that straddles calls does, and its reading is
 *              appended at the index of the whole blocks the stream completed — dropped like any other at or beyond the capacity — and
 *              is what mtr_engine_results reports; the states get their + 1e-20f and the open block is left as behind a block's end.
 *              r = 0 adds nothing: the block's end was the stream's.
 *   frames[s] == 0, or a stream that is already closed: nothing of it changes — states, tpb_level / tpb_peak, the open block, the
 *              series, the interpolator's 47 frames of history.
 * A stream that ends inside the call leaves the 47 frames in front of its own end as its history.  mtr_engine_tpb_series keeps its
 * lock-step *n_points / *dropped — the counts of a stream that was never closed — and the rows of a closed stream hold 0.0f behind its
 * own points, whose number mtr_engine_tpb_points gives (the getter hands out the lock-step number of points: a truncated point that lies
 * behind the engine's last whole block is in the series' memory and in mtr_engine_results, and comes out once the engine has completed
 * another block).  Once a stream is closed, every later call on the streams that hold it
 * (mtr_engine_process_device / _host, an LV2 block) runs the length-masking kernels, end 0 for the closed ones.
 * Engines that hold SURROUND or SCOPE, or meter 3 .. 5 channels: MTR_ERR_UNSUPPORTED, nothing queued, engine unchanged.  The PCM entry
 * points take lengths for EBU / TRUEPEAK engines only, as before.  The state blob's layout does not change.
 * The _host form indexes `frames` by stream as mtr_engine_process_host's chunks do (bit for bit the _device form).
 * replaces: a host that stops calling TruePeakdsp::process (truepeakdsp.cc:41) at the track's end, its last call cut to the frames left,
 * and reads the meter there. */
int  mtr_engine_process_device_tpb (mtr_engine* e, const float* d_audio, uint64_t n_frames,
                                    uint64_t stream_stride_frames, const uint64_t* frames, void* hip_stream);
int  mtr_engine_process_host_tpb (mtr_engine* e, const float* h_audio, uint64_t n_frames,
                                  uint64_t stream_stride_frames, const uint64_t* frames);
/* points [count]: the points each stream's own TPBALLIST series has got since reset, dropped ones included: the whole blocks it completed
 * and, if it was closed inside one, the truncated block (the arithmetic of mtr_series_cut).  Period 0: no series, 0.  Counted on the
 * host: no device work, no synchronisation.  Zeroed by mtr_engine_reset; a stream that mtr_engine_state_import writes stands where the
 * open streams do.  No TPBALLIST in the engine, a stream range out of bounds or a NULL pointer: MTR_ERR_ARG.
 * replaces: the host's own count of the process () / read () pairs it made for a track. */
int  mtr_engine_tpb_points (mtr_engine* e, uint32_t first, uint32_t count, uint64_t* points);

#ifdef __cplusplus
}
#endif

#endif
