/* mtr_any.h — track lengths for the scope and the surround meter: the call of mtr_engine_process_device_tpb / _host_tpb for engines that
 * also hold MTR_METER_SCOPE, and for MTR_METER_SURROUND engines; each stream's own count of the scope's analyses and series points.  Included by mtr_engine.h, next to
 * mtr_tpb_ends.h; additions inside MTR_ABI_VERSION 2, looked up by name. */
#ifndef MTR_ANY_H
#define MTR_ANY_H

#ifndef MTR_ENGINE_H
#error "include mtr_engine.h: it defines mtr_engine and includes this header"
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* Track lengths for the scope and the surround meter: a sixth pair of calls with per-stream ends, beside _lengths / _tracks / _ragged / _ends / _tpb (which keep
 * their meter sets, their refusals and their texts).  The semantics of the _tracks pair, word for word (frames[s] <= n_frames;
 * < n_frames closes stream s; 0 closes it untouched; a closed stream is changed by no later call of any entry point until
 * mtr_engine_reset; closure is not part of the state blob: an imported stream is open again and stands where the open streams do; a NULL
 * argument or frames[s] > n_frames: MTR_ERR_ARG before anything is queued), for
 *   stereo and mono engines whose mask is any non-empty combination of the meters _tpb takes (EBU, TRUEPEAK, DR14, KMETER, BITSTATS,
 *     SIGDIST, STCORR, NEEDLE, SPECTR30, TPBALLIST) and SCOPE (stereo);
 *   engines of 3 .. 5 channels with EBU / TRUEPEAK and SURROUND, and of 6 .. 8 channels with SURROUND, with a period or without.
 * An engine whose mask _tpb accepts gives bit for bit what _tpb gives, a 3 .. 5 channel EBU / TRUEPEAK engine what _lengths gives, under
 * those pairs' own limits (n_frames < 2^32 - 1 with SPECTR30, ...); a stream with frames[s] == n_frames comes out bit for bit as
 * mtr_engine_process_device leaves it.  An engine with a frame layout set is treated as _tpb treats it.  The PCM entry points take
 * lengths for EBU / TRUEPEAK engines only, as before.  The state blob's layout does not change.
 * One call is refused (MTR_ERR_UNSUPPORTED, nothing queued, engine unchanged): a SURROUND engine with a period whose open block stands
 * inside a group of four frames when the call starts (fill mod 4 != 0), and a stream with 0 < frames[s] < 4 - fill mod 4 — it ends before
 * that group completes.  Its last sur_run would have to drop the whole group from the K-meters' filter and peak (Kmeterdsp::process takes
 * n / 4 groups), and the surround meter keeps no state in front of a group that a call left open.  Calls of a multiple of four frames, or a
 * period that is one, never meet it.
 *
 * SCOPE, per stream: what fftx_run and the two process_audio over it leave when the host stops feeding the stream at its last frame
 * (gui/fft.c:289-361; gui/stereoscope.c:705-741, gui/phasewheel.c:1307-1339).  With E = frames[s] and `first` the call frame at which the
 * call's first analysis ends (hop - the frames since the last one):
 *   the analyses of the stream in the call are those that end at or before E: E < first ? 0 : (E - first) / hop + 1.  A hop that is not
 *     full runs no analysis (fft.c:308-311).  mtr_scope_series_cut with frames[s] for n_frames counts them;
 *   phase, plevel, power_l and power_r are what the stream's OWN last analysis leaves; a stream without an analysis in the call keeps all
 *     seven arrays of mtr_engine_scope_read as they were;
 *   the stream's last W frames, for the calls to come (an imported stream may go on), are the W frames in front of E;
 *   no frame at or behind E has any influence on any result, whatever the buffer holds there;
 *   frames[s] == 0, or a stream that is already closed: nothing of it changes.
 * SURROUND, per stream: sur_run's result after exactly its own frames (src/surmeter.c:115-147).
 *   period 0   the closing call is one sur_run of f = frames[s] frames.  Per channel one
 * Kmeterdsp::process (p, f): f & ~3 frames in groups of four, the weights counted back from its own last group, no group for f < 4, and
 * fpp = f with the fall-back factor of f (jmeters/kmeterdsp.cc:65-70, 79); per pair one Stcorrdsp::process with its flushes and + 1e-10f at
 * f (jmeters/stcorrdsp.cc:47-76).
 *   period P   (mtr_engine_surround_set_period) the blocks are the engine's lock-step blocks.  Whole blocks that end at or before the
 *              stream's end give their points as ever.  A stream that ends r frames into a block, 0 < r < P, gets one last sur_run of r
 *              frames: r & ~3 frames for the K-meters, fpp = r with its own fall-back factor, no group for r < 4; Stcorrdsp's lower
 *              bound on P does not apply to r.  Its reading is appended at the index of the whole blocks the stream completed — dropped
 *              like any other at or beyond the capacity — and is what mtr_engine_surround_read reports.  r = 0 adds nothing.
 *              mtr_engine_series_points (e, MTR_METER_SURROUND, ..) gives each stream's own number of points (mtr_series_cut is its
 *              arithmetic); mtr_engine_surround_series keeps its lock-step *n_points / *dropped and hands out 0.0f behind a closed
 *              stream's own points.
 * mtr_engine_surround_read / _pair_states report where a closed stream stood at its end.  No frame at or behind frames[s] is read;
 * frames[s] == 0 or a closed stream: nothing of it changes — mtr_sur_state, readings, open block, series.
 * The scope's reading series (mtr_scope_series.h): the groups of K analyses stay the engine's lock-step cursor, and a stream appends the points
 * among its own analyses.  mtr_engine_scope_analyses and the *n_points / *dropped of mtr_engine_scope_series stay lock-step — the counts of
 * a stream that was never closed — and the rows of a closed stream hold 0.0f behind its own points.
 * Once a stream is closed, every later call on the streams that hold it (mtr_engine_process_device / _host, an LV2 block) runs the
 * length-masking kernels, end 0 for the closed ones.
 * The _host form indexes `frames` by stream as mtr_engine_process_host's chunks do (bit for bit the _device form).
 * replaces: a host that stops calling fftx_run (gui/fft.c:289) / sur_run (src/surmeter.c:115) at the track's end, its last call cut to the
 * frames left. */
int  mtr_engine_process_device_any (mtr_engine* e, const float* d_audio, uint64_t n_frames,
                                    uint64_t stream_stride_frames, const uint64_t* frames, void* hip_stream);
int  mtr_engine_process_host_any (mtr_engine* e, const float* h_audio, uint64_t n_frames,
                                  uint64_t stream_stride_frames, const uint64_t* frames);
/* analyses [count], points [count]: the analyses each stream's own scope has run since reset, and the points its own series has got,
 * dropped ones included (no series: 0).  Either pointer may be NULL.  Counted on the host: no device work, no synchronisation.  Zeroed by
 * mtr_engine_reset / mtr_engine_scope_reset; a stream that mtr_engine_state_import writes takes the lock-step numbers.  No SCOPE in the
 * engine or a stream range out of bounds: MTR_ERR_ARG.
 * replaces: the host's own count of the fftx_run calls that returned 0 for a track (gui/stereoscope.c:709). */
int  mtr_engine_scope_points (mtr_engine* e, uint32_t first, uint32_t count, uint64_t* analyses, uint64_t* points);

#ifdef __cplusplus
}
#endif

#endif
