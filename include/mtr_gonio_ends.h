/* mtr_gonio_ends.h — track lengths for the goniometer (MTR_METER_GONIO): a seventh pair of calls with per-stream ends, the arithmetic of a
 * stream's last display update, and each stream's own count of its updates.  Included by mtr_engine.h behind mtr_gonio.h; additions inside
 * MTR_ABI_VERSION 2, looked up by name. */
#ifndef MTR_GONIO_ENDS_H
#define MTR_GONIO_ENDS_H

#ifndef MTR_ENGINE_H
#error "include mtr_engine.h: it defines mtr_engine and includes this header"
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* Track lengths for the goniometer, beside _lengths / _tracks / _ragged / _ends / _tpb / _any (which keep their meter sets, their refusals
 * and their texts: they refuse an engine that holds GONIO).  The semantics of the _tracks pair, word for word (frames[s] <= n_frames;
 * < n_frames closes stream s; 0 closes it untouched; a closed stream is changed by no later call of any entry point until
 * mtr_engine_reset; closure is not part of the state blob: an imported stream is open again and stands where the open streams do; a NULL
 * argument or frames[s] > n_frames: MTR_ERR_ARG before anything is queued), for stereo engines that hold GONIO, alone or beside any of the
 * stereo meters _any takes (EBU, TRUEPEAK, DR14, KMETER, BITSTATS, SIGDIST, STCORR, NEEDLE, SPECTR30, TPBALLIST, SCOPE) — those give bit for
 * bit what _any gives an engine without GONIO, under its limits.  An engine without GONIO: MTR_ERR_UNSUPPORTED (it is _any's).  n_frames
 * per call < 2^32 - 1: the cuts are 32 bits (and so for every call once a stream is closed).  A frame layout and the PCM entry points are
 * treated as _any treats them.  The state blob's layout does not change.
 *
 * GONIO, per stream: what draw_rb leaves when the host stops calling run () at the track's end and exposes the display once more.
 * goniometer_run (src/goniometerlv2.c:145-186) fills the ring, draw_rb (gui/goniometer.c:299-538) takes what the ring holds
 * (n_samples = gmrb_read_space, :301) and returns at n_samples < 64 (:302).  The engine's display updates are its lock-step blocks of P
 * frames; with E = frames[s], `fill` the frames into the open block at the call's start and r = (fill + E) mod P for a stream the call
 * closes (0 < E < n_frames):
 *   whole blocks that end at or before E give their points, image cells and gain updates as ever;
 *   r = 0      nothing more;
 *   r >= 64    one closing draw_rb of r frames: its frames as ever (:401-449), :494-495 at its end and, with auto gain, :497-536 with
 *              n_samples = r — elapsed = (float) ((size_t) r / rate) (:499), rms_c = r (:507), `attack` of :524 from that elapsed, derived
 *              on the host with libm's log10f / logf as mtr_gonio_derive derives the block's.  Its point (the gain behind the update,
 *              painted inside, painted outside) is appended at the index of the whole blocks the stream completed — dropped like any
 *              other at or beyond the capacity;
 *   0 < r < 64 no closing update: the r frames stay in the ring, never filtered, never drawn.  The stream stands where its last whole
 *              block left it — lp, last point, gain, image, counters — and the r frames count as neither drawn, clipped nor skipped.
 *              (Never in front of the call's first frame: what earlier calls drew of the open block stays drawn.  A stream whose last
 *              whole block lies before this call is left untouched by it, apart from being closed.)
 * Behind its end the stream's open-block accumulators are zero, as behind any update.  E = 0, or a stream that is already closed:
 * nothing of it changes.  E = n_frames: bit for bit what mtr_engine_process_device leaves.  No frame at or behind E is read, and none has
 * any influence on any result, whatever the buffer holds there.  Once a stream is closed, every later call on the streams that hold it
 * (mtr_engine_process_device / _host, an LV2 block) runs the ENDS kernels, end 0 for the closed ones.
 * mtr_engine_gonio_blocks and the held points of mtr_engine_gonio_series stay lock-step — the counts of a stream that was never closed —
 * and the rows of a closed stream hold 0 behind its own points.
 * The _host form indexes `frames` by stream as mtr_engine_process_host's chunks do (bit for bit the _device form).
 * replaces: a host that stops calling run () (src/goniometerlv2.c:145) at the track's end and lets the UI draw once more. */
int  mtr_engine_process_device_gonio_ends (mtr_engine* e, const float* d_audio, uint64_t n_frames,
                                           uint64_t stream_stride_frames, const uint64_t* frames, void* hip_stream);
int  mtr_engine_process_host_gonio_ends (mtr_engine* e, const float* h_audio, uint64_t n_frames,
                                         uint64_t stream_stride_frames, const uint64_t* frames);
/* The arithmetic above for one stream that takes `frames` of a call of n_frames which starts `fill` frames into a display update of
 * `period` frames (64 .. 2^20; cfg's own period_frames is not read) at `rate`; needs no engine and no device.  *whole: display updates of
 * `period` frames it completes; *closing_frames: r where a closing update runs, else 0; *drawn_frames: the call frame at which its
 * drawing ends (frames, or frames - r for 0 < r < 64, never below 0); attack [2]: the closing update's `attack` of :524 from cfg's dials
 * ([0] where the target is below the gain, [1] otherwise; negative where the formula gives it so: r = 64 at 192 kHz), 0 without one.
 * MTR_ERR_ARG: a NULL, fill >= period, frames > n_frames, or what mtr_gonio_derive refuses.
 * Everything here counts INPUT frames, with or without oversampling (mtr_gonio_os.h): draw_rb's floor of 64 and `elapsed` do; a closing
 * update of r frames then walks r f points with rms_c = r f. */
int  mtr_gonio_cut (uint64_t fill, uint32_t period, double rate, uint64_t n_frames, uint64_t frames, const mtr_gonio_config* cfg,
                    uint64_t* whole, uint32_t* closing_frames, uint64_t* drawn_frames, float attack[2]);
/* updates [count], points [count]: each stream's own display updates since reset, closing ones included, and the points its series has
 * got, dropped ones included (every update appends one: the two are equal).  Either pointer may be NULL.  Counted on the host: no device
 * work, no synchronisation.  Zeroed by mtr_engine_reset / mtr_engine_gonio_reset; a stream that mtr_engine_state_import writes takes the
 * lock-step number.  No GONIO in the engine or a stream range out of bounds: MTR_ERR_ARG.
 * replaces: the host's own count of the exposes that drew (draw_rb calls that passed :302). */
int  mtr_engine_gonio_points (mtr_engine* e, uint32_t first, uint32_t count, uint64_t* updates, uint64_t* points);

#ifdef __cplusplus
}
#endif

#endif
