/* mtr_tracks.h — track lengths for the whole-track meters of the engine's C ABI: a batch of tracks that end where their audio ends, for
 * DR-14, the K-meter reading, the bit statistics and the signal-distribution histogram (and EBU R128 / true peak beside them).  Included by
 * mtr_engine.h, next to the _lengths pair whose semantics these entries share; additions inside MTR_ABI_VERSION 2, looked up by name. */
#ifndef MTR_TRACKS_H
#define MTR_TRACKS_H

#ifndef MTR_ENGINE_H
#error "include mtr_engine.h: it defines mtr_engine and includes this header"
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* The call of mtr_engine_process_device_lengths / _host_lengths for the meters whose answer is one per TRACK.  The semantics are those of
 * that pair, word for word (frames[s] <= n_frames; < n_frames closes stream s; 0 closes it untouched; a closed stream is changed by no
 * later call of any entry point until mtr_engine_reset; closure is not part of the state blob; frames == NULL or frames[s] > n_frames:
 * MTR_ERR_ARG before anything is queued), for engines whose mask is any combination of EBU, TRUEPEAK, DR14, KMETER, BITSTATS and
 * SIGDIST (channel rules as mtr_config.n_channels states them).  An EBU / TRUEPEAK-only engine gives bit for bit what _lengths gives.
 * Per stream, the result is the reference's after exactly the stream's own frames, fed in the same call blocks with the last one
 * truncated:
 *   DR14      windows are counted per stream; the window a track ends in stays open, as dr14_run leaves it (src/dr14.c:394-412) — zero
 *             padding would close it;
 *   KMETER    the closing call is one Kmeterdsp::process (p, frames[s]): frames[s] / 4 groups, fall-back factor and hold count-down of
 *             that many frames (jmeters/kmeterdsp.cc:56-140) — "where the needle stood when the track ended", no decay over padding;
 *   BITSTATS  the track's own samples only: no padding zeros in `zero` (src/bitmeter.c:63-105);
 *   SIGDIST   likewise, and the sample index the moments divide by counts the track's samples only (src/sigdistlv2.c:296-327).
 * A stream with frames[s] == n_frames comes out bit for bit as mtr_engine_process_device leaves it.  Once a stream is closed, every later
 * call on the streams that hold it (mtr_engine_process_device / _host, an LV2 block) runs the length-masking kernels, end 0 for the
 * closed ones.  The per-meter resets (mtr_engine_dr14_reset, _kmeter_reset, _intstat_reset) reopen nothing.
 * Engines that hold SPECTR30, TPBALLIST, STCORR, NEEDLE or SURROUND: MTR_ERR_UNSUPPORTED, nothing queued, engine unchanged (STCORR and
 * NEEDLE beside these meters: mtr_engine_process_device_ragged / _host_ragged, mtr_ragged.h).  A KMETER engine with a period
 * (mtr_engine_kmeter_set_period, mtr_kmeter.h) keeps a reading over time and is refused likewise: it takes the _ragged pair.
 * replaces: a host that stops calling run() at the track's end. */
int  mtr_engine_process_device_tracks (mtr_engine* e, const float* d_audio, uint64_t n_frames,
                                       uint64_t stream_stride_frames, const uint64_t* frames, void* hip_stream);
int  mtr_engine_process_host_tracks (mtr_engine* e, const float* h_audio, uint64_t n_frames,
                                     uint64_t stream_stride_frames, const uint64_t* frames);

#ifdef __cplusplus
}
#endif

#endif
