/* mtr_planes.h — plane layouts: the process calls take PLANAR audio, per stream one plane per channel, as a (batch, channel, time) tensor,
 * a (channel, time) array of an audio library or split-mono files hold it.  Included by mtr_engine.h; additions inside MTR_ABI_VERSION 2,
 * looked up by name.
 *
 * After mtr_engine_set_plane_layout (e, P, map) the buffers of every later process call hold, per stream, P planes of one channel each,
 * and the call's stream_stride_frames is the PLANE stride: plane p of stream s starts at base + (s * P + p) * stride * sample bytes and
 * holds the call's n_frames samples (f32, or the integer samples of the _pcm entry points).  Engine channel c is plane map[c] (map:
 * n_channels entries, each < P; the same plane may be named more than once: 1, {0, 0} is a mono file on a stereo engine; P may be smaller
 * or larger than n_channels, 1 .. MTR_MAX_FRAME_CHANNELS).  A contiguous (B, C, T) tensor is stride = T; a window [t0, t0 + n) of a long
 * one is base + t0 samples, stride = T: a long batch is walked in calls without a copy.  Planes the map does not name are never metered,
 * whatever they hold, and nothing at or behind n_frames samples of a plane is read.
 * It applies to every entry point that honours a frame layout: mtr_engine_process_device / _host, _pcm, _lengths, _tracks, _ragged, _ends,
 * _tpb, _any, _gonio_ends.  mtr_engine_process_planar_host / _prepare_host (the LV2 block path, n_streams == 1) are not affected.
 * A call with a plane layout runs k_plane (mtr_source.hip) in front of the meters: the planes (for host memory: as they crossed the link,
 * one 2-D copy of the chunk's P planes per stream) are decoded and interleaved into the float chunk the default layout would have staged —
 * for device memory in chunks of mtr_engine_set_host_chunk_bytes, as mtr_engine_process_device_pcm (set it to the decoded batch where HBM
 * allows) —, so every result is bit for bit that of the same entry point with the default layout on mtr_plane_decode_host () of each
 * stream, at the same mtr_engine_set_host_chunk_bytes. */
#ifndef MTR_PLANES_H
#define MTR_PLANES_H

#ifndef MTR_ENGINE_H
#error "include mtr_engine.h: it defines mtr_engine and includes this header"
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* n_planes == 0 (map ignored): back to the default.  Plane and frame layout exclude each other: a successful call of this setter puts the
 * frame layout back to its default (mtr_engine_frame_layout then answers n_channels and the identity), a successful
 * mtr_engine_set_frame_layout takes the plane layout away.  Like the frame layout it describes buffers, not streams: callable between any
 * two process calls, not part of the state blob, kept across mtr_engine_reset.  The identity (n_planes == n_channels, map 0 ..
 * n_channels - 1) is a plane layout like any other: the buffers are planar.
 * n_planes > MTR_MAX_FRAME_CHANNELS, map == NULL with n_planes > 0, an entry >= n_planes: MTR_ERR_ARG, nothing changed. */
int  mtr_engine_set_plane_layout (mtr_engine* e, uint32_t n_planes, const uint8_t* map /* [n_channels] */);
/* *n_planes: what is set, 0 without a plane layout (map then: the identity).  Either pointer may be NULL. */
int  mtr_engine_plane_layout (const mtr_engine* e, uint32_t* n_planes, uint8_t* map /* [n_channels], may be NULL */);
/* The definition the kernel is held against, plain C on the host, ONE stream (format 0 = f32, else MTR_PCM_*): dst [i * n_channels + c] =
 * sample i of plane map[c], plane p at src + p * stride_frames * sample bytes (any alignment).  f32 samples are copied as bit patterns (a
 * NaN keeps its payload), integers convert exactly as mtr_pcm_decode_host does.  n_planes 0 or > MTR_MAX_FRAME_CHANNELS, n_channels 0 or
 * > 8, map == NULL, an entry >= n_planes, stride_frames < n_frames, an unknown format: MTR_ERR_ARG. */
int  mtr_plane_decode_host (int format, const void* src, size_t n_frames, uint64_t stride_frames,
                            uint32_t n_planes, const uint8_t* map, uint32_t n_channels, float* dst /* [n_frames][n_channels] */);
/* chunks that went through k_plane since create (mtr_engine_layout_stats does not count them; mtr_engine_pcm_stats counts the chunks of
 * integer planes as PCM chunks, their bytes n_planes wide).  The pointer may be NULL. */
int  mtr_engine_plane_stats (mtr_engine* e, uint64_t* staged_chunks);

#ifdef __cplusplus
}
#endif

#endif
