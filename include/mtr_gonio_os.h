/* mtr_gonio_os.h — the goniometer's "Oversampling" preference (gui/goniometer.c:155-189, :359-377): a factor of 2 .. 32 that puts a zita
 * Resampler (setup (rate, rate * f, 2, 12, 1.0)) in front of draw_rb.  Included by mtr_engine.h; additions inside MTR_ABI_VERSION 2,
 * looked up by name.  mtr_gonio_config keeps its size and fields.
 *
 * With factor f every input frame becomes f points (zita-resampler/resampler.cc:171-262 with np = f, hl = 12, pstep = 1, after setup_src's
 * 8192 zero frames): point m f + ph of a channel, x the stream's input since reset with zeros in front of it, is
 *     s = 1e-20f;  for i = 0 .. 11: s += x [m - 23 + i] * c1 [i] + x [m - i] * c2 [i];  out = s - 1e-20f
 * with c1 = ctab [ph], c2 = ctab [f - ph], every operation a separate f32 operation in that order (no fused multiply-add) — phase 0
 * included, whose side taps are about 3.8e-17, not 0.  draw_rb then walks the points as it walks frames: a display update of P input
 * frames is P f points, rms_c is P f, hpw is that of mtr_gonio_os_hpw, while `elapsed` — and with it the attack pair — stays P / rate and
 * the `n_samples < 64` floor counts input frames.  The results are the reference's bit for bit, wherever the calls cut the audio: the
 * engine keeps every stream's last 23 input frames from call to call.
 * Series, image, counters and mtr_engine_gonio_read keep their meaning: drawn + clipped + skipped counts points, f per input frame;
 * mtr_engine_gonio_blocks counts display updates of P input frames; mtr_engine_gonio_points and mtr_gonio_cut count input frames. */
#ifndef MTR_GONIO_OS_H
#define MTR_GONIO_OS_H

#ifndef MTR_ENGINE_H
#error "include mtr_engine.h: it defines mtr_engine and includes this header"
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define MTR_GONIO_OS_MAX  32       /* gui/goniometer.c:974: the preference's range is 2 .. 32, 4 by default */
#define MTR_GONIO_OS_TAPS 12       /* hlen of setup_src: a row of the table; a point reads 2 * 12 input frames */

/* out [(factor + 1) * 12]: Resampler_table's _ctab for fr = 1.0, hl = 12, np = factor, built in double as
 * zita-resampler/resampler-table.cc:52-75 builds it: out [j * 12 + 11 - i] = (float) (sinc (t) * wind (t / 12)), t = j / factor + i.
 * Needs no engine and no device.  factor 2 .. 32, else MTR_ERR_ARG. */
int  mtr_gonio_os_table (uint32_t factor, float* out);
/* *hpw = expf (-2.0 * M_PI * 20 / (rate * (float) factor))  (:175: rate a double, the factor a float).  factor 1 .. 32 (1: the value of
 * mtr_gonio_derived), rate >= 8000, else MTR_ERR_ARG.  Needs no engine and no device. */
int  mtr_gonio_os_hpw (double rate, uint32_t factor, float* hpw);
/* factor 1: off (the default), 2 .. 32: on.  Like mtr_engine_gonio_configure only on an engine that has processed nothing since create /
 * reset (else MTR_ERR_STATE); resets the meter.  MTR_ERR_ARG: factor 0 or above 32, an engine without the meter, or a factor above 1 with
 * a display update longer than floor (rate) frames — the reference's scratch holds `rate` frames (:173-181) — in whichever order this
 * call and mtr_engine_gonio_configure come: the later one is refused.  mtr_engine_gonio_configure keeps the factor; mtr_engine_reset and
 * mtr_engine_gonio_reset keep it too and zero the streams' input history.
 * With a factor above 1: a process call whose n_frames * factor does not stay below 2^32 - 1 is refused (MTR_ERR_ARG); the engine holds
 * one more scratch of n_streams * tune_piece * 8 bytes (a piece of a call is tune_piece / factor input frames, never more than tune_piece
 * points); the state blob carries the factor and the history rows, and an engine takes a blob of its own factor only (MTR_ERR_STATE).  An
 * engine at factor 1, told so or never told, exports the blob it always did. */
int  mtr_engine_gonio_set_oversample (mtr_engine* e, uint32_t factor);
/* *factor: what is set; *hpw: what the chain runs on — mtr_gonio_os_hpw (rate, factor).  (mtr_engine_gonio_config's derived.hpw goes on
 * answering the factor-1 value of :165, whatever the factor.)  Either may be NULL. */
int  mtr_engine_gonio_oversample (mtr_engine* e, uint32_t* factor, float* hpw);
/* For measurements (tools/gonio_rate.py), beside mtr_engine_gonio_timing, which switches the timing on and off and answers the other two
 * kernels: *os_ms: k_gonio_os' time summed over the *pieces timed since the last query of THIS getter, which are then forgotten.
 * Synchronises. */
int  mtr_engine_gonio_os_timing (mtr_engine* e, float* os_ms, uint32_t* pieces);

#ifdef __cplusplus
}
#endif

#endif
