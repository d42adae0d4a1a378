/* mtr_gonio.h — the goniometer's part of the engine's C ABI (MTR_METER_GONIO): the M/S point image of draw_rb (gui/goniometer.c:299-538),
 * its auto gain and a reading series, for a batch.  Included by mtr_engine.h; additions inside MTR_ABI_VERSION 2, looked up by name. */
#ifndef MTR_GONIO_H
#define MTR_GONIO_H

#ifndef MTR_ENGINE_H
#error "include mtr_engine.h: it defines mtr_engine and includes this header"
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define MTR_GONIO_BOUNDS 373       /* gui/goniometer.c:56  GM_BOUNDS: the surface is 373 x 373 */

/* The goniometer for a batch (MTR_METER_GONIO; stereo engines only — a pair of a wider frame goes through mtr_engine_set_frame_layout).
 * Combines with every other stereo meter.  Track lengths: mtr_engine_process_device_gonio_ends / _host_gonio_ends (mtr_gonio_ends.h); the six
 * older pairs of calls with per-stream ends (mtr_engine_process_*_lengths .. _any) refuse the meter.
 * What is reproduced is draw_rb in points mode (s_line false), with or without oversampling (src_fact 1, the default, or 2 .. 32 through
 * mtr_engine_gonio_set_oversample: mtr_gonio_os.h, which says what a frame below becomes then), with infinite persistence
 * (persist >= 1.0, gui/goniometer.c:327) and without inflate, in the reference's f32 / double operations and their order: per frame
 * (:401-449) the one-pole per channel, lp += hpw (d - lp), lp += 1e-12f; ax = lp0 - lp1, ay = lp0 + lp1; x = 186.5f - gain ax 100.f, y
 * alike; a frame whose point moved less than sqrt (2) from the last painted one is skipped, any other is painted at
 * px = rintf (last_x - w * .5), py alike (:470, half to even): inside the surface it increments cell [py >> shift][px >> shift] of the
 * stream's image, uint32 [G][G] with G = (373 + (1 << shift) - 1) >> shift, outside of it (NaN coordinates included) it counts as clipped.
 * One display update is one BLOCK of exactly P frames, counted from reset wherever the process calls cut the audio (a lock-step cursor);
 * at its end (:494-537) an lp that is not finite becomes 0 and, with auto gain, the gain moves as :497-527 move it (the fader's side
 * effects, :529-534, never reach ui->gain), and one point — the gain behind the update, the block's painted points inside the surface and
 * its clipped ones — is appended to the stream's series of `capacity` points (points past the capacity are counted, not written). */
typedef struct mtr_gonio_config {
	uint32_t struct_size;        /* sizeof (mtr_gonio_config) */
	uint32_t period_frames;      /* P: 0 = rint (rate / 25) (src/goniometerlv2.c:25,81), else 64 (draw_rb's `n_samples < 64` return) .. 2^20 */
	uint32_t capacity;           /* points per stream the series holds; 0 with P = 0: 4096, 0 with P set: MTR_ERR_ARG */
	uint32_t shift;              /* 0 = 2; 1, 2 or 3: G = 187, 94 or 47 */
	uint32_t autogain;           /* 0: off; 1: on, the reference's dials (attack 54, decay 58, target 40, rms 50: src/goniometerlv2.c:101-104; the
	                              * four fields below must be 0); 2: on, the four dials below as given, 0 .. 100 each */
	float    gain;               /* ui->gain at reset (:1091); 0 = 1.0f; finite, > 0 */
	float    point_width;        /* w (src/goniometerlv2.c:97); 0 = 1.75f; finite, > 0 */
	float    g_attack, g_decay, g_target, g_rms;   /* the dials of cb_autosettings (:897-912) */
	uint32_t tune_piece;         /* frames per launch of the two kernels (the cell codes' scratch holds that many per stream); 0 = 4096, else 64 .. 2^20 */
} mtr_gonio_config;

/* What the meter runs on, derived on the host with libm as the reference derives it */
typedef struct mtr_gonio_derived {
	uint32_t period_frames;      /* P, resolved */
	uint32_t G;                  /* cells per image row and column */
	float    hpw;                /* expf (-2.0 * M_PI * 20 / rate)  (:165): the factor-1 value, whatever mtr_engine_gonio_set_oversample set
	                              * (what the chain runs on then: mtr_engine_gonio_oversample) */
	float    attack[2];          /* `attack` of :524 for elapsed = P / rate: [0] where the target is below the gain, [1] otherwise */
	float    g_target, g_rms;    /* :906-912 */
} mtr_gonio_derived;

/* Resolves and derives; needs no engine and no device.  MTR_ERR_ARG: a NULL, a bad struct_size, a value outside the ranges above,
 * rate < 8000. */
int  mtr_gonio_derive (const mtr_gonio_config* cfg, double rate, mtr_gonio_derived* out);
/* Replaces the instantiate-time and preferences set-up of the UI (:1086-1091, :897-912, state_to_ui).  Only on an engine that has
 * processed nothing since create / reset (else MTR_ERR_STATE); bad values: MTR_ERR_ARG.  Resets the meter.  An engine that was never
 * configured runs the all-zero configuration. */
int  mtr_engine_gonio_configure (mtr_engine* e, const mtr_gonio_config* cfg);
/* The configuration with every zero resolved (dials included: autogain 1 answers 54, 58, 40, 50), and what was derived from it; either may be NULL. */
int  mtr_engine_gonio_config (mtr_engine* e, mtr_gonio_config* cfg, mtr_gonio_derived* derived);
/* The port JF_GAIN / the fader (set_gain, :864-870): ui->gain of every stream = gain, from the next process call's first frame.  With
 * auto gain on the loop moves it on from there, as the reference's does.  mtr_engine_reset returns to the configured gain.  Finite, > 0. */
int  mtr_engine_gonio_set_gain (mtr_engine* e, float gain);
/* img [count][G][G], drawn / clipped / skipped [count]: the surfaces ui->sf (:470-490) as counts per cell, and the frames of :446-449
 * since reset or mtr_engine_gonio_image_clear: painted inside the surface, painted outside of it, skipped.  Cell counts wrap at 2^32. */
int  mtr_engine_gonio_image (mtr_engine* e, uint32_t first, uint32_t count, uint32_t* img, uint64_t* drawn, uint64_t* clipped, uint64_t* skipped);
/* gain [count], lp [count][2], last [count][2] = last_x, last_y: ui->gain, ui->lp0 / lp1, ui->last_x / last_y as they stand (:128-134). */
int  mtr_engine_gonio_read (mtr_engine* e, uint32_t first, uint32_t count, float* gain, float* lp, float* last);
/* *blocks: display updates (draw_rb calls, :299) completed since reset; *held: those of them the series holds (min (*blocks, capacity)). */
int  mtr_engine_gonio_blocks (mtr_engine* e, uint64_t* blocks, uint64_t* held);
/* Points [from, from + n) of each stream's series into gain / drawn / clipped [count][n]: ui->gain behind the block's update (:536), the
 * block's rectangles inside the surface (:470) and those outside.  from + n beyond the held points: MTR_ERR_ARG. */
int  mtr_engine_gonio_series (mtr_engine* e, uint32_t first, uint32_t count, uint64_t from, uint32_t n, float* gain, uint32_t* drawn, uint32_t* clipped);
/* Clears the images and the three counters of every stream (the "clear" of the surfaces, ALLOC_SF :284-291); filters, last point, gain,
 * the open block and the series stay. */
int  mtr_engine_gonio_image_clear (mtr_engine* e);
/* The state of :1086-1091 (lp 0, last point at the centre, the configured gain), images, counters and series emptied; the configuration
 * stays.  Part of mtr_engine_reset. */
int  mtr_engine_gonio_reset (mtr_engine* e);
/* For measurements (tools/gonio_rate.py): enable != 0 starts timing the two kernels of every piece with events, 0 stops it; *points_ms /
 * *image_ms: k_gonio_points' and k_gonio_image's time summed over the *pieces timed since the last query, which are then forgotten.  No
 * reference counterpart.  Synchronises.  (k_gonio_os of an oversampling engine: mtr_engine_gonio_os_timing, mtr_gonio_os.h.) */
int  mtr_engine_gonio_timing (mtr_engine* e, int enable, float* points_ms, float* image_ms, uint32_t* pieces);
/* Getters synchronise; any output pointer may be NULL; a NULL engine or one without the meter: MTR_ERR_ARG. */

#ifdef __cplusplus
}
#endif

#endif
