/* mtr_scope_series.h — the stereo / frequency scope's reading series, part of the engine's C ABI (MTR_METER_SCOPE).  Included by
 * mtr_scope.h; additions inside MTR_ABI_VERSION 2, looked up by name. */
#ifndef MTR_SCOPE_SERIES_H
#define MTR_SCOPE_SERIES_H

#ifndef MTR_SCOPE_H
#error "include mtr_engine.h: it includes mtr_scope.h, which includes this header"
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* The reference's two GUIs repaint after EVERY analysis: process_audio ends in queue_draw (gui/stereoscope.c:738, gui/phasewheel.c:1339)
 * and the expose handlers paint what that analysis left (stereoscope.c:349-352 under expose_event :439; plot_data_fft, phasewheel.c:571,
 * under expose_event :675) — 25 pictures a second, where mtr_engine_scope_read hands out the last of a call alone.  The series keeps
 * what they would have painted: after every K-th analysis, one POINT per stream — exactly what mtr_engine_scope_read would answer at
 * that moment.  The fields of a point, one bit each (which arrays of the two process_audio it keeps): */
#define MTR_SCOPE_F_LEVEL    1u    /* the stereoscope's smoothed level [B] (stereoscope.c:733) */
#define MTR_SCOPE_F_LR       2u    /* ... and balance [B] (stereoscope.c:734) */
#define MTR_SCOPE_F_PHASE    4u    /* the phase wheel's phase difference of that analysis [B] (phasewheel.c:1322-1326) */
#define MTR_SCOPE_F_PLEVEL   8u    /* ... and its level [B] (phasewheel.c:1323-1327) */
#define MTR_SCOPE_F_PEAK     16u   /* ... and its peak after that analysis' update, one number (phasewheel.c:1333-1335) */
#define MTR_SCOPE_F_POWER_L  32u   /* |X|^2 of that analysis, left [B] (fa->power: ft_analyze, gui/fft.c:175) */
#define MTR_SCOPE_F_POWER_R  64u   /* ... and right (fb->power) */
#define MTR_SCOPE_F_ALL      127u

/* every_analyses 0 (the default): the series is off — no memory held, the kernel of a call is the one without it.  K = 1 .. 2^20: after
 * every K-th analysis counted from create / mtr_engine_reset / mtr_engine_scope_reset, wherever the process calls cut the audio (a
 * lock-step cursor, as the hop is), one point is appended to rings of capacity_points points per stream in engine-owned device memory,
 * one ring per field of `fields` — a non-empty subset of MTR_SCOPE_F_ALL; a field that is not selected costs no memory and no stores
 * (all of them at W = 1024: 12 KB per point and stream).  K = 1 is the reference's queue_draw after every analysis (stereoscope.c:738,
 * phasewheel.c:1339); a larger K is a GUI that paints every K-th of them.  Points past the capacity are counted (dropped), never written;
 * capacity_points 0 is allowed (the counts alone).  Bins 0 and B - 1 of a point hold what mtr_engine_scope_read gives them.
 * MTR_ERR_ARG: no SCOPE in the engine, K > 2^20, K > 0 with fields 0 or with bits outside MTR_SCOPE_F_ALL.  MTR_ERR_STATE: the engine
 * has processed something since create / reset (as mtr_engine_scope_configure).  MTR_ERR_NOMEM: the rings cannot be had, or their size
 * overflows size_t; the series is then off.  mtr_engine_scope_configure keeps K, the capacity and the fields and re-sizes the rings for
 * its window; mtr_engine_reset and mtr_engine_scope_reset empty the series and its counts and forget the open group of K, and keep the
 * settings.  A state blob of an engine with a series carries K and the analyses since the last point (not the points): it goes into an
 * engine of the same K only — fields and capacity need not match — and an engine that has processed must stand at the same analyses
 * since its last point (else MTR_ERR_STATE).  With the series off the blob is byte for byte what it is without this header. */
int  mtr_engine_scope_set_series (mtr_engine* e, uint32_t every_analyses, uint32_t capacity_points, uint32_t fields);
/* what is set (every_analyses 0: off, the other two 0 then); any pointer may be NULL */
int  mtr_engine_scope_series_config (const mtr_engine* e, uint32_t* every_analyses, uint32_t* capacity_points, uint32_t* fields);
/* The points since reset that the rings hold — what stereoscope.c:349-352 and plot_data_fft (phasewheel.c:571) were handed analysis by
 * analysis: level, lr, phase, plevel, power_l, power_r [count][capacity][B], peak [count][capacity]; the first
 * min (*n_points, capacity, capacity_points) points of each stream are copied, the rest of each row is left as it was.  *n_points: points
 * completed since reset, *dropped: those of them past the rings' capacity (lock-step: one number each; either may be NULL).  A pointer may
 * be NULL; a non-NULL pointer for a field that is not selected, or the series off: MTR_ERR_ARG.  Waits for the caller's stream. */
int  mtr_engine_scope_series (mtr_engine* e, uint32_t first, uint32_t count,
                              float* level, float* lr, float* phase, float* plevel, float* peak, float* power_l, float* power_r,
                              uint32_t capacity, uint32_t* n_points, uint32_t* dropped);
/* Host only, no device — how a call cuts the series (the step of a process call uses this same function): a stream that stands `fill`
 * frames behind its last analysis (fftx_run's counter of frames towards the next one, gui/fft.c:289-361) and `since` analyses behind its
 * last point gets n_frames more.  *analyses: the analyses the call completes, (fill + n_frames) / hop; *points: the points it appends,
 * (since + *analyses) / every — 0 with every 0 (the series off; since is not looked at then).
 * MTR_ERR_ARG: fill >= hop, since >= every > 0, hop outside 64 .. 2^20, a NULL pointer. */
int  mtr_scope_series_cut (uint32_t fill, uint32_t hop, uint32_t since, uint32_t every, uint64_t n_frames,
                           uint64_t* analyses, uint64_t* points);

#ifdef __cplusplus
}
#endif

#endif
