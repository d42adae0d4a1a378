/* mtr_internal.h — what more than one TU of libmtr_engine.so needs of the kernels: the arguments and launchers of the fused path (the host side
 * is mtr_call.hip), the stream state, the set-up math.  A side meter's arguments, state and launcher are in the meter's own file, next to
 * its kernels and its host code.  Not installed. */
#ifndef MTR_INTERNAL_H
#define MTR_INTERNAL_H

#include <stdint.h>

#include "mtr_engine.h"

#define MTR_FIR_HALO   47          /* 2*hl - 1 frames of history the 48-tap window needs */
#define MTR_WARM_SEC   0.075f      /* K-filter warm-up for mid-stream segments of the wave-per-segment kernels, in whole tiles (two of ~2500
                                    * frames at 48 kHz: |lambda|^4992 = 1.5e-11; see MTR_SEG_WARM_SEC.  Was 0.2 s = four tiles: 1e-21) */
#ifndef MTR_SEG_WARM_SEC
#define MTR_SEG_WARM_SEC 0.075f    /* the segments of the lane = segment kernel (layout 7): |lambda|^(0.075 fs) = 1.6e-8 of the state a segment
                                    * starts without — under f32's own resolution of it, 6e-8, which 0.0694 s reach (any rate: the slowest
                                    * pole is the 38 Hz high-pass).  Measured: 0.2 -> 0.1 s -2.9 % kernel time, 0.1 -> 0.075 s -0.9 % */
#endif

typedef struct mtr_stream_state mtr_stream_state;
typedef struct mtr_fused_args mtr_fused_args;
typedef struct mtr_gate_args mtr_gate_args;

/* Per-stream persistent state (device). */
struct mtr_stream_state {
	float    kz[8];            /* K-filter states z1..z4, channel-interleaved: z1L z1R z2L z2R ... */
	float    frpwr;            /* partial power of the fragment in progress (Ebu_r128_proc::_frpwr) */
	float    ring[64];         /* _power[], chronological: ring[63] is the newest fragment */
	int32_t  div1, div2;
	float    loud_M, max_M, loud_S, max_S;
	float    integ, integ_thr, rmin, rmax, rthr;
	int32_t  cnt_M, cnt_S, err_M, err_S;
	uint32_t tp_call[2];       /* float bits, atomicMax target of the fused kernel; zero between calls */
	float    tp_last[2];       /* peak of the most recent call (process_max + read) */
	float    tp_hold[2];       /* max since reset */
	float    tpb_z1[2], tpb_z2[2], tpb_m[2], tpb_p[2];   /* TPBALLIST */
};

/* Arguments of the fused K-weighting + true-peak kernel (by value in the kernarg segment). */
struct mtr_fused_args {
	const float*    audio;        /* [S][stride][2] */
	uint64_t        stride;       /* frames */
	const float*    hist;         /* [S][47][2]: the 47 frames before frame 0 of this call */
	const uint32_t* tile_start;   /* [n_tiles + 1] frame offsets; tile j = [start[j], start[j+1]) */
	const uint32_t* seg_tile;     /* [n_segs + 1] first tile of each time segment */
	const float*    scan_m;       /* [6][16] (A^K)^(2^d), row-major, for the wave scan */
	mtr_stream_state* state;      /* [S] */
	float*          tile_power;   /* [S][n_tiles] channel-weighted sum of y^2 over the tile */
	uint32_t        n_streams, n_segs, n_tiles, warm_tiles;
	uint64_t        n_frames;     /* frames per stream in this call (bounds for staging) */
	uint32_t        buf_slots;    /* wave-specialised kernel: 8-byte slots per LDS buffer (multiple of 128) */
	uint32_t        fir_form;     /* 0 = mirror-symmetric form (120 ops/frame), 1 = dense 3 x 48 taps (144) */
	uint32_t        rotate;       /* wave-specialised kernel: rotate the loader / K-filter role over the four waves */
	uint32_t        prune;        /* exact peak pruning: skip the interpolator where L1 * max|x| cannot beat the running peak */
	uint32_t*       prune_stats;  /* [4] tile passes considered / skipped, channel-blocks screened / completed (device counters), may be NULL */
	const uint16_t* mfma_a;       /* layout 6: [12][64][8] hi / lo A fragments of the matrix-pipe interpolator (mtr_mfma16_fir.h) */
	float           a0, a1, a2, b1, b2, c3, c4;
	float           gain_l, gain_r;
	/* per-stream lengths (mtr_engine_process_*_lengths; NULL on every other call, which then launches the dense instantiations):
	 * ends [S] = frames of stream s in this call (<= n_frames; 0: the stream is not touched), from_tile [S] = first tile of the
	 * launch's one segment that stream s covers (0xFFFFFFFF: none; NULL: every tile) — k_seg's peak hand-over, mtr_seg.hip */
	const uint32_t* ends;
	const uint32_t* from_tile;
};

/* Arguments of the lane = time segment kernel (mtr_seg.hip, layout 7).  The launch covers the whole fragments of a call,
 * from `head` frames into it (the rest of a fragment the call started in, k_kwtp16's); every tile is tile_frames long — any
 * length of at least four steps: a tile that is not a multiple of MTR_SEG_STEP ends inside a step.  Segment q of a stream
 * answers for seg_base + (q < seg_rem) consecutive tiles, and every lane processes n_main = seg_base + (seg_rem > 0) of
 * them, starting one tile early where its own segment is the shorter kind. */
#define MTR_SEG_STEP 16            /* frames per lane and step: one column of the block-Toeplitz product */
typedef struct mtr_seg_args {
	const float*    audio;        /* [S][stride][2]: the call's buffer (8-byte aligned: a segment may start on any frame) */
	uint64_t        stride;       /* frames */
	const float*    hist;         /* [S][47][2]: the 47 frames before frame 0 of this call */
	uint32_t        head;         /* frames of this call in front of the launch's first tile (the rest of a fragment the call started in) */
	uint32_t        tile0;        /* ... and how many tiles of the plan they are: tile_power index of the launch's first tile */
	mtr_stream_state* state;      /* [S] */
	float*          tile_power;   /* [S][n_tiles] */
	const uint16_t* mfma_a;       /* [12][64][8] hi / lo A fragments and, behind them, the [3][64][8] core fragments (mtr_mfma16_fir.h) */
	uint32_t        n_streams, n_segs, n_tiles, tile_frames;
	uint32_t        seg_base, seg_rem, n_main;
	uint32_t        warm_steps;   /* K-filter warm-up in front of a segment that does not start the call: steps of 16 frames, multiple of 4 */
	int64_t         p0_end;       /* phase 0 (|x[n - 24]|) of this call covers the frames below n_frames - 24: that frame, counted from the first tile */
	uint32_t        screen;       /* 0: dense.  1: each 16-column chunk gets its first product and the other two only where they may reach the peak (bit for bit the dense peak).
	                               * 2: the same, and a step that completes chunks hands their peaks to the stream's reference at once (the peek: fewer completions, the same bits).
	                               * 3: rule 2 without the lo halves of the f16 split in the step: a completing chunk builds them from the stream's samples (the lazy form:
	                               *    the same chunks, the same bits; a call with `ends` runs form 2)
	                               * 4: form 3 with the screen's product cut to the taps' 32-sample core: three MFMAs per chunk on the three fragments behind
	                               *    mfma_a's twelve, a larger bound (the core form: more chunks complete, the same bits; a call with `ends` runs form 2) */
	uint32_t*       seg_stats;    /* screen: [2] chunks screened / completed (device counters), may be NULL */
	float           a0, a1, a2, b1, b2, c3, c4;
	float           gain_l, gain_r;
	const uint32_t* ends;         /* per-stream lengths, CALL-relative (head included), or NULL: see mtr_fused_args and mtr_seg.hip */
} mtr_seg_args;

/* Arguments of the multichannel K-weighting + true-peak kernel (mtr_kwmc.hip, layout 8: n_channels 3, 4 or 5). */
#define MTR_MAX_CHANNELS 5         /* Ebu_r128_proc::MAXCH, ebumeter/ebu_r128_proc.h:26: what the K-weighting kernels take */
#define MTR_MAX_ENGINE_CHANNELS 8  /* ... and an engine (6 .. 8: MTR_METER_SURROUND alone), k_pick and the frame map: the surround8 plugin's, = MTR_MAX_FRAME_CHANNELS */
#define MTR_KWMC_RUN     20        /* K: frames per lane run (tiles of at most 1280 frames: half a fragment at 48 kHz) */
typedef struct mtr_kwmc_args {
	const float*    audio;        /* [S][stride][C] */
	uint64_t        stride;       /* frames */
	const float*    hist;         /* [S][47][C]: the 47 frames before frame 0 of this call */
	const uint32_t* tile_start;   /* the plan, as mtr_fused_args */
	const uint32_t* seg_tile;
	const float*    scan_m;       /* [6][16] (A^K)^(2^d), the functionals and M^1 .. M^32 for K = MTR_KWMC_RUN */
	float*          kz;           /* [S][C][4] K-filter states z1..z4 per channel */
	uint32_t*       tp_call;      /* [S][C] float bits, atomicMax target; zero between calls */
	float*          tile_power;   /* [S][n_tiles] sum_c gain_c sum y_c^2 over the tile */
	const uint16_t* mfma_a;       /* [12][64][8] hi / lo A fragments (mtr_mfma16_fir.h) */
	uint32_t        n_streams, n_segs, n_tiles, warm_tiles;
	uint64_t        n_frames;
	float           a0, a1, a2, b1, b2, c3, c4;
	float           gain[MTR_MAX_CHANNELS];   /* _chan_gain (ebu_r128_proc.cc:29) */
} mtr_kwmc_args;
#ifdef __cplusplus
/* ... of a call with per-stream lengths (a struct of its own, as mtr_gate_len_args): ends [S] = frames of stream s in this call */
struct mtr_kwmc_len_args : mtr_kwmc_args {
	const uint32_t* ends;
};
#endif

struct mtr_gate_args {
	mtr_stream_state* state;      /* [S] */
	int32_t*        hist;         /* [S][2][751] */
	const float*    tile_power;   /* [S][n_tiles] */
	const uint32_t* frag_tile;    /* [n_frag + 1] first tile of each fragment that ENDS in this call */
	float*          frag_power;   /* [S][n_frag] out (mean power per fragment), may be NULL */
	const float*    bin_power;    /* [100] 10^(j/100) as powf gives it on the host */
	uint32_t        n_streams, n_tiles, n_frag;
	uint32_t        tail_tile;    /* first tile after the last complete fragment (tiles of the open fragment) */
	float           fragm;        /* frames per fragment, as float */
	int32_t         integr;       /* integration on? */
	int32_t*        max_scratch;  /* [S][2] max-hold of M / S as sortable ints, for the multi-workgroup path */
	uint32_t        polite_grid;  /* 0: one workgroup per stream; else at most this many workgroups, each walking several streams (deferred gate) */
	int32_t         fold_tp;      /* 1: fold tp_call into tp_last / tp_hold here (the serial order); 0: k_history has done it (deferred gate) */
};
/* ... of a call with per-stream lengths (a struct of its own: the dense gate's kernel arguments stay as they were):
 * frag_lim [S] = fragments of this call that stream s inserts (<= n_frag), | MTR_GATE_CLOSING if the call closes it (its open
 * fragment is not carried); MTR_GATE_UNTOUCHED: the workgroup leaves the stream as it is, fold included */
#ifdef __cplusplus
struct mtr_gate_len_args : mtr_gate_args {
	const uint32_t* frag_lim;
};
#endif
#define MTR_GATE_CLOSING   0x80000000u
#define MTR_GATE_UNTOUCHED 0xFFFFFFFFu

/* The loudness log (mtr_engine_loudlog_set_period; host side: mtr_loudlog.hip) as a gate sees it — a struct of its own again, behind the
 * gate's arguments in the LOG instantiations only.  Where the streams of the call stand is computed by the host at queue time (a
 * deferred gate runs beside the next call): fragment f of the call is fragment phase + f of the period that was open when the call
 * began, point j = (phase + f + 1) / period - 1 of the call is completed by the fragment with (phase + f + 1) % period == 0 and lands
 * in row [s][point0 + j] if j < room. */
typedef struct mtr_loudlog_args {
	float*          M;            /* [S][cap] series of the view's streams */
	float*          S;
	float*          run;          /* [S][2] MTR_LOUDLOG_MAX: max M / S of the period open between two calls (-inf: no fragment yet) */
	int32_t*        run_new;      /* [S][2] ... and, as sortable ints, of the period the multi-workgroup path leaves open (-inf between calls) */
	uint32_t        period, phase;
	uint32_t        cap, point0, room;   /* row pitch; points every open stream completed before the call (clamped to cap); cap - point0 */
	int32_t         mode;         /* MTR_LOUDLOG_SAMPLE / _MAX */
} mtr_loudlog_args;
#define MTR_LOUDLOG_EMPTY 0x807fffff   /* -inf as a sortable int (mtr_gate.hip): what the series and run_new are cleared to */

/* The integration log (mtr_engine_integlog_set_every; host side: mtr_integlog.hip) as a gate sees it — behind the gate's arguments (and
 * the loudness log's) in the EVAL instantiations only.  Where a stream stands in it is device state: count [s] = evaluations (fragments
 * at which _div2 wrapped while the integration ran) since the log was set or reset, read and advanced by the stream's workgroup, so a
 * deferred gate, a call with lengths or a chunk of a host call needs no host-side cursor.  Evaluation n (1-based) with n % every == 0
 * is point n / every - 1 and lands in v [k][s][n / every - 1] if that is < cap. */
#define MTR_INTEGLOG_FIELDS 5          /* integrated, integ_thr, range_min, range_max, range_thr */
typedef struct mtr_integlog_args {
	float*          v;            /* [5][S_engine][cap] the series, field-major; the view's first stream's row of field 0 */
	uint64_t        field_pitch;  /* floats between two fields: S_engine * cap */
	uint32_t*       count;        /* [S] evaluations of the view's streams */
	uint32_t        every, cap;
} mtr_integlog_args;

/* per-stream state of BITSTATS: shared by mtr_bitstats.hip (the kernel) and mtr_intstat.hip (the meter's host side) */
typedef struct mtr_bitstats_state {
	int32_t hist[MTR_BIM_LAST];      /* src/uris.h:53-60 layout */
	int32_t n_zero, n_pos, n_nan, n_inf, n_den;
	float   vmin, vmax;              /* bim_min (init +inf), bim_max (init 0) */
} mtr_bitstats_state;

typedef struct mtr_tpb_args mtr_tpb_args;
struct mtr_tpb_args {
	const float*    audio;        /* [S][stride][C] */
	uint64_t        stride, n_frames;
	const float*    hist;         /* [S][47][2] */
	const uint16_t* mfma_a;       /* A fragments of the matrix-pipe interpolator (mtr_mfma16_fir.h) */
	mtr_stream_state* state;
	uint32_t        n_streams, n_channels;
	float           w1, w2, w3, g;   /* truepeakdsp.cc:154-157 */
};

#ifdef __cplusplus
extern "C" {
#endif
/* host-side setup math (mtr_setup.c, plain C, no FMA contraction) */
void mtr_setup_kweight (float fsamp, float* out7);
void mtr_setup_fir_table (float* out120);
void mtr_setup_band (double rate, uint32_t band, double* out36);
void mtr_setup_bin_power (float* out100);
void mtr_setup_kweight_matrix (const float* k7, double* A16, double* B4);
void mtr_setup_hist_loudness (const int32_t* hist_M, const int32_t* hist_S, float* integ, float* integ_thr,
                              float* rmin, float* rmax, float* rthr);
size_t mtr_setup_pcm_sample_bytes (int format);
int  mtr_setup_pcm_decode (int format, const void* src, size_t n, float* dst);   /* -1: unknown format */
/* frames of fc samples (format 0 = f32, else MTR_PCM_*) to frames of C floats, channel c = source channel map[c]; -1: bad argument */
int  mtr_setup_pick_decode (int format, const void* src, size_t n_frames, uint32_t fc, const uint8_t* map, uint32_t C, float* dst);
/* one stream's P planes (plane p at src + p * stride samples) to frames of C floats, channel c = plane map[c]; -1: bad argument */
int  mtr_setup_plane_decode (int format, const void* src, size_t n_frames, uint64_t stride, uint32_t P, const uint8_t* map, uint32_t C, float* dst);
void mtr_setup_stcorr (float fsamp, float* out2);   /* w1, w2 of Stcorrdsp::init ((int) fsamp, 2e3f, 0.3f) */
int  mtr_setup_needle (uint32_t kind, float fsamp, float* out4);   /* w1 w2 w3 g of the needle meters' init (VU: w, 4 w, 0, g); -1: unknown kind */
void mtr_setup_scope_window (uint32_t n, float* out);   /* the Hann window of ft_gen_window (gui/fft.c): n floats */
float mtr_setup_needle_gain (float db);             /* Msppmdsp::set_gain: powf (10, .05 * db) */
#ifdef __cplusplus
}

/* kernel launchers (one per HIP TU) */
int  mtr_launch_fused2 (int run, bool ebu, bool tp, const mtr_fused_args& a, uint32_t n_units, void* stream);
int  mtr_launch_kw (int run, const mtr_fused_args& a, uint32_t n_units, void* stream);
int  mtr_launch_kwtp16 (int run, bool ebu, const mtr_fused_args& a, uint32_t n_units, void* stream);
int  mtr_launch_seg (bool ebu, const mtr_seg_args& a, uint32_t n_waves, void* stream);
size_t mtr_seg_lds_bytes (void);
int  mtr_fused2_upload_taps (const float* g144);
/* A trailing `ends` / `frag_lim` (per stream, device memory) selects the instantiation of a call with per-stream lengths; NULL the
 * dense one. */
int  mtr_launch_kwmc (int C, bool ebu, bool tp, const mtr_kwmc_args& a, const uint32_t* ends, uint32_t n_units, void* stream);
/* ... and for a 5-channel engine whose call's buffer holds WAVE 5.1 frames (a.audio: [S][stride][6], L R C LFE Ls Rs;
 * mtr_engine_set_frame_layout with 6, {0, 1, 2, 4, 5} on device f32): the kernel reads the wide frames itself */
int  mtr_launch_kwmc51 (bool ebu, bool tp, const mtr_kwmc_args& a, const uint32_t* ends, uint32_t n_units, void* stream);
/* The interpolator history for the next call, the last step of a call (mtr_history.hip).  Which frames a stream leaves: */
enum HistCut {
	HIST_CALL_END,             /* the frames in front of the call's end, every stream touched: the dense call */
	HIST_CALL_END_IF_TOUCHED,  /* ... of a stream with ends [s] != 0, one that closes included (it keeps what follows its end); ends [s] == 0: its row stays */
	HIST_OWN_END               /* the frames in front of the stream's OWN end, ends [s]; ends [s] == 0: its row stays */
};
/* ... and what a stream's row is: */
enum HistRow {
	HIST_ROW_FIR,              /* [47][HC]: the true-peak interpolator's (MTR_FIR_HALO) */
	HIST_ROW_GONIO             /* OS_HROW floats: [OS_HALO][2], then two words k_history never writes (HC == 2; HIST_CALL_END and HIST_OWN_END only) */
};
/* the goniometer's oversampling (mtr_gonio.hip): frames of input history its 12-tap rows need, and the floats of a stream's history row —
 * [23][2], then the two words of the state blob's header (mtr_gonio_os_hdr), on 16 bytes */
constexpr int OS_HALO = 2 * MTR_GONIO_OS_TAPS - 1, OS_HROW = 48;
static_assert (OS_HROW == 2 * OS_HALO + 2 && OS_HROW % 4 == 0, "OS_HROW: 2 * MTR_GONIO_OS_TAPS - 1 stereo frames and two header words");
struct mtr_history_args {
	const float*    audio;        /* [S][stride][FC] */
	uint64_t        stride, n_frames;
	const float*    hist_in;      /* [S][47][HC] (HIST_ROW_GONIO: [S][OS_HROW]): what the call read */
	float*          hist_out;     /* ... and what the next one reads (the buffers ping-pong: a row that stays is copied across) */
	uint32_t        n_streams;
	const uint32_t* ends;         /* [S] frames of stream s in this call (<= n_frames; 0: untouched, not folded either), NULL: HIST_CALL_END */
	uint32_t        C, FC, HC;    /* channels of the engine (1 .. 5), samples per frame of `audio` (C; 6: WAVE 5.1 frames, C == 5), channels per
	                               * frame of the history (2 for C <= 2 — mono keeps a zero right channel —, else C) */
	mtr_stream_state* fold_state; /* [S] stereo, deferred gate: mtr_fold_truepeak here (NULL: k_gate folds the peaks) */
	uint32_t*       tp_call;      /* layout 8, all [S][C]: mtr_fold_truepeak_mc on these and `state` (NULL: no fold of this kind) */
	float*          tp_last;
	float*          tp_hold;
	mtr_stream_state* state;      /* [S] */
};
/* -1: an ends rule without ends, C outside 1 .. 5, FC neither C nor 6 with C == 5; HIST_ROW_GONIO with HC != 2 or HIST_CALL_END_IF_TOUCHED */
int  mtr_launch_history (HistCut cut, HistRow row, const mtr_history_args& a, void* stream);
/* log != NULL: the instantiations that append the call's points to the loudness log; NULL: the kernels as they are without it.
 * ev != NULL: the EVAL instantiations of k_gate, which evaluate at every recorded wrap of _div2 and append to the integration log —
 * a call of any length then goes through k_gate, one workgroup per stream */
int  mtr_launch_gate (const mtr_gate_args& a, const uint32_t* frag_lim, const mtr_loudlog_args* log, const mtr_integlog_args* ev, void* stream);
int  mtr_launch_delay (uint32_t us, void* stream);
int  mtr_launch_state_init (mtr_stream_state* st, int32_t* hist, uint32_t n_streams, int what, void* stream);
int  mtr_launch_tpb (const mtr_tpb_args& a, void* stream);
/* TPBALLIST with a period (mtr_tpb.h): per (stream, channel) the block that is open between two calls — the running maxima of
 * truepeakdsp.cc:58-84; the states themselves stay in mtr_stream_state, raw.  In front, for the state blob: the engine's period and the
 * frames into the open block (the host's copies rule, export writes them in) */
struct mtr_tpb_open {
	uint32_t period, fill;
	float    zm[2], pk[2];        /* max (z1 + z2) and max |v| of the open block so far */
};
/* what the SERIES instantiations of k_tpb take beside the dense call's arguments (the dense ones' kernarg segment stays as it is) */
struct mtr_tpb_series_args : mtr_tpb_args {
	uint32_t        period;       /* P: 16 .. 8192 */
	uint32_t        fill;         /* frames of the open block in front of the call: 0 = the call starts a block */
	uint32_t        e0;           /* call frame at which the block open on entry ends: P - fill */
	uint32_t        capacity;     /* points per stream the series hold */
	uint32_t        point0, room; /* index of the call's first point; points the series still take, from that one on */
	mtr_tpb_open*   open;         /* [S] */
	float*          s_level;      /* [S][capacity][C], NULL if capacity == 0 */
	float*          s_peak;
};
int  mtr_launch_tpb_series (const mtr_tpb_series_args& a, void* stream);
/* ... and the ENDS instantiations (mtr_engine_process_*_tpb, or any call once a stream of the view is closed): structs of their own again, the
 * existing kernels' arguments stay as they are.  ends [S] = the call frame at which stream s of the view ends (<= n_frames; < n_frames: the call
 * closes it there; 0: untouched) */
struct mtr_tpb_ends_args : mtr_tpb_args {
	const uint32_t* ends;
};
struct mtr_tpb_series_ends_args : mtr_tpb_series_args {
	const uint32_t* ends;
};
int  mtr_launch_tpb_ends (const mtr_tpb_ends_args& a, void* stream);
int  mtr_launch_tpb_series_ends (const mtr_tpb_series_ends_args& a, void* stream);
/* ends != NULL: the LEN instantiation, stream s of the view ends at call frame ends[s] (0: untouched) */
int  mtr_launch_bitstats (const float* audio, uint64_t stride, uint64_t n_frames, mtr_bitstats_state* out,
                          uint32_t n_streams, const uint32_t* ends, void* stream);
int  mtr_launch_aggregate (const mtr_stream_state* st, const int32_t* hist, uint32_t n_streams, int32_t* d_hist, float* d_max, void* stream);
/* The source step (mtr_source.hip): the caller's bytes to rows of n_frames x n_channels f32.  What the source is: */
enum mtr_decode_kind {
	MTR_DECODE_NONE,           /* f32 frames of n_channels: the meters read them where they lie */
	MTR_DECODE_ROWS,           /* k_pcm: rows of n_frames x n_channels packed integer samples (format MTR_PCM_*), `pitch` bytes from row to row */
	MTR_DECODE_FRAMES,         /* k_pick: rows of n_frames frames of `width` samples, channel c = source channel map[c] */
	MTR_DECODE_PLANES          /* k_plane: per row `width` planes of n_frames samples, `pitch` bytes from PLANE to plane (plane p of row r
	                            * at src + (r * width + p) * pitch), channel c = plane map[c] */
};
struct mtr_decode_args {
	mtr_decode_kind kind;
	int             format;       /* 0 = f32 (FRAMES and PLANES only), else MTR_PCM_* */
	const void*     src;
	uint64_t        pitch;        /* bytes */
	uint32_t        width;        /* frame_channels or n_planes; ROWS: not read */
	const uint8_t*  map;          /* [n_channels] entries below width; ROWS: not read */
	uint32_t        n_channels;
	float*          dst;
	uint64_t        dst_pitch;    /* floats */
	uint32_t        n_rows;
	uint64_t        n_frames;
	void*           stream;
};
/* -1: a kind, format, width, channel count or map entry out of range, planes that overlap (pitch < n_frames samples), a launch error */
int  mtr_launch_decode (const mtr_decode_args& a);
int  mtr_launch_synth (float* d_audio, uint32_t n_streams, uint64_t n_frames, uint64_t stride,
                       uint32_t seed, float fs, int kind, void* stream);
#endif

#ifdef __HIPCC__
/* TruePeakdsp::read () as the LV2 glue uses it (src/ebulv2.cc:361-365): the call's peak becomes the value a getter sees and
 * enters the max-hold; tp_call is zero again for the next call's atomicMax.  One lane per stream. */
__device__ __forceinline__ void mtr_fold_truepeak (mtr_stream_state* st)
{
	const float cl = __uint_as_float (st->tp_call[0]), cr = __uint_as_float (st->tp_call[1]);
	st->tp_last[0] = cl; st->tp_last[1] = cr;
	if (cl > st->tp_hold[0]) st->tp_hold[0] = cl;
	if (cr > st->tp_hold[1]) st->tp_hold[1] = cr;
	st->tp_call[0] = 0; st->tp_call[1] = 0;
}
/* ... and per channel for stream s of a multichannel engine (layout 8; tp_call, tp_last, tp_hold: [S][C]); the programme's true peak, the
 * max over the channels, goes to the stream state's two slots — what mtr_engine_results, k_aggregate and the reduction read */
__device__ __forceinline__ void mtr_fold_truepeak_mc (uint32_t* tp_call, float* tp_last, float* tp_hold, mtr_stream_state* st, uint32_t s, uint32_t C)
{
	float last = 0.f, hold = 0.f;
	for (uint32_t c = 0; c < C; ++c) {
		const size_t k = (size_t) s * C + c;
		const float v = __uint_as_float (tp_call[k]);
		tp_last[k] = v;
		if (v > tp_hold[k]) tp_hold[k] = v;
		tp_call[k] = 0;
		last = fmaxf (last, v);
		hold = fmaxf (hold, tp_hold[k]);
	}
	st->tp_last[0] = st->tp_last[1] = last;
	st->tp_hold[0] = st->tp_hold[1] = hold;
	st->tp_call[0] = st->tp_call[1] = 0;
}
#endif

#define MTR_INIT_ALL     0
#define MTR_INIT_INTEGR  1
#define MTR_INIT_TP      2

#endif
