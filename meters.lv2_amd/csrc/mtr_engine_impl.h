// mtr_engine_impl.h — what the host side of libmtr_engine.so shares between its TUs: mtr_engine.hip (create / reset, the tail, the
// EBU / true-peak getters), mtr_call.hip (one process call), mtr_source.hip (the source step and the engine's source layout), mtr_state.hip (the state blob) and the host half of every side meter, which
// lives next to its kernels (mtr_bank.hip, mtr_intstat.hip, mtr_dr14.hip, mtr_kmeter.hip, mtr_stcorr.hip, mtr_needle.hip, mtr_surround.hip, mtr_scope.hip, mtr_tpb.hip, mtr_gonio.hip), and mtr_loudlog.hip (the host
// side of the loudness log, whose points the gate writes).  Not installed; needs the HIP
// runtime header, so the planner (mtr_plan.cpp) never sees it.
#ifndef MTR_ENGINE_IMPL_H
#define MTR_ENGINE_IMPL_H

#include <hip/hip_runtime.h>

#include <vector>

#include "mtr_internal.h"
#include "mtr_host.h"
#include "mtr_series.h"
#include "mtr_km_consts.h"

#pragma GCC visibility push(hidden)   // (cross-TU helpers, not ABI)

// Everything the engine allocates is owned by a member that frees it: mtr_engine_destroy selects the device, waits for it and
// deletes the engine.  None of the owners can be copied.
// PINNED: page-locked host memory (staging of the n_streams = 1 host path, plan uploads, result snapshots)
// (T may be incomplete where the engine is only passed around: sizeof (T) is needed by reserve alone)
template <typename T, bool PINNED> struct Buf {
	T*     p = nullptr;
	size_t n = 0;
	Buf () = default;
	Buf (const Buf&) = delete;
	Buf& operator= (const Buf&) = delete;
	~Buf () { drop (); }
	void drop () { if (p) (void) (PINNED ? hipHostFree (p) : hipFree (p)); p = nullptr; n = 0; }
	int reserve (size_t want) {
		if (want <= n) return 0;
		drop ();
		if ((PINNED ? hipHostMalloc ((void**) &p, want * sizeof (T), hipHostMallocDefault) : hipMalloc ((void**) &p, want * sizeof (T))) != hipSuccess) return -1;
		n = want;
		return 0;
	}
};
template <typename T> using DevBuf = Buf<T, false>;
template <typename T> using PinBuf = Buf<T, true>;

// An event that is created where it is first needed (ensure), so that a path that never needs it — an LV2 run () — never pays for it
struct Event {
	hipEvent_t v = nullptr;
	Event () = default;
	Event (Event&& o) noexcept : v (o.v) { o.v = nullptr; }
	~Event () { if (v) (void) hipEventDestroy (v); }
	hipError_t ensure (unsigned flags = hipEventDisableTiming) { return v ? hipSuccess : hipEventCreateWithFlags (&v, flags); }
};

// ... and a stream of the engine's own, likewise
struct Stream {
	hipStream_t v = nullptr;
	Stream () = default;
	Stream (const Stream&) = delete;
	Stream& operator= (const Stream&) = delete;
	~Stream () { if (v) (void) hipStreamDestroy (v); }
	hipError_t ensure () { return v ? hipSuccess : hipStreamCreateWithFlags (&v, hipStreamNonBlocking); }
};

// The tiling plan of a call lives in one of PLAN_SLOTS device buffers, uploaded from page-locked memory ON THE CALL'S
// STREAM: a call whose (n_frames, fragment phase) differs from the previous one — every call, for 1024-frame blocks at
// 48 kHz — never overwrites arrays that kernels of an earlier call may still be reading, and never blocks the host.
constexpr int PLAN_SLOTS = 4;

// The per-stream arrays of a call with lengths (mtr_engine_process_*_lengths / _tracks / _ragged / _ends, or any call once a stream is closed) ride the same
// way: [ends S | frag_lim S | from_tile S], then the words of every side meter of the engine that has some of its own (SideMeter::ends_words
// per stream, in the order of SIDE_METERS), in the next slot of their own ring, uploaded on the call's stream,
// busy until the call's last readers (the last kernel of the call on its stream — the side meters' LEN kernels, k_history under an ends rule — and the
// gate on whichever stream it ran) have passed.
constexpr int LEN_SLOTS = 4;
struct LenSlot {
	DevBuf<uint32_t> dev;
	PinBuf<uint32_t> pin;
	Event            done[2];
	bool             pending[2] = { false, false };
};
struct PlanSlot {
	DevBuf<uint32_t> dev;       // [tile_start (n_tiles + 1) | seg_tile (n_segs + 1) | frag_tile (n_frag + 1)]
	PinBuf<uint32_t> pin;
	Event            done;             // recorded behind the last kernel that reads `dev`
	bool             pending = false;
};

struct Plan {
	std::vector<uint32_t> frag_end;   // call frame at which fragment f of the call ends (per-stream lengths: fragments that end at or before a stream's end)
	uint64_t n_frames = 0;
	uint32_t frcnt_in = 0;      // frames left in the open fragment when the call starts
	uint32_t frcnt_out = 0;
	uint32_t n_tiles = 0, n_frag = 0, n_segs = 0, tail_tile = 0, buf_slots = 0, kw_slots = 0;
	uint32_t body_tiles = 0;    // whole-fragment tiles (the lane = segment kernel's part of the call), 0 = none
	uint32_t head_tiles = 0;    // ... and the tiles in front of them (the rest of a fragment the call started in)
	bool     valid = false;
};

// The lock-step cursors: where the streams of the engine stand between two process calls.  A call reads them, computes their
// successors as it goes and stores them in ONE place, behind its last launch (CallRun::run) — a chunk of a host call that is
// not the last stores nothing, nor does a call that fails.  That is all the CALL PATH needs of a cursor added here; whose it is — a side
// meter's, as a rule — resets it in its reset hook and, if a state blob has to carry it, puts it into its blob header (struct SideMeter).
struct Cursors {
	uint32_t frcnt = 0;           // frames remaining in the open fragment
	int      hist_cur = 0;        // which of fir_hist [2] / mc_hist [2] holds the 47 frames before the next call
	int      bank_ac_cur = 0;     // ... and which of bank.ac [2] the dither parity
	SeriesPos bk;                 // SPECTR30 with a period: where its reading series stands (mtr_series.h)
	uint64_t dr_scnt = 0;         // samples in the open DR-14 window
	uint32_t km_fpp = 0;          // Kmeterdsp's frames per period and the fall-back factor that goes with it
	float    km_fall = 0.f;
	SeriesPos km;                 // KMETER with a period: where its reading series stands (km_fpp / km_fall are then the period's)
	SeriesPos sc, nd, su;         // STCORR, NEEDLE, SURROUND: where their reading series stand (mtr_series.h)
	uint32_t su_fpp = 0;          // SURROUND: its Kmeterdsps' frames per period with the fall-back factor that goes with it
	float    su_fall = 0.f;
	uint32_t sp_fill = 0;         // SCOPE: frames since the last analysis ...
	uint64_t sp_analyses = 0;     // ... and analyses completed since reset
	uint32_t sp_since = 0;        // SCOPE with a series: analyses since the last point ...
	uint64_t sp_points = 0;       // ... and points completed since reset (what the rings do not hold of them is dropped)
	uint64_t seg_calls = 0, seg_frames = 0;   // calls / frames k_seg took
	uint64_t ll_frags = 0;        // loudness log: fragments the open streams have ended since it was set / reset
	SeriesPos tb;                 // TPBALLIST with a period: where its reading series stands (mtr_series.h)
	SeriesPos go;                 // GONIO: frames into the open display update, updates completed since reset (mtr_series.h)
	int      go_hist_cur = 0;     // GONIO oversampled: which of go.os_hist [2] holds the 23 input frames before the next call
};

// What the buffers of a process call hold (mtr_engine_set_frame_layout, mtr_engine_set_plane_layout: one at a time).  MTR_DECODE_NONE: frames
// of the engine's channels, the default — an explicit identity frame layout is that too; _FRAMES: frames of `width` samples, engine
// channel c = source channel map[c], every chunk through k_pick; _PLANES: `width` planes of one channel per stream, channel c = plane
// map[c], every chunk through k_plane
struct SourceLayout {
	mtr_decode_kind kind = MTR_DECODE_NONE;
	uint32_t        width = 0;
	uint8_t         map[MTR_MAX_ENGINE_CHANNELS] = { 0, 1, 2, 3, 4, 5, 6, 7 };
	bool            wave51 = false;   // frames of 6, {0, 1, 2, 4, 5} on a 5-channel engine: device f32 calls go to k_kwmc51 instead of k_pick
};

// per-stream state of the side meters: defined where their kernels are
struct mtr_sigdist_state;
struct mtr_dr14_state;
struct mtr_kmeter_state;
struct mtr_stcorr_state;
struct mtr_needle_hdr;
struct mtr_sur_state;

// The engine: core, tail, plan rings, host path, then one member per side meter
struct mtr_engine {
	mtr_config cfg;
	int      run = 39;            // K: frames per lane run
	int      layout = 6;          // 3 = exact-f32 VALU interpolator (mtr_fused2.hip), 4 = k_kw, 6 = k_kwtp16 (+ 7: k_seg for the calls it fits), 8 = k_kwmc
	bool     seg_ok = false;      // layout 7: calls that fit go through k_seg (mtr_seg.hip), the rest through k_kwtp16
	uint32_t seg_slots = 1024;    // resident k_seg waves: one per SIMD
	uint32_t fragm = 0;           // frames per 50 ms fragment
	Cursors  pos;
	bool     integr = false;
	bool     advanced = false;    // a process call has run since create / reset: `pos` is no longer a fresh engine's
	float    kw[7];
	hipStream_t last_stream = nullptr;
	bool             queued = false;         // something has been launched on last_stream
	Event            xs_event;               // orders a new stream behind the previous one

	DevBuf<mtr_stream_state> state;
	DevBuf<int32_t>  hist;
	DevBuf<int32_t>  gate_max;      // [S][2] max-hold scratch of the multi-workgroup gate path
	DevBuf<float>    fir_hist[2];   // ping-pong 47-frame history (pos.hist_cur)
	DevBuf<float>    scan_m, bin_power, tile_power[2], frag_power, stage;
	// layout 8 (n_channels 1, 3, 4, 5 with EBU / TRUEPEAK, mtr_kwmc.hip): per-channel side buffers; the stream state's kz / tp_* stay unused
	// by the kernel, its tp_last / tp_hold [0..1] carry the max over the channels (mtr_fold_truepeak_mc in k_history)
	DevBuf<float>    mc_kz;         // [S][C][4]
	DevBuf<float>    mc_hist[2];    // [S][47][C] ping-pong with hist_cur
	DevBuf<uint32_t> mc_tp_call;    // [S][C]
	DevBuf<float>    mc_tp_last, mc_tp_hold;   // [S][C]
	DevBuf<float>    fir_g;         // [3][48] taps in device memory
	DevBuf<uint16_t> m16_a;         // layouts 6, 7: hi / lo A fragments of the f32-grade MFMA interpolator (mtr_mfma16_fir.h)
	DevBuf<uint32_t> prune_cnt;     // [4] interpolator tile passes considered / skipped, channel-blocks screened / completed
	uint64_t         prune_tot[4] = { 0, 0, 0, 0 };
	float            tpb_w[4];      // w1 w2 w3 g of TruePeakdsp::init
	uint32_t         seg_screen = 4;         // k_seg's products screened by the first of the three (mtr_seg.hip: SCREEN): 0 = the dense form, 1 = screened, the stream
	                                         // reference fed by sample peaks until a flush, 2 = screened, completed interpolated peaks fed into it as they are found
	                                         // (the peek), 3 = rule 2 with the lo words of the split built only where a chunk completes
	                                         // (the lazy form; calls with per-stream ends run 2), 4 = form 3 with each chunk screened by the taps' 32-sample
	                                         // core, three MFMAs in place of six (the core form, the default; ends: 2).  MTR_SEG_SCREEN=0 .. 4 selects one
	uint32_t         last_n_frag = 0;
	// Per-stream lengths: frames metered per stream since create / reset, and which streams a call with lengths has closed (a closed
	// stream is left untouched by every later call until mtr_engine_reset; neither is part of the state blob).
	std::vector<uint64_t> metered;
	std::vector<uint8_t>  closed;
	uint32_t         n_closed = 0;

	// The call's tail — k_gate, then the job's reduction (k_aggregate + the RCCL all-reduce) — DEFERRED to an engine-owned side
	// stream: the fused kernel of call i + 1 needs only what the fused kernel and k_history of call i wrote (K-filter state, FIR
	// history), never the gate's bookkeeping, so the tail of call i runs beside it instead of in front of it.  tile_power is
	// double-buffered (the gate of call i reads one while the fused kernel of call i + 1 fills the other); the true-peak fold
	// moves from the gate into k_history on the caller's stream (tp_call is already being raised by call i + 1).  Results are
	// bit for bit those of the serial order: same kernels, same inputs, the fragment inserts in fragment order (gates follow
	// one another on the side stream; ebumeter/ebu_r128_proc.cc:217-244).
	int              tail_mode = 0;          // 0 auto (a k_seg batch of >= TAIL_AUTO_STREAMS streams and >= TAIL_AUTO_FRAMES stream-frames in an EBU / TRUEPEAK engine), 1 never, 2 always
	Stream           tail_stream;
	Event            ev_fused;               // caller's stream -> side: the call's fused kernels are done
	Event            ev_gate[2];             // side -> caller's: the gate that read tile_power[b] is done
	bool             gate_pending[2] = { false, false };
	Event            ev_red;                 // side -> caller's: the reduction that read the peak holds is done (the next fold waits for it)
	bool             red_pending = false;
	Event            ev_main;                // caller's -> side: everything the reduction reads from the caller's stream (the fold) is done
	Event            ev_join;
	bool             tail_pending = false;   // the side stream holds work nobody has waited for yet
	bool             last_deferred = false;  // the most recent process call deferred its tail: mtr_engine_reduce follows it there
	int              tp_cur = 0;             // tile_power buffer of the most recent call
	uint64_t         deferred_calls = 0;
	uint32_t         tail_gate_grid = 512;   // workgroups of a deferred gate: two per CU (set from the device's CU count)
	uint32_t         tail_delay_us = 100;    // see CallRun::gate: the deferred gate must not be dispatched together with the next fused kernel

	// the plan and lengths rings
	PlanSlot         plan_slot[PLAN_SLOTS];
	int              plan_cur = 0;
	const uint32_t*  tile_start = nullptr;   // into plan_slot[plan_cur].dev
	const uint32_t*  seg_tile = nullptr;
	const uint32_t*  frag_tile = nullptr;
	const uint32_t*  head_seg = nullptr;     // {0, first tile of the k_seg body}: the one segment of the k_kwtp16 launch in front of it (if any)
	const uint32_t*  tail_seg = nullptr;     // {first tile behind the k_seg body, n_tiles}: the one segment of the k_kwtp16 launch that finishes such a call
	Plan             plan;
	LenSlot          len_slot[LEN_SLOTS];
	int              len_cur = 0;

	// n_streams = 1 host path (the shape of an LV2 run ()): own stream, page-locked staging, and ONE synchronisation per
	// block — the state (and the bank's levels) come back with the same wait and serve the result getters
	Stream           own_stream;
	PinBuf<float>    pin_in;
	PinBuf<mtr_stream_state> pin_state;
	PinBuf<float>    pin_bank;               // [2][30] val, max
	bool             snap_valid = false;
	// the chunked host path (mtr_engine_process_host)
	size_t           host_chunk_bytes = (size_t) 256 << 20;
	Stream           copy_stream;
	Event            ev_copied[2], ev_computed[2];   // per staging buffer: the chunk has landed / its landing buffer has been read
	// The source step (mtr_source.hip): whatever is not resident f32 frames of n_channels — integer PCM, a frame layout, a plane layout —
	// is decoded chunk by chunk into `stage`, from two raw landing buffers of one chunk each (host memory) or from the caller's rows
	// (device memory)
	DevBuf<uint8_t>  pcm_raw;
	SourceLayout     src;
	uint64_t         pcm_chunks = 0, pcm_bytes = 0;   // integer formats only, whichever kernel decoded them
	uint64_t         lay_staged = 0, lay_direct = 0;  // chunks through k_pick; device calls whose kernels read WAVE 5.1 frames themselves
	uint64_t         plane_staged = 0;                // chunks through k_plane
	std::vector<Event> pcm_ev;      // while timing is on: pairs around the decode kernels not yet summed into pcm_ms
	uint32_t         pcm_timed = 0;
	float            pcm_ms = 0.f;

	bool timing = false;
	std::vector<Event> ev;          // groups of EV_PER_CALL: start, fused end, gate begin, gate end (those two on the stream the gate ran on), rest begin, end; a PCM chunk's start in front of its decode
	std::vector<uint8_t> ev_decode; // per timed call: it began with a decode (its whole span starts at the group's last event, not at the first)
	uint32_t timed_calls = 0;

	// the side meters, each with its host code next to its kernels
	struct Bank {                               // SPECTR30 (mtr_bank.hip)
		DevBuf<double>   coef, z;
		DevBuf<float>    val, max;
		DevBuf<int32_t>  ac[2];                 // ping-pong (pos.bank_ac_cur): k_bank reads one, writes the other
		float            omega = 0.f;
		// the reading series (mtr_engine_spectr_set_period, P > 0): k_bank_series
		SeriesCfg        ser;                   // frames per spectrum_run of the series (0: the call), points per stream it holds
		int              peak_mode = 0;         // MTR_SPECTR_PEAK_*
		DevBuf<float>    s_val, s_max;          // [S][cap][30]
		DevBuf<unsigned char> open;             // [S] mtr_bank_open: the blob's copy of (period, peak mode, frames into the open block)
		std::vector<uint64_t> points;           // [S] points of each stream's own series since reset (mtr_engine_process_*_ends: mtr_ends.h)
	} bank;
	struct IntStat {                            // BITSTATS, SIGDIST (mtr_intstat.hip)
		DevBuf<mtr_bitstats_state> bim;
		DevBuf<mtr_sigdist_state>  sdh;
	} is;
	struct Dr14 {                               // DR14 (mtr_dr14.hip)
		DevBuf<mtr_dr14_state>     state;
		DevBuf<uint32_t>           hist;        // [S][C][8000]
		DevBuf<double>             sum;         // [S][pieces][2]
		DevBuf<float>              peak;
	} dr;
	struct Kmeter {                             // KMETER (mtr_kmeter.hip)
		DevBuf<mtr_kmeter_state>   state;       // [S][2]
		DevBuf<double>             piece;
		DevBuf<float>              max;
		mtr_km_consts              k;           // Kmeterdsp's constants (mtr_km_consts.h), the lane step that of k_kmeter_blocks
		// the reading series (mtr_engine_kmeter_set_period, P > 0): k_kmeter_blocks
		SeriesCfg                  ser;         // frames per process () of the series (0: the call), points per stream it holds
		DevBuf<unsigned char>      open;        // [S] mtr_kmeter_open: the blob's header and the open block's carry per channel
		DevBuf<double>             bpiece;      // [S][pieces][C][MTR_KMB_PIECE]
		DevBuf<float>              s_rms, s_peak;   // [S][cap][C]
		std::vector<uint64_t>      points;      // [S] points of each stream's own series since reset (ragged calls: mtr_ragged.h)
	} km;
	struct Stcorr {                             // STCORR (mtr_stcorr.hip)
		DevBuf<mtr_stcorr_state>   state;       // [S]
		DevBuf<double>             piece;       // [S][pieces][MTR_STCORR_PIECE]
		DevBuf<float>              series;      // [S][cap]
		SeriesCfg                  ser;         // frames per process () of the series (0: the call), points per stream it holds
		float                      w[2];        // w1, w2 of Stcorrdsp::init
		uint32_t                   warm = 0, chunk = 0;   // the pieces' geometry
		std::vector<uint64_t>      points;      // [S] points of each stream's own series since reset (ragged calls: mtr_ragged.h)
	} sc;
	struct Needle {                             // NEEDLE (mtr_needle.hip)
		DevBuf<unsigned char>      state;       // [S] of { mtr_needle_hdr, mtr_needle_state [kinds][C] }
		DevBuf<float>              series;      // [kinds][S][cap][C]
		uint32_t                   kinds = 0;   // MTR_NEEDLE_* selected
		SeriesCfg                  ser;         // frames per process () of the series (0: the call), points per stream and kind
		uint32_t                   kind[4] = { 0, 0, 0, 0 };         // the selected kinds in the order of their bits ...
		float                      w[4][4];     // ... and their w1 w2 w3 g
		float                      db[2], mv[2];   // Msppmdsp's gains, M and S: a control (it survives a reset)
		DevBuf<float>              back;        // [S][kinds][C][2] z1 z2 in front of the group of four frames that is open between two calls
		std::vector<uint64_t>      points;      // [S] points of each stream's own series since reset (ragged calls: mtr_ragged.h)
	} nd;
	struct Surround {                           // SURROUND (mtr_surround.hip)
		DevBuf<mtr_sur_state>      state;       // [S]
		DevBuf<double>             piece;       // [S][pieces][MTR_SUR_PIECE]
		DevBuf<float>              s_level, s_peak, s_corr;   // [S][cap][C], [S][cap][C], [S][cap][4]
		SeriesCfg                  ser;         // frames per sur_run of the series (0: the call), points per stream it holds
		uint8_t                    pa[4] = { 0, 0, 0, 0 }, pb[4] = { 0, 0, 0, 0 };   // the pairs' channels: a control (it survives a reset)
		float                      w[2];        // w1, w2 of Stcorrdsp::init
		mtr_sur_consts             k;           // Kmeterdsp's constants and the pieces kernel's own (mtr_km_consts.h)
		uint32_t                   warm = 0, chunk = 0;   // the pieces' geometry
		std::vector<uint64_t>      points;      // [S] points of each stream's own series since reset (mtr_engine_process_*_any: mtr_any.h)
	} su;
	struct Scope {                              // SCOPE (mtr_scope.hip)
		DevBuf<float>              tail;        // [S][W][2] the last W frames of every stream
		DevBuf<float>              level, lr, phase, plevel, power_l, power_r;   // [S][W / 2]
		DevBuf<float>              peak;        // [S]
		DevBuf<unsigned char>      hdr;         // [S] mtr_scope_hdr: the blob's copy of the configuration and the cursors (written at export)
		DevBuf<float>              win, tw;     // [W] the window, [W][2] the twiddles
		uint32_t                   W = 0, H = 0;   // frames per window and per hop (resolved: never 0): a control (it survives a reset)
		float                      thresh = 0.f;   // the phase wheel's threshold on the powers
		// the reading series (mtr_engine_scope_set_series, K > 0): the SERIES instantiation of k_scope
		struct Series {
			uint32_t               every = 0, cap = 0, fields = 0;   // K (0: off), points per stream a ring holds, MTR_SCOPE_F_*: a control
			DevBuf<float>          ring[7];     // per selected field, in the order of the bits: [S][cap][B]; peak: [S][cap]
			DevBuf<unsigned char>  open;        // [S] mtr_scope_open: the blob's copy of (K, analyses since the last point)
		} ser;
		std::vector<uint64_t>      analyses, points;   // [S] each stream's own analyses and series points since reset (mtr_engine_process_*_any: mtr_any.h)
	} sp;
	struct LoudLog {                            // the loudness log of an EBU engine (mtr_loudlog.hip; the gate appends: mtr_gate.hip)
		DevBuf<float>              M, S;        // [S][cap]
		DevBuf<float>              run;         // [S][2] MAX: maxima of the period open between two calls
		DevBuf<int32_t>            run_new;     // [S][2] ... scratch of the multi-workgroup gate, sortable ints
		uint32_t                   period = 0, cap = 0;   // fragments per point (0: off), points per stream the series holds
		int                        mode = 0;
		std::vector<uint64_t>      points;      // [S] periods each stream has completed (streams end at their own lengths)
	} ll;
	struct IntegLog {                           // the integration log of an EBU engine (mtr_integlog.hip; the gate appends: the EVAL instantiations of mtr_gate.hip)
		DevBuf<float>              v;           // [5][S][cap] integrated, integ_thr, range_min, range_max, range_thr
		DevBuf<uint32_t>           count;       // [S] evaluations of each stream since the log was set / reset: the gate advances it
		uint32_t                   every = 0, cap = 0;   // evaluations per point (0: off), points per stream the series holds
	} il;
	struct Tpb {                                // the reading series of TPBALLIST (mtr_tpb.hip; the meter's states are the stream state's)
		SeriesCfg                  ser;         // frames per process () of the series (0: the call), points per stream it holds
		DevBuf<mtr_tpb_open>       open;        // [S] the blob's header and the open block's maxima per channel
		DevBuf<float>              s_level, s_peak;   // [S][cap][C]
		std::vector<uint64_t>      points;      // [S] points of each stream's own series since reset (mtr_engine_process_*_tpb: mtr_tpb.h)
	} tb;
	struct Gonio {                              // GONIO (mtr_gonio.hip)
		DevBuf<unsigned char>      state;       // [S] of { mtr_gonio_state, uint32 image [G][G] }, `pitch` bytes each
		DevBuf<float>              series;      // [3][S][cap]: gain (f32), drawn, clipped (u32) per display update
		DevBuf<uint16_t>           codes;       // [S][code_pitch] the cell codes of one piece of a call: k_gonio_points writes, k_gonio_image reads
		mtr_gonio_config           cfg;         // resolved: no zeros left
		mtr_gonio_derived          der;
		SeriesCfg                  ser;         // P (never 0), points per stream the series holds
		size_t                     pitch = 0;
		uint32_t                   code_pitch = 0;
		std::vector<Event>         ev;          // while mtr_engine_gonio_timing is on: three per piece, around its two kernels
		bool                       timed = false;
		std::vector<uint64_t>      updates;     // [S] each stream's own display updates since reset, closing ones included (mtr_gonio_ends.h)
		// oversampling (mtr_gonio_os.h): a control (it survives a reset).  Everything below is allocated only with a factor above 1
		uint32_t                   os = 1;      // the factor: 1 (off) or 2 .. 32
		float                      os_hpw = 0.f;   // the hpw the chain runs on with the factor (:175)
		DevBuf<float>              os_tab;      // [os + 1][12] Resampler_table's _ctab
		DevBuf<float>              os_pts;      // [S][os_pitch][2] the points of one piece of a call: k_gonio_os writes, k_gonio_points reads
		DevBuf<float>              os_hist[2];  // [S] rows of 48 floats, ping-pong (pos.go_hist_cur): the last 23 input frames, then the blob's header
		DevBuf<uint32_t>           os_cut;      // [S] a ragged call's cuts as k_gonio_os rebases them to the piece's first point
		uint32_t                   os_pitch = 0;   // points per stream of os_pts: even, so that a row starts on 16 bytes
		std::vector<Event>         os_ev;       // while mtr_engine_gonio_timing is on: two per piece, around k_gonio_os
	} go;
};

constexpr int EV_PER_CALL = 7;

// What a process call is told.  Every entry point (device memory, with or without lengths; each chunk of the host path; an LV2
// block) builds one and hands it to process_call: nothing about a call is parked in the engine between the two.
struct Call {
	const float*    audio;        // device memory, [cnt][stride][C]
	uint64_t        n_frames, stride;
	hipStream_t     st;
	uint32_t        off, cnt;     // the VIEW of the batch the call covers: streams [off, off + cnt); every per-stream array is indexed from off
	const uint64_t* frames;       // per-stream lengths, indexed from the view's first stream, or nullptr
	bool            chunk;        // a chunk of a host call (mtr_engine_process_host walks the batch view by view), not a batch of its own
	bool            commit;       // the lock-step cursors move with this call: the last view of a host call, every other call
	// The source step: the call first decodes the view's rows from dec.src (device memory) into `audio` — a staging buffer of the
	// engine's — and records dec.read (if any) behind that: the source has been read.  The fields are mtr_decode_args' (width: the
	// samples of a source frame — n_channels for _ROWS —, or the planes); the default: no decode
	struct Decode {
		mtr_decode_kind kind = MTR_DECODE_NONE;
		const void*     src = nullptr;
		uint64_t        pitch = 0;
		int             format = 0;
		uint32_t        width = 0;
		hipEvent_t      read = nullptr;
	} dec;
	// ... or `audio` itself holds WAVE 5.1 frames, [cnt][stride][6], which the 5-channel kernels read themselves (k_kwmc51, k_history with FC = 6)
	bool            wave51 = false;
};

// the frames stream i of the view takes of call `c`: its own length or the call's, 0 for a closed stream (every call leaves it untouched)
inline uint64_t call_frames (const mtr_engine* e, const Call& c, uint32_t i)
{
	return e->closed[c.off + i] ? 0 : c.frames ? c.frames[i] : c.n_frames;
}
// the ping-pong histories of the view: flip = 0 what the call reads, 1 what k_history writes for the next one
inline float* fir_hist (const mtr_engine* e, const Call& c, int flip) { return e->fir_hist[e->pos.hist_cur ^ flip].p + (size_t) c.off * MTR_FIR_HALO * 2; }
inline float* mc_hist (const mtr_engine* e, const Call& c, int flip) { return e->mc_hist[e->pos.hist_cur ^ flip].p + (size_t) c.off * MTR_FIR_HALO * e->cfg.n_channels; }

// The per-stream ends of a ragged call on the device, as a side meter's step gets them: ends[i] = the call frame at which stream i of the
// view ends (0: closed, untouched); own = the meter's own words of the call (SideMeter::ends_words per stream, as its ends_fill laid them
// out), null if it has none; note = what that fill returned.  All null / 0 on a dense call: the steps then launch the dense instantiations.
struct StreamEnds {
	const uint32_t* ends = nullptr;
	const uint32_t* own = nullptr;
	uint64_t        note = 0;
};

struct StateSection { const void* base; size_t elem; };   // a per-stream array of the state blob: `elem` bytes per stream

// ---- mtr_engine.hip -------------------------------------------------------------------------------------------------------------
// `st` waits for everything the side stream holds (a serial gate, a reset, the caller's own aggregate behind deferred gates)
int join_tail (mtr_engine* e, hipStream_t st);
// the host waits for the caller's stream and the side stream
int sync_all (mtr_engine* e);
// "null engine" / "stream range out of bounds"
int check_range (mtr_engine* e, uint32_t first, uint32_t count);
// what a side meter's getter begins with: the meter is in the engine (`none` if not) and the streams are ("stream range") ...
int meter_range (const mtr_engine* e, bool has, const char* none, uint32_t first, uint32_t count);
// ... then the engine's device selected and its stream waited for
int wait_stream (mtr_engine* e);

// ---- the reading series on the device (mtr_series.h has the part that needs no device) -----------------------------------------------
// What `who` (an entry point that sets P) refuses: MTR_ERR_ARG unless `period` is 0 or min_period (in words: min_text) .. 2^31 - 2 frames,
// MTR_ERR_STATE on an engine that has processed something since create / reset
int series_configure_check (const mtr_engine* e, const char* who, uint32_t period, uint32_t min_period, const char* min_text);
// a ring of n floats, zeroed (n = 0: nothing); `what`: the text of MTR_ERR_NOMEM
int series_ring (DevBuf<float>& ring, size_t n, const char* what);
// `take` points of `width` floats of each of `count` streams from `first` on: rows of `cap` points at `src` to rows of `capacity` at `out`
int series_fetch (float* out, const float* src, size_t width, uint32_t first, uint32_t cap, uint32_t capacity, size_t take, uint32_t count);

// ---- a side meter as the engine, a call and the state blob see it ------------------------------------------------------------------
// The part of a meter's per-stream entry of the blob that the HOST owns (configuration and cursors: the blob's own header has no room
// for them): `bytes` bytes at `offset` of every stream's entry of the meter's first section, the same in all of them.  mtr_state.hip
// stages, compares and copies the bytes; the hooks give them their meaning.  `h`: `bytes` bytes of a buffer of the host's, aligned for
// any type (write: zeroed), which a hook may read or fill as the struct they are.
struct BlobHeader {
	size_t      offset, bytes;
	const char* corrupt;                                          // MTR_ERR_STATE text: the streams' headers differ
	void (*write) (const mtr_engine* e, void* h);                 // export: the host's copies rule, not whatever the device's entry holds
	int  (*check) (const mtr_engine* e, const void* h, bool fresh);   // import: MTR_ERR_STATE with the text set if `h` is corrupt, not the
	                                                              // engine's configuration or — `fresh` false — not where the engine stands
	void (*take) (mtr_engine* e, const void* h);                  // import into a fresh engine, after the copies succeeded
};
// One row per side meter, in the order of SIDE_METERS: the order of the blob's sections and of a call's steps.  A hook runs only in an
// engine that has one of `bits`.
// A reading series that counts its points per stream (streams end at their own lengths: mtr_ragged.h, mtr_ends.h), as the call path,
// the state import and the points getters see it: P and the capacity, the series' cursor in Cursors, the counts since reset [S]
struct SeriesView {
	const SeriesCfg*       cfg;
	SeriesPos Cursors::*   pos;
	std::vector<uint64_t>* points;
};
struct SideMeter {
	uint32_t    bits;                                             // MTR_METER_*
	uint64_t    max_frames;                                       // a call of this many frames or more is refused (0: no limit of its own) ...
	const char* max_text;                                         // ... with this text
	int  (*create) (mtr_engine* e);                               // create-time set-up, or null
	int  (*reset) (mtr_engine* e);                                // the meter's part of mtr_engine_reset: its state and its cursors in e->pos (where the
	                                                              // meter has a reset of its own in the C ABI, that entry point), or null
	// queues the meter's kernels for the view of call `c` and moves the meter's cursors in `nx` (CallRun::run stores them), or null
	int  (*step) (mtr_engine* e, const Call& c, Cursors& nx, const StreamEnds& se);
	void (*sections) (const mtr_engine* e, std::vector<StateSection>& v);   // appends the arrays a stream carries from call to call
	const BlobHeader* hdr;                                        // in the first of them, or null
	SeriesView (*series) (mtr_engine* e);                         // the meter's reading series, if it counts its points per stream, or null
	// what stream g counts that is no block of a `series`, or null.  With a call: g took `frames` of call *c, which starts at e->pos;
	// c == nullptr: g was imported and takes the lock-step numbers
	void (*count) (mtr_engine* e, size_t g, const Call* c, uint64_t frames);
	// The meter's own per-stream words of a ragged call: ends_words per stream in the lengths ring (0: none), in an engine that holds the
	// meter.  ends_fill writes the ends_words * c.cnt host words of the view at `own` — laid out as the meter likes, read by its step at
	// StreamEnds::own — from call_frames and e->pos, where the CALL started (every chunk of a host call sees the same cuts), and returns
	// one host-side note for that step (StreamEnds::note)
	uint32_t ends_words;
	uint64_t (*ends_fill) (const mtr_engine* e, const Call& c, uint32_t* own);
};
// (Constant-initialised and never written, but not declared const: the device pass of a .hip file would emit a const object of namespace
// scope too, and there the host functions it names do not exist.  Everything reads the rows through SIDE_METERS' pointers to const.)
extern SideMeter bank_meter, intstat_meter, dr14_meter, kmeter_meter, stcorr_meter, needle_meter, surround_meter, scope_meter, kmeter_series_meter,
                 bank_series_meter, scope_series_meter, tpb_meter, gonio_meter, gonio_os_meter;
inline constexpr const SideMeter* SIDE_METERS[] = { &bank_meter, &intstat_meter, &dr14_meter, &kmeter_meter, &stcorr_meter, &needle_meter, &surround_meter, &scope_meter,
                                                    &kmeter_series_meter,     // (KMETER's second row: nothing but the blob section of its open block, behind every older one)
                                                    &bank_series_meter,       // (SPECTR30's second row, likewise)
                                                    &scope_series_meter,      // (SCOPE's second row, likewise)
                                                    &tpb_meter,               // (TPBALLIST: its states are the stream state's; the section is its series' open block)
                                                    &gonio_meter,
                                                    &gonio_os_meter };        // (GONIO's second row: the input history of its oversampling — its kernel, the call's last of
                                                                              // the meter, and its blob section with the factor; nothing at factor 1)
// the points of each of streams [first, first + count) in the series of the meter with `bit`, which the engine holds and which keeps such counts
void series_points_of (mtr_engine* e, uint32_t bit, uint32_t first, uint32_t count, uint64_t* points);
// Stream g's own counts, every meter's of the engine: the points of the reading series (the blocks the stream completed and, closed inside one,
// the truncated block) and what the `count` hooks keep.  With a call: g took `frames` of call *c, which starts at e->pos; c == nullptr:
// g was imported and stands where the open streams do
void stream_counts (mtr_engine* e, size_t g, const Call* c, uint64_t frames);

// Kmeterdsp's fall-back factor for each stream of the view that ends inside call `c`, 0.f for every other, as floats at own [c.cnt]: the
// ends_fill of KMETER and of SURROUND's K-meters, each with its own cursor's fill and its period (mtr_kmeter.hip)
void kmeter_falls (const mtr_engine* e, const Call& c, uint64_t fill, uint64_t P, uint32_t* own);
// the loudness log (no side meter: the gate writes it): what the gate of a call that starts at cursors `pos` appends to, for the view
// [off, off + cnt) (false: the log is off); its part of mtr_engine_reset
bool loudlog_args (const mtr_engine* e, const Cursors& pos, uint32_t off, mtr_loudlog_args* out);
int  loudlog_reset (mtr_engine* e, hipStream_t st);
bool integlog_args (const mtr_engine* e, uint32_t off, mtr_integlog_args* out);
int  integlog_reset (mtr_engine* e, hipStream_t st);

#pragma GCC visibility pop

#endif
