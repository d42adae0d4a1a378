// mtr_engine.hip — host side of libmtr_engine.so: the C ABI of include/mtr_engine.h.
//
// Owns device state for `n_streams` lock-step streams, turns each process call into a tiling
// plan (mtr_plan.cpp: tiles never cross 50 ms fragment boundaries; time segments give the fused kernel enough
// independent waves when the batch is small) and launches the HIP kernels on the caller's
// stream.  There is no CPU fallback anywhere in this file: without a HIP device create() fails.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "mtr_internal.h"
#include "mtr_host.h"
#include "mtr_mfma16_fir.h"

static thread_local std::string g_err;

int fail (int code, const char* what, int hip_error)
{
	char buf[256];
	if (hip_error) snprintf (buf, sizeof (buf), "%s: %s", what, hipGetErrorString ((hipError_t) hip_error));
	else           snprintf (buf, sizeof (buf), "%s", what);
	g_err = buf;
	return code;
}

// Everything the engine allocates is owned by a member that frees it: mtr_engine_destroy selects the device, waits for it and
// deletes the engine.  None of the owners can be copied.
// PINNED: page-locked host memory (staging of the n_streams = 1 host path, plan uploads, result snapshots)
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

// The per-stream arrays of a call with lengths (mtr_engine_process_*_lengths, or any call once a stream is closed) ride the same way:
// [ends S | frag_lim S | from_tile S] in the next slot of their own ring, uploaded on the call's stream, busy until the call's last
// readers (k_history_len on the call's stream, the gate on whichever stream it ran) have passed.
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
// successors as it goes and stores them in ONE place, behind its last launch (process_call) — a chunk of a host call that is
// not the last stores nothing, nor does a call that fails.  A cursor added here needs no other book-keeping.
struct Cursors {
	uint32_t frcnt = 0;           // frames remaining in the open fragment
	int      hist_cur = 0;        // which of fir_hist [2] / mc_hist [2] holds the 47 frames before the next call
	int      bank_ac_cur = 0;     // ... and which of bank_ac [2] the dither parity
	uint64_t dr_scnt = 0;         // samples in the open DR-14 window
	uint32_t km_fpp = 0;          // Kmeterdsp's frames per period and the fall-back factor that goes with it
	float    km_fall = 0.f;
	uint64_t sc_fill = 0;         // STCORR: frames in the open period of the reading series ...
	uint64_t sc_points = 0;       // ... and periods completed since reset
	uint64_t seg_calls = 0, seg_frames = 0;   // calls / frames k_seg took
};

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
	float    omega = 0.f;
	hipStream_t last_stream = nullptr;

	DevBuf<mtr_stream_state> state;
	DevBuf<int32_t>  hist;
	DevBuf<int32_t>  gate_max;      // [S][2] max-hold scratch of the multi-workgroup gate path
	DevBuf<float>    fir_hist[2];   // ping-pong 47-frame history (pos.hist_cur)
	DevBuf<float>    scan_m, bin_power, tile_power[2], frag_power, stage;
	// The call's tail — k_gate, then the job's reduction (k_aggregate + the RCCL all-reduce) — DEFERRED to an engine-owned side
	// stream: the fused kernel of call i + 1 needs only what the fused kernel and k_history of call i wrote (K-filter state, FIR
	// history), never the gate's bookkeeping, so the tail of call i runs beside it instead of in front of it.  tile_power is
	// double-buffered (the gate of call i reads one while the fused kernel of call i + 1 fills the other); the true-peak fold
	// moves from the gate into k_history on the caller's stream (tp_call is already being raised by call i + 1).  Results are
	// bit for bit those of the serial order: same kernels, same inputs, the fragment inserts in fragment order (gates follow
	// one another on the side stream; ebumeter/ebu_r128_proc.cc:217-244).
	bool             seg_screen = true;      // k_seg's products screened by the first of the three (mtr_seg.hip: SCREEN); MTR_SEG_SCREEN=0 forces the dense form
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
	uint32_t         tail_delay_us = 100;    // see process_device: the deferred gate must not be dispatched together with the next fused kernel
	PlanSlot         plan_slot[PLAN_SLOTS];
	int              plan_cur = 0;
	const uint32_t*  tile_start = nullptr;   // into plan_slot[plan_cur].dev
	const uint32_t*  seg_tile = nullptr;
	const uint32_t*  frag_tile = nullptr;
	const uint32_t*  head_seg = nullptr;     // {0, first tile of the k_seg body}: the one segment of the k_kwtp16 launch in front of it (if any)
	const uint32_t*  tail_seg = nullptr;     // {first tile behind the k_seg body, n_tiles}: the one segment of the k_kwtp16 launch that finishes such a call
	// n_streams = 1 host path (the shape of an LV2 run ()): own stream, page-locked staging, and ONE synchronisation per
	// block — the state (and the bank's levels) come back with the same wait and serve the result getters
	Stream           own_stream;
	PinBuf<float>    pin_in;
	PinBuf<mtr_stream_state> pin_state;
	PinBuf<float>    pin_bank;               // [2][30] val, max
	bool             snap_valid = false;
	bool             queued = false;         // something has been launched on last_stream
	Event            xs_event;               // orders a new stream behind the previous one
	DevBuf<double>   bank_coef, bank_z;
	DevBuf<float>    bank_val, bank_max;
	DevBuf<int32_t>  bank_ac[2];     // ping-pong (pos.bank_ac_cur): k_bank reads one, writes the other
	DevBuf<mtr_bitstats_state> bim;
	DevBuf<mtr_sigdist_state>  sdh;
	DevBuf<mtr_dr14_state>     dr_state;
	DevBuf<uint32_t>           dr_hist;       // [S][C][8000]
	DevBuf<double>             dr_sum;        // [S][pieces][2]
	DevBuf<float>              dr_peak;
	DevBuf<mtr_kmeter_state>   km_state;      // [S][2]
	DevBuf<double>             km_piece;
	DevBuf<float>              km_max;
	double                     km_pw1[3];
	DevBuf<mtr_stcorr_state>   sc_state;      // [S]
	DevBuf<double>             sc_piece;      // [S][pieces][MTR_STCORR_PIECE]
	DevBuf<float>              sc_series;     // [S][sc_cap]
	uint32_t                   sc_period = 0, sc_cap = 0;   // frames per process () of the series (0: the call), points per stream it holds
	float                      sc_w[2];       // w1, w2 of Stcorrdsp::init
	uint32_t                   sc_warm = 0, sc_chunk = 0;   // mtr_stcorr_geometry
	// layout 8 (n_channels 1, 3, 4, 5 with EBU / TRUEPEAK, mtr_kwmc.hip): per-channel side buffers; the stream state's kz / tp_* stay unused
	// by the kernel, its tp_last / tp_hold [0..1] carry the max over the channels (k_history_mc)
	DevBuf<float>    mc_kz;         // [S][C][4]
	DevBuf<float>    mc_hist[2];    // [S][47][C] ping-pong with hist_cur
	DevBuf<uint32_t> mc_tp_call;    // [S][C]
	DevBuf<float>    mc_tp_last, mc_tp_hold;   // [S][C]
	DevBuf<float>    fir_g;         // [3][48] taps in device memory
	DevBuf<uint16_t> m16_a;         // layouts 6, 7: hi / lo A fragments of the f32-grade MFMA interpolator (mtr_mfma16_fir.h)
	DevBuf<uint32_t> prune_cnt;     // [4] interpolator tile passes considered / skipped, channel-blocks screened / completed
	uint64_t         prune_tot[4] = { 0, 0, 0, 0 };
	float            tpb_w[4];      // w1 w2 w3 g of TruePeakdsp::init
	Plan             plan;
	uint32_t         last_n_frag = 0;
	// Per-stream lengths: frames metered per stream since create / reset, and which streams a call with lengths has closed (a closed
	// stream is left untouched by every later call until mtr_engine_reset; neither is part of the state blob).
	std::vector<uint64_t> metered;
	std::vector<uint8_t>  closed;
	uint32_t         n_closed = 0;
	LenSlot          len_slot[LEN_SLOTS];
	int              len_cur = 0;

	// the chunked host path (mtr_engine_process_host)
	size_t           host_chunk_bytes = (size_t) 256 << 20;
	Stream           copy_stream;
	Event            ev_copied[2], ev_computed[2];   // per staging buffer: the chunk has landed / its landing buffer has been read
	// integer PCM in (mtr_engine_process_*_pcm): the host form's integer rows land in two raw buffers of one chunk each, k_pcm
	// (mtr_pcm.hip) decodes a chunk from there — or from the caller's device rows — into `stage`
	DevBuf<uint8_t>  pcm_raw;
	uint64_t         pcm_chunks = 0, pcm_bytes = 0;
	std::vector<Event> pcm_ev;      // while timing is on: pairs around the decode kernels not yet summed into pcm_ms
	uint32_t         pcm_timed = 0;
	float            pcm_ms = 0.f;
	// frame layout (mtr_engine_set_frame_layout): the buffers of a process call hold frames of frame_channels samples, engine channel c
	// is source channel frame_map[c]; 0 = the default.  `picks`: the layout is not the identity, every chunk goes through k_pick
	// (mtr_pick.hip) — from the raw landing buffers (host memory) or the caller's rows (device memory) into `stage`
	uint32_t         frame_channels = 0;
	uint8_t          frame_map[MTR_MAX_CHANNELS] = { 0, 1, 2, 3, 4 };
	bool             picks = false;
	bool             wave51 = false;      // ... and it is 6, {0, 1, 2, 4, 5} on a 5-channel engine: device f32 calls go to k_kwmc51 instead
	uint64_t         lay_staged = 0, lay_direct = 0;

	bool timing = false;
	std::vector<Event> ev;          // groups of EV_PER_CALL: start, fused end, gate begin, gate end (those two on the stream the gate ran on), rest begin, end; a PCM chunk's start in front of its decode
	std::vector<uint8_t> ev_decode; // per timed call: it began with a decode (its whole span starts at the group's last event, not at the first)
	uint32_t timed_calls = 0;
};

constexpr int EV_PER_CALL = 7;
constexpr uint32_t TAIL_AUTO_STREAMS = 4096;       // ... and streams per call
constexpr uint64_t TAIL_AUTO_FRAMES = 1ull << 24;   // stream-frames per call (134 MB of stereo f32: ~40 us of the fused kernel) from which the tail is deferred

static void mat4_mul (const double* a, const double* b, double* c)
{
	double t[16];
	for (int i = 0; i < 4; ++i)
		for (int j = 0; j < 4; ++j) {
			double s = 0;
			for (int k = 0; k < 4; ++k) s += a[i * 4 + k] * b[k * 4 + j];
			t[i * 4 + j] = s;
		}
	memcpy (c, t, sizeof (t));
}

static int upload_consts (mtr_engine* e)
{
	// (A^K)^(2^d), d = 0..5, in double, rounded once to float
	double A[16], B[4], P[16];
	mtr_setup_kweight_matrix (e->kw, A, B);
	for (int i = 0; i < 16; ++i) P[i] = (i % 5 == 0) ? 1.0 : 0.0;
	for (int i = 0; i < e->run; ++i) mat4_mul (A, P, P);
	const int K = e->run;
	std::vector<float> m (96 + 4 * K + 4 + 32 * 16);
	{
		// M^1 .. M^32 (M = A^K) for the row-broadcast steps of the DPP scan (mtr_wave.h), after the functionals
		double Q[16];
		memcpy (Q, P, sizeof (Q));
		for (int p = 0; p < 32; ++p) {
			for (int i = 0; i < 16; ++i) m[96 + 4 * K + 4 + 16 * p + i] = (float) Q[i];
			mat4_mul (P, Q, Q);
		}
	}
	for (int d = 0; d < 6; ++d) {
		for (int i = 0; i < 16; ++i) m[d * 16 + i] = (float) P[i];
		mat4_mul (P, P, P);
	}
	// end-state functionals of a K-frame run from zero state: F[n] = A^(K-1-n) B, n = 0..K-1, and the
	// constant response to the +1e-15f bias, e0 = (sum_n A^(K-1-n) B) * 1e-15
	{
		double v[4] = { B[0], B[1], B[2], B[3] }, acc[4] = { 0, 0, 0, 0 };
		for (int n = K - 1; n >= 0; --n) {
			for (int j = 0; j < 4; ++j) { m[96 + 4 * n + j] = (float) v[j]; acc[j] += v[j]; }
			double w[4];
			for (int i = 0; i < 4; ++i) w[i] = A[i * 4] * v[0] + A[i * 4 + 1] * v[1] + A[i * 4 + 2] * v[2] + A[i * 4 + 3] * v[3];
			memcpy (v, w, sizeof (v));
		}
		for (int j = 0; j < 4; ++j) m[96 + 4 * K + j] = (float) (acc[j] * (double) 1e-15f);
	}
	if (e->scan_m.reserve (m.size ())) return fail (MTR_ERR_NOMEM, "hipMalloc scan_m");
	HIPCHK (hipMemcpy (e->scan_m.p, m.data (), m.size () * sizeof (float), hipMemcpyHostToDevice));

	float bp[100];
	mtr_setup_bin_power (bp);
	if (e->bin_power.reserve (100)) return fail (MTR_ERR_NOMEM, "hipMalloc bin_power");
	HIPCHK (hipMemcpy (e->bin_power.p, bp, sizeof (bp), hipMemcpyHostToDevice));

	// 48-tap kernels of phases 1..3 from the 5x24 table (resampler.cc:216-227)
	float tab[120], g[3][48];
	mtr_setup_fir_table (tab);
	for (int ph = 1; ph <= 3; ++ph)
		for (int i = 0; i < 48; ++i)
			g[ph - 1][i] = (i < 24) ? tab[24 * ph + i] : tab[24 * (4 - ph) + (47 - i)];
	if (mtr_fused2_upload_taps (&g[0][0])) return fail (MTR_ERR_HIP, "hipMemcpyToSymbol c_fir");
	if (e->fir_g.reserve (144) || e->prune_cnt.reserve (4)) return fail (MTR_ERR_NOMEM, "hipMalloc fir_g");
	HIPCHK (hipMemset (e->prune_cnt.p, 0, 16));
	HIPCHK (hipMemcpy (e->fir_g.p, g, sizeof (g), hipMemcpyHostToDevice));
	{
		// and as A fragments of the matrix-pipe interpolator
		std::vector<uint16_t> a16 (MTR_M16_A_HALVES);
		mtr_m16_build_a (&g[0][0], a16.data ());
		if (e->m16_a.reserve (a16.size ())) return fail (MTR_ERR_NOMEM, "hipMalloc m16_a");
		HIPCHK (hipMemcpy (e->m16_a.p, a16.data (), a16.size () * sizeof (uint16_t), hipMemcpyHostToDevice));
	}
	// TruePeakdsp::init, jmeters/truepeakdsp.cc:154-157 — float / float / double, stored as float
	const float fs = e->cfg.sample_rate;
	e->tpb_w[0] = 4000.0f / fs / 4.0;
	e->tpb_w[1] = 17200.0f / fs / 4.0;
	e->tpb_w[2] = 1.0f - 7.0f / fs / 4.0;
	e->tpb_w[3] = 0.502f;
	return MTR_OK;
}

// `st` waits for everything the side stream holds (a serial gate, a reset, the caller's own aggregate behind deferred gates)
static int join_tail (mtr_engine* e, hipStream_t st)
{
	if (!e->tail_pending || !e->tail_stream.v) return MTR_OK;
	HIPCHK (e->ev_join.ensure ());
	HIPCHK (hipEventRecord (e->ev_join.v, e->tail_stream.v));
	HIPCHK (hipStreamWaitEvent (st, e->ev_join.v, 0));
	// (only the engine's own stream carries the later calls and the host's waits: a join onto any other stream settles nothing for them)
	if (st == e->last_stream) { e->tail_pending = false; e->gate_pending[0] = e->gate_pending[1] = false; e->red_pending = false; }
	return MTR_OK;
}

// the host waits for the caller's stream and the side stream
static int sync_all (mtr_engine* e)
{
	HIPCHK (hipStreamSynchronize (e->last_stream));
	if (e->tail_stream.v && e->tail_pending) {
		HIPCHK (hipStreamSynchronize (e->tail_stream.v));
		e->tail_pending = false; e->gate_pending[0] = e->gate_pending[1] = false; e->red_pending = false;
	}
	return MTR_OK;
}

static int tail_setup (mtr_engine* e)
{
	if (e->tail_stream.v) return MTR_OK;
	HIPCHK (e->tail_stream.ensure ());
	for (Event* v : { &e->ev_fused, &e->ev_gate[0], &e->ev_gate[1], &e->ev_red, &e->ev_main }) HIPCHK (v->ensure ());
	return MTR_OK;
}

static int state_init (mtr_engine* e, int what, hipStream_t st)
{
	{ const int jrc = join_tail (e, st); if (jrc) return jrc; }       // (a deferred gate may still be writing what this clears)
	e->queued = true;                // (work on last_stream: a caller that moves to another stream must be ordered behind it)
	if (mtr_launch_state_init (e->state.p, e->hist.p, e->cfg.n_streams, what, st)) return fail (MTR_ERR_HIP, "k_state_init");
	return MTR_OK;
}

// the per-channel true-peak arrays of layout 8 (TruePeakdsp::reset per channel)
static int mc_tp_clear (mtr_engine* e, hipStream_t st)
{
	HIPCHK (hipMemsetAsync (e->mc_tp_call.p, 0, e->mc_tp_call.n * sizeof (uint32_t), st));
	HIPCHK (hipMemsetAsync (e->mc_tp_last.p, 0, e->mc_tp_last.n * sizeof (float), st));
	HIPCHK (hipMemsetAsync (e->mc_tp_hold.p, 0, e->mc_tp_hold.n * sizeof (float), st));
	return MTR_OK;
}

extern "C" {

const char* mtr_last_error (void) { return g_err.c_str (); }
// A library built with MTR_TIMING_ONLY_BUILD may carry kernels with a role switched off (tools/: elimination runs that price a
// part of a kernel — WRONG RESULTS by construction): it says so here, and meters.lv2_amd/engine.py refuses to load it outside tools/.
#ifdef MTR_TIMING_ONLY_BUILD
const char* mtr_version (void) { return "meters.lv2_amd 0.1 (gfx950) TIMING-ONLY BUILD: results are wrong by construction"; }
#else
const char* mtr_version (void) { return "meters.lv2_amd 0.1 (gfx950)"; }
#endif
int mtr_abi_version (void) { return MTR_ABI_VERSION; }

int mtr_kweight_coef (float sample_rate, float* out7)
{
	if (!out7 || !(sample_rate > 0)) return fail (MTR_ERR_ARG, "mtr_kweight_coef");
	mtr_setup_kweight (sample_rate, out7);
	return MTR_OK;
}

int mtr_fir_table (float* out120)
{
	if (!out120) return fail (MTR_ERR_ARG, "mtr_fir_table");
	mtr_setup_fir_table (out120);
	return MTR_OK;
}

int mtr_band_coef (double rate, uint32_t band, double* out36)
{
	if (!out36 || band >= MTR_NBANDS || !(rate > 0)) return fail (MTR_ERR_ARG, "mtr_band_coef");
	mtr_setup_band (rate, band, out36);
	return MTR_OK;
}

void mtr_hist_loudness (const int32_t* hm, const int32_t* hs, float* integ, float* integ_thr,
                        float* rmin, float* rmax, float* rthr)
{
	float d[5];
	mtr_setup_hist_loudness (hm, hs, &d[0], &d[1], &d[2], &d[3], &d[4]);
	if (integ) *integ = d[0];
	if (integ_thr) *integ_thr = d[1];
	if (rmin) *rmin = d[2];
	if (rmax) *rmax = d[3];
	if (rthr) *rthr = d[4];
}


int mtr_engine_create (const mtr_config* cfg, mtr_engine** out)
{
	if (!cfg || !out || cfg->struct_size != sizeof (mtr_config)) return fail (MTR_ERR_ARG, "mtr_engine_create: bad config");
	*out = nullptr;
	if (cfg->n_streams == 0 || !(cfg->sample_rate >= 8000.f) || cfg->meters == 0) return fail (MTR_ERR_ARG, "mtr_engine_create: n_streams / sample_rate / meters");
	if (cfg->n_channels < 1 || cfg->n_channels > MTR_MAX_CHANNELS) return fail (MTR_ERR_ARG, "n_channels must be 1 .. 5");
	if (cfg->meters & ~(uint32_t) (MTR_METER_EBU | MTR_METER_TRUEPEAK | MTR_METER_SPECTR30 | MTR_METER_TPBALLIST | MTR_METER_BITSTATS
	                               | MTR_METER_SIGDIST | MTR_METER_DR14 | MTR_METER_KMETER | MTR_METER_STCORR))
		return fail (MTR_ERR_ARG, "unknown bits in the meters mask");
	if (cfg->n_channels == 1 && (cfg->meters & (MTR_METER_EBU | MTR_METER_TRUEPEAK)))
		return fail (MTR_ERR_UNSUPPORTED, "EBU / TRUEPEAK take 2 .. 5 channels, not mono");
	if (cfg->n_channels == 1 && (cfg->meters & MTR_METER_STCORR))
		return fail (MTR_ERR_UNSUPPORTED, "STCORR is the correlation of a stereo pair: n_channels 2");
	// 3 .. 5 channels: EBU R128 and true peak only (Ebu_r128_proc::init takes up to five, ebumeter/ebu_r128_proc.h:26)
	if (cfg->n_channels > 2 && (cfg->meters & ~(uint32_t) (MTR_METER_EBU | MTR_METER_TRUEPEAK)))
		return fail (MTR_ERR_UNSUPPORTED, "3 .. 5 channels: only EBU and TRUEPEAK meter them");
	if ((cfg->meters & (MTR_METER_BITSTATS | MTR_METER_SIGDIST)) && cfg->n_channels != 1)
		return fail (MTR_ERR_UNSUPPORTED, "BITSTATS / SIGDIST take mono streams (the reference's bitmeter / SigDistHist are mono plugins)");
	{
		int l_, r_; bool k_;
		if (const char* why = resolve_layout (cfg, &l_, &r_, &k_)) return fail (MTR_ERR_ARG, why);
	}

	int ndev = 0;
	if (hipGetDeviceCount (&ndev) != hipSuccess || ndev <= 0)
		return fail (MTR_ERR_NODEVICE, "no HIP device: the engine has no CPU path");
	if (cfg->device < 0 || cfg->device >= ndev) return fail (MTR_ERR_ARG, "device ordinal out of range");
	HIPCHK (hipSetDevice (cfg->device));

	mtr_engine* e = new (std::nothrow) mtr_engine ();
	if (!e) return fail (MTR_ERR_NOMEM, "new mtr_engine");
	e->cfg = *cfg;
	// layout 4 = k_kw, the K-weighting-only kernel (mtr_kw.hip): the default when no true peak is asked for;
	// layout 6 = k_kwtp16 (mtr_fused4.hip): wherever a true peak is asked for — the interpolator on the matrix pipe at f32
	//            grade, one wave per (stream, time segment);
	// layout 7 (the default with a true peak) = layout 6 plus k_seg (mtr_seg.hip, lane = time segment) for every call that
	//            fits it: a big batch that starts on a fragment boundary (seg_plan below);
	// layout 3 = the exact-f32 VALU interpolator (mtr_fused2.hip), kept as the bit-for-bit cross-check of the matrix-pipe paths.
	{
		const char* why = resolve_layout (cfg, &e->layout, &e->run, &e->seg_ok);
		if (why) { delete e; return fail (MTR_ERR_ARG, why); }
	}
	{
		hipDeviceProp_t pr;
		if (hipGetDeviceProperties (&pr, cfg->device) == hipSuccess && pr.multiProcessorCount > 0) { e->seg_slots = 4u * (uint32_t) pr.multiProcessorCount; e->tail_gate_grid = 2u * (uint32_t) pr.multiProcessorCount; }
	}
	// (test knobs: the whole -m gpu suite and the fuzzers run green with MTR_TAIL_MODE=2 — every call of every test with its tail on the side stream)
	if (const char* v = getenv ("MTR_TAIL_MODE")) { const int m = atoi (v); if (m >= 0 && m <= 2) e->tail_mode = m; }
	if (const char* v = getenv ("MTR_SEG_SCREEN")) e->seg_screen = atoi (v) != 0;   // (test knob: 0 = k_seg's dense form, the screened one's bit-for-bit yardstick)
	if (const char* v = getenv ("MTR_TAIL_DELAY_US")) e->tail_delay_us = (uint32_t) atoi (v);
	if (const char* v = getenv ("MTR_TAIL_GATE_GRID")) e->tail_gate_grid = (uint32_t) atoi (v);   // (tools/r06_tail_probe.py: the experiment behind the default)
	e->fragm = (uint32_t) ((int) cfg->sample_rate / 20);     // ebu_r128_proc.cc:170
	e->pos.frcnt = e->fragm;
	mtr_setup_kweight (cfg->sample_rate, e->kw);
	e->omega = 1.0f - expf (-2.0 * M_PI * 1.0 / (double) cfg->sample_rate);   // spectrumlv2.c:98
	mtr_setup_stcorr (cfg->sample_rate, e->sc_w);
	mtr_stcorr_geometry (e->sc_w[0], &e->sc_warm, &e->sc_chunk);

	const uint32_t S = cfg->n_streams;
	int rc = MTR_OK;
	if (e->state.reserve (S) || e->hist.reserve ((size_t) S * 2 * MTR_HIST_LEN)
	    || e->fir_hist[0].reserve ((size_t) S * MTR_FIR_HALO * 2) || e->fir_hist[1].reserve ((size_t) S * MTR_FIR_HALO * 2))
		rc = fail (MTR_ERR_NOMEM, "hipMalloc stream state");
	if (rc == MTR_OK) rc = upload_consts (e);
	if (rc == MTR_OK && e->layout == 8) {
		const size_t C = cfg->n_channels;
		if (e->mc_kz.reserve ((size_t) S * C * 4) || e->mc_hist[0].reserve ((size_t) S * MTR_FIR_HALO * C) || e->mc_hist[1].reserve ((size_t) S * MTR_FIR_HALO * C)
		    || e->mc_tp_call.reserve ((size_t) S * C) || e->mc_tp_last.reserve ((size_t) S * C) || e->mc_tp_hold.reserve ((size_t) S * C))
			rc = fail (MTR_ERR_NOMEM, "hipMalloc multichannel state");
	}
	if (rc == MTR_OK) {
		// max-hold scratch of the multi-workgroup gate: "minus infinity" as a sortable int (mtr_gate.hip)
		std::vector<int32_t> m ((size_t) S * 2, (int32_t) 0x807fffff);
		if (e->gate_max.reserve (m.size ())) rc = fail (MTR_ERR_NOMEM, "hipMalloc gate scratch");
		else if (hipMemcpy (e->gate_max.p, m.data (), m.size () * 4, hipMemcpyHostToDevice) != hipSuccess) rc = fail (MTR_ERR_HIP, "hipMemcpy gate scratch");
	}
	if (rc == MTR_OK && (cfg->meters & MTR_METER_SPECTR30)) {
		std::vector<double> c (MTR_NBANDS * 6 * 5);
		for (uint32_t b = 0; b < MTR_NBANDS; ++b) {
			double w[36];
			mtr_setup_band ((double) cfg->sample_rate, b, w);
			for (int i = 0; i < 6; ++i) {
				double* o = &c[(b * 6 + i) * 5];
				o[0] = w[i * 6 + 3]; o[1] = w[i * 6 + 4]; o[2] = w[i * 6 + 5];   // b0 b1 b2
				o[3] = w[i * 6 + 1]; o[4] = w[i * 6 + 2];                         // a1 a2
			}
		}
		if (e->bank_coef.reserve (c.size ()) || e->bank_z.reserve ((size_t) S * MTR_NBANDS * 12)
		    || e->bank_val.reserve ((size_t) S * MTR_NBANDS) || e->bank_max.reserve ((size_t) S * MTR_NBANDS)
		    || e->bank_ac[0].reserve (S) || e->bank_ac[1].reserve (S))
			rc = fail (MTR_ERR_NOMEM, "hipMalloc bank state");
		else if (hipMemcpy (e->bank_coef.p, c.data (), c.size () * sizeof (double), hipMemcpyHostToDevice) != hipSuccess)
			rc = fail (MTR_ERR_HIP, "hipMemcpy bank_coef");
	}
	if (rc != MTR_OK) { mtr_engine_destroy (e); return rc; }
	rc = mtr_engine_reset (e);
	if (rc != MTR_OK) { mtr_engine_destroy (e); return rc; }     // never an error code together with a live handle
	*out = e;
	return MTR_OK;
}

void mtr_engine_destroy (mtr_engine* e)
{
	if (!e) return;
	(void) hipSetDevice (e->cfg.device);        // (in front of the members' destructors: they free on the current device)
	(void) hipDeviceSynchronize ();
	delete e;
}

int mtr_engine_reset (mtr_engine* e)
{
	if (!e) return fail (MTR_ERR_ARG, "null engine");
	e->snap_valid = false;
	HIPCHK (hipSetDevice (e->cfg.device));
	hipStream_t st = e->last_stream;
	int rc = state_init (e, MTR_INIT_ALL, st);
	if (rc) return rc;
	const size_t hb = (size_t) e->cfg.n_streams * MTR_FIR_HALO * 2 * sizeof (float);
	HIPCHK (hipMemsetAsync (e->fir_hist[0].p, 0, hb, st));
	HIPCHK (hipMemsetAsync (e->fir_hist[1].p, 0, hb, st));
	if (e->layout == 8) {
		HIPCHK (hipMemsetAsync (e->mc_kz.p, 0, e->mc_kz.n * sizeof (float), st));
		HIPCHK (hipMemsetAsync (e->mc_hist[0].p, 0, e->mc_hist[0].n * sizeof (float), st));
		HIPCHK (hipMemsetAsync (e->mc_hist[1].p, 0, e->mc_hist[1].n * sizeof (float), st));
		const int trc = mc_tp_clear (e, st);
		if (trc) return trc;
	}
	if (e->cfg.meters & MTR_METER_SPECTR30) {
		HIPCHK (hipMemsetAsync (e->bank_z.p, 0, e->bank_z.n * sizeof (double), st));
		HIPCHK (hipMemsetAsync (e->bank_val.p, 0, e->bank_val.n * sizeof (float), st));
		HIPCHK (hipMemsetAsync (e->bank_max.p, 0, e->bank_max.n * sizeof (float), st));
		HIPCHK (hipMemsetAsync (e->bank_ac[0].p, 0, e->bank_ac[0].n * sizeof (int32_t), st));
		HIPCHK (hipMemsetAsync (e->bank_ac[1].p, 0, e->bank_ac[1].n * sizeof (int32_t), st));
		e->pos.bank_ac_cur = 0;
	}
	e->pos.frcnt = e->fragm;
	e->integr = false;
	e->advanced = false;
	e->metered.assign (e->cfg.n_streams, 0);                         // (every stream open again)
	e->closed.assign (e->cfg.n_streams, 0);
	e->n_closed = 0;
	e->pos.hist_cur = 0;
	e->last_n_frag = 0;
	e->last_deferred = false;
	if (e->cfg.meters & MTR_METER_DR14) { const int drc = mtr_engine_dr14_reset (e); if (drc) return drc; }
	if (e->cfg.meters & MTR_METER_KMETER) { const int krc = mtr_engine_kmeter_reset (e); if (krc) return krc; e->pos.km_fpp = 0; e->pos.km_fall = 0.f; }
	if (e->cfg.meters & MTR_METER_STCORR) { const int src = mtr_engine_stcorr_reset (e); if (src) return src; }
	if (e->cfg.meters & (MTR_METER_BITSTATS | MTR_METER_SIGDIST)) return mtr_engine_intstat_reset (e);
	return MTR_OK;
}

int mtr_stcorr_coef (float sample_rate, float* out2)
{
	if (!out2 || !(sample_rate >= 1.f)) return fail (MTR_ERR_ARG, "mtr_stcorr_coef");
	mtr_setup_stcorr (sample_rate, out2);
	return MTR_OK;
}

static int no_stcorr (const mtr_engine* e) { return !e || !(e->cfg.meters & MTR_METER_STCORR); }

int mtr_engine_stcorr_reset (mtr_engine* e)
{
	if (no_stcorr (e)) return fail (MTR_ERR_ARG, "no STCORR in this engine");
	e->snap_valid = false;
	HIPCHK (hipSetDevice (e->cfg.device));
	const uint32_t S = e->cfg.n_streams;
	if (e->sc_state.reserve (S)) return fail (MTR_ERR_NOMEM, "hipMalloc STCORR state");
	std::vector<mtr_stcorr_state> h (S);
	memset (h.data (), 0, S * sizeof (mtr_stcorr_state));          // stcorrdsp.cc:33-36
	for (auto& v : h) v.period = e->sc_period;
	HIPCHK (hipStreamSynchronize (e->last_stream));
	HIPCHK (hipMemcpy (e->sc_state.p, h.data (), S * sizeof (mtr_stcorr_state), hipMemcpyHostToDevice));
	e->pos.sc_fill = 0;
	e->pos.sc_points = 0;
	return MTR_OK;
}

int mtr_engine_stcorr_set_period (mtr_engine* e, uint32_t period_frames, uint32_t capacity_points)
{
	if (no_stcorr (e)) return fail (MTR_ERR_ARG, "no STCORR in this engine");
	if (period_frames && (period_frames < (uint32_t) e->cfg.sample_rate / 20 || period_frames >= 0x7fffffffu))
		return fail (MTR_ERR_ARG, "mtr_engine_stcorr_set_period: a period is 0 or at least (uint32_t) sample_rate / 20 frames");
	if (e->advanced) return fail (MTR_ERR_STATE, "mtr_engine_stcorr_set_period: only on an engine that has processed nothing since create / reset");
	HIPCHK (hipSetDevice (e->cfg.device));
	HIPCHK (hipStreamSynchronize (e->last_stream));
	const size_t n = (size_t) e->cfg.n_streams * capacity_points;
	if (n && e->sc_series.reserve (n)) return fail (MTR_ERR_NOMEM, "hipMalloc STCORR series");
	if (n) HIPCHK (hipMemset (e->sc_series.p, 0, n * sizeof (float)));
	e->sc_period = period_frames;
	e->sc_cap = capacity_points;
	return mtr_engine_stcorr_reset (e);
}

int mtr_engine_stcorr_read (mtr_engine* e, uint32_t first, uint32_t count, float* corr, float* state5)
{
	if (no_stcorr (e) || !corr) return fail (MTR_ERR_ARG, "no STCORR in this engine");
	if ((uint64_t) first + count > e->cfg.n_streams) return fail (MTR_ERR_ARG, "stream range");
	HIPCHK (hipSetDevice (e->cfg.device));
	HIPCHK (hipStreamSynchronize (e->last_stream));
	std::vector<mtr_stcorr_state> h (count);
	if (count) HIPCHK (hipMemcpy (h.data (), e->sc_state.p + first, count * sizeof (mtr_stcorr_state), hipMemcpyDeviceToHost));
	for (uint32_t i = 0; i < count; ++i) {
		corr[i] = h[i].corr;
		if (state5) memcpy (state5 + (size_t) i * 5, h[i].z, sizeof (h[i].z));
	}
	return MTR_OK;
}

int mtr_engine_stcorr_series (mtr_engine* e, uint32_t first, uint32_t count, float* out, uint32_t capacity, uint32_t* n_points, uint32_t* dropped)
{
	if (no_stcorr (e)) return fail (MTR_ERR_ARG, "no STCORR in this engine");
	if ((uint64_t) first + count > e->cfg.n_streams) return fail (MTR_ERR_ARG, "stream range");
	const uint64_t n = e->pos.sc_points, kept = std::min<uint64_t> (n, e->sc_cap);
	if (n_points) *n_points = (uint32_t) std::min<uint64_t> (n, 0xFFFFFFFFull);
	if (dropped) *dropped = (uint32_t) std::min<uint64_t> (n - kept, 0xFFFFFFFFull);
	const size_t take = (size_t) std::min<uint64_t> (kept, capacity);
	if (!out || !count || !take) return MTR_OK;
	HIPCHK (hipSetDevice (e->cfg.device));
	HIPCHK (hipStreamSynchronize (e->last_stream));
	HIPCHK (hipMemcpy2D (out, (size_t) capacity * sizeof (float), e->sc_series.p + (size_t) first * e->sc_cap, (size_t) e->sc_cap * sizeof (float),
	                     take * sizeof (float), count, hipMemcpyDeviceToHost));
	return MTR_OK;
}

int mtr_engine_kmeter_reset (mtr_engine* e)
{
	if (!e || !(e->cfg.meters & MTR_METER_KMETER)) return fail (MTR_ERR_ARG, "no KMETER in this engine");
	e->snap_valid = false;
	HIPCHK (hipSetDevice (e->cfg.device));
	const size_t n = (size_t) e->cfg.n_streams * 2;
	if (e->km_state.reserve (n)) return fail (MTR_ERR_NOMEM, "hipMalloc KMETER state");
	mtr_kmeter_powers (9.72f / e->cfg.sample_rate, e->km_pw1);           // kmeterdsp.cc:52
	HIPCHK (hipStreamSynchronize (e->last_stream));
	HIPCHK (hipMemset (e->km_state.p, 0, n * sizeof (mtr_kmeter_state)));   // :142-146
	return MTR_OK;
}

int mtr_engine_kmeter_read (mtr_engine* e, uint32_t first, uint32_t count, float* rms, float* peak)
{
	if (!e || !rms || !peak || !(e->cfg.meters & MTR_METER_KMETER)) return fail (MTR_ERR_ARG, "no KMETER in this engine");
	if ((uint64_t) first + count > e->cfg.n_streams) return fail (MTR_ERR_ARG, "stream range");
	HIPCHK (hipSetDevice (e->cfg.device));
	HIPCHK (hipStreamSynchronize (e->last_stream));
	std::vector<mtr_kmeter_state> h ((size_t) count * 2);
	HIPCHK (hipMemcpy (h.data (), e->km_state.p + (size_t) first * 2, h.size () * sizeof (mtr_kmeter_state), hipMemcpyDeviceToHost));
	for (size_t i = 0; i < h.size (); ++i) { rms[i] = h[i].rms; peak[i] = h[i].peak; h[i].flag = 1; }
	HIPCHK (hipMemcpy (e->km_state.p + (size_t) first * 2, h.data (), h.size () * sizeof (mtr_kmeter_state), hipMemcpyHostToDevice));
	return MTR_OK;
}

int mtr_engine_dr14_reset (mtr_engine* e)
{
	if (!e || !(e->cfg.meters & MTR_METER_DR14)) return fail (MTR_ERR_ARG, "no DR14 in this engine");
	e->snap_valid = false;
	HIPCHK (hipSetDevice (e->cfg.device));
	const uint32_t S = e->cfg.n_streams;
	if (e->dr_state.reserve (S) || e->dr_hist.reserve ((size_t) S * e->cfg.n_channels * MTR_DR_HISTBINS))
		return fail (MTR_ERR_NOMEM, "hipMalloc DR14 state");
	std::vector<mtr_dr14_state> h (S);
	memset (h.data (), 0, S * sizeof (mtr_dr14_state));
	for (auto& v : h) for (int c = 0; c < 2; ++c) { v.m_rms[c] = -81.f; v.m_peak[c] = -81.f; }   // dr14.c:247-248
	HIPCHK (hipStreamSynchronize (e->last_stream));
	HIPCHK (hipMemcpy (e->dr_state.p, h.data (), S * sizeof (mtr_dr14_state), hipMemcpyHostToDevice));
	HIPCHK (hipMemset (e->dr_hist.p, 0, (size_t) S * e->cfg.n_channels * MTR_DR_HISTBINS * sizeof (uint32_t)));
	e->pos.dr_scnt = 0;
	return MTR_OK;
}

int mtr_engine_dr14_results (mtr_engine* e, uint32_t first, uint32_t count, mtr_dr14_result* out)
{
	if (!e || !out || !(e->cfg.meters & MTR_METER_DR14)) return fail (MTR_ERR_ARG, "no DR14 in this engine");
	if ((uint64_t) first + count > e->cfg.n_streams) return fail (MTR_ERR_ARG, "stream range");
	HIPCHK (hipSetDevice (e->cfg.device));
	HIPCHK (hipStreamSynchronize (e->last_stream));
	std::vector<mtr_dr14_state> h (count);
	HIPCHK (hipMemcpy (h.data (), e->dr_state.p + first, count * sizeof (mtr_dr14_state), hipMemcpyDeviceToHost));
	const int C = (int) e->cfg.n_channels;
	for (uint32_t i = 0; i < count; ++i) {
		mtr_dr14_result& r = out[i];
		memset (&r, 0, sizeof (r));
		float total = 0.f;
		int valid = 0;
		for (int c = 0; c < C; ++c) {                          // dr14.c:430-441
			const float rdb = h[i].m_rms[c], pdb = h[i].m_peak[c];
			const float dr = (0.f < pdb ? 0.f : pdb) - rdb;
			const bool ok = rdb > -80.f && pdb > -80.f;
			if (ok) { total += dr; ++valid; }
			const float cl = 20.f < dr ? 20.f : dr;
			r.dr[c] = ok ? (1.f > cl ? 1.f : cl) : 21.f;
			r.m_rms[c] = rdb; r.m_peak[c] = pdb;
		}
		if (C > 1) {                                           // :443-450
			if (valid > 0) { const float m = total / (float) valid; const float cl = 20.f < m ? 20.f : m; r.dr_total = 1.f > cl ? 1.f : cl; }
			else r.dr_total = 21.f;
		}
		r.block_count = 3.0f * (float) h[i].num_fragments;
	}
	return MTR_OK;
}

int mtr_engine_intstat_reset (mtr_engine* e)
{
	if (!e) return fail (MTR_ERR_ARG, "null engine");
	e->snap_valid = false;
	HIPCHK (hipSetDevice (e->cfg.device));
	const uint32_t S = e->cfg.n_streams;
	HIPCHK (hipStreamSynchronize (e->last_stream));
	if (e->cfg.meters & MTR_METER_BITSTATS) {
		std::vector<mtr_bitstats_state> h (S);
		memset (h.data (), 0, S * sizeof (mtr_bitstats_state));
		for (auto& b : h) { b.vmin = INFINITY; b.vmax = 0; }          // bim_clear, src/bitmeter.c:47-55
		if (e->bim.reserve (S)) return fail (MTR_ERR_NOMEM, "hipMalloc bitstats state");
		HIPCHK (hipMemcpy (e->bim.p, h.data (), S * sizeof (mtr_bitstats_state), hipMemcpyHostToDevice));
	}
	if (e->cfg.meters & MTR_METER_SIGDIST) {
		if (e->sdh.reserve (S)) return fail (MTR_ERR_NOMEM, "hipMalloc sigdist state");
		std::vector<mtr_sigdist_state> h (S);
		memset (h.data (), 0, S * sizeof (mtr_sigdist_state));
		for (auto& d : h) d.peak_bin = -1;                            // sdh_reset, src/sigdistlv2.c:54: no peak yet
		HIPCHK (hipMemcpy (e->sdh.p, h.data (), S * sizeof (mtr_sigdist_state), hipMemcpyHostToDevice));
	}
	return MTR_OK;
}

int mtr_engine_bitstats (mtr_engine* e, uint32_t first, uint32_t count, int32_t* hist, int32_t* counters, float* minmax)
{
	if (!e || !(e->cfg.meters & MTR_METER_BITSTATS)) return fail (MTR_ERR_ARG, "no BITSTATS in this engine");
	if ((uint64_t) first + count > e->cfg.n_streams) return fail (MTR_ERR_ARG, "stream range out of bounds");
	if (count == 0) return MTR_OK;
	int rc = mtr_engine_sync (e);
	if (rc) return rc;
	std::vector<mtr_bitstats_state> h (count);
	HIPCHK (hipMemcpy (h.data (), e->bim.p + first, count * sizeof (mtr_bitstats_state), hipMemcpyDeviceToHost));
	for (uint32_t i = 0; i < count; ++i) {
		if (hist) memcpy (hist + (size_t) i * MTR_BIM_LAST, h[i].hist, sizeof (h[i].hist));
		if (counters) { int32_t* c = counters + (size_t) i * 5; c[0] = h[i].n_zero; c[1] = h[i].n_pos; c[2] = h[i].n_nan; c[3] = h[i].n_inf; c[4] = h[i].n_den; }
		if (minmax) { minmax[2 * i] = h[i].vmin; minmax[2 * i + 1] = h[i].vmax; }
	}
	return MTR_OK;
}

int mtr_engine_sigdist (mtr_engine* e, uint32_t first, uint32_t count, int32_t* bins, int32_t* peak, double* moments, int64_t* n)
{
	if (!e || !(e->cfg.meters & MTR_METER_SIGDIST)) return fail (MTR_ERR_ARG, "no SIGDIST in this engine");
	if ((uint64_t) first + count > e->cfg.n_streams) return fail (MTR_ERR_ARG, "stream range out of bounds");
	if (count == 0) return MTR_OK;
	int rc = mtr_engine_sync (e);
	if (rc) return rc;
	std::vector<mtr_sigdist_state> h (count);
	HIPCHK (hipMemcpy (h.data (), e->sdh.p + first, count * sizeof (mtr_sigdist_state), hipMemcpyDeviceToHost));
	for (uint32_t i = 0; i < count; ++i) {
		if (bins) memcpy (bins + (size_t) i * MTR_DIST_BIN, h[i].bins, sizeof (h[i].bins));
		if (peak) { peak[2 * i] = h[i].peak_cnt; peak[2 * i + 1] = h[i].peak_bin; }
		if (moments) { moments[3 * i] = h[i].avg; moments[3 * i + 1] = h[i].var_m; moments[3 * i + 2] = h[i].var_s; }
		if (n) n[i] = h[i].count;
	}
	return MTR_OK;
}

int mtr_engine_integr_start (mtr_engine* e) { if (!e) return fail (MTR_ERR_ARG, "null engine"); e->integr = true;  return MTR_OK; }
int mtr_engine_integr_pause (mtr_engine* e) { if (!e) return fail (MTR_ERR_ARG, "null engine"); e->integr = false; return MTR_OK; }
int mtr_engine_integr_reset (mtr_engine* e)
{
	if (!e) return fail (MTR_ERR_ARG, "null engine");
	e->snap_valid = false;
	HIPCHK (hipSetDevice (e->cfg.device));
	return state_init (e, MTR_INIT_INTEGR, e->last_stream);
}
int mtr_engine_truepeak_reset (mtr_engine* e)
{
	if (!e) return fail (MTR_ERR_ARG, "null engine");
	e->snap_valid = false;
	HIPCHK (hipSetDevice (e->cfg.device));
	const int rc = state_init (e, MTR_INIT_TP, e->last_stream);
	if (rc || e->layout != 8) return rc;
	return mc_tp_clear (e, e->last_stream);
}

int mtr_engine_spectr_set_speed (mtr_engine* e, float v)
{
	if (!e) return fail (MTR_ERR_ARG, "null engine");
	if (v < 0.01) v = 0.01;                                    // spectrumlv2.c:172-175
	if (v > 15.0) v = 15.0;
	e->omega = 1.0f - expf (-2.0 * M_PI * v / (double) e->cfg.sample_rate);
	return MTR_OK;
}

int mtr_engine_spectr_reset_peak (mtr_engine* e)
{
	if (!e || !(e->cfg.meters & MTR_METER_SPECTR30)) return fail (MTR_ERR_ARG, "no SPECTR30 in this engine");
	e->snap_valid = false;
	HIPCHK (hipSetDevice (e->cfg.device));
	HIPCHK (hipMemsetAsync (e->bank_max.p, 0, e->bank_max.n * sizeof (float), e->last_stream));
	e->queued = true;
	return MTR_OK;
}

} // extern "C"

static PlanCtx plan_ctx (const mtr_engine* e)
{
	return { e->cfg, e->seg_ok, e->layout, e->run, e->fragm, e->pos.frcnt, e->seg_slots };
}

// A launch behind build_plan's upload failed: the slot stays busy until the stream has passed this point, the plan is not reused.
static void plan_abort (mtr_engine* e, hipStream_t st)
{
	PlanSlot& ps = e->plan_slot[e->plan_cur];
	if (ps.done.v && hipEventRecord (ps.done.v, st) == hipSuccess) ps.pending = true;
	e->plan.valid = false;
}

// The plan of a call on the device: its tiling (mtr_plan.cpp) in the next slot of the plan ring.
static int build_plan (mtr_engine* e, uint64_t N, uint32_t head, uint32_t body_tiles, hipStream_t st)
{
	Plan& pl = e->plan;
	if (pl.valid && pl.n_frames == N && pl.frcnt_in == e->pos.frcnt && pl.body_tiles == body_tiles) return MTR_OK;
	pl.valid = false;
	const PlanCtx ctx = plan_ctx (e);
	Tiling til;
	if (const char* why = plan_tiling (&ctx, N, head, body_tiles, til)) return fail (MTR_ERR_ARG, why);
	const std::vector<uint32_t>& ts = til.ts;
	const std::vector<uint32_t>& ft = til.ft;
	const std::vector<uint32_t>& sg = til.sg;
	const uint32_t n_tiles = til.n_tiles, n_frag = til.n_frag, tail = til.tail, head_tiles = til.head_tiles, n_segs = til.n_segs, left = til.frcnt_out;

	// (with head-room: an LV2 host's blocks see a fragment end in some calls and none in others, and a buffer that grows
	// by one word then is a hipMalloc — 0.3 ms — in the audio thread)
	// (a buffer that grows is freed first, and hipFree waits for the device: no deferred gate still reads it)
	if (e->tile_power[0].reserve ((size_t) e->cfg.n_streams * std::max<uint32_t> (n_tiles, 16))
	    || e->tile_power[1].reserve ((size_t) e->cfg.n_streams * std::max<uint32_t> (n_tiles, 16))
	    || e->frag_power.reserve ((size_t) e->cfg.n_streams * std::max<uint32_t> (n_frag, 16)))
		return fail (MTR_ERR_NOMEM, "hipMalloc plan buffers");
	// the next slot of the ring; its previous contents were last read PLAN_SLOTS plans ago
	const int slot = (e->plan_cur + 1) % PLAN_SLOTS;
	PlanSlot& ps = e->plan_slot[slot];
	if (ps.pending) { HIPCHK (hipEventSynchronize (ps.done.v)); ps.pending = false; }
	const uint32_t tseg[4] = { 0, head_tiles, head_tiles + body_tiles, n_tiles };
	const size_t words = ts.size () + sg.size () + ft.size () + 4;
	if (ps.dev.reserve (std::max<size_t> (words, 256)) || ps.pin.reserve (std::max<size_t> (words, 256))) return fail (MTR_ERR_NOMEM, "plan slot");
	HIPCHK (ps.done.ensure ());
	memcpy (ps.pin.p, ts.data (), ts.size () * 4);
	memcpy (ps.pin.p + ts.size (), sg.data (), sg.size () * 4);
	memcpy (ps.pin.p + ts.size () + sg.size (), ft.data (), ft.size () * 4);
	memcpy (ps.pin.p + ts.size () + sg.size () + ft.size (), tseg, 16);
	HIPCHK (hipMemcpyAsync (ps.dev.p, ps.pin.p, words * 4, hipMemcpyHostToDevice, st));
	// (the slot is busy from here on: its `done` event is recorded behind the plan's last reader, k_gate — or by plan_abort ()
	// if a launch behind this copy fails, so that the slot is never handed out again under a pending upload: ADVICE r2.
	// One hipEventRecord per call, not two: it is 2-3 us of an LV2 run ().)
	e->plan_cur = slot;
	e->tile_start = ps.dev.p; e->seg_tile = ps.dev.p + ts.size (); e->frag_tile = ps.dev.p + ts.size () + sg.size ();
	e->head_seg = e->frag_tile + ft.size ();
	e->tail_seg = e->head_seg + 2;

	pl.frag_end.resize (n_frag);
	for (uint32_t f = 0; f < n_frag; ++f) pl.frag_end[f] = ts[ft[f + 1]];
	pl.n_frames = N; pl.frcnt_in = e->pos.frcnt; pl.frcnt_out = left;
	pl.n_tiles = n_tiles; pl.n_frag = n_frag; pl.n_segs = n_segs; pl.tail_tile = tail; pl.body_tiles = body_tiles; pl.head_tiles = head_tiles;
	const uint32_t maxlen = til.maxlen;
	// + look-ahead frames of the FIR register tile + 4 slots for the carried K-filter state (layout 3)
	pl.buf_slots = (maxlen + 48 + 13 + 4 + 127) / 128 * 128;
	pl.kw_slots = (maxlen + 1 + 127) / 128 * 128;               // k_kw: the tile + one frame of alignment slack
	pl.valid = true;
	return MTR_OK;
}

static hipEvent_t next_event (std::vector<Event>& ev, size_t idx)
{
	while (ev.size () <= idx) {
		Event v;
		if (v.ensure (hipEventDefault) != hipSuccess) return nullptr;
		ev.push_back (std::move (v));
	}
	return ev[idx].v;
}
static hipEvent_t next_event (mtr_engine* e, size_t idx) { return next_event (e->ev, idx); }

// ---- one process call -------------------------------------------------------------------------------------------------------

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
	// integer PCM: the call first decodes the view's rows from `pcm` (device memory, row pitch in bytes) into `audio` — a staging buffer
	// of the engine's — with k_pcm, and records `pcm_read` (if any) behind that: the integer rows have been read
	const void*     pcm = nullptr;
	uint64_t        pcm_pitch = 0;
	int             pcm_format = 0;
	hipEvent_t      pcm_read = nullptr;
	// frame layout: the rows at `pcm` (format 0: f32) hold frames of pick_fc samples, k_pick decodes and picks them (0: k_pcm on frames of C)
	uint32_t        pick_fc = 0;
	// ... or `audio` itself holds WAVE 5.1 frames, [cnt][stride][6], which the 5-channel kernels read themselves (k_kwmc51, k_history_mc51)
	bool            wave51 = false;
};

// Where a call goes (pure apart from reading the engine)
struct Route {
	bool    ragged = false;       // per-stream lengths: the LEN instantiations of the kernels; every other call the dense ones
	bool    defer = false;        // the tail (k_gate; the job's reduction if mtr_engine_reduce follows) on the side stream
	SegPlan sp;                   // the whole fragments through k_seg?
};

// K-weighting coefficients and channel gains (_chan_gain, ebu_r128_proc.cc:29: L R C Ls Rs) of a fused kernel's arguments
constexpr float CHAN_GAIN[MTR_MAX_CHANNELS] = { 1.0f, 1.0f, 1.0f, 1.41f, 1.41f };
template <typename A> static void set_kweight (const mtr_engine* e, A& a)
{
	a.a0 = e->kw[0]; a.a1 = e->kw[1]; a.a2 = e->kw[2]; a.b1 = e->kw[3]; a.b2 = e->kw[4]; a.c3 = e->kw[5]; a.c4 = e->kw[6];
	if constexpr (requires { a.gain_l; }) { a.gain_l = CHAN_GAIN[0]; a.gain_r = CHAN_GAIN[1]; }
	else for (int c = 0; c < MTR_MAX_CHANNELS; ++c) a.gain[c] = CHAN_GAIN[c];
}

// every per-meter limit is checked before anything is launched or any host-side state moves
static int check_limits (const mtr_engine* e, uint64_t n_frames)
{
	if ((e->cfg.meters & (MTR_METER_BITSTATS | MTR_METER_SIGDIST)) && n_frames >= 0x7fffffffull)
		return fail (MTR_ERR_ARG, "BITSTATS / SIGDIST: n_frames per call must be < 2^31 - 1");
	if ((e->cfg.meters & MTR_METER_KMETER) && n_frames >= 0x7fffffffull)
		return fail (MTR_ERR_ARG, "KMETER: n_frames per call must be < 2^31 - 1 (the reference's int n)");
	if ((e->cfg.meters & MTR_METER_STCORR) && n_frames >= 0x7fffffffull)
		return fail (MTR_ERR_ARG, "STCORR: n_frames per call must be < 2^31 - 1 (the reference's int n)");
	if ((e->cfg.meters & MTR_METER_TPBALLIST) && n_frames >= 0x7ffff000ull)
		return fail (MTR_ERR_ARG, "TPBALLIST: n_frames per call must be < 2^31 - 4096");
	if ((e->cfg.meters & (MTR_METER_EBU | MTR_METER_TRUEPEAK)) && n_frames >= 0xFFFFFFFFull)
		return fail (MTR_ERR_ARG, "n_frames per call must be < 2^32 - 1");
	return MTR_OK;
}

// the call's stream becomes the engine's: a caller that moved to another one is ordered behind what the previous one still has to do
static int enter_stream (mtr_engine* e, hipStream_t st)
{
	if (st != e->last_stream && e->queued) {
		HIPCHK (e->xs_event.ensure ());
		HIPCHK (hipEventRecord (e->xs_event.v, e->last_stream));
		HIPCHK (hipStreamWaitEvent (st, e->xs_event.v, 0));
	}
	e->last_stream = st;
	e->queued = true;
	e->snap_valid = false;
	e->advanced = true;
	return MTR_OK;
}

// One call in progress: what its steps share, and the steps in the order of the launches
struct CallRun {
	mtr_engine* const e;
	const Call&  c;
	const Plan&  pl = e->plan;
	const bool   ebu = e->cfg.meters & MTR_METER_EBU, tp = e->cfg.meters & MTR_METER_TRUEPEAK;
	const bool   tm = e->timing && e->timed_calls < 4096;             // this call is timed ...
	const size_t ev0 = (size_t) e->timed_calls * EV_PER_CALL;         // ... with the events from here
	Route        r;
	Cursors      nx = e->pos;          // the cursors behind this call: computed as it goes, stored by its commit
	// the per-stream arrays of a ragged call on the device (null otherwise: the launchers then take the dense instantiation)
	const uint32_t* d_ends = nullptr;
	const uint32_t* d_lim = nullptr;
	const uint32_t* d_from = nullptr;
	bool         any_from = false;     // k_seg left a closing stream's last peaks to k_kwtp16
	LenSlot*     ls = nullptr;
	int          tb = 0;               // tile_power buffer of the call
	float*       tile_power = nullptr;
	bool         fold_in_history = false;   // (deferred gate: k_history folds the call's true peak in its place)

	// the ping-pong histories of the view: flip = 0 what the call reads, 1 what k_history writes for the next one
	float* fir_hist (int flip) const { return e->fir_hist[e->pos.hist_cur ^ flip].p + (size_t) c.off * MTR_FIR_HALO * 2; }
	float* mc_hist (int flip) const { return e->mc_hist[e->pos.hist_cur ^ flip].p + (size_t) c.off * MTR_FIR_HALO * e->cfg.n_channels; }

	// timing event `idx` of the call on stream `s`, if the call is timed
	int mark (int idx, hipStream_t s) const
	{
		if (!tm) return MTR_OK;
		const hipEvent_t v = next_event (e, ev0 + EV_PER_CALL - 1) ? e->ev[ev0 + idx].v : nullptr;   // (the whole group exists or none of it is used)
		if (v) HIPCHK (hipEventRecord (v, s));
		return MTR_OK;
	}

	// A PCM chunk's first step: its integer rows to floats, where the meters will read them
	int decode ()
	{
		const uint64_t n = c.n_frames * e->cfg.n_channels;
		hipEvent_t t0 = nullptr, t1 = nullptr;
		if (c.pick_fc && !c.pcm_format) {                          // wide f32 frames: picked, nothing of it counts as PCM
			if (mtr_launch_pick (0, c.pcm, c.pcm_pitch, c.pick_fc, e->frame_map, e->cfg.n_channels, const_cast<float*> (c.audio),
			                     c.stride * e->cfg.n_channels, c.cnt, c.n_frames, c.st))
				return fail (MTR_ERR_HIP, "k_pick launch");
			if (c.pcm_read) HIPCHK (hipEventRecord (c.pcm_read, c.st));
			e->lay_staged++;
			return MTR_OK;
		}
		if (e->timing && e->pcm_timed < 4096) {
			t0 = next_event (e->pcm_ev, (size_t) e->pcm_timed * 2);
			t1 = next_event (e->pcm_ev, (size_t) e->pcm_timed * 2 + 1);
		}
		if (t0 && t1) HIPCHK (hipEventRecord (t0, c.st));
		if (c.pick_fc) {
			if (mtr_launch_pick (c.pcm_format, c.pcm, c.pcm_pitch, c.pick_fc, e->frame_map, e->cfg.n_channels, const_cast<float*> (c.audio),
			                     c.stride * e->cfg.n_channels, c.cnt, c.n_frames, c.st))
				return fail (MTR_ERR_HIP, "k_pick launch");
			e->lay_staged++;
		} else if (mtr_launch_pcm (c.pcm_format, c.pcm, c.pcm_pitch, const_cast<float*> (c.audio), c.stride * e->cfg.n_channels, c.cnt, n, c.st))
			return fail (MTR_ERR_HIP, "k_pcm launch");
		if (t0 && t1) { HIPCHK (hipEventRecord (t1, c.st)); e->pcm_timed++; }
		if (c.pcm_read) HIPCHK (hipEventRecord (c.pcm_read, c.st));
		e->pcm_chunks++;
		e->pcm_bytes += (uint64_t) c.cnt * c.n_frames * (c.pick_fc ? c.pick_fc : e->cfg.n_channels) * mtr_setup_pcm_sample_bytes (c.pcm_format);
		return MTR_OK;
	}

	Route route () const
	{
		Route o;
		if (!ebu && !tp) return o;
		// Per-stream lengths: a call with them, or any call once a stream of this view is closed (its end is then 0: untouched).
		o.ragged = c.frames != nullptr;
		for (uint32_t i = 0; !o.ragged && e->n_closed && i < c.cnt; ++i) o.ragged = e->closed[c.off + i] != 0;
		const PlanCtx pctx = plan_ctx (e);
		o.sp = seg_plan (&pctx, c.audio, c.n_frames);
		// (k_seg hands the peak of a closing stream's last segments to k_kwtp16, whose tiles hold at most 64 x 38 frames: a whole
		// fragment up to 48.6 kHz.  Above that a call with lengths takes k_kwtp16 alone.)
		if (o.ragged && o.sp.use && e->fragm > 64u * (uint32_t) e->run) o.sp.use = false;
		// The tail of this call on the side stream?  Auto: a batch whose whole fragments go through k_seg, in an engine that meters
		// nothing else — measured (profiles/r06_tail.md): beside k_seg (issue-bound, one wave per SIMD, registers and LDS to spare) the
		// step is 0.04 - 1.4 % shorter than with the gate in front of it; beside k_kw (HBM-bound, eight waves per CU) it costs 8 %
		// MORE; behind k_bank it would start exactly when the next k_seg does; the chunks of a host call are link-bound anyway.
		const bool only_fused = (e->cfg.meters & ~(uint32_t) (MTR_METER_EBU | MTR_METER_TRUEPEAK)) == 0;
		// (and a batch of thousands of streams: the gate's serial time grows with the streams, what deferring it costs does not — at 1024 streams x 60 s
		// the serial order is 0.5 % FASTER, at 8192 x 10 s the deferred one by 0.4 - 1.4 % across boxes)
		o.defer = e->layout != 8 && (e->tail_mode == 2 || (e->tail_mode == 0 && !c.chunk && o.sp.use && only_fused && c.cnt >= TAIL_AUTO_STREAMS
		                                                   && (uint64_t) c.cnt * c.n_frames >= TAIL_AUTO_FRAMES));
		return o;
	}

	// [ends S | frag_lim S | from_tile S] of a ragged call into the next slot of the lengths ring, uploaded on the call's stream
	int upload_lengths ()
	{
		const SegPlan& sp = r.sp;
		const uint32_t S = c.cnt;
		const int slot = (e->len_cur + 1) % LEN_SLOTS;
		ls = &e->len_slot[slot];
		for (int i = 0; i < 2; ++i) if (ls->pending[i]) { HIPCHK (hipEventSynchronize (ls->done[i].v)); ls->pending[i] = false; }
		for (int i = 0; i < 2; ++i) HIPCHK (ls->done[i].ensure ());
		if (ls->dev.reserve ((size_t) 3 * S) || ls->pin.reserve ((size_t) 3 * S)) return fail (MTR_ERR_NOMEM, "per-stream lengths");
		uint32_t* const h_end = ls->pin.p;
		uint32_t* const h_lim = h_end + S;
		uint32_t* const h_from = h_end + 2 * (size_t) S;
		for (uint32_t i = 0; i < S; ++i) {
			const uint64_t f = e->closed[c.off + i] ? 0 : c.frames ? c.frames[i] : c.n_frames;
			h_end[i] = (uint32_t) f;
			// fragments that end at or before the stream's end
			const uint32_t nf = (uint32_t) (std::upper_bound (pl.frag_end.begin (), pl.frag_end.end (), (uint32_t) f) - pl.frag_end.begin ());
			h_lim[i] = f == 0 ? MTR_GATE_UNTOUCHED : f < c.n_frames ? (nf | MTR_GATE_CLOSING) : pl.n_frag;
			h_from[i] = 0xFFFFFFFFu;
			if (sp.use && f < c.n_frames) {
				// k_seg keeps the peak of every segment that reaches past f - 24 to itself; k_kwtp16 covers them from the first one on
				for (uint32_t q = 0; q < sp.n_segs; ++q) {
					const uint64_t fq = (uint64_t) q * sp.base + std::min (q, sp.rem), cq = sp.base + (q < sp.rem ? 1u : 0u);
					if ((fq + cq) * e->fragm + 24 + sp.head > f) { h_from[i] = pl.head_tiles + (uint32_t) fq; any_from = true; break; }
				}
			}
		}
		HIPCHK (hipMemcpyAsync (ls->dev.p, ls->pin.p, (size_t) 3 * S * sizeof (uint32_t), hipMemcpyHostToDevice, c.st));
		e->len_cur = slot;
		d_ends = ls->dev.p; d_lim = d_ends + S; d_from = d_ends + 2 * (size_t) S;
		return MTR_OK;
	}

	// The batch path: whole fragments through k_seg; the rest of an open fragment in front of them and what is left of the call
	// behind them (less than a fragment each) through k_kwtp16, each as ONE segment that picks the K-filter state up where its
	// predecessor in the stream left it.  `fa`: the call's k_kwtp16 arguments.
	int seg_batch (mtr_fused_args& fa)
	{
		const SegPlan& sp = r.sp;
		const uint32_t S = c.cnt;
		int lrc = 0;
		if (pl.head_tiles) {
			fa.seg_tile = e->head_seg; fa.n_segs = 1;
			lrc = mtr_launch_kwtp16 (e->run, ebu, fa, S, c.st);
		}
		mtr_seg_args sa;
		sa.audio = c.audio; sa.stride = c.stride; sa.hist = fir_hist (0); sa.state = fa.state; sa.tile_power = tile_power;
		sa.head = sp.head; sa.tile0 = pl.head_tiles;
		sa.mfma_a = e->m16_a.p;
		sa.n_streams = S; sa.n_segs = sp.n_segs; sa.n_tiles = pl.n_tiles; sa.tile_frames = e->fragm;
		sa.seg_base = sp.base; sa.seg_rem = sp.rem; sa.n_main = sp.n_main; sa.warm_steps = sp.warm_steps;
		sa.p0_end = (int64_t) c.n_frames - 24 - (int64_t) sp.head;
		sa.screen = e->seg_screen ? 1u : 0u; sa.seg_stats = e->prune_cnt.p + 2;
		set_kweight (e, sa);
		sa.ends = d_ends;
		const uint64_t units = (uint64_t) S * sp.n_segs;
		if (!lrc) lrc = mtr_launch_seg (ebu, sa, (uint32_t) ((units + 63) / 64), c.st);
		if (!lrc && any_from) {
			// the peaks k_seg left to k_kwtp16: from each closing stream's first such segment to its end (true peak only)
			fa.seg_tile = e->head_seg + 1; fa.n_segs = 1; fa.from_tile = d_from;
			lrc = mtr_launch_kwtp16 (e->run, false, fa, S, c.st);
			fa.from_tile = nullptr;
		}
		if (!lrc && pl.n_tiles > pl.head_tiles + sp.tiles) {
			fa.seg_tile = e->tail_seg; fa.n_segs = 1;
			lrc = mtr_launch_kwtp16 (e->run, ebu, fa, S, c.st);
		}
		nx.seg_calls += 1; nx.seg_frames += (uint64_t) sp.tiles * e->fragm;
		return lrc;
	}

	// layout 8: k_kwmc with its per-channel side buffers
	int kwmc (uint32_t warm_tiles) const
	{
		const size_t C = e->cfg.n_channels;
		mtr_kwmc_args ma;
		ma.audio = c.audio; ma.stride = c.stride; ma.hist = mc_hist (0);
		ma.tile_start = e->tile_start; ma.seg_tile = e->seg_tile; ma.scan_m = e->scan_m.p;
		ma.kz = e->mc_kz.p + c.off * C * 4; ma.tp_call = e->mc_tp_call.p + c.off * C;
		ma.tile_power = tile_power; ma.mfma_a = e->m16_a.p;
		ma.n_streams = c.cnt; ma.n_segs = pl.n_segs; ma.n_tiles = pl.n_tiles; ma.warm_tiles = warm_tiles;
		ma.n_frames = c.n_frames;
		set_kweight (e, ma);
		if (c.wave51) return mtr_launch_kwmc51 (ebu, tp, ma, d_ends, c.cnt * pl.n_segs, c.st);
		return mtr_launch_kwmc ((int) C, ebu, tp, ma, d_ends, c.cnt * pl.n_segs, c.st);
	}

	// the call's K-weighting / true-peak kernels: k_seg's batch path, layout 8, or one launch of layout 3 / 4 / 6
	int fused_kernels ()
	{
		const uint32_t S = c.cnt;
		// (deferred: the other tile_power buffer than the previous call's, whose gate may still be reading; the gate that read
		// this one two calls ago must be through — it has been for a whole call)
		tb = r.defer ? (e->tp_cur ^ 1) : 0;
		if (r.defer && e->gate_pending[tb]) { HIPCHK (hipStreamWaitEvent (c.st, e->ev_gate[tb].v, 0)); e->gate_pending[tb] = false; }
		e->tp_cur = tb;
		tile_power = e->tile_power[tb].p + (size_t) c.off * pl.n_tiles;
		const uint32_t warm_tiles = (uint32_t) std::ceil (MTR_WARM_SEC * e->cfg.sample_rate / (float) (64 * e->run));
		int lrc = 0;
		if (e->layout == 8) lrc = kwmc (warm_tiles);
		else {
			mtr_fused_args fa;
			fa.audio = c.audio; fa.stride = c.stride; fa.hist = fir_hist (0);
			fa.tile_start = e->tile_start; fa.seg_tile = e->seg_tile; fa.scan_m = e->scan_m.p;
			fa.state = e->state.p + c.off; fa.tile_power = tile_power;
			fa.n_streams = S; fa.n_segs = pl.n_segs; fa.n_tiles = pl.n_tiles; fa.warm_tiles = warm_tiles;
			set_kweight (e, fa);
			fa.n_frames = c.n_frames;
			fa.buf_slots = e->layout >= 4 ? pl.kw_slots : pl.buf_slots;
			fa.mfma_a = e->m16_a.p;
			fa.fir_form = e->cfg.tune_fir;
			fa.rotate = e->layout == 3;
			fa.prune = e->cfg.tune_prune > 2 ? 2 : (int) e->cfg.tune_prune;
			fa.prune_stats = e->prune_cnt.p;
			fa.ends = d_ends; fa.from_tile = nullptr;
			lrc = r.sp.use     ? seg_batch (fa)
			    : e->layout == 6 ? mtr_launch_kwtp16 (e->run, ebu, fa, S * pl.n_segs, c.st)
			    : e->layout == 4 ? mtr_launch_kw (e->run, fa, S * pl.n_segs, c.st)
			                     : mtr_launch_fused2 (e->run, ebu, tp, fa, S * pl.n_segs, c.st);
		}
		if (lrc) { plan_abort (e, c.st); return fail (MTR_ERR_HIP, "k_fused launch", hipGetLastError ()); }
		return mark (1, c.st);
	}

	// k_gate behind the fused kernels: on the call's stream, or — deferred — handed over to the side stream
	int gate ()
	{
		hipStream_t gst = c.st;                                       // the stream the gate runs on
		if (r.defer) {
			gst = e->tail_stream.v;
			HIPCHK (hipEventRecord (e->ev_fused.v, c.st));
			HIPCHK (hipStreamWaitEvent (gst, e->ev_fused.v, 0));
			// The gate becomes runnable at the very moment the NEXT call's fused kernel does (both wait for this call's), and
			// its 8192 workgroups would flood the CUs while k_seg's 1024 one-wave workgroups are being placed, one per SIMD:
			// measured, k_seg then takes 15.4 ms instead of 9.5 (profiles/r06_tail.md) — the placement of a persistent kernel
			// is for good.  So the side stream first idles for tail_delay_us: by then k_seg is resident (its dispatch takes
			// ~10 us) and the gate's waves (72 VGPRs) fill in beside it (344 of 512).  Off the critical path by construction.
			if (e->tail_delay_us && mtr_launch_delay (e->tail_delay_us, gst)) { plan_abort (e, c.st); return fail (MTR_ERR_HIP, "k_delay launch"); }
			e->tail_pending = true;
			e->deferred_calls++;
			fold_in_history = tp;
		}
		{ const int rc = mark (2, gst); if (rc) return rc; }
		mtr_gate_args ga;
		ga.state = e->state.p + c.off; ga.hist = e->hist.p + (size_t) c.off * 2 * MTR_HIST_LEN; ga.tile_power = tile_power;
		ga.frag_tile = e->frag_tile; ga.frag_power = e->frag_power.p + (size_t) c.off * pl.n_frag; ga.bin_power = e->bin_power.p;
		ga.n_streams = c.cnt; ga.n_tiles = ebu ? pl.n_tiles : 0; ga.n_frag = ebu ? pl.n_frag : 0;
		ga.tail_tile = ebu ? pl.tail_tile : 0;
		ga.fragm = (float) e->fragm; ga.integr = e->integr ? 1 : 0;
		ga.max_scratch = e->gate_max.p + (size_t) c.off * 2;
		ga.fold_tp = (fold_in_history || e->layout == 8) ? 0 : 1;   // (layout 8: k_history_mc folds the per-channel peaks)
		ga.polite_grid = r.defer ? e->tail_gate_grid : 0;
		if (mtr_launch_gate (ga, d_lim, gst)) { plan_abort (e, gst); return fail (MTR_ERR_HIP, "k_gate launch"); }
		if (ls) { HIPCHK (hipEventRecord (ls->done[1].v, gst)); ls->pending[1] = true; }
		{ const int rc = mark (3, gst); if (rc) return rc; }
		{
			PlanSlot& ps = e->plan_slot[e->plan_cur];                 // k_gate is the plan's last reader
			HIPCHK (hipEventRecord (ps.done.v, gst));
			ps.pending = true;
		}
		if (r.defer) { HIPCHK (hipEventRecord (e->ev_gate[tb].v, gst)); e->gate_pending[tb] = true; }
		e->last_n_frag = ga.n_frag;
		nx.frcnt = pl.frcnt_out;
		return MTR_OK;
	}

	int bank ()
	{
		const size_t vo = c.off;
		mtr_bank_args ba;
		ba.audio = c.audio; ba.stride = c.stride; ba.n_frames = c.n_frames;
		ba.coef = e->bank_coef.p; ba.z = e->bank_z.p + vo * MTR_NBANDS * 12; ba.val = e->bank_val.p + vo * MTR_NBANDS; ba.mx = e->bank_max.p + vo * MTR_NBANDS;
		ba.ac_in = e->bank_ac[e->pos.bank_ac_cur].p + vo; ba.ac_out = e->bank_ac[e->pos.bank_ac_cur ^ 1].p + vo;
		ba.n_streams = c.cnt; ba.n_channels = e->cfg.n_channels; ba.omega = e->omega;
		if (mtr_launch_bank (ba, c.st)) return fail (MTR_ERR_HIP, "k_bank launch");
		nx.bank_ac_cur = e->pos.bank_ac_cur ^ 1;
		return MTR_OK;
	}

	// (the integer tables are int32, as the reference's, which stops counting at 2^31 - 1 samples; the kernels index
	// a call's samples with 32 bits: checked on entry)
	int intstat () const
	{
		if (e->cfg.meters & MTR_METER_BITSTATS)
			if (mtr_launch_bitstats (c.audio, c.stride, c.n_frames, e->bim.p + c.off, c.cnt, c.st)) return fail (MTR_ERR_HIP, "k_bitstats launch");
		if (e->cfg.meters & MTR_METER_SIGDIST)
			if (mtr_launch_sigdist (c.audio, c.stride, c.n_frames, e->sdh.p + c.off, c.cnt, c.st)) return fail (MTR_ERR_HIP, "k_sigdist launch");
		return MTR_OK;
	}

	int dr14 ()
	{
		const size_t vo = c.off;
		mtr_dr14_args da;
		da.audio = c.audio; da.stride = c.stride; da.n_frames = c.n_frames;
		da.window = (uint64_t) rintf (e->cfg.sample_rate * 3.0f) + 1;       // dr14.c:155, :404
		da.e0 = da.window - e->pos.dr_scnt;
		const uint64_t tot = e->pos.dr_scnt + c.n_frames;
		da.n_windows = (uint32_t) (tot / da.window);
		da.n_pieces = da.n_windows + (tot % da.window ? 1 : 0);
		da.n_streams = c.cnt; da.n_channels = e->cfg.n_channels;
		if (e->dr_sum.reserve ((size_t) e->cfg.n_streams * da.n_pieces * 2) || e->dr_peak.reserve ((size_t) e->cfg.n_streams * da.n_pieces * 2))
			return fail (MTR_ERR_NOMEM, "hipMalloc DR14 pieces");
		da.state = e->dr_state.p + vo; da.hist = e->dr_hist.p + vo * e->cfg.n_channels * MTR_DR_HISTBINS;
		da.piece_sum = e->dr_sum.p + vo * da.n_pieces * 2; da.piece_peak = e->dr_peak.p + vo * da.n_pieces * 2;
		if (mtr_launch_dr14 (da, c.st)) return fail (MTR_ERR_HIP, "k_dr14 launch");
		nx.dr_scnt = tot % da.window;
		return MTR_OK;
	}

	int kmeter ()
	{
		const size_t vo = c.off;
		mtr_kmeter_args ka;
		ka.audio = c.audio; ka.stride = c.stride; ka.n_groups = c.n_frames / 4;
		ka.n_streams = c.cnt; ka.n_channels = e->cfg.n_channels;
		ka.n_pieces = mtr_kmeter_pieces (ka.n_groups);
		if (nx.km_fpp != (uint32_t) c.n_frames) {                          // kmeterdsp.cc:60-65
			nx.km_fall = powf (10.0f, -0.05f * 15.0f * ((float) c.n_frames / e->cfg.sample_rate));
			nx.km_fpp = (uint32_t) c.n_frames;
		}
		ka.fpp = nx.km_fpp; ka.fall = nx.km_fall;
		ka.hold = (int32_t) (0.5f * e->cfg.sample_rate + 0.5f);             // :51
		ka.omega = 9.72f / e->cfg.sample_rate;
		memcpy (ka.pw1, e->km_pw1, sizeof (ka.pw1));
		ka.state = e->km_state.p + vo * 2;
		if (e->km_piece.reserve ((size_t) e->cfg.n_streams * std::max<uint32_t> (ka.n_pieces, 1) * 4) || e->km_max.reserve ((size_t) e->cfg.n_streams * std::max<uint32_t> (ka.n_pieces, 1) * 2))
			return fail (MTR_ERR_NOMEM, "hipMalloc KMETER pieces");
		ka.piece_state = e->km_piece.p + vo * ka.n_pieces * 4; ka.piece_max = e->km_max.p + vo * ka.n_pieces * 2;
		if (mtr_launch_kmeter (ka, c.st)) return fail (MTR_ERR_HIP, "k_kmeter launch");
		return MTR_OK;
	}

	// The periods of the reading series are cut from where the CALL started (e->pos): every chunk of a host call sees the same cuts
	int stcorr ()
	{
		const size_t vo = c.off;
		const uint64_t P = e->sc_period;
		mtr_stcorr_args sa;
		sa.audio = c.audio; sa.stride = c.stride; sa.n_frames = c.n_frames;
		sa.period = P; sa.e0 = P ? P - e->pos.sc_fill : c.n_frames;
		sa.n_streams = c.cnt; sa.chunk = e->sc_chunk; sa.warm = e->sc_warm;
		sa.n_pieces = mtr_stcorr_pieces (c.n_frames, sa.e0, P, sa.chunk);
		sa.w1 = e->sc_w[0]; sa.w2 = e->sc_w[1];
		sa.capacity = e->sc_cap; sa.point0 = e->pos.sc_points;
		if (e->sc_piece.reserve ((size_t) e->cfg.n_streams * sa.n_pieces * MTR_STCORR_PIECE)) return fail (MTR_ERR_NOMEM, "hipMalloc STCORR pieces");
		sa.state = e->sc_state.p + vo; sa.piece = e->sc_piece.p + vo * sa.n_pieces * MTR_STCORR_PIECE;
		sa.series = e->sc_cap ? e->sc_series.p + vo * e->sc_cap : nullptr;
		if (mtr_launch_stcorr (sa, c.st)) return fail (MTR_ERR_HIP, "k_stcorr launch");
		const uint64_t tot = e->pos.sc_fill + c.n_frames;
		nx.sc_fill = P ? tot % P : 0;
		nx.sc_points = e->pos.sc_points + (P ? tot / P : 0);
		return MTR_OK;
	}

	int tpb () const
	{
		mtr_tpb_args ta;
		ta.audio = c.audio; ta.stride = c.stride; ta.n_frames = c.n_frames;
		ta.hist = fir_hist (0); ta.mfma_a = e->m16_a.p; ta.state = e->state.p + c.off;
		ta.n_streams = c.cnt; ta.n_channels = e->cfg.n_channels;
		ta.w1 = e->tpb_w[0]; ta.w2 = e->tpb_w[1]; ta.w3 = e->tpb_w[2]; ta.g = e->tpb_w[3];
		if (mtr_launch_tpb (ta, c.st)) return fail (MTR_ERR_HIP, "k_tpb launch");
		return MTR_OK;
	}

	// the 47 frames before the next call; after every consumer of the current history
	int history ()
	{
		const uint32_t C = e->cfg.n_channels;
		mtr_stream_state* const state = e->state.p + c.off;
		// (deferred: the fold of this call's peaks rides here — behind the reduction of the previous call, which reads the holds)
		if (fold_in_history && e->red_pending) { HIPCHK (hipStreamWaitEvent (c.st, e->ev_red.v, 0)); e->red_pending = false; }
		if (e->layout != 8) {
			const int hrc = C == 2 ? mtr_launch_history (c.audio, c.stride, c.n_frames, fir_hist (0), fir_hist (1), c.cnt, fold_in_history ? state : nullptr, d_ends, c.st)
			                       : mtr_launch_history_mono (c.audio, c.stride, c.n_frames, fir_hist (0), fir_hist (1), c.cnt, c.st);
			if (hrc) return fail (MTR_ERR_HIP, "k_history launch");
		} else if (tp) {
			const size_t vc = (size_t) c.off * C;
			if (c.wave51 ? mtr_launch_history_mc51 (c.audio, c.stride, c.n_frames, mc_hist (0), mc_hist (1), c.cnt, e->mc_tp_call.p + vc, e->mc_tp_last.p + vc,
			                                        e->mc_tp_hold.p + vc, state, d_ends, c.st)
			             : mtr_launch_history_mc (c.audio, c.stride, c.n_frames, C, mc_hist (0), mc_hist (1), c.cnt, e->mc_tp_call.p + vc, e->mc_tp_last.p + vc, e->mc_tp_hold.p + vc,
			                           state, d_ends, c.st))
				return fail (MTR_ERR_HIP, "k_history_mc launch");
		}
		nx.hist_cur = e->pos.hist_cur ^ 1;
		return MTR_OK;
	}

	// The steps of a call, in the order of the launches.  What describes QUEUED WORK (last_stream / queued, the plan and lengths rings,
	// tp_cur, the pending flags of the side stream, the timing events) moves where the work is queued: it must be true even if a later
	// launch fails.  What describes the METERING POSITION moves at the end: an error return has not advanced the engine.
	int run ()
	{
		int rc = check_limits (e, c.n_frames);
		if (rc) return rc;
		if ((rc = enter_stream (e, c.st))) return rc;
		const bool fused = ebu || tp;
		const uint32_t meters = e->cfg.meters;
		if (c.pcm && ((rc = mark (6, c.st)) || (rc = decode ()))) return rc;
		if ((rc = mark (0, c.st))) return rc;
		if (tm) {
			if (e->ev_decode.size () <= e->timed_calls) e->ev_decode.resize ((size_t) e->timed_calls + 1);
			e->ev_decode[e->timed_calls] = c.pcm != nullptr;
		}

		r = route ();
		if (r.defer) rc = tail_setup (e);
		else if (fused) rc = join_tail (e, c.st);                     // a serial gate follows the deferred ones
		if (rc) return rc;
		e->last_deferred = r.defer;

		if (fused) {
			if ((rc = build_plan (e, c.n_frames, r.sp.use ? r.sp.head : 0, r.sp.use ? r.sp.tiles : 0, c.st))) return rc;
			if (r.ragged && (rc = upload_lengths ())) return rc;
			if ((rc = fused_kernels ())) return rc;
			if ((rc = gate ())) return rc;
		} else {
			for (int i = 1; i <= 3; ++i) if ((rc = mark (i, c.st))) return rc;
		}
		if ((rc = mark (4, c.st))) return rc;

		if ((meters & MTR_METER_SPECTR30) && (rc = bank ())) return rc;
		if ((meters & (MTR_METER_BITSTATS | MTR_METER_SIGDIST)) && (rc = intstat ())) return rc;
		if ((meters & MTR_METER_DR14) && (rc = dr14 ())) return rc;
		if ((meters & MTR_METER_KMETER) && (rc = kmeter ())) return rc;
		if ((meters & MTR_METER_STCORR) && (rc = stcorr ())) return rc;
		if ((meters & MTR_METER_TPBALLIST) && (rc = tpb ())) return rc;
		if ((meters & (MTR_METER_TRUEPEAK | MTR_METER_TPBALLIST)) && (rc = history ())) return rc;
		if (ls) {                                                     // (the lengths' last reader on this stream: k_history_len, or the fused kernels)
			HIPCHK (hipEventRecord (ls->done[0].v, c.st));
			ls->pending[0] = true;
		}
		if (tm) {
			const hipEvent_t v = next_event (e, ev0 + 5);
			if (v) { HIPCHK (hipEventRecord (v, c.st)); e->timed_calls++; }   // (a call without all of its events is not a timed call)
		}
		// everything is queued.  Frames metered per stream; a stream that ends inside a call with lengths is closed by it
		for (uint32_t i = 0; i < c.cnt; ++i) {
			const size_t g = (size_t) c.off + i;
			if (e->closed[g]) continue;
			const uint64_t f = c.frames ? c.frames[i] : c.n_frames;
			e->metered[g] += f;
			if (f < c.n_frames) { e->closed[g] = 1; e->n_closed++; }
		}
		if (c.commit) e->pos = nx;
		return MTR_OK;
	}
};

static int process_call (mtr_engine* e, const Call& c) { return CallRun { e, c }.run (); }

struct Source;
static int process_chunked (mtr_engine* e, const Source& src, uint64_t n_frames, uint64_t stride, const uint64_t* frames);
static int process_device_picked (mtr_engine* e, const float* d_audio, uint64_t n_frames, uint64_t stride, const uint64_t* frames, void* hip_stream);

static int process_device (mtr_engine* e, const float* d_audio, uint64_t n_frames, uint64_t stride, const uint64_t* frames, void* hip_stream)
{
	// A frame layout.  WAVE 5.1 on a 5-channel engine: k_kwmc51 and k_history_mc51 read the 6-channel frames where they lie (a pick pass
	// in front of an HBM-bound kernel would read 6/5 and write 5/5 of the batch on top).  Every other map: the wide rows are picked chunk
	// by chunk into the staging buffers, as device PCM is decoded.
	const bool direct = e->picks && e->wave51;
	if (e->picks && !direct) return process_device_picked (e, d_audio, n_frames, stride, frames, hip_stream);
	if (n_frames == 0) return MTR_OK;
	if (stride < n_frames) return fail (MTR_ERR_ARG, "stream_stride_frames < n_frames");
	HIPCHK (hipSetDevice (e->cfg.device));
	Call c { d_audio, n_frames, stride, (hipStream_t) hip_stream, 0, e->cfg.n_streams, frames, false, true };
	c.wave51 = direct;
	const int rc = process_call (e, c);
	if (!rc && direct) e->lay_direct++;
	return rc;
}

extern "C" {

int mtr_engine_process_device (mtr_engine* e, const float* d_audio, uint64_t n_frames,
                               uint64_t stride, void* hip_stream)
{
	if (!e || !d_audio) return fail (MTR_ERR_ARG, "mtr_engine_process_device: null argument");
	return process_device (e, d_audio, n_frames, stride, nullptr, hip_stream);
}

// Per-stream lengths need EBU / TRUEPEAK alone (every layout, 2 .. 5 channels)
static int lengths_check (mtr_engine* e, uint64_t n_frames, const uint64_t* frames, uint32_t n)
{
	if ((e->cfg.meters & ~(uint32_t) (MTR_METER_EBU | MTR_METER_TRUEPEAK)) || !(e->cfg.meters & (MTR_METER_EBU | MTR_METER_TRUEPEAK)))
		return fail (MTR_ERR_UNSUPPORTED, "per-stream lengths: EBU / TRUEPEAK engines only");
	for (uint32_t i = 0; i < n; ++i)
		if (frames[i] > n_frames) return fail (MTR_ERR_ARG, "per-stream lengths: frames[s] > n_frames");
	return MTR_OK;
}

int mtr_engine_process_device_lengths (mtr_engine* e, const float* d_audio, uint64_t n_frames, uint64_t stride,
                                       const uint64_t* frames, void* hip_stream)
{
	if (!e || !d_audio || !frames) return fail (MTR_ERR_ARG, "mtr_engine_process_device_lengths: null argument");
	const int crc = lengths_check (e, n_frames, frames, e->cfg.n_streams);
	if (crc) return crc;
	return process_device (e, d_audio, n_frames, stride, frames, hip_stream);
}

int mtr_engine_stream_frames (mtr_engine* e, uint32_t first, uint32_t count, uint64_t* frames, uint8_t* closed)
{
	if (!e) return fail (MTR_ERR_ARG, "null engine");
	if ((uint64_t) first + count > e->cfg.n_streams) return fail (MTR_ERR_ARG, "stream range");
	for (uint32_t i = 0; i < count; ++i) {
		if (frames) frames[i] = e->metered[first + i];
		if (closed) closed[i] = e->closed[first + i];
	}
	return MTR_OK;
}

int mtr_engine_set_host_chunk_bytes (mtr_engine* e, uint64_t bytes)
{
	if (!e) return fail (MTR_ERR_ARG, "null engine");
	e->host_chunk_bytes = bytes ? (size_t) bytes : (size_t) 256 << 20;
	return MTR_OK;
}

// Where a chunked call takes its samples from: host or device memory, f32 or integer PCM (format MTR_PCM_*, 0 = f32)
struct Source {
	const void* p;
	int         format;
	bool        host;
	void*       hip_stream;   // device source: the caller's stream (a host source runs on the engine's own)
};

// Memory in, CHUNKED by streams (results are per stream: chunking is exact, and the routing of a call — which kernel,
// how many time segments — is decided for the whole batch, so every stream sees the arithmetic it would see resident):
// chunk k + 1 crosses the host link on a copy stream while the kernels of chunk k run on the engine's own; two device
// buffers of one chunk each instead of a copy of the whole batch.  End to end the call runs at the link's rate
// (bench.py: extra.end_to_end_host).
// Integer PCM is the same loop with one more step: the chunk's INTEGER rows cross the link into one of two raw buffers (rows on 16
// bytes), and the chunk's call decodes them into the float buffer first (CallRun::decode) — the float chunk is laid out exactly as the
// float path stages it (same dstride, same chunks: host_chunk_bytes counts decoded bytes), so the meters see the very same call.  The
// raw buffer is free again once the decode has read it, the float buffer once the meters have: stream order, both on the engine's stream.
// PCM in device memory: the same chunks without the copy, decoded straight from the caller's rows on the caller's stream.
static int process_chunked (mtr_engine* e, const Source& src, uint64_t n_frames, uint64_t stride, const uint64_t* frames)
{
	if (n_frames == 0) return MTR_OK;
	if (stride < n_frames) return fail (MTR_ERR_ARG, "stream_stride_frames < n_frames");
	int rc = check_limits (e, n_frames);
	if (rc) return rc;
	HIPCHK (hipSetDevice (e->cfg.device));
	const size_t C = e->cfg.n_channels;
	const uint32_t S = e->cfg.n_streams;
	const size_t sb = src.format ? mtr_setup_pcm_sample_bytes (src.format) : sizeof (float);   // bytes per sample at the source
	// (streams start on 16 bytes in the staging buffers — an even stride of stereo frames, a multiple of four mono ones — so that
	// every layout can take the call and k_tpb's LDS-DMA its source)
	const uint64_t dstride = C == 2 ? (n_frames + 1) & ~(uint64_t) 1 : (n_frames + 3) & ~(uint64_t) 3;   // (and 1, 3, 4, 5 channels: a multiple of four frames)
	const size_t row = (size_t) dstride * C;                                  // floats per staged stream
	uint32_t cs = (uint32_t) std::min<uint64_t> (S, std::max<uint64_t> (1, e->host_chunk_bytes / (row * sizeof (float))));
	const uint32_t n_chunks = (S + cs - 1) / cs;
	cs = (S + n_chunks - 1) / n_chunks;                                         // even chunks
	const size_t buf_floats = ((size_t) cs * row + 63) & ~(size_t) 63;         // the second buffer starts on 256 bytes
	// frame layout: the source rows hold frames of FC samples (the default: C), picked by the chunk's first step as PCM is decoded by it
	const bool pick = e->picks;
	const size_t FC = pick ? e->frame_channels : C;
	const size_t raw_pitch = (n_frames * FC * sb + 15) & ~(size_t) 15;         // PCM / wide frames from the host: bytes per landed row ...
	const size_t raw_bytes = ((size_t) cs * raw_pitch + 255) & ~(size_t) 255;  // ... and per raw buffer
	const bool landing = src.host && (src.format || pick);
	hipStream_t st = (hipStream_t) src.hip_stream;
	if (src.host) {
		HIPCHK (e->own_stream.ensure ());
		st = e->own_stream.v;
		HIPCHK (e->copy_stream.ensure ());
		for (int b = 0; b < 2; ++b) {
			HIPCHK (e->ev_copied[b].ensure ());
			HIPCHK (e->ev_computed[b].ensure ());
		}
		// the staging buffers may still be read by the previous call (on whatever stream that ran)
		HIPCHK (hipStreamSynchronize (e->last_stream));
	} else if (e->stage.n < buf_floats * (n_chunks > 1 ? 2 : 1)) {
		// (a device source never waits for the previous call — the chunk's call orders its stream behind it before the decode writes the
		// staging buffer — unless that buffer has to grow)
		if ((rc = sync_all (e))) return rc;
	}
	if (e->stage.reserve (buf_floats * (n_chunks > 1 ? 2 : 1))) return fail (MTR_ERR_NOMEM, "hipMalloc staging buffers");
	if (landing && e->pcm_raw.reserve (raw_bytes * (n_chunks > 1 ? 2 : 1))) return fail (MTR_ERR_NOMEM, "hipMalloc PCM buffers");
	// (every exit behind the first copy goes through ONE place that waits for the copy stream: the source is pageable caller
	// memory and the copies are truly asynchronous — the caller may free or reuse it as soon as we return, error or not)
	hipError_t he = hipSuccess;
	const char* what = nullptr;
#define HOSTCHK(call) do { he = (call); if (he != hipSuccess) { what = #call; goto done; } } while (0)
	for (uint32_t k = 0, off = 0; k < n_chunks; ++k, off += cs) {
		const uint32_t cnt = std::min (cs, S - off);
		const int b = (int) (k & 1);
		float* const dst = e->stage.p + (size_t) b * buf_floats;
		// (the lengths of the chunk's streams are indexed from its first; the cursors move with the last chunk)
		Call c { dst, n_frames, dstride, st, off, cnt, frames ? frames + off : nullptr, true, k + 1 == n_chunks };
		const uint8_t* from = (const uint8_t*) src.p + (size_t) off * stride * FC * sb;
		size_t pitch = stride * FC * sb;
		if (src.host) {
			void* const land = landing ? (void*) (e->pcm_raw.p + (size_t) b * raw_bytes) : (void*) dst;
			const size_t land_pitch = landing ? raw_pitch : row * sizeof (float);
			if (k >= 2) HOSTCHK (hipStreamWaitEvent (e->copy_stream.v, e->ev_computed[b].v, 0));   // the kernels of chunk k - 2 have read this buffer
			HOSTCHK (hipMemcpy2DAsync (land, land_pitch, from, pitch, n_frames * FC * sb, cnt, hipMemcpyHostToDevice, e->copy_stream.v));
			HOSTCHK (hipEventRecord (e->ev_copied[b].v, e->copy_stream.v));
			HOSTCHK (hipStreamWaitEvent (st, e->ev_copied[b].v, 0));
			from = (const uint8_t*) land;
			pitch = land_pitch;
		}
		if (src.format || pick) {
			c.pcm = from;
			c.pcm_pitch = pitch;
			c.pcm_format = src.format;
			c.pick_fc = pick ? (uint32_t) FC : 0;
			if (landing) c.pcm_read = e->ev_computed[b].v;
		}
		rc = process_call (e, c);
		if (rc) goto done;
		if (src.host && !landing) HOSTCHK (hipEventRecord (e->ev_computed[b].v, st));
	}
#undef HOSTCHK
done:
	if (src.host) {
		// wait for the copies (not for the kernels)
		const hipError_t hs = hipStreamSynchronize (e->copy_stream.v);
		if (what) return fail (MTR_ERR_HIP, what, he);
		if (rc) return rc;
		if (hs != hipSuccess) return fail (MTR_ERR_HIP, "hipStreamSynchronize (copy stream)", hs);
	}
	return rc;
}

}   // extern "C"

static int process_device_picked (mtr_engine* e, const float* d_audio, uint64_t n_frames, uint64_t stride, const uint64_t* frames, void* hip_stream)
{
	return process_chunked (e, { d_audio, 0, false, hip_stream }, n_frames, stride, frames);
}

extern "C" {

static int process_host (mtr_engine* e, const float* h_audio, uint64_t n_frames, uint64_t stride, const uint64_t* frames)
{
	return process_chunked (e, { h_audio, 0, true, nullptr }, n_frames, stride, frames);
}

int mtr_engine_process_host (mtr_engine* e, const float* h_audio, uint64_t n_frames, uint64_t stride)
{
	if (!e || !h_audio) return fail (MTR_ERR_ARG, "mtr_engine_process_host: null argument");
	return process_host (e, h_audio, n_frames, stride, nullptr);
}

int mtr_engine_process_host_lengths (mtr_engine* e, const float* h_audio, uint64_t n_frames, uint64_t stride, const uint64_t* frames)
{
	if (!e || !h_audio || !frames) return fail (MTR_ERR_ARG, "mtr_engine_process_host_lengths: null argument");
	const int crc = lengths_check (e, n_frames, frames, e->cfg.n_streams);
	if (crc) return crc;
	return process_host (e, h_audio, n_frames, stride, frames);
}

// Integer PCM: what every PCM entry point checks before anything is queued
static int pcm_check (mtr_engine* e, const void* pcm, int format, uint64_t n_frames, const uint64_t* frames, const char* who)
{
	if (!e || !pcm) return fail (MTR_ERR_ARG, who);
	if (!mtr_setup_pcm_sample_bytes (format)) return fail (MTR_ERR_ARG, "unknown PCM format (MTR_PCM_S16, _S24, _S32)");
	return frames ? lengths_check (e, n_frames, frames, e->cfg.n_streams) : MTR_OK;
}

int mtr_engine_process_host_pcm (mtr_engine* e, const void* h_pcm, int format, uint64_t n_frames, uint64_t stride, const uint64_t* frames)
{
	const int crc = pcm_check (e, h_pcm, format, n_frames, frames, "mtr_engine_process_host_pcm: null argument");
	if (crc) return crc;
	return process_chunked (e, { h_pcm, format, true, nullptr }, n_frames, stride, frames);
}

int mtr_engine_process_device_pcm (mtr_engine* e, const void* d_pcm, int format, uint64_t n_frames, uint64_t stride,
                                   const uint64_t* frames, void* hip_stream)
{
	const int crc = pcm_check (e, d_pcm, format, n_frames, frames, "mtr_engine_process_device_pcm: null argument");
	if (crc) return crc;
	return process_chunked (e, { d_pcm, format, false, hip_stream }, n_frames, stride, frames);
}

size_t mtr_pcm_sample_bytes (int format) { return mtr_setup_pcm_sample_bytes (format); }

int mtr_pcm_decode_host (int format, const void* src, size_t n_samples, float* dst)
{
	if (!mtr_setup_pcm_sample_bytes (format)) return fail (MTR_ERR_ARG, "unknown PCM format (MTR_PCM_S16, _S24, _S32)");
	if (n_samples && (!src || !dst)) return fail (MTR_ERR_ARG, "mtr_pcm_decode_host: null argument");
	return mtr_setup_pcm_decode (format, src, n_samples, dst) ? fail (MTR_ERR_ARG, "mtr_pcm_decode_host") : MTR_OK;
}

int mtr_engine_pcm_stats (mtr_engine* e, uint64_t* chunks, uint64_t* bytes, float* decode_ms)
{
	if (!e) return fail (MTR_ERR_ARG, "null engine");
	if (e->pcm_timed) {
		const int rc = mtr_engine_sync (e);
		if (rc) return rc;
		for (uint32_t i = 0; i < e->pcm_timed && (size_t) 2 * i + 1 < e->pcm_ev.size (); ++i) {
			float ms;
			if (hipEventElapsedTime (&ms, e->pcm_ev[2 * i].v, e->pcm_ev[2 * i + 1].v) == hipSuccess) e->pcm_ms += ms;
		}
		e->pcm_timed = 0;
	}
	if (chunks) *chunks = e->pcm_chunks;
	if (bytes) *bytes = e->pcm_bytes;
	if (decode_ms) *decode_ms = e->pcm_ms;
	return MTR_OK;
}

int mtr_engine_set_frame_layout (mtr_engine* e, uint32_t frame_channels, const uint8_t* map)
{
	if (!e) return fail (MTR_ERR_ARG, "null engine");
	const uint32_t C = e->cfg.n_channels;
	if (frame_channels == 0) {
		e->frame_channels = 0;
		for (uint32_t c = 0; c < MTR_MAX_CHANNELS; ++c) e->frame_map[c] = (uint8_t) c;
		e->picks = e->wave51 = false;
		return MTR_OK;
	}
	if (frame_channels > MTR_MAX_FRAME_CHANNELS) return fail (MTR_ERR_ARG, "mtr_engine_set_frame_layout: frame_channels > MTR_MAX_FRAME_CHANNELS");
	if (!map) return fail (MTR_ERR_ARG, "mtr_engine_set_frame_layout: null map");
	bool identity = frame_channels == C;
	for (uint32_t c = 0; c < C; ++c) {
		if (map[c] >= frame_channels) return fail (MTR_ERR_ARG, "mtr_engine_set_frame_layout: a map entry >= frame_channels");
		identity = identity && map[c] == c;
	}
	e->frame_channels = frame_channels;
	for (uint32_t c = 0; c < C; ++c) e->frame_map[c] = map[c];
	e->picks = !identity;                                          // (the explicit identity is the default and takes its paths)
	e->wave51 = e->layout == 8 && C == 5 && frame_channels == 6 && map[0] == 0 && map[1] == 1 && map[2] == 2 && map[3] == 4 && map[4] == 5;
	return MTR_OK;
}

int mtr_engine_frame_layout (const mtr_engine* e, uint32_t* frame_channels, uint8_t* map)
{
	if (!e) return fail (MTR_ERR_ARG, "null engine");
	if (frame_channels) *frame_channels = e->frame_channels ? e->frame_channels : e->cfg.n_channels;
	if (map) for (uint32_t c = 0; c < e->cfg.n_channels; ++c) map[c] = e->frame_map[c];
	return MTR_OK;
}

int mtr_pick_decode_host (int format, const void* src, size_t n_frames, uint32_t frame_channels, const uint8_t* map, uint32_t n_channels, float* dst)
{
	if (format && !mtr_setup_pcm_sample_bytes (format)) return fail (MTR_ERR_ARG, "unknown format (0 = f32, MTR_PCM_S16, _S24, _S32)");
	if (!map || !frame_channels || frame_channels > MTR_MAX_FRAME_CHANNELS || !n_channels || n_channels > MTR_MAX_CHANNELS)
		return fail (MTR_ERR_ARG, "mtr_pick_decode_host: map / frame_channels / n_channels");
	if (n_frames && (!src || !dst)) return fail (MTR_ERR_ARG, "mtr_pick_decode_host: null argument");
	return mtr_setup_pick_decode (format, src, n_frames, frame_channels, map, n_channels, dst)
	       ? fail (MTR_ERR_ARG, "mtr_pick_decode_host: a map entry >= frame_channels") : MTR_OK;
}

int mtr_engine_layout_stats (mtr_engine* e, uint64_t* staged_chunks, uint64_t* direct_calls)
{
	if (!e) return fail (MTR_ERR_ARG, "null engine");
	if (staged_chunks) *staged_chunks = e->lay_staged;
	if (direct_calls) *direct_calls = e->lay_direct;
	return MTR_OK;
}

// One LV2 block: interleave into page-locked memory, one H2D copy, the kernels, one D2H copy of the stream's state
// (and the bank's levels), ONE wait.  No allocation after the first block of a given size.
int mtr_engine_process_planar_host (mtr_engine* e, const float* const* ch, uint32_t n_frames)
{
	if (!e || !ch || !ch[0]) return fail (MTR_ERR_ARG, "mtr_engine_process_planar_host: null argument");
	if (e->cfg.n_streams != 1) return fail (MTR_ERR_ARG, "planar host input is the n_streams == 1 (LV2) path");
	if (n_frames == 0) return MTR_OK;
	const uint32_t C = e->cfg.n_channels;
	for (uint32_t c = 1; c < C; ++c) if (!ch[c]) return fail (MTR_ERR_ARG, "mtr_engine_process_planar_host: a channel pointer is NULL");
	HIPCHK (hipSetDevice (e->cfg.device));
	HIPCHK (e->own_stream.ensure ());
	const hipStream_t st = e->own_stream.v;
	if (e->last_stream != st) HIPCHK (hipStreamSynchronize (e->last_stream));   // resets queued before the first block
	const size_t total = (size_t) n_frames * C;
	if (e->pin_in.n < total || e->stage.n < total) {
		HIPCHK (hipStreamSynchronize (st));
		if (e->pin_in.reserve (total) || e->stage.reserve (total)) return fail (MTR_ERR_NOMEM, "staging buffers");
	}
	if (e->pin_state.reserve (1) || e->pin_bank.reserve (2 * MTR_NBANDS)) return fail (MTR_ERR_NOMEM, "hipHostMalloc snapshot");
	float* const il = e->pin_in.p;                 // free: the previous block ended with a wait
	if (C == 2) for (uint32_t i = 0; i < n_frames; ++i) { il[2 * i] = ch[0][i]; il[2 * i + 1] = ch[1][i]; }
	else if (C == 1) memcpy (il, ch[0], (size_t) n_frames * sizeof (float));
	else for (uint32_t i = 0; i < n_frames; ++i) for (uint32_t c = 0; c < C; ++c) il[(size_t) i * C + c] = ch[c][i];
	HIPCHK (hipMemcpyAsync (e->stage.p, il, total * sizeof (float), hipMemcpyHostToDevice, st));
	const int rc = process_call (e, { e->stage.p, n_frames, n_frames, st, 0, 1, nullptr, false, true });
	if (rc) return rc;
	{ const int jrc = join_tail (e, st); if (jrc) return jrc; }     // (a deferred gate — tail mode 2 only, at this size — writes the state copied next)
	HIPCHK (hipMemcpyAsync (e->pin_state.p, e->state.p, sizeof (mtr_stream_state), hipMemcpyDeviceToHost, st));
	if (e->cfg.meters & MTR_METER_SPECTR30) {
		HIPCHK (hipMemcpyAsync (e->pin_bank.p, e->bank_val.p, MTR_NBANDS * sizeof (float), hipMemcpyDeviceToHost, st));
		HIPCHK (hipMemcpyAsync (e->pin_bank.p + MTR_NBANDS, e->bank_max.p, MTR_NBANDS * sizeof (float), hipMemcpyDeviceToHost, st));
	}
	HIPCHK (hipStreamSynchronize (st));
	e->snap_valid = true;
	return MTR_OK;
}

int mtr_engine_prepare_host (mtr_engine* e, uint32_t max_block_frames)
{
	if (!e) return fail (MTR_ERR_ARG, "null engine");
	if (e->cfg.n_streams != 1) return fail (MTR_ERR_ARG, "mtr_engine_prepare_host is for the n_streams == 1 (LV2) path");
	if (max_block_frames == 0) return MTR_OK;
	// one silent block of the largest size: page-locked staging, device buffers, the engine's stream and every kernel's
	// code object exist afterwards (a first launch loads the module: milliseconds); then back to the state of a new engine
	std::vector<float> zeros (max_block_frames, 0.f);
	const float* ch[2] = { zeros.data (), zeros.data () };
	int rc = mtr_engine_process_planar_host (e, ch, max_block_frames);
	if (rc) return rc;
	return mtr_engine_reset (e);
}

int mtr_engine_sync (mtr_engine* e)
{
	if (!e) return fail (MTR_ERR_ARG, "null engine");
	HIPCHK (hipSetDevice (e->cfg.device));
	return sync_all (e);
}

int mtr_engine_set_deferred_tail (mtr_engine* e, int mode)
{
	if (!e || mode < 0 || mode > 2) return fail (MTR_ERR_ARG, "mtr_engine_set_deferred_tail: mode must be 0 (auto), 1 (never) or 2 (always)");
	e->tail_mode = mode;
	return MTR_OK;
}

int mtr_engine_join (mtr_engine* e, void* hip_stream)
{
	if (!e) return fail (MTR_ERR_ARG, "null engine");
	HIPCHK (hipSetDevice (e->cfg.device));
	return join_tail (e, (hipStream_t) hip_stream);
}

int mtr_engine_deferred_stats (mtr_engine* e, uint64_t* calls)
{
	if (!e) return fail (MTR_ERR_ARG, "null engine");
	if (calls) *calls = e->deferred_calls;
	return MTR_OK;
}

static int check_range (mtr_engine* e, uint32_t first, uint32_t count)
{
	if (!e) return fail (MTR_ERR_ARG, "null engine");
	if ((uint64_t) first + count > e->cfg.n_streams) return fail (MTR_ERR_ARG, "stream range out of bounds");
	return MTR_OK;
}

int mtr_engine_results (mtr_engine* e, uint32_t first, uint32_t count, mtr_stream_result* out)
{
	int rc = check_range (e, first, count);
	if (rc) return rc;
	if (!out) return fail (MTR_ERR_ARG, "null output");
	if (count == 0) return MTR_OK;
	// (the one-stream snapshot path — an LV2 run () — touches no heap: the state came back with the block's own wait)
	std::vector<mtr_stream_state> hv;
	const mtr_stream_state* h = nullptr;
	if (e->snap_valid && e->cfg.n_streams == 1) {
		h = e->pin_state.p;
	} else {
		rc = mtr_engine_sync (e);
		if (rc) return rc;
		hv.resize (count);
		HIPCHK (hipMemcpy (hv.data (), e->state.p + first, count * sizeof (mtr_stream_state), hipMemcpyDeviceToHost));
		h = hv.data ();
	}
	for (uint32_t i = 0; i < count; ++i) {
		const mtr_stream_state& s = h[i];
		mtr_stream_result& r = out[i];
		r.loudness_M = s.loud_M; r.maxloudn_M = s.max_M; r.loudness_S = s.loud_S; r.maxloudn_S = s.max_S;
		r.integrated = s.integ; r.integ_thr = s.integ_thr;
		r.range_min = s.rmin; r.range_max = s.rmax; r.range_thr = s.rthr;
		r.hist_M_count = s.cnt_M; r.hist_S_count = s.cnt_S;
		for (int c = 0; c < 2; ++c) {
			r.truepeak[c] = s.tp_hold[c]; r.truepeak_call[c] = s.tp_last[c];
			r.tpb_level[c] = s.tpb_m[c]; r.tpb_peak[c] = s.tpb_p[c];
		}
	}
	return MTR_OK;
}

// TruePeakdsp::read () per channel (src/ebulv2.cc:361-365 for each of n_channels): what the stereo engine reports in
// mtr_stream_result.truepeak / truepeak_call, channel by channel
int mtr_engine_truepeak_channels (mtr_engine* e, uint32_t first, uint32_t count, float* hold, float* last)
{
	int rc = check_range (e, first, count);
	if (rc) return rc;
	if (!hold && !last) return fail (MTR_ERR_ARG, "mtr_engine_truepeak_channels: null outputs");
	if (!(e->cfg.meters & MTR_METER_TRUEPEAK)) return fail (MTR_ERR_ARG, "no TRUEPEAK in this engine");
	if (count == 0) return MTR_OK;
	const size_t C = e->cfg.n_channels;
	if (e->layout != 8) {
		mtr_stream_result* r = new (std::nothrow) mtr_stream_result[count];
		if (!r) return fail (MTR_ERR_NOMEM, "mtr_engine_truepeak_channels");
		rc = mtr_engine_results (e, first, count, r);
		if (rc == MTR_OK)
			for (uint32_t i = 0; i < count; ++i)
				for (size_t c = 0; c < C; ++c) { if (hold) hold[i * C + c] = r[i].truepeak[c]; if (last) last[i * C + c] = r[i].truepeak_call[c]; }
		delete[] r;
		return rc;
	}
	rc = mtr_engine_sync (e);
	if (rc) return rc;
	if (hold) HIPCHK (hipMemcpy (hold, e->mc_tp_hold.p + (size_t) first * C, count * C * sizeof (float), hipMemcpyDeviceToHost));
	if (last) HIPCHK (hipMemcpy (last, e->mc_tp_last.p + (size_t) first * C, count * C * sizeof (float), hipMemcpyDeviceToHost));
	return MTR_OK;
}

int mtr_engine_histograms (mtr_engine* e, uint32_t first, uint32_t count, int32_t* hm, int32_t* hs)
{
	int rc = check_range (e, first, count);
	if (rc) return rc;
	if (count == 0) return MTR_OK;
	rc = mtr_engine_sync (e);
	if (rc) return rc;
	std::vector<int32_t> h ((size_t) count * 2 * MTR_HIST_LEN);
	HIPCHK (hipMemcpy (h.data (), e->hist.p + (size_t) first * 2 * MTR_HIST_LEN, h.size () * 4, hipMemcpyDeviceToHost));
	for (uint32_t i = 0; i < count; ++i) {
		if (hm) memcpy (hm + (size_t) i * MTR_HIST_LEN, &h[(size_t) i * 2 * MTR_HIST_LEN], MTR_HIST_LEN * 4);
		if (hs) memcpy (hs + (size_t) i * MTR_HIST_LEN, &h[(size_t) i * 2 * MTR_HIST_LEN + MTR_HIST_LEN], MTR_HIST_LEN * 4);
	}
	return MTR_OK;
}

int mtr_engine_fragment_powers (mtr_engine* e, uint32_t first, uint32_t count, float* out,
                                uint32_t cap, uint32_t* n_frag)
{
	int rc = check_range (e, first, count);
	if (rc) return rc;
	if (n_frag) *n_frag = e->last_n_frag;
	if (!out || count == 0 || e->last_n_frag == 0) return MTR_OK;
	if (cap < e->last_n_frag) return fail (MTR_ERR_ARG, "capacity_per_stream < n_frag");
	rc = mtr_engine_sync (e);
	if (rc) return rc;
	HIPCHK (hipMemcpy2D (out, (size_t) cap * 4, e->frag_power.p + (size_t) first * e->last_n_frag,
	                     (size_t) e->last_n_frag * 4, (size_t) e->last_n_frag * 4, count, hipMemcpyDeviceToHost));
	return MTR_OK;
}

int mtr_engine_spectrum (mtr_engine* e, uint32_t first, uint32_t count, float* val, float* mx, float* val_db, float* max_db)
{
	int rc = check_range (e, first, count);
	if (rc) return rc;
	if (!(e->cfg.meters & MTR_METER_SPECTR30)) return fail (MTR_ERR_ARG, "no SPECTR30 in this engine");
	if (count == 0) return MTR_OK;
	const size_t n = (size_t) count * MTR_NBANDS;
	std::vector<float> hv;
	const float* v = nullptr; const float* m = nullptr;
	if (e->snap_valid && e->cfg.n_streams == 1) {
		v = e->pin_bank.p; m = e->pin_bank.p + MTR_NBANDS;            // came back with the block's own wait: no heap, no copy
	} else {
		rc = mtr_engine_sync (e);
		if (rc) return rc;
		hv.resize (2 * n);
		HIPCHK (hipMemcpy (hv.data (), e->bank_val.p + (size_t) first * MTR_NBANDS, n * 4, hipMemcpyDeviceToHost));
		HIPCHK (hipMemcpy (hv.data () + n, e->bank_max.p + (size_t) first * MTR_NBANDS, n * 4, hipMemcpyDeviceToHost));
		v = hv.data (); m = hv.data () + n;
	}
	for (size_t i = 0; i < n; ++i) {
		// spectrumlv2.c:240-247.  The stored val carries the +1e-20f of :237; above the -100 dB floor
		// (val > 5e-11) that addition does not change the float, so the port value is unaffected.
		const float vs = sqrtf (2. * v[i]);
		const float ms = sqrtf (2. * m[i]);
		if (val) val[i] = v[i];
		if (mx) mx[i] = m[i];
		if (val_db) val_db[i] = vs > .00001f ? 20.0 * log10f (vs) : -100.0;
		if (max_db) max_db[i] = ms > .00001f ? 20.0 * log10f (ms) : -100.0;
	}
	return MTR_OK;
}

int mtr_engine_aggregate_device (mtr_engine* e, int32_t* d_hist, float* d_max, void* hip_stream)
{
	if (!e || !d_hist || !d_max) return fail (MTR_ERR_ARG, "mtr_engine_aggregate_device: null argument");
	HIPCHK (hipSetDevice (e->cfg.device));
	{ const int jrc = join_tail (e, (hipStream_t) hip_stream); if (jrc) return jrc; }   // behind the deferred gates: it reads what they write
	if (mtr_launch_aggregate (e->state.p, e->hist.p, e->cfg.n_streams, d_hist, d_max, hip_stream))
		return fail (MTR_ERR_HIP, "k_aggregate launch");
	return MTR_OK;
}

int mtr_engine_reduce (mtr_engine* e, mtr_comm* c, int32_t* d_hist, float* d_max, void* hip_stream)
{
	if (!e || !c || !d_hist || !d_max) return fail (MTR_ERR_ARG, "mtr_engine_reduce: null argument");
	{ const int crc = comm_check (c, e->cfg.device); if (crc) return crc; }
	hipStream_t st = (hipStream_t) hip_stream;
	const bool deferred = e->last_deferred && e->tail_stream.v;
	if (deferred) {
		// behind the deferred gate, on the side stream: the aggregate reads what the gate wrote there and what the caller's stream
		// has written up to now (the fold of the call's peaks in k_history); d_hist / d_max are valid after mtr_engine_join /
		// mtr_engine_sync.  The next call's fold waits for ev_red.
		HIPCHK (hipSetDevice (e->cfg.device));
		HIPCHK (hipEventRecord (e->ev_main.v, st));
		HIPCHK (hipStreamWaitEvent (e->tail_stream.v, e->ev_main.v, 0));
		st = e->tail_stream.v;
		e->tail_pending = true;
		if (mtr_launch_aggregate (e->state.p, e->hist.p, e->cfg.n_streams, d_hist, d_max, st)) return fail (MTR_ERR_HIP, "k_aggregate launch");
	} else {
		const int rc = mtr_engine_aggregate_device (e, d_hist, d_max, hip_stream);
		if (rc) return rc;
	}
	{ const int rc = comm_all_reduce (c, d_hist, d_max, st); if (rc) return rc; }
	if (deferred) { HIPCHK (hipEventRecord (e->ev_red.v, st)); e->red_pending = true; }
	return MTR_OK;
}

// ---- per-stream state: checkpoint / resume, re-sharding ----------------------------------------------------------------
} // extern "C"
namespace {

struct StateHeader {
	uint32_t magic, version, header_bytes;
	uint32_t meters, n_channels;
	float    sample_rate;
	uint32_t count, per_stream_bytes, stream_state_bytes;
	// the engine's lock-step cursors
	uint32_t frcnt, integr;
	float    omega;
	uint64_t dr_scnt;
	uint64_t payload_fnv;       // FNV-1a (64 bit) of everything behind the header: a checkpoint file that rotted is refused, not trusted
};
constexpr uint32_t STATE_MAGIC = 0x5352544du;   // "MTRS"
constexpr uint32_t STATE_VERSION = 2;           // 2: + payload_fnv

uint64_t fnv1a64 (const unsigned char* p, size_t n)
{
	uint64_t h = 0xcbf29ce484222325ull;
	for (size_t i = 0; i < n; ++i) { h ^= p[i]; h *= 0x100000001b3ull; }
	return h;
}

struct StateSection { const void* base; size_t elem; };   // a per-stream array: `elem` bytes per stream

// every array a stream carries from call to call, in the blob's order (a function of the configuration alone)
std::vector<StateSection> state_sections (const mtr_engine* e)
{
	std::vector<StateSection> v;
	const uint32_t m = e->cfg.meters;
	v.push_back ({ e->state.p, sizeof (mtr_stream_state) });
	v.push_back ({ e->hist.p, (size_t) 2 * MTR_HIST_LEN * sizeof (int32_t) });
	v.push_back ({ e->fir_hist[e->pos.hist_cur].p, (size_t) MTR_FIR_HALO * 2 * sizeof (float) });
	if (m & MTR_METER_SPECTR30) {
		v.push_back ({ e->bank_z.p, (size_t) MTR_NBANDS * 12 * sizeof (double) });
		v.push_back ({ e->bank_val.p, (size_t) MTR_NBANDS * sizeof (float) });
		v.push_back ({ e->bank_max.p, (size_t) MTR_NBANDS * sizeof (float) });
		v.push_back ({ e->bank_ac[e->pos.bank_ac_cur].p, sizeof (int32_t) });
	}
	if (m & MTR_METER_BITSTATS) v.push_back ({ e->bim.p, sizeof (mtr_bitstats_state) });
	if (m & MTR_METER_SIGDIST) v.push_back ({ e->sdh.p, sizeof (mtr_sigdist_state) });
	if (m & MTR_METER_DR14) {
		v.push_back ({ e->dr_state.p, sizeof (mtr_dr14_state) });
		v.push_back ({ e->dr_hist.p, (size_t) e->cfg.n_channels * MTR_DR_HISTBINS * sizeof (uint32_t) });
	}
	if (m & MTR_METER_KMETER) v.push_back ({ e->km_state.p, 2 * sizeof (mtr_kmeter_state) });
	if (e->layout == 8) {                                      // the per-channel side buffers (stereo blobs are unchanged)
		const size_t C = e->cfg.n_channels;
		v.push_back ({ e->mc_kz.p, C * 4 * sizeof (float) });
		v.push_back ({ e->mc_hist[e->pos.hist_cur].p, (size_t) MTR_FIR_HALO * C * sizeof (float) });
		v.push_back ({ e->mc_tp_last.p, C * sizeof (float) });
		v.push_back ({ e->mc_tp_hold.p, C * sizeof (float) });
	}
	// (the LAST section, and only of an engine with the bit: every other blob is byte for byte what it was.  The header has no room
	// for the period and the frames into the open one: they travel in every stream's mtr_stcorr_state, written by the export)
	if (m & MTR_METER_STCORR) v.push_back ({ e->sc_state.p, sizeof (mtr_stcorr_state) });
	return v;
}

size_t state_per_stream (const mtr_engine* e)
{
	size_t n = 0;
	for (const StateSection& s : state_sections (e)) n += s.elem;
	return n;
}

}  // namespace
extern "C" {

size_t mtr_engine_state_bytes (const mtr_engine* e, uint32_t count)
{
	if (!e) return 0;
	return sizeof (StateHeader) + (size_t) count * state_per_stream (e);
}

uint32_t mtr_state_blob_count (const void* blob, size_t bytes)
{
	StateHeader h;
	if (!blob || bytes < sizeof (h)) return 0;
	memcpy (&h, blob, sizeof (h));
	if (h.magic != STATE_MAGIC || h.version != STATE_VERSION || h.header_bytes != sizeof (h)) return 0;
	if (bytes < sizeof (h) + (size_t) h.count * h.per_stream_bytes) return 0;
	return h.count;
}

int mtr_engine_state_export (mtr_engine* e, uint32_t first, uint32_t count, void* blob, size_t capacity)
{
	int rc = check_range (e, first, count);
	if (rc) return rc;
	if (!blob) return fail (MTR_ERR_ARG, "mtr_engine_state_export: null blob");
	const size_t need = mtr_engine_state_bytes (e, count);
	if (capacity < need) return fail (MTR_ERR_ARG, "mtr_engine_state_export: capacity < mtr_engine_state_bytes ()");
	rc = mtr_engine_sync (e);
	if (rc) return rc;
	StateHeader h;
	memset (&h, 0, sizeof (h));
	h.magic = STATE_MAGIC; h.version = STATE_VERSION; h.header_bytes = sizeof (h);
	h.meters = e->cfg.meters; h.n_channels = e->cfg.n_channels; h.sample_rate = e->cfg.sample_rate;
	h.count = count; h.per_stream_bytes = (uint32_t) state_per_stream (e); h.stream_state_bytes = sizeof (mtr_stream_state);
	h.frcnt = e->pos.frcnt; h.integr = e->integr ? 1u : 0u; h.omega = e->omega; h.dr_scnt = e->pos.dr_scnt;
	unsigned char* const o0 = static_cast<unsigned char*> (blob) + sizeof (h);
	unsigned char* o = o0;
	for (const StateSection& s : state_sections (e)) {
		if (count) HIPCHK (hipMemcpy (o, static_cast<const unsigned char*> (s.base) + (size_t) first * s.elem, (size_t) count * s.elem, hipMemcpyDeviceToHost));
		o += (size_t) count * s.elem;
	}
	if (e->cfg.meters & MTR_METER_STCORR)
		for (uint32_t k = 0; k < count; ++k) {                   // the host's cursors, not whatever the device copy holds
			mtr_stcorr_state v;
			unsigned char* const at = o - (size_t) (count - k) * sizeof (v);
			memcpy (&v, at, sizeof (v));
			v.period = e->sc_period; v.fill = (uint32_t) e->pos.sc_fill;
			memcpy (at, &v, sizeof (v));
		}
	h.payload_fnv = fnv1a64 (o0, (size_t) (o - o0));
	memcpy (blob, &h, sizeof (h));
	return MTR_OK;
}

int mtr_engine_state_import (mtr_engine* e, uint32_t first, const void* blob, size_t bytes)
{
	if (!e || !blob) return fail (MTR_ERR_ARG, "mtr_engine_state_import: null argument");
	StateHeader h;
	if (bytes < sizeof (h)) return fail (MTR_ERR_STATE, "mtr_engine_state_import: not a state blob (too short)");
	memcpy (&h, blob, sizeof (h));
	if (h.magic != STATE_MAGIC) return fail (MTR_ERR_STATE, "mtr_engine_state_import: not a state blob (magic)");
	if (h.version != STATE_VERSION || h.header_bytes != sizeof (h)) return fail (MTR_ERR_STATE, "mtr_engine_state_import: blob of another format version");
	if (h.meters != e->cfg.meters || h.n_channels != e->cfg.n_channels || h.sample_rate != e->cfg.sample_rate)
		return fail (MTR_ERR_STATE, "mtr_engine_state_import: the blob comes from another configuration (meters, channels or sample rate)");
	if (h.stream_state_bytes != sizeof (mtr_stream_state) || h.per_stream_bytes != state_per_stream (e))
		return fail (MTR_ERR_STATE, "mtr_engine_state_import: the blob's per-stream layout is not this build's");
	if (bytes < sizeof (h) + (size_t) h.count * h.per_stream_bytes) return fail (MTR_ERR_STATE, "mtr_engine_state_import: truncated blob");
	int rc = check_range (e, first, h.count);
	if (rc) return rc;
	// the cursors go straight into the tiling of the next call, the payload's ring indices and counters into the kernels:
	// nothing of a blob is trusted before it has been checked
	if (h.frcnt == 0 || h.frcnt > e->fragm) return fail (MTR_ERR_STATE, "mtr_engine_state_import: corrupt blob (frames left in the open fragment)");
	if (h.integr > 1 || !(h.omega > 0.f && h.omega < 1.f)) return fail (MTR_ERR_STATE, "mtr_engine_state_import: corrupt blob (integration flag / bank speed)");
	if (h.dr_scnt > (uint64_t) rintf (e->cfg.sample_rate * 3.0f)) return fail (MTR_ERR_STATE, "mtr_engine_state_import: corrupt blob (open DR-14 window)");
	const unsigned char* const i0 = static_cast<const unsigned char*> (blob) + sizeof (h);
	if (fnv1a64 (i0, (size_t) h.count * h.per_stream_bytes) != h.payload_fnv) return fail (MTR_ERR_STATE, "mtr_engine_state_import: corrupt blob (checksum of the payload)");
	// the streams of an engine advance in lock step: a fresh engine takes the blob's cursors — integration on / off and the bank's
	// speed included, whatever integr_start / spectr_set_speed said before: they are part of where the streams stand — any other
	// must stand at the same ones
	const bool fresh = !e->advanced;
	uint32_t sc_period = e->sc_period, sc_fill = (uint32_t) e->pos.sc_fill;
	if ((e->cfg.meters & MTR_METER_STCORR) && h.count) {
		const unsigned char* const sec = i0 + (size_t) h.count * (h.per_stream_bytes - sizeof (mtr_stcorr_state));
		for (uint32_t k = 0; k < h.count; ++k) {
			mtr_stcorr_state v;
			memcpy (&v, sec + (size_t) k * sizeof (v), sizeof (v));
			if (k == 0) { sc_period = v.period; sc_fill = v.fill; }
			if (v.period != sc_period || v.fill != sc_fill || (sc_period ? sc_fill >= sc_period || sc_period < (uint32_t) e->cfg.sample_rate / 20 : sc_fill != 0))
				return fail (MTR_ERR_STATE, "mtr_engine_state_import: corrupt blob (period of the STCORR series)");
		}
		if (!fresh && (sc_period != e->sc_period || sc_fill != e->pos.sc_fill))
			return fail (MTR_ERR_STATE, "mtr_engine_state_import: the engine does not stand where the blob's streams do (period of the STCORR series)");
	}
	if (!fresh && (e->pos.frcnt != h.frcnt || e->integr != (h.integr != 0) || e->omega != h.omega || e->pos.dr_scnt != h.dr_scnt))
		return fail (MTR_ERR_STATE, "mtr_engine_state_import: the engine does not stand where the blob's streams do (fragment phase, integration, bank speed or DR-14 window)");
	rc = mtr_engine_sync (e);
	if (rc) return rc;
	e->snap_valid = false;
	const unsigned char* i = i0;
	for (const StateSection& s : state_sections (e)) {
		if (h.count) HIPCHK (hipMemcpy (const_cast<unsigned char*> (static_cast<const unsigned char*> (s.base)) + (size_t) first * s.elem, i, (size_t) h.count * s.elem, hipMemcpyHostToDevice));
		i += (size_t) h.count * s.elem;
	}
	for (uint32_t k = 0; k < h.count; ++k) {                     // (an imported stream is open — closure is not part of the blob — and
		if (e->closed[first + k]) { e->closed[first + k] = 0; e->n_closed--; }   // its count starts again: the blob does not carry one)
		e->metered[first + k] = 0;
	}
	if (fresh) {                                                 // (only now: a failed sync or copy has not moved the engine)
		e->pos.frcnt = h.frcnt; e->integr = h.integr != 0; e->omega = h.omega; e->pos.dr_scnt = h.dr_scnt;
		e->sc_period = sc_period; e->pos.sc_fill = sc_fill;
		e->plan.valid = false;
		e->advanced = true;
	}
	return MTR_OK;
}

int mtr_engine_layout (const mtr_engine* e) { return e ? (e->seg_ok ? 7 : e->layout) : MTR_ERR_ARG; }

int mtr_engine_seg_stats (mtr_engine* e, uint64_t* calls, uint64_t* frames)
{
	if (!e) return fail (MTR_ERR_ARG, "null engine");
	if (calls) *calls = e->pos.seg_calls;
	if (frames) *frames = e->pos.seg_frames;
	return MTR_OK;
}

static int drain_prune_counters (mtr_engine* e)
{
	if (!e) return fail (MTR_ERR_ARG, "null engine");
	int rc = mtr_engine_sync (e);
	if (rc) return rc;
	uint32_t h[4];
	HIPCHK (hipMemcpy (h, e->prune_cnt.p, 16, hipMemcpyDeviceToHost));
	HIPCHK (hipMemset (e->prune_cnt.p, 0, 16));      // 32-bit device counters are drained into 64-bit totals
	for (int i = 0; i < 4; ++i) e->prune_tot[i] += h[i];
	return MTR_OK;
}

int mtr_engine_prune_stats (mtr_engine* e, uint64_t* considered, uint64_t* skipped)
{
	int rc = drain_prune_counters (e);
	if (rc) return rc;
	if (considered) *considered = e->prune_tot[0];
	if (skipped) *skipped = e->prune_tot[1];
	return MTR_OK;
}

int mtr_engine_refine_stats (mtr_engine* e, uint64_t* screened, uint64_t* completed)
{
	int rc = drain_prune_counters (e);
	if (rc) return rc;
	if (screened) *screened = e->prune_tot[2];
	if (completed) *completed = e->prune_tot[3];
	return MTR_OK;
}

int mtr_engine_timing_enable (mtr_engine* e, int on)
{
	if (!e) return fail (MTR_ERR_ARG, "null engine");
	e->timing = on != 0;
	e->timed_calls = 0;
	return MTR_OK;
}

int mtr_engine_timing_query (mtr_engine* e, float* ms_fused, float* ms_gate, float* ms_bank, uint32_t* calls)
{
	if (!e) return fail (MTR_ERR_ARG, "null engine");
	int rc = mtr_engine_sync (e);
	if (rc) return rc;
	float f = 0, g = 0, b = 0;
	for (uint32_t i = 0; i < e->timed_calls && (size_t) i * EV_PER_CALL + EV_PER_CALL - 1 < e->ev.size (); ++i) {
		float t;
		const Event* const v = &e->ev[(size_t) i * EV_PER_CALL];
		if (hipEventElapsedTime (&t, v[0].v, v[1].v) == hipSuccess) f += t;
		if (hipEventElapsedTime (&t, v[2].v, v[3].v) == hipSuccess) g += t;
		if (hipEventElapsedTime (&t, v[4].v, v[5].v) == hipSuccess) b += t;
	}
	if (ms_fused) *ms_fused = f;
	if (ms_gate) *ms_gate = g;
	if (ms_bank) *ms_bank = b;
	if (calls) *calls = e->timed_calls;
	e->timed_calls = 0;
	return MTR_OK;
}

int mtr_engine_timing_calls (mtr_engine* e, float* out, uint32_t cap, uint32_t* calls)
{
	if (!e || (!out && cap)) return fail (MTR_ERR_ARG, "mtr_engine_timing_calls: null argument");
	int rc = mtr_engine_sync (e);
	if (rc) return rc;
	if (calls) *calls = e->timed_calls;
	for (uint32_t i = 0; i < e->timed_calls && i < cap && (size_t) i * EV_PER_CALL + EV_PER_CALL - 1 < e->ev.size (); ++i) {
		float* o = out + (size_t) i * 4;
		const Event* const v = &e->ev[(size_t) i * EV_PER_CALL];
		for (int k = 0; k < 3; ++k)
			if (hipEventElapsedTime (&o[k], v[2 * k].v, v[2 * k + 1].v) != hipSuccess) o[k] = 0.f;
		const int first = i < e->ev_decode.size () && e->ev_decode[i] ? 6 : 0;        // (a PCM chunk's span holds its decode)
		if (hipEventElapsedTime (&o[3], v[first].v, v[5].v) != hipSuccess) o[3] = 0.f;     // (on the caller's stream: a deferred gate is not in it)
	}
	return MTR_OK;
}

int mtr_synth_fill_device (float* d_audio, uint32_t n_streams, uint64_t n_frames, uint64_t stride,
                           uint32_t seed, float fs, int kind, void* hip_stream)
{
	if (!d_audio || stride < n_frames) return fail (MTR_ERR_ARG, "mtr_synth_fill_device");
	if (n_frames == 0 || n_streams == 0) return MTR_OK;
	if (mtr_launch_synth (d_audio, n_streams, n_frames, stride, seed, fs, kind, hip_stream)) return fail (MTR_ERR_HIP, "k_synth launch");
	return MTR_OK;
}

} // extern "C"
