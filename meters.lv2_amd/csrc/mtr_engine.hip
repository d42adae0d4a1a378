// mtr_engine.hip — the engine itself: the error path, create / destroy / reset, the call's tail on the side stream, and the getters of
// the EBU R128 / true-peak state (part of the C ABI of include/mtr_engine.h).
//
// Owns device state for `n_streams` lock-step streams (struct mtr_engine: mtr_engine_impl.h).  A process call is mtr_call.hip's, the
// state blob mtr_state.hip's, a side meter's host code is in the file of its kernels.  There is no CPU fallback anywhere in the host
// code: without a HIP device create() fails.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "mtr_engine_impl.h"
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
		// (behind the twelve: the three core fragments of k_seg's core screen, which alone reads them)
		std::vector<uint16_t> a16 (MTR_M16_A_HALVES + MTR_M16_CORE_HALVES);
		mtr_m16_build_a (&g[0][0], a16.data ());
		mtr_m16_build_core (&g[0][0], a16.data () + MTR_M16_A_HALVES);
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
int join_tail (mtr_engine* e, hipStream_t st)
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
int sync_all (mtr_engine* e)
{
	HIPCHK (hipStreamSynchronize (e->last_stream));
	if (e->tail_stream.v && e->tail_pending) {
		HIPCHK (hipStreamSynchronize (e->tail_stream.v));
		e->tail_pending = false; e->gate_pending[0] = e->gate_pending[1] = false; e->red_pending = false;
	}
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

int check_range (mtr_engine* e, uint32_t first, uint32_t count)
{
	if (!e) return fail (MTR_ERR_ARG, "null engine");
	if ((uint64_t) first + count > e->cfg.n_streams) return fail (MTR_ERR_ARG, "stream range out of bounds");
	return MTR_OK;
}

int meter_range (const mtr_engine* e, bool has, const char* none, uint32_t first, uint32_t count)
{
	if (!has) return fail (MTR_ERR_ARG, none);
	if ((uint64_t) first + count > e->cfg.n_streams) return fail (MTR_ERR_ARG, "stream range");
	return MTR_OK;
}

int wait_stream (mtr_engine* e)
{
	HIPCHK (hipSetDevice (e->cfg.device));
	HIPCHK (hipStreamSynchronize (e->last_stream));
	return MTR_OK;
}

int series_configure_check (const mtr_engine* e, const char* who, uint32_t period, uint32_t min_period, const char* min_text)
{
	char text[160];
	if (period && (period < min_period || period >= 0x7fffffffu)) {
		snprintf (text, sizeof (text), "%s: a period is 0 or at least %s frames", who, min_text);
		return fail (MTR_ERR_ARG, text);
	}
	if (e->advanced) {
		snprintf (text, sizeof (text), "%s: only on an engine that has processed nothing since create / reset", who);
		return fail (MTR_ERR_STATE, text);
	}
	return MTR_OK;
}

int series_ring (DevBuf<float>& ring, size_t n, const char* what)
{
	if (!n) return MTR_OK;
	if (ring.reserve (n)) return fail (MTR_ERR_NOMEM, what);
	HIPCHK (hipMemset (ring.p, 0, n * sizeof (float)));
	return MTR_OK;
}

int series_fetch (float* out, const float* src, size_t width, uint32_t first, uint32_t cap, uint32_t capacity, size_t take, uint32_t count)
{
	HIPCHK (hipMemcpy2D (out, (size_t) capacity * width * sizeof (float), src + (size_t) first * cap * width, (size_t) cap * width * sizeof (float),
	                     take * width * sizeof (float), count, hipMemcpyDeviceToHost));
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

// (for tests/test_seg_core_bound.py, which pins the core fragments k_seg's core screen multiplies with to its own rebuild of them
// from mtr_fir_table: what mtr_m16_build_core makes of the engine's taps, [3][64][8] f16 bit patterns; not part of the ABI header)
extern "C" int mtr_debug_m16_core (uint16_t* out1536)
{
	if (!out1536) return fail (MTR_ERR_ARG, "mtr_debug_m16_core");
	float tab[120], g[3][48];
	mtr_setup_fir_table (tab);
	for (int ph = 1; ph <= 3; ++ph)
		for (int i = 0; i < 48; ++i)
			g[ph - 1][i] = (i < 24) ? tab[24 * ph + i] : tab[24 * (4 - ph) + (47 - i)];
	mtr_m16_build_core (&g[0][0], out1536);
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
	if (cfg->n_channels < 1 || cfg->n_channels > MTR_MAX_ENGINE_CHANNELS) return fail (MTR_ERR_ARG, "n_channels must be 1 .. 5 (6 .. 8: MTR_METER_SURROUND alone)");
	if (cfg->meters & ~(uint32_t) (MTR_METER_EBU | MTR_METER_TRUEPEAK | MTR_METER_SPECTR30 | MTR_METER_TPBALLIST | MTR_METER_BITSTATS
	                               | MTR_METER_SIGDIST | MTR_METER_DR14 | MTR_METER_KMETER | MTR_METER_STCORR | MTR_METER_NEEDLE | MTR_METER_SURROUND | MTR_METER_SCOPE | MTR_METER_GONIO))
		return fail (MTR_ERR_ARG, "unknown bits in the meters mask");
	// 6 .. 8 channels: the surround meter alone (no other meter has a kernel that wide; with EBU / TRUEPEAK it stays the argument
	// error it was: Ebu_r128_proc::MAXCH)
	if (cfg->n_channels > MTR_MAX_CHANNELS && cfg->meters != MTR_METER_SURROUND)
		return fail (MTR_ERR_ARG, "n_channels must be 1 .. 5 (6 .. 8: MTR_METER_SURROUND alone)");
	if (cfg->n_channels < 3 && (cfg->meters & MTR_METER_SURROUND))
		return fail (MTR_ERR_UNSUPPORTED, "SURROUND meters 3 .. 8 channels (stereo: KMETER | STCORR)");
	if (cfg->n_channels == 1 && (cfg->meters & (MTR_METER_EBU | MTR_METER_TRUEPEAK)))
		return fail (MTR_ERR_UNSUPPORTED, "EBU / TRUEPEAK take 2 .. 5 channels, not mono");
	if (cfg->n_channels == 1 && (cfg->meters & MTR_METER_STCORR))
		return fail (MTR_ERR_UNSUPPORTED, "STCORR is the correlation of a stereo pair: n_channels 2");
	if (cfg->n_channels == 1 && (cfg->meters & MTR_METER_SCOPE))
		return fail (MTR_ERR_UNSUPPORTED, "SCOPE is the analysis of a stereo pair: n_channels 2");
	if (cfg->n_channels != 2 && (cfg->meters & MTR_METER_GONIO))
		return fail (MTR_ERR_UNSUPPORTED, "GONIO is the M/S picture of a stereo pair: n_channels 2");
	// 3 .. 5 channels: EBU R128 and true peak (Ebu_r128_proc::init takes up to five, ebumeter/ebu_r128_proc.h:26), and the surround meter
	if (cfg->n_channels > 2 && (cfg->meters & ~(uint32_t) (MTR_METER_EBU | MTR_METER_TRUEPEAK | MTR_METER_SURROUND)))
		return fail (MTR_ERR_UNSUPPORTED, "3 .. 5 channels: only EBU, TRUEPEAK and SURROUND meter them");
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
	// (test knob: 0 = k_seg's dense form, the screened ones' bit-for-bit yardstick; 1 = the screen without the peek, whose completed-chunk
	// counts tests pin; 2 = the screen with the peek — mtr_seg.hip: the stream reference; 3 = rule 2 with the lo words of
	// the split built only where a chunk completes — mtr_seg.hip: LAZY; 4 = form 3 screening with the taps' 32-sample core, three
	// MFMAs per chunk, the default — mtr_seg.hip: CORE; calls with per-stream ends run form 2)
	if (const char* v = getenv ("MTR_SEG_SCREEN")) { const int m = atoi (v); e->seg_screen = m == 0 ? 0u : (m == 2 ? 2u : (m == 3 ? 3u : (m == 4 ? 4u : 1u))); }
	if (const char* v = getenv ("MTR_TAIL_DELAY_US")) e->tail_delay_us = (uint32_t) atoi (v);
	if (const char* v = getenv ("MTR_TAIL_GATE_GRID")) e->tail_gate_grid = (uint32_t) atoi (v);   // (tools/r06_tail_probe.py: the experiment behind the default)
	e->fragm = (uint32_t) ((int) cfg->sample_rate / 20);     // ebu_r128_proc.cc:170
	e->pos.frcnt = e->fragm;
	mtr_setup_kweight (cfg->sample_rate, e->kw);
	(void) mtr_engine_spectr_set_speed (e, 1.0f);              // (spectrumlv2.c:98; every engine has one: a state blob's header carries it)

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
	for (const SideMeter* m : SIDE_METERS)
		if (rc == MTR_OK && (cfg->meters & m->bits) && m->create) rc = m->create (e);
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
	e->pos.frcnt = e->fragm;
	e->integr = false;
	e->advanced = false;
	e->metered.assign (e->cfg.n_streams, 0);                         // (every stream open again)
	e->closed.assign (e->cfg.n_streams, 0);
	e->n_closed = 0;
	e->pos.hist_cur = 0;
	e->last_n_frag = 0;
	e->last_deferred = false;
	for (const SideMeter* m : SIDE_METERS)
		if ((e->cfg.meters & m->bits) && m->reset && (rc = m->reset (e))) return rc;
	if (e->ll.period && (rc = loudlog_reset (e, st))) return rc;
	if (e->il.every) return integlog_reset (e, st);
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
