// mtr_dr14.hip — DR-14 (the dr14 plugins' dynamic-range meter) for a whole batch of tracks (gfx950).
//
// Replaces the dr_operation_mode part of dr14_run (src/dr14.c:394-412: per sample rms_sum += v*v and
// peak_cur = max (peak_cur, v), a window closed every n_sample_cnt + 1 samples) and dr14_calc_rms_score
// (src/dr14.c:283-352: silent windows dropped, the window's RMS into an 8000-bin histogram of 0.01 dB, the
// two highest window peaks, the score = RMS of the loudest 20 % of the windows).  The true-peak and K-meter
// halves of the plugin are MTR_METER_TPBALLIST and host plumbing (lv2_dr14.c).
//
// A window is 3 s: the per-sample part is a pure streaming reduction (HBM-bound), so the call is cut at the
// window boundaries and one workgroup reduces one (stream, piece); a second, tiny kernel walks each stream's
// pieces in order, closes the windows and, at the end of the call, evaluates the score from the histogram
// exactly as the reference does after its last window.  The reference sums the squares sequentially in f32;
// here the partial sums are double (closer to the true value): a window's RMS can land in the neighbouring
// 0.01 dB bin, which moves the score by at most that — tests/test_gpu_dr14.py states +-0.01 dB (DR_TOL).  Where both sums put every
// window into the same bin the score is the reference's to 1e-4 dB and the histogram and the window peaks are exact:
// tests/test_gpu_dr14_score.py (many windows, window and call edges, the histogram's ends, the second-highest peak).
//
// LEN (both kernels): the call carries per-stream ends (a.ends, call-relative: mtr_engine_process_*_tracks, or any call once a stream of
// its view is closed).  Stream s ends at frame E = ends [s], workgroup-uniform (one scalar load): its pieces end at min (b1, E), its
// windows are (dr_scnt + E) / W, and the window E falls into stays open in the state, as the reference leaves it when run () is no
// longer called.  A workgroup of k_dr14_sums whose piece starts at or past E returns before it touches memory and writes NO piece slot:
// k_dr14_windows walks the stream's own pieces only — it never reads those slots.  E = 0 (a closed stream, frames [s] == 0): both
// kernels return at once, the state keeps every bit.  E moves the tail of a piece, never its start: the 16-byte path's parity handling
// is the dense one's.  The dense instantiations are the kernels as they always were.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <type_traits>
#include <vector>

#include "mtr_engine_impl.h"

/* DR-14 per-stream state (src/dr14.c LV2dr14: rms_sum, peak_cur, peak_hist, m_rms, m_peak, num_fragments) */
typedef struct mtr_dr14_state {
	float    rms_sum[2], peak_cur[2], peak_hist[2][2], m_rms[2], m_peak[2];
	uint32_t num_fragments;
} mtr_dr14_state;

typedef struct mtr_dr14_args {
	const float*    audio;        /* [S][stride][C] */
	uint64_t        stride, n_frames;
	uint64_t        window;       /* n_sample_cnt + 1 samples close a window (dr14.c:404) */
	uint64_t        e0;           /* call frame at which the window open on entry closes */
	uint32_t        n_streams, n_channels, n_pieces, n_windows;
	mtr_dr14_state* state;        /* [S] */
	uint32_t*       hist;         /* [S][C][8000] */
	double*         piece_sum;    /* [S][n_pieces][2] */
	float*          piece_peak;   /* [S][n_pieces][2] */
	const uint32_t* ends;         /* [S] per-stream ends of a ragged call (the LEN instantiations), NULL on a dense one */
} mtr_dr14_args;

namespace {

constexpr int NT = 256;

__device__ __forceinline__ float coeff_to_db (float c) { return c < .0001f ? -80.f : 20.f * log10f (c); }   // dr14.c:235-238
__device__ __forceinline__ float db_to_coeff (float db) { return db <= -80.f ? 0.f : powf (10.f, 0.05f * db); } // dr14.c:240-243

// piece i of a call: frames [b (i), b (i + 1)), b (0) = 0, b (i) = min (N, e0 + (i - 1) W), e0 = W - c_in
__device__ __forceinline__ uint64_t piece_start (uint32_t i, uint64_t e0, uint64_t W, uint64_t N)
{
	if (i == 0) return 0;
	const uint64_t b = e0 + (uint64_t) (i - 1) * W;
	return b < N ? b : N;
}

template <int C, bool LEN>
__global__ __launch_bounds__ (NT) void k_dr14_sums (const mtr_dr14_args a)
{
	const uint32_t piece = blockIdx.x, s = blockIdx.y;
	uint64_t N = a.n_frames;
	if constexpr (LEN) {
		N = a.ends[s];
		if (N == 0 || (piece > 0 && a.e0 + (uint64_t) (piece - 1) * a.window >= N)) return;   // not one of the stream's own pieces
	}
	const uint64_t b0 = piece_start (piece, a.e0, a.window, N), b1 = piece_start (piece + 1, a.e0, a.window, N);
	const float* const src = a.audio + (size_t) s * a.stride * C;
	double sl = 0, sr = 0;
	float pl = 0.f, pr = 0.f;                                  // dr14.c:401: max (peak_cur, v), signed v, from 0
	if (C == 2) {
		// 16-byte loads: two frames per lane; a piece that starts on an odd frame of the buffer gives its first
		// frame (and one that ends on an odd frame its last) to a single lane
		const uint64_t odd = ((size_t) s * a.stride + b0 + (reinterpret_cast<size_t> (a.audio) >> 3)) & 1;
		const uint64_t h0 = b0 + (odd && b0 < b1 ? 1 : 0);
		const uint64_t np = (b1 - h0) >> 1;                    // whole pairs
		auto one = [&] (uint64_t f) {
			const float2 v = *reinterpret_cast<const float2*> (src + 2 * f);
			sl += (double) (v.x * v.x); sr += (double) (v.y * v.y);
			pl = fmaxf (pl, v.x); pr = fmaxf (pr, v.y);
		};
		if (threadIdx.x == 0 && h0 > b0) one (b0);
		if (threadIdx.x == 1 && h0 + 2 * np < b1) one (b1 - 1);
		const float4* const p4 = reinterpret_cast<const float4*> (src + 2 * h0);
		for (uint64_t i = threadIdx.x; i < np; i += NT) {
			const float4 v = p4[i];
			sl += (double) (v.x * v.x) + (double) (v.z * v.z); sr += (double) (v.y * v.y) + (double) (v.w * v.w);
			pl = fmaxf (pl, fmaxf (v.x, v.z)); pr = fmaxf (pr, fmaxf (v.y, v.w));
		}
	} else {
		for (uint64_t f = b0 + threadIdx.x; f < b1; f += NT) {
			const float v = src[f];
			sl += (double) (v * v);
			pl = fmaxf (pl, v);
		}
	}
	__shared__ double sh_s[2][NT / 64];
	__shared__ float sh_p[2][NT / 64];
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) {
		sl += __shfl_xor (sl, d, 64); sr += __shfl_xor (sr, d, 64);
		pl = fmaxf (pl, __shfl_xor (pl, d, 64)); pr = fmaxf (pr, __shfl_xor (pr, d, 64));
	}
	const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
	if (lane == 0) { sh_s[0][wid] = sl; sh_s[1][wid] = sr; sh_p[0][wid] = pl; sh_p[1][wid] = pr; }
	__syncthreads ();
	if (threadIdx.x == 0) {
		for (int w = 1; w < NT / 64; ++w) { sl += sh_s[0][w]; sr += sh_s[1][w]; pl = fmaxf (pl, sh_p[0][w]); pr = fmaxf (pr, sh_p[1][w]); }
		const size_t o = ((size_t) s * a.n_pieces + piece) * 2;
		a.piece_sum[o] = sl; a.piece_sum[o + 1] = sr;
		a.piece_peak[o] = pl; a.piece_peak[o + 1] = pr;
	}
}

// one WAVE per stream: lane 0 does the window bookkeeping of dr14_calc_rms_score over this call's pieces (a
// handful of windows), all 64 lanes look for the occupied histogram bins of the score (one thread walking
// 8000 bins per channel took 0.37 ms for 8192 streams)
template <int C, bool LEN>
__global__ __launch_bounds__ (64) void k_dr14_windows (const mtr_dr14_args a)
{
	const uint32_t s = blockIdx.x;
	const int lane = threadIdx.x;
	uint32_t n_pieces = a.n_pieces, n_windows = a.n_windows;        // the stream's own (LEN), the call's otherwise
	if constexpr (LEN) {
		const uint64_t E = a.ends[s];
		if (E == 0) return;
		const uint64_t tot = a.window - a.e0 + E;                  // dr_scnt + E
		n_windows = (uint32_t) (tot / a.window);
		n_pieces = n_windows + (tot % a.window ? 1 : 0);
	}
	__shared__ bool st_closed;
	if (lane == 0) {
	mtr_dr14_state* const st = a.state + s;
	uint32_t* const hist = a.hist + (size_t) s * C * MTR_DR_HISTBINS;
	float rs[2] = { st->rms_sum[0], st->rms_sum[1] };
	float pk[2] = { st->peak_cur[0], st->peak_cur[1] };
	const float nsc = (float) (a.window - 1);                  // n_sample_cnt
	bool closed = false;
	for (uint32_t i = 0; i < n_pieces; ++i) {
		const size_t o = ((size_t) s * a.n_pieces + i) * 2;
		for (int c = 0; c < C; ++c) {
			rs[c] = (float) ((double) rs[c] + a.piece_sum[o + c]);
			pk[c] = fmaxf (pk[c], a.piece_peak[o + c]);
		}
		if (i >= n_windows) break;                           // the last piece leaves an open window
		// ---- a window closes (dr14.c:283-352) ----
		bool silent = true;
		for (int c = 0; c < C; ++c) if (rs[c] > 1e-9 * (double) nsc) silent = false;    // :290 (float > double product)
		if (!silent) {
			st->num_fragments++;
			closed = true;
			for (int c = 0; c < C; ++c) {
				const float rms = sqrtf (2.f * rs[c] / nsc);
				int bin = (int) rintf (100.f * (80.f + coeff_to_db (rms))) - 1;
				if (bin >= MTR_DR_HISTBINS) bin = MTR_DR_HISTBINS - 1;
				if (bin > 0) hist[c * MTR_DR_HISTBINS + bin]++;
				if (pk[c] >= st->peak_hist[c][0]) { st->peak_hist[c][1] = st->peak_hist[c][0]; st->peak_hist[c][0] = pk[c]; }
				else if (pk[c] > st->peak_hist[c][1]) st->peak_hist[c][1] = pk[c];
				pk[c] = 0.f;
			}
		}
		for (int c = 0; c < C; ++c) rs[c] = 0.f;               // silent windows keep their peak (dr14.c:296-301)
	}
	for (int c = 0; c < C; ++c) { st->rms_sum[c] = rs[c]; st->peak_cur[c] = pk[c]; }
	st_closed = closed;
	}
	// (lane 0's stores to the histogram are visible to the wave after this)
	__threadfence_block ();
	const bool closed = __builtin_amdgcn_readfirstlane ((int) st_closed) != 0;
	if (!closed) return;
	// the score after the call's last window: bins from the top, 64 at a time, in descending order
	mtr_dr14_state* const st = a.state + s;
	const uint32_t* const hist = a.hist + (size_t) s * C * MTR_DR_HISTBINS;
	const uint32_t nf = st->num_fragments;
	const float cutf = floorf (nf / 5.0f);
	const uint32_t m_cut = cutf > 1 ? (uint32_t) cutf : 1;
	for (int c = 0; c < C; ++c) {
		uint32_t n_cut = 0;
		float score = 0.f;
		if (nf > 2) {
			for (int top = MTR_DR_HISTBINS - 1; top > 0 && n_cut < m_cut; top -= 64) {
				const int b = top - lane;                          // lane 0 holds the highest bin of the chunk
				const uint32_t bc = b > 0 ? hist[c * MTR_DR_HISTBINS + b] : 0u;
				unsigned long long occupied = __ballot (bc != 0);
				while (occupied && n_cut < m_cut) {                // wave-uniform walk over the occupied bins
					const int l = __ffsll ((long long) occupied) - 1;
					occupied &= occupied - 1;
					const uint32_t cnt = (uint32_t) __builtin_amdgcn_readlane ((int) bc, l);
					const float cd = db_to_coeff ((float) ((top - l - MTR_DR_HISTBINS + 1) / 100.0));
					score += cd * cd * (float) cnt;
					n_cut += cnt;
				}
			}
		}
		if (lane == 0) {
			st->m_rms[c] = n_cut > 0 ? coeff_to_db (sqrtf (score / n_cut)) : -81.f;
			st->m_peak[c] = nf > 2 ? coeff_to_db (st->peak_hist[c][1]) : -81.f;
		}
	}
}

}  // namespace

static int mtr_launch_dr14 (const mtr_dr14_args& a, void* stream)
{
	hipStream_t st = (hipStream_t) stream;
	// (n_channels, per-stream ends or none) to the kernels' template arguments, once
	const auto launch = [&] (auto C, auto LEN) {
		hipLaunchKernelGGL ((k_dr14_sums<C.value, LEN.value>), dim3 (a.n_pieces, a.n_streams), dim3 (NT), 0, st, a);
		hipLaunchKernelGGL ((k_dr14_windows<C.value, LEN.value>), dim3 (a.n_streams), dim3 (64), 0, st, a);
	};
	using One = std::integral_constant<int, 1>;
	using Two = std::integral_constant<int, 2>;
	if (a.n_channels == 2) { if (a.ends) launch (Two {}, std::true_type {}); else launch (Two {}, std::false_type {}); }
	else                   { if (a.ends) launch (One {}, std::true_type {}); else launch (One {}, std::false_type {}); }
	return hipGetLastError () == hipSuccess ? 0 : -1;
}

// ---- DR14 in the engine: the call's step, the blob's sections, reset, the results ------------------------------------------------------

static int dr14_step (mtr_engine* e, const Call& c, Cursors& nx, const StreamEnds& se)
{
	const size_t vo = c.off;
	mtr_dr14_args da;
	da.audio = c.audio; da.stride = c.stride; da.n_frames = c.n_frames;
	da.window = (uint64_t) rintf (e->cfg.sample_rate * 3.0f) + 1;       // dr14.c:155, :404
	da.e0 = da.window - e->pos.dr_scnt;
	const uint64_t tot = e->pos.dr_scnt + c.n_frames;
	da.n_windows = (uint32_t) (tot / da.window);
	da.n_pieces = da.n_windows + (tot % da.window ? 1 : 0);
	da.n_streams = c.cnt; da.n_channels = e->cfg.n_channels; da.ends = se.ends;
	if (e->dr.sum.reserve ((size_t) e->cfg.n_streams * da.n_pieces * 2) || e->dr.peak.reserve ((size_t) e->cfg.n_streams * da.n_pieces * 2))
		return fail (MTR_ERR_NOMEM, "hipMalloc DR14 pieces");
	da.state = e->dr.state.p + vo; da.hist = e->dr.hist.p + vo * e->cfg.n_channels * MTR_DR_HISTBINS;
	da.piece_sum = e->dr.sum.p + vo * da.n_pieces * 2; da.piece_peak = e->dr.peak.p + vo * da.n_pieces * 2;
	if (mtr_launch_dr14 (da, c.st)) return fail (MTR_ERR_HIP, "k_dr14 launch");
	nx.dr_scnt = tot % da.window;
	return MTR_OK;
}

static void dr14_sections (const mtr_engine* e, std::vector<StateSection>& v)
{
	v.push_back ({ e->dr.state.p, sizeof (mtr_dr14_state) });
	v.push_back ({ e->dr.hist.p, (size_t) e->cfg.n_channels * MTR_DR_HISTBINS * sizeof (uint32_t) });
}

constinit SideMeter dr14_meter = { .bits = MTR_METER_DR14, .reset = mtr_engine_dr14_reset, .step = dr14_step, .sections = dr14_sections };

extern "C" {

int mtr_engine_dr14_reset (mtr_engine* e)
{
	if (!e || !(e->cfg.meters & MTR_METER_DR14)) return fail (MTR_ERR_ARG, "no DR14 in this engine");
	e->snap_valid = false;
	HIPCHK (hipSetDevice (e->cfg.device));
	const uint32_t S = e->cfg.n_streams;
	if (e->dr.state.reserve (S) || e->dr.hist.reserve ((size_t) S * e->cfg.n_channels * MTR_DR_HISTBINS))
		return fail (MTR_ERR_NOMEM, "hipMalloc DR14 state");
	std::vector<mtr_dr14_state> h (S);
	memset (h.data (), 0, S * sizeof (mtr_dr14_state));
	for (auto& v : h) for (int c = 0; c < 2; ++c) { v.m_rms[c] = -81.f; v.m_peak[c] = -81.f; }   // dr14.c:247-248
	HIPCHK (hipStreamSynchronize (e->last_stream));
	HIPCHK (hipMemcpy (e->dr.state.p, h.data (), S * sizeof (mtr_dr14_state), hipMemcpyHostToDevice));
	HIPCHK (hipMemset (e->dr.hist.p, 0, (size_t) S * e->cfg.n_channels * MTR_DR_HISTBINS * sizeof (uint32_t)));
	e->pos.dr_scnt = 0;
	return MTR_OK;
}

int mtr_engine_dr14_results (mtr_engine* e, uint32_t first, uint32_t count, mtr_dr14_result* out)
{
	int rc = meter_range (e, e && out && (e->cfg.meters & MTR_METER_DR14), "no DR14 in this engine", first, count);
	if (rc || (rc = wait_stream (e))) return rc;
	std::vector<mtr_dr14_state> h (count);
	HIPCHK (hipMemcpy (h.data (), e->dr.state.p + first, count * sizeof (mtr_dr14_state), hipMemcpyDeviceToHost));
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

} // extern "C"
