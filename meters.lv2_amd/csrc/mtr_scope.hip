// mtr_scope.hip — the stereo / frequency scope's and the phase wheel's analysis for a batch (gfx950): MTR_METER_SCOPE.
//
// Replaces process_audio of gui/stereoscope.c:705-741 and gui/phasewheel.c:1307-1339 with the fftx_run under them (gui/fft.c:289-361,
// ft_analyze :163-180, the Hann window of ft_gen_window :122-161).  After every H frames of a stream — counted across the process calls,
// a lock-step cursor — one ANALYSIS runs on the last W frames (zeros in front of the stream's start): window, forward DFT per channel,
// |X|^2 and arg X for the bins 1 .. B - 2 (B = W / 2), then per bin
//     stereoscope:  both powers < 1e-20: lr = .5, level = 0; else lv = max (pL, pR), lr_t = .5 + .5 (sqrt pR - sqrt pL) / sqrt lv,
//                   level += .1 (lv - level) + 1e-20, lr += .1 (lr_t - lr) + 1e-10                 (in the reference's C types)
//     phase wheel:  either power < thresh: phase = 0, plevel = -100; else phase = argR - argL, plevel = max (pL, pR);
//                   peak += .04 (max plevel - peak) + 1e-15, NaN -> 0, at most 1000
//
// ONE workgroup walks ONE stream's analyses of the call in order (the smoothers are serial), bins on lanes:
//   * an interleaved stereo frame is the complex number L + iR: one complex FFT of length W in LDS gives both channels by the
//     even / odd split X_L [k] = (Z [k] + conj Z [W - k]) / 2, X_R [k] = (Z [k] - conj Z [W - k]) / 2i;
//   * the transform is in place, decimation in frequency: radix-4 passes (two radix-2 stages fused: three twiddles w^j, w^2j, w^3j read
//     from a table made on the host in double and rounded once — no sine or cosine is computed here) and one radix-2 pass where log2 W
//     is odd; X [k] ends at slot bitrev (k), the split reads it from there;
//   * LDS slot of element i: i + (i >> 5) + (i >> 10) complex f32 (pad ()): the strided accesses of the late passes and the
//     bit-reversed reads of the split then spread over the banks;
//   * level and lr of the thread's bins stay in registers for the whole call; phase, plevel and the two powers are what the LAST
//     analysis of the call leaves (every analysis overwrites them), so only that one computes atan2f and writes them;
//   * an analysis reads its W frames from the call's buffer, the frames in front of the call from the stream's tail (the last W frames,
//     kept in device memory and rewritten at the end of every call through LDS).  H > W: the frames between two windows are never read.
// Each analysis is a function of its W frames and the carried state alone: the result does not depend on where the calls cut the audio.
//
// The reading series (mtr_scope_series.h; what the GUIs' queue_draw after every analysis shows over time: stereoscope.c:738,
// phasewheel.c:1339): k_scope<LOGW, true>, launched only by an engine with K > 0.  Every K-th analysis, counted from reset, is a POINT: it
// does what otherwise only the call's last analysis does — the second pass over the split with atan2f — and writes the selected fields to
// point p of the stream's rings, [S][cap][B] per field (a thread's bins are t + r NT: a wave's stores are contiguous), if p is below the
// capacity: level and lr from the registers they live in, peak by one thread behind its update, the rest from the pass.  A point is what
// mtr_engine_scope_read answers after that analysis, bins 0 and B - 1 included.  k_scope<LOGW, false> is the kernel as it was: another
// argument struct, no instruction of the series.
//
// Track lengths (mtr_any.h): k_scope<LOGW, SERIES, true>, launched only by a call that carries per-stream ends.  A workgroup is a stream, so
// the stream's end is one scalar: it bounds the analyses, names the stream's own last one and places the tail; see the kernel.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <type_traits>
#include <vector>

#include "mtr_engine_impl.h"

/* what the state blob carries of the engine's cursors and configuration, in front of every stream's arrays (the host's copies rule) */
typedef struct mtr_scope_hdr {
	uint32_t window, hop;
	float    thresh;
	uint32_t fill;                /* frames since the last analysis */
	uint64_t analyses;
} mtr_scope_hdr;

typedef struct mtr_scope_args {
	const float*    audio;        /* [S][stride][2] */
	uint64_t        stride, n_frames;
	uint64_t        first;        /* call frame at which the first analysis of the call ends (exclusive) */
	uint32_t        n_streams, n_an, hop;
	float           thresh;
	const float*    win;          /* [W] */
	const float2*   tw;           /* [W] exp (-2 pi i m / W) */
	float*          tail;         /* [S][W][2] */
	float*          level;        /* [S][B] ... */
	float*          lr;
	float*          phase;
	float*          plevel;
	float*          power_l;
	float*          power_r;
	float*          peak;         /* [S] */
} mtr_scope_args;

// the reading series: what its instantiation of k_scope takes on top — a struct of its own, so that the kernel without a series keeps its
// arguments
typedef struct mtr_scope_series_args : mtr_scope_args {
	float*          ring[7];      /* per field in the order of MTR_SCOPE_F_*: [S][cap][B], peak [S][cap], from the view's first stream; null: not selected */
	uint64_t        point0;       /* the index of the call's first point: min (points since reset, cap) */
	uint32_t        every, since; /* K; analyses since the last point when the call starts, < K */
	uint32_t        cap, fields;
} mtr_scope_series_args;

// per-stream ends (mtr_any.h): what the ENDS instantiations take on top of either struct — again structs of their own, so that the two
// kernels of a dense call keep their arguments
typedef struct mtr_scope_ends_args : mtr_scope_args {
	const uint32_t* ends;         /* [S] call frame at which the stream ends, <= n_frames; 0: closed, nothing of it is touched */
} mtr_scope_ends_args;
typedef struct mtr_scope_series_ends_args : mtr_scope_series_args {
	const uint32_t* ends;
} mtr_scope_series_ends_args;

/* SCOPE's second section of the blob: all of an entry is its host-owned header */
typedef struct mtr_scope_open { uint32_t every, since; } mtr_scope_open;

namespace {

constexpr uint32_t K_MAX = 1u << 20;
constexpr int F_PEAK_AT = 4;      // MTR_SCOPE_F_PEAK's bit: the one ring with one float per point
constexpr uint32_t F_PASS = MTR_SCOPE_F_PHASE | MTR_SCOPE_F_PLEVEL | MTR_SCOPE_F_POWER_L | MTR_SCOPE_F_POWER_R;   // the fields the second pass makes
constexpr uint32_t W_MIN = 256, W_MAX = 16384, W_DEFAULT = 1024;
constexpr uint32_t H_MIN = 64, H_MAX = 1u << 20;

__host__ __device__ constexpr uint32_t pad (uint32_t i) { return i + (i >> 5) + (i >> 10); }
constexpr uint32_t lds_slots (uint32_t W) { return pad (W - 1) + 1; }
constexpr int threads_of (int logw) { return (1 << logw) / 4 < 512 ? (1 << logw) / 4 : 512; }

__device__ __forceinline__ float2 cadd (float2 a, float2 b) { return float2{a.x + b.x, a.y + b.y}; }
__device__ __forceinline__ float2 csub (float2 a, float2 b) { return float2{a.x - b.x, a.y - b.y}; }
__device__ __forceinline__ float2 cmul (float2 a, float2 w) { return float2{a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x}; }

// frame f of the stream as the call sees it: f >= 0 from the call's buffer, f < 0 from the tail (the W frames in front of the call)
template <int W> __device__ __forceinline__ float2 frame_at (const float* src, const float* tail, int64_t f, bool al8)
{
	const float* p = f >= 0 ? src + 2 * f : tail + 2 * ((int64_t) W + f);
	if (al8 || f < 0) return *reinterpret_cast<const float2*> (p);
	return float2{p[0], p[1]};
}

// bin i of both channels from the packed transform (X [k] at slot bitrev (k)): the even / odd split, then ft_analyze's power (fft.c:175)
struct Bin { float lre, lim, rre, rim, pl, pr; };
template <int LOGW> __device__ __forceinline__ Bin bin_of (const float2* z, uint32_t i)
{
	const float2 zi = z[pad (__brev (i) >> (32 - LOGW))], zc = z[pad (__brev ((1u << LOGW) - i) >> (32 - LOGW))];
	Bin b;
	b.lre = 0.5f * (zi.x + zc.x); b.lim = 0.5f * (zi.y - zc.y);
	b.rre = 0.5f * (zi.y + zc.y); b.rim = 0.5f * (zc.x - zi.x);
	b.pl = b.lre * b.lre + b.lim * b.lim; b.pr = b.rre * b.rre + b.rim * b.rim;
	return b;
}

template <bool SERIES, bool ENDS> using scope_args_of = std::conditional_t<ENDS, std::conditional_t<SERIES, mtr_scope_series_ends_args, mtr_scope_ends_args>,
                                                                            std::conditional_t<SERIES, mtr_scope_series_args, mtr_scope_args>>;

// ENDS: stream s ends at call frame a.ends[s] (mtr_any.h).  Its analyses are those that end at or before its end — a hop that is not full
// runs none, as fftx_run when the host stops feeding it (gui/fft.c:308-311) — `last` is its OWN last one, its tail the W frames in front of
// its end, and no frame at or behind the end is read.  End 0: the workgroup returns before it touches anything.  The stream is the
// workgroup's, so everything this changes is uniform; the instantiations without ENDS are the kernels as they were.
template <int LOGW, bool SERIES, bool ENDS = false> __global__ __launch_bounds__ (threads_of (LOGW))
void k_scope (const scope_args_of<SERIES, ENDS> a)
{
	constexpr int W = 1 << LOGW, B = W / 2, NT = threads_of (LOGW), BPT = B / NT;
	extern __shared__ __attribute__ ((aligned (16))) unsigned char smem[];
	float2* const z = reinterpret_cast<float2*> (smem);
	__shared__ float red[NT / 64];
	const uint32_t s = blockIdx.x, t = threadIdx.x;
	uint64_t end = a.n_frames;                                         // the stream's frames in the call ...
	uint32_t n_an = a.n_an;                                            // ... and the analyses that end inside them
	if constexpr (ENDS) {
		end = a.ends[s];
		if (end == 0) return;
		n_an = end < a.first ? 0 : (uint32_t) ((end - a.first) / a.hop) + 1;
	}
	const float* const src = a.audio + (size_t) s * a.stride * 2;
	float* const tail = a.tail + (size_t) s * W * 2;
	const bool al8 = (reinterpret_cast<uintptr_t> (src) & 7) == 0;
	const size_t so = (size_t) s * B;

	float level[BPT] = {}, lr[BPT] = {};
	float peak = 0.f;
	if (n_an) {
#pragma unroll
		for (int r = 0; r < BPT; ++r) { level[r] = a.level[so + t + r * NT]; lr[r] = a.lr[so + t + r * NT]; }
		peak = a.peak[s];
	}
	[[maybe_unused]] uint32_t since = 0;                               // SERIES: analyses since the last point; the next point's index
	[[maybe_unused]] uint64_t pidx = 0;
	if constexpr (SERIES) { since = a.since; pidx = a.point0; }

	for (uint32_t j = 0; j < n_an; ++j) {
		const int64_t f0 = (int64_t) (a.first + (uint64_t) j * a.hop) - W;   // the analysis' first frame
		const bool last = j + 1 == n_an;
		[[maybe_unused]] bool keep = false;                            // SERIES: the analysis is a point the rings have room for, row `at` of them
		[[maybe_unused]] size_t at = 0;
		if constexpr (SERIES) {
			if (++since == a.every) {
				since = 0;
				keep = pidx < a.cap;
				at = (size_t) s * a.cap + (size_t) pidx;
				++pidx;
			}
		}
		// ---- the windowed frames, L + iR ----
#pragma unroll 2
		for (int r = 0; r < W / NT; ++r) {
			const int i = t + r * NT;
			const float2 x = frame_at<W> (src, tail, f0 + i, al8);
			const float w = a.win[i];
			z[pad (i)] = float2{x.x * w, x.y * w};
		}
		__syncthreads ();
		// ---- the transform, in place: X [k] ends at slot bitrev (k) ----
#pragma unroll
		for (int ln = LOGW; ln >= 2; ln -= 2) {
			const int n = 1 << ln, q = n >> 2;
#pragma unroll 1
			for (int r = 0; r < W / 4 / NT; ++r) {
				// (which lane takes which butterfly: where a sub-transform has 8 .. 32 elements, consecutive lanes take the same butterfly of
				// consecutive sub-transforms — lane stride n + n / 32 slots, and one twiddle for the wave — instead of consecutive butterflies)
				const int b0 = t + r * NT;
				const int bf = ln >= 3 && ln <= 5 ? ((b0 & ((1 << (LOGW - ln)) - 1)) << (ln - 2)) + (b0 >> (LOGW - ln)) : b0;
				const int jj = bf & (q - 1), base = ((bf >> (ln - 2)) << ln) + jj;
				const uint32_t i0 = pad (base), i1 = pad (base + q), i2 = pad (base + 2 * q), i3 = pad (base + 3 * q);
				const float2 a0 = z[i0], a1 = z[i1], a2 = z[i2], a3 = z[i3];
				const float2 t0 = cadd (a0, a2), t1 = cadd (a1, a3), u = csub (a0, a2), d = csub (a1, a3);
				const float2 v = float2{d.y, -d.x};                    // -i (a1 - a3)
				float2 y0 = cadd (t0, t1), y1 = csub (t0, t1), y2 = cadd (u, v), y3 = csub (u, v);
				if (ln > 2) {
					const int m = jj << (LOGW - ln);
					y1 = cmul (y1, a.tw[2 * m]); y2 = cmul (y2, a.tw[m]); y3 = cmul (y3, a.tw[3 * m]);
				}
				z[i0] = y0; z[i1] = y1; z[i2] = y2; z[i3] = y3;
			}
			__syncthreads ();
		}
		if (LOGW & 1) {
#pragma unroll 1
			for (int r = 0; r < W / 2 / NT; ++r) {
				const int bf = t + r * NT;
				const uint32_t i0 = pad (2 * bf), i1 = pad (2 * bf + 1);
				const float2 a0 = z[i0], a1 = z[i1];
				z[i0] = cadd (a0, a1); z[i1] = csub (a0, a1);
			}
			__syncthreads ();
		}
		// ---- the split, the powers, the smoothers ----
		float pk = 0.f;
#pragma unroll
		for (int r = 0; r < BPT; ++r) {
			const uint32_t i = t + r * NT;
			if (i < 1 || i > B - 2) continue;                          // (bins 0 and B - 1 are never written: ft_analyze, fft.c:174)
			const Bin b = bin_of<LOGW> (z, i);
			const float pl = b.pl, pr = b.pr;
			// stereoscope.c:713-737
			if (pl < 1e-20f && pr < 1e-20f) { lr[r] = 0.5f; level[r] = 0.f; }
			else {
				const float lv = pl > pr ? pl : pr;
				const float lt = (float) __dadd_rn (.5, __ddiv_rn (__dmul_rn (.5, (double) __fsub_rn (sqrtf (pr), sqrtf (pl))), (double) sqrtf (lv)));
				level[r] = (float) __dadd_rn ((double) level[r], __dadd_rn (__dmul_rn (.1, (double) __fsub_rn (lv, level[r])), 1e-20));
				lr[r] = (float) __dadd_rn ((double) lr[r], __dadd_rn (__dmul_rn (.1, (double) __fsub_rn (lt, lr[r])), 1e-10));
			}
			// phasewheel.c:1316-1331
			const bool below = pl < a.thresh || pr < a.thresh;
			const float pv = pl > pr ? pl : pr;
			if (!below && pv > pk) pk = pv;
		}
		if constexpr (SERIES) {
			// a point's level and lr: the registers, bins 0 and B - 1 with them (they hold what the state arrays do)
			if (keep && (a.fields & (MTR_SCOPE_F_LEVEL | MTR_SCOPE_F_LR))) {
#pragma unroll
				for (int r = 0; r < BPT; ++r) {
					const size_t o = at * B + t + r * NT;
					if (a.fields & MTR_SCOPE_F_LEVEL) a.ring[0][o] = level[r];
					if (a.fields & MTR_SCOPE_F_LR) a.ring[1][o] = lr[r];
				}
			}
			// ... and the pass below on every point that keeps one of its fields, not on the call's last analysis alone
			if (last || (keep && (a.fields & F_PASS))) {
#pragma unroll 1
				for (int r = 0; r < BPT; ++r) {
					const uint32_t i = t + r * NT;
					const size_t o = at * B + i;
					if (i < 1 || i > B - 2) {                              // (never written: a point gets what mtr_engine_scope_read would)
						if (keep) {
							if (a.fields & MTR_SCOPE_F_PHASE) a.ring[2][o] = a.phase[so + i];
							if (a.fields & MTR_SCOPE_F_PLEVEL) a.ring[3][o] = a.plevel[so + i];
							if (a.fields & MTR_SCOPE_F_POWER_L) a.ring[5][o] = a.power_l[so + i];
							if (a.fields & MTR_SCOPE_F_POWER_R) a.ring[6][o] = a.power_r[so + i];
						}
						continue;
					}
					const Bin b = bin_of<LOGW> (z, i);
					const bool below = b.pl < a.thresh || b.pr < a.thresh;
					const float ph = below ? 0.f : __fsub_rn (atan2f (b.rim, b.rre), atan2f (b.lim, b.lre));
					const float pv = below ? -100.f : b.pl > b.pr ? b.pl : b.pr;
					if (last) {
						a.phase[so + i] = ph; a.plevel[so + i] = pv;
						a.power_l[so + i] = b.pl; a.power_r[so + i] = b.pr;
					}
					if (keep) {
						if (a.fields & MTR_SCOPE_F_PHASE) a.ring[2][o] = ph;
						if (a.fields & MTR_SCOPE_F_PLEVEL) a.ring[3][o] = pv;
						if (a.fields & MTR_SCOPE_F_POWER_L) a.ring[5][o] = b.pl;
						if (a.fields & MTR_SCOPE_F_POWER_R) a.ring[6][o] = b.pr;
					}
				}
			}
		} else
		// what only the call's last analysis leaves: the phase wheel's bins and the powers (the split once more: atan2f stays out of the loop above)
		if (last) {
#pragma unroll 1
			for (int r = 0; r < BPT; ++r) {
				const uint32_t i = t + r * NT;
				if (i < 1 || i > B - 2) continue;
				const Bin b = bin_of<LOGW> (z, i);
				const bool below = b.pl < a.thresh || b.pr < a.thresh;
				a.phase[so + i] = below ? 0.f : __fsub_rn (atan2f (b.rim, b.rre), atan2f (b.lim, b.lre));
				a.plevel[so + i] = below ? -100.f : b.pl > b.pr ? b.pl : b.pr;
				a.power_l[so + i] = b.pl; a.power_r[so + i] = b.pr;
			}
		}
		// the analysis' largest plevel (a NaN never is: `>`), then phasewheel.c:1333-1335
#pragma unroll
		for (int d = 32; d >= 1; d >>= 1) pk = fmaxf (pk, __shfl_xor (pk, d, 64));
		if ((t & 63) == 0) red[t >> 6] = pk;
		__syncthreads ();                                              // (and every read of z is done: the next analysis may overwrite it)
#pragma unroll
		for (int w = 0; w < NT / 64; ++w) pk = fmaxf (pk, red[w]);
		peak = (float) __dadd_rn ((double) peak, __dadd_rn (__dmul_rn (.04, (double) __fsub_rn (pk, peak)), 1e-15));
		if (isnan (peak)) peak = 0.f;
		if (peak > 1000.f) peak = 1000.f;
		if constexpr (SERIES) {
			if (keep && (a.fields & MTR_SCOPE_F_PEAK) && t == 0) a.ring[F_PEAK_AT][at] = peak;
		}
	}

	if (n_an) {
#pragma unroll
		for (int r = 0; r < BPT; ++r) {
			const uint32_t i = t + r * NT;
			if (i < 1 || i > B - 2) continue;
			a.level[so + i] = level[r]; a.lr[so + i] = lr[r];
		}
		if (t == 0) a.peak[s] = peak;
	}
	// ---- the stream's last W frames, for the calls to come (through LDS: the old tail is read before it is overwritten) ----
	const int64_t t0 = (int64_t) end - W;
	for (int i = t; i < W; i += NT) z[pad (i)] = frame_at<W> (src, tail, t0 + i, al8);
	__syncthreads ();
	for (int i = t; i < W; i += NT) *reinterpret_cast<float2*> (tail + 2 * i) = z[pad (i)];
}

// A: mtr_scope_args — the kernel without a series — or mtr_scope_series_args, or the struct with ends on top of either
template <int LOGW, typename A> int launch (const A& a, hipStream_t st)
{
	constexpr bool SERIES = std::is_base_of_v<mtr_scope_series_args, A>;
	constexpr bool ENDS = !std::is_same_v<A, mtr_scope_args> && !std::is_same_v<A, mtr_scope_series_args>;
	static_assert (std::is_same_v<A, scope_args_of<SERIES, ENDS>>, "k_scope's arguments");
	constexpr uint32_t bytes = lds_slots (1u << LOGW) * sizeof (float2);
	if (bytes > 48 * 1024) {                                           // (per instantiation: each is a kernel of its own)
		static const hipError_t once = hipFuncSetAttribute ((const void*) k_scope<LOGW, SERIES, ENDS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int) bytes);
		(void) once;
	}
	hipLaunchKernelGGL ((k_scope<LOGW, SERIES, ENDS>), dim3 (a.n_streams), dim3 (threads_of (LOGW)), bytes, st, a);
	return hipGetLastError () == hipSuccess ? 0 : -1;
}

template <typename A> int mtr_launch_scope (uint32_t W, const A& a, hipStream_t st)
{
	switch (W) {
	case 256:   return launch<8> (a, st);
	case 512:   return launch<9> (a, st);
	case 1024:  return launch<10> (a, st);
	case 2048:  return launch<11> (a, st);
	case 4096:  return launch<12> (a, st);
	case 8192:  return launch<13> (a, st);
	case 16384: return launch<14> (a, st);
	}
	return -1;
}

// how a call cuts the series (mtr_scope_series_cut): the arguments have been checked
void series_cut (uint32_t fill, uint32_t hop, uint32_t since, uint32_t every, uint64_t n_frames, uint64_t* analyses, uint64_t* points)
{
	*analyses = n_frames / hop + (fill + n_frames % hop) / hop;       // (fill + n_frames) / hop without the sum's overflow
	*points = every ? (since + *analyses) / every : 0;
}

// K, the capacity and the fields into the engine, with rings for its window (K = 0: none); the series empty.  On failure it is off
int series_set (mtr_engine* e, uint32_t K, uint32_t cap, uint32_t fields)
{
	mtr_engine::Scope::Series& sr = e->sp.ser;
	const auto off = [&sr] { for (auto& r : sr.ring) r.drop (); sr.open.drop (); sr.every = sr.cap = sr.fields = 0; };
	off ();
	e->pos.sp_since = 0; e->pos.sp_points = 0;
	e->sp.points.assign (e->cfg.n_streams, 0);
	if (!K) return MTR_OK;
	const size_t S = e->cfg.n_streams, B = e->sp.W / 2;
	size_t rows, n;
	if (__builtin_mul_overflow (S, (size_t) cap, &rows) || __builtin_mul_overflow (rows, B, &n) || n > SIZE_MAX / sizeof (float))
		return fail (MTR_ERR_NOMEM, "mtr_engine_scope_set_series: the rings' size overflows size_t");
	for (int k = 0; k < 7; ++k) {
		if (!(fields >> k & 1)) continue;
		if (const int rc = series_ring (sr.ring[k], k == F_PEAK_AT ? rows : n, "hipMalloc SCOPE series")) { off (); return rc; }
	}
	if (sr.open.reserve (S * sizeof (mtr_scope_open))) { off (); return fail (MTR_ERR_NOMEM, "hipMalloc SCOPE series (open groups)"); }
	if (hipMemset (sr.open.p, 0, sr.open.n) != hipSuccess) { off (); return fail (MTR_ERR_HIP, "hipMemset SCOPE series", hipGetLastError ()); }
	sr.every = K; sr.cap = cap; sr.fields = fields;
	return MTR_OK;
}

// 0: a window the engine takes; MTR_ERR_UNSUPPORTED: one only the reference takes (reinitialize_fft, stereoscope.c:123-131: 64 .. 8192 bins,
// rounded up by its own bit smear — powers of two and a few more, 12288 among them); MTR_ERR_ARG: neither
int window_check (uint32_t W)
{
	if (W < 128 || W > W_MAX || (W & 1)) return MTR_ERR_ARG;
	uint32_t b = W / 2 - 1;
	b |= 0x3f; b |= b >> 2; b |= b >> 4; b |= b >> 8; b |= b >> 16;
	if (b + 1 != W / 2) return MTR_ERR_ARG;
	return W >= W_MIN && (W & (W - 1)) == 0 ? MTR_OK : MTR_ERR_UNSUPPORTED;
}

int no_scope (const mtr_engine* e) { return !e || !(e->cfg.meters & MTR_METER_SCOPE); }

// window, hop and threshold into the engine: memory for W, the window and the twiddles (in double, rounded once) on the device
int configure (mtr_engine* e, uint32_t W, uint32_t H, float thresh)
{
	const size_t S = e->cfg.n_streams, B = W / 2;
	mtr_engine::Scope& sp = e->sp;
	HIPCHK (hipSetDevice (e->cfg.device));
	HIPCHK (hipStreamSynchronize (e->last_stream));
	if (sp.tail.reserve (S * W * 2) || sp.level.reserve (S * B) || sp.lr.reserve (S * B) || sp.phase.reserve (S * B) || sp.plevel.reserve (S * B)
	    || sp.power_l.reserve (S * B) || sp.power_r.reserve (S * B) || sp.peak.reserve (S) || sp.hdr.reserve (S * sizeof (mtr_scope_hdr))
	    || sp.win.reserve (W) || sp.tw.reserve ((size_t) W * 2))
		return fail (MTR_ERR_NOMEM, "hipMalloc SCOPE state");
	std::vector<float> h (W), tw ((size_t) W * 2);
	mtr_setup_scope_window (W, h.data ());
	for (uint32_t m = 0; m < W; ++m) {
		const double ph = 2.0 * M_PI * (double) m / (double) W;
		tw[2 * m] = (float) cos (ph); tw[2 * m + 1] = (float) -sin (ph);
	}
	HIPCHK (hipMemcpy (sp.win.p, h.data (), W * sizeof (float), hipMemcpyHostToDevice));
	HIPCHK (hipMemcpy (sp.tw.p, tw.data (), tw.size () * sizeof (float), hipMemcpyHostToDevice));
	HIPCHK (hipMemset (sp.hdr.p, 0, S * sizeof (mtr_scope_hdr)));
	sp.W = W; sp.H = H; sp.thresh = thresh;
	// the series keeps its settings; its rings are those of the new window
	if (const int rc = series_set (e, sp.ser.every, sp.ser.cap, sp.ser.fields)) return rc;
	return mtr_engine_scope_reset (e);
}

uint32_t default_hop (const mtr_engine* e) { return (uint32_t) ceil ((double) e->cfg.sample_rate / 25.0); }   // fftx_init (.., 25): fft.c:219

}  // namespace

// ---- SCOPE in the engine: set-up, the call's step, the blob's sections and the cursors in them, the C entry points ------------------------

static int scope_create (mtr_engine* e) { return configure (e, W_DEFAULT, default_hop (e), 1e-6f); }   // stereoscope.c:641, phasewheel.c:1212

// A call with ends (mtr_engine_process_*_any, or any call once a stream of the view is closed: se.ends is then the view's ends, 0 for a closed
// stream) takes the ENDS instantiations; every other call the dense ones, as ever.
static int scope_step (mtr_engine* e, const Call& c, Cursors& nx, const StreamEnds& se)
{
	const mtr_engine::Scope& sp = e->sp;
	const size_t vo = c.off, B = sp.W / 2;
	const uint64_t tot = (uint64_t) e->pos.sp_fill + c.n_frames;
	const uint32_t K = sp.ser.every;
	uint64_t n_an, n_pt;
	series_cut (e->pos.sp_fill, sp.H, e->pos.sp_since, K, c.n_frames, &n_an, &n_pt);
	mtr_scope_args sa;
	sa.audio = c.audio; sa.stride = c.stride; sa.n_frames = c.n_frames;
	sa.first = sp.H - e->pos.sp_fill; sa.n_streams = c.cnt; sa.n_an = (uint32_t) n_an; sa.hop = sp.H; sa.thresh = sp.thresh;
	sa.win = sp.win.p; sa.tw = reinterpret_cast<const float2*> (sp.tw.p);
	sa.tail = sp.tail.p + vo * sp.W * 2;
	sa.level = sp.level.p + vo * B; sa.lr = sp.lr.p + vo * B; sa.phase = sp.phase.p + vo * B; sa.plevel = sp.plevel.p + vo * B;
	sa.power_l = sp.power_l.p + vo * B; sa.power_r = sp.power_r.p + vo * B; sa.peak = sp.peak.p + vo;
	if (K) {
		// the groups of K are counted from where the CALL started (e->pos): every view of a host call sees the same cuts and appends at the same points
		const uint32_t cap = sp.ser.cap;
		mtr_scope_series_args ss;
		static_cast<mtr_scope_args&> (ss) = sa;
		for (int k = 0; k < 7; ++k) ss.ring[k] = sp.ser.ring[k].p ? sp.ser.ring[k].p + vo * cap * (k == F_PEAK_AT ? 1 : B) : nullptr;
		ss.point0 = std::min<uint64_t> (e->pos.sp_points, cap);
		ss.every = K; ss.since = e->pos.sp_since; ss.cap = cap; ss.fields = cap ? sp.ser.fields : 0;
		if (se.ends) {
			mtr_scope_series_ends_args es;
			static_cast<mtr_scope_series_args&> (es) = ss;
			es.ends = se.ends;
			if (mtr_launch_scope (sp.W, es, c.st)) return fail (MTR_ERR_HIP, "k_scope launch (series, ends)", hipGetLastError ());
		} else if (mtr_launch_scope (sp.W, ss, c.st)) return fail (MTR_ERR_HIP, "k_scope launch (series)", hipGetLastError ());
		nx.sp_since = (uint32_t) ((e->pos.sp_since + n_an) % K);
		nx.sp_points = e->pos.sp_points + n_pt;
	} else if (se.ends) {
		mtr_scope_ends_args ea;
		static_cast<mtr_scope_args&> (ea) = sa;
		ea.ends = se.ends;
		if (mtr_launch_scope (sp.W, ea, c.st)) return fail (MTR_ERR_HIP, "k_scope launch (ends)", hipGetLastError ());
	} else if (mtr_launch_scope (sp.W, sa, c.st)) return fail (MTR_ERR_HIP, "k_scope launch", hipGetLastError ());
	nx.sp_fill = (uint32_t) (tot % sp.H);
	nx.sp_analyses = e->pos.sp_analyses + sa.n_an;
	return MTR_OK;
}

// stream g's own analyses and points (mtr_engine_scope_points; SideMeter::count — analyses and the points among them, not blocks of a period:
// no `series` hook): those of its `frames` frames of a call that starts at e->pos; an imported stream takes the lock-step numbers
static void scope_count (mtr_engine* e, size_t g, const Call* c, uint64_t frames)
{
	if (!c) { e->sp.analyses[g] = e->pos.sp_analyses; e->sp.points[g] = e->pos.sp_points; return; }
	uint64_t an, pt;
	series_cut (e->pos.sp_fill, e->sp.H, e->pos.sp_since, e->sp.ser.every, frames, &an, &pt);
	e->sp.analyses[g] += an; e->sp.points[g] += pt;
}

static void scope_sections (const mtr_engine* e, std::vector<StateSection>& v)
{
	const mtr_engine::Scope& sp = e->sp;
	const size_t B = sp.W / 2;
	v.push_back ({ sp.hdr.p, sizeof (mtr_scope_hdr) });
	v.push_back ({ sp.tail.p, (size_t) sp.W * 2 * sizeof (float) });
	for (const float* p : { sp.level.p, sp.lr.p, sp.phase.p, sp.plevel.p }) v.push_back ({ p, B * sizeof (float) });
	v.push_back ({ sp.peak.p, sizeof (float) });
	v.push_back ({ sp.power_l.p, B * sizeof (float) });
	v.push_back ({ sp.power_r.p, B * sizeof (float) });
}

// The blob header: the whole entry of the first section — window, hop, threshold, the frames since the last analysis and the analyses
// counted.  The configuration must be the engine's; a fresh engine takes the cursors
constexpr const char* SCOPE_CORRUPT = "mtr_engine_state_import: corrupt blob (cursor of the SCOPE analyses)";

static void scope_hdr_write (const mtr_engine* e, void* out)
{
	*static_cast<mtr_scope_hdr*> (out) = { e->sp.W, e->sp.H, e->sp.thresh, e->pos.sp_fill, e->pos.sp_analyses };
}

static int scope_hdr_check (const mtr_engine* e, const void* in, bool fresh)
{
	const mtr_scope_hdr& h = *static_cast<const mtr_scope_hdr*> (in);
	if (h.hop < H_MIN || h.hop > H_MAX || h.fill >= h.hop) return fail (MTR_ERR_STATE, SCOPE_CORRUPT);
	if (h.window != e->sp.W || h.hop != e->sp.H || memcmp (&h.thresh, &e->sp.thresh, sizeof (float)))
		return fail (MTR_ERR_STATE, "mtr_engine_state_import: the blob's SCOPE configuration (window, hop, threshold) is not the engine's");
	if (!fresh && h.fill != e->pos.sp_fill)
		return fail (MTR_ERR_STATE, "mtr_engine_state_import: the engine does not stand where the blob's streams do (hop of the SCOPE analyses)");
	return MTR_OK;
}

static void scope_hdr_take (mtr_engine* e, const void* in)
{
	const mtr_scope_hdr& h = *static_cast<const mtr_scope_hdr*> (in);
	e->pos.sp_fill = h.fill; e->pos.sp_analyses = h.analyses;
}

static constinit BlobHeader scope_hdr = { .offset = 0, .bytes = sizeof (mtr_scope_hdr), .corrupt = SCOPE_CORRUPT, .write = scope_hdr_write, .check = scope_hdr_check, .take = scope_hdr_take };
constinit SideMeter scope_meter = { .bits = MTR_METER_SCOPE, .max_frames = 0x7fffffffull, .max_text = "SCOPE: n_frames per call must be < 2^31 - 1",
                                    .create = scope_create, .reset = mtr_engine_scope_reset, .step = scope_step, .sections = scope_sections, .hdr = &scope_hdr, .count = scope_count };

// With a series the blob carries one more section, behind every older one (the second row of the meter in SIDE_METERS): where the open group
// of K analyses stands.  All of an entry is its host-owned header — K and the analyses since the last point.  An engine takes a blob of its
// own K only; fields and capacity need not match, and the points are not part of the blob.
static void scope_open_sections (const mtr_engine* e, std::vector<StateSection>& v)
{
	if (e->sp.ser.every) v.push_back ({ e->sp.ser.open.p, sizeof (mtr_scope_open) });
}

constexpr const char* SCOPE_SERIES_CORRUPT = "mtr_engine_state_import: corrupt blob (the SCOPE series' analyses per point)";

static void scope_open_write (const mtr_engine* e, void* out)
{
	const mtr_scope_open h = { e->sp.ser.every, e->pos.sp_since };
	memcpy (out, &h, sizeof (h));
}

static int scope_open_check (const mtr_engine* e, const void* in, bool fresh)
{
	mtr_scope_open h;
	memcpy (&h, in, sizeof (h));
	if (!h.every || h.every > K_MAX || h.since >= h.every) return fail (MTR_ERR_STATE, SCOPE_SERIES_CORRUPT);
	if (h.every != e->sp.ser.every || (!fresh && h.since != e->pos.sp_since))
		return fail (MTR_ERR_STATE, "mtr_engine_state_import: the engine does not stand where the blob's streams do (analyses per point of the SCOPE series, or since the last one)");
	return MTR_OK;
}

static void scope_open_take (mtr_engine* e, const void* in)
{
	mtr_scope_open h;
	memcpy (&h, in, sizeof (h));
	e->pos.sp_since = h.since;
}

static constinit BlobHeader scope_open_hdr = { .offset = 0, .bytes = sizeof (mtr_scope_open), .corrupt = SCOPE_SERIES_CORRUPT, .write = scope_open_write, .check = scope_open_check, .take = scope_open_take };
// (no reset and no step: the meter's first row resets and queues all of it)
constinit SideMeter scope_series_meter = { .bits = MTR_METER_SCOPE, .sections = scope_open_sections, .hdr = &scope_open_hdr };

extern "C" {

int mtr_scope_window (uint32_t window_frames, float* out)
{
	const int rc = window_check (window_frames);
	if (rc) return fail (rc, rc == MTR_ERR_UNSUPPORTED ? "mtr_scope_window: the engine takes powers of two, 256 .. 16384" : "mtr_scope_window: window_frames");
	if (!out) return fail (MTR_ERR_ARG, "mtr_scope_window: null argument");
	mtr_setup_scope_window (window_frames, out);
	return MTR_OK;
}

int mtr_engine_scope_configure (mtr_engine* e, uint32_t window_frames, uint32_t hop_frames, float phase_thresh_power)
{
	if (no_scope (e)) return fail (MTR_ERR_ARG, "no SCOPE in this engine");
	const int rc = window_check (window_frames);
	if (rc) return fail (rc, rc == MTR_ERR_UNSUPPORTED ? "mtr_engine_scope_configure: the engine takes powers of two, 256 .. 16384" : "mtr_engine_scope_configure: window_frames");
	if (hop_frames && (hop_frames < H_MIN || hop_frames > H_MAX)) return fail (MTR_ERR_ARG, "mtr_engine_scope_configure: hop_frames is 0 or 64 .. 2^20");
	if (!(phase_thresh_power >= 0.f)) return fail (MTR_ERR_ARG, "mtr_engine_scope_configure: phase_thresh_power must be >= 0");
	if (e->advanced) return fail (MTR_ERR_STATE, "mtr_engine_scope_configure: only on an engine that has processed nothing since create / reset");
	return configure (e, window_frames, hop_frames ? hop_frames : default_hop (e), phase_thresh_power);
}

int mtr_engine_scope_config (const mtr_engine* e, uint32_t* window_frames, uint32_t* hop_frames, float* phase_thresh_power)
{
	if (no_scope (e)) return fail (MTR_ERR_ARG, "no SCOPE in this engine");
	if (window_frames) *window_frames = e->sp.W;
	if (hop_frames) *hop_frames = e->sp.H;
	if (phase_thresh_power) *phase_thresh_power = e->sp.thresh;
	return MTR_OK;
}

// reinitialize_fft (stereoscope.c:143-146, phasewheel.c:202-205) and fftx_reset (fft.c:191-205); the configuration is kept
int mtr_engine_scope_reset (mtr_engine* e)
{
	if (no_scope (e)) return fail (MTR_ERR_ARG, "no SCOPE in this engine");
	e->snap_valid = false;
	HIPCHK (hipSetDevice (e->cfg.device));
	mtr_engine::Scope& sp = e->sp;
	const size_t n = (size_t) e->cfg.n_streams * (sp.W / 2);
	HIPCHK (hipStreamSynchronize (e->last_stream));
	const std::vector<float> m100 (n, -100.f), half (n, .5f);
	HIPCHK (hipMemcpy (sp.level.p, m100.data (), n * sizeof (float), hipMemcpyHostToDevice));
	HIPCHK (hipMemcpy (sp.plevel.p, m100.data (), n * sizeof (float), hipMemcpyHostToDevice));
	HIPCHK (hipMemcpy (sp.lr.p, half.data (), n * sizeof (float), hipMemcpyHostToDevice));
	HIPCHK (hipMemset (sp.phase.p, 0, n * sizeof (float)));
	HIPCHK (hipMemset (sp.power_l.p, 0, n * sizeof (float)));
	HIPCHK (hipMemset (sp.power_r.p, 0, n * sizeof (float)));
	HIPCHK (hipMemset (sp.peak.p, 0, e->cfg.n_streams * sizeof (float)));
	HIPCHK (hipMemset (sp.tail.p, 0, (size_t) e->cfg.n_streams * sp.W * 2 * sizeof (float)));
	e->pos.sp_fill = 0;
	e->pos.sp_analyses = 0;
	// the reading series: emptied (what a ring holds past its count is never handed out), the open group gone, the settings kept
	e->pos.sp_since = 0;
	e->pos.sp_points = 0;
	sp.analyses.assign (e->cfg.n_streams, 0);
	sp.points.assign (e->cfg.n_streams, 0);
	return MTR_OK;
}

int mtr_engine_scope_read (mtr_engine* e, uint32_t first, uint32_t count, float* level, float* lr, float* phase, float* plevel, float* peak,
                           float* power_l, float* power_r)
{
	int rc = meter_range (e, !no_scope (e), "no SCOPE in this engine", first, count);
	if (rc || !count || (rc = wait_stream (e))) return rc;
	const mtr_engine::Scope& sp = e->sp;
	const size_t B = sp.W / 2;
	const struct { float* out; const float* dev; size_t per; } arr[] = {
		{ level, sp.level.p, B }, { lr, sp.lr.p, B }, { phase, sp.phase.p, B }, { plevel, sp.plevel.p, B }, { peak, sp.peak.p, 1 },
		{ power_l, sp.power_l.p, B }, { power_r, sp.power_r.p, B },
	};
	for (const auto& v : arr)
		if (v.out) HIPCHK (hipMemcpy (v.out, v.dev + (size_t) first * v.per, (size_t) count * v.per * sizeof (float), hipMemcpyDeviceToHost));
	return MTR_OK;
}

int mtr_engine_scope_analyses (mtr_engine* e, uint64_t* n)
{
	if (no_scope (e) || !n) return fail (MTR_ERR_ARG, "mtr_engine_scope_analyses: no SCOPE in this engine, or a null argument");
	*n = e->pos.sp_analyses;
	return MTR_OK;
}

int mtr_engine_scope_points (mtr_engine* e, uint32_t first, uint32_t count, uint64_t* analyses, uint64_t* points)
{
	const int rc = meter_range (e, !no_scope (e), "no SCOPE in this engine", first, count);
	if (rc) return rc;
	for (uint32_t i = 0; i < count; ++i) {
		if (analyses) analyses[i] = e->sp.analyses[first + i];
		if (points) points[i] = e->sp.points[first + i];
	}
	return MTR_OK;
}

// ---- the reading series (mtr_scope_series.h) ----

int mtr_scope_series_cut (uint32_t fill, uint32_t hop, uint32_t since, uint32_t every, uint64_t n_frames, uint64_t* analyses, uint64_t* points)
{
	if (!analyses || !points) return fail (MTR_ERR_ARG, "mtr_scope_series_cut: null argument");
	if (hop < H_MIN || hop > H_MAX) return fail (MTR_ERR_ARG, "mtr_scope_series_cut: hop is 64 .. 2^20");
	if (fill >= hop) return fail (MTR_ERR_ARG, "mtr_scope_series_cut: fill must be < hop");
	if (every && since >= every) return fail (MTR_ERR_ARG, "mtr_scope_series_cut: since must be < every");
	series_cut (fill, hop, since, every, n_frames, analyses, points);
	return MTR_OK;
}

int mtr_engine_scope_set_series (mtr_engine* e, uint32_t every_analyses, uint32_t capacity_points, uint32_t fields)
{
	if (no_scope (e)) return fail (MTR_ERR_ARG, "no SCOPE in this engine");
	if (every_analyses > K_MAX) return fail (MTR_ERR_ARG, "mtr_engine_scope_set_series: every_analyses is 0 or 1 .. 2^20");
	if (every_analyses && (!fields || (fields & ~MTR_SCOPE_F_ALL)))
		return fail (MTR_ERR_ARG, "mtr_engine_scope_set_series: fields is a non-empty subset of MTR_SCOPE_F_ALL");
	if (e->advanced) return fail (MTR_ERR_STATE, "mtr_engine_scope_set_series: only on an engine that has processed nothing since create / reset");
	const int rc = wait_stream (e);
	if (rc) return rc;
	return series_set (e, every_analyses, every_analyses ? capacity_points : 0, every_analyses ? fields : 0);
}

int mtr_engine_scope_series_config (const mtr_engine* e, uint32_t* every_analyses, uint32_t* capacity_points, uint32_t* fields)
{
	if (no_scope (e)) return fail (MTR_ERR_ARG, "no SCOPE in this engine");
	if (every_analyses) *every_analyses = e->sp.ser.every;
	if (capacity_points) *capacity_points = e->sp.ser.cap;
	if (fields) *fields = e->sp.ser.fields;
	return MTR_OK;
}

int mtr_engine_scope_series (mtr_engine* e, uint32_t first, uint32_t count, float* level, float* lr, float* phase, float* plevel, float* peak,
                             float* power_l, float* power_r, uint32_t capacity, uint32_t* n_points, uint32_t* dropped)
{
	int rc = meter_range (e, !no_scope (e), "no SCOPE in this engine", first, count);
	if (rc) return rc;
	const mtr_engine::Scope::Series& sr = e->sp.ser;
	if (!sr.every) return fail (MTR_ERR_ARG, "mtr_engine_scope_series: the series is off (mtr_engine_scope_set_series)");
	float* const out[7] = { level, lr, phase, plevel, peak, power_l, power_r };
	bool any = false;
	for (int k = 0; k < 7; ++k) {
		if (out[k] && !(sr.fields >> k & 1)) return fail (MTR_ERR_ARG, "mtr_engine_scope_series: a pointer for a field the series does not keep");
		any |= out[k] != nullptr;
	}
	const size_t take = series_counts (e->pos.sp_points, sr.cap, capacity, n_points, dropped);
	if (!any || !count || !take) return MTR_OK;
	if ((rc = wait_stream (e))) return rc;
	const size_t B = e->sp.W / 2;
	for (int k = 0; k < 7; ++k) {
		if (!out[k]) continue;
		const size_t w = k == F_PEAK_AT ? 1 : B;
		if ((rc = series_fetch (out[k], sr.ring[k].p, w, first, sr.cap, capacity, take, count))) return rc;
		// (a stream that was closed has fewer points of its own than the open ones: 0.0f behind them, whatever the ring still holds there)
		for (uint32_t i = 0; i < count; ++i) {
			const uint64_t own = e->sp.points[first + i];
			if (own < take) memset (out[k] + ((size_t) i * capacity + (size_t) own) * w, 0, (take - (size_t) own) * w * sizeof (float));
		}
	}
	return MTR_OK;
}

} // extern "C"
