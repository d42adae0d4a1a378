// mtr_bank.hip — 30-band 1/3-octave filter bank for gfx950 + the synthetic-signal fill kernel.
//
// Replaces the per-sample loop of spectrum_run (src/spectrumlv2.c:210-227) around
// bandpass_process / proc_one (src/spectr.c:68-87): mono down-mix, 30 bands x 6 cascaded
// TDF-II biquads in double, float EMA of v^2 with peak hold.
//
// Mapping: one lane per (stream, band), bands of consecutive streams packed back to back — lane p of the launch is
// stream p / 30, band p % 30 — so all 64 lanes of every wave work (a layout of 32 lanes per stream idles two in
// every 32: 6 % of a kernel that issues VALU instructions 100 % of the time).  The 12-state recurrence of a band
// is serial in time and, with pole radii up to 0.99991, not worth an exact time split (a 12x12 carry matrix per
// band); with >= 4096 streams there are >= 122k independent lanes, which fills the chip.  A wave of 64 lanes
// covers 2.1 streams: it stages chunks of frames of the (up to) four streams it touches through its own LDS buffers,
// forming the mono mix (L+R)/2 and adding the anti-denormal toggle once per frame instead of once per
// band; lanes then read their stream's row as an LDS broadcast.  Workgroup = one wave: no barrier anywhere.  Coefficients and states live in registers for the
// whole call.  fp64 VALU bound: 25 fp64 + 4 fp32 instructions per (frame, band), 4 cycles each, and nothing else in
// the loop — the kernel runs at that instruction floor (profiles/).
#include <hip/hip_runtime.h>

#include <cmath>
#include <type_traits>
#include <vector>

#include "mtr_engine_impl.h"

struct mtr_bank_args {
	const float*    audio;
	uint64_t        stride;
	uint64_t        n_frames;
	const double*   coef;         /* [30][6][5]: b0 b1 b2 a1 a2 per section */
	double*         z;            /* [S][30][12] section states */
	float*          val;          /* [S][30] */
	float*          mx;           /* [S][30] */
	const int32_t*  ac_in;        /* [S] dither toggle parity at the start of the call (shared by the 30 bands of a stream) */
	int32_t*        ac_out;       /* [S] ... and after it: ANOTHER buffer (a workgroup that starts late must still read the old one) */
	uint32_t        n_streams, n_channels;
	float           omega;
};

// the reading series (mtr_spectr.h): what its instantiation of k_bank takes on top — a struct of its own, so that the dense kernel's
// arguments stay what they were
struct mtr_bank_series_args : mtr_bank_args {
	float*          s_val;        /* [S][cap][30] (null with cap 0) */
	float*          s_mx;
	uint32_t        period;       /* P > 0 */
	uint32_t        e0;           /* frames from the call's start to the end of the block open on entry: 1 .. P */
	uint64_t        point0;       /* blocks completed before the call */
	uint32_t        cap;
	int32_t         peak_block;   /* MTR_SPECTR_PEAK_BLOCK: max = 0 behind every point */
};

// track lengths (mtr_ends.h): what the two ENDS instantiations of k_bank take on top of the dense and the series form — structs of their own again,
// so that those two kernels' arguments, and with them their code, stay what they were
struct mtr_bank_ends_args : mtr_bank_args {
	const uint32_t* ends;         /* [S] the call frame at which each stream ends: 0 (closed, untouched) .. n_frames */
};
struct mtr_bank_series_ends_args : mtr_bank_series_args {
	const uint32_t* ends;
};

#define BANK_ROWS  4      /* streams a wave of 64 lanes can touch: ceil (63 / 30) + 1 */
#define BANK_CHUNK 128    /* frames staged per stream per iteration: two per lane */
#define BANK_PITCH (BANK_CHUNK + 2)   /* doubles per row: rows four banks apart, so the <= 4 rows a wave reads never collide */

// One frame of one band — the step both instantiations of k_bank share, on the kernel's W, z, val, mx and omega.  (A macro, not a function or
// a lambda: either changes the order of operands in the dense kernel's code, and that kernel stays the one it was, instruction for instruction.)
// six TDF-II sections (spectr.c:68-76).  Section 0 carries the normalisation g: numerator
// g (1, 2, 1); sections 1-5 have (1, +-2, 1): b0 in = b2 in = in and b1 in = +-2 in are exact, so
// sharing the product changes nothing but the operation count (25 instead of 31 fp64 ops).
// `val > mx ? val : mx` (spectrumlv2.c:222) as one v_max_f32: a NaN val loses either way, mx is never NaN
#define BANK_FRAME(in) \
	{ \
		double out = (in); \
		{ \
			const double gi = W[0][0] * out; \
			const double y = gi + z[0]; \
			z[0] = fma (-W[0][3], y, fma (2.0, gi, z[1])); \
			z[1] = fma (-W[0][4], y, gi); \
			out = y; \
		} \
		_Pragma ("unroll") \
		for (int i = 1; i < 6; ++i) { \
			const double y = out + z[2 * i]; \
			z[2 * i]     = fma (-W[i][3], y, fma (W[i][1], out, z[2 * i + 1])); \
			z[2 * i + 1] = fma (-W[i][4], y, out); \
			out = y; \
		} \
		const float v = (float) out; \
		const float q = v * v; \
		val += omega * (q - val); \
		mx = __builtin_fmaxf (mx, val); \
	}

// One wave per workgroup, NO barrier: the wave stages the chunks of the (up to four) streams it touches through its own
// two LDS buffers — chunk c + 1 is written, and chunk c + 2's loads are in flight, while chunk c is computed — so nothing
// in the loop ever waits for another wave (round 2's four-wave workgroups spent 17 % of the SIMD time outside the
// arithmetic: two barriers per 256 frames, on a kernel whose waves do not run in lock step).
//
// A = mtr_bank_series_args (SERIES, P > 0): the spectrum_runs are the blocks of exactly P frames counted from reset, not the calls.  Same mapping, same
// staging, same per-frame step (BANK_FRAME: one piece of source); the loop over a chunk runs in pieces that end at the chunk's end or at the
// block's, whichever comes first — where the blocks end follows from the arguments alone, so the split is scalar control flow — and at a
// block's end the live lanes do spectrum_run's epilogue (spectrumlv2.c:230-238) and append their (val, max); the call's end stores the states
// as they stand.
//
// A = mtr_bank_ends_args / mtr_bank_series_ends_args (ENDS): every stream ends at its own frame of the call, ends[s] <= n_frames.  The (up to) four
// ends a wave meets are uniform values, read with scalar loads.  fetch takes no frame at or behind its row's end; the wave's chunk loop runs to the
// LAST end among its rows and stops there; a chunk runs in pieces that end at the chunk's end, a block's end (SERIES) or any row's end, so the set
// of live lanes is constant inside a piece and the per-frame code carries no per-lane compare.  At a row's end its lanes do the epilogue — in the
// series form, r frames into a block with 0 < r < P, with the truncated point — and drop out: nothing behind changes their registers, which the
// kernel's end stores as they stand.  A row with end 0 is neither computed nor stored; its dither parity is COPIED to the other buffer.
template <typename A> __global__ __launch_bounds__ (64) void k_bank (const A a)
{
	constexpr bool SERIES = std::is_base_of_v<mtr_bank_series_args, A>;
	constexpr bool ENDS = requires { a.ends; };
	__shared__ double mix[2][BANK_ROWS][BANK_PITCH];    // mono mix + the +-1e-12 anti-denormal toggle, as double

	const int lane = threadIdx.x;
	const uint64_t pair0 = (uint64_t) blockIdx.x * 64;             // first (stream, band) pair of the wave
	const uint64_t pair  = pair0 + lane;
	const uint32_t s0 = (uint32_t) (pair0 / MTR_NBANDS);           // first stream the wave touches
	const uint32_t s  = (uint32_t) (pair / MTR_NBANDS);
	const int band = (int) (pair - (uint64_t) s * MTR_NBANDS);
	const int row  = (int) (s - s0);
	const bool live = s < a.n_streams;

	double W[6][5];
	double z[12];
	float  val = 0.f, mx = 0.f;
	if (live) {
#pragma unroll
		for (int i = 0; i < 6; ++i)
#pragma unroll
			for (int k = 0; k < 5; ++k) W[i][k] = a.coef[(band * 6 + i) * 5 + k];
#pragma unroll
		for (int i = 0; i < 12; ++i) z[i] = a.z[((size_t) s * MTR_NBANDS + band) * 12 + i];
		val = a.val[(size_t) s * MTR_NBANDS + band];
		mx  = a.mx[(size_t) s * MTR_NBANDS + band];
	} else {
#pragma unroll
		for (int i = 0; i < 6; ++i)
#pragma unroll
			for (int k = 0; k < 5; ++k) W[i][k] = 0;
#pragma unroll
		for (int i = 0; i < 12; ++i) z[i] = 0;
	}
	const float omega = a.omega;
	// the toggle parity each staged row starts the call with (all lanes keep all four: the staging is by frame, not by row)
	int par0[BANK_ROWS];
#pragma unroll
	for (int g = 0; g < BANK_ROWS; ++g) par0[g] = (s0 + g < a.n_streams) ? a.ac_in[s0 + g] : 0;
	const int my_par = live ? a.ac_in[s] : 0;
	// ENDS: the rows' ends (uniform; 0 for a row past the batch), the last of them, and the lane's own
	[[maybe_unused]] uint32_t rend[BANK_ROWS] = { 0, 0, 0, 0 };
	[[maybe_unused]] uint32_t my_end = 0;
	uint64_t stop = a.n_frames;                  // where the wave's chunk loop ends
	if constexpr (ENDS) {
		uint32_t last = 0;
#pragma unroll
		for (int g = 0; g < BANK_ROWS; ++g) {
			rend[g] = (s0 + g < a.n_streams) ? min (a.ends[s0 + g], (uint32_t) a.n_frames) : 0;
			last = max (last, rend[g]);
		}
		stop = last;
		my_end = live ? min (a.ends[s], (uint32_t) a.n_frames) : 0;
	}

	// lane t stages frames 2 t, 2 t + 1 of every row
	float2 raw[BANK_ROWS][2];
	auto fetch = [&] (uint64_t base) {
#pragma unroll
		for (int g = 0; g < BANK_ROWS; ++g) {
			const uint32_t sg = s0 + g;
#pragma unroll
			for (int k = 0; k < 2; ++k) {
				const uint64_t f = base + 2 * lane + k;
				float2 v = make_float2 (0.f, 0.f);
				bool in;
				if constexpr (ENDS) in = f < rend[g];
				else                in = sg < a.n_streams && f < a.n_frames;
				if (in) {
					if (a.n_channels == 2) v = reinterpret_cast<const float2*> (a.audio)[(size_t) sg * a.stride + f];
					else                   v.x = a.audio[(size_t) sg * a.stride + f];
				}
				raw[g][k] = v;
			}
		}
	};
	auto stage = [&] (int buf, uint64_t base) {
#pragma unroll
		for (int g = 0; g < BANK_ROWS; ++g)
#pragma unroll
			for (int k = 0; k < 2; ++k) {
				const float m = a.n_channels == 2 ? (raw[g][k].x + raw[g][k].y) / 2.0f : raw[g][k].x;   // spectrumlv2.c:216
				// bandpass_process toggles `ac` before use: sample i of the call gets +1e-12 when ac0 ^ 1 ^ (i & 1)
				const int pz = par0[g] ^ 1 ^ (int) ((base + k) & 1);                                       // (2 lane is even)
				mix[buf][g][2 * lane + k] = (double) m + (pz ? 1e-12 : -1e-12);                               // spectr.c:81-82
			}
	};

	// the staged chunk is written by all lanes and read by others: a workgroup-scope release / acquire around a wave barrier
	// makes that hand-over explicit (one wave: no cost but a wait for the LDS writes; ADVICE r3 — in-order LDS alone is not a contract)
	auto handover = [] () {
		__builtin_amdgcn_fence (__ATOMIC_RELEASE, "workgroup");
		__builtin_amdgcn_wave_barrier ();
		__builtin_amdgcn_fence (__ATOMIC_ACQUIRE, "workgroup");
	};
	[[maybe_unused]] uint32_t to_end = 0;     // SERIES: frames to the end of the open block; blocks completed so far
	[[maybe_unused]] uint64_t point = 0;
	if constexpr (SERIES) { to_end = a.e0; point = a.point0; }
	fetch (0);
	stage (0, 0);
	handover ();
	fetch (BANK_CHUNK);
	int buf = 0;
	for (uint64_t base = 0; base < stop; base += BANK_CHUNK, buf ^= 1) {
		const int nf = (int) min ((uint64_t) BANK_CHUNK, stop - base);
		// the next chunk into the other buffer (its previous readers are behind us in this wave's own instruction stream),
		// the one after it into the registers: both land under this chunk's arithmetic
		if (base + BANK_CHUNK < stop) {
			handover ();                                  // (the other buffer's readers of the chunk before are done)
			stage (buf ^ 1, base + BANK_CHUNK);
			handover ();
			fetch (base + 2 * BANK_CHUNK);
		}
		const double* const my = &mix[buf][row][0];
		if constexpr (ENDS) {
			auto frame = [&] (const double in) { BANK_FRAME (in) };
			// spectrum_run's epilogue (spectrumlv2.c:230-238) and, SERIES, the point with the host's peak-reset handshake behind it (:191-198)
			auto epilogue = [&] () {
				if (!isfinite (val)) val = 0;
				if (!isfinite (mx))  mx = 0;
#pragma unroll
				for (int i = 0; i < 12; ++i) if (!isfinite (z[i])) z[i] = 0;
				val += 1e-20f;
				if constexpr (SERIES) {
					if (point < a.cap) {
						const size_t o = ((size_t) s * a.cap + point) * MTR_NBANDS + band;
						a.s_val[o] = val;
						a.s_mx[o]  = mx;
					}
					if (a.peak_block) mx = 0;
				}
			};
			for (int n = 0; n < nf; ) {
				// the piece: to the chunk's end, the block's or the next end of a row, whichever comes first — all uniform
				const uint32_t cur = (uint32_t) base + (uint32_t) n;
				uint32_t len = (uint32_t) (nf - n);
#pragma unroll
				for (int g = 0; g < BANK_ROWS; ++g) if (rend[g] > cur) len = min (len, rend[g] - cur);
				if constexpr (SERIES) { len = min (len, to_end); to_end -= len; }
				const int end = n + (int) len;
				const bool on = cur < my_end;                 // the lane's row has not ended: true or false for the whole piece
				if (on) {
					if ((n & 1) && n < end) { frame (my[n]); ++n; }
#pragma unroll 2
					for (int j = n >> 1; j < end >> 1; ++j) {
						frame (my[2 * j]);
						frame (my[2 * j + 1]);
					}
					if (end > n && (end & 1)) frame (my[end - 1]);
				}
				n = end;
				const bool ended = on && my_end == cur + len;  // the row's last frame
				if constexpr (SERIES) {
					if (to_end == 0) {
						// the block's last frame (a row that ends with it ends there: r = 0, no second epilogue)
						if (on) epilogue ();
						++point;
						to_end = a.period;
					} else if (ended && my_end < (uint32_t) a.n_frames) epilogue ();   // closed r frames into a block: the truncated point (an open stream's call just ends)
				} else if (ended) epilogue ();                    // the stream's spectrum_run of the call ends here
			}
		} else if constexpr (!SERIES) {
			for (int n = 0; n < nf; ++n) BANK_FRAME (my[n])
		} else {
			// (the step behind a lambda: as the compiler stands, this instantiation then takes 120 VGPRs — four waves per SIMD like the dense
			// kernel — against 130 and three waves with the macro spelled out at the four places below; profiles/r24_bank_series.md)
			auto frame = [&] (const double in) { BANK_FRAME (in) };
			for (int n = 0; n < nf; ) {
				const int end = n + (int) min ((uint32_t) (nf - n), to_end);      // uniform: the chunk's end or the block's
				to_end -= (uint32_t) (end - n);
				// a frame to reach an even one, pairs (each one aligned 16-byte read of the row; unrolled twice: the dense loop's four frames per
				// iteration, 28.75 VALU instructions per frame), a frame left over
				if ((n & 1) && n < end) { frame (my[n]); ++n; }
#pragma unroll 2
				for (int j = n >> 1; j < end >> 1; ++j) {
					frame (my[2 * j]);
					frame (my[2 * j + 1]);
				}
				if (end > n && (end & 1)) frame (my[end - 1]);
				n = end;
				if (to_end == 0) {
					// the block's last frame: spectrum_run's epilogue (spectrumlv2.c:230-238), the point, and — MTR_SPECTR_PEAK_BLOCK — the
					// peak-reset handshake of the host that reads it (:191-198)
					if (live) {
						if (!isfinite (val)) val = 0;
						if (!isfinite (mx))  mx = 0;
#pragma unroll
						for (int i = 0; i < 12; ++i) if (!isfinite (z[i])) z[i] = 0;
						val += 1e-20f;
						if (point < a.cap) {
							const size_t o = ((size_t) s * a.cap + point) * MTR_NBANDS + band;
							a.s_val[o] = val;
							a.s_mx[o]  = mx;
						}
						if (a.peak_block) mx = 0;
					}
					++point;
					to_end = a.period;
				}
			}
		}
	}

	if constexpr (ENDS) {
		// every row did its epilogue where it ended: the states as they stand; a row with end 0 is not written at all
		if (live && my_end) {
#pragma unroll
			for (int i = 0; i < 12; ++i) a.z[((size_t) s * MTR_NBANDS + band) * 12 + i] = z[i];
			a.val[(size_t) s * MTR_NBANDS + band] = val;
			a.mx[(size_t) s * MTR_NBANDS + band]  = mx;
		}
		// the parity advances by the stream's own frames; the buffers swap with every call, so end 0 copies it
		if (live && band == 0) a.ac_out[s] = my_par ^ (int) (my_end & 1);
	} else if (live) {
		if constexpr (!SERIES) {
			// spectrum_run epilogue, state part (spectrumlv2.c:230-238)
			if (!isfinite (val)) val = 0;
			if (!isfinite (mx))  mx = 0;
#pragma unroll
			for (int i = 0; i < 12; ++i) {
				if (!isfinite (z[i])) z[i] = 0;
				a.z[((size_t) s * MTR_NBANDS + band) * 12 + i] = z[i];
			}
			a.val[(size_t) s * MTR_NBANDS + band] = val + 1e-20f;
			a.mx[(size_t) s * MTR_NBANDS + band]  = mx;
		} else {
			// the call ends where it ends: the states as they stand (the blocks' ends did the epilogue)
#pragma unroll
			for (int i = 0; i < 12; ++i) a.z[((size_t) s * MTR_NBANDS + band) * 12 + i] = z[i];
			a.val[(size_t) s * MTR_NBANDS + band] = val;
			a.mx[(size_t) s * MTR_NBANDS + band]  = mx;
		}
		// the parity of the next call goes to the OTHER buffer: a wave that starts late must not see this call's update
		if (band == 0) a.ac_out[s] = my_par ^ (int) (a.n_frames & 1);
	}
}

// the four instantiations (dense or series, with ends or without): same grid, same lane map
template <typename A> static int mtr_launch_bank (const A& a, void* stream)
{
	const uint64_t pairs = (uint64_t) a.n_streams * MTR_NBANDS;
	const uint32_t nb = (uint32_t) ((pairs + 63) / 64);
	hipLaunchKernelGGL (k_bank<A>, dim3 (nb), dim3 (64), 0, (hipStream_t) stream, a);
	return hipGetLastError () == hipSuccess ? 0 : -1;
}

// ---- synthetic programme signal ------------------------------------------------------------------
// kind 0: LCG noise (two draws per frame, L then R), u = ((s >> 8) - 2^23) / 2^23
// kind 2: kind 0 under a monotonically rising level (2^-8 .. 1): the pruning-hostile case of bench.py
// kind 1: programme-like: env(t) * (0.5 u + 0.5 sin(2 pi f t)), f_L = 440, f_R = 3000,
//         env = 0.05 + 0.45 (0.5 + 0.5 sin(2 pi 0.2 t)); stream s uses seed + s.
// The LCG is jumped to each thread's position with the closed form s_n = A^n s_0 + C (A^n - 1)/(A - 1),
// evaluated by square-and-multiply on (A, C) pairs, so the fill is embarrassingly parallel and
// reproduces the serial generator bit-for-bit.

__device__ __forceinline__ void lcg_jump (uint32_t n, uint32_t& mul, uint32_t& add)
{
	uint32_t cm = 1664525u, ca = 1013904223u;   // one step
	mul = 1u; add = 0u;
	while (n) {
		if (n & 1u) { mul = mul * cm; add = add * cm + ca; }
		ca = ca * cm + ca;
		cm = cm * cm;
		n >>= 1;
	}
}

#define SYNTH_RUN 256   /* frames per thread */

__global__ void k_synth (float* audio, uint32_t n_streams, uint64_t n_frames, uint64_t stride,
                         uint32_t seed, float fs, int kind)
{
	const uint64_t runs = (n_frames + SYNTH_RUN - 1) / SYNTH_RUN;
	const uint64_t g = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
	if (g >= runs * n_streams) return;
	const uint32_t s = (uint32_t) (g / runs);
	const uint64_t f0 = (g % runs) * SYNTH_RUN;
	uint32_t mul, add;
	lcg_jump ((uint32_t) (2 * f0), mul, add);
	uint32_t st = mul * (seed + s) + add;
	float2* dst = reinterpret_cast<float2*> (audio) + (size_t) s * stride;
	const uint64_t f1 = min (f0 + SYNTH_RUN, n_frames);
	for (uint64_t f = f0; f < f1; ++f) {
		st = 1664525u * st + 1013904223u;
		float ul = (float) (int32_t) ((st >> 8) - 8388608u) * (1.0f / 8388608.0f);
		st = 1664525u * st + 1013904223u;
		float ur = (float) (int32_t) ((st >> 8) - 8388608u) * (1.0f / 8388608.0f);
		if (kind == 1) {
			const float t = (float) f / fs;
			const float env = 0.05f + 0.45f * (0.5f + 0.5f * __sinf (6.2831853f * 0.2f * t));
			// phase reduced in integer arithmetic so long streams stay accurate
			const float pl = (float) ((f * 440ull) % (uint64_t) fs) / fs;
			const float pr = (float) ((f * 3000ull) % (uint64_t) fs) / fs;
			ul = env * (0.5f * ul + 0.5f * __sinf (6.2831853f * pl));
			ur = env * (0.5f * ur + 0.5f * __sinf (6.2831853f * pr));
		} else if (kind == 2) {
			// noise under a level that rises monotonically by 48 dB over the stream: every block's maximum beats everything
			// before it — the worst case of exact peak pruning (nothing can be skipped, every screened block is completed)
			const float env = exp2f (-8.0f + 8.0f * (float) f / (float) n_frames);
			ul *= env; ur *= env;
		}
		dst[f] = make_float2 (ul, ur);
	}
}

int mtr_launch_synth (float* d_audio, uint32_t n_streams, uint64_t n_frames, uint64_t stride,
                      uint32_t seed, float fs, int kind, void* stream)
{
	const uint64_t runs = (n_frames + SYNTH_RUN - 1) / SYNTH_RUN;
	const uint64_t n = runs * n_streams;
	hipLaunchKernelGGL (k_synth, dim3 ((uint32_t) ((n + 255) / 256)), dim3 (256), 0, (hipStream_t) stream,
	                    d_audio, n_streams, n_frames, stride, seed, fs, kind);
	return hipGetLastError () == hipSuccess ? 0 : -1;
}

// ---- SPECTR30 in the engine: set-up, reset, the call's step, the blob's sections, the getters ----------------------------------------

static int bank_create (mtr_engine* e)
{
	const mtr_config* const cfg = &e->cfg;
	const uint32_t S = cfg->n_streams;
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
	if (e->bank.coef.reserve (c.size ()) || e->bank.z.reserve ((size_t) S * MTR_NBANDS * 12)
	    || e->bank.val.reserve ((size_t) S * MTR_NBANDS) || e->bank.max.reserve ((size_t) S * MTR_NBANDS)
	    || e->bank.ac[0].reserve (S) || e->bank.ac[1].reserve (S))
		return fail (MTR_ERR_NOMEM, "hipMalloc bank state");
	if (hipMemcpy (e->bank.coef.p, c.data (), c.size () * sizeof (double), hipMemcpyHostToDevice) != hipSuccess)
		return fail (MTR_ERR_HIP, "hipMemcpy bank_coef");
	e->bank.points.assign (S, 0);
	return MTR_OK;
}

static int bank_reset (mtr_engine* e)
{
	const hipStream_t st = e->last_stream;
	HIPCHK (hipMemsetAsync (e->bank.z.p, 0, e->bank.z.n * sizeof (double), st));
	HIPCHK (hipMemsetAsync (e->bank.val.p, 0, e->bank.val.n * sizeof (float), st));
	HIPCHK (hipMemsetAsync (e->bank.max.p, 0, e->bank.max.n * sizeof (float), st));
	HIPCHK (hipMemsetAsync (e->bank.ac[0].p, 0, e->bank.ac[0].n * sizeof (int32_t), st));
	HIPCHK (hipMemsetAsync (e->bank.ac[1].p, 0, e->bank.ac[1].n * sizeof (int32_t), st));
	e->pos.bank_ac_cur = 0;
	// the reading series: emptied, the open block gone, P, the capacity and the mode kept
	if (e->bank.s_val.n) HIPCHK (hipMemsetAsync (e->bank.s_val.p, 0, e->bank.s_val.n * sizeof (float), st));
	if (e->bank.s_max.n) HIPCHK (hipMemsetAsync (e->bank.s_max.p, 0, e->bank.s_max.n * sizeof (float), st));
	e->pos.bk = {};
	e->bank.points.assign (e->cfg.n_streams, 0);
	return MTR_OK;
}

static int bank_step (mtr_engine* e, const Call& c, Cursors& nx, const StreamEnds& se)
{
	const size_t vo = c.off;
	mtr_bank_args ba;
	ba.audio = c.audio; ba.stride = c.stride; ba.n_frames = c.n_frames;
	ba.coef = e->bank.coef.p; ba.z = e->bank.z.p + vo * MTR_NBANDS * 12; ba.val = e->bank.val.p + vo * MTR_NBANDS; ba.mx = e->bank.max.p + vo * MTR_NBANDS;
	ba.ac_in = e->bank.ac[e->pos.bank_ac_cur].p + vo; ba.ac_out = e->bank.ac[e->pos.bank_ac_cur ^ 1].p + vo;
	ba.n_streams = c.cnt; ba.n_channels = e->cfg.n_channels; ba.omega = e->bank.omega;
	if (const uint32_t P = e->bank.ser.period) {
		// the blocks are cut from where the CALL started (e->pos): every view of a host call sees the same cuts and appends at the same points
		const uint32_t cap = e->bank.ser.cap;
		mtr_bank_series_args sa;
		static_cast<mtr_bank_args&> (sa) = ba;
		sa.s_val = cap ? e->bank.s_val.p + vo * cap * MTR_NBANDS : nullptr;
		sa.s_mx  = cap ? e->bank.s_max.p + vo * cap * MTR_NBANDS : nullptr;
		sa.period = P; sa.e0 = (uint32_t) series_e0 (e->pos.bk, P, c.n_frames); sa.point0 = e->pos.bk.points;
		sa.cap = cap; sa.peak_block = e->bank.peak_mode == MTR_SPECTR_PEAK_BLOCK;
		if (se.ends) {
			// (the ends of the view's own streams: upload_lengths fills them from the view's first stream on, as the kernel indexes them)
			mtr_bank_series_ends_args ea;
			static_cast<mtr_bank_series_args&> (ea) = sa;
			ea.ends = se.ends;
			if (mtr_launch_bank (ea, c.st)) return fail (MTR_ERR_HIP, "k_bank launch (series, ends)");
		} else if (mtr_launch_bank (sa, c.st)) return fail (MTR_ERR_HIP, "k_bank launch (series)");
		nx.bk = series_advance (e->pos.bk, P, c.n_frames);
	} else if (se.ends) {
		mtr_bank_ends_args ea;
		static_cast<mtr_bank_args&> (ea) = ba;
		ea.ends = se.ends;
		if (mtr_launch_bank (ea, c.st)) return fail (MTR_ERR_HIP, "k_bank launch (ends)");
	} else if (mtr_launch_bank (ba, c.st)) return fail (MTR_ERR_HIP, "k_bank launch");
	nx.bank_ac_cur = e->pos.bank_ac_cur ^ 1;
	return MTR_OK;
}

static void bank_sections (const mtr_engine* e, std::vector<StateSection>& v)
{
	v.push_back ({ e->bank.z.p, (size_t) MTR_NBANDS * 12 * sizeof (double) });
	v.push_back ({ e->bank.val.p, (size_t) MTR_NBANDS * sizeof (float) });
	v.push_back ({ e->bank.max.p, (size_t) MTR_NBANDS * sizeof (float) });
	v.push_back ({ e->bank.ac[e->pos.bank_ac_cur].p, sizeof (int32_t) });
}

static SeriesView bank_series (mtr_engine* e) { return { &e->bank.ser, &Cursors::bk, &e->bank.points }; }

constinit SideMeter bank_meter = { .bits = MTR_METER_SPECTR30, .create = bank_create, .reset = bank_reset, .step = bank_step, .sections = bank_sections, .series = bank_series };

// With a period the blob carries one more section, behind every older one (the second row of the meter in SIDE_METERS): where the open block
// stands.  All of an entry is its host-owned header — period, peak mode, the frames into the open block; the block's levels and filter states are
// the first row's, stored as they stand.  An engine takes a blob of its own period and mode only.  The ring is not part of the blob.
struct mtr_bank_open { uint32_t period, peak_mode, fill; };

static void bank_open_sections (const mtr_engine* e, std::vector<StateSection>& v)
{
	if (e->bank.ser.period) v.push_back ({ e->bank.open.p, sizeof (mtr_bank_open) });
}

constexpr const char* BANK_CORRUPT = "mtr_engine_state_import: corrupt blob (period of the SPECTR30 series)";

static void bank_hdr_write (const mtr_engine* e, void* out)
{
	const mtr_bank_open h = { e->bank.ser.period, (uint32_t) e->bank.peak_mode, (uint32_t) e->pos.bk.fill };
	memcpy (out, &h, sizeof (h));
}

static int bank_hdr_check (const mtr_engine* e, const void* in, bool fresh)
{
	mtr_bank_open h;
	memcpy (&h, in, sizeof (h));
	if (!h.period || !series_blob_ok (h.period, h.fill, 1, 0x7ffffffeu) || h.peak_mode > MTR_SPECTR_PEAK_BLOCK) return fail (MTR_ERR_STATE, BANK_CORRUPT);
	if (h.period != e->bank.ser.period || (int) h.peak_mode != e->bank.peak_mode || (!fresh && h.fill != e->pos.bk.fill))
		return fail (MTR_ERR_STATE, "mtr_engine_state_import: the engine does not stand where the blob's streams do (period or peak mode of the SPECTR30 series)");
	return MTR_OK;
}

static void bank_hdr_take (mtr_engine* e, const void* in)
{
	mtr_bank_open h;
	memcpy (&h, in, sizeof (h));
	e->pos.bk.fill = h.fill;
}

static constinit BlobHeader bank_hdr = { .offset = 0, .bytes = sizeof (mtr_bank_open), .corrupt = BANK_CORRUPT, .write = bank_hdr_write, .check = bank_hdr_check, .take = bank_hdr_take };
// (no reset and no step: the meter's first row resets and queues all of it)
constinit SideMeter bank_series_meter = { .bits = MTR_METER_SPECTR30, .sections = bank_open_sections, .hdr = &bank_hdr };

// spectrumlv2.c:240-247 for n levels: the raw val_f / max_f and the dB values of ports 0-29 / 30-59 (any output may be null).  The stored val
// carries the +1e-20f of :237; above the -100 dB floor (val > 5e-11) that addition does not change the float, so the port value is unaffected.
static void bank_ports (const float* v, const float* m, size_t n, float* val, float* mx, float* val_db, float* max_db)
{
	for (size_t i = 0; i < n; ++i) {
		const float vs = sqrtf (2. * v[i]);
		const float ms = sqrtf (2. * m[i]);
		if (val) val[i] = v[i];
		if (mx) mx[i] = m[i];
		if (val_db) val_db[i] = vs > .00001f ? 20.0 * log10f (vs) : -100.0;
		if (max_db) max_db[i] = ms > .00001f ? 20.0 * log10f (ms) : -100.0;
	}
}

static int no_bank (const mtr_engine* e) { return !e || !(e->cfg.meters & MTR_METER_SPECTR30); }
static const char* const NO_BANK = "no SPECTR30 in this engine";

extern "C" {

int mtr_engine_spectr_set_speed (mtr_engine* e, float v)
{
	if (!e) return fail (MTR_ERR_ARG, "null engine");
	if (v < 0.01) v = 0.01;                                    // spectrumlv2.c:172-175
	if (v > 15.0) v = 15.0;
	e->bank.omega = 1.0f - expf (-2.0 * M_PI * v / (double) e->cfg.sample_rate);
	return MTR_OK;
}

int mtr_engine_spectr_reset_peak (mtr_engine* e)
{
	if (!e || !(e->cfg.meters & MTR_METER_SPECTR30)) return fail (MTR_ERR_ARG, "no SPECTR30 in this engine");
	e->snap_valid = false;
	HIPCHK (hipSetDevice (e->cfg.device));
	HIPCHK (hipMemsetAsync (e->bank.max.p, 0, e->bank.max.n * sizeof (float), e->last_stream));
	e->queued = true;
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
		HIPCHK (hipMemcpy (hv.data (), e->bank.val.p + (size_t) first * MTR_NBANDS, n * 4, hipMemcpyDeviceToHost));
		HIPCHK (hipMemcpy (hv.data () + n, e->bank.max.p + (size_t) first * MTR_NBANDS, n * 4, hipMemcpyDeviceToHost));
		v = hv.data (); m = hv.data () + n;
	}
	bank_ports (v, m, n, val, mx, val_db, max_db);
	return MTR_OK;
}

int mtr_engine_spectr_set_period (mtr_engine* e, uint32_t period_frames, uint32_t capacity_points, int peak_mode)
{
	if (no_bank (e)) return fail (MTR_ERR_ARG, NO_BANK);
	if (peak_mode != MTR_SPECTR_PEAK_HOLD && peak_mode != MTR_SPECTR_PEAK_BLOCK)
		return fail (MTR_ERR_ARG, "mtr_engine_spectr_set_period: peak_mode is MTR_SPECTR_PEAK_HOLD or MTR_SPECTR_PEAK_BLOCK");
	if (period_frames >= 0x7fffffffu) return fail (MTR_ERR_ARG, "mtr_engine_spectr_set_period: a period is at most 2^31 - 2 frames");
	int rc = series_configure_check (e, "mtr_engine_spectr_set_period", period_frames, 1, "1");
	if (rc || (rc = wait_stream (e))) return rc;
	mtr_engine::Bank& b = e->bank;
	b.ser = {};                                                        // (off until everything below has succeeded)
	b.peak_mode = MTR_SPECTR_PEAK_HOLD;
	e->pos.bk = {};
	b.s_val.drop (); b.s_max.drop (); b.open.drop ();
	if (!period_frames) return MTR_OK;
	const size_t n = (size_t) e->cfg.n_streams * capacity_points * MTR_NBANDS;
	if ((rc = series_ring (b.s_val, n, "hipMalloc SPECTR30 series")) || (rc = series_ring (b.s_max, n, "hipMalloc SPECTR30 series"))) { b.s_val.drop (); b.s_max.drop (); return rc; }
	if (b.open.reserve ((size_t) e->cfg.n_streams * sizeof (mtr_bank_open))) { b.s_val.drop (); b.s_max.drop (); return fail (MTR_ERR_NOMEM, "hipMalloc SPECTR30 open blocks"); }
	HIPCHK (hipMemset (b.open.p, 0, b.open.n));
	b.ser = { period_frames, capacity_points };
	b.peak_mode = peak_mode;
	return MTR_OK;
}

// mtr_ends.h: counted on the host by CallRun::run
int mtr_engine_spectr_points (mtr_engine* e, uint32_t first, uint32_t count, uint64_t* points)
{
	if (no_bank (e)) return fail (MTR_ERR_ARG, NO_BANK);
	if (!points) return fail (MTR_ERR_ARG, "mtr_engine_spectr_points: null argument");
	if ((uint64_t) first + count > e->cfg.n_streams) return fail (MTR_ERR_ARG, "stream range");
	series_points_of (e, MTR_METER_SPECTR30, first, count, points);
	return MTR_OK;
}

int mtr_engine_spectr_period (const mtr_engine* e, uint32_t* period_frames, uint32_t* capacity_points, int* peak_mode)
{
	if (no_bank (e)) return fail (MTR_ERR_ARG, NO_BANK);
	if (period_frames) *period_frames = e->bank.ser.period;
	if (capacity_points) *capacity_points = e->bank.ser.cap;
	if (peak_mode) *peak_mode = e->bank.peak_mode;
	return MTR_OK;
}

int mtr_engine_spectr_series (mtr_engine* e, uint32_t first, uint32_t count, float* val, float* mx, float* val_db, float* max_db,
                              uint32_t capacity, uint32_t* n_points, uint32_t* dropped)
{
	int rc = meter_range (e, !no_bank (e), NO_BANK, first, count);
	if (rc) return rc;
	if (!e->bank.ser.period) return fail (MTR_ERR_ARG, "mtr_engine_spectr_series: the series is off (mtr_engine_spectr_set_period)");
	const uint32_t cap = e->bank.ser.cap;
	const size_t take = series_counts (e->pos.bk.points, cap, capacity, n_points, dropped);
	if ((!val && !mx && !val_db && !max_db) || !count || !take) return MTR_OK;
	if ((rc = wait_stream (e))) return rc;
	// the kept points of the streams, rows of `take` points; then the ports' arithmetic row by row into the caller's rows of `capacity`
	const size_t w = take * MTR_NBANDS;
	std::vector<float> hv (2 * (size_t) count * w);
	float* const hm = hv.data () + (size_t) count * w;
	if ((rc = series_fetch (hv.data (), e->bank.s_val.p, MTR_NBANDS, first, cap, (uint32_t) take, take, count))) return rc;
	if ((rc = series_fetch (hm, e->bank.s_max.p, MTR_NBANDS, first, cap, (uint32_t) take, take, count))) return rc;
	for (uint32_t k = 0; k < count; ++k) {
		const size_t o = (size_t) k * capacity * MTR_NBANDS;
		bank_ports (hv.data () + k * w, hm + k * w, w, val ? val + o : nullptr, mx ? mx + o : nullptr, val_db ? val_db + o : nullptr, max_db ? max_db + o : nullptr);
	}
	return MTR_OK;
}

} // extern "C"
