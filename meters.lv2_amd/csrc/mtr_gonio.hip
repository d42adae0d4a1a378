// mtr_gonio.hip — the goniometer (draw_rb, gui/goniometer.c:299-538: points mode, infinite persistence, no inflate; oversampling by 2 .. 32
// as an option: k_gonio_os, further down, and k_history's 23-frame rows) for a batch: the M/S point image as counts per cell, the auto gain, a point per
// display update (gfx950).
//
// Per frame (:401-449), all in f32 and in the reference's order — this file is compiled without FMA contraction and without fast-math,
// f32 subnormals are kept:
//     lp += hpw (d - lp), lp += 1e-12f per channel;  ax = lp0 - lp1, ay = lp0 + lp1;  x = 186.5f - gain ax 100.f, y alike;
//     l2 = (last_x - x)^2 + (last_y - y)^2;  l2 < 2.0: the frame is skipped;  else last_x = x, last_y = y and the rectangle of :470 is painted
// and, with auto gain, the extremes of ax, ay and the sums of lp0^2, lp1^2 of the display update.  A display update is a BLOCK of exactly P
// frames, wherever the calls cut the audio; at its end (:494-537) an lp that is not finite becomes 0, the gain moves (auto gain) and a
// point (gain, painted inside the surface, painted outside) is appended to the stream's series.
//
// Serial in time, per stream: the two lp chains, the skip rule (it hangs on the last PAINTED point), the rms sums (serial f32 sums), the
// gain from block to block.  Not serial: the image — integer adds commute.  So a call is walked in pieces of `tune_piece` frames, two
// kernels per piece:
//   k_gonio_points  the chain.  Lane = stream; a workgroup is ONE wave and takes NS streams (16: 512 waves at 8192 streams; 64 from 16384
//                   streams up, where the chip is full either way and idle lanes would cost issue slots).  All 64 lanes stage chunks of
//                   2048 / NS frames per stream into LDS by 16-byte loads (a row whose chunk does not start on 16 bytes, and the chunk at
//                   the piece's end, dword by dword), the next chunk in flight in registers under the chain; a row is padded by one frame:
//                   the chain lanes read the same frame of different rows, two banks apart (ds_read_b64, conflict-free in both lane
//                   groups), eight frames' reads issued together.  State in registers across the piece; the streams stand in lock step, so
//                   a block's end is scalar control flow, and a frame has no branch at all: skip rule, range test and counts are selects
//                   and masks, so the scheduler runs frame k + 1's filters under frame k's point.  Per frame the lane leaves a uint16 CELL
//                   CODE — (py >> shift) G + (px >> shift), or 0xFFFF: nothing to add — in an LDS row of its own (odd pitch in dwords: no
//                   conflicts); per chunk the wave copies the rows out to the engine's scratch [S][piece] in 16-byte stores.  It counts
//                   drawn / clipped / skipped itself, does the gain update at a block's end and stores the series point, with plain
//                   vector stores.
//   k_gonio_image   the histogram.  A workgroup owns one stream: its image in LDS (shift 1: 139 888 B, 1024 threads — one workgroup per CU;
//                   shift 2: 35 344 B, 256 threads — four per CU; shift 3: 8 848 B — the wave slots bound it), the cell codes read
//                   coalesced, 16 bytes per lane, added with LDS integer atomics (ds_add_u32); at the end the image is walked in 16-byte
//                   quads and those that are not zero — few, in a piece of 4096 frames — are added onto the stream's image in global
//                   memory with plain loads and stores — one workgroup owns the stream: no global atomics.
// (atomicAdds from the chain lanes straight onto [S][G][G] would put one lane on each destination row: an order of magnitude below the
// atomic rate.)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <type_traits>
#include <vector>

#include "mtr_engine_impl.h"

/* the blob's copy of the configuration and the cursor, in front of every stream's entry (the host's copies rule; export writes them in) */
typedef struct mtr_gonio_hdr {
	uint32_t period, shift, autogain, fill;
} mtr_gonio_hdr;

/* a stream's entry: this, then its image uint32 [G][G] */
typedef struct mtr_gonio_state {
	mtr_gonio_hdr hdr;
	float    lp0, lp1, last_x, last_y, gain;       /* ui->lp0 lp1 last_x last_y gain */
	float    xmax, xmin, ymax, ymin, rms0, rms1;   /* the open block's ag_xmax .. ag_ymin, rms_0, rms_1 (:379-385) */
	uint32_t b_drawn, b_clipped;                   /* ... and its points painted inside / outside the surface */
	uint32_t pad;
	uint64_t drawn, clipped, skipped;              /* frames since reset / image_clear, the open block's included */
} mtr_gonio_state;
static_assert (sizeof (mtr_gonio_state) == 96, "mtr_gonio_state");

typedef struct mtr_gonio_args {
	const float*   audio;        /* [S][stride][2] */
	uint64_t       stride;
	uint64_t       f0;           /* the piece's first frame in the call */
	uint32_t       n;            /* ... and its frames */
	uint32_t       n_streams;
	uint32_t       P, fill;      /* frames per block; frames into the open block at the piece's start */
	uint64_t       point0;       /* blocks completed before the piece */
	uint32_t       capacity, shift, G;
	uint32_t       code_pitch;   /* codes per stream of the scratch: a multiple of 128 */
	float          hpw, attack[2], g_target, g_rms;
	float          hw;           /* line_width * .5 (:470): exact in f32 */
	unsigned char* state;        /* [S] of { mtr_gonio_state, image }, `pitch` bytes each */
	uint64_t       pitch;
	float*         s_gain;       /* [S][capacity], from the view's first stream */
	uint32_t*      s_drawn;
	uint32_t*      s_clipped;
	uint16_t*      codes;        /* [S][code_pitch] */
} mtr_gonio_args;

/* per-stream ends (mtr_gonio_ends.h): what the ENDS instantiations take on top — a struct of its own, so that the dense kernels' arguments
 * stay what they were.  All three from the view's first stream, written by CallRun::upload_lengths */
typedef struct mtr_gonio_ends_args : mtr_gonio_args {
	const uint32_t* cut;         /* [S] the call frame at which the stream's drawing ends; MTR_GONIO_OPEN: not in this call; 0: closed, untouched */
	const uint32_t* closing;     /* [S] r, the frames of the closing display update behind the cut (>= 64), or 0: none */
	const float*    c_attack;    /* [S][2] `attack` of :524 for elapsed = r / rate */
} mtr_gonio_ends_args;
constexpr uint32_t MTR_GONIO_OPEN = 0xFFFFFFFFu;

namespace {

// the frames of the piece in front of a stream's cut: 0 .. n
__device__ inline int gonio_limit (uint32_t cut, uint64_t f0, int n)
{
	return cut == MTR_GONIO_OPEN ? n : (uint64_t) cut <= f0 ? 0 : (int) min ((uint64_t) cut - f0, (uint64_t) n);
}

// ENDS (mtr_gonio_ends.h): stream s draws the frames in front of call frame a.cut[s] and no other.  The streams still stand in lock step —
// j and point go on for every lane — so a chunk in which no live lane's cut falls runs the dense body as it is: a lane whose cut lies
// behind it (a DEAD lane: it stored its state at its cut and stores nothing any more) computes on the zeros its row was staged with, and
// nothing of that is kept.  A chunk that holds a cut takes the cold path: frame by frame, each lane up to its own limit, code 0xFFFF
// behind it; then the lanes that end here run their closing update (its own count r and attack pair), store their point and their state
// and die.  A workgroup (one wave) whose lanes are all dead leaves the chunk loop.  Staging never loads a frame at or behind its row's cut.
template <int NS, bool AG, bool ENDS = false>
__global__ __launch_bounds__ (64) void k_gonio_points (const std::conditional_t<ENDS, mtr_gonio_ends_args, mtr_gonio_args> a)
{
	constexpr int CH = 2048 / NS;                // frames per staged chunk
	constexpr int PITCH = 2 * CH + 2;            // dwords of a row's chunk, padded by one frame
	constexpr int NQ = CH / 2;                   // 16-byte quads (two frames) of a row's chunk
	constexpr int PER = NS * NQ / 64;            // ... per lane: 16
	constexpr int CP = CH / 2 + 1;               // dwords of a row of cell codes: odd
	constexpr int CQ = CH / 8;                   // 16-byte quads of a row of cell codes
	constexpr int CPER = NS * CQ / 64;           // ... per lane: 4
	__shared__ float lds[NS * PITCH];
	__shared__ uint32_t cds[(NS + (ENDS && NS < 64 ? 1 : 0)) * CP];   // (ENDS: a row behind the last for the idle lanes, which no longer mirror lane 0)
	__shared__ int rlim[ENDS ? NS : 1];          // ENDS: the rows' frame limits in the piece

	const int lane = threadIdx.x;
	const uint32_t s0 = blockIdx.x * NS;
	const int n = (int) a.n;
	const int nchunks = (n + CH - 1) / CH;
	int lim = n;                                 // ENDS: the lane's own
	bool ends_here = false;                      // ... and whether its drawing ends in this piece
	if constexpr (ENDS) {
		const uint32_t sl = s0 + (uint32_t) lane;
		if (lane < NS) {
			const uint32_t cut = sl < a.n_streams ? a.cut[sl] : 0u;
			lim = gonio_limit (cut, a.f0, n);
			ends_here = cut != MTR_GONIO_OPEN && (uint64_t) cut <= a.f0 + (uint64_t) n;
			rlim[lane] = lim;
		}
		__syncthreads ();
	}

	// ---- staging: item i = (row, quad) ----
	float4 pre[PER];
	auto fetch = [&] (int T) __attribute__ ((always_inline)) {
#pragma unroll
		for (int j = 0; j < PER; ++j) {
			const int i = lane + j * 64, r = i / NQ, q = i - r * NQ;
			const uint32_t s = s0 + (uint32_t) r;
			const int f = T + 2 * q;                                   // the quad's first frame in the piece
			float4 v = float4{0.f, 0.f, 0.f, 0.f};
			int rn = n;                                                // (ENDS: no frame at or behind the row's cut is loaded)
			if constexpr (ENDS) rn = rlim[r];
			if (s < a.n_streams && f < rn) {
				const float* const p = a.audio + ((uint64_t) s * a.stride + a.f0 + (uint64_t) f) * 2;
				if (f + 1 < rn && (reinterpret_cast<size_t> (p) & 15) == 0) v = *reinterpret_cast<const float4*> (p);
				else {
					v.x = p[0]; v.y = p[1];
					if (f + 1 < rn) { v.z = p[2]; v.w = p[3]; }
				}
			}
			pre[j] = v;
		}
	};
	auto stash = [&] () __attribute__ ((always_inline)) {
#pragma unroll
		for (int j = 0; j < PER; ++j) {
			const int i = lane + j * 64, r = i / NQ, q = i - r * NQ;
			float2* const dst = reinterpret_cast<float2*> (&lds[r * PITCH + 4 * q]);
			dst[0] = float2{pre[j].x, pre[j].y};
			dst[1] = float2{pre[j].z, pre[j].w};
		}
	};

	// ---- the chain: lane = stream ----
	const uint32_t s = s0 + (uint32_t) lane;
	bool live = lane < NS && s < a.n_streams;
	if constexpr (ENDS) {
		live = live && lim > 0;                                        // (a closed stream, or one whose cut lies in front of the piece)
		if (!__any (live)) return;                                     // (the workgroup is one wave: uniform)
	}
	mtr_gonio_state* const st = reinterpret_cast<mtr_gonio_state*> (a.state + (size_t) (live ? s : s0) * a.pitch);
	float lp0 = st->lp0, lp1 = st->lp1, last_x = st->last_x, last_y = st->last_y, gain = st->gain;
	float xmax = st->xmax, xmin = st->xmin, ymax = st->ymax, ymin = st->ymin, rms0 = st->rms0, rms1 = st->rms1;
	uint32_t bd = st->b_drawn, bc = st->b_clipped;
	const uint32_t bd_in = bd, bc_in = bc;
	uint32_t td = 0, tc = 0;                                           // of the blocks the piece completed
	const float hpw = a.hpw;
	const float hwf = a.hw;
	const int shift = (int) a.shift, G = (int) (a.G & 0xFFu);              // (G <= 187: a 24-bit multiply)
	const uint32_t P = a.P;
	uint32_t j = a.fill;
	uint64_t point = a.point0;
	const float* const row = &lds[(lane < NS ? lane : 0) * PITCH];
	uint16_t* const crow = reinterpret_cast<uint16_t*> (&cds[(lane < NS ? lane : ENDS ? NS : 0) * CP]);

	// one frame: branch-free, so that the scheduler can run frame k + 1's filters under frame k's point
	auto frame = [&] (float2 d, int k) __attribute__ ((always_inline)) {
		lp0 += hpw * (d.x - lp0);                                          // :401-405
		lp1 += hpw * (d.y - lp1);
		lp0 += 1e-12f;
		lp1 += 1e-12f;
		const float ax = lp0 - lp1, ay = lp0 + lp1;
		if constexpr (AG) {                                                // :413-421
			if (ax > xmax) xmax = ax;
			if (ax < xmin) xmin = ax;
			if (ay > ymax) ymax = ay;
			if (ay < ymin) ymin = ay;
			rms0 += lp0 * lp0;
			rms1 += lp1 * lp1;
		}
		const float x = 186.5f - gain * ax * 100.f, y = 186.5f - gain * ay * 100.f;   // :441-442
		const float l2 = (last_x - x) * (last_x - x) + (last_y - y) * (last_y - y);
		const bool paint = !(l2 < 2.0f);                                   // :446 `continue` otherwise; a NaN is painted
		last_x = paint ? x : last_x;
		last_y = paint ? y : last_y;
		// :470 rintf (last_x - line_width * .5): the double difference of two f32 values, rounded to f32, IS their f32 difference — a double
		// has 53 >= 2 * 24 + 2 bits, so rounding twice is innocuous for a sum — and line_width * .5 is an f32 exactly (configure checks)
		const float px = rintf (x - hwf), py = rintf (y - hwf);
		// 0 <= px < 373 for a px that rintf made whole, or NaN (which fails): |px - 186| <= 186, the difference exact where it matters
		const bool in = fabsf (px - 186.f) <= 186.f && fabsf (py - 186.f) <= 186.f;
		// (the cast behind a clamp: NaN occurs.  No select with a costly arm anywhere here, or the compiler turns it into a branch per frame,
		// which the scheduler cannot move the next frame's filters across)
		const int cx = (int) fminf (fmaxf (px, 0.f), 372.f) >> shift, cy = (int) fminf (fmaxf (py, 0.f), 372.f) >> shift;
		const uint32_t hit = paint && in ? 1u : 0u, out = paint && !in ? 1u : 0u;
		bd += hit;
		bc += out;
		crow[k] = (uint16_t) ((uint32_t) (__mul24 (cy, G) + cx) | (hit - 1u));   // (cy, G < 2^8; not hit: 0xFFFF)
	};
	auto at = [&] (int k) __attribute__ ((always_inline)) { return *reinterpret_cast<const float2*> (row + 2 * k); };

	fetch (0);
	for (int c = 0; c < nchunks; ++c) {
		if constexpr (ENDS) if (!__any (live)) break;
		stash ();
		__syncthreads ();
		if (c + 1 < nchunks) fetch ((c + 1) * CH);
		const int nf = min (CH, n - c * CH);
		int k = 0;
		if constexpr (ENDS) {
			// the cold path's block end (:494-537 for the lane itself): `cnt` frames, its attack pair, its point at index `pt`.  (Defined here: a closure
			// in the dense instantiations, used or not, moves their register allocation — they are the parent's instruction streams)
			auto update = [&] (float cnt, float att0, float att1, uint64_t pt) __attribute__ ((always_inline)) {
				if (!isfinite (lp0)) lp0 = 0.f;
				if (!isfinite (lp1)) lp1 = 0.f;
				if constexpr (AG) {
					const float xdif = xmax - xmin, ydif = ymax - ymin;
					float mx = (float) sqrt ((double) (xdif * xdif + ydif * ydif));
					mx = (float) ((double) mx * .707);
					if (a.g_rms > 0.f && isfinite (a.g_rms)) {
						const float r = rms0 > rms1 ? sqrtf (rms0 / cnt) : sqrtf (rms1 / cnt);
						const float rms = (float) (5.436 * (double) r);
						mx = (float) ((double) mx * (1.0 - (double) a.g_rms) + (double) rms * (double) a.g_rms);
					}
					mx *= a.g_target;
					if (!isfinite (mx)) mx = 0.f;
					float tg;
					if ((double) mx < .01) tg = 100.0f;
					else if (mx > 100.0f) tg = .02f;
					else tg = (float) (2.0 / (double) mx);
					const float attack = tg < gain ? att0 : att1;
					tg = gain + attack * (tg - gain);
					if ((double) tg < .001) tg = .001f;
					gain = tg;
					xmax = xmin = ymax = ymin = rms0 = rms1 = 0.f;
				}
				if (pt < a.capacity) {
					const size_t slot = (size_t) s * a.capacity + pt;
					a.s_gain[slot] = gain; a.s_drawn[slot] = bd; a.s_clipped[slot] = bc;
				}
				td += bd; tc += bc;
				bd = bc = 0;
			};
			if (__any (live && ends_here && lim <= c * CH + nf)) {         // the cold path: some live lane's cut falls in this chunk
				for (; k < nf; ++k) {
					const bool on = live && c * CH + k < lim;
					if (on) frame (at (k), k);
					else crow[k] = (uint16_t) 0xFFFFu;
					if (++j == P) {                                        // (a block that ends at the lane's cut is still a whole one)
						if (on) update ((float) P, a.attack[0], a.attack[1], point);
						++point;
						j = 0;
					}
				}
				if (live && ends_here && lim <= c * CH + nf) {
					const uint32_t r = a.closing[s];
					if (r) update ((float) r, a.c_attack[2 * (size_t) s], a.c_attack[2 * (size_t) s + 1], a.point0 + ((uint64_t) a.fill + (uint32_t) lim) / P);
					st->lp0 = lp0; st->lp1 = lp1; st->last_x = last_x; st->last_y = last_y; st->gain = gain;
					st->xmax = xmax; st->xmin = xmin; st->ymax = ymax; st->ymin = ymin; st->rms0 = rms0; st->rms1 = rms1;
					st->b_drawn = bd; st->b_clipped = bc;
					const uint32_t dd = td + bd - bd_in, dc = tc + bc - bc_in;
					st->drawn += dd; st->clipped += dc; st->skipped += (uint32_t) lim - dd - dc;
					live = false;
				}
			}
		}
		while (k < nf) {
			int run = (int) min ((uint32_t) (nf - k), P - j);
			j += (uint32_t) run;
			for (; run >= 8; run -= 8, k += 8) {                           // eight frames' LDS reads issued together
				const float2 d0 = at (k), d1 = at (k + 1), d2 = at (k + 2), d3 = at (k + 3), d4 = at (k + 4), d5 = at (k + 5), d6 = at (k + 6), d7 = at (k + 7);
				frame (d0, k); frame (d1, k + 1); frame (d2, k + 2); frame (d3, k + 3);
				frame (d4, k + 4); frame (d5, k + 5); frame (d6, k + 6); frame (d7, k + 7);
			}
			for (; run > 0; --run, ++k) frame (at (k), k);
			if (j == P) {                                                  // :494-537 (scalar: the streams stand in lock step)
				if (!isfinite (lp0)) lp0 = 0.f;
				if (!isfinite (lp1)) lp1 = 0.f;
				if constexpr (AG) {
					const float xdif = xmax - xmin, ydif = ymax - ymin;
					float mx = (float) sqrt ((double) (xdif * xdif + ydif * ydif));
					mx = (float) ((double) mx * .707);
					if (a.g_rms > 0.f && isfinite (a.g_rms)) {
						const float cnt = (float) P;                           // rms_c
						const float r = rms0 > rms1 ? sqrtf (rms0 / cnt) : sqrtf (rms1 / cnt);
						const float rms = (float) (5.436 * (double) r);
						mx = (float) ((double) mx * (1.0 - (double) a.g_rms) + (double) rms * (double) a.g_rms);
					}
					mx *= a.g_target;
					if (!isfinite (mx)) mx = 0.f;
					float tg;
					if ((double) mx < .01) tg = 100.0f;
					else if (mx > 100.0f) tg = .02f;
					else tg = (float) (2.0 / (double) mx);
					const float attack = tg < gain ? a.attack[0] : a.attack[1];
					tg = gain + attack * (tg - gain);
					if ((double) tg < .001) tg = .001f;
					gain = tg;
					xmax = xmin = ymax = ymin = rms0 = rms1 = 0.f;
				}
				if (live && point < a.capacity) {
					const size_t slot = (size_t) s * a.capacity + point;
					a.s_gain[slot] = gain; a.s_drawn[slot] = bd; a.s_clipped[slot] = bc;
				}
				td += bd; tc += bc;
				bd = bc = 0;
				++point;
				j = 0;
			}
		}
		__syncthreads ();
		// the chunk's cell codes: rows of CH codes out of the LDS, 16 bytes per lane (what lies behind the piece's last frame is not read)
#pragma unroll
		for (int jj = 0; jj < CPER; ++jj) {
			const int i = lane + jj * 64, r = i / CQ, q = i - r * CQ;
			const uint32_t sr = s0 + (uint32_t) r;
			int rn = n;                                                    // (ENDS: nor what lies behind the row's cut)
			if constexpr (ENDS) rn = rlim[r];
			if (sr < a.n_streams && c * CH + 8 * q < rn) {
				const uint32_t* const src = &cds[r * CP + 4 * q];
				*reinterpret_cast<uint4*> (a.codes + (size_t) sr * a.code_pitch + (size_t) c * CH + 8 * q) = uint4{src[0], src[1], src[2], src[3]};
			}
		}
		__syncthreads ();
	}
	if (!live) return;
	st->lp0 = lp0; st->lp1 = lp1; st->last_x = last_x; st->last_y = last_y; st->gain = gain;
	st->xmax = xmax; st->xmin = xmin; st->ymax = ymax; st->ymin = ymin; st->rms0 = rms0; st->rms1 = rms1;
	st->b_drawn = bd; st->b_clipped = bc;
	const uint32_t dd = td + bd - bd_in, dc = tc + bc - bc_in;
	st->drawn += dd; st->clipped += dc; st->skipped += (uint32_t) n - dd - dc;
}

// NT threads own one stream.  The image is walked in uint4: the LDS copy is padded to a multiple of four cells, and so is the stream's
// entry in global memory (its pitch is a multiple of 16 bytes behind a 96-byte state) — the pad cells stay zero: no code names them
// ENDS: the stream's frames of the piece in front of its cut take the place of n — one scalar load, the workgroup is a stream: what an
// earlier piece left in the scratch behind the cut is not added, and a stream with nothing in the piece returns before it clears its image
template <int G, int NT, bool ENDS = false>
__global__ __launch_bounds__ (NT) void k_gonio_image (const std::conditional_t<ENDS, mtr_gonio_ends_args, mtr_gonio_args> a)
{
	constexpr int CELLS = G * G, QUADS = (CELLS + 3) / 4;
	__shared__ uint4 img4[QUADS];
	uint32_t* const img = reinterpret_cast<uint32_t*> (img4);
	const int tid = threadIdx.x;
	const uint32_t s = blockIdx.x;
	int n = (int) a.n;
	if constexpr (ENDS) {
		n = gonio_limit (a.cut[s], a.f0, n);
		if (n == 0) return;
	}
	for (int i = tid; i < QUADS; i += NT) img4[i] = uint4{0u, 0u, 0u, 0u};
	__syncthreads ();
	const uint16_t* const row = a.codes + (size_t) s * a.code_pitch;
	for (int i = tid * 8; i < n; i += NT * 8) {
		const uint4 v = *reinterpret_cast<const uint4*> (row + i);
		const uint32_t w[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
		for (int e = 0; e < 8; ++e) {
			const uint32_t code = (w[e >> 1] >> (16 * (e & 1))) & 0xFFFFu;
			if (i + e < n && code < (uint32_t) CELLS) atomicAdd (&img[code], 1u);
		}
	}
	__syncthreads ();
	uint4* const out = reinterpret_cast<uint4*> (a.state + (size_t) s * a.pitch + sizeof (mtr_gonio_state));
	for (int i = tid; i < QUADS; i += NT) {
		const uint4 v = img4[i];
		if (v.x | v.y | v.z | v.w) {                                       // (most quads of a piece are empty: nothing is loaded or stored for them)
			uint4 o = out[i];
			o.x += v.x; o.y += v.y; o.z += v.z; o.w += v.w;
			out[i] = o;
		}
	}
}

constexpr uint32_t cells_of (uint32_t shift) { return (MTR_GONIO_BOUNDS + (1u << shift) - 1) >> shift; }

// ---- oversampling (mtr_gonio_os.h): the Resampler in front of draw_rb (gui/goniometer.c:359-377; zita-resampler/resampler.cc:215-228) ----
// With a factor f above 1 a piece is walked by three kernels: k_gonio_os writes the piece's n f points [S][n f][2] into the engine's
// scratch, then k_gonio_points and k_gonio_image run on that scratch as on a call's buffer — audio = the scratch, stride = its pitch,
// f0 = 0, with P f, fill f, n f and the oversampled hpw — and behind the call's last piece k_history (mtr_history.hip, HIST_ROW_GONIO:
// gonio_os_step) leaves every stream's last 23 input frames for the next call.
//   k_gonio_os    throughput work: every point is independent of every other.  A workgroup of 256 lanes takes a tile of OS_TILE input
//                 frames of one stream: the table (pitch 13 dwords: the lanes of a wave read f different rows at the same tap, 13 is odd, so
//                 up to 32 rows fall into different banks) and the tile with its 23-frame halo (from the call's buffer, or — in front of the
//                 call's first frame — from the stream's history row) go into LDS; a lane takes one point and both its channels, two serial
//                 sums of 12 steps in exactly the reference's operations (two products, their sum, the sum onto s: this file is built without
//                 contraction), the frames read as ds_read_b64 (lanes of one frame: a broadcast; of neighbouring frames: neighbouring banks),
//                 and stores its 8 bytes next to its neighbour's.
//                 ENDS: nothing at or behind a stream's cut is loaded or written (the interpolator is causal), and the first tile's first lane
//                 leaves the cut REBASED to the piece's first point in os_cut[s] — which is what lets the ENDS instantiations of the two older
//                 kernels run with f0 = 0 on the scratch, unchanged: they only ever compare the cut with f0 and f0 + n.
// (OS_HALO, the 23 frames, and OS_HROW, the floats of a history row: mtr_internal.h — k_history's instantiations are made of them)
constexpr int OS_TAPS = MTR_GONIO_OS_TAPS, OS_TILE = 128, OS_TPITCH = OS_TAPS + 1;

typedef struct mtr_gonio_os_args {
	const float*    audio;       /* [S][stride][2] */
	uint64_t        stride;
	uint64_t        f0;          /* the piece's first frame in the call */
	uint32_t        n;           /* ... and its input frames */
	uint32_t        n_streams;
	uint32_t        f;           /* the factor, 2 .. 32 */
	uint32_t        tiles;       /* tiles of OS_TILE frames per stream: the grid is n_streams * tiles */
	const float*    hist;        /* [S][OS_HROW] the 23 frames in front of the call */
	const float*    tab;         /* [f + 1][12] */
	float*          pts;         /* [S][pitch][2] */
	uint64_t        pitch;       /* points per stream of the scratch */
	const uint32_t* cut;         /* ENDS: [S] the call POINT at which the stream's drawing ends (mtr_gonio_ends_args::cut) */
	uint32_t*       piece_cut;   /* ENDS: [S] out: the same, counted from the piece's first point */
} mtr_gonio_os_args;

template <bool ENDS>
__global__ __launch_bounds__ (256) void k_gonio_os (const mtr_gonio_os_args a)
{
	__shared__ float tab[(MTR_GONIO_OS_MAX + 1) * OS_TPITCH];
	__shared__ float2 x[OS_TILE + OS_HALO];
	const int tid = threadIdx.x;
	const uint32_t s = blockIdx.x / a.tiles, tile = blockIdx.x - s * a.tiles;
	const int f = (int) a.f;
	const int t0 = (int) tile * OS_TILE;                                 // the tile's first frame in the piece
	int lim = (int) a.n;                                                 // the frames of the piece the stream takes
	if constexpr (ENDS) {
		const uint32_t cut = a.cut[s];
		const uint64_t p0 = a.f0 * (uint64_t) f;
		if (tile == 0 && tid == 0) a.piece_cut[s] = cut == MTR_GONIO_OPEN ? cut : (uint64_t) cut <= p0 ? 0u : (uint32_t) ((uint64_t) cut - p0);
		lim = gonio_limit (cut == MTR_GONIO_OPEN ? cut : cut / (uint32_t) f, a.f0, lim);   // (a cut is a whole number of frames)
	}
	const int nf = min (OS_TILE, lim - t0);
	if (nf <= 0) return;
	for (int i = tid; i < (f + 1) * OS_TAPS; i += 256) tab[(i / OS_TAPS) * OS_TPITCH + i % OS_TAPS] = a.tab[i];
	for (int k = tid; k < nf + OS_HALO; k += 256) {                      // x [k]: piece frame t0 - 23 + k, < t0 + nf <= lim
		const int64_t g = (int64_t) a.f0 + t0 - OS_HALO + k;                 // ... and call frame g
		const float* const p = g >= 0 ? a.audio + ((uint64_t) s * a.stride + (uint64_t) g) * 2 : a.hist + (size_t) s * OS_HROW + (size_t) (OS_HALO + g) * 2;
		x[k] = float2{p[0], p[1]};
	}
	__syncthreads ();
	float2* const out = reinterpret_cast<float2*> (a.pts) + (size_t) s * a.pitch + (size_t) t0 * f;
	for (int p = tid; p < nf * f; p += 256) {
		const int m = p / f, ph = p - m * f;
		const float* const c1 = &tab[ph * OS_TPITCH];
		const float* const c2 = &tab[(f - ph) * OS_TPITCH];
		float s0 = 1e-20f, s1 = 1e-20f;                                  // resampler.cc:221-228, both channels
#pragma unroll
		for (int i = 0; i < OS_TAPS; ++i) {
			const float2 q1 = x[m + i], q2 = x[m + OS_HALO - i];             // frames m - 23 + i and m - i
			s0 += q1.x * c1[i] + q2.x * c2[i];
			s1 += q1.y * c1[i] + q2.y * c2[i];
		}
		out[p] = float2{s0 - 1e-20f, s1 - 1e-20f};
	}
}

}  // namespace

// a piece's two kernels.  A = mtr_gonio_ends_args: a call with per-stream ends, the ENDS instantiations on the same grids
template <typename A>
static int mtr_launch_gonio (const A& a, bool autogain, hipStream_t st, hipEvent_t* ev)
{
	constexpr bool ENDS = std::is_same_v<A, mtr_gonio_ends_args>;
	const auto points = [&] (auto NS) {
		const dim3 grid ((a.n_streams + NS.value - 1) / NS.value);
		if (autogain) hipLaunchKernelGGL ((k_gonio_points<NS.value, true, ENDS>), grid, dim3 (64), 0, st, a);
		else hipLaunchKernelGGL ((k_gonio_points<NS.value, false, ENDS>), grid, dim3 (64), 0, st, a);
	};
	if (ev && hipEventRecord (ev[0], st) != hipSuccess) return -1;
	if (a.n_streams >= 16384) points (std::integral_constant<int, 64> {}); else points (std::integral_constant<int, 16> {});
	if (ev && hipEventRecord (ev[1], st) != hipSuccess) return -1;
	const dim3 grid (a.n_streams);
	if (a.shift == 1) hipLaunchKernelGGL ((k_gonio_image<cells_of (1), 1024, ENDS>), grid, dim3 (1024), 0, st, a);
	else if (a.shift == 2) hipLaunchKernelGGL ((k_gonio_image<cells_of (2), 256, ENDS>), grid, dim3 (256), 0, st, a);
	else hipLaunchKernelGGL ((k_gonio_image<cells_of (3), 256, ENDS>), grid, dim3 (256), 0, st, a);
	if (ev && hipEventRecord (ev[2], st) != hipSuccess) return -1;
	return hipGetLastError () == hipSuccess ? 0 : -1;
}

// the interpolator of a piece (factor above 1), in front of the two launchers above: `ends` selects the ENDS instantiation
static int mtr_launch_gonio_os (mtr_gonio_os_args& a, bool ends, hipStream_t st, hipEvent_t* ev)
{
	a.tiles = (a.n + OS_TILE - 1) / OS_TILE;
	const dim3 grid (a.n_streams * a.tiles);
	if (ev && hipEventRecord (ev[0], st) != hipSuccess) return -1;
	if (ends) hipLaunchKernelGGL (k_gonio_os<true>, grid, dim3 (256), 0, st, a);
	else hipLaunchKernelGGL (k_gonio_os<false>, grid, dim3 (256), 0, st, a);
	if (ev && hipEventRecord (ev[1], st) != hipSuccess) return -1;
	return hipGetLastError () == hipSuccess ? 0 : -1;
}

// ---- GONIO in the engine: set-up, the call's step, the blob's section and the cursor in it, the C entry points ---------------------------

// `attack` of :524 for a display update of `frames` frames (elapsed of :499), from the dials of a resolved configuration (:897-904):
// [0] where the target is below the gain, [1] otherwise.  The block's (P frames) and a closing update's (r frames) alike
static void gonio_attack (const mtr_gonio_config& c, double rate, uint64_t frames, float out[2])
{
	float g_attack = c.g_attack, g_decay = c.g_decay;
	g_attack = 0.1 * exp (0.06 * g_attack) - .09;
	g_decay = 0.1 * exp (0.06 * g_decay) - .09;
	if (g_attack < .01) g_attack = .01;
	if (g_decay < .01) g_decay = .01;
	const float elapsed = (size_t) frames / rate;                                    // :499
	out[0] = g_attack * (.31 + .1 * log10f (elapsed));                               // :524
	out[1] = g_decay * (.03 + .007 * logf (elapsed));
}

static int gonio_resolve (const mtr_gonio_config* in, double rate, mtr_gonio_config* c, mtr_gonio_derived* d)
{
	if (!in || in->struct_size != sizeof (mtr_gonio_config) || !(rate >= 8000.0)) return fail (MTR_ERR_ARG, "mtr_gonio_config: NULL, struct_size, or rate < 8000");
	*c = *in;
	if (c->period_frames && (c->period_frames < 64 || c->period_frames > (1u << 20)))
		return fail (MTR_ERR_ARG, "mtr_gonio_config: period_frames is 0 or 64 (draw_rb's n_samples < 64 return) .. 2^20");
	if (!c->capacity) {
		if (c->period_frames) return fail (MTR_ERR_ARG, "mtr_gonio_config: a period needs a capacity");
		c->capacity = 4096;
	}
	if (!c->period_frames) c->period_frames = (uint32_t) rint (rate / 25.0);        // src/goniometerlv2.c:25,81
	if (c->period_frames < 64 || c->period_frames > (1u << 20)) return fail (MTR_ERR_ARG, "mtr_gonio_config: rint (rate / 25) is outside 64 .. 2^20");
	if (!c->shift) c->shift = 2;
	if (c->shift > 3) return fail (MTR_ERR_ARG, "mtr_gonio_config: shift is 1, 2 or 3");
	if (c->autogain > 2) return fail (MTR_ERR_ARG, "mtr_gonio_config: autogain is 0, 1 or 2");
	if (c->gain == 0.f) c->gain = 1.0f;                                              // :1091
	if (c->point_width == 0.f) c->point_width = 1.75f;                               // src/goniometerlv2.c:97
	if (!std::isfinite (c->gain) || !(c->gain > 0.f) || !std::isfinite (c->point_width) || !(c->point_width > 0.f))
		return fail (MTR_ERR_ARG, "mtr_gonio_config: gain and point_width are finite and > 0");
	if ((double) (float) (c->point_width * .5) != c->point_width * .5) return fail (MTR_ERR_ARG, "mtr_gonio_config: point_width * .5 is not an f32 (a subnormal width)");
	const float* const dial = &c->g_attack;
	if (c->autogain != 2) {
		for (int i = 0; i < 4; ++i) if (dial[i] != 0.f) return fail (MTR_ERR_ARG, "mtr_gonio_config: the four dials are given with autogain 2 only");
		c->g_attack = 54.f; c->g_decay = 58.f; c->g_target = 40.f; c->g_rms = 50.f;   // src/goniometerlv2.c:101-104
	} else
		for (int i = 0; i < 4; ++i) if (!(dial[i] >= 0.f && dial[i] <= 100.f)) return fail (MTR_ERR_ARG, "mtr_gonio_config: a dial is 0 .. 100");
	if (!c->tune_piece) c->tune_piece = 4096;
	if (c->tune_piece < 64 || c->tune_piece > (1u << 20)) return fail (MTR_ERR_ARG, "mtr_gonio_config: tune_piece is 0 or 64 .. 2^20");

	d->period_frames = c->period_frames;
	d->G = cells_of (c->shift);
	d->hpw = expf (-2.0 * M_PI * 20 / rate);                                         // :165
	const float g_rms = .01 * c->g_rms;                                              // :906-912
	float g_target = c->g_target;
	g_target = exp (1.8 * (-.02 * g_target + 1.0));
	if (g_target < .15) g_target = .15;
	gonio_attack (*c, rate, c->period_frames, d->attack);
	d->g_target = g_target; d->g_rms = g_rms;
	return MTR_OK;
}

static int no_gonio (const mtr_engine* e) { return !e || !(e->cfg.meters & MTR_METER_GONIO); }
constexpr const char* NO_GONIO = "no GONIO in this engine";

static int gonio_apply (mtr_engine* e, const mtr_gonio_config& c, const mtr_gonio_derived& d)
{
	const uint32_t S = e->cfg.n_streams;
	const size_t pitch = (sizeof (mtr_gonio_state) + (size_t) d.G * d.G * sizeof (uint32_t) + 15) & ~(size_t) 15;
	const uint32_t code_pitch = (c.tune_piece + 127u) & ~127u;
	if (e->go.state.reserve ((size_t) S * pitch) || e->go.codes.reserve ((size_t) S * code_pitch)) return fail (MTR_ERR_NOMEM, "hipMalloc GONIO state");
	int rc = series_ring (e->go.series, (size_t) 3 * S * c.capacity, "hipMalloc GONIO series");
	if (rc) return rc;
	e->go.cfg = c; e->go.der = d;
	e->go.ser = { c.period_frames, c.capacity };
	e->go.pitch = pitch; e->go.code_pitch = code_pitch;
	return MTR_OK;
}

// ---- oversampling: the table, hpw, the engine's buffers ----
// Resampler_table for fr = 1.0, hl = 12, np = F in double, as zita-resampler/resampler-table.cc:52-75 builds it (t grows by additions of 1)
static double os_sinc (double x) { x = fabs (x); if (x < 1e-6) return 1.0; x *= M_PI; return sin (x) / x; }
static double os_wind (double x) { x = fabs (x); if (x >= 1.0) return 0.0; x *= M_PI; return 0.384 + 0.500 * cos (x) + 0.116 * cos (2 * x); }
static void gonio_os_table (uint32_t F, float* out)
{
	const double fr = 1.0;
	for (uint32_t j = 0; j <= F; ++j) {
		double t = (double) j / (double) F;
		for (uint32_t i = 0; i < (uint32_t) OS_TAPS; ++i, t += 1) out[j * OS_TAPS + OS_TAPS - 1 - i] = (float) (fr * os_sinc (t * fr) * os_wind (t / OS_TAPS));
	}
}

static float gonio_os_hpw (double rate, uint32_t F) { return expf ((float) (-2.0 * M_PI * 20 / (rate * (double) (float) F))); }   // :175 (F = 1: :165)

constexpr const char* GONIO_OS_PERIOD = "GONIO oversampled: a display update is at most floor (rate) frames (the reference's scratch, gui/goniometer.c:173-181)";

// the engine's buffers for factor F and the configuration it holds (F = 1: none are kept)
static int gonio_os_apply (mtr_engine* e, uint32_t F)
{
	const size_t S = e->cfg.n_streams;
	e->go.os = F;
	e->go.os_hpw = gonio_os_hpw ((double) e->cfg.sample_rate, F);
	if (F <= 1) {
		e->go.os_pts.drop (); e->go.os_tab.drop (); e->go.os_cut.drop ();
		for (auto& h : e->go.os_hist) h.drop ();
		return MTR_OK;
	}
	e->go.os_pitch = (e->go.cfg.tune_piece + 1u) & ~1u;
	if (e->go.os_pts.reserve (S * e->go.os_pitch * 2) || e->go.os_tab.reserve ((size_t) (MTR_GONIO_OS_MAX + 1) * OS_TAPS) || e->go.os_cut.reserve (S)
	    || e->go.os_hist[0].reserve (S * OS_HROW) || e->go.os_hist[1].reserve (S * OS_HROW))
		return fail (MTR_ERR_NOMEM, "hipMalloc GONIO oversampling");
	float tab[(MTR_GONIO_OS_MAX + 1) * OS_TAPS];
	gonio_os_table (F, tab);
	HIPCHK (hipMemcpy (e->go.os_tab.p, tab, (size_t) (F + 1) * OS_TAPS * sizeof (float), hipMemcpyHostToDevice));
	return MTR_OK;
}

static int gonio_create (mtr_engine* e)
{
	mtr_gonio_config z, c;
	mtr_gonio_derived d;
	memset (&z, 0, sizeof (z));
	z.struct_size = sizeof (z);
	const int rc = gonio_resolve (&z, (double) e->cfg.sample_rate, &c, &d);
	return rc ? rc : gonio_apply (e, c, d);                            // (mtr_engine_create resets)
}

// the streams' mtr_gonio_state, [count] on the host <-> every pitch-th bytes on the device
static hipError_t gonio_states (mtr_engine* e, uint32_t first, uint32_t count, mtr_gonio_state* h, bool up)
{
	if (!count) return hipSuccess;
	unsigned char* const dev = e->go.state.p + (size_t) first * e->go.pitch;
	return up ? hipMemcpy2D (dev, e->go.pitch, h, sizeof (*h), sizeof (*h), count, hipMemcpyHostToDevice)
	          : hipMemcpy2D (h, sizeof (*h), dev, e->go.pitch, sizeof (*h), count, hipMemcpyDeviceToHost);
}

// Track lengths (mtr_gonio_ends.h).  draw_rb returns at n_samples < 64 (:302): a closing stream gets one last update of the r frames it has
// of its open block if r >= 64, and stands where its last whole block left it otherwise — but never in front of the call's first frame:
// what earlier calls drew of the open block stays drawn.
// What a stream that takes `frames` of a call of n_frames draws, the call starting `fill` frames into a display update of P (mtr_gonio_cut
// is this): `whole` updates of P frames it completes, a closing one of `closing` frames (0: none; else >= 64) with its attack pair, and
// `drawn`: the call frame at which its drawing ends.  `c`: a resolved configuration (its dials are read)
struct GonioCut { uint64_t whole = 0, drawn = 0; uint32_t closing = 0; float attack[2] = { 0.f, 0.f }; };
static GonioCut gonio_cut (uint64_t fill, uint32_t P, double rate, uint64_t n_frames, uint64_t frames, const mtr_gonio_config& c)
{
	GonioCut o;
	const uint64_t tot = fill + frames, r = tot % P;
	o.whole = tot / P;
	o.drawn = frames;
	if (!(frames > 0 && frames < n_frames) || r == 0) return o;
	if (r < 64) { o.drawn = frames - std::min (frames, r); return o; }
	o.closing = (uint32_t) r;
	gonio_attack (c, rate, r, o.attack);
	return o;
}

// the cut of a stream that takes `frames` of call `c`, taken from where the CALL started (e->pos): every chunk of a host call sees the same ones
static GonioCut gonio_cut (const mtr_engine* e, const Call& c, uint64_t frames)
{
	return gonio_cut (e->pos.go.fill, e->go.cfg.period_frames, (double) e->cfg.sample_rate, c.n_frames, frames, e->go.cfg);
}

// stream g's own display updates (SideMeter::count — with draw_rb's 64-frame floor, not every partial block: no `series` hook): those of
// its `frames` frames of the call, the closing one included; an imported stream takes the lock-step number
static void gonio_count (mtr_engine* e, size_t g, const Call* c, uint64_t frames)
{
	if (!c) { e->go.updates[g] = e->pos.go.points; return; }
	const GonioCut k = gonio_cut (e, *c, frames);
	e->go.updates[g] += k.whole + (k.closing ? 1 : 0);
}

// The meter's words of a ragged call (SideMeter::ends_fill): [cut S | closing S | attack S x 2], per stream of the view the call frame at
// which its drawing ends (MTR_GONIO_OPEN: not in this call), the frames of its closing display update or 0, that update's attack pair —
// cut and closing in POINTS, F per frame, where the engine oversamples.  The note: the last call frame (an input frame) any stream of the view draws
static uint64_t gonio_ends_fill (const mtr_engine* e, const Call& c, uint32_t* own)
{
	const size_t S = c.cnt;
	const uint32_t F = e->go.os;
	uint64_t last = 0;
	for (uint32_t i = 0; i < S; ++i) {
		const uint64_t f = call_frames (e, c, i);
		const GonioCut k = gonio_cut (e, c, f);
		// (oversampled: the kernels walk POINTS, F per frame — check_limits keeps n_frames F below 2^32 - 1; the cut itself counts input frames)
		own[i] = f == c.n_frames ? 0xFFFFFFFFu : (uint32_t) (k.drawn * F);   // (MTR_GONIO_OPEN: the stream does not end in this call)
		own[S + i] = k.closing * F;
		memcpy (own + 2 * S + 2 * (size_t) i, k.attack, sizeof (k.attack));
		last = std::max (last, k.drawn);
	}
	return last;
}

static int gonio_step (mtr_engine* e, const Call& c, Cursors& nx, const StreamEnds& se)
{
	const mtr_gonio_config& g = e->go.cfg;
	const mtr_gonio_derived& d = e->go.der;
	const uint32_t P = g.period_frames, cap = g.capacity;
	const uint32_t F = e->go.os;                                       // oversampling: F points per input frame (1: none — today's launches, argument for argument)
	const uint32_t piece = g.tune_piece / F;                           // input frames per piece: never more than tune_piece points (>= 2: tune_piece >= 64, F <= 32)
	const size_t S = e->cfg.n_streams;
	mtr_gonio_ends_args a;                                             // (a dense call launches on its base)
	memset (static_cast<void*> (&a), 0, sizeof (a));
	if (se.own) { a.cut = se.own; a.closing = se.own + c.cnt; a.c_attack = reinterpret_cast<const float*> (se.own + 2 * (size_t) c.cnt); }   // (gonio_ends_fill)
	a.audio = c.audio; a.stride = c.stride; a.n_streams = c.cnt;
	a.P = P * F; a.capacity = cap; a.shift = g.shift; a.G = d.G; a.code_pitch = e->go.code_pitch;
	a.hpw = F > 1 ? e->go.os_hpw : d.hpw; a.attack[0] = d.attack[0]; a.attack[1] = d.attack[1]; a.g_target = d.g_target; a.g_rms = d.g_rms;
	a.hw = (float) (g.point_width * .5);
	a.pitch = e->go.pitch;
	a.state = e->go.state.p + (size_t) c.off * a.pitch;
	a.s_gain = e->go.series.p + (size_t) c.off * cap;
	a.s_drawn = reinterpret_cast<uint32_t*> (e->go.series.p + S * cap) + (size_t) c.off * cap;
	a.s_clipped = reinterpret_cast<uint32_t*> (e->go.series.p + 2 * S * cap) + (size_t) c.off * cap;
	a.codes = e->go.codes.p;                                           // (a scratch: every view of a host call takes it from the start)
	mtr_gonio_os_args o;
	memset (&o, 0, sizeof (o));
	if (F > 1) {
		// k_gonio_os reads the call, the two older kernels read its points: the scratch [cnt][os_pitch][2] as their `audio`, every piece at f0 = 0,
		// and — a ragged call — the cuts as k_gonio_os rebases them to the piece (both scratches are taken from the start, like the codes)
		o.audio = c.audio; o.stride = c.stride; o.n_streams = c.cnt; o.f = F;
		o.hist = e->go.os_hist[e->pos.go_hist_cur].p + (size_t) c.off * OS_HROW;
		o.tab = e->go.os_tab.p; o.pts = e->go.os_pts.p; o.pitch = e->go.os_pitch;
		o.cut = a.cut; o.piece_cut = e->go.os_cut.p;
		a.audio = e->go.os_pts.p; a.stride = e->go.os_pitch;
		if (se.own) a.cut = e->go.os_cut.p;
	}
	// the periods are cut from where the CALL started (e->pos): every chunk of a host call sees the same cuts
	SeriesPos pos = e->pos.go;
	for (uint64_t f0 = 0; f0 < c.n_frames; f0 += piece) {
		const uint32_t nf = (uint32_t) std::min<uint64_t> (piece, c.n_frames - f0);   // the piece's input frames
		a.f0 = F > 1 ? 0 : f0;
		a.n = nf * F;
		a.fill = (uint32_t) pos.fill * F; a.point0 = pos.points;
		// (per-stream ends: only the pieces in which some stream of the view still draws are launched; the cursor moves on regardless)
		if (se.ends && f0 >= se.note) { pos = series_advance (pos, P, nf); continue; }
		hipEvent_t ev[3], oev[2];
		const bool tm = e->go.timed && c.commit;
		if (tm) {
			for (int i = 0; i < 3; ++i) {
				e->go.ev.emplace_back ();
				HIPCHK (e->go.ev.back ().ensure (hipEventDefault));
				ev[i] = e->go.ev.back ().v;
			}
			for (int i = 0; F > 1 && i < 2; ++i) {
				e->go.os_ev.emplace_back ();
				HIPCHK (e->go.os_ev.back ().ensure (hipEventDefault));
				oev[i] = e->go.os_ev.back ().v;
			}
		}
		if (F > 1) {
			o.f0 = f0; o.n = nf;
			if (mtr_launch_gonio_os (o, se.ends != nullptr, c.st, tm ? oev : nullptr)) return fail (MTR_ERR_HIP, "k_gonio_os launch");
		}
		if (se.ends ? mtr_launch_gonio (a, g.autogain != 0, c.st, tm ? ev : nullptr) : mtr_launch_gonio<mtr_gonio_args> (a, g.autogain != 0, c.st, tm ? ev : nullptr))
			return fail (MTR_ERR_HIP, "k_gonio launch");
		pos = series_advance (pos, P, nf);
	}
	nx.go = pos;
	return MTR_OK;
}

static void gonio_sections (const mtr_engine* e, std::vector<StateSection>& v)
{
	v.push_back ({ e->go.state.p, e->go.pitch });
}

constexpr const char* GONIO_CORRUPT = "mtr_engine_state_import: corrupt blob (configuration of the goniometer)";

static void gonio_hdr_write (const mtr_engine* e, void* out)
{
	*static_cast<mtr_gonio_hdr*> (out) = { e->go.cfg.period_frames, e->go.cfg.shift, e->go.cfg.autogain != 0, (uint32_t) e->pos.go.fill };
}

static int gonio_hdr_check (const mtr_engine* e, const void* in, bool fresh)
{
	const mtr_gonio_hdr& h = *static_cast<const mtr_gonio_hdr*> (in);
	if (!series_blob_ok (h.period, h.fill, 64, 1u << 20) || !h.period || h.shift < 1 || h.shift > 3 || h.autogain > 1) return fail (MTR_ERR_STATE, GONIO_CORRUPT);
	if (h.period != e->go.cfg.period_frames || h.shift != e->go.cfg.shift || h.autogain != (e->go.cfg.autogain != 0))
		return fail (MTR_ERR_STATE, "mtr_engine_state_import: the blob's goniometer is configured otherwise (period, shift or auto gain)");
	if (!fresh && h.fill != e->pos.go.fill)
		return fail (MTR_ERR_STATE, "mtr_engine_state_import: the engine does not stand where the blob's streams do (display update of the goniometer)");
	return MTR_OK;
}

static void gonio_hdr_take (mtr_engine* e, const void* in) { e->pos.go.fill = static_cast<const mtr_gonio_hdr*> (in)->fill; }

static constinit BlobHeader gonio_hdr = { .offset = 0, .bytes = sizeof (mtr_gonio_hdr), .corrupt = GONIO_CORRUPT, .write = gonio_hdr_write, .check = gonio_hdr_check, .take = gonio_hdr_take };

// ---- oversampling: the second row of the meter (SIDE_METERS): its step is the call's last kernel of the meter, its section the history ----
static int gonio_os_step (mtr_engine* e, const Call& c, Cursors& nx, const StreamEnds& se)
{
	if (e->go.os <= 1) return MTR_OK;
	mtr_history_args h = {};                                           // (no fold pointers: the row and nothing else)
	h.audio = c.audio; h.stride = c.stride; h.n_frames = c.n_frames; h.n_streams = c.cnt; h.ends = se.ends;
	h.C = h.FC = h.HC = 2;
	h.hist_in = e->go.os_hist[e->pos.go_hist_cur].p + (size_t) c.off * OS_HROW;
	h.hist_out = e->go.os_hist[e->pos.go_hist_cur ^ 1].p + (size_t) c.off * OS_HROW;
	// (a stream that ends inside the call leaves the frames in front of its OWN end — an open one's end is the call's length, end 0, closed
	// or untouched, keeps the old row — so that its part of the state blob does not depend on what lies behind it)
	if (mtr_launch_history (se.ends ? HIST_OWN_END : HIST_CALL_END, HIST_ROW_GONIO, h, c.st)) return fail (MTR_ERR_HIP, "k_history launch (GONIO)");
	nx.go_hist_cur = e->pos.go_hist_cur ^ 1;
	return MTR_OK;
}

// With a factor above 1 the blob carries one more section, behind every older one: a stream's history row, and in the two words behind its
// 23 frames the factor.  An engine takes a blob of its own factor only.  (At factor 1 there is no section and the blob is what it was.)
typedef struct mtr_gonio_os_hdr { uint32_t factor, zero; } mtr_gonio_os_hdr;
static_assert (OS_HALO * 2 * sizeof (float) + sizeof (mtr_gonio_os_hdr) == OS_HROW * sizeof (float), "mtr_gonio_os_hdr");

static void gonio_os_sections (const mtr_engine* e, std::vector<StateSection>& v)
{
	if (e->go.os > 1) v.push_back ({ e->go.os_hist[e->pos.go_hist_cur].p, OS_HROW * sizeof (float) });
}

constexpr const char* GONIO_OS_CORRUPT = "mtr_engine_state_import: corrupt blob (oversampling of the goniometer)";

static void gonio_os_hdr_write (const mtr_engine* e, void* out) { *static_cast<mtr_gonio_os_hdr*> (out) = { e->go.os, 0 }; }

static int gonio_os_hdr_check (const mtr_engine* e, const void* in, bool)
{
	const mtr_gonio_os_hdr& h = *static_cast<const mtr_gonio_os_hdr*> (in);
	if (h.factor < 2 || h.factor > MTR_GONIO_OS_MAX || h.zero) return fail (MTR_ERR_STATE, GONIO_OS_CORRUPT);
	if (h.factor != e->go.os) return fail (MTR_ERR_STATE, "mtr_engine_state_import: the blob's goniometer oversamples by another factor");
	return MTR_OK;
}

static void gonio_os_hdr_take (mtr_engine*, const void*) {}

static constinit BlobHeader gonio_os_hdr = { .offset = OS_HALO * 2 * sizeof (float), .bytes = sizeof (mtr_gonio_os_hdr), .corrupt = GONIO_OS_CORRUPT,
                                             .write = gonio_os_hdr_write, .check = gonio_os_hdr_check, .take = gonio_os_hdr_take };
// (no create and no reset: the meter's first row does both)
constinit SideMeter gonio_os_meter = { .bits = MTR_METER_GONIO, .step = gonio_os_step, .sections = gonio_os_sections, .hdr = &gonio_os_hdr };

constinit SideMeter gonio_meter = { .bits = MTR_METER_GONIO, .create = gonio_create, .reset = mtr_engine_gonio_reset, .step = gonio_step, .sections = gonio_sections,
                                    .hdr = &gonio_hdr, .count = gonio_count, .ends_words = 4, .ends_fill = gonio_ends_fill };

extern "C" {

int mtr_gonio_derive (const mtr_gonio_config* cfg, double rate, mtr_gonio_derived* out)
{
	if (!out) return fail (MTR_ERR_ARG, "mtr_gonio_derive: null argument");
	mtr_gonio_config c;
	return gonio_resolve (cfg, rate, &c, out);
}

int mtr_engine_gonio_reset (mtr_engine* e)
{
	if (no_gonio (e)) return fail (MTR_ERR_ARG, NO_GONIO);
	e->snap_valid = false;
	HIPCHK (hipSetDevice (e->cfg.device));
	const uint32_t S = e->cfg.n_streams;
	mtr_gonio_state v;
	memset (&v, 0, sizeof (v));
	v.last_x = v.last_y = 186.5f;                                      // :1086-1091
	v.gain = e->go.cfg.gain;
	std::vector<mtr_gonio_state> h (S, v);
	HIPCHK (hipStreamSynchronize (e->last_stream));
	HIPCHK (hipMemset (e->go.state.p, 0, (size_t) S * e->go.pitch));
	HIPCHK (gonio_states (e, 0, S, h.data (), true));
	if (e->go.series.n) HIPCHK (hipMemset (e->go.series.p, 0, e->go.series.n * sizeof (float)));
	if (e->go.os > 1)                                                  // (the input history: zeros in front of the stream, as setup_src primes the resampler)
		for (auto& h : e->go.os_hist) HIPCHK (hipMemset (h.p, 0, (size_t) S * OS_HROW * sizeof (float)));
	e->pos.go = {};
	e->pos.go_hist_cur = 0;
	e->go.updates.assign (S, 0);
	e->go.ev.clear ();
	e->go.os_ev.clear ();
	return MTR_OK;
}

int mtr_engine_gonio_configure (mtr_engine* e, const mtr_gonio_config* cfg)
{
	if (no_gonio (e)) return fail (MTR_ERR_ARG, NO_GONIO);
	mtr_gonio_config c;
	mtr_gonio_derived d;
	int rc = gonio_resolve (cfg, (double) e->cfg.sample_rate, &c, &d);
	if (rc) return rc;
	if (e->go.os > 1 && (double) c.period_frames > floor ((double) e->cfg.sample_rate)) return fail (MTR_ERR_ARG, GONIO_OS_PERIOD);
	if (e->advanced) return fail (MTR_ERR_STATE, "mtr_engine_gonio_configure: only on an engine that has processed nothing since create / reset");
	if ((rc = wait_stream (e)) || (rc = gonio_apply (e, c, d)) || (rc = gonio_os_apply (e, e->go.os))) return rc;   // (the factor stays)
	return mtr_engine_gonio_reset (e);
}

int mtr_engine_gonio_config (mtr_engine* e, mtr_gonio_config* cfg, mtr_gonio_derived* derived)
{
	if (no_gonio (e)) return fail (MTR_ERR_ARG, NO_GONIO);
	if (cfg) *cfg = e->go.cfg;
	if (derived) *derived = e->go.der;
	return MTR_OK;
}

int mtr_engine_gonio_set_gain (mtr_engine* e, float gain)
{
	if (no_gonio (e)) return fail (MTR_ERR_ARG, NO_GONIO);
	if (!std::isfinite (gain) || !(gain > 0.f)) return fail (MTR_ERR_ARG, "mtr_engine_gonio_set_gain: a finite gain > 0");
	int rc = wait_stream (e);
	if (rc) return rc;
	e->snap_valid = false;
	const uint32_t S = e->cfg.n_streams;
	std::vector<mtr_gonio_state> h (S);
	HIPCHK (gonio_states (e, 0, S, h.data (), false));
	for (auto& v : h) v.gain = gain;                                   // :866
	HIPCHK (gonio_states (e, 0, S, h.data (), true));
	return MTR_OK;
}

int mtr_engine_gonio_image (mtr_engine* e, uint32_t first, uint32_t count, uint32_t* img, uint64_t* drawn, uint64_t* clipped, uint64_t* skipped)
{
	int rc = meter_range (e, !no_gonio (e), NO_GONIO, first, count);
	if (rc || (rc = wait_stream (e))) return rc;
	if (!count) return MTR_OK;
	const size_t row = (size_t) e->go.der.G * e->go.der.G * sizeof (uint32_t);
	if (img) HIPCHK (hipMemcpy2D (img, row, e->go.state.p + (size_t) first * e->go.pitch + sizeof (mtr_gonio_state), e->go.pitch, row, count, hipMemcpyDeviceToHost));
	if (drawn || clipped || skipped) {
		std::vector<mtr_gonio_state> h (count);
		HIPCHK (gonio_states (e, first, count, h.data (), false));
		for (uint32_t i = 0; i < count; ++i) {
			if (drawn) drawn[i] = h[i].drawn;
			if (clipped) clipped[i] = h[i].clipped;
			if (skipped) skipped[i] = h[i].skipped;
		}
	}
	return MTR_OK;
}

int mtr_engine_gonio_read (mtr_engine* e, uint32_t first, uint32_t count, float* gain, float* lp, float* last)
{
	int rc = meter_range (e, !no_gonio (e), NO_GONIO, first, count);
	if (rc || (rc = wait_stream (e))) return rc;
	std::vector<mtr_gonio_state> h (count);
	HIPCHK (gonio_states (e, first, count, h.data (), false));
	for (uint32_t i = 0; i < count; ++i) {
		if (gain) gain[i] = h[i].gain;
		if (lp) { lp[2 * (size_t) i] = h[i].lp0; lp[2 * (size_t) i + 1] = h[i].lp1; }
		if (last) { last[2 * (size_t) i] = h[i].last_x; last[2 * (size_t) i + 1] = h[i].last_y; }
	}
	return MTR_OK;
}

int mtr_engine_gonio_blocks (mtr_engine* e, uint64_t* blocks, uint64_t* held)
{
	if (no_gonio (e)) return fail (MTR_ERR_ARG, NO_GONIO);
	if (blocks) *blocks = e->pos.go.points;
	if (held) *held = std::min<uint64_t> (e->pos.go.points, e->go.cfg.capacity);
	return MTR_OK;
}

int mtr_engine_gonio_series (mtr_engine* e, uint32_t first, uint32_t count, uint64_t from, uint32_t n, float* gain, uint32_t* drawn, uint32_t* clipped)
{
	int rc = meter_range (e, !no_gonio (e), NO_GONIO, first, count);
	if (rc) return rc;
	const uint32_t cap = e->go.cfg.capacity;
	const uint64_t held = std::min<uint64_t> (e->pos.go.points, cap);
	if (from > held || n > held - from) return fail (MTR_ERR_ARG, "mtr_engine_gonio_series: from + n is beyond the points the series holds");
	if (!count || !n || (!gain && !drawn && !clipped)) return MTR_OK;
	if ((rc = wait_stream (e))) return rc;
	const size_t S = e->cfg.n_streams;
	void* const out[3] = { gain, drawn, clipped };
	for (int k = 0; k < 3; ++k)
		if (out[k]) HIPCHK (hipMemcpy2D (out[k], (size_t) n * 4, e->go.series.p + (size_t) k * S * cap + (size_t) first * cap + from, (size_t) cap * 4, (size_t) n * 4, count, hipMemcpyDeviceToHost));
	return MTR_OK;
}

int mtr_gonio_cut (uint64_t fill, uint32_t period, double rate, uint64_t n_frames, uint64_t frames, const mtr_gonio_config* cfg,
                   uint64_t* whole, uint32_t* closing_frames, uint64_t* drawn_frames, float attack[2])
{
	if (!cfg || !whole || !closing_frames || !drawn_frames || !attack) return fail (MTR_ERR_ARG, "mtr_gonio_cut: null argument");
	if (!period || fill >= period || frames > n_frames) return fail (MTR_ERR_ARG, "mtr_gonio_cut: fill < period, frames <= n_frames");
	mtr_gonio_config in = *cfg, c;
	mtr_gonio_derived d;
	in.period_frames = period;                                         // (the period is the argument's, whatever the configuration names)
	if (!in.capacity) in.capacity = 1;
	const int rc = gonio_resolve (&in, rate, &c, &d);
	if (rc) return rc;
	const GonioCut k = gonio_cut (fill, period, rate, n_frames, frames, c);
	*whole = k.whole; *closing_frames = k.closing; *drawn_frames = k.drawn;
	attack[0] = k.attack[0]; attack[1] = k.attack[1];
	return MTR_OK;
}

int mtr_engine_gonio_points (mtr_engine* e, uint32_t first, uint32_t count, uint64_t* updates, uint64_t* points)
{
	const int rc = meter_range (e, !no_gonio (e), NO_GONIO, first, count);
	if (rc) return rc;
	for (uint32_t i = 0; i < count; ++i) {
		if (updates) updates[i] = e->go.updates[first + i];
		if (points) points[i] = e->go.updates[first + i];               // (every update appends a point, written or dropped)
	}
	return MTR_OK;
}

int mtr_engine_gonio_image_clear (mtr_engine* e)
{
	if (no_gonio (e)) return fail (MTR_ERR_ARG, NO_GONIO);
	int rc = wait_stream (e);
	if (rc) return rc;
	e->snap_valid = false;
	const uint32_t S = e->cfg.n_streams;
	std::vector<mtr_gonio_state> h (S);
	HIPCHK (gonio_states (e, 0, S, h.data (), false));
	for (auto& v : h) v.drawn = v.clipped = v.skipped = 0;
	HIPCHK (gonio_states (e, 0, S, h.data (), true));
	HIPCHK (hipMemset2D (e->go.state.p + sizeof (mtr_gonio_state), e->go.pitch, 0, e->go.pitch - sizeof (mtr_gonio_state), S));
	return MTR_OK;
}

int mtr_gonio_os_table (uint32_t factor, float* out)
{
	if (!out || factor < 2 || factor > MTR_GONIO_OS_MAX) return fail (MTR_ERR_ARG, "mtr_gonio_os_table: a factor of 2 .. 32 and a table");
	gonio_os_table (factor, out);
	return MTR_OK;
}

int mtr_gonio_os_hpw (double rate, uint32_t factor, float* hpw)
{
	if (!hpw || factor < 1 || factor > MTR_GONIO_OS_MAX || !(rate >= 8000.0)) return fail (MTR_ERR_ARG, "mtr_gonio_os_hpw: a factor of 1 .. 32, rate >= 8000");
	*hpw = gonio_os_hpw (rate, factor);
	return MTR_OK;
}

int mtr_engine_gonio_set_oversample (mtr_engine* e, uint32_t factor)
{
	if (no_gonio (e)) return fail (MTR_ERR_ARG, NO_GONIO);
	if (factor < 1 || factor > MTR_GONIO_OS_MAX) return fail (MTR_ERR_ARG, "mtr_engine_gonio_set_oversample: the factor is 1 (off) or 2 .. 32");
	if (factor > 1 && (double) e->go.cfg.period_frames > floor ((double) e->cfg.sample_rate)) return fail (MTR_ERR_ARG, GONIO_OS_PERIOD);
	if (e->advanced) return fail (MTR_ERR_STATE, "mtr_engine_gonio_set_oversample: only on an engine that has processed nothing since create / reset");
	int rc = wait_stream (e);
	if (rc || (rc = gonio_os_apply (e, factor))) return rc;
	return mtr_engine_gonio_reset (e);
}

int mtr_engine_gonio_oversample (mtr_engine* e, uint32_t* factor, float* hpw)
{
	if (no_gonio (e)) return fail (MTR_ERR_ARG, NO_GONIO);
	if (factor) *factor = e->go.os;
	if (hpw) *hpw = e->go.os > 1 ? e->go.os_hpw : e->go.der.hpw;
	return MTR_OK;
}

int mtr_engine_gonio_os_timing (mtr_engine* e, float* os_ms, uint32_t* pieces)
{
	if (no_gonio (e)) return fail (MTR_ERR_ARG, NO_GONIO);
	int rc = wait_stream (e);
	if (rc) return rc;
	float t = 0.f;
	const size_t n = e->go.os_ev.size () / 2;
	for (size_t i = 0; i < n; ++i) {
		float x = 0.f;
		HIPCHK (hipEventElapsedTime (&x, e->go.os_ev[2 * i].v, e->go.os_ev[2 * i + 1].v));
		t += x;
	}
	e->go.os_ev.clear ();
	if (os_ms) *os_ms = t;
	if (pieces) *pieces = (uint32_t) n;
	return MTR_OK;
}

/* tools/gonio_rate.py: enable != 0 starts timing the two kernels of every piece (events around them); *points_ms / *image_ms: their sums
 * over the *pieces timed since the last query, which are then forgotten.  Synchronises. */
int mtr_engine_gonio_timing (mtr_engine* e, int enable, float* points_ms, float* image_ms, uint32_t* pieces)
{
	if (no_gonio (e)) return fail (MTR_ERR_ARG, NO_GONIO);
	int rc = wait_stream (e);
	if (rc) return rc;
	float p = 0.f, im = 0.f;
	const size_t n = e->go.ev.size () / 3;
	for (size_t i = 0; i < n; ++i) {
		float x = 0.f, y = 0.f;
		HIPCHK (hipEventElapsedTime (&x, e->go.ev[3 * i].v, e->go.ev[3 * i + 1].v));
		HIPCHK (hipEventElapsedTime (&y, e->go.ev[3 * i + 1].v, e->go.ev[3 * i + 2].v));
		p += x; im += y;
	}
	e->go.ev.clear ();
	e->go.timed = enable != 0;
	if (points_ms) *points_ms = p;
	if (image_ms) *image_ms = im;
	if (pieces) *pieces = (uint32_t) n;
	return MTR_OK;
}

} // extern "C"
