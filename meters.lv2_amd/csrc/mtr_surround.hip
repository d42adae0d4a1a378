// mtr_surround.hip — sur_run (src/surmeter.c:115-147: the surround3 .. surround8 plugins) for a batch (gfx950): per stream of C = 3 .. 8
// channels C x Kmeterdsp::process + read (m, p) (jmeters/kmeterdsp.cc:56-153) and n_pairs = C > 3 ? 4 : 3 x Stcorrdsp::process + read ()
// (jmeters/stcorrdsp.cc:47-93) on the channel pairs (a [p], b [p]) — from ONE read of the frames.
//
// One sur_run is the engine call, or — with a period P, for the reading series — every block of exactly P frames, wherever the calls
// cut the audio.  A call is cut into PIECES exactly as mtr_stcorr.hip cuts it (mtr_stcorr_scan.h: never across a block boundary, at
// most `chunk` frames — a multiple of four, so that a block's pieces start on Kmeterdsp's groups of four); one workgroup reduces one
// (stream, piece), one thread per (stream, channel) and one per (stream, pair) walk the pieces in order and do everything that happens
// at a block's end.  No atomics; the same bits on every run.
//
// A workgroup takes its piece tile by tile (1792 frames = 256 lanes x 7; the tiles are aligned to the piece's END, the first one starts
// `warm` frames or more in front of it).  The tile's frames — C x 1792 contiguous floats of the stream's row — are loaded ONCE with
// 16-byte loads on 16-byte addresses of the buffer (the floats in front of the first / behind the last whole quad that lies inside the
// stream's frames [lo, b1) one by one: an odd C leaves a row only 4-byte aligned, and nothing outside [lo, b1) is ever read) and stored
// channel-planar in LDS: [C][1792] floats, 57 344 bytes at C = 8.  Everything else reads LDS: lane t owns frames 7 t .. 7 t + 6 of the
// tile (stride 7 dwords: no bank conflicts).
//
//  * K-meters.  Kmeterdsp's end state is linear in the squares s = x^2, so every frame of a piece weighs into z1 and z2 at the piece's end
//    by powers that depend on its place in its block alone: mtr_kmeter_dsp.h derives these pointwise weights and holds the piece's
//    geometry, the lane's powers, the rule for a square that is not finite and the walk's arithmetic for KMETER's reading series and
//    for the walk here; k_sur_pieces writes the geometry and the powers out itself.  Frames at j >= L - L mod 4 (L = P, or the call's
//    length) weigh nothing and do not enter the maximum (kmeterdsp.cc:71), nor do the warm-up frames in front of the piece.  A lane
//    takes the powers of its first frame in the first tile from exp (), steps them through its seven frames and from tile to tile by
//    constants (no pow () in the loop); the sums are double.  The walk (final_channel) carries (z1, z2) from piece to piece in closed
//    form and rounds to f32 where the reference ends a process ().
//  * Correlations.  Per pair exactly k_stcorr_pieces' two passes (the head of mtr_stcorr.hip explains them: the carried zl / zr at
//    "frame -1", the first stage rebuilt over `warm` frames, what the sums "owe" behind a period end that flushed), on 7-frame runs;
//    the four pairs walk the staged tile one after the other, and the second pass computes its inputs from the staged samples again
//    instead of holding them: with the constants every lane would compute alike passed from the host (scalar registers), every pair's
//    carried first-stage state in LDS and the rare "owes" sums reduced where they arise, the kernel holds 223 .. 248 VGPRs, no
//    scratch, and two workgroups fit a CU.  The walk over a pair's pieces is stcorr_walk (mtr_stcorr_scan.h).
//
// Track lengths (mtr_any.h): k_sur_pieces<C, true> and k_sur_final<true>, launched only by a call that carries
// per-stream ends.  A workgroup is one (stream, piece), so the stream's end is one scalar: it cuts the piece, and the block it cuts has
// the length the K-meters count their groups and weights from; see the kernels.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <type_traits>
#include <vector>

#include "mtr_engine_impl.h"
#include "mtr_kmeter_dsp.h"
#include "mtr_stcorr_scan.h"

#define MTR_SUR_MAXCH 8
#define MTR_SUR_PAIRS 4

/* per (stream, channel): Kmeterdsp (jmeters/kmeterdsp.h).  z1, z2 are doubles: inside a block that a call cut they are the exact
 * continuation; at a block's end they hold the f32 the reference stores */
typedef struct mtr_sur_chan {
	double   z1, z2;
	float    level, peak;         /* read (m, p): P = 0 _rms (max-held until read) and _peak; P > 0 those after the last completed block */
	float    tmax;                /* max x^2 of the open block so far */
	int32_t  cnt, flag;
	uint32_t pad_;
} mtr_sur_chan;

/* per (stream, pair): Stcorrdsp (jmeters/stcorrdsp.h) and its last reading */
typedef struct mtr_sur_pair {
	float    z[5];                /* zl zr zlr zll zrr */
	float    corr;
} mtr_sur_pair;

/* per stream; in front, for the state blob (whose header has no room for them): the engine's period, the frames into the open block,
 * Kmeterdsp's _fpp / _fall and the pairs — the host's copies rule, export writes them in */
typedef struct mtr_sur_state {
	uint32_t     period, fill;
	uint32_t     fpp;
	float        fall;
	uint8_t      pa[MTR_SUR_PAIRS], pb[MTR_SUR_PAIRS];
	mtr_sur_chan ch[MTR_SUR_MAXCH];
	mtr_sur_pair pr[MTR_SUR_PAIRS];
} mtr_sur_state;

/* doubles per (stream, piece): MTR_SUR_PIECE_PAIR per pair (mtr_stcorr_scan.h), and per channel what the piece's frames give to z1 and z2
 * at its end, max x^2 */
#define MTR_SUR_PIECE (MTR_SUR_PAIRS * MTR_SUR_PIECE_PAIR + 3 * MTR_SUR_MAXCH)

/* mtr_sur_consts (mtr_km_consts.h) as k_sur_pieces takes it: flat, in the order its scalar loads are grouped by.  The pieces kernel
 * steps its lanes' powers itself (the statements of KmLane, on 7-frame runs out of LDS): through KmLane and the nested struct it
 * measured 0.2 - 0.6 % slower without a period, dense and with track lengths, outside the spread of this one's own runs
 * (profiles/r38_dsp_once.md) */
typedef struct mtr_sur_pieces_consts {
	double lkr, lkb, lq;          /* log kr, log kb, log q */
	double kri, kai, kbi, kr3;    /* 1 / kr, 1 / ka, 1 / kb, kr^3 */
	double ca, cb;                /* the z2 weight of a frame is kr^(..) (ca ka^k + cb kb^k) */
	double st1, sta, stb, sq;     /* kr^-TILE, ka^-(TILE / 4), kb^-(TILE / 4), q^-TILE: from tile to tile */
	double d1, d2, d4, d8, d64;   /* r^K to the powers of the wave scan */
} mtr_sur_pieces_consts;

typedef struct mtr_sur_args {
	const float*    audio;        /* [S][stride][C] */
	uint64_t        stride, n_frames;
	uint64_t        period;       /* frames per sur_run of the reading series; 0: the call is one */
	uint64_t        e0;           /* call frame at which the block open on entry ends (period 0: n_frames) */
	uint64_t        block;        /* L: frames per block (the period, or the call's length) */
	uint32_t        n_streams, n_channels, n_pairs, n_pieces;
	uint32_t        chunk, warm;
	float           w1, w2;       /* Stcorrdsp::init */
	float           omega, fall;  /* Kmeterdsp: omega, the fall-back factor of fpp */
	uint32_t        fpp;
	int32_t         hold;
	double          pw[3];        /* A = [[a, 0], [c, b]] per group of four frames (mtr_kmeter_dsp.h) */
	mtr_sur_pieces_consts k;      /* what every lane would compute alike: in scalar registers */
	uint8_t         pa[MTR_SUR_PAIRS], pb[MTR_SUR_PAIRS];
	uint32_t        capacity;     /* points per stream the series hold */
	uint64_t        point0;       /* blocks completed before this call */
	mtr_sur_state*  state;        /* [S] */
	double*         piece;        /* [S][n_pieces][MTR_SUR_PIECE] */
	float*          s_level;      /* [S][capacity][C], NULL if capacity == 0 */
	float*          s_peak;       /* [S][capacity][C] */
	float*          s_corr;       /* [S][capacity][4] */
} mtr_sur_args;

// per-stream ends (mtr_any.h): what the LEN instantiations take on top — a struct of its own, so that the dense kernels
// keep their arguments
typedef struct mtr_sur_len_args : mtr_sur_args {
	const uint32_t* ends;         /* [S] call frame at which the stream ends, <= n_frames; 0: closed, nothing of it is touched */
	const float*    falls;        /* [S] Kmeterdsp's fall-back factor of each stream that ends inside the call: that of the frames it has of its last block */
} mtr_sur_len_args;

namespace {

using namespace mtr_sc;
using namespace mtr_km;                  // the K-meters' geometry, weights and walk (mtr_kmeter_dsp.h)

constexpr int NT = 256;                  // threads per workgroup
constexpr int K = 7;                     // frames per lane run: an odd dword stride in LDS
constexpr int TILE = NT * K;             // frames per tile: 1792
constexpr int MAX_TILES = 8;             // tiles per piece (chunk + warm)

__device__ __forceinline__ int64_t block_start (const mtr_sur_args& a, const Piece& pc) { return km_block_start (a.e0, a.block, a.period, pc.b0); }

// Kmeterdsp's constants for the walk (one thread per channel), out of the flat arguments
__device__ __forceinline__ mtr_km_consts km_of (const mtr_sur_args& a)
{
	return mtr_km_consts{a.omega, a.hold, {a.pw[0], a.pw[1], a.pw[2]}, a.k.lkr, a.k.lkb, a.k.kri, a.k.kai, a.k.kbi, a.k.kr3, a.k.ca, a.k.cb, a.k.st1, a.k.sta, a.k.stb};
}

template <bool LEN> using sur_args_of = std::conditional_t<LEN, mtr_sur_len_args, mtr_sur_args>;

// LEN: the stream ends at call frame a.ends[s] (0: closed, untouched; n_frames: the dense call's stream).  Its piece is [b0, min (b1, end)):
// one that starts at or behind the end returns before it touches memory, as k_stcorr_pieces<LEN>; a truncated one has its tiles aligned
// to the stream's end, so that nothing at or behind it is read.  The block an end inside the call cuts has L = the frames the stream has
// of it, as in k_kmeter_blocks: the K-meters take L & ~3 of them, the weights counted back from the stream's own last group.  A workgroup
// is one (stream, piece): all of this is uniform, no lane holds a second set of weights.
template <int C, bool LEN = false>
__global__ __launch_bounds__ (NT, 2) void k_sur_pieces (const sur_args_of<LEN> a)
{
	const uint32_t s = blockIdx.y;
	const Piece pc = piece_of (a, blockIdx.x);
	const float* const src = a.audio + (size_t) s * a.stride * C;
	int64_t pb1 = pc.b1, L = (int64_t) a.block;
	if constexpr (LEN) {
		const int64_t end = (int64_t) a.ends[s];
		if (pc.b0 >= end) return;                                  // (uniform in the workgroup; end 0: every piece of the stream)
		const int64_t bs = block_start (a, pc);
		if (end < (int64_t) a.n_frames && end < bs + L) L = end - bs;   // one last sur_run, of the frames the stream has of the block
		if (end < pb1) pb1 = end;
	}
	const int64_t b0 = pc.b0, b1 = pb1;
	const int64_t warm = b0 == 0 ? 1 : (int64_t) a.warm;          // (the call's first piece: only the slot of frame -1)
	const int nt = (int) ((b1 - b0 + warm + TILE - 1) / TILE);      // <= MAX_TILES: chunk + warm <= MAX_TILES * TILE
	const int64_t lo = b0 - warm > 0 ? b0 - warm : 0;              // the first frame that is read
	const int64_t T0 = b1 - (int64_t) nt * TILE;                    // < b0
	const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;

	__shared__ float lds[C * TILE];
	__shared__ double sh_tot[NT / 64][2];
	__shared__ double sh_red[NT / 64][5];
	__shared__ double sh_zt[MTR_SUR_PAIRS][2];                     // zl, zr of every pair in front of the tile (the first one starts from nothing)
	__shared__ double sh_owe[NT / 64][MTR_SUR_PAIRS][2];           // per wave: sum c rho zl, sum c rho zr of a piece behind a period end
	if (tid < 2 * MTR_SUR_PAIRS) sh_zt[tid >> 1][tid & 1] = 0.0;
	if (tid < 2 * MTR_SUR_PAIRS * (NT / 64)) (&sh_owe[0][0][0])[tid] = 0.0;
	double* const out = a.piece + ((size_t) s * a.n_pieces + blockIdx.x) * MTR_SUR_PIECE;

	// ---- the K-meters' geometry: block offsets ----
	const int64_t blk0 = block_start (a, pc);
	const int64_t Lg = LEN ? L & ~(int64_t) 3 : (int64_t) (a.block & ~(uint64_t) 3);   // frames of a block the K-meters take
	// block offset at which the piece's z1 stands: its end, but never inside the block's dropped trailing frames — a call may end there
	// (P mod 4 != 0), and Kmeterdsp never runs z1 over them
	const int64_t E1 = b1 - blk0 < Lg ? b1 - blk0 : Lg;
	const int64_t pe = E1 & ~(int64_t) 3;                           // ... and its last group end
	// the powers of the lane's first frame in the first tile — its distance to the piece's end E1 for z1, inside its group and in group
	// ends behind it for z2 — from exp (); from tile to tile (1792 frames = 448 groups) they move by constants
	const int64_t jt0 = T0 + (int64_t) K * tid - blk0;
	const int64_t gt0 = (jt0 | 3) + 1;                             // its group's end
	int32_t kt = (int32_t) ((pe - gt0) >> 2);                      // group ends behind that one inside the piece; < 0: none
	double pt1 = (double) a.omega * exp ((double) (E1 - 1 - jt0) * a.k.lkr);
	double pta = a.k.ca * exp ((double) (4 * kt) * a.k.lkr), ptb = a.k.cb * exp ((double) kt * a.k.lkb);
	const double pg0 = ipow (1.0 - (double) a.omega, (uint64_t) (gt0 - 1 - jt0));
	double e1[C], e2[C];
	float tm[C];
#pragma unroll
	for (int c = 0; c < C; ++c) { e1[c] = 0.0; e2[c] = 0.0; tm[c] = 0.f; }

	// ---- the correlations' constants (mtr_stcorr.hip) ----
	const double w1 = (double) a.w1, r = 1.0 - w1, q1 = 1.0 - (double) a.w2, bias = (double) 1e-20f;
	ScanPow sp;
	sp.d1 = a.k.d1; sp.d2 = a.k.d2; sp.d4 = a.k.d4; sp.d8 = a.k.d8;
	sp.dp = ipow (sp.d1, (lane & 15) + 1);
	sp.dq = lane >= 32 ? ipow (sp.d1, lane - 31) : 0.0;
	const double dl = ipow (sp.d1, lane);                          // from the wave's first frame to this lane's run
	const double d64 = a.k.d64;                                    // ... and over a whole wave
	// weight of a run's sums at the piece's end: w2 q^(frames behind the run); from tile to tile it grows by q^-TILE
	double W = (double) a.w2 * exp ((double) ((int64_t) nt * TILE - (int64_t) K * (tid + 1)) * a.k.lq);
	double tot[MTR_SUR_PAIRS][3];                                  // lr ll rr
#pragma unroll
	for (int p = 0; p < MTR_SUR_PAIRS; ++p) tot[p][0] = tot[p][1] = tot[p][2] = 0.0;

	// 16-byte loads on 16-byte addresses: quads of floats from a float of the BUFFER whose index is a multiple of four
	const int64_t base = (int64_t) ((reinterpret_cast<size_t> (src) >> 2) & 3);
	const int64_t glo = lo * C, ghi = b1 * C;                      // the floats of the stream's row that may be read

	for (int t = 0; t < nt; ++t) {
		const int64_t T = T0 + (int64_t) t * TILE;
		// ---- stage the tile: floats [T C, (T + TILE) C) of the row, channel-planar ----
		{
			const int64_t gt = T * C;
			const int64_t gq0 = gt - ((base + gt) & 3);
#pragma unroll 2
			for (int i = tid; i < TILE * C / 4 + 1; i += NT) {
				const int64_t gq = gq0 + 4 * (int64_t) i;
				float v[4] = { 0.f, 0.f, 0.f, 0.f };
				if (gq >= glo && gq + 3 < ghi) {
					const float4 q = *reinterpret_cast<const float4*> (src + gq);
					v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
				} else {
#pragma unroll
					for (int e = 0; e < 4; ++e) if (gq + e >= glo && gq + e < ghi) v[e] = src[gq + e];
				}
#pragma unroll
				for (int e = 0; e < 4; ++e) {
					const int64_t li = gq + e - gt;
					if (li >= 0 && li < (int64_t) TILE * C) {
						const uint32_t u = (uint32_t) li, fr = u / C, ch = u - fr * C;
						lds[ch * TILE + fr] = v[e];
					}
				}
			}
		}
		__syncthreads ();
		const bool head = T < b0;                                  // frames in front of the piece: they rebuild zl, zr and weigh nothing
		const int64_t f0 = T + (int64_t) K * tid;

		// ---- the K-meters: the lane's seven frames of every channel ----
		if (f0 + K > b0) {                                         // (frames of the piece end at the tile's end)
			// the lane's powers stepped frame by frame, every channel's square in turn
			const int64_t j0 = f0 - blk0;
			int32_t kk = kt;
			double p1 = pt1, pa = pta, pb = ptb, pg = pg0;           // omega kr^(E1 - 1 - j), ca ka^k, cb kb^k, kr^(ge - 1 - j)
#pragma unroll
			for (int k = 0; k < K; ++k) {
				const int64_t jk = j0 + k;
				if (f0 + k >= b0 && jk < Lg) {                     // (jk < E1 with it: E1 = min (Lg, b1 - blk0))
					const double wz1 = p1, wz2 = kk >= 0 ? pg * (pa + pb) : 0.0;
#pragma unroll
					for (int c = 0; c < C; ++c) {
						const float x = lds[c * TILE + tid * K + k];
						float sq = x * x;
						tm[c] = tm[c] < sq ? sq : tm[c];               // kmeterdsp.cc:84: if (t < s) t = s (a NaN never enters)
						if (!isfinite (sq) && !(jk == Lg - 1 && sq == INFINITY)) sq = NAN;   // (see the head of the file)
						e1[c] = fma (wz1, (double) sq, e1[c]);
						e2[c] = fma (wz2, (double) sq, e2[c]);
					}
				}
				p1 *= a.k.kri;
				if (((jk + 1) & 3) == 0) { kk -= 1; pa *= a.k.kai; pb *= a.k.kbi; pg = a.k.kr3; }
				else pg *= a.k.kri;
			}
		}
		pt1 *= a.k.st1; pta *= a.k.sta; ptb *= a.k.stb; kt -= TILE / 4;

		// ---- the correlations: the pairs one after the other over the staged tile ----
#pragma unroll
		for (int p = 0; p < MTR_SUR_PAIRS; ++p) {
			if (p >= (int) a.n_pairs) break;
			const float* const la = lds + (uint32_t) a.pa[p] * TILE + tid * K;
			const float* const lb = lds + (uint32_t) a.pb[p] * TILE + tid * K;
			double zc[2] = { 0.0, 0.0 };                           // the carried zl, zr: "frame -1" (in the call's first tile alone)
			if (T < 0) { zc[0] = (double) a.state[s].pr[p].z[0]; zc[1] = (double) a.state[s].pr[p].z[1]; }
			if (pc.after_period) {                                 // (not finite: the period before is flushed, its zl with it)
				if (!isfinite (zc[0])) zc[0] = 0.0;
				if (!isfinite (zc[1])) zc[1] = 0.0;
			}
			double* const po = out + p * MTR_SUR_PIECE_PAIR;
			// the inputs of the one-pole (both passes compute them from the staged samples: fourteen doubles less to hold)
			auto input = [&] (int k, double& ul, double& ur) {
				float xa = la[k], xb = lb[k];
				if (!head) {
					ul = fma (w1, (double) xa, bias); ur = fma (w1, (double) xb, bias);
				} else {
					const int64_t f = f0 + k;
					if (pc.after_period && f < b0) {
						if (!isfinite (xa)) xa = 0.f;
						if (!isfinite (xb)) xb = 0.f;
					}
					ul = f >= 0 ? fma (w1, (double) xa, bias) : f == -1 ? zc[0] : 0.0;
					ur = f >= 0 ? fma (w1, (double) xb, bias) : f == -1 ? zc[1] : 0.0;
				}
			};
			// pass 1: the run's end value from zero
			double vl = 0.0, vr = 0.0;
#pragma unroll
			for (int k = 0; k < K; ++k) {
				double ul, ur;
				input (k, ul, ur);
				vl = fma (r, vl, ul); vr = fma (r, vr, ur);
			}
			// the state each run starts from: scan across the wave, then across the waves
			vl = scan (vl, sp); vr = scan (vr, sp);
			__syncthreads ();                                      // (the pair before has read sh_tot)
			if (lane == 63) { sh_tot[wid][0] = vl; sh_tot[wid][1] = vr; }
			__syncthreads ();
			double cin[2] = { 0.0, 0.0 }, zt[2] = { sh_zt[p][0], sh_zt[p][1] };
#pragma unroll
			for (int w = 0; w < NT / 64; ++w) {
				if (w == wid) { cin[0] = zt[0]; cin[1] = zt[1]; }
				zt[0] = fma (d64, zt[0], sh_tot[w][0]); zt[1] = fma (d64, zt[1], sh_tot[w][1]);
			}
			__syncthreads ();                                      // (every lane has read the state in front of this tile)
			if (tid == 0) { sh_zt[p][0] = zt[0]; sh_zt[p][1] = zt[1]; }
			double zl = fma (dl, cin[0], dppd<0x138, 0xF> (vl));   // (wave_shr:1: the scan of the lane to the left, lane 0 reads 0)
			double zr = fma (dl, cin[1], dppd<0x138, 0xF> (vr));
			// pass 2: the products, carried to the run's end
			const bool owes = pc.after_period && T < b0 + warm;    // uniform
			double alr = 0.0, all = 0.0, arr = 0.0, abl = 0.0, abr = 0.0;
			double rho = owes && f0 > b0 ? ipow (r, (uint64_t) (f0 - b0)) : 1.0;
#pragma unroll
			for (int k = 0; k < K; ++k) {
				double ul, ur;
				input (k, ul, ur);
				zl = fma (r, zl, ul); zr = fma (r, zr, ur);
				double plr = zl * zr, pll = zl * zl, prr = zr * zr;
				if (head && f0 + k < b0) { plr = 0.0; pll = 0.0; prr = 0.0; }
				alr = fma (alr, q1, plr); all = fma (all, q1, pll); arr = fma (arr, q1, prr);
				if (owes) {
					const int64_t f = f0 + k;
					if (f == b0 - 1) { po[7] = zl; po[8] = zr; }   // the start state itself (one lane of the workgroup)
					const bool in = f >= b0;
					if (in) rho *= r;
					abl = fma (abl, q1, in ? rho * zl : 0.0); abr = fma (abr, q1, in ? rho * zr : 0.0);
				}
			}
			tot[p][0] = fma (W, alr, tot[p][0]); tot[p][1] = fma (W, all, tot[p][1]); tot[p][2] = fma (W, arr, tot[p][2]);
			if (owes) {                                            // (the first tiles of such a piece alone: summed over the wave at once)
				abl *= W; abr *= W;
#pragma unroll
				for (int d = 32; d >= 1; d >>= 1) { abl += __shfl_xor (abl, d, 64); abr += __shfl_xor (abr, d, 64); }
				if (lane == 0) { sh_owe[wid][p][0] += abl; sh_owe[wid][p][1] += abr; }
			}
		}
		W *= a.k.sq;
		__syncthreads ();                                          // (every lane has read its runs: the next tile may overwrite them)
	}

	// ---- the workgroup's sums: the pairs, then the channels ----
#pragma unroll
	for (int p = 0; p < MTR_SUR_PAIRS; ++p) {
		if (p >= (int) a.n_pairs) break;
#pragma unroll
		for (int d = 32; d >= 1; d >>= 1)
#pragma unroll
			for (int j = 0; j < 3; ++j) tot[p][j] += __shfl_xor (tot[p][j], d, 64);
		__syncthreads ();
		if (lane == 0) { for (int j = 0; j < 3; ++j) sh_red[wid][j] = tot[p][j]; sh_red[wid][3] = sh_owe[wid][p][0]; sh_red[wid][4] = sh_owe[wid][p][1]; }
		__syncthreads ();
		if (tid == 0) {
			double* const po = out + p * MTR_SUR_PIECE_PAIR;
			for (int j = 0; j < 5; ++j) {
				double e = 0.0;
				for (int w = 0; w < NT / 64; ++w) e += sh_red[w][j];
				po[j < 3 ? j : j + 2] = e;
			}
			po[3] = sh_zt[p][0]; po[4] = sh_zt[p][1];
		}
	}
#pragma unroll
	for (int c = 0; c < C; ++c) {
#pragma unroll
		for (int d = 32; d >= 1; d >>= 1) {
			e1[c] += __shfl_xor (e1[c], d, 64); e2[c] += __shfl_xor (e2[c], d, 64);
			tm[c] = fmaxf (tm[c], __shfl_xor (tm[c], d, 64));
		}
		__syncthreads ();
		if (lane == 0) { sh_red[wid][0] = e1[c]; sh_red[wid][1] = e2[c]; sh_red[wid][2] = (double) tm[c]; }
		__syncthreads ();
		if (tid == 0) {
			double x1 = 0.0, x2 = 0.0, xm = 0.0;
			for (int w = 0; w < NT / 64; ++w) { x1 += sh_red[w][0]; x2 += sh_red[w][1]; xm = fmax (xm, sh_red[w][2]); }
			double* const co = out + MTR_SUR_PAIRS * MTR_SUR_PIECE_PAIR + 3 * c;
			co[0] = x1; co[1] = x2; co[2] = xm;
		}
	}
}

// one thread per (stream, channel): the pieces in order, and kmeterdsp.cc:74-75, 101-138 + read (m, p) at every end of a block
// LEN: the pieces up to the stream's end; an end inside the call closes the block there — one Kmeterdsp::process (p, L) of the L frames the
// stream has of it: L & ~3 frames, fpp = L with the fall-back factor a.falls[s] (kmeterdsp.cc:65-70, 79)
template <bool LEN>
__device__ void final_channel (const sur_args_of<LEN>& a, uint32_t s, uint32_t c, int64_t end)
{
#pragma clang fp contract(off)     // (the f32 steps at a block's end are the reference's, one rounding each: no fused multiply-add)
	mtr_sur_chan* const st = &a.state[s].ch[c];
	const mtr_km_consts km = km_of (a);
	double z1 = st->z1, z2 = st->z2;
	float level = st->level, peak = st->peak, tmax = st->tmax;
	int32_t cnt = st->cnt, flag = st->flag;
	uint64_t point = a.point0;
	for (uint32_t i = 0; i < a.n_pieces; ++i) {
		const Piece pc = piece_of (a, i);
		if constexpr (LEN) {
			if (pc.b0 >= end) break;
		}
		const KmGeom g = km_geom<LEN> (pc, block_start (a, pc), a.block, end, a.n_frames);
		if (g.p0 == 0) {
			km_open (z1, z2);
			tmax = 0.f;
		}
		const double* const pv = a.piece + ((size_t) s * a.n_pieces + i) * MTR_SUR_PIECE + MTR_SUR_PAIRS * MTR_SUR_PIECE_PAIR + 3 * c;
		if (g.E1 > g.p0) km_carry (km, g.p0, g.E1, pv[0], pv[1], z1, z2);
		const float pm = (float) pv[2];
		tmax = tmax < pm ? pm : tmax;
		if (!g.closes) continue;
		const KmClose r = km_close (z1, z2, tmax);
		if (a.period || flag) { level = r.rms; flag = 0; }         // :112-121 (a host that reads after every block always finds the flag set)
		else if (r.rms > level) level = r.rms;
		uint32_t fpp = a.fpp;
		float fall = a.fall;
		if constexpr (LEN) {
			if (g.L != (int64_t) a.block) { fpp = (uint32_t) g.L; fall = a.falls[s]; }
		}
		km_peak_hold (r.t, peak, cnt, a.hold, fpp, fall);
		if (a.period) {
			if (point < a.capacity) {
				const size_t o = ((size_t) s * a.capacity + point) * a.n_channels + c;
				a.s_level[o] = level; a.s_peak[o] = peak;
			}
			++point;
		}
	}
	st->z1 = z1; st->z2 = z2; st->level = level; st->peak = peak; st->tmax = tmax; st->cnt = cnt; st->flag = flag;
}

// one thread per (stream, pair): stcorr_walk (mtr_stcorr_scan.h) over the pair's slots, as k_stcorr_final
template <bool LEN>
__device__ void final_pair (const sur_args_of<LEN>& a, uint32_t s, uint32_t p, int64_t end)
{
	mtr_sur_pair* const st = &a.state[s].pr[p];
	const StcorrWalk v = { st->z, &st->corr, a.piece + (size_t) s * a.n_pieces * MTR_SUR_PIECE + p * MTR_SUR_PIECE_PAIR, MTR_SUR_PIECE,
	                       a.capacity ? a.s_corr + (size_t) s * a.capacity * MTR_SUR_PAIRS + p : nullptr, MTR_SUR_PAIRS };
	stcorr_walk<LEN> (a, v, end);
}

template <bool LEN>
__global__ void k_sur_final (const sur_args_of<LEN> a)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, per = a.n_channels + a.n_pairs;
	if (i >= a.n_streams * per) return;
	const uint32_t s = i / per, u = i % per;
	int64_t end = (int64_t) a.n_frames;
	if constexpr (LEN) {
		end = (int64_t) a.ends[s];
		if (end == 0) return;                                          // closed, or closed by this call untouched
	}
	if (u < a.n_channels) final_channel<LEN> (a, s, u, end);
	else final_pair<LEN> (a, s, u - a.n_channels, end);
}

}  // namespace

static void mtr_sur_geometry (float w1, uint32_t* warm, uint32_t* chunk)
{
	// |1 - w1|^J < 2^-48, as mtr_stcorr_geometry; the chunk a multiple of four frames (Kmeterdsp's groups)
	const double ar = fabs (1.0 - (double) w1);
	double J = ar > 0.0 && ar < 1.0 ? ceil (-48.0 * log (2.0) / log (ar)) : 1.0;
	const double most = (double) (MAX_TILES / 2 * TILE);
	if (!(J >= 1.0)) J = 1.0;
	if (J > most) J = most;
	*warm = ((uint32_t) J + K) / K * K;                            // (+ the slot of frame -1)
	*chunk = (MAX_TILES * TILE - *warm) & ~3u;
}

// A: mtr_sur_args — the dense kernels — or mtr_sur_len_args
template <typename A> static int mtr_launch_sur (const A& a, void* stream)
{
	constexpr bool LEN = std::is_same_v<A, mtr_sur_len_args>;
	hipStream_t st = (hipStream_t) stream;
	const dim3 g (a.n_pieces, a.n_streams), b (NT);
	switch (a.n_channels) {
	case 3: hipLaunchKernelGGL ((k_sur_pieces<3, LEN>), g, b, 0, st, a); break;
	case 4: hipLaunchKernelGGL ((k_sur_pieces<4, LEN>), g, b, 0, st, a); break;
	case 5: hipLaunchKernelGGL ((k_sur_pieces<5, LEN>), g, b, 0, st, a); break;
	case 6: hipLaunchKernelGGL ((k_sur_pieces<6, LEN>), g, b, 0, st, a); break;
	case 7: hipLaunchKernelGGL ((k_sur_pieces<7, LEN>), g, b, 0, st, a); break;
	case 8: hipLaunchKernelGGL ((k_sur_pieces<8, LEN>), g, b, 0, st, a); break;
	default: return -1;
	}
	const uint32_t n = a.n_streams * (a.n_channels + a.n_pairs);
	hipLaunchKernelGGL (k_sur_final<LEN>, dim3 ((n + 63) / 64), dim3 (64), 0, st, a);
	return hipGetLastError () == hipSuccess ? 0 : -1;
}

// ---- SURROUND in the engine: set-up, the call's step, the blob's section and the cursors in it, the C entry points --------------------

static uint32_t sur_pairs (const mtr_engine* e) { return e->cfg.n_channels > 3 ? 4u : 3u; }

static uint32_t sur_min_period (const mtr_engine* e) { return (uint32_t) e->cfg.sample_rate / 20; }

static int surround_create (mtr_engine* e)
{
	const uint32_t C = e->cfg.n_channels;
	mtr_setup_stcorr (e->cfg.sample_rate, e->su.w);
	mtr_sur_geometry (e->su.w[0], &e->su.warm, &e->su.chunk);
	mtr_sur_consts& k = e->su.k;
	km_setup (e->cfg.sample_rate, TILE, &k.km);                    // (a lane of k_sur_pieces: seven frames, every tile)
	const double r = 1.0 - (double) e->su.w[0], q = 1.0 - (double) e->su.w[1];
	k.lq = log (q); k.sq = pow (q, (double) -TILE);
	k.d1 = ipow (r, K); k.d2 = k.d1 * k.d1; k.d4 = k.d2 * k.d2; k.d8 = k.d4 * k.d4; k.d64 = ipow (k.d8, 8);
	for (uint32_t p = 0; p < MTR_SUR_PAIRS; ++p) {                 // the surround8 port defaults (lv2ttl/surmeter.h), clamped
		e->su.pa[p] = (uint8_t) std::min (2 * p, C - 1); e->su.pb[p] = (uint8_t) std::min (2 * p + 1, C - 1);
	}
	return MTR_OK;
}

// The blocks of the reading series are cut from where the CALL started (e->pos): every chunk of a host call sees the same cuts
// A call with ends (mtr_engine_process_*_any, or any call once a stream of the view is closed) takes the LEN instantiations; every other
// call the dense ones, as ever.
static int surround_step (mtr_engine* e, const Call& c, Cursors& nx, const StreamEnds& se)
{
	const size_t vo = c.off;
	const uint64_t P = e->su.ser.period;
	const uint32_t cap = e->su.ser.cap;
	mtr_sur_args sa;
	memset (&sa, 0, sizeof (sa));
	sa.audio = c.audio; sa.stride = c.stride; sa.n_frames = c.n_frames;
	sa.period = P; sa.e0 = series_e0 (e->pos.su, P, c.n_frames);
	sa.block = P ? P : c.n_frames;
	sa.n_streams = c.cnt; sa.n_channels = e->cfg.n_channels; sa.n_pairs = sur_pairs (e);
	sa.chunk = e->su.chunk; sa.warm = e->su.warm;
	sa.n_pieces = mtr_sc::n_pieces (c.n_frames, sa.e0, P, sa.chunk);
	sa.w1 = e->su.w[0]; sa.w2 = e->su.w[1];
	const uint32_t fpp = P ? (uint32_t) P : (uint32_t) c.n_frames;
	if (nx.su_fpp != fpp) {                                        // kmeterdsp.cc:65-70
		nx.su_fall = km_fall (e->cfg.sample_rate, fpp);
		nx.su_fpp = fpp;
	}
	sa.fpp = nx.su_fpp; sa.fall = nx.su_fall;
	const mtr_sur_consts& k = e->su.k;
	sa.omega = k.km.omega; sa.hold = k.km.hold;
	memcpy (sa.pw, k.km.pw, sizeof (sa.pw));
	sa.k = { k.km.lkr, k.km.lkb, k.lq, k.km.kri, k.km.kai, k.km.kbi, k.km.kr3, k.km.ca, k.km.cb, k.km.st1, k.km.sta, k.km.stb, k.sq, k.d1, k.d2, k.d4, k.d8, k.d64 };
	memcpy (sa.pa, e->su.pa, sizeof (sa.pa)); memcpy (sa.pb, e->su.pb, sizeof (sa.pb));
	sa.capacity = cap; sa.point0 = e->pos.su.points;
	if (e->su.piece.reserve ((size_t) e->cfg.n_streams * sa.n_pieces * MTR_SUR_PIECE)) return fail (MTR_ERR_NOMEM, "hipMalloc SURROUND pieces");
	sa.state = e->su.state.p + vo; sa.piece = e->su.piece.p + vo * sa.n_pieces * MTR_SUR_PIECE;
	if (cap) {
		sa.s_level = e->su.s_level.p + vo * cap * sa.n_channels;
		sa.s_peak = e->su.s_peak.p + vo * cap * sa.n_channels;
		sa.s_corr = e->su.s_corr.p + vo * cap * MTR_SUR_PAIRS;
	}
	if (se.ends) {
		mtr_sur_len_args la;
		static_cast<mtr_sur_args&> (la) = sa;
		la.ends = se.ends; la.falls = reinterpret_cast<const float*> (se.own);
		if (mtr_launch_sur (la, c.st)) return fail (MTR_ERR_HIP, "k_sur launch (ends)");
	} else if (mtr_launch_sur (sa, c.st)) return fail (MTR_ERR_HIP, "k_sur launch");
	nx.su = series_advance (e->pos.su, P, c.n_frames);
	return MTR_OK;
}

// the meter's word of a ragged call (SideMeter::ends_fill): its K-meters' fall-back factor, as KMETER's from the meter's own cursor
static uint64_t surround_ends_fill (const mtr_engine* e, const Call& c, uint32_t* own) { kmeter_falls (e, c, e->pos.su.fill, e->su.ser.period, own); return 0; }

static void surround_sections (const mtr_engine* e, std::vector<StateSection>& v)
{
	v.push_back ({ e->su.state.p, sizeof (mtr_sur_state) });
}

// The blob header: period, the frames into the open block, _fpp / _fall and the pairs — what stands in front of `ch` in every stream's
// entry.  A fresh engine takes them; any other must stand at the same period, fill and pairs
constexpr size_t SUR_HDR_BYTES = offsetof (mtr_sur_state, ch);
constexpr const char* SUR_CORRUPT = "mtr_engine_state_import: corrupt blob (period or pairs of the SURROUND meter)";

static void surround_hdr_write (const mtr_engine* e, void* out)
{
	mtr_sur_state h;
	memset (&h, 0, SUR_HDR_BYTES);
	h.period = e->su.ser.period; h.fill = (uint32_t) e->pos.su.fill; h.fpp = e->pos.su_fpp; h.fall = e->pos.su_fall;
	memcpy (h.pa, e->su.pa, sizeof (h.pa)); memcpy (h.pb, e->su.pb, sizeof (h.pb));
	memcpy (out, &h, SUR_HDR_BYTES);
}

static int surround_hdr_check (const mtr_engine* e, const void* in, bool fresh)
{
	const uint32_t C = e->cfg.n_channels;
	mtr_sur_state h;
	memcpy (&h, in, SUR_HDR_BYTES);
	bool ok = series_blob_ok (h.period, h.fill, sur_min_period (e), 0x7ffffffeu);
	for (int p = 0; p < MTR_SUR_PAIRS; ++p) ok = ok && h.pa[p] < C && h.pb[p] < C;
	if (!ok) return fail (MTR_ERR_STATE, SUR_CORRUPT);
	if (!fresh && (h.period != e->su.ser.period || h.fill != e->pos.su.fill || memcmp (h.pa, e->su.pa, sizeof (h.pa)) || memcmp (h.pb, e->su.pb, sizeof (h.pb))))
		return fail (MTR_ERR_STATE, "mtr_engine_state_import: the engine does not stand where the blob's streams do (period or pairs of the SURROUND meter)");
	return MTR_OK;
}

static void surround_hdr_take (mtr_engine* e, const void* in)
{
	mtr_sur_state h;
	memcpy (&h, in, SUR_HDR_BYTES);
	e->su.ser.period = h.period; e->pos.su.fill = h.fill; e->pos.su_fpp = h.fpp; e->pos.su_fall = h.fall;
	memcpy (e->su.pa, h.pa, sizeof (h.pa)); memcpy (e->su.pb, h.pb, sizeof (h.pb));
}

static constinit BlobHeader surround_hdr = { .offset = 0, .bytes = SUR_HDR_BYTES, .corrupt = SUR_CORRUPT, .write = surround_hdr_write, .check = surround_hdr_check, .take = surround_hdr_take };
static SeriesView surround_series (mtr_engine* e) { return { &e->su.ser, &Cursors::su, &e->su.points }; }
constinit SideMeter surround_meter = { .bits = MTR_METER_SURROUND, .max_frames = 0x7fffffffull, .max_text = "SURROUND: n_frames per call must be < 2^31 - 1 (the reference's int n)",
                                       .create = surround_create, .reset = mtr_engine_surround_reset, .step = surround_step, .sections = surround_sections, .hdr = &surround_hdr,
                                       .series = surround_series, .ends_words = 1, .ends_fill = surround_ends_fill };

extern "C" {

static int no_sur (const mtr_engine* e) { return !e || !(e->cfg.meters & MTR_METER_SURROUND); }
static const char* const NO_SUR = "no SURROUND in this engine";

int mtr_engine_surround_reset (mtr_engine* e)
{
	if (no_sur (e)) return fail (MTR_ERR_ARG, NO_SUR);
	e->snap_valid = false;
	HIPCHK (hipSetDevice (e->cfg.device));
	const uint32_t S = e->cfg.n_streams;
	if (e->su.state.reserve (S)) return fail (MTR_ERR_NOMEM, "hipMalloc SURROUND state");
	HIPCHK (hipStreamSynchronize (e->last_stream));
	HIPCHK (hipMemset (e->su.state.p, 0, S * sizeof (mtr_sur_state)));   // kmeterdsp.cc:33-40, stcorrdsp.cc:33-36
	e->pos.su = {};
	e->su.points.assign (S, 0);
	e->pos.su_fpp = 0;
	e->pos.su_fall = 0.f;
	return MTR_OK;
}

int mtr_engine_surround_set_pairs (mtr_engine* e, const uint8_t* a4, const uint8_t* b4)
{
	if (no_sur (e) || !a4 || !b4) return fail (MTR_ERR_ARG, e && (e->cfg.meters & MTR_METER_SURROUND) ? "mtr_engine_surround_set_pairs: null argument" : NO_SUR);
	if (e->su.ser.period && e->pos.su.fill) return fail (MTR_ERR_STATE, "mtr_engine_surround_set_pairs: a block of the reading series is open");
	const uint8_t top = (uint8_t) (e->cfg.n_channels - 1);
	for (int p = 0; p < MTR_SUR_PAIRS; ++p) {                      // surmeter.c:124-125
		e->su.pa[p] = std::min (a4[p], top); e->su.pb[p] = std::min (b4[p], top);
	}
	return MTR_OK;
}

int mtr_engine_surround_pairs (const mtr_engine* e, uint8_t* a4, uint8_t* b4)
{
	if (no_sur (e)) return fail (MTR_ERR_ARG, NO_SUR);
	if (a4) memcpy (a4, e->su.pa, MTR_SUR_PAIRS);
	if (b4) memcpy (b4, e->su.pb, MTR_SUR_PAIRS);
	return MTR_OK;
}

int mtr_engine_surround_set_period (mtr_engine* e, uint32_t period_frames, uint32_t capacity_points)
{
	if (no_sur (e)) return fail (MTR_ERR_ARG, NO_SUR);
	int rc = series_configure_check (e, "mtr_engine_surround_set_period", period_frames, sur_min_period (e), "(uint32_t) sample_rate / 20");
	if (rc || (rc = wait_stream (e))) return rc;
	const size_t n = (size_t) e->cfg.n_streams * capacity_points, C = e->cfg.n_channels;
	if ((rc = series_ring (e->su.s_level, n * C, "hipMalloc SURROUND series")) || (rc = series_ring (e->su.s_peak, n * C, "hipMalloc SURROUND series"))
	    || (rc = series_ring (e->su.s_corr, n * MTR_SUR_PAIRS, "hipMalloc SURROUND series"))) return rc;
	e->su.ser = { period_frames, capacity_points };
	return mtr_engine_surround_reset (e);
}

static int sur_states (mtr_engine* e, uint32_t first, uint32_t count, std::vector<mtr_sur_state>& h)
{
	int rc = meter_range (e, !no_sur (e), NO_SUR, first, count);
	if (rc || (rc = wait_stream (e))) return rc;
	h.resize (count);
	if (count) HIPCHK (hipMemcpy (h.data (), e->su.state.p + first, count * sizeof (mtr_sur_state), hipMemcpyDeviceToHost));
	return MTR_OK;
}

int mtr_engine_surround_read (mtr_engine* e, uint32_t first, uint32_t count, float* level, float* peak, float* corr)
{
	std::vector<mtr_sur_state> h;
	const int rc = sur_states (e, first, count, h);
	if (rc) return rc;
	const uint32_t C = e->cfg.n_channels;
	for (uint32_t i = 0; i < count; ++i) {
		for (uint32_t c = 0; c < C; ++c) {
			if (level) level[(size_t) i * C + c] = h[i].ch[c].level;
			if (peak) peak[(size_t) i * C + c] = h[i].ch[c].peak;
			h[i].ch[c].flag = 1;
		}
		if (corr) for (int p = 0; p < MTR_SUR_PAIRS; ++p) corr[(size_t) i * MTR_SUR_PAIRS + p] = h[i].pr[p].corr;
	}
	// (P = 0: Kmeterdsp::read arms the next process () to restart the rms maximum, kmeterdsp.cc:154)
	if (!e->su.ser.period && count) HIPCHK (hipMemcpy (e->su.state.p + first, h.data (), count * sizeof (mtr_sur_state), hipMemcpyHostToDevice));
	return MTR_OK;
}

int mtr_engine_surround_pair_states (mtr_engine* e, uint32_t first, uint32_t count, float* state5)
{
	if (!state5) return fail (MTR_ERR_ARG, "mtr_engine_surround_pair_states: null argument");
	std::vector<mtr_sur_state> h;
	const int rc = sur_states (e, first, count, h);
	if (rc) return rc;
	for (uint32_t i = 0; i < count; ++i)
		for (int p = 0; p < MTR_SUR_PAIRS; ++p) memcpy (state5 + ((size_t) i * MTR_SUR_PAIRS + p) * 5, h[i].pr[p].z, sizeof (h[i].pr[p].z));
	return MTR_OK;
}

int mtr_engine_surround_series (mtr_engine* e, uint32_t first, uint32_t count, float* level, float* peak, float* corr,
                                uint32_t capacity, uint32_t* n_points, uint32_t* dropped)
{
	int rc = meter_range (e, !no_sur (e), NO_SUR, first, count);
	if (rc) return rc;
	const size_t take = series_counts (e->pos.su.points, e->su.ser.cap, capacity, n_points, dropped);
	if ((!level && !peak && !corr) || !count || !take) return MTR_OK;
	if ((rc = wait_stream (e))) return rc;
	const size_t C = e->cfg.n_channels;
	const struct { float* out; const float* src; size_t w; } row[3] = { { level, e->su.s_level.p, C }, { peak, e->su.s_peak.p, C }, { corr, e->su.s_corr.p, MTR_SUR_PAIRS } };
	for (const auto& q : row) {
		if (!q.out) continue;
		if ((rc = series_fetch (q.out, q.src, q.w, first, e->su.ser.cap, capacity, take, count))) return rc;
		// (a stream that was closed has fewer points of its own than the open ones: 0.0f behind them, whatever the ring still holds there)
		for (uint32_t i = 0; i < count; ++i) {
			const uint64_t own = e->su.points[first + i];
			if (own < take) memset (q.out + ((size_t) i * capacity + (size_t) own) * q.w, 0, (take - (size_t) own) * q.w * sizeof (float));
		}
	}
	return MTR_OK;
}

} // extern "C"
