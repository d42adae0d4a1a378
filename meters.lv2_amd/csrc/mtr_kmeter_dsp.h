// mtr_kmeter_dsp.h — Kmeterdsp (jmeters/kmeterdsp.cc) as the three "pieces + walk" meters compute it: KMETER's reading series
// (mtr_kmeter.hip: k_kmeter_blocks / k_kmeter_walk), SURROUND's C K-meters (mtr_surround.hip: the walk, final_channel) and, for the
// rule for a square that is not finite (k_kmeter_pieces) and the bookkeeping at the end of a process () (k_kmeter_final), KMETER without
// a period.  One copy of the constants, of a piece's geometry, of
// a lane's weights and of what a walker does between two pieces and at a block's end.  Host + device, header only; the loops — how a
// lane gets its frames, how a workgroup reduces, what a meter carries between two calls — stay with the kernels.  k_sur_pieces computes
// the same weights by statements of its own (mtr_surround.hip says why): whoever changes KmLane or km_square changes them there too.
//
// THE POINTWISE WEIGHTS.  Per channel Kmeterdsp runs, on s = x^2 (w = omega, r = 1 - w),
//     z1 += w (s - z1) for each frame;  z2 += 4 w (z1 - z2) at the end of each group of four frames;  t = max s,
// a block (one process ()) of L frames taking its first Lg = L - L mod 4 of them (:79).  Both states are linear in the squares, so what a
// frame gives to them can be written down frame by frame.  z1 is a one-pole: the frame at block offset j gives
//     w r^(E - 1 - j) s                                                        to z1 at block offset E > j.
// z2 moves at group ends only.  Over one group (z1, z2) -> A (z1, z2) + input, A = [[a, 0], [c, b]], a = r^4, b = 1 - 4 w, c = 4 w a;
// A^k = [[a^k, 0], [c_k, b^k]], c_k = c (a^k - b^k) / (a - b) (mat_pow).  At its own group's end ge the frame has given w r^(ge - 1 - j) s
// to z1 and 4 w times that to z2; k group ends later z2 holds c_k of the former and b^k of the latter:
//     w r^(ge - 1 - j) (c_k + 4 w b^k) s = r^(ge - 1 - j) (ca a^k + cb b^k) s   to z2 at the k-th group end behind ge,
// ca = w c / (a - b), cb = w (4 w - c / (a - b)).  A PIECE [b0, b1) of a block sums these weights times its squares up to where its states
// stand — z1 at E1 = min (b1 - blk0, Lg), z2 at the last group end pe = E1 & ~3 at or in front of it; a frame whose group ends behind pe
// has not reached z2 yet, it arrives through z1 (km_carry).  Frames at j >= Lg weigh nothing and do not enter the maximum.  The groups
// restart at each block's start, so a piece may start and end inside one.
// A lane takes the powers of its first frame from exp () of logarithms the host computed (KmLane::init) and moves them by constants:
// frame by frame (next_frame) and from one of its steps to the next (next_step: st1, sta, stb are the powers over the frames between
// two steps, 4 x 256 in k_kmeter_blocks, a tile in k_sur_pieces).  The sums are double.
// A square that is not finite makes the reference's z1 NaN at the next frame (Inf - Inf) unless it is the block's last counted frame: a
// NaN is added for it (km_square), so the sums become what the reference's would be.
//
// THE WALK.  One thread per channel takes the pieces in order: km_open where a block starts (:74-75), km_carry over a piece — the
// states in front of it advanced in closed form, also through a piece that starts or ends inside a group, plus the piece's sums — and at
// a block's end km_close (:101-109) and km_peak_hold (:124-139) in f32, one rounding per operation.
#ifndef MTR_KMETER_DSP_H
#define MTR_KMETER_DSP_H

#include <hip/hip_runtime.h>

#include <cmath>

#include "mtr_km_consts.h"
#include "mtr_stcorr_scan.h"

// Kmeterdsp::init; frames_per_lane_step: the frames between two steps of a lane of the pieces kernel (a multiple of four)
inline void km_setup (float sample_rate, int frames_per_lane_step, mtr_km_consts* k)
{
	k->omega = 9.72f / sample_rate;
	k->hold = (int32_t) (0.5f * sample_rate + 0.5f);
	const double w = (double) k->omega, kr = 1.0 - w, ka = pow (kr, 4.0), kb = 1.0 - 4.0 * w, c = 4.0 * w * ka, cab = c / (ka - kb);
	const int n = frames_per_lane_step;
	k->pw[0] = ka; k->pw[1] = c; k->pw[2] = kb;
	k->lkr = log (kr); k->lkb = log (kb);
	k->kri = 1.0 / kr; k->kai = 1.0 / ka; k->kbi = 1.0 / kb; k->kr3 = kr * kr * kr;
	k->ca = w * cab; k->cb = w * (4.0 * w - cab);
	k->st1 = pow (kr, (double) -n); k->sta = pow (ka, (double) (-n / 4)); k->stb = pow (kb, (double) (-n / 4));
}

// kmeterdsp.cc:60-65: the fall-back factor of a process () of n frames (15 dB/s)
inline float km_fall (float sample_rate, uint64_t n)
{
	return powf (10.0f, -0.05f * 15.0f * ((float) n / sample_rate));
}

namespace mtr_km {

using mtr_sc::Piece;
using mtr_sc::ipow;

struct Mat { double a, c, b; };          // [[a, 0], [c, b]]
__host__ __device__ inline Mat mat_pow (double a1, double c1, double b1, double k)
{
	// A^k for A = [[a1, 0], [c1, b1]]: c_k = c1 (a1^k - b1^k) / (a1 - b1)
	const double ak = pow (a1, k), bk = pow (b1, k);
	return Mat{ak, c1 * (ak - bk) / (a1 - b1), bk};
}

// ---- a piece's geometry ---------------------------------------------------------------------------------------------------------------

// the call frame at which the block of the piece that starts at b0 starts (negative: it started in an earlier call).  e0: where the block
// open on entry ends; `block`: its length (the period, or — period 0 — the call's)
__device__ __forceinline__ int64_t km_block_start (uint64_t e0, uint64_t block, uint64_t period, int64_t b0)
{
	if ((uint64_t) b0 < e0) return (int64_t) e0 - (int64_t) block;
	return (int64_t) (e0 + ((uint64_t) b0 - e0) / period * period);
}

struct KmGeom {
	int64_t L, Lg;                       // frames of the piece's block, and those of them that count (kmeterdsp.cc:79)
	int64_t p0, E1, pe;                  // block offsets: the piece's start; where its z1 stands — its end, but never inside the block's dropped
	                                     // trailing frames (a call may end there, and Kmeterdsp never runs z1 over them); its last group end
	int64_t b1;                          // the call frame at which the piece ends ...
	bool    closes;                      // ... and whether a process () ends there
};

// LEN: the stream ends at call frame `end` (> pc.b0).  The block an end inside the call cuts has L = the frames the stream has of it — one
// last process (p, L) — and the piece that holds the end stops there
template <bool LEN>
__device__ __forceinline__ KmGeom km_geom (const Piece& pc, int64_t blk0, uint64_t block, int64_t end, uint64_t n_frames)
{
	KmGeom g;
	g.L = (int64_t) block; g.b1 = pc.b1; g.closes = pc.closes;
	if constexpr (LEN) {
		if (end < (int64_t) n_frames && end < blk0 + g.L) g.L = end - blk0;
		if (end <= g.b1) {
			g.b1 = end;
			if (g.L != (int64_t) block) g.closes = true;
		}
	}
	g.Lg = g.L & ~(int64_t) 3;
	g.p0 = pc.b0 - blk0;
	g.E1 = g.b1 - blk0 < g.Lg ? g.b1 - blk0 : g.Lg;
	g.pe = g.E1 & ~(int64_t) 3;
	return g;
}

// ---- a lane's weights -----------------------------------------------------------------------------------------------------------------

// the powers of one frame, at block offset j: its distance to E1 for z1, inside its group (ge: the group's end) and in group ends behind
// it inside the piece for z2
struct KmLane {
	double  p1, pa, pb, pg;              // omega kr^(E1 - 1 - j), ca ka^kt, cb kb^kt, kr^(ge - 1 - j)
	int64_t kt;                          // group ends behind ge inside the piece; < 0: none, the frame's group ends behind the piece's last

	__device__ __forceinline__ void init (const mtr_km_consts& k, int64_t E1, int64_t pe, int64_t jt0)
	{
		const int64_t gt0 = (jt0 | 3) + 1;
		kt = (pe - gt0) >> 2;
		p1 = (double) k.omega * exp ((double) (E1 - 1 - jt0) * k.lkr);
		pa = k.ca * exp ((double) (4 * kt) * k.lkr); pb = k.cb * exp ((double) kt * k.lkb);
		pg = ipow (1.0 - (double) k.omega, (uint64_t) (gt0 - 1 - jt0));
	}
	__device__ __forceinline__ double z1_weight () const { return p1; }
	__device__ __forceinline__ double z2_weight () const { return pg * (pa + pb); }            // (where kt >= 0)
	__device__ __forceinline__ double front_weight (double up) const { return p1 * up; }       // to z1 at pe: up = kri^(E1 - pe)
	// to the frame behind (jk: this one's block offset)
	__device__ __forceinline__ void next_frame (const mtr_km_consts& k, int64_t jk)
	{
		p1 *= k.kri;
		if (((jk + 1) & 3) == 0) { kt -= 1; pa *= k.kai; pb *= k.kbi; pg = k.kr3; }
		else pg *= k.kri;
	}
	// to the lane's next step, `groups` groups of four frames on (the place inside the group stays)
	__device__ __forceinline__ void next_step (const mtr_km_consts& k, int groups)
	{
		p1 *= k.st1; pa *= k.sta; pb *= k.stb; kt -= groups;
	}
};

// what the filter takes for the square s of the frame at block offset jk (the maximum takes s itself, :84)
__device__ __forceinline__ float km_square (float s, int64_t jk, int64_t Lg)
{
	return !isfinite (s) && !(jk == Lg - 1 && s == INFINITY) ? NAN : s;
}

// ---- the walkers' arithmetic ----------------------------------------------------------------------------------------------------------

// kmeterdsp.cc:74-75, where a block starts (a NaN state falls through, as there; it is an f32 here)
__device__ __forceinline__ void km_open (double& z1, double& z2)
{
	z1 = z1 > 50 ? 50 : (z1 < 0 ? 0 : z1);
	z2 = z2 > 50 ? 50 : (z2 < 0 ? 0 : z2);
}

// over a piece of block offsets [p0, E1), E1 > p0: (z1, z2) in front of it carried to E1 (z2: to the last group end there) in closed form,
// plus what the piece's own frames give there (pv_z1, pv_z2).  A piece that starts inside a group: z1 stands p0 & 3 frames into it
__device__ __forceinline__ void km_carry (const mtr_km_consts& k, int64_t p0, int64_t E1, double pv_z1, double pv_z2, double& z1, double& z2)
{
#pragma clang fp contract(off)
	const int64_t m = (E1 >> 2) - (p0 >> 2);                       // group ends in (p0, E1]
	if (m > 0) {
		const Mat g = mat_pow (k.pw[0], k.pw[1], k.pw[2], (double) m);
		z2 = g.b * z2 + g.c * ipow (k.kri, (uint64_t) (p0 & 3)) * z1 + pv_z2;
	}
	z1 = pow (1.0 - (double) k.omega, (double) (E1 - p0)) * z1 + pv_z1;
}

// kmeterdsp.cc:101-109 at a block's end, in f32, one rounding per operation: the states as the reference stores them, and what the
// reading takes — rms, and the block's peak (tmax: its max x^2)
struct KmClose { float rms, t; };
__device__ __forceinline__ KmClose km_close (double& z1, double& z2, float tmax)
{
#pragma clang fp contract(off)
	float f1 = (float) z1, f2 = (float) z2, t = tmax;
	if (isnan (f1)) f1 = 0;                                        // :101-103
	if (isnan (f2)) f2 = 0;
	if (!isfinite (t)) t = 0;
	z1 = (double) (f1 + 1e-20f);                                   // :106-107
	z2 = (double) (f2 + 1e-20f);
	return KmClose{sqrtf (2.0f * f2), sqrtf (t)};                  // :109
}

// kmeterdsp.cc:124-139: the peak's hold and fall-back after a process () of fpp frames
__device__ __forceinline__ void km_peak_hold (float t, float& peak, int32_t& cnt, int32_t hold, uint32_t fpp, float fall)
{
#pragma clang fp contract(off)
	if (t >= peak) { peak = t; cnt = hold; }
	else if (cnt > 0) cnt -= (int32_t) fpp;
	else { peak *= fall; peak += 1e-10f; }
}

}  // namespace mtr_km

#endif
