// mtr_stcorr_scan.h — what the two Stcorrdsp kernels share (mtr_stcorr.hip: one stereo pair per stream; mtr_surround.hip: up to four
// pairs of a 3 .. 8 channel frame): how a call is cut into pieces that never span a period boundary, the (decay, value) scan of
// the first-stage one-poles across a wave, and the walk over a pair's pieces (stcorr_walk: what k_stcorr_final and k_sur_final do per
// pair).  Device code, header only; the kernels' own geometry (threads, frames per lane run, tile) stays with them.  The pieces of
// mtr_kmeter_dsp.h are cut the same way.
#ifndef MTR_STCORR_SCAN_H
#define MTR_STCORR_SCAN_H

#include <hip/hip_runtime.h>

#include <cstdint>

#define MTR_STCORR_PIECE 9         /* doubles per (stream, piece, pair): the sums of zlr zll zrr carried to the piece's end, zl and zr there; of a
                                    * piece that starts where a period ended inside the call also sum c rho zl, sum c rho zr (rho = (1 - w1)^(frames
                                    * since the period end): what the sums owe to the start state) and the zl, zr it started from */
#define MTR_SUR_PIECE_PAIR MTR_STCORR_PIECE

namespace mtr_sc {

struct Piece {
	int64_t b0, b1;                      // frames [b0, b1) of the call
	bool    after_period;                // starts where a period ended inside this call
	bool    closes;                      // ends a process (): a period, or (period 0) the call
};

__host__ __device__ inline uint64_t div_up (uint64_t a, uint64_t b) { return (a + b - 1) / b; }

// piece i of a call: the open period's rest [0, e0), then whole periods, then what the call leaves open — each cut at `chunk`
// (A: the kernel's arguments — n_frames, e0, period, chunk)
template <typename A>
__device__ inline Piece piece_of (const A& a, uint32_t i)
{
	const uint64_t N = a.n_frames, first = a.e0 < N ? a.e0 : N;
	const uint32_t c0 = (uint32_t) div_up (first, a.chunk);
	uint64_t s0, s1;
	uint32_t k;
	if (i < c0) { s0 = 0; s1 = a.e0; k = i; }
	else {
		const uint32_t cp = (uint32_t) div_up (a.period, a.chunk);
		s0 = a.e0 + (uint64_t) ((i - c0) / cp) * a.period; s1 = s0 + a.period; k = (i - c0) % cp;
	}
	const uint64_t e = s1 < N ? s1 : N;
	Piece p;
	p.b0 = (int64_t) (s0 + (uint64_t) k * a.chunk);
	p.b1 = (int64_t) (p.b0 + a.chunk < e ? p.b0 + a.chunk : e);
	p.after_period = k == 0 && s0 > 0;
	p.closes = (uint64_t) p.b1 == e && s1 <= N;
	return p;
}

// ... and how many there are
inline uint32_t n_pieces (uint64_t n_frames, uint64_t e0, uint64_t period, uint32_t chunk)
{
	const uint64_t first = e0 < n_frames ? e0 : n_frames;
	uint64_t n = div_up (first, chunk);
	if (period && n_frames > e0) {
		const uint64_t rest = n_frames - e0;
		n += rest / period * div_up (period, chunk) + div_up (rest % period, chunk);
	}
	return (uint32_t) n;
}

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dppd (double v)
{
	// (lanes without a source — out of row, masked row — read 0)
	const int lo = __builtin_amdgcn_update_dpp (0, __double2loint (v), CTRL, ROW_MASK, 0xF, true);
	const int hi = __builtin_amdgcn_update_dpp (0, __double2hiint (v), CTRL, ROW_MASK, 0xF, true);
	return __hiloint2double (hi, lo);
}

// x^n, n >= 0 small (x may be negative: 1 - w1 = -0.57 at 8 kHz)
__host__ __device__ inline double ipow (double x, uint64_t n)
{
	double y = 1.0;
	for (; n; n >>= 1, x *= x) if (n & 1) y *= x;
	return y;
}

// the constant decays of the wave scan: d = r^K per lane
struct ScanPow {
	double d1, d2, d4, d8;               // wave-uniform
	double dp, dq;                       // d^((lane & 15) + 1), d^(lane - 31) (lanes 32 .. 63)
};

// in-place inclusive scan over the wave: v_l <- sum_{j <= l} d^(l - j) v_j (the pattern of mtrw::scan, one-pole)
__device__ __forceinline__ double scan (double v, const ScanPow& s)
{
	v = fma (s.d1, dppd<0x111, 0xF> (v), v);
	v = fma (s.d2, dppd<0x112, 0xF> (v), v);
	v = fma (s.d4, dppd<0x114, 0xF> (v), v);
	v = fma (s.d8, dppd<0x118, 0xF> (v), v);
	v = fma (s.dp, dppd<0x142, 0xA> (v), v);     // rows 1, 3 <- the complete scan of lane 15 / 47's row
	v = fma (s.dq, dppd<0x143, 0xC> (v), v);     // rows 2, 3 <- the complete scan at lane 31
	return v;
}

// ---- the walk: one thread per (stream, pair) takes the pieces in order ----------------------------------------------------------------

// where one pair's state, piece slots and series live
struct StcorrWalk {
	float*        z5;                    // zl zr zlr zll zrr
	float*        corr;                  // the last reading
	const double* piece;                 // the pair's slot (MTR_STCORR_PIECE doubles) of the stream's first piece ...
	size_t        piece_stride;          // ... and the doubles from one piece to the next
	float*        series;                // the pair's point 0 of the stream (not read where capacity == 0) ...
	size_t        series_stride;         // ... and the floats from one point to the next
};

// z = q^len z + sum per piece, and stcorrdsp.cc:65-75 + read () at every end of a process ().
// (A: the kernel's arguments — what piece_of needs, w1, w2, capacity, point0, n_pieces)
// LEN: the pieces up to the stream's end (> 0); the one that holds it is the stream's last, with its own length, and — if the stream ends
// inside the call — it ends a process () whether a period ends there or not: the truncated block, appended at the stream's own point index.
// Compiled without contraction, so that neither caller's surroundings decide a rounding and the f32 steps at a period's end are the
// reference's, one rounding per operation.  (The pragma pins them; __fadd_rn (__fmul_rn (..)) does not — the header's own `*` and `+`
// are compiled under the default contraction and fuse into one v_fma_f32 once inlined.)
template <bool LEN, typename A>
__device__ void stcorr_walk (const A& a, const StcorrWalk& v, int64_t end)
{
#pragma clang fp contract(off)
	const double q1 = 1.0 - (double) a.w2;
	double z[3] = { (double) v.z5[2], (double) v.z5[3], (double) v.z5[4] };
	float zl = v.z5[0], zr = v.z5[1], corr = *v.corr;
	uint64_t point = a.point0;
	int64_t len_of = -1;
	double qp = 1.0;
	bool flushed[2] = { false, false };
	for (uint32_t i = 0; i < a.n_pieces; ++i) {
		Piece pc = piece_of (a, i);
		bool ends_here = false;                                        // (LEN: the stream's last piece)
		if constexpr (LEN) {
			if (pc.b0 >= end) break;
			if (end <= pc.b1) {
				ends_here = true;
				if ((uint64_t) end < a.n_frames) pc.closes = true;         // one last process (), of what the stream has of the block
				pc.b1 = end;
			}
		}
		const int64_t len = pc.b1 - pc.b0;
		if (len != len_of) { qp = pow (q1, (double) len); len_of = len; }
		const double* const pv = v.piece + (size_t) i * v.piece_stride;
		double sum[3] = { pv[0], pv[1], pv[2] }, el = pv[3], er = pv[4];
		if (pc.after_period && (flushed[0] || flushed[1])) {
			// the period before left zl (zr) = 0 where the piece started from pv[7] (pv[8]): with rho = r^(frames since), zl' = zl + rho dl
			const double dl = flushed[0] ? -pv[7] : 0.0, dr = flushed[1] ? -pv[8] : 0.0;
			const double r = 1.0 - (double) a.w1, r2 = r * r;
			double cq = 0.0, rr = 1.0;                                 // sum c rho^2 = w2 sum_m q^(len - m) r^(2m), m = 1 .. len
			for (int64_t m = 1; m <= len && rr > 1e-300; ++m) { rr *= r2; cq += ipow (q1, (uint64_t) (len - m)) * rr; }
			cq *= (double) a.w2;
			sum[0] += dr * pv[5] + dl * pv[6] + dl * dr * cq;
			sum[1] += 2.0 * dl * pv[5] + dl * dl * cq;
			sum[2] += 2.0 * dr * pv[6] + dr * dr * cq;
			const double re = ipow (r, (uint64_t) len);
			el += re * dl; er += re * dr;
		}
		if (pc.after_period) flushed[0] = flushed[1] = false;
		for (int j = 0; j < 3; ++j) z[j] = fma (qp, z[j], sum[j]);
		const bool last = i + 1 == a.n_pieces || ends_here;
		if (last) { zl = (float) el; zr = (float) er; }
		if (!pc.closes) continue;
		float f[3] = { (float) z[0], (float) z[1], (float) z[2] };
		flushed[0] = !isfinite (f[1]); flushed[1] = !isfinite (f[2]);  // this period leaves zl (zr) = 0 to the next
		// (the channel's first stage: not finite anywhere in the process () means not finite at its end, stcorrdsp.cc:65-66)
		if (last && (!isfinite (zl) || !isfinite (f[1]))) zl = 0.f;
		if (last && (!isfinite (zr) || !isfinite (f[2]))) zr = 0.f;
		for (int j = 0; j < 3; ++j) {
			if (!isfinite (f[j])) f[j] = 0.f;                      // :67-69
			f[j] = f[j] + 1e-10f;                                  // :73-75
			z[j] = (double) f[j];
		}
		corr = f[0] / sqrtf (f[1] * f[2] + 1e-10f);                // :81 (two roundings, as the reference's: see above)
		if (a.period) {
			if (point < a.capacity) v.series[(size_t) point * v.series_stride] = corr;
			++point;
		}
	}
	v.z5[0] = zl; v.z5[1] = zr;
	for (int j = 0; j < 3; ++j) v.z5[2 + j] = (float) z[j];
	*v.corr = corr;
}

}  // namespace mtr_sc

#endif
