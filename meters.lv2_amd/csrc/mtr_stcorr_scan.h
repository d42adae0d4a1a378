// mtr_stcorr_scan.h — what the two Stcorrdsp kernels share (mtr_stcorr.hip: one stereo pair per stream; mtr_surround.hip: up to four
// pairs of a 3 .. 8 channel frame): how a call is cut into pieces that never span a period boundary, and the (decay, value) scan of
// the first-stage one-poles across a wave.  Device code, header only; the kernels' own geometry (threads, frames per lane run, tile)
// stays with them.
#ifndef MTR_STCORR_SCAN_H
#define MTR_STCORR_SCAN_H

#include <hip/hip_runtime.h>

#include <cstdint>

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

}  // namespace mtr_sc

#endif
