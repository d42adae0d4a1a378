// mtr_kwmc.hip — K-weighting and (optionally) the 4x true peak for C = 3, 4 or 5 channels (gfx950), layout 8.
//
// Replaces, for a whole batch, Ebu_r128_proc::detect_process with nchan = 3 .. 5 (ebumeter/ebu_r128_proc.cc:302-337: channel i
// weighted by _chan_gain[i] = {1, 1, 1, 1.41, 1.41}) and, per channel, Resampler::process +
// TruePeakdsp::process_max (zita-resampler/resampler.cc:211-235, jmeters/truepeakdsp.cc:101-124).
//
// One wave per (stream, time segment), workgroup = one wave, on the plan every layout shares (tile_start, seg_tile,
// warm_tiles, the powers of A^K for K = MTR_KWMC_RUN).  Per tile (at most 64 K frames):
//   1. lane l loads its run, frames [t0 + K l, t0 + K l + K) x C channels: K C contiguous floats, 16-byte loads where the
//      run is aligned and inside the call (K C is a multiple of four: every lane of a tile has the same alignment);
//      frames past the tile are zeroed in the registers;
//   2. EBU: per pair of channels (the last one padded with a silent channel when C is odd) the exact time-parallel
//      K-filter of k_kw — pass 1 from a zero state, DPP scan with the powers of A^K, pass 2 from the true state
//      (mtr_kw_steps.h) — and sum_c gain_c * sum y_c^2 into tile_power;
//   3. TP: per channel, the run as scaled f16 hi / lo pair words in LDS behind the 48-position halo, and the
//      matrix-pipe interpolator of k_kwtp16 (mtr_mfma16_fir.h: three f16 products, f32 accumulation) over the tile;
//      phase 0 (|x[n - 24]|) on the VALU.  The peaks go by atomicMax into tp_call[s][c].
// The f32 samples never pass through LDS (k_kwtp16's finding: the register fetch beat LDS-DMA staging by 2-3 %), so LDS
// holds only one channel's words at a time: 5.3 KB per wave, whatever C is.
// Non-finite K-filter states are dropped per channel at tile ends (ebu_r128_proc.cc:331-334): a NaN in one channel costs
// only that channel's state.
#include <hip/hip_runtime.h>

#include <utility>

#include <type_traits>

#include "mtr_internal.h"
#include "mtr_mfma16_fir.h"
#include "mtr_wave.h"
#include "mtr_kw_steps.h"

namespace {

constexpr int K = MTR_KWMC_RUN;                 // 20: even (sample pairs of the interpolator's words never straddle two lanes)
constexpr int HALO = MTR_M16_HALO;              // 48
constexpr int LT = 64 * K;
constexpr int WN = (HALO + 64 * K) / 2;         // words per array: positions 0 .. HALO + 64 K - 1
constexpr int CMAX = (HALO + 64 * K) / 16 - 4;  // last column whose 64-sample window lies inside the arrays
static_assert (WN % 4 == 0, "arrays start on 16 bytes");

__device__ __forceinline__ float scrub1 (float v) { return isfinite (v) ? v : 0.f; }

// power-of-two scale that puts a value with exponent field `e` into [2^14, 2^15), and 2^-15 / scale (as k_kwtp16)
__device__ __forceinline__ void pow2_scale (uint32_t e_, float& scale, float& unscale)
{
	const int e = (int) e_;
	const int se = min (238, 268 - e);
	scale = __uint_as_float ((uint32_t) se << 23);
	unscale = __uint_as_float ((uint32_t) (239 - se) << 23);
}

// LEN: the call carries per-stream lengths (mtr_kwmc_len_args, mtr_engine_process_*_lengths).  Frames at or past stream s's end E are
// read as +0.0f, per channel, before they reach the scale, the K-filter or the interpolator's window (no load is issued for them);
// only columns t < E count towards a channel's peak (phase 0 of the last 24 frames never does, as at a call's end); a segment starts
// and stops at E, and one that starts at or past it does nothing.  Tile powers behind E feed fragments the gate never inserts for the
// stream.  The dense instantiation (LEN false) takes the struct it always took and is the kernel's code as it always was.
template <bool LEN> using kwmc_args_t = std::conditional_t<LEN, mtr_kwmc_len_args, mtr_kwmc_args>;
template <bool LEN> __device__ __forceinline__ int64_t kwmc_end (const kwmc_args_t<LEN>& a, uint32_t s)
{
	if constexpr (LEN) return min ((int64_t) a.ends[s], (int64_t) a.n_frames);
	else return 0;
}

// FC: samples per frame of the buffer.  FC == C: the engine's own frames, the kernel as it always was.  FC == 6 with C == 5: WAVE 5.1
// frames L R C LFE Ls Rs read where they lie (mtr_engine_set_frame_layout with map {0, 1, 2, 4, 5}): engine channel c is source channel
// wide_ch (c), a compile-time index everywhere — the lane's K x 6 floats arrive in the same 16-byte loads, one float4 in flight, and
// the LFE is dropped as the pieces arrive; xr stays K x C.
template <int C, int FC> __device__ __forceinline__ constexpr int wide_ch (int c) { return FC == C ? c : (c < 3 ? c : c + 1); }

#define KWMC_KERNEL_HEAD template <int C, bool EBU, bool TP, bool LEN> __global__ __launch_bounds__ (64) void k_kwmc (const kwmc_args_t<LEN> a)
#define KWMC_LOCALS constexpr int FC = C;
#include "mtr_kwmc_body.h"
#undef KWMC_KERNEL_HEAD
#undef KWMC_LOCALS

// five channels from WAVE 5.1 frames (a.audio: [S][stride][6])
#define KWMC_KERNEL_HEAD template <bool EBU, bool TP, bool LEN> __global__ __launch_bounds__ (64) void k_kwmc51 (const kwmc_args_t<LEN> a)
#define KWMC_LOCALS constexpr int C = 5, FC = 6;
#include "mtr_kwmc_body.h"
#undef KWMC_KERNEL_HEAD
#undef KWMC_LOCALS

template <bool LEN>
int launch_51 (bool ebu, bool tp, const kwmc_args_t<LEN>& a, uint32_t n_units, hipStream_t st)
{
	if (ebu && tp)  hipLaunchKernelGGL ((k_kwmc51<true, true, LEN>), dim3 (n_units), dim3 (64), 0, st, a);
	else if (ebu)   hipLaunchKernelGGL ((k_kwmc51<true, false, LEN>), dim3 (n_units), dim3 (64), 0, st, a);
	else if (tp)    hipLaunchKernelGGL ((k_kwmc51<false, true, LEN>), dim3 (n_units), dim3 (64), 0, st, a);
	else return -2;
	return hipGetLastError () == hipSuccess ? 0 : -1;
}

template <int C, bool LEN>
int launch_c (bool ebu, bool tp, const kwmc_args_t<LEN>& a, uint32_t n_units, hipStream_t st)
{
	if (ebu && tp)  hipLaunchKernelGGL ((k_kwmc<C, true, true, LEN>), dim3 (n_units), dim3 (64), 0, st, a);
	else if (ebu)   hipLaunchKernelGGL ((k_kwmc<C, true, false, LEN>), dim3 (n_units), dim3 (64), 0, st, a);
	else if (tp)    hipLaunchKernelGGL ((k_kwmc<C, false, true, LEN>), dim3 (n_units), dim3 (64), 0, st, a);
	else return -2;
	return hipGetLastError () == hipSuccess ? 0 : -1;
}

template <bool LEN>
int launch_any (int C, bool ebu, bool tp, const kwmc_args_t<LEN>& a, uint32_t n_units, hipStream_t st)
{
	switch (C) {
	case 3: return launch_c<3, LEN> (ebu, tp, a, n_units, st);
	case 4: return launch_c<4, LEN> (ebu, tp, a, n_units, st);
	case 5: return launch_c<5, LEN> (ebu, tp, a, n_units, st);
	default: return -2;
	}
}

}  // namespace

int mtr_launch_kwmc (int C, bool ebu, bool tp, const mtr_kwmc_args& a, const uint32_t* ends, uint32_t n_units, void* stream)
{
	if (!ends) return launch_any<false> (C, ebu, tp, a, n_units, (hipStream_t) stream);
	mtr_kwmc_len_args la;
	static_cast<mtr_kwmc_args&> (la) = a;
	la.ends = ends;
	return launch_any<true> (C, ebu, tp, la, n_units, (hipStream_t) stream);
}

int mtr_launch_kwmc51 (bool ebu, bool tp, const mtr_kwmc_args& a, const uint32_t* ends, uint32_t n_units, void* stream)
{
	if (!ends) return launch_51<false> (ebu, tp, a, n_units, (hipStream_t) stream);
	mtr_kwmc_len_args la;
	static_cast<mtr_kwmc_args&> (la) = a;
	la.ends = ends;
	return launch_51<true> (ebu, tp, la, n_units, (hipStream_t) stream);
}
