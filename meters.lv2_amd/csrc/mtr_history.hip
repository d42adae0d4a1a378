// mtr_history.hip — k_history: the last step of every call of an engine with MTR_METER_TRUEPEAK or MTR_METER_TPBALLIST.  The new
// 47-frame history = the last 47 frames of (old history ++ this call's audio): what Resampler::process keeps in its window between
// calls (zita-resampler/resampler.cc:229-262).  The histories ping-pong (hist_in: what the call read, hist_out: what the next one
// reads), so a row that stays is copied across.
//
// One lane per (stream, history frame).  Which frames "the last 47" are is the CUT rule of the call (HistCut, mtr_internal.h;
// CallRun::history picks it) — i = the row's frame, 0 .. 46, f = the call frame it takes, f < 0: frame 47 + f of the old row:
//   HIST_CALL_END             f = n_frames - 47 + i, every stream touched: the dense call.
//   HIST_CALL_END_IF_TOUCHED  ends [s] != 0 ? n_frames - 47 + i : i - 47: a call with lengths.  An untouched stream keeps its row; a
//                             stream that closes keeps whatever follows its end in the buffer: nothing reads it again.
//   HIST_OWN_END              f = ends [s] - 47 + i: a call with ends of a TPBALLIST engine.  A stream that ends inside the call leaves the
//                             frames in front of its OWN end, so that its part of the state blob does not depend on what lies behind
//                             it; end 0: every f < 0, the old row.
// The row is [47][HC]: HC = 2 for the mono and stereo engines (mono: the right channel stays zero), C for 3 .. 5 channels.  The
// buffer's frames hold FC samples: C, or 6 for five channels read from WAVE 5.1 frames (L R C LFE Ls Rs, the call k_kwmc51 served).
//
// Lane i == 0 of a touched stream also folds the call's true peak where the gate does not: tp_call != NULL (layout 8) per channel,
// else fold_state != NULL (a deferred gate: mtr_engine.hip) the stereo pair — mtr_fold_truepeak_mc / mtr_fold_truepeak, mtr_internal.h.
// Bounds: f < n_frames (or ends [s]) <= stride, 47 + f in 0 .. 46, c < HC; a lane at or behind n_streams * 47 returns at once.
#include <hip/hip_runtime.h>

#include "mtr_internal.h"

namespace {

template <HistCut CUT>
__global__ void k_history (const mtr_history_args a)
{
	const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
	if (g >= a.n_streams * MTR_FIR_HALO) return;
	const uint32_t s = g / MTR_FIR_HALO, i = g % MTR_FIR_HALO;
	const uint32_t end = CUT == HIST_CALL_END ? 1u : a.ends[s];
	const bool touched = end != 0;
	const int64_t f = (int64_t) i - MTR_FIR_HALO + (CUT == HIST_OWN_END ? (int64_t) end : touched ? (int64_t) a.n_frames : 0);
	const bool wave51 = a.FC == 6 && a.C == 5;
	for (uint32_t c = 0; c < a.HC; ++c) {
		float v = 0.f;                                                      // (mono: the right channel stays zero)
		if (c < a.C) v = f >= 0 ? a.audio[((size_t) s * a.stride + (size_t) f) * a.FC + (wave51 && c >= 3 ? c + 1 : c)]
		                        : a.hist_in[((size_t) s * MTR_FIR_HALO + (size_t) (MTR_FIR_HALO + f)) * a.HC + c];
		a.hist_out[((size_t) s * MTR_FIR_HALO + i) * a.HC + c] = v;
	}
	if (!touched || i != 0) return;
	if (a.tp_call) mtr_fold_truepeak_mc (a.tp_call, a.tp_last, a.tp_hold, a.state + s, s, a.C);
	else if (a.fold_state && a.C == 2) mtr_fold_truepeak (a.fold_state + s);
}

}  // namespace

int mtr_launch_history (HistCut cut, const mtr_history_args& a, void* stream)
{
	if ((cut != HIST_CALL_END && !a.ends) || a.C < 1 || a.C > MTR_MAX_CHANNELS || (a.FC != a.C && !(a.FC == 6 && a.C == 5))) return -1;
	const dim3 grid ((a.n_streams * MTR_FIR_HALO + 255) / 256);
	hipStream_t st = (hipStream_t) stream;
	switch (cut) {
	case HIST_CALL_END:            hipLaunchKernelGGL (k_history<HIST_CALL_END>, grid, dim3 (256), 0, st, a); break;
	case HIST_CALL_END_IF_TOUCHED: hipLaunchKernelGGL (k_history<HIST_CALL_END_IF_TOUCHED>, grid, dim3 (256), 0, st, a); break;
	case HIST_OWN_END:             hipLaunchKernelGGL (k_history<HIST_OWN_END>, grid, dim3 (256), 0, st, a); break;
	default: return -1;
	}
	return hipGetLastError () == hipSuccess ? 0 : -1;
}
