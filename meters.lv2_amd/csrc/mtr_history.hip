// mtr_history.hip — k_history: the last step of every call of an engine with MTR_METER_TRUEPEAK or MTR_METER_TPBALLIST, and of every call of a
// goniometer that oversamples (gonio_os_step, mtr_gonio.hip).  The new history = the last FRAMES frames of (old history ++ this call's
// audio): what Resampler::process keeps in its window between calls (zita-resampler/resampler.cc:229-262).  The histories ping-pong
// (hist_in: what the call read, hist_out: what the next one reads), so a row that stays is copied across.
//
// The row's geometry is the instantiation's (HistRow, mtr_internal.h; the launcher's second argument):
//   HIST_ROW_FIR    FRAMES = 47 (the 48-tap interpolator), a stream's row is [47][HC] and nothing else: ROW = 0, "47 * a.HC floats".  HC = 2
//                   for the mono and stereo engines (mono: the right channel stays zero), C for 3 .. 5 channels.
//   HIST_ROW_GONIO  FRAMES = 23 (the goniometer's 12-tap rows), a stream's row is ROW = 48 floats: [23][2], then two words of the state
//                   blob's header, which are the host's (written at export) — the kernel writes floats 0 .. 2 * 23 - 1 of a row and never
//                   those two: HC = 2, which the launcher insists on.
// One lane per (stream, history frame).  Which frames "the last FRAMES" are is the CUT rule of the call (HistCut, mtr_internal.h;
// CallRun::history and gonio_os_step pick it) — i = the row's frame, 0 .. FRAMES - 1, f = the call frame it takes, f < 0: frame
// FRAMES + f of the old row (a call shorter than the row mixes the two):
//   HIST_CALL_END             f = n_frames - FRAMES + i, every stream touched: the dense call.
//   HIST_CALL_END_IF_TOUCHED  ends [s] != 0 ? n_frames - FRAMES + i : i - FRAMES: a call with lengths.  An untouched stream keeps its row; a
//                             stream that closes keeps whatever follows its end in the buffer: nothing reads it again.  (47-frame rows only.)
//   HIST_OWN_END              f = ends [s] - FRAMES + i: a call with ends of a TPBALLIST engine or of the goniometer.  A stream that ends inside
//                             the call leaves the frames in front of its OWN end, so that its part of the state blob does not depend on what
//                             lies behind it; end 0: every f < 0, the old row.
// The buffer's frames hold FC samples: C, or 6 for five channels read from WAVE 5.1 frames (L R C LFE Ls Rs, the call k_kwmc51 served).
//
// Lane i == 0 of a touched stream also folds the call's true peak where the gate does not: tp_call != NULL (layout 8) per channel,
// else fold_state != NULL (a deferred gate: mtr_engine.hip) the stereo pair — mtr_fold_truepeak_mc / mtr_fold_truepeak, mtr_internal.h.
// The goniometer passes neither.
// Bounds: f < n_frames (or ends [s]) <= stride, FRAMES + f in 0 .. FRAMES - 1, c < HC; a lane at or behind n_streams * FRAMES returns at once.
#include <hip/hip_runtime.h>

#include "mtr_internal.h"

namespace {

template <HistCut CUT, int FRAMES, int ROW>
__global__ void k_history (const mtr_history_args a)
{
	const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
	if (g >= a.n_streams * FRAMES) return;
	const uint32_t s = g / FRAMES, i = g % FRAMES;
	const uint32_t end = CUT == HIST_CALL_END ? 1u : a.ends[s];
	const bool touched = end != 0;
	const int64_t f = (int64_t) i - FRAMES + (CUT == HIST_OWN_END ? (int64_t) end : touched ? (int64_t) a.n_frames : 0);
	const bool wave51 = a.FC == 6 && a.C == 5;
	const auto at = [&] (size_t k, uint32_t c) { return ROW ? (size_t) s * ROW + k * a.HC + c : ((size_t) s * FRAMES + k) * a.HC + c; };   // channel c of the row's frame k
	for (uint32_t c = 0; c < a.HC; ++c) {
		float v = 0.f;                                                      // (mono: the right channel stays zero)
		if (c < a.C) v = f >= 0 ? a.audio[((size_t) s * a.stride + (size_t) f) * a.FC + (wave51 && c >= 3 ? c + 1 : c)]
		                        : a.hist_in[at ((size_t) (FRAMES + f), c)];
		a.hist_out[at (i, c)] = v;
	}
	if (!touched || i != 0) return;
	if (a.tp_call) mtr_fold_truepeak_mc (a.tp_call, a.tp_last, a.tp_hold, a.state + s, s, a.C);
	else if (a.fold_state && a.C == 2) mtr_fold_truepeak (a.fold_state + s);
}

}  // namespace

int mtr_launch_history (HistCut cut, HistRow row, const mtr_history_args& a, void* stream)
{
	if ((cut != HIST_CALL_END && !a.ends) || a.C < 1 || a.C > MTR_MAX_CHANNELS || (a.FC != a.C && !(a.FC == 6 && a.C == 5))) return -1;
	if (row == HIST_ROW_GONIO && a.HC != 2) return -1;                       // (floats 2 * OS_HALO, 2 * OS_HALO + 1 of a row are the blob header's)
	const auto launch = [&] (auto kernel, int frames) {
		hipLaunchKernelGGL (kernel, dim3 ((a.n_streams * frames + 255) / 256), dim3 (256), 0, (hipStream_t) stream, a);
		return hipGetLastError () == hipSuccess ? 0 : -1;
	};
	if (row == HIST_ROW_GONIO) switch (cut) {
	case HIST_CALL_END:            return launch (k_history<HIST_CALL_END, OS_HALO, OS_HROW>, OS_HALO);
	case HIST_OWN_END:             return launch (k_history<HIST_OWN_END, OS_HALO, OS_HROW>, OS_HALO);
	default: return -1;
	}
	switch (cut) {
	case HIST_CALL_END:            return launch (k_history<HIST_CALL_END, MTR_FIR_HALO, 0>, MTR_FIR_HALO);
	case HIST_CALL_END_IF_TOUCHED: return launch (k_history<HIST_CALL_END_IF_TOUCHED, MTR_FIR_HALO, 0>, MTR_FIR_HALO);
	case HIST_OWN_END:             return launch (k_history<HIST_OWN_END, MTR_FIR_HALO, 0>, MTR_FIR_HALO);
	default: return -1;
	}
}
