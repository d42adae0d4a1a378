// mtr_host.h — what ALL the host-side TUs of libmtr_engine.so share, the planner (mtr_plan.cpp) and the communicator (mtr_comm.hip)
// included: the error path, the planner's interface, the communicator's.  No HIP header here: the planner is built without one.  What
// needs one — the engine itself, a call — is in mtr_engine_impl.h.
#ifndef MTR_HOST_H
#define MTR_HOST_H

#include <cstdint>
#include <vector>

#include "mtr_engine.h"

#pragma GCC visibility push(hidden)   // (cross-TU helpers, not ABI)

// sets what mtr_last_error () returns (per thread) and returns `code`; `hip_error` != 0: a hipError_t whose text is appended (mtr_engine.hip)
int fail (int code, const char* what, int hip_error = 0);

#define HIPCHK(call) do { hipError_t he_ = (call); if (he_ != hipSuccess) return fail (MTR_ERR_HIP, #call, he_); } while (0)

// ---- the planner (mtr_plan.cpp): pure, no device, no engine --------------------------------------------------------------
// everything the planning needs from an engine: mtr_plan_query builds one from a configuration alone, without a device
struct PlanCtx {
	mtr_config cfg;
	bool       seg_ok;
	int        layout, run;
	uint32_t   fragm, frcnt, seg_slots;
};

// The lane = time segment kernel's share of a call (mtr_seg.hip, layout 7): `tiles` whole fragments from frame 0, cut into
// n_segs segments per stream of base (+ 1 for the first rem) tiles; every lane walks n_main of them.
struct SegPlan {
	bool     use = false;
	uint32_t head = 0;          // frames of the call in front of the first whole fragment (the rest of the open one)
	uint32_t tiles = 0, n_segs = 0, base = 0, rem = 0, n_main = 0, warm_steps = 0;
};

// Tiling of a call of N frames that starts with `frcnt` frames left in the open fragment (pure).  body_tiles > 0: behind the
// `head` frames that finish the open fragment (0 if the call starts on a boundary) body_tiles tiles are whole fragments
// (k_seg's part), whatever their length.
struct Tiling {
	std::vector<uint32_t> ts, ft, sg;       // tile starts (+ N), first tile of every fragment that ends in the call, segment starts
	uint32_t n_tiles = 0, n_frag = 0, tail = 0, head_tiles = 0, n_segs = 0, frcnt_out = 0, maxlen = 0;
};

// Which kernels serve a configuration (mtr_engine_create and mtr_plan_query share it).  Returns what is wrong with it, or NULL.
const char* resolve_layout (const mtr_config* cfg, int* layout, int* run, bool* seg_ok);
SegPlan     seg_plan (const PlanCtx* e, const float* d_audio, uint64_t N);
const char* plan_tiling (const PlanCtx* e, uint64_t N, uint32_t head, uint32_t body_tiles, Tiling& t);

// ---- the communicator (mtr_comm.hip): RCCL behind the C ABI ----------------------------------------------------------------
// mtr_engine_reduce's checks of its communicator: alive, and on the engine's device
int comm_check (const mtr_comm* c, int device);
// the job's one collective: the sum of the histograms and the max of the peaks as ONE group on `stream`, polled to the communicator's deadline
int comm_all_reduce (mtr_comm* c, int32_t* d_hist, float* d_max, void* stream);
#pragma GCC visibility pop

#endif
