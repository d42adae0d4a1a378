// mtr_loudlog.hip — the host side of the loudness log (include/mtr_loudlog.h): momentary / short-term loudness over time, a (M, S) point
// per period of P fragments and stream.  The points are written by the gate, which computes M and S of every fragment anyway (the LOG
// instantiations of mtr_gate.hip); here are the memory, the cursor arithmetic the gate's arguments come from, and the getters.
//
// The cursor (Cursors::ll_frags: fragments the open streams have ended since the log was set or reset) moves with the other lock-step
// cursors, behind a call's last launch; a chunk of a host call writes the rows of its own streams from the same cursor.  The
// arguments of a gate are computed when it is queued, so a deferred gate — it runs beside the fused kernel of the next call, behind the
// gates before it on the side stream — appends where its own call stands.  Streams end at their own lengths: the points a stream has
// completed are counted per stream, on the host (CallRun::run, next to the frames it has metered).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "mtr_engine_impl.h"

constexpr uint32_t LOUDLOG_MAX_PERIOD = 1u << 20;

bool loudlog_args (const mtr_engine* e, const Cursors& pos, uint32_t off, mtr_loudlog_args* out)
{
	const mtr_engine::LoudLog& l = e->ll;
	if (!l.period) return false;
	const uint64_t done = pos.ll_frags / l.period;
	out->M = l.M.p + (size_t) off * l.cap;
	out->S = l.S.p + (size_t) off * l.cap;
	out->run = l.run.p + (size_t) off * 2;
	out->run_new = l.run_new.p + (size_t) off * 2;
	out->period = l.period;
	out->phase = (uint32_t) (pos.ll_frags % l.period);
	out->cap = l.cap;
	out->point0 = (uint32_t) std::min<uint64_t> (done, l.cap);
	out->room = l.cap - out->point0;
	out->mode = l.mode;
	return true;
}

// series and running maxima to "no fragment yet", counts and phase to zero; queued on `st` behind whatever the side stream holds
int loudlog_reset (mtr_engine* e, hipStream_t st)
{
	mtr_engine::LoudLog& l = e->ll;
	const size_t S = e->cfg.n_streams;
	{ const int jrc = join_tail (e, st); if (jrc) return jrc; }       // (a deferred gate may still be appending)
	e->queued = true;
	// (-inf as a sortable int: what the multi-workgroup gate's atomicMax starts from; a point is only read once it has been written)
	if (l.M.n) HIPCHK (hipMemsetD32Async ((hipDeviceptr_t) l.M.p, MTR_LOUDLOG_EMPTY, l.M.n, st));
	if (l.S.n) HIPCHK (hipMemsetD32Async ((hipDeviceptr_t) l.S.p, MTR_LOUDLOG_EMPTY, l.S.n, st));
	HIPCHK (hipMemsetD32Async ((hipDeviceptr_t) l.run.p, (int) 0xff800000, 2 * S, st));        // -inf
	HIPCHK (hipMemsetD32Async ((hipDeviceptr_t) l.run_new.p, MTR_LOUDLOG_EMPTY, 2 * S, st));
	l.points.assign (S, 0);
	e->pos.ll_frags = 0;
	return MTR_OK;
}

static void loudlog_off (mtr_engine* e)
{
	mtr_engine::LoudLog& l = e->ll;
	l.M.drop (); l.S.drop (); l.run.drop (); l.run_new.drop ();
	l.period = 0; l.cap = 0; l.mode = 0;
	l.points.clear ();
	e->pos.ll_frags = 0;
}

extern "C" {

int mtr_engine_loudlog_set_period (mtr_engine* e, uint32_t period_fragments, uint32_t capacity_points, int mode)
{
	if (!e) return fail (MTR_ERR_ARG, "null engine");
	if (!(e->cfg.meters & MTR_METER_EBU)) return fail (MTR_ERR_ARG, "mtr_engine_loudlog_set_period: the log is a setting of an engine that has MTR_METER_EBU");
	if (period_fragments > LOUDLOG_MAX_PERIOD) return fail (MTR_ERR_ARG, "mtr_engine_loudlog_set_period: a period is at most 2^20 fragments");
	if (mode != MTR_LOUDLOG_SAMPLE && mode != MTR_LOUDLOG_MAX) return fail (MTR_ERR_ARG, "mtr_engine_loudlog_set_period: mode is MTR_LOUDLOG_SAMPLE or MTR_LOUDLOG_MAX");
	if (e->advanced) return fail (MTR_ERR_STATE, "mtr_engine_loudlog_set_period: only on an engine that has processed nothing since create / reset");
	HIPCHK (hipSetDevice (e->cfg.device));
	{ const int rc = sync_all (e); if (rc) return rc; }               // (memory is about to be freed: a reset may still be clearing it)
	loudlog_off (e);
	if (!period_fragments) return MTR_OK;
	mtr_engine::LoudLog& l = e->ll;
	const uint64_t S = e->cfg.n_streams, n = S * capacity_points;      // (both below 2^32: the product fits)
	if (n > SIZE_MAX / sizeof (float)) return fail (MTR_ERR_NOMEM, "mtr_engine_loudlog_set_period: n_streams * capacity_points floats do not fit a size_t");
	if (l.M.reserve ((size_t) n) || l.S.reserve ((size_t) n) || l.run.reserve ((size_t) S * 2) || l.run_new.reserve ((size_t) S * 2)) {
		(void) hipGetLastError ();
		loudlog_off (e);
		return fail (MTR_ERR_NOMEM, "hipMalloc loudness log");
	}
	l.period = period_fragments; l.cap = capacity_points; l.mode = mode;
	const int rc = loudlog_reset (e, e->last_stream);
	if (rc) loudlog_off (e);
	return rc;
}

int mtr_engine_loudlog_period (const mtr_engine* e, uint32_t* period_fragments, uint32_t* capacity_points, int* mode)
{
	if (!e) return fail (MTR_ERR_ARG, "null engine");
	if (period_fragments) *period_fragments = e->ll.period;
	if (capacity_points) *capacity_points = e->ll.cap;
	if (mode) *mode = e->ll.mode;
	return MTR_OK;
}

int mtr_engine_loudlog_series (mtr_engine* e, uint32_t first, uint32_t count, float* M, float* S, uint32_t capacity, uint32_t* n_points, uint32_t* dropped)
{
	int rc = check_range (e, first, count);
	if (rc) return rc;
	const mtr_engine::LoudLog& l = e->ll;
	if (!l.period) return fail (MTR_ERR_ARG, "mtr_engine_loudlog_series: the log is off (mtr_engine_loudlog_set_period)");
	size_t width = 0;                                                  // the longest row to fetch
	for (uint32_t i = 0; i < count; ++i) {
		const uint64_t n = l.points[first + i], kept = std::min<uint64_t> (n, l.cap);
		if (n_points) n_points[i] = (uint32_t) std::min<uint64_t> (n, 0xFFFFFFFFull);
		if (dropped) dropped[i] = (uint32_t) std::min<uint64_t> (n - kept, 0xFFFFFFFFull);
		width = std::max (width, (size_t) std::min<uint64_t> (kept, capacity));
	}
	HIPCHK (hipSetDevice (e->cfg.device));
	if ((rc = sync_all (e))) return rc;
	if ((!M && !S) || !width) return MTR_OK;
	std::vector<float> h ((size_t) count * width);
	const float* const src[2] = { l.M.p, l.S.p };
	float* const dst[2] = { M, S };
	for (int k = 0; k < 2; ++k) {
		if (!dst[k]) continue;
		HIPCHK (hipMemcpy2D (h.data (), width * sizeof (float), src[k] + (size_t) first * l.cap, (size_t) l.cap * sizeof (float),
		                     width * sizeof (float), count, hipMemcpyDeviceToHost));
		for (uint32_t i = 0; i < count; ++i) {
			const size_t take = (size_t) std::min<uint64_t> (std::min<uint64_t> (l.points[first + i], l.cap), capacity);
			std::copy_n (h.data () + (size_t) i * width, take, dst[k] + (size_t) i * capacity);
		}
	}
	return MTR_OK;
}

int mtr_engine_loudlog_reset (mtr_engine* e)
{
	if (!e) return fail (MTR_ERR_ARG, "null engine");
	if (!e->ll.period) return MTR_OK;
	e->snap_valid = false;
	HIPCHK (hipSetDevice (e->cfg.device));
	return loudlog_reset (e, e->last_stream);
}

} // extern "C"
