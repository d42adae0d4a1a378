// mtr_integlog.hip — the host side of the integration log (include/mtr_integlog.h): integrated loudness and loudness range over time, a
// point (integrated, integ_thr, range_min, range_max, range_thr) per K evaluations and stream.  An evaluation is what
// Ebu_r128_proc::process does whenever _div2 wraps while the integration runs (ebumeter/ebu_r128_proc.cc:236-242); the points are
// written by the gate, which then evaluates at every recorded wrap and not only at a call's last (the EVAL instantiations of k_gate,
// mtr_gate.hip).  Here are the memory, the gate's arguments and the getters.
//
// Unlike the loudness log there is no host-side cursor: how many evaluations a stream has made follows from its _div2, which is device
// state — the state blob carries it, a call with lengths freezes it, mtr_engine_integr_reset zeroes it, and a deferred gate runs a call
// late.  So the count lives in device memory next to the series, the stream's workgroup advances it, and the series getter copies the
// counts it needs; chunked host calls, every lengths family and both tail modes come out right with nothing of their own.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "mtr_engine_impl.h"

constexpr uint32_t INTEGLOG_MAX_EVERY = 1u << 20;

bool integlog_args (const mtr_engine* e, uint32_t off, mtr_integlog_args* out)
{
	const mtr_engine::IntegLog& l = e->il;
	if (!l.every) return false;
	out->v = l.v.p + (size_t) off * l.cap;
	out->field_pitch = (uint64_t) e->cfg.n_streams * l.cap;
	out->count = l.count.p + off;
	out->every = l.every;
	out->cap = l.cap;
	return true;
}

// the counts to zero (a point is only read once it has been counted: the series needs no clearing); queued on `st` behind whatever the
// side stream holds
int integlog_reset (mtr_engine* e, hipStream_t st)
{
	mtr_engine::IntegLog& l = e->il;
	{ const int jrc = join_tail (e, st); if (jrc) return jrc; }       // (a deferred gate may still be appending)
	e->queued = true;
	HIPCHK (hipMemsetAsync (l.count.p, 0, (size_t) e->cfg.n_streams * sizeof (uint32_t), st));
	return MTR_OK;
}

static void integlog_off (mtr_engine* e)
{
	mtr_engine::IntegLog& l = e->il;
	l.v.drop (); l.count.drop ();
	l.every = 0; l.cap = 0;
}

// how many evaluations and points `n_fragments` integrating fragments add to a stream that stands at (div2, evaluations)
static void integlog_cut (uint32_t div2, uint64_t evaluations, uint32_t every, uint64_t n_fragments, uint64_t* ev_out, uint64_t* pt_out)
{
	const uint64_t ev = (div2 + n_fragments) / 10;                    // _div2 wraps at every tenth fragment
	*ev_out = ev;
	*pt_out = every ? (evaluations + ev) / every - evaluations / every : 0;
}

extern "C" {

int mtr_engine_integlog_set_every (mtr_engine* e, uint32_t every_evaluations, uint32_t capacity_points)
{
	if (!e) return fail (MTR_ERR_ARG, "null engine");
	if (!(e->cfg.meters & MTR_METER_EBU)) return fail (MTR_ERR_ARG, "mtr_engine_integlog_set_every: the log is a setting of an engine that has MTR_METER_EBU");
	if (every_evaluations > INTEGLOG_MAX_EVERY) return fail (MTR_ERR_ARG, "mtr_engine_integlog_set_every: a point is at most every 2^20 evaluations");
	if (e->advanced) return fail (MTR_ERR_STATE, "mtr_engine_integlog_set_every: only on an engine that has processed nothing since create / reset");
	HIPCHK (hipSetDevice (e->cfg.device));
	{ const int rc = sync_all (e); if (rc) return rc; }               // (memory is about to be freed: a reset may still be clearing it)
	integlog_off (e);
	if (!every_evaluations) return MTR_OK;
	mtr_engine::IntegLog& l = e->il;
	const uint64_t S = e->cfg.n_streams, n = S * capacity_points;      // (both below 2^32: the product fits)
	if (n > SIZE_MAX / (MTR_INTEGLOG_FIELDS * sizeof (float))) return fail (MTR_ERR_NOMEM, "mtr_engine_integlog_set_every: 5 * n_streams * capacity_points floats do not fit a size_t");
	if (l.v.reserve ((size_t) n * MTR_INTEGLOG_FIELDS) || l.count.reserve ((size_t) S)) {
		(void) hipGetLastError ();
		integlog_off (e);
		return fail (MTR_ERR_NOMEM, "hipMalloc integration log");
	}
	l.every = every_evaluations; l.cap = capacity_points;
	const int rc = integlog_reset (e, e->last_stream);
	if (rc) integlog_off (e);
	return rc;
}

int mtr_engine_integlog_every (const mtr_engine* e, uint32_t* every_evaluations, uint32_t* capacity_points)
{
	if (!e) return fail (MTR_ERR_ARG, "null engine");
	if (every_evaluations) *every_evaluations = e->il.every;
	if (capacity_points) *capacity_points = e->il.cap;
	return MTR_OK;
}

int mtr_engine_integlog_series (mtr_engine* e, uint32_t first, uint32_t count, float* integrated, float* integ_thr, float* range_min, float* range_max, float* range_thr,
                                uint32_t capacity, uint32_t* n_points, uint32_t* dropped)
{
	int rc = check_range (e, first, count);
	if (rc) return rc;
	const mtr_engine::IntegLog& l = e->il;
	if (!l.every) return fail (MTR_ERR_ARG, "mtr_engine_integlog_series: the log is off (mtr_engine_integlog_set_every)");
	HIPCHK (hipSetDevice (e->cfg.device));
	if ((rc = sync_all (e))) return rc;
	std::vector<uint32_t> ev (count);
	if (count) HIPCHK (hipMemcpy (ev.data (), l.count.p + first, (size_t) count * sizeof (uint32_t), hipMemcpyDeviceToHost));
	size_t width = 0;                                                  // the longest row to fetch
	for (uint32_t i = 0; i < count; ++i) {
		const uint32_t n = ev[i] / l.every, kept = std::min (n, l.cap);
		if (n_points) n_points[i] = n;
		if (dropped) dropped[i] = n - kept;
		ev[i] = std::min (kept, capacity);                             // (from here on: the points of the row to hand out)
		width = std::max (width, (size_t) ev[i]);
	}
	float* const dst[MTR_INTEGLOG_FIELDS] = { integrated, integ_thr, range_min, range_max, range_thr };
	if (!width) return MTR_OK;
	std::vector<float> h ((size_t) count * width);
	for (int k = 0; k < MTR_INTEGLOG_FIELDS; ++k) {
		if (!dst[k]) continue;
		const float* const src = l.v.p + ((size_t) k * e->cfg.n_streams + first) * l.cap;
		HIPCHK (hipMemcpy2D (h.data (), width * sizeof (float), src, (size_t) l.cap * sizeof (float), width * sizeof (float), count, hipMemcpyDeviceToHost));
		for (uint32_t i = 0; i < count; ++i) std::copy_n (h.data () + (size_t) i * width, ev[i], dst[k] + (size_t) i * capacity);
	}
	return MTR_OK;
}

int mtr_engine_integlog_reset (mtr_engine* e)
{
	if (!e) return fail (MTR_ERR_ARG, "null engine");
	if (!e->il.every) return MTR_OK;
	e->snap_valid = false;
	HIPCHK (hipSetDevice (e->cfg.device));
	return integlog_reset (e, e->last_stream);
}

int mtr_integlog_cut (uint32_t div2, uint64_t evaluations_so_far, uint32_t every_evaluations, uint64_t n_fragments, uint64_t* evaluations_out, uint64_t* points_out)
{
	if (!evaluations_out || !points_out) return fail (MTR_ERR_ARG, "mtr_integlog_cut: null argument");
	if (div2 > 9) return fail (MTR_ERR_ARG, "mtr_integlog_cut: div2 is 0 .. 9");
	if (every_evaluations > INTEGLOG_MAX_EVERY) return fail (MTR_ERR_ARG, "mtr_integlog_cut: a point is at most every 2^20 evaluations");
	if (n_fragments > UINT64_MAX - 9 || (div2 + n_fragments) / 10 > UINT64_MAX - evaluations_so_far)
		return fail (MTR_ERR_ARG, "mtr_integlog_cut: the evaluations do not fit 64 bits");
	integlog_cut (div2, evaluations_so_far, every_evaluations, n_fragments, evaluations_out, points_out);
	return MTR_OK;
}

} // extern "C"
