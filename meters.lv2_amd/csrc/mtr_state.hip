// mtr_state.hip — per-stream state as a blob: checkpoint / resume, re-sharding (mtr_engine_state_bytes / _export / _import,
// mtr_state_blob_count).  The blob is a header with the engine's lock-step cursors and, per array a stream carries from call to call,
// the streams' entries back to back; which arrays, and what is in them, is the meters' business (their *_sections hooks).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "mtr_engine_impl.h"

namespace {

struct StateHeader {
	uint32_t magic, version, header_bytes;
	uint32_t meters, n_channels;
	float    sample_rate;
	uint32_t count, per_stream_bytes, stream_state_bytes;
	// the engine's lock-step cursors
	uint32_t frcnt, integr;
	float    omega;
	uint64_t dr_scnt;
	uint64_t payload_fnv;       // FNV-1a (64 bit) of everything behind the header: a checkpoint file that rotted is refused, not trusted
};
constexpr uint32_t STATE_MAGIC = 0x5352544du;   // "MTRS"
constexpr uint32_t STATE_VERSION = 2;           // 2: + payload_fnv

uint64_t fnv1a64 (const unsigned char* p, size_t n)
{
	uint64_t h = 0xcbf29ce484222325ull;
	for (size_t i = 0; i < n; ++i) { h ^= p[i]; h *= 0x100000001b3ull; }
	return h;
}

// every array a stream carries from call to call, in the blob's order (a function of the configuration alone): the core's, then the
// side meters' in the order the meters came to the engine
std::vector<StateSection> state_sections (const mtr_engine* e)
{
	std::vector<StateSection> v;
	const uint32_t m = e->cfg.meters;
	v.push_back ({ e->state.p, sizeof (mtr_stream_state) });
	v.push_back ({ e->hist.p, (size_t) 2 * MTR_HIST_LEN * sizeof (int32_t) });
	v.push_back ({ e->fir_hist[e->pos.hist_cur].p, (size_t) MTR_FIR_HALO * 2 * sizeof (float) });
	if (m & MTR_METER_SPECTR30) bank_sections (e, v);
	if (m & (MTR_METER_BITSTATS | MTR_METER_SIGDIST)) intstat_sections (e, v);
	if (m & MTR_METER_DR14) dr14_sections (e, v);
	if (m & MTR_METER_KMETER) kmeter_sections (e, v);
	if (e->layout == 8) {                                      // the per-channel side buffers (stereo blobs are unchanged)
		const size_t C = e->cfg.n_channels;
		v.push_back ({ e->mc_kz.p, C * 4 * sizeof (float) });
		v.push_back ({ e->mc_hist[e->pos.hist_cur].p, (size_t) MTR_FIR_HALO * C * sizeof (float) });
		v.push_back ({ e->mc_tp_last.p, C * sizeof (float) });
		v.push_back ({ e->mc_tp_hold.p, C * sizeof (float) });
	}
	// (the LAST section, and only of an engine with the bit: every other blob is byte for byte what it was.  The header has no room
	// for the period and the frames into the open one: they travel in every stream's entry, stcorr_export_cursors / _import_cursors)
	if (m & MTR_METER_STCORR) stcorr_sections (e, v);
	// (behind it, likewise: kinds, period, cursor and gains in every stream's entry, needle_export_cursors / _import_cursors)
	if (m & MTR_METER_NEEDLE) needle_sections (e, v);
	// (and the surround meter's — never beside those two, which meter one or two channels: period, cursor, _fpp and pairs in every stream's
	// entry, surround_export_cursors / _import_cursors)
	if (m & MTR_METER_SURROUND) surround_sections (e, v);
	// (and the scope's — a stereo meter, so behind STCORR's and NEEDLE's: configuration and cursors in every stream's entry of the first of
	// them, scope_export_cursors / _import_cursors)
	if (m & MTR_METER_SCOPE) scope_sections (e, v);
	return v;
}

// where the entries of section `idx` start in the payload of a blob of `count` streams
size_t section_offset (const std::vector<StateSection>& secs, size_t idx, uint32_t count)
{
	size_t o = 0;
	for (size_t i = 0; i < idx; ++i) o += (size_t) count * secs[i].elem;
	return o;
}

// SCOPE's sections are the last ones, STCORR's and NEEDLE's in front of them, in this order; SURROUND's (3 .. 8 channels: never in their
// engine) is the last one
size_t scope_section (const mtr_engine*, const std::vector<StateSection>& secs) { return secs.size () - scope_n_sections (); }
size_t surround_section (const mtr_engine*, const std::vector<StateSection>& secs) { return secs.size () - 1; }
size_t needle_section (const mtr_engine* e, const std::vector<StateSection>& secs)
{
	return secs.size () - 1 - ((e->cfg.meters & MTR_METER_SCOPE) ? scope_n_sections () : 0);
}
size_t stcorr_section (const mtr_engine* e, const std::vector<StateSection>& secs)
{
	return needle_section (e, secs) - ((e->cfg.meters & MTR_METER_NEEDLE) ? 1 : 0);
}

size_t state_per_stream (const mtr_engine* e)
{
	size_t n = 0;
	for (const StateSection& s : state_sections (e)) n += s.elem;
	return n;
}

}  // namespace
extern "C" {

size_t mtr_engine_state_bytes (const mtr_engine* e, uint32_t count)
{
	if (!e) return 0;
	return sizeof (StateHeader) + (size_t) count * state_per_stream (e);
}

uint32_t mtr_state_blob_count (const void* blob, size_t bytes)
{
	StateHeader h;
	if (!blob || bytes < sizeof (h)) return 0;
	memcpy (&h, blob, sizeof (h));
	if (h.magic != STATE_MAGIC || h.version != STATE_VERSION || h.header_bytes != sizeof (h)) return 0;
	if (bytes < sizeof (h) + (size_t) h.count * h.per_stream_bytes) return 0;
	return h.count;
}

int mtr_engine_state_export (mtr_engine* e, uint32_t first, uint32_t count, void* blob, size_t capacity)
{
	int rc = check_range (e, first, count);
	if (rc) return rc;
	if (!blob) return fail (MTR_ERR_ARG, "mtr_engine_state_export: null blob");
	const size_t need = mtr_engine_state_bytes (e, count);
	if (capacity < need) return fail (MTR_ERR_ARG, "mtr_engine_state_export: capacity < mtr_engine_state_bytes ()");
	rc = mtr_engine_sync (e);
	if (rc) return rc;
	StateHeader h;
	memset (&h, 0, sizeof (h));
	h.magic = STATE_MAGIC; h.version = STATE_VERSION; h.header_bytes = sizeof (h);
	h.meters = e->cfg.meters; h.n_channels = e->cfg.n_channels; h.sample_rate = e->cfg.sample_rate;
	h.count = count; h.per_stream_bytes = (uint32_t) state_per_stream (e); h.stream_state_bytes = sizeof (mtr_stream_state);
	h.frcnt = e->pos.frcnt; h.integr = e->integr ? 1u : 0u; h.omega = e->bank.omega; h.dr_scnt = e->pos.dr_scnt;
	unsigned char* const o0 = static_cast<unsigned char*> (blob) + sizeof (h);
	unsigned char* o = o0;
	const std::vector<StateSection> secs = state_sections (e);
	for (const StateSection& s : secs) {
		if (count) HIPCHK (hipMemcpy (o, static_cast<const unsigned char*> (s.base) + (size_t) first * s.elem, (size_t) count * s.elem, hipMemcpyDeviceToHost));
		o += (size_t) count * s.elem;
	}
	// the host's cursors, not whatever the device copy holds
	if (e->cfg.meters & MTR_METER_STCORR) stcorr_export_cursors (e, o0 + section_offset (secs, stcorr_section (e, secs), count), count);
	if (e->cfg.meters & MTR_METER_NEEDLE) needle_export_cursors (e, o0 + section_offset (secs, needle_section (e, secs), count), count);
	if (e->cfg.meters & MTR_METER_SURROUND) surround_export_cursors (e, o0 + section_offset (secs, surround_section (e, secs), count), count);
	if (e->cfg.meters & MTR_METER_SCOPE) scope_export_cursors (e, o0 + section_offset (secs, scope_section (e, secs), count), count);
	h.payload_fnv = fnv1a64 (o0, (size_t) (o - o0));
	memcpy (blob, &h, sizeof (h));
	return MTR_OK;
}

int mtr_engine_state_import (mtr_engine* e, uint32_t first, const void* blob, size_t bytes)
{
	if (!e || !blob) return fail (MTR_ERR_ARG, "mtr_engine_state_import: null argument");
	StateHeader h;
	if (bytes < sizeof (h)) return fail (MTR_ERR_STATE, "mtr_engine_state_import: not a state blob (too short)");
	memcpy (&h, blob, sizeof (h));
	if (h.magic != STATE_MAGIC) return fail (MTR_ERR_STATE, "mtr_engine_state_import: not a state blob (magic)");
	if (h.version != STATE_VERSION || h.header_bytes != sizeof (h)) return fail (MTR_ERR_STATE, "mtr_engine_state_import: blob of another format version");
	if (h.meters != e->cfg.meters || h.n_channels != e->cfg.n_channels || h.sample_rate != e->cfg.sample_rate)
		return fail (MTR_ERR_STATE, "mtr_engine_state_import: the blob comes from another configuration (meters, channels or sample rate)");
	if (h.stream_state_bytes != sizeof (mtr_stream_state) || h.per_stream_bytes != state_per_stream (e))
		return fail (MTR_ERR_STATE, "mtr_engine_state_import: the blob's per-stream layout is not this build's");
	if (bytes < sizeof (h) + (size_t) h.count * h.per_stream_bytes) return fail (MTR_ERR_STATE, "mtr_engine_state_import: truncated blob");
	int rc = check_range (e, first, h.count);
	if (rc) return rc;
	// the cursors go straight into the tiling of the next call, the payload's ring indices and counters into the kernels:
	// nothing of a blob is trusted before it has been checked
	if (h.frcnt == 0 || h.frcnt > e->fragm) return fail (MTR_ERR_STATE, "mtr_engine_state_import: corrupt blob (frames left in the open fragment)");
	if (h.integr > 1 || !(h.omega > 0.f && h.omega < 1.f)) return fail (MTR_ERR_STATE, "mtr_engine_state_import: corrupt blob (integration flag / bank speed)");
	if (h.dr_scnt > (uint64_t) rintf (e->cfg.sample_rate * 3.0f)) return fail (MTR_ERR_STATE, "mtr_engine_state_import: corrupt blob (open DR-14 window)");
	const unsigned char* const i0 = static_cast<const unsigned char*> (blob) + sizeof (h);
	if (fnv1a64 (i0, (size_t) h.count * h.per_stream_bytes) != h.payload_fnv) return fail (MTR_ERR_STATE, "mtr_engine_state_import: corrupt blob (checksum of the payload)");
	// the streams of an engine advance in lock step: a fresh engine takes the blob's cursors — integration on / off and the bank's
	// speed included, whatever integr_start / spectr_set_speed said before: they are part of where the streams stand — any other
	// must stand at the same ones
	const bool fresh = !e->advanced;
	const std::vector<StateSection> secs = state_sections (e);
	uint32_t sc_period = e->sc.period, sc_fill = (uint32_t) e->pos.sc_fill;
	if ((e->cfg.meters & MTR_METER_STCORR) && h.count) {
		rc = stcorr_import_cursors (e, i0 + section_offset (secs, stcorr_section (e, secs), h.count), h.count, fresh, &sc_period, &sc_fill);
		if (rc) return rc;
	}
	std::vector<unsigned char> nd_hdr (needle_hdr_bytes ());
	const bool nd_take = (e->cfg.meters & MTR_METER_NEEDLE) && h.count;
	if (nd_take) {
		rc = needle_import_cursors (e, i0 + section_offset (secs, needle_section (e, secs), h.count), h.count, fresh, reinterpret_cast<mtr_needle_hdr*> (nd_hdr.data ()));
		if (rc) return rc;
	}
	std::vector<unsigned char> su_hdr (surround_hdr_bytes ());
	const bool su_take = (e->cfg.meters & MTR_METER_SURROUND) && h.count;
	if (su_take) {
		rc = surround_import_cursors (e, i0 + section_offset (secs, surround_section (e, secs), h.count), h.count, fresh, su_hdr.data ());
		if (rc) return rc;
	}
	uint32_t sp_fill = e->pos.sp_fill;
	uint64_t sp_analyses = e->pos.sp_analyses;
	if ((e->cfg.meters & MTR_METER_SCOPE) && h.count) {
		rc = scope_import_cursors (e, i0 + section_offset (secs, scope_section (e, secs), h.count), h.count, fresh, &sp_fill, &sp_analyses);
		if (rc) return rc;
	}
	if (!fresh && (e->pos.frcnt != h.frcnt || e->integr != (h.integr != 0) || e->bank.omega != h.omega || e->pos.dr_scnt != h.dr_scnt))
		return fail (MTR_ERR_STATE, "mtr_engine_state_import: the engine does not stand where the blob's streams do (fragment phase, integration, bank speed or DR-14 window)");
	rc = mtr_engine_sync (e);
	if (rc) return rc;
	e->snap_valid = false;
	const unsigned char* i = i0;
	for (const StateSection& s : secs) {
		if (h.count) HIPCHK (hipMemcpy (const_cast<unsigned char*> (static_cast<const unsigned char*> (s.base)) + (size_t) first * s.elem, i, (size_t) h.count * s.elem, hipMemcpyHostToDevice));
		i += (size_t) h.count * s.elem;
	}
	for (uint32_t k = 0; k < h.count; ++k) {                     // (an imported stream is open — closure is not part of the blob — and
		if (e->closed[first + k]) { e->closed[first + k] = 0; e->n_closed--; }   // its count starts again: the blob does not carry one)
		e->metered[first + k] = 0;
	}
	if (fresh) {                                                 // (only now: a failed sync or copy has not moved the engine)
		e->pos.frcnt = h.frcnt; e->integr = h.integr != 0; e->bank.omega = h.omega; e->pos.dr_scnt = h.dr_scnt;
		e->sc.period = sc_period; e->pos.sc_fill = sc_fill;
		if (nd_take) needle_take_cursors (e, reinterpret_cast<const mtr_needle_hdr*> (nd_hdr.data ()));
		if (su_take) surround_take_cursors (e, su_hdr.data ());
		e->pos.sp_fill = sp_fill; e->pos.sp_analyses = sp_analyses;
		e->plan.valid = false;
		e->advanced = true;
	}
	return MTR_OK;
}

} // extern "C"
