// mtr_state.hip — per-stream state as a blob: checkpoint / resume, re-sharding (mtr_engine_state_bytes / _export / _import,
// mtr_state_blob_count).  The blob is a header with the engine's lock-step cursors and, per array a stream carries from call to call,
// the streams' entries back to back; which arrays, and what is in them, is the meters' business (the sections hook of their rows in
// SIDE_METERS), as is the meaning of the configuration and cursors that some of them keep in their entries (the rows' BlobHeader).
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

constexpr size_t N_SIDE = sizeof (SIDE_METERS) / sizeof (SIDE_METERS[0]);

// every array a stream carries from call to call, in the blob's order (a function of the configuration alone): the core's, then the
// side meters' in the order of SIDE_METERS — with the core's per-channel arrays of layout 8, which came to the blob before STCORR did,
// in front of STCORR's.  first[i]: the index of the first section of side meter i, if the engine has it; NO_SECTION: the row pushed
// none in this engine (KMETER's second row without a period), wherever the row stands in the table.
constexpr size_t NO_SECTION = ~(size_t) 0;
std::vector<StateSection> state_sections (const mtr_engine* e, size_t* first = nullptr)
{
	std::vector<StateSection> v;
	v.push_back ({ e->state.p, sizeof (mtr_stream_state) });
	v.push_back ({ e->hist.p, (size_t) 2 * MTR_HIST_LEN * sizeof (int32_t) });
	v.push_back ({ e->fir_hist[e->pos.hist_cur].p, (size_t) MTR_FIR_HALO * 2 * sizeof (float) });
	for (size_t i = 0; i < N_SIDE; ++i) {
		if (SIDE_METERS[i] == &stcorr_meter && e->layout == 8) {   // the per-channel side buffers (stereo blobs are unchanged)
			const size_t C = e->cfg.n_channels;
			v.push_back ({ e->mc_kz.p, C * 4 * sizeof (float) });
			v.push_back ({ e->mc_hist[e->pos.hist_cur].p, (size_t) MTR_FIR_HALO * C * sizeof (float) });
			v.push_back ({ e->mc_tp_last.p, C * sizeof (float) });
			v.push_back ({ e->mc_tp_hold.p, C * sizeof (float) });
		}
		if (!(e->cfg.meters & SIDE_METERS[i]->bits)) continue;
		const size_t n0 = v.size ();
		SIDE_METERS[i]->sections (e, v);
		if (first) first[i] = v.size () > n0 ? n0 : NO_SECTION;
	}
	return v;
}

// The host-owned headers of the side meters in a payload of `count` streams: where the first stream's header of meter i is, and the
// pitch from one stream's to the next (null: the engine has no such meter, or the meter no header)
struct HeaderAt { unsigned char* p; size_t pitch; };
HeaderAt header_at (const mtr_engine* e, const std::vector<StateSection>& secs, const size_t* first, size_t i, uint32_t count, const unsigned char* payload)
{
	const BlobHeader* const hd = SIDE_METERS[i]->hdr;
	if (!hd || !(e->cfg.meters & SIDE_METERS[i]->bits)) return { nullptr, 0 };
	if (first[i] == NO_SECTION) return { nullptr, 0 };             // (a header lives in the row's first section: no section, no header)
	size_t o = hd->offset;
	for (size_t k = 0; k < first[i]; ++k) o += (size_t) count * secs[k].elem;
	return { const_cast<unsigned char*> (payload) + o, secs[first[i]].elem };
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
	size_t sec0[N_SIDE] = {};
	const std::vector<StateSection> secs = state_sections (e, sec0);
	for (const StateSection& s : secs) {
		if (count) HIPCHK (hipMemcpy (o, static_cast<const unsigned char*> (s.base) + (size_t) first * s.elem, (size_t) count * s.elem, hipMemcpyDeviceToHost));
		o += (size_t) count * s.elem;
	}
	// the side meters' headers: the host's copies, not whatever the device's entries hold
	std::vector<unsigned char> hb;
	for (size_t i = 0; i < N_SIDE; ++i) {
		const HeaderAt at = header_at (e, secs, sec0, i, count, o0);
		if (!at.p) continue;
		hb.assign (SIDE_METERS[i]->hdr->bytes, 0);
		SIDE_METERS[i]->hdr->write (e, hb.data ());
		for (uint32_t k = 0; k < count; ++k) memcpy (at.p + (size_t) k * at.pitch, hb.data (), hb.size ());
	}
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
	size_t sec0[N_SIDE] = {};
	const std::vector<StateSection> secs = state_sections (e, sec0);
	// the side meters' headers, in the order of SIDE_METERS: every stream's equals the first's, and that one is one the engine can take
	std::vector<unsigned char> staged[N_SIDE];
	for (size_t i = 0; i < N_SIDE && h.count; ++i) {
		const HeaderAt at = header_at (e, secs, sec0, i, h.count, i0);
		if (!at.p) continue;
		const BlobHeader* const hd = SIDE_METERS[i]->hdr;
		staged[i].assign (at.p, at.p + hd->bytes);
		if (!blob_headers_agree (at.p, at.pitch, hd->bytes, h.count)) return fail (MTR_ERR_STATE, hd->corrupt);
		rc = hd->check (e, staged[i].data (), fresh);
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
		for (size_t i = 0; i < N_SIDE; ++i)
			if (!staged[i].empty ()) SIDE_METERS[i]->hdr->take (e, staged[i].data ());
		e->plan.valid = false;
		e->advanced = true;
	}
	// (... and an imported stream stands where the open streams do, a fresh engine's at the cursors it just took: its own counts — the
	// points of its series, what the meters' count hooks keep — are the lock-step numbers)
	for (uint32_t k = 0; k < h.count; ++k) stream_counts (e, first + k, nullptr, 0);
	return MTR_OK;
}

} // extern "C"
