// mtr_plan.cpp — the launch planner: which kernels serve a configuration, how a call of N frames is tiled, and whether its whole
// fragments go through the lane = time segment kernel.  Pure arithmetic on a PlanCtx: no device, no HIP call, no engine object — the
// engine's host code fills a PlanCtx per call, mtr_plan_query from a configuration alone.  Built with the flags of the other
// host code: its floating-point decisions (best > t6, the ceils) are part of what a call computes.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "mtr_internal.h"
#include "mtr_host.h"

const char* resolve_layout (const mtr_config* cfg, int* layout, int* run, bool* seg_ok)
{
	const bool fused = cfg->meters & (MTR_METER_EBU | MTR_METER_TRUEPEAK);
	if (cfg->n_channels < 1 || cfg->n_channels > MTR_MAX_ENGINE_CHANNELS || (cfg->n_channels > MTR_MAX_CHANNELS && cfg->meters != MTR_METER_SURROUND))
		return "n_channels must be 1 .. 5 (6 .. 8: MTR_METER_SURROUND alone)";
	if (cfg->n_channels > 2 && fused) {
		// every EBU / TRUEPEAK engine of 3 .. 5 channels runs k_kwmc (layout 8, mtr_kwmc.hip)
		if (cfg->tune_layout != 0 && cfg->tune_layout != 8) return "n_channels 3 .. 5: tune_layout must be 0 or 8 (k_kwmc is the only multichannel kernel)";
		if (cfg->tune_run != 0 && cfg->tune_run != MTR_KWMC_RUN) return "layout 8 runs 20-frame lane runs: tune_run must be 0 or 20";
		if (cfg->tune_prune != 0) return "layout 8 has no peak pruning: tune_prune must be 0";
		if (cfg->tune_fir != 0) return "layout 8 has one interpolator form: tune_fir must be 0";
		*layout = 8; *run = MTR_KWMC_RUN; *seg_ok = false;
		return nullptr;
	}
	if (cfg->tune_layout == 8) return "layout 8 is the multichannel kernel (n_channels 3, 4 or 5 with EBU / TRUEPEAK)";
	if (cfg->tune_run != 0 && cfg->tune_run != 19 && cfg->tune_run != 38 && cfg->tune_run != 39) return "tune_run must be 0, 19, 38 or 39";
	if (cfg->tune_layout != 0 && cfg->tune_layout != 3 && cfg->tune_layout != 4 && cfg->tune_layout != 6 && cfg->tune_layout != 7)
		return "tune_layout must be 0, 3, 4, 6 or 7 (layouts 1, 2 and 5 of earlier versions are gone)";
	if (cfg->tune_fir > 1) return "tune_fir must be 0 or 1";
	const bool kw_only = (cfg->meters & MTR_METER_EBU) && !(cfg->meters & MTR_METER_TRUEPEAK);
	const bool has_tp = cfg->meters & MTR_METER_TRUEPEAK;
	int lay = cfg->tune_layout ? (int) cfg->tune_layout : kw_only ? 4 : (has_tp && (cfg->tune_run == 0 || cfg->tune_run == 38)) ? 7 : 3;
	*seg_ok = lay == 7 && cfg->tune_prune == 0;
	if (lay == 7) lay = 6;
	*layout = lay;
	*run = cfg->tune_run ? (int) cfg->tune_run : (lay == 6 ? 38 : 39);
	if ((lay == 6) != (*run == 38)) return "layouts 6 and 7 run 38-frame lane runs, and only they do";
	if (lay == 6 && !has_tp) return "layouts 6 and 7 are true-peak kernels: need TRUEPEAK";
	if (lay == 4 && !kw_only) return "layout 4 is the EBU-only kernel";
	if (lay == 3 && *run != 39) return "layout 3 needs tune_run 39";
	if (lay == 4 && *run != 39 && *run != 19) return "layout 4 needs tune_run 19 or 39";
	return nullptr;
}

// Does this call go through k_seg?  It must hold at least one whole fragment behind the one it may start in, and it must be
// a BATCH: the kernel's unit of parallelism is a lane, so it needs ~64 x the units of
// k_kwtp16 to fill the chip.  The number of segments per stream is the one that minimises the modelled time — rounds of
// resident waves x steps per wave, a warm-up step (K-filter only) at 0.3 of a full one — and the call takes this path
// when that beats the model of k_kwtp16 (1.2 x the time per frame when both fill the machine, measured: 11.7 vs 9.75 ms,
// profiles/r03*; k_kwtp16's waves are a stream-tile each, so it fills the machine with any batch).
SegPlan seg_plan (const PlanCtx* e, const float* d_audio, uint64_t N)
{
	SegPlan sp;
	const bool ebu = e->cfg.meters & MTR_METER_EBU;
	if (!e->seg_ok || e->layout != 6 || e->cfg.n_channels != 2) return sp;
	if (e->fragm < 4 * MTR_SEG_STEP) return sp;
	if (reinterpret_cast<uintptr_t> (d_audio) & 7) return sp;
	// (a segment may start on any frame — odd strides, 2205-frame fragments, a call that starts inside a fragment: the kernel's
	// loads only assume a frame's 8 bytes.)  The rest of an open fragment in front (`head`) and what is left behind the last whole
	// fragment go to k_kwtp16, in stream order.  A tile that is not a whole number of steps (44.1 / 88.2 kHz) lets a lane read up
	// to 15 frames past its last tile — the next segment's; the lanes of a stream's last segment stop at the frame (mtr_seg.hip).
	const uint64_t head = e->frcnt != e->fragm ? e->frcnt : 0;
	if (head >= N) return sp;
	const uint64_t Nb = N - head;
	const uint64_t tiles = Nb / e->fragm;
	if (tiles == 0 || tiles > 0x7fffffffull / (e->fragm / MTR_SEG_STEP + 1)) return sp;
	sp.head = (uint32_t) head;
	const double spt = (double) e->fragm / MTR_SEG_STEP;
	const uint32_t warm_steps = ebu ? ((uint32_t) std::ceil (MTR_SEG_WARM_SEC * e->cfg.sample_rate / (float) MTR_SEG_STEP) + 3) / 4 * 4 : 0;
	const uint32_t warm_tiles = (warm_steps * MTR_SEG_STEP + e->fragm - 1) / e->fragm;
	const uint64_t S = e->cfg.n_streams;
	uint64_t gmax = ebu ? tiles / (warm_tiles + 2) : tiles;
	if (gmax < 1) gmax = 1;
	if (e->cfg.tune_segments) gmax = std::min<uint64_t> (gmax, e->cfg.tune_segments);
	const uint64_t g0 = e->cfg.tune_segments ? gmax : 1;
	// Candidates: for a given number of tiles per lane n = ceil (tiles / g) the smallest g has the fewest rounds, so only the g
	// at which n changes are evaluated — O (sqrt (tiles)) of them instead of every g up to 65536 (this runs on every process
	// call, in the caller's thread: one stream x one hour cost 0.17 ms here before it was told to take k_kwtp16).
	double best = 0; uint64_t bg = 0;
	for (uint64_t g = g0; g <= gmax && g <= 65536; ) {
		const uint64_t waves = (S * g + 63) / 64, rounds = (waves + e->seg_slots - 1) / e->seg_slots;
		const uint64_t n_main = tiles / g + (tiles % g ? 1 : 0);
		const double t = (double) rounds * ((double) n_main * spt + (g > 1 ? 0.3 * warm_steps : 0.0));
		if (!bg || t < best) { best = t; bg = g; }
		if (n_main <= 1) break;
		g = std::max<uint64_t> (g + 1, (tiles + n_main - 2) / (n_main - 1));      // the smallest g with fewer tiles per lane
	}
	const double t6 = 1.2 * (double) S * (double) tiles * spt / (64.0 * e->seg_slots);
	if (!e->cfg.tune_segments && best > t6) return sp;
	sp.use = true;
	sp.tiles = (uint32_t) tiles; sp.n_segs = (uint32_t) bg;
	sp.base = (uint32_t) (tiles / bg); sp.rem = (uint32_t) (tiles % bg); sp.n_main = sp.base + (sp.rem ? 1 : 0);
	sp.warm_steps = bg > 1 ? warm_steps : 0;
	return sp;
}

// Tiling of a call of N frames that starts with `frcnt` frames left in the open fragment (pure).  body_tiles > 0: behind the
// `head` frames that finish the open fragment (0 if the call starts on a boundary) body_tiles tiles are whole fragments
// (k_seg's part), whatever their length.
const char* plan_tiling (const PlanCtx* e, uint64_t N, uint32_t head, uint32_t body_tiles, Tiling& t)
{
	const uint32_t LT = 64u * (uint32_t) e->run;
	std::vector<uint32_t>& ts = t.ts;
	std::vector<uint32_t>& ft = t.ft;
	ts.clear (); ft.clear ();
	ts.reserve ((size_t) (N / LT + N / e->fragm + 4));
	uint64_t pos = 0;
	uint32_t left = e->frcnt;
	uint32_t head_tiles = 0, body_done = 0;
	ft.push_back (0);
	while (pos < N) {
		const bool body = body_done < body_tiles && pos >= head;
		if (body && body_done == 0) head_tiles = (uint32_t) ts.size ();
		body_done += body;
		const uint32_t piece = body ? e->fragm : (uint32_t) std::min<uint64_t> (std::min<uint64_t> (LT, left), N - pos);
		ts.push_back ((uint32_t) pos);
		pos += piece;
		left -= piece;
		if (left == 0) { ft.push_back ((uint32_t) ts.size ()); left = e->fragm; }
	}
	ts.push_back ((uint32_t) N);
	const uint32_t n_tiles = (uint32_t) ts.size () - 1;
	const uint32_t n_frag  = (uint32_t) ft.size () - 1;      // fragments that end inside this call
	const uint32_t tail    = ft.back ();
	ft.resize ((size_t) n_frag + 1);

	// time segments: enough (stream, segment) waves to fill the chip; each at least 4 warm-up spans long
	const uint32_t warm_tiles = (uint32_t) std::ceil (MTR_WARM_SEC * e->cfg.sample_rate / (float) LT);
	const uint64_t min_seg_frames = (uint64_t) 4 * warm_tiles * LT;
	uint32_t n_segs = e->cfg.tune_segments;
	if (n_segs == 0) {
		// one-wave workgroups (layouts 4-6): eight per CU are resident, 2048 in all — exactly one round of them keeps the
		// warm-up overhead of the segments smallest (one stream x 3600 s: 0.29 ms with 2048 segments, 0.37 with 8192);
		// the four-wave workgroups of layouts 1-3 want more, smaller units
		const uint32_t target_units = e->layout >= 4 ? 2048 : 8192;
		n_segs = (target_units + e->cfg.n_streams - 1) / e->cfg.n_streams;
	}
	const uint64_t max_segs = std::max<uint64_t> (1, N / std::max<uint64_t> (min_seg_frames, 1));
	n_segs = (uint32_t) std::min<uint64_t> (n_segs, max_segs);
	if (body_tiles) n_segs = 1;                                 // k_kwtp16 only starts / finishes such a call: one segment each (head_seg, tail_seg)
	n_segs = std::max<uint32_t> (1, std::min<uint32_t> (n_segs, n_tiles));
	t.sg.assign (n_segs + 1, 0);
	for (uint32_t q = 0; q <= n_segs; ++q) t.sg[q] = (uint32_t) ((uint64_t) q * n_tiles / n_segs);
	for (uint32_t q = 1; q < n_segs; ++q)
		if ((uint64_t) ts[t.sg[q]] < (uint64_t) warm_tiles * LT) return "internal: segment shorter than its warm-up";
	t.n_tiles = n_tiles; t.n_frag = n_frag; t.tail = tail; t.head_tiles = head_tiles; t.n_segs = n_segs; t.frcnt_out = left;
	t.maxlen = n_segs > 1 ? LT : 0;                             // warm-up tiles are full tiles
	for (uint32_t j = 0; j < n_tiles; ++j)
		if (j < head_tiles || j >= head_tiles + body_tiles) t.maxlen = std::max (t.maxlen, ts[j + 1] - ts[j]);
	return nullptr;
}

extern "C" int mtr_plan_query (const mtr_config* cfg, uint32_t frames_left_in_fragment, uint64_t n_frames, uint32_t n_slots, mtr_plan_info* out)
{
	if (!cfg || !out) return fail (MTR_ERR_ARG, "null argument");
	if (cfg->struct_size != sizeof (mtr_config)) return fail (MTR_ERR_ARG, "mtr_plan_query: bad config (struct_size)");
	if (cfg->n_streams == 0 || !(cfg->sample_rate >= 1000.0f) || n_frames == 0 || n_frames > 0xffffffffull) return fail (MTR_ERR_ARG, "mtr_plan_query: streams, rate or frames out of range");
	PlanCtx c;
	c.cfg = *cfg;
	if (const char* why = resolve_layout (cfg, &c.layout, &c.run, &c.seg_ok)) return fail (MTR_ERR_ARG, why);
	c.fragm = (uint32_t) ((int) cfg->sample_rate / 20);
	c.frcnt = frames_left_in_fragment ? frames_left_in_fragment : c.fragm;
	if (c.frcnt > c.fragm) return fail (MTR_ERR_ARG, "mtr_plan_query: more frames left than a fragment has");
	c.seg_slots = n_slots ? n_slots : 1024;
	memset (out, 0, sizeof (*out));
	const bool fused = cfg->meters & (MTR_METER_EBU | MTR_METER_TRUEPEAK);
	out->layout = c.seg_ok ? 7u : (uint32_t) c.layout;
	if (!fused) { out->frames_left_after = c.frcnt; return MTR_OK; }
	const SegPlan sp = seg_plan (&c, nullptr, n_frames);
	Tiling t;
	if (const char* why = plan_tiling (&c, n_frames, sp.use ? sp.head : 0, sp.use ? sp.tiles : 0, t)) return fail (MTR_ERR_ARG, why);
	out->uses_seg = sp.use;
	out->head_frames = sp.use ? sp.head : 0; out->body_fragments = sp.use ? sp.tiles : 0; out->segments = sp.use ? sp.n_segs : 0;
	out->fragments_per_lane = sp.use ? sp.n_main : 0; out->warm_steps = sp.use ? sp.warm_steps : 0;
	out->n_tiles = t.n_tiles; out->head_tiles = t.head_tiles; out->n_fragments_ended = t.n_frag;
	out->kw_segments = sp.use ? 0 : t.n_segs;
	out->frames_left_after = t.frcnt_out;
	return MTR_OK;
}
