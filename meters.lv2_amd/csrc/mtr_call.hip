// mtr_call.hip — one process call: every process entry point of the C ABI (device or host memory, f32 or integer PCM, frame layouts,
// per-stream lengths and track lengths, the LV2 block path) ends in process_call, which turns the call into a tiling plan (mtr_plan.cpp: tiles never
// cross 50 ms fragment boundaries; time segments give the fused kernel enough independent waves when the batch is small) and queues
// the kernels on the caller's stream, in the order CallRun::run spells out.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <iterator>
#include <vector>

#include "mtr_engine_impl.h"

constexpr uint32_t TAIL_AUTO_STREAMS = 4096;       // ... and streams per call
constexpr uint64_t TAIL_AUTO_FRAMES = 1ull << 24;   // stream-frames per call (134 MB of stereo f32: ~40 us of the fused kernel) from which the tail is deferred

static PlanCtx plan_ctx (const mtr_engine* e)
{
	return { e->cfg, e->seg_ok, e->layout, e->run, e->fragm, e->pos.frcnt, e->seg_slots };
}

// A launch behind build_plan's upload failed: the slot stays busy until the stream has passed this point, the plan is not reused.
static void plan_abort (mtr_engine* e, hipStream_t st)
{
	PlanSlot& ps = e->plan_slot[e->plan_cur];
	if (ps.done.v && hipEventRecord (ps.done.v, st) == hipSuccess) ps.pending = true;
	e->plan.valid = false;
}

// The plan of a call on the device: its tiling (mtr_plan.cpp) in the next slot of the plan ring.
static int build_plan (mtr_engine* e, uint64_t N, uint32_t head, uint32_t body_tiles, hipStream_t st)
{
	Plan& pl = e->plan;
	if (pl.valid && pl.n_frames == N && pl.frcnt_in == e->pos.frcnt && pl.body_tiles == body_tiles) return MTR_OK;
	pl.valid = false;
	const PlanCtx ctx = plan_ctx (e);
	Tiling til;
	if (const char* why = plan_tiling (&ctx, N, head, body_tiles, til)) return fail (MTR_ERR_ARG, why);
	const std::vector<uint32_t>& ts = til.ts;
	const std::vector<uint32_t>& ft = til.ft;
	const std::vector<uint32_t>& sg = til.sg;
	const uint32_t n_tiles = til.n_tiles, n_frag = til.n_frag, tail = til.tail, head_tiles = til.head_tiles, n_segs = til.n_segs, left = til.frcnt_out;

	// (with head-room: an LV2 host's blocks see a fragment end in some calls and none in others, and a buffer that grows
	// by one word then is a hipMalloc — 0.3 ms — in the audio thread)
	// (a buffer that grows is freed first, and hipFree waits for the device: no deferred gate still reads it)
	if (e->tile_power[0].reserve ((size_t) e->cfg.n_streams * std::max<uint32_t> (n_tiles, 16))
	    || e->tile_power[1].reserve ((size_t) e->cfg.n_streams * std::max<uint32_t> (n_tiles, 16))
	    || e->frag_power.reserve ((size_t) e->cfg.n_streams * std::max<uint32_t> (n_frag, 16)))
		return fail (MTR_ERR_NOMEM, "hipMalloc plan buffers");
	// the next slot of the ring; its previous contents were last read PLAN_SLOTS plans ago
	const int slot = (e->plan_cur + 1) % PLAN_SLOTS;
	PlanSlot& ps = e->plan_slot[slot];
	if (ps.pending) { HIPCHK (hipEventSynchronize (ps.done.v)); ps.pending = false; }
	const uint32_t tseg[4] = { 0, head_tiles, head_tiles + body_tiles, n_tiles };
	const size_t words = ts.size () + sg.size () + ft.size () + 4;
	if (ps.dev.reserve (std::max<size_t> (words, 256)) || ps.pin.reserve (std::max<size_t> (words, 256))) return fail (MTR_ERR_NOMEM, "plan slot");
	HIPCHK (ps.done.ensure ());
	memcpy (ps.pin.p, ts.data (), ts.size () * 4);
	memcpy (ps.pin.p + ts.size (), sg.data (), sg.size () * 4);
	memcpy (ps.pin.p + ts.size () + sg.size (), ft.data (), ft.size () * 4);
	memcpy (ps.pin.p + ts.size () + sg.size () + ft.size (), tseg, 16);
	HIPCHK (hipMemcpyAsync (ps.dev.p, ps.pin.p, words * 4, hipMemcpyHostToDevice, st));
	// (the slot is busy from here on: its `done` event is recorded behind the plan's last reader, k_gate — or by plan_abort ()
	// if a launch behind this copy fails, so that the slot is never handed out again under a pending upload: ADVICE r2.
	// One hipEventRecord per call, not two: it is 2-3 us of an LV2 run ().)
	e->plan_cur = slot;
	e->tile_start = ps.dev.p; e->seg_tile = ps.dev.p + ts.size (); e->frag_tile = ps.dev.p + ts.size () + sg.size ();
	e->head_seg = e->frag_tile + ft.size ();
	e->tail_seg = e->head_seg + 2;

	pl.frag_end.resize (n_frag);
	for (uint32_t f = 0; f < n_frag; ++f) pl.frag_end[f] = ts[ft[f + 1]];
	pl.n_frames = N; pl.frcnt_in = e->pos.frcnt; pl.frcnt_out = left;
	pl.n_tiles = n_tiles; pl.n_frag = n_frag; pl.n_segs = n_segs; pl.tail_tile = tail; pl.body_tiles = body_tiles; pl.head_tiles = head_tiles;
	const uint32_t maxlen = til.maxlen;
	// + look-ahead frames of the FIR register tile + 4 slots for the carried K-filter state (layout 3)
	pl.buf_slots = (maxlen + 48 + 13 + 4 + 127) / 128 * 128;
	pl.kw_slots = (maxlen + 1 + 127) / 128 * 128;               // k_kw: the tile + one frame of alignment slack
	pl.valid = true;
	return MTR_OK;
}

static hipEvent_t next_event (std::vector<Event>& ev, size_t idx)
{
	while (ev.size () <= idx) {
		Event v;
		if (v.ensure (hipEventDefault) != hipSuccess) return nullptr;
		ev.push_back (std::move (v));
	}
	return ev[idx].v;
}

// Where a call goes (pure apart from reading the engine)
struct Route {
	bool    ragged = false;       // per-stream lengths: the LEN instantiations of the kernels (side meters included); every other call the dense ones
	bool    defer = false;        // the tail (k_gate; the job's reduction if mtr_engine_reduce follows) on the side stream
	SegPlan sp;                   // the whole fragments through k_seg?
};

// K-weighting coefficients and channel gains (_chan_gain, ebu_r128_proc.cc:29: L R C Ls Rs) of a fused kernel's arguments
constexpr float CHAN_GAIN[MTR_MAX_CHANNELS] = { 1.0f, 1.0f, 1.0f, 1.41f, 1.41f };
template <typename A> static void set_kweight (const mtr_engine* e, A& a)
{
	a.a0 = e->kw[0]; a.a1 = e->kw[1]; a.a2 = e->kw[2]; a.b1 = e->kw[3]; a.b2 = e->kw[4]; a.c3 = e->kw[5]; a.c4 = e->kw[6];
	if constexpr (requires { a.gain_l; }) { a.gain_l = CHAN_GAIN[0]; a.gain_r = CHAN_GAIN[1]; }
	else for (int c = 0; c < MTR_MAX_CHANNELS; ++c) a.gain[c] = CHAN_GAIN[c];
}

// every per-meter limit is checked before anything is launched or any host-side state moves: the first that applies answers — the side
// meters' in the order of their table, then the core's
static int check_limits (const mtr_engine* e, uint64_t n_frames)
{
	for (const SideMeter* m : SIDE_METERS)
		if ((e->cfg.meters & m->bits) && m->max_frames && n_frames >= m->max_frames) return fail (MTR_ERR_ARG, m->max_text);
	// (once a stream is closed every call runs the bank's ENDS kernels, whose ends are 32 bits: mtr_ends.h)
	if ((e->cfg.meters & MTR_METER_SPECTR30) && e->n_closed && n_frames > 0xFFFFFFFEull)
		return fail (MTR_ERR_ARG, "SPECTR30 with a closed stream: n_frames per call must be < 2^32 - 1");
	if ((e->cfg.meters & MTR_METER_GONIO) && e->n_closed && n_frames > 0xFFFFFFFEull)   // (likewise: mtr_gonio_ends.h)
		return fail (MTR_ERR_ARG, "GONIO with a closed stream: n_frames per call must be < 2^32 - 1");
	if ((e->cfg.meters & MTR_METER_GONIO) && e->go.os > 1 && n_frames > 0xFFFFFFFEull / e->go.os)   // (its kernels count points: mtr_gonio_os.h)
		return fail (MTR_ERR_ARG, "GONIO oversampled: n_frames * factor per call must be < 2^32 - 1");
	if ((e->cfg.meters & MTR_METER_TPBALLIST) && n_frames >= 0x7ffff000ull) return fail (MTR_ERR_ARG, "TPBALLIST: n_frames per call must be < 2^31 - 4096");
	if ((e->cfg.meters & (MTR_METER_EBU | MTR_METER_TRUEPEAK)) && n_frames >= 0xFFFFFFFFull) return fail (MTR_ERR_ARG, "n_frames per call must be < 2^32 - 1");
	return MTR_OK;
}

// the call's stream becomes the engine's: a caller that moved to another one is ordered behind what the previous one still has to do
static int enter_stream (mtr_engine* e, hipStream_t st)
{
	if (st != e->last_stream && e->queued) {
		HIPCHK (e->xs_event.ensure ());
		HIPCHK (hipEventRecord (e->xs_event.v, e->last_stream));
		HIPCHK (hipStreamWaitEvent (st, e->xs_event.v, 0));
	}
	e->last_stream = st;
	e->queued = true;
	e->snap_valid = false;
	e->advanced = true;
	return MTR_OK;
}

static int tail_setup (mtr_engine* e)
{
	if (e->tail_stream.v) return MTR_OK;
	HIPCHK (e->tail_stream.ensure ());
	for (Event* v : { &e->ev_fused, &e->ev_gate[0], &e->ev_gate[1], &e->ev_red, &e->ev_main }) HIPCHK (v->ensure ());
	return MTR_OK;
}

// One call in progress: what its steps share, and the steps in the order of the launches
struct CallRun {
	mtr_engine* const e;
	const Call&  c;
	const Plan&  pl = e->plan;
	const bool   ebu = e->cfg.meters & MTR_METER_EBU, tp = e->cfg.meters & MTR_METER_TRUEPEAK;
	const bool   tm = e->timing && e->timed_calls < 4096;             // this call is timed ...
	const size_t ev0 = (size_t) e->timed_calls * EV_PER_CALL;         // ... with the events from here
	Route        r;
	Cursors      nx = e->pos;          // the cursors behind this call: computed as it goes, stored by its commit
	// the per-stream arrays of a ragged call on the device (null otherwise: the launchers then take the dense instantiation)
	const uint32_t* d_ends = nullptr;
	const uint32_t* d_lim = nullptr;
	const uint32_t* d_from = nullptr;
	StreamEnds   se[std::size (SIDE_METERS)];   // ... and what each row's step gets of them: the ends, the row's own words behind them (all null otherwise)
	bool         any_from = false;     // k_seg left a closing stream's last peaks to k_kwtp16
	LenSlot*     ls = nullptr;
	int          tb = 0;               // tile_power buffer of the call
	float*       tile_power = nullptr;
	bool         fold_in_history = false;   // (deferred gate: k_history folds the call's true peak in its place)

	// timing event `idx` of the call on stream `s`, if the call is timed
	int mark (int idx, hipStream_t s) const
	{
		if (!tm) return MTR_OK;
		const hipEvent_t v = next_event (e->ev, ev0 + EV_PER_CALL - 1) ? e->ev[ev0 + idx].v : nullptr;   // (the whole group exists or none of it is used)
		if (v) HIPCHK (hipEventRecord (v, s));
		return MTR_OK;
	}

	// A chunk's first step (mtr_source.hip): its source — integer rows, wide frames, planes — to f32 frames, where the meters will read them
	int decode ()
	{
		const Call::Decode& d = c.dec;
		const uint32_t C = e->cfg.n_channels;
		const bool pcm = d.format != 0;                            // (wide f32 frames and f32 planes are staged, and nothing of it counts as PCM)
		hipEvent_t t0 = nullptr, t1 = nullptr;
		if (pcm && e->timing && e->pcm_timed < 4096) {
			t0 = next_event (e->pcm_ev, (size_t) e->pcm_timed * 2);
			t1 = next_event (e->pcm_ev, (size_t) e->pcm_timed * 2 + 1);
		}
		if (t0 && t1) HIPCHK (hipEventRecord (t0, c.st));
		if (mtr_launch_decode ({ d.kind, d.format, d.src, d.pitch, d.width, e->src.map, C, const_cast<float*> (c.audio), c.stride * C, c.cnt, c.n_frames, c.st }))
			return fail (MTR_ERR_HIP, d.kind == MTR_DECODE_PLANES ? "k_plane launch" : d.kind == MTR_DECODE_FRAMES ? "k_pick launch" : "k_pcm launch");
		if (t0 && t1) { HIPCHK (hipEventRecord (t1, c.st)); e->pcm_timed++; }
		if (d.read) HIPCHK (hipEventRecord (d.read, c.st));
		// the counters: chunks per staging kernel; chunks and source bytes of the integer formats, whichever kernel decoded them
		e->plane_staged += d.kind == MTR_DECODE_PLANES;
		e->lay_staged += d.kind == MTR_DECODE_FRAMES;
		if (pcm) {
			e->pcm_chunks++;
			e->pcm_bytes += (uint64_t) c.cnt * c.n_frames * d.width * mtr_setup_pcm_sample_bytes (d.format);
		}
		return MTR_OK;
	}

	Route route () const
	{
		Route o;
		// Per-stream lengths: a call with them, or any call once a stream of this view is closed (its end is then 0: untouched).
		o.ragged = c.frames != nullptr;
		for (uint32_t i = 0; !o.ragged && e->n_closed && i < c.cnt; ++i) o.ragged = e->closed[c.off + i] != 0;
		if (!ebu && !tp) return o;
		const PlanCtx pctx = plan_ctx (e);
		o.sp = seg_plan (&pctx, c.audio, c.n_frames);
		// (k_seg hands the peak of a closing stream's last segments to k_kwtp16, whose tiles hold at most 64 x 38 frames: a whole
		// fragment up to 48.6 kHz.  Above that a call with lengths takes k_kwtp16 alone.)
		if (o.ragged && o.sp.use && e->fragm > 64u * (uint32_t) e->run) o.sp.use = false;
		// The tail of this call on the side stream?  Auto: a batch whose whole fragments go through k_seg, in an engine that meters
		// nothing else — measured (profiles/r06_tail.md): beside k_seg (issue-bound, one wave per SIMD, registers and LDS to spare) the
		// step is 0.04 - 1.4 % shorter than with the gate in front of it; beside k_kw (HBM-bound, eight waves per CU) it costs 8 %
		// MORE; behind k_bank it would start exactly when the next k_seg does; the chunks of a host call are link-bound anyway.
		const bool only_fused = (e->cfg.meters & ~(uint32_t) (MTR_METER_EBU | MTR_METER_TRUEPEAK)) == 0;
		// (and a batch of thousands of streams: the gate's serial time grows with the streams, what deferring it costs does not — at 1024 streams x 60 s
		// the serial order is 0.5 % FASTER, at 8192 x 10 s the deferred one by 0.4 - 1.4 % across boxes)
		o.defer = e->layout != 8 && (e->tail_mode == 2 || (e->tail_mode == 0 && !c.chunk && o.sp.use && only_fused && c.cnt >= TAIL_AUTO_STREAMS
		                                                   && (uint64_t) c.cnt * c.n_frames >= TAIL_AUTO_FRAMES));
		return o;
	}

	// [ends S | frag_lim S | from_tile S] of a ragged call into the next slot of the lengths ring, behind them the own words of every row of
	// the engine that has some (SideMeter::ends_words per stream, filled by its ends_fill), in the order of the table; uploaded on the
	// call's stream (an engine without EBU / TRUEPEAK has no plan: its frag_lim / from_tile are never read)
	int upload_lengths ()
	{
		const SegPlan& sp = r.sp;
		const uint32_t S = c.cnt;
		const bool fused = ebu || tp;
		size_t words = (size_t) 3 * S;
		for (const SideMeter* m : SIDE_METERS) if (e->cfg.meters & m->bits) words += (size_t) m->ends_words * S;
		const int slot = (e->len_cur + 1) % LEN_SLOTS;
		ls = &e->len_slot[slot];
		for (int i = 0; i < 2; ++i) if (ls->pending[i]) { HIPCHK (hipEventSynchronize (ls->done[i].v)); ls->pending[i] = false; }
		for (int i = 0; i < 2; ++i) HIPCHK (ls->done[i].ensure ());
		if (ls->dev.reserve (words) || ls->pin.reserve (words)) return fail (MTR_ERR_NOMEM, "per-stream lengths");
		uint32_t* const h_end = ls->pin.p;
		uint32_t* const h_lim = h_end + S;
		uint32_t* const h_from = h_end + 2 * (size_t) S;
		for (uint32_t i = 0; i < S; ++i) {
			const uint64_t f = call_frames (e, c, i);
			h_end[i] = (uint32_t) f;
			if (!fused) { h_lim[i] = h_from[i] = 0; continue; }
			// fragments that end at or before the stream's end
			const uint32_t nf = (uint32_t) (std::upper_bound (pl.frag_end.begin (), pl.frag_end.end (), (uint32_t) f) - pl.frag_end.begin ());
			h_lim[i] = f == 0 ? MTR_GATE_UNTOUCHED : f < c.n_frames ? (nf | MTR_GATE_CLOSING) : pl.n_frag;
			h_from[i] = 0xFFFFFFFFu;
			if (sp.use && f < c.n_frames) {
				// k_seg keeps the peak of every segment that reaches past f - 24 to itself; k_kwtp16 covers them from the first one on
				for (uint32_t q = 0; q < sp.n_segs; ++q) {
					const uint64_t fq = (uint64_t) q * sp.base + std::min (q, sp.rem), cq = sp.base + (q < sp.rem ? 1u : 0u);
					if ((fq + cq) * e->fragm + 24 + sp.head > f) { h_from[i] = pl.head_tiles + (uint32_t) fq; any_from = true; break; }
				}
			}
		}
		d_ends = ls->dev.p; d_lim = d_ends + S; d_from = d_ends + 2 * (size_t) S;
		size_t at = (size_t) 3 * S;                                   // where the next row's own words begin
		for (size_t k = 0; k < std::size (SIDE_METERS); ++k) {
			const SideMeter* const m = SIDE_METERS[k];
			if (!(e->cfg.meters & m->bits)) continue;
			se[k].ends = d_ends;
			if (!m->ends_words) continue;
			se[k].own = d_ends + at;
			se[k].note = m->ends_fill (e, c, h_end + at);
			at += (size_t) m->ends_words * S;
		}
		HIPCHK (hipMemcpyAsync (ls->dev.p, ls->pin.p, words * sizeof (uint32_t), hipMemcpyHostToDevice, c.st));
		e->len_cur = slot;
		return MTR_OK;
	}

	// The batch path: whole fragments through k_seg; the rest of an open fragment in front of them and what is left of the call
	// behind them (less than a fragment each) through k_kwtp16, each as ONE segment that picks the K-filter state up where its
	// predecessor in the stream left it.  `fa`: the call's k_kwtp16 arguments.
	int seg_batch (mtr_fused_args& fa)
	{
		const SegPlan& sp = r.sp;
		const uint32_t S = c.cnt;
		int lrc = 0;
		if (pl.head_tiles) {
			fa.seg_tile = e->head_seg; fa.n_segs = 1;
			lrc = mtr_launch_kwtp16 (e->run, ebu, fa, S, c.st);
		}
		mtr_seg_args sa;
		sa.audio = c.audio; sa.stride = c.stride; sa.hist = fir_hist (e, c, 0); sa.state = fa.state; sa.tile_power = tile_power;
		sa.head = sp.head; sa.tile0 = pl.head_tiles;
		sa.mfma_a = e->m16_a.p;
		sa.n_streams = S; sa.n_segs = sp.n_segs; sa.n_tiles = pl.n_tiles; sa.tile_frames = e->fragm;
		sa.seg_base = sp.base; sa.seg_rem = sp.rem; sa.n_main = sp.n_main; sa.warm_steps = sp.warm_steps;
		sa.p0_end = (int64_t) c.n_frames - 24 - (int64_t) sp.head;
		sa.screen = e->seg_screen; sa.seg_stats = e->prune_cnt.p + 2;
		set_kweight (e, sa);
		sa.ends = d_ends;
		const uint64_t units = (uint64_t) S * sp.n_segs;
		if (!lrc) lrc = mtr_launch_seg (ebu, sa, (uint32_t) ((units + 63) / 64), c.st);
		if (!lrc && any_from) {
			// the peaks k_seg left to k_kwtp16: from each closing stream's first such segment to its end (true peak only)
			fa.seg_tile = e->head_seg + 1; fa.n_segs = 1; fa.from_tile = d_from;
			lrc = mtr_launch_kwtp16 (e->run, false, fa, S, c.st);
			fa.from_tile = nullptr;
		}
		if (!lrc && pl.n_tiles > pl.head_tiles + sp.tiles) {
			fa.seg_tile = e->tail_seg; fa.n_segs = 1;
			lrc = mtr_launch_kwtp16 (e->run, ebu, fa, S, c.st);
		}
		nx.seg_calls += 1; nx.seg_frames += (uint64_t) sp.tiles * e->fragm;
		return lrc;
	}

	// layout 8: k_kwmc with its per-channel side buffers
	int kwmc (uint32_t warm_tiles) const
	{
		const size_t C = e->cfg.n_channels;
		mtr_kwmc_args ma;
		ma.audio = c.audio; ma.stride = c.stride; ma.hist = mc_hist (e, c, 0);
		ma.tile_start = e->tile_start; ma.seg_tile = e->seg_tile; ma.scan_m = e->scan_m.p;
		ma.kz = e->mc_kz.p + c.off * C * 4; ma.tp_call = e->mc_tp_call.p + c.off * C;
		ma.tile_power = tile_power; ma.mfma_a = e->m16_a.p;
		ma.n_streams = c.cnt; ma.n_segs = pl.n_segs; ma.n_tiles = pl.n_tiles; ma.warm_tiles = warm_tiles;
		ma.n_frames = c.n_frames;
		set_kweight (e, ma);
		if (c.wave51) return mtr_launch_kwmc51 (ebu, tp, ma, d_ends, c.cnt * pl.n_segs, c.st);
		return mtr_launch_kwmc ((int) C, ebu, tp, ma, d_ends, c.cnt * pl.n_segs, c.st);
	}

	// the call's K-weighting / true-peak kernels: k_seg's batch path, layout 8, or one launch of layout 3 / 4 / 6
	int fused_kernels ()
	{
		const uint32_t S = c.cnt;
		// (deferred: the other tile_power buffer than the previous call's, whose gate may still be reading; the gate that read
		// this one two calls ago must be through — it has been for a whole call)
		tb = r.defer ? (e->tp_cur ^ 1) : 0;
		if (r.defer && e->gate_pending[tb]) { HIPCHK (hipStreamWaitEvent (c.st, e->ev_gate[tb].v, 0)); e->gate_pending[tb] = false; }
		e->tp_cur = tb;
		tile_power = e->tile_power[tb].p + (size_t) c.off * pl.n_tiles;
		const uint32_t warm_tiles = (uint32_t) std::ceil (MTR_WARM_SEC * e->cfg.sample_rate / (float) (64 * e->run));
		int lrc = 0;
		if (e->layout == 8) lrc = kwmc (warm_tiles);
		else {
			mtr_fused_args fa;
			fa.audio = c.audio; fa.stride = c.stride; fa.hist = fir_hist (e, c, 0);
			fa.tile_start = e->tile_start; fa.seg_tile = e->seg_tile; fa.scan_m = e->scan_m.p;
			fa.state = e->state.p + c.off; fa.tile_power = tile_power;
			fa.n_streams = S; fa.n_segs = pl.n_segs; fa.n_tiles = pl.n_tiles; fa.warm_tiles = warm_tiles;
			set_kweight (e, fa);
			fa.n_frames = c.n_frames;
			fa.buf_slots = e->layout >= 4 ? pl.kw_slots : pl.buf_slots;
			fa.mfma_a = e->m16_a.p;
			fa.fir_form = e->cfg.tune_fir;
			fa.rotate = e->layout == 3;
			fa.prune = e->cfg.tune_prune > 2 ? 2 : (int) e->cfg.tune_prune;
			fa.prune_stats = e->prune_cnt.p;
			fa.ends = d_ends; fa.from_tile = nullptr;
			lrc = r.sp.use     ? seg_batch (fa)
			    : e->layout == 6 ? mtr_launch_kwtp16 (e->run, ebu, fa, S * pl.n_segs, c.st)
			    : e->layout == 4 ? mtr_launch_kw (e->run, fa, S * pl.n_segs, c.st)
			                     : mtr_launch_fused2 (e->run, ebu, tp, fa, S * pl.n_segs, c.st);
		}
		if (lrc) { plan_abort (e, c.st); return fail (MTR_ERR_HIP, "k_fused launch", hipGetLastError ()); }
		return mark (1, c.st);
	}

	// k_gate behind the fused kernels: on the call's stream, or — deferred — handed over to the side stream
	int gate ()
	{
		hipStream_t gst = c.st;                                       // the stream the gate runs on
		if (r.defer) {
			gst = e->tail_stream.v;
			HIPCHK (hipEventRecord (e->ev_fused.v, c.st));
			HIPCHK (hipStreamWaitEvent (gst, e->ev_fused.v, 0));
			// The gate becomes runnable at the very moment the NEXT call's fused kernel does (both wait for this call's), and
			// its 8192 workgroups would flood the CUs while k_seg's 1024 one-wave workgroups are being placed, one per SIMD:
			// measured, k_seg then takes 15.4 ms instead of 9.5 (profiles/r06_tail.md) — the placement of a persistent kernel
			// is for good.  So the side stream first idles for tail_delay_us: by then k_seg is resident (its dispatch takes
			// ~10 us) and the gate's waves (72 VGPRs) fill in beside it (344 of 512).  Off the critical path by construction.
			if (e->tail_delay_us && mtr_launch_delay (e->tail_delay_us, gst)) { plan_abort (e, c.st); return fail (MTR_ERR_HIP, "k_delay launch"); }
			e->tail_pending = true;
			e->deferred_calls++;
			fold_in_history = tp;
		}
		{ const int rc = mark (2, gst); if (rc) return rc; }
		mtr_gate_args ga;
		ga.state = e->state.p + c.off; ga.hist = e->hist.p + (size_t) c.off * 2 * MTR_HIST_LEN; ga.tile_power = tile_power;
		ga.frag_tile = e->frag_tile; ga.frag_power = e->frag_power.p + (size_t) c.off * pl.n_frag; ga.bin_power = e->bin_power.p;
		ga.n_streams = c.cnt; ga.n_tiles = ebu ? pl.n_tiles : 0; ga.n_frag = ebu ? pl.n_frag : 0;
		ga.tail_tile = ebu ? pl.tail_tile : 0;
		ga.fragm = (float) e->fragm; ga.integr = e->integr ? 1 : 0;
		ga.max_scratch = e->gate_max.p + (size_t) c.off * 2;
		ga.fold_tp = (fold_in_history || e->layout == 8) ? 0 : 1;   // (layout 8: k_history folds the per-channel peaks)
		ga.polite_grid = r.defer ? e->tail_gate_grid : 0;
		// (the loudness log: where the streams stand in it is an argument, computed here — the gate may run a call late)
		mtr_loudlog_args la;
		const bool log = ebu && loudlog_args (e, e->pos, c.off, &la);
		// (the integration log: where a stream stands in it is device state, the gate's own)
		mtr_integlog_args ia;
		const bool evl = ebu && integlog_args (e, c.off, &ia);
		if (mtr_launch_gate (ga, d_lim, log ? &la : nullptr, evl ? &ia : nullptr, gst)) { plan_abort (e, gst); return fail (MTR_ERR_HIP, "k_gate launch"); }
		if (ls) { HIPCHK (hipEventRecord (ls->done[1].v, gst)); ls->pending[1] = true; }
		{ const int rc = mark (3, gst); if (rc) return rc; }
		{
			PlanSlot& ps = e->plan_slot[e->plan_cur];                 // k_gate is the plan's last reader
			HIPCHK (hipEventRecord (ps.done.v, gst));
			ps.pending = true;
		}
		if (r.defer) { HIPCHK (hipEventRecord (e->ev_gate[tb].v, gst)); e->gate_pending[tb] = true; }
		e->last_n_frag = ga.n_frag;
		nx.frcnt = pl.frcnt_out;
		if (log) nx.ll_frags = e->pos.ll_frags + ga.n_frag;
		return MTR_OK;
	}

	// the 47 frames before the next call; after every consumer of the current history
	int history ()
	{
		const uint32_t C = e->cfg.n_channels;
		mtr_stream_state* const state = e->state.p + c.off;
		// (deferred: the fold of this call's peaks rides here — behind the reduction of the previous call, which reads the holds)
		if (fold_in_history && e->red_pending) { HIPCHK (hipStreamWaitEvent (c.st, e->ev_red.v, 0)); e->red_pending = false; }
		mtr_history_args ha = {};
		ha.audio = c.audio; ha.stride = c.stride; ha.n_frames = c.n_frames; ha.n_streams = c.cnt; ha.ends = d_ends;
		ha.C = C; ha.FC = c.wave51 ? 6 : C;
		if (e->layout != 8) {
			ha.HC = 2; ha.hist_in = fir_hist (e, c, 0); ha.hist_out = fir_hist (e, c, 1);
			ha.fold_state = fold_in_history ? state : nullptr;
		} else {
			const size_t vc = (size_t) c.off * C;
			ha.HC = C; ha.hist_in = mc_hist (e, c, 0); ha.hist_out = mc_hist (e, c, 1);
			ha.tp_call = e->mc_tp_call.p + vc; ha.tp_last = e->mc_tp_last.p + vc; ha.tp_hold = e->mc_tp_hold.p + vc; ha.state = state;
		}
		// (beside the true-peak bar a stream that ends inside the call leaves the frames in front of its OWN end; everywhere else a call with
		// lengths leaves those in front of the call's end: the two rules of mtr_history.hip)
		const HistCut cut = !d_ends ? HIST_CALL_END : e->layout != 8 && (e->cfg.meters & MTR_METER_TPBALLIST) ? HIST_OWN_END : HIST_CALL_END_IF_TOUCHED;
		if ((e->layout != 8 || tp) && mtr_launch_history (cut, HIST_ROW_FIR, ha, c.st)) return fail (MTR_ERR_HIP, "k_history launch");
		nx.hist_cur = e->pos.hist_cur ^ 1;
		return MTR_OK;
	}

	// The steps of a call, in the order of the launches.  What describes QUEUED WORK (last_stream / queued, the plan and lengths rings,
	// tp_cur, the pending flags of the side stream, the timing events) moves where the work is queued: it must be true even if a later
	// launch fails.  What describes the METERING POSITION moves at the end: an error return has not advanced the engine.
	int run ()
	{
		int rc = check_limits (e, c.n_frames);
		if (rc) return rc;
		if ((rc = enter_stream (e, c.st))) return rc;
		const bool fused = ebu || tp;
		const uint32_t meters = e->cfg.meters;
		if (c.dec.kind && ((rc = mark (6, c.st)) || (rc = decode ()))) return rc;
		if ((rc = mark (0, c.st))) return rc;
		if (tm) {
			if (e->ev_decode.size () <= e->timed_calls) e->ev_decode.resize ((size_t) e->timed_calls + 1);
			e->ev_decode[e->timed_calls] = c.dec.kind != MTR_DECODE_NONE;
		}

		r = route ();
		if (r.defer) rc = tail_setup (e);
		else if (fused) rc = join_tail (e, c.st);                     // a serial gate follows the deferred ones
		if (rc) return rc;
		e->last_deferred = r.defer;

		if (fused) {
			if ((rc = build_plan (e, c.n_frames, r.sp.use ? r.sp.head : 0, r.sp.use ? r.sp.tiles : 0, c.st))) return rc;
			if (r.ragged && (rc = upload_lengths ())) return rc;
			if ((rc = fused_kernels ())) return rc;
			if ((rc = gate ())) return rc;
		} else {
			if (r.ragged && (rc = upload_lengths ())) return rc;       // (the side meters' steps read the ends)
			for (int i = 1; i <= 3; ++i) if ((rc = mark (i, c.st))) return rc;
		}
		if ((rc = mark (4, c.st))) return rc;

		for (size_t k = 0; k < std::size (SIDE_METERS); ++k) {
			const SideMeter* const m = SIDE_METERS[k];
			if ((meters & m->bits) && m->step && (rc = m->step (e, c, nx, se[k]))) return rc;
		}
		if ((meters & (MTR_METER_TRUEPEAK | MTR_METER_TPBALLIST)) && (rc = history ())) return rc;
		if (ls) {                                                     // (the lengths' last reader on this stream: k_history under one of its ends rules, a side meter's LEN kernel, or the fused kernels)
			HIPCHK (hipEventRecord (ls->done[0].v, c.st));
			ls->pending[0] = true;
		}
		if (tm) {
			const hipEvent_t v = next_event (e->ev, ev0 + 5);
			if (v) { HIPCHK (hipEventRecord (v, c.st)); e->timed_calls++; }   // (a call without all of its events is not a timed call)
		}
		// everything is queued.  Frames metered per stream; a stream that ends inside a call with lengths is closed by it
		const bool log = ebu && e->ll.period;
		for (uint32_t i = 0; i < c.cnt; ++i) {
			const size_t g = (size_t) c.off + i;
			if (e->closed[g]) continue;
			const uint64_t f = call_frames (e, c, i);
			e->metered[g] += f;
			stream_counts (e, g, &c, f);
			if (log) {
				// periods the stream completed: those that end within the fragments it ended (as upload_lengths counts them)
				const uint64_t nf = f == c.n_frames ? pl.n_frag : (uint64_t) (std::upper_bound (pl.frag_end.begin (), pl.frag_end.end (), (uint32_t) f) - pl.frag_end.begin ());
				e->ll.points[g] += (e->pos.ll_frags % e->ll.period + nf) / e->ll.period;
			}
			if (f < c.n_frames) { e->closed[g] = 1; e->n_closed++; }
		}
		if (c.commit) e->pos = nx;
		return MTR_OK;
	}
};

static int process_call (mtr_engine* e, const Call& c) { return CallRun { e, c }.run (); }

// Where a chunked call takes its samples from: host or device memory, f32 or integer PCM (format MTR_PCM_*, 0 = f32)
struct Source {
	const void* p;
	int         format;
	bool        host;
	void*       hip_stream;   // device source: the caller's stream (a host source runs on the engine's own)
};

// Memory in, CHUNKED by streams (results are per stream: chunking is exact, and the routing of a call — which kernel,
// how many time segments — is decided for the whole batch, so every stream sees the arithmetic it would see resident):
// chunk k + 1 crosses the host link on a copy stream while the kernels of chunk k run on the engine's own; two device
// buffers of one chunk each instead of a copy of the whole batch.  End to end the call runs at the link's rate
// (bench.py: extra.end_to_end_host).
// Integer PCM is the same loop with one more step: the chunk's INTEGER rows cross the link into one of two raw buffers (rows on 16
// bytes), and the chunk's call decodes them into the float buffer first (CallRun::decode) — the float chunk is laid out exactly as the
// float path stages it (same dstride, same chunks: host_chunk_bytes counts decoded bytes), so the meters see the very same call.  The
// raw buffer is free again once the decode has read it, the float buffer once the meters have: stream order, both on the engine's stream.
// PCM in device memory: the same chunks without the copy, decoded straight from the caller's rows on the caller's stream.
// A plane layout (mtr_planes.h) is one more source geometry of the same loop: the chunk's cnt * P planes cross the link as the rows of
// ONE 2-D copy into the raw buffer (or are read where they lie in device memory), and k_plane is the chunk's first step.
static int process_chunked (mtr_engine* e, const Source& src, uint64_t n_frames, uint64_t stride, const uint64_t* frames)
{
	if (n_frames == 0) return MTR_OK;
	if (stride < n_frames) return fail (MTR_ERR_ARG, "stream_stride_frames < n_frames");
	int rc = check_limits (e, n_frames);
	if (rc) return rc;
	HIPCHK (hipSetDevice (e->cfg.device));
	const size_t C = e->cfg.n_channels;
	const uint32_t S = e->cfg.n_streams;
	// (streams start on 16 bytes in the staging buffers — an even stride of stereo frames, a multiple of four mono ones — so that
	// every layout can take the call and k_tpb's LDS-DMA its source)
	const uint64_t dstride = C == 2 ? (n_frames + 1) & ~(uint64_t) 1 : (n_frames + 3) & ~(uint64_t) 3;   // (and 1, 3, 4, 5 channels: a multiple of four frames)
	const size_t row = (size_t) dstride * C;                                  // floats per staged stream
	uint32_t cs = (uint32_t) std::min<uint64_t> (S, std::max<uint64_t> (1, e->host_chunk_bytes / (row * sizeof (float))));
	const uint32_t n_chunks = (S + cs - 1) / cs;
	cs = (S + n_chunks - 1) / n_chunks;                                         // even chunks
	const size_t buf_floats = ((size_t) cs * row + 63) & ~(size_t) 63;         // the second buffer starts on 256 bytes
	// The source's geometry, once.  A ROW is what one row of the link copy and of the landing buffer is: a stream's frames — of the layout's
	// width under a frame layout, which the chunk's first step picks as PCM is decoded by it —, or under a plane layout ONE PLANE of n_frames
	// samples, `stride` samples from plane to plane, a chunk cnt * width of them, interleaved by the chunk's first step
	const mtr_decode_kind kind = e->src.kind ? e->src.kind : src.format ? MTR_DECODE_ROWS : MTR_DECODE_NONE;
	const bool planes = kind == MTR_DECODE_PLANES;
	struct {
		size_t sb, width;             // bytes per sample at the source; samples of a source frame, or planes of a stream
		size_t rows, row_samples;     // rows per stream, samples per row
		size_t pitch, land_pitch;     // bytes from row to row at the source, and where a host source's rows land
	} g;
	g.sb = src.format ? mtr_setup_pcm_sample_bytes (src.format) : sizeof (float);
	g.width = e->src.kind ? e->src.width : C;
	g.rows = planes ? g.width : 1;
	g.row_samples = planes ? n_frames : n_frames * g.width;
	g.pitch = (planes ? stride : stride * g.width) * g.sb;
	const bool landing = src.host && kind;                                     // PCM / wide frames / planes from the host land raw, rows on 16 bytes
	g.land_pitch = landing ? (g.row_samples * g.sb + 15) & ~(size_t) 15 : row * sizeof (float);
	const size_t raw_bytes = ((size_t) cs * g.rows * g.land_pitch + 255) & ~(size_t) 255;   // bytes per raw buffer
	hipStream_t st = (hipStream_t) src.hip_stream;
	if (src.host) {
		HIPCHK (e->own_stream.ensure ());
		st = e->own_stream.v;
		HIPCHK (e->copy_stream.ensure ());
		for (int b = 0; b < 2; ++b) {
			HIPCHK (e->ev_copied[b].ensure ());
			HIPCHK (e->ev_computed[b].ensure ());
		}
		// the staging buffers may still be read by the previous call (on whatever stream that ran)
		HIPCHK (hipStreamSynchronize (e->last_stream));
	} else if (e->stage.n < buf_floats * (n_chunks > 1 ? 2 : 1)) {
		// (a device source never waits for the previous call — the chunk's call orders its stream behind it before the decode writes the
		// staging buffer — unless that buffer has to grow)
		if ((rc = sync_all (e))) return rc;
	}
	if (e->stage.reserve (buf_floats * (n_chunks > 1 ? 2 : 1))) return fail (MTR_ERR_NOMEM, "hipMalloc staging buffers");
	if (landing && e->pcm_raw.reserve (raw_bytes * (n_chunks > 1 ? 2 : 1))) return fail (MTR_ERR_NOMEM, "hipMalloc PCM buffers");
	// (every exit behind the first copy goes through ONE place that waits for the copy stream: the source is pageable caller
	// memory and the copies are truly asynchronous — the caller may free or reuse it as soon as we return, error or not)
	hipError_t he = hipSuccess;
	const char* what = nullptr;
#define HOSTCHK(call) do { he = (call); if (he != hipSuccess) { what = #call; goto done; } } while (0)
	for (uint32_t k = 0, off = 0; k < n_chunks; ++k, off += cs) {
		const uint32_t cnt = std::min (cs, S - off);
		const int b = (int) (k & 1);
		float* const dst = e->stage.p + (size_t) b * buf_floats;
		// (the lengths of the chunk's streams are indexed from its first; the cursors move with the last chunk)
		Call c { dst, n_frames, dstride, st, off, cnt, frames ? frames + off : nullptr, true, k + 1 == n_chunks };
		const uint8_t* from = (const uint8_t*) src.p + (size_t) off * g.rows * g.pitch;
		size_t pitch = g.pitch;
		if (src.host) {
			void* const land = landing ? (void*) (e->pcm_raw.p + (size_t) b * raw_bytes) : (void*) dst;
			if (k >= 2) HOSTCHK (hipStreamWaitEvent (e->copy_stream.v, e->ev_computed[b].v, 0));   // the kernels of chunk k - 2 have read this buffer
			HOSTCHK (hipMemcpy2DAsync (land, g.land_pitch, from, g.pitch, g.row_samples * g.sb, cnt * g.rows, hipMemcpyHostToDevice, e->copy_stream.v));
			HOSTCHK (hipEventRecord (e->ev_copied[b].v, e->copy_stream.v));
			HOSTCHK (hipStreamWaitEvent (st, e->ev_copied[b].v, 0));
			from = (const uint8_t*) land;
			pitch = g.land_pitch;
		}
		if (kind) c.dec = { kind, from, pitch, src.format, (uint32_t) g.width, landing ? e->ev_computed[b].v : nullptr };
		rc = process_call (e, c);
		if (rc) goto done;
		if (src.host && !landing) HOSTCHK (hipEventRecord (e->ev_computed[b].v, st));
	}
#undef HOSTCHK
done:
	if (src.host) {
		// wait for the copies (not for the kernels)
		const hipError_t hs = hipStreamSynchronize (e->copy_stream.v);
		if (what) return fail (MTR_ERR_HIP, what, he);
		if (rc) return rc;
		if (hs != hipSuccess) return fail (MTR_ERR_HIP, "hipStreamSynchronize (copy stream)", hs);
	}
	return rc;
}

static int process_device (mtr_engine* e, const float* d_audio, uint64_t n_frames, uint64_t stride, const uint64_t* frames, void* hip_stream)
{
	// A frame layout.  WAVE 5.1 on a 5-channel engine: k_kwmc51 and k_history (FC = 6) read the 6-channel frames where they lie (a pick pass
	// in front of an HBM-bound kernel would read 6/5 and write 5/5 of the batch on top).  Every other map: the wide rows are picked chunk
	// by chunk into the staging buffers, as device PCM is decoded.
	// (not beside the surround meter, whose kernel takes frames of the engine's five channels: that engine stages the call like any other map)
	const bool direct = e->src.wave51 && !(e->cfg.meters & MTR_METER_SURROUND);
	// A plane layout: always staged, chunk by chunk through k_plane (no kernel of the meters reads planes)
	if (e->src.kind && !direct) return process_chunked (e, { d_audio, 0, false, hip_stream }, n_frames, stride, frames);
	if (n_frames == 0) return MTR_OK;
	if (stride < n_frames) return fail (MTR_ERR_ARG, "stream_stride_frames < n_frames");
	HIPCHK (hipSetDevice (e->cfg.device));
	Call c { d_audio, n_frames, stride, (hipStream_t) hip_stream, 0, e->cfg.n_streams, frames, false, true };
	c.wave51 = direct;
	const int rc = process_call (e, c);
	if (!rc && direct) e->lay_direct++;
	return rc;
}

void stream_counts (mtr_engine* e, size_t g, const Call* c, uint64_t frames)
{
	for (const SideMeter* m : SIDE_METERS) {
		if (!(e->cfg.meters & m->bits)) continue;
		if (m->count) m->count (e, g, c, frames);
		if (!m->series) continue;
		const SeriesView v = m->series (e);
		uint64_t whole = 0;
		uint32_t partial = 0;
		if (!c) (*v.points)[g] = (e->pos.*v.pos).points;
		else if (v.cfg->period && series_cut ((e->pos.*v.pos).fill, v.cfg->period, c->n_frames, frames, &whole, &partial)) (*v.points)[g] += whole + partial;
	}
}

// the counts of the one row of SIDE_METERS that has `bit` and keeps them (mtr_engine_series_points, mtr_engine_spectr_points)
void series_points_of (mtr_engine* e, uint32_t bit, uint32_t first, uint32_t count, uint64_t* points)
{
	for (const SideMeter* m : SIDE_METERS) {
		if (!(m->bits & bit) || !m->series) continue;
		const std::vector<uint64_t>& v = *m->series (e).points;
		for (uint32_t i = 0; i < count; ++i) points[i] = v[first + i];
	}
}

extern "C" {

int mtr_engine_process_device (mtr_engine* e, const float* d_audio, uint64_t n_frames,
                               uint64_t stride, void* hip_stream)
{
	if (!e || !d_audio) return fail (MTR_ERR_ARG, "mtr_engine_process_device: null argument");
	return process_device (e, d_audio, n_frames, stride, nullptr, hip_stream);
}

// The six families of calls with per-stream ends (mtr_engine_process_{device,host}_*): which meters a family admits — an engine of some
// of them and of no other — and what else it refuses.  frames_ends: applies a row, then takes the call.
// _lengths: EBU / TRUEPEAK alone (every layout, 2 .. 5 channels); _tracks: and the whole-track meters (DR14, KMETER, BITSTATS, SIGDIST);
// _ragged: and the two that keep a reading series, STCORR and NEEDLE (mtr_ragged.h); _ends: and the 30-band bank (mtr_ends.h);
// _tpb: and the true-peak bar (mtr_tpb.h); _any: and the scope and the surround meter, with no limit on the channels of its own
// (mtr_any.h).  What is left outside is one call of the surround meter with a period: a stream that ends before the group of four completes
// which the call before left open needs its K-meters' state in front of that group, as KMETER's series carries it (mtr_kmeter.hip: bz1,
// btmax), and the surround meter's dense kernel and state do not make it (family_check)
constexpr uint32_t LENGTHS_METERS = MTR_METER_EBU | MTR_METER_TRUEPEAK;
constexpr uint32_t TRACKS_METERS = LENGTHS_METERS | MTR_METER_DR14 | MTR_METER_KMETER | MTR_METER_BITSTATS | MTR_METER_SIGDIST;
constexpr uint32_t RAGGED_METERS = TRACKS_METERS | MTR_METER_STCORR | MTR_METER_NEEDLE;
constexpr uint32_t ENDS_METERS = RAGGED_METERS | MTR_METER_SPECTR30;
constexpr uint32_t TPB_METERS = ENDS_METERS | MTR_METER_TPBALLIST;
constexpr uint32_t ANY_METERS = TPB_METERS | MTR_METER_SCOPE | MTR_METER_SURROUND;
struct Family {
	const char* name;            // of its entry points: "<name>: null argument"
	uint32_t    meters;
	const char* unsupported;     // MTR_ERR_UNSUPPORTED: the engine holds another meter, or none of these
	const char* too_long;        // MTR_ERR_ARG: frames[s] > n_frames
	bool        no_km_series;    // _tracks: a KMETER engine with a period is refused
	bool        bank_ends;       // _ends: at most two channels; 32-bit ends with SPECTR30
	bool        wide = false;    // _any: ... but the channels are whatever mtr_engine_create accepted for the engine's meters
	uint32_t    need = 0;        // _gonio_ends: the engine holds this meter; its cuts are 32 bits whatever else it holds
};
enum { LENGTHS, TRACKS, RAGGED, ENDS, TPB, ANY, GONIO_ENDS };
constexpr Family FAMILIES[] = {
	{ "lengths", LENGTHS_METERS, "per-stream lengths: EBU / TRUEPEAK engines only", "per-stream lengths: frames[s] > n_frames", false, false },
	{ "tracks", TRACKS_METERS, "track lengths: EBU / TRUEPEAK / DR14 / KMETER / BITSTATS / SIGDIST engines only", "track lengths: frames[s] > n_frames", true, false },
	{ "ragged", RAGGED_METERS, "ragged batches: EBU / TRUEPEAK / DR14 / KMETER / BITSTATS / SIGDIST / STCORR / NEEDLE engines only",
	  "ragged batches: frames[s] > n_frames", false, false },
	{ "ends", ENDS_METERS,
	  "track lengths for the bank: EBU / TRUEPEAK / DR14 / KMETER / BITSTATS / SIGDIST / STCORR / NEEDLE / SPECTR30 engines of one or two channels only",
	  "track lengths for the bank: frames[s] > n_frames", false, true },
	{ "tpb", TPB_METERS,
	  "track lengths for the true-peak bar: EBU / TRUEPEAK / DR14 / KMETER / BITSTATS / SIGDIST / STCORR / NEEDLE / SPECTR30 / TPBALLIST engines of one or two channels only",
	  "track lengths for the true-peak bar: frames[s] > n_frames", false, true },
	{ "any", ANY_METERS,
	  "track lengths for every meter: EBU / TRUEPEAK / DR14 / KMETER / BITSTATS / SIGDIST / STCORR / NEEDLE / SPECTR30 / TPBALLIST / SCOPE / SURROUND engines only",
	  "track lengths for every meter: frames[s] > n_frames", false, true, true },
	// (the seventh, mtr_gonio_ends.h: the goniometer beside the stereo meters of _any — SURROUND needs three channels, GONIO two)
	{ "gonio_ends", ANY_METERS | MTR_METER_GONIO,
	  "track lengths for the goniometer: stereo engines that hold GONIO, beside EBU / TRUEPEAK / DR14 / KMETER / BITSTATS / SIGDIST / STCORR / NEEDLE / SPECTR30 / TPBALLIST / SCOPE only",
	  "track lengths for the goniometer: frames[s] > n_frames", false, true, true, MTR_METER_GONIO },
};

static int family_check (const mtr_engine* e, const Family& fam, uint64_t n_frames, const uint64_t* frames)
{
	const uint32_t meters = e->cfg.meters;
	if ((meters & ~fam.meters) || !(meters & fam.meters) || (fam.bank_ends && !fam.wide && e->cfg.n_channels > 2) || (fam.need && !(meters & fam.need)))
		return fail (MTR_ERR_UNSUPPORTED, fam.unsupported);
	if (fam.need && n_frames > 0xFFFFFFFEull) return fail (MTR_ERR_ARG, "track lengths for the goniometer: n_frames per call must be < 2^32 - 1");
	if (fam.no_km_series && (meters & MTR_METER_KMETER) && e->km.ser.period)
		return fail (MTR_ERR_UNSUPPORTED, "track lengths: a KMETER engine with a period keeps a reading series (mtr_engine_process_*_ragged)");
	// (SURROUND with a period, a block open on entry that stands inside a group of four frames, and a stream that ends before that group
	// completes: its last sur_run would have to drop the whole group from the K-meters' filter and peak, and the state in front of the
	// group is not kept — mtr_any.h.  The one call _any cannot take)
	if (fam.wide && (meters & MTR_METER_SURROUND) && e->su.ser.period && (e->pos.su.fill & 3))
		for (uint32_t i = 0; i < e->cfg.n_streams; ++i)
			if (!e->closed[i] && frames[i] && frames[i] < n_frames && frames[i] < 4 - (e->pos.su.fill & 3))
				return fail (MTR_ERR_UNSUPPORTED, "track lengths for every meter: SURROUND with a period: a stream ends before the group of four frames completes that the call before left open");
	if (fam.bank_ends && (meters & MTR_METER_SPECTR30) && n_frames > 0xFFFFFFFEull)
		return fail (MTR_ERR_ARG, "track lengths for the bank: n_frames per call must be < 2^32 - 1");
	for (uint32_t i = 0; i < e->cfg.n_streams; ++i)
		if (frames[i] > n_frames) return fail (MTR_ERR_ARG, fam.too_long);
	return MTR_OK;
}

// what the twelve entry points of the families are: `audio` in host memory (`host`) or in device memory, on `hip_stream`
static int frames_ends (mtr_engine* e, int family, bool host, const float* audio, uint64_t n_frames, uint64_t stride, const uint64_t* frames, void* hip_stream)
{
	const Family& fam = FAMILIES[family];
	if (!e || !audio || !frames) {
		char who[64];
		snprintf (who, sizeof (who), "mtr_engine_process_%s_%s: null argument", host ? "host" : "device", fam.name);
		return fail (MTR_ERR_ARG, who);
	}
	const int crc = family_check (e, fam, n_frames, frames);
	if (crc) return crc;
	return host ? process_chunked (e, { audio, 0, true, nullptr }, n_frames, stride, frames) : process_device (e, audio, n_frames, stride, frames, hip_stream);
}

int mtr_engine_process_device_lengths (mtr_engine* e, const float* d_audio, uint64_t n_frames, uint64_t stride, const uint64_t* frames, void* hip_stream)
{
	return frames_ends (e, LENGTHS, false, d_audio, n_frames, stride, frames, hip_stream);
}

int mtr_engine_process_device_tracks (mtr_engine* e, const float* d_audio, uint64_t n_frames, uint64_t stride, const uint64_t* frames, void* hip_stream)
{
	return frames_ends (e, TRACKS, false, d_audio, n_frames, stride, frames, hip_stream);
}

int mtr_engine_process_device_ragged (mtr_engine* e, const float* d_audio, uint64_t n_frames, uint64_t stride, const uint64_t* frames, void* hip_stream)
{
	return frames_ends (e, RAGGED, false, d_audio, n_frames, stride, frames, hip_stream);
}

int mtr_engine_process_device_ends (mtr_engine* e, const float* d_audio, uint64_t n_frames, uint64_t stride, const uint64_t* frames, void* hip_stream)
{
	return frames_ends (e, ENDS, false, d_audio, n_frames, stride, frames, hip_stream);
}

int mtr_engine_process_device_tpb (mtr_engine* e, const float* d_audio, uint64_t n_frames, uint64_t stride, const uint64_t* frames, void* hip_stream)
{
	return frames_ends (e, TPB, false, d_audio, n_frames, stride, frames, hip_stream);
}

int mtr_engine_process_host_tpb (mtr_engine* e, const float* h_audio, uint64_t n_frames, uint64_t stride, const uint64_t* frames)
{
	return frames_ends (e, TPB, true, h_audio, n_frames, stride, frames, nullptr);
}

int mtr_engine_process_device_any (mtr_engine* e, const float* d_audio, uint64_t n_frames, uint64_t stride, const uint64_t* frames, void* hip_stream)
{
	return frames_ends (e, ANY, false, d_audio, n_frames, stride, frames, hip_stream);
}

int mtr_engine_process_host_any (mtr_engine* e, const float* h_audio, uint64_t n_frames, uint64_t stride, const uint64_t* frames)
{
	return frames_ends (e, ANY, true, h_audio, n_frames, stride, frames, nullptr);
}

int mtr_engine_process_device_gonio_ends (mtr_engine* e, const float* d_audio, uint64_t n_frames, uint64_t stride, const uint64_t* frames, void* hip_stream)
{
	return frames_ends (e, GONIO_ENDS, false, d_audio, n_frames, stride, frames, hip_stream);
}

int mtr_engine_process_host_gonio_ends (mtr_engine* e, const float* h_audio, uint64_t n_frames, uint64_t stride, const uint64_t* frames)
{
	return frames_ends (e, GONIO_ENDS, true, h_audio, n_frames, stride, frames, nullptr);
}

int mtr_engine_process_host_lengths (mtr_engine* e, const float* h_audio, uint64_t n_frames, uint64_t stride, const uint64_t* frames)
{
	return frames_ends (e, LENGTHS, true, h_audio, n_frames, stride, frames, nullptr);
}

int mtr_engine_process_host_tracks (mtr_engine* e, const float* h_audio, uint64_t n_frames, uint64_t stride, const uint64_t* frames)
{
	return frames_ends (e, TRACKS, true, h_audio, n_frames, stride, frames, nullptr);
}

int mtr_engine_process_host_ragged (mtr_engine* e, const float* h_audio, uint64_t n_frames, uint64_t stride, const uint64_t* frames)
{
	return frames_ends (e, RAGGED, true, h_audio, n_frames, stride, frames, nullptr);
}

int mtr_engine_process_host_ends (mtr_engine* e, const float* h_audio, uint64_t n_frames, uint64_t stride, const uint64_t* frames)
{
	return frames_ends (e, ENDS, true, h_audio, n_frames, stride, frames, nullptr);
}

int mtr_engine_series_points (mtr_engine* e, uint32_t meter, uint32_t first, uint32_t count, uint64_t* points)
{
	if (!e || !points) return fail (MTR_ERR_ARG, "mtr_engine_series_points: null argument");
	if ((meter != MTR_METER_STCORR && meter != MTR_METER_NEEDLE && meter != MTR_METER_KMETER && meter != MTR_METER_SURROUND) || !(e->cfg.meters & meter))
		return fail (MTR_ERR_ARG, "mtr_engine_series_points: meter is MTR_METER_STCORR, MTR_METER_NEEDLE, MTR_METER_KMETER or MTR_METER_SURROUND, one the engine holds");
	if ((uint64_t) first + count > e->cfg.n_streams) return fail (MTR_ERR_ARG, "stream range");
	series_points_of (e, meter, first, count, points);
	return MTR_OK;
}

int mtr_series_cut (uint64_t fill, uint64_t period, uint64_t n_frames, uint64_t frames, uint64_t* whole, uint32_t* partial)
{
	if (!whole || !partial || !series_cut (fill, period, n_frames, frames, whole, partial))
		return fail (MTR_ERR_ARG, "mtr_series_cut: fill < period (or period 0), frames <= n_frames, two results");
	return MTR_OK;
}

int mtr_engine_stream_frames (mtr_engine* e, uint32_t first, uint32_t count, uint64_t* frames, uint8_t* closed)
{
	if (!e) return fail (MTR_ERR_ARG, "null engine");
	if ((uint64_t) first + count > e->cfg.n_streams) return fail (MTR_ERR_ARG, "stream range");
	for (uint32_t i = 0; i < count; ++i) {
		if (frames) frames[i] = e->metered[first + i];
		if (closed) closed[i] = e->closed[first + i];
	}
	return MTR_OK;
}

int mtr_engine_set_host_chunk_bytes (mtr_engine* e, uint64_t bytes)
{
	if (!e) return fail (MTR_ERR_ARG, "null engine");
	e->host_chunk_bytes = bytes ? (size_t) bytes : (size_t) 256 << 20;
	return MTR_OK;
}

int mtr_engine_process_host (mtr_engine* e, const float* h_audio, uint64_t n_frames, uint64_t stride)
{
	if (!e || !h_audio) return fail (MTR_ERR_ARG, "mtr_engine_process_host: null argument");
	return process_chunked (e, { h_audio, 0, true, nullptr }, n_frames, stride, nullptr);
}

// Integer PCM: what every PCM entry point checks before anything is queued
static int pcm_check (mtr_engine* e, const void* pcm, int format, uint64_t n_frames, const uint64_t* frames, const char* who)
{
	if (!e || !pcm) return fail (MTR_ERR_ARG, who);
	if (!mtr_setup_pcm_sample_bytes (format)) return fail (MTR_ERR_ARG, "unknown PCM format (MTR_PCM_S16, _S24, _S32)");
	return frames ? family_check (e, FAMILIES[LENGTHS], n_frames, frames) : MTR_OK;
}

int mtr_engine_process_host_pcm (mtr_engine* e, const void* h_pcm, int format, uint64_t n_frames, uint64_t stride, const uint64_t* frames)
{
	const int crc = pcm_check (e, h_pcm, format, n_frames, frames, "mtr_engine_process_host_pcm: null argument");
	if (crc) return crc;
	return process_chunked (e, { h_pcm, format, true, nullptr }, n_frames, stride, frames);
}

int mtr_engine_process_device_pcm (mtr_engine* e, const void* d_pcm, int format, uint64_t n_frames, uint64_t stride,
                                   const uint64_t* frames, void* hip_stream)
{
	const int crc = pcm_check (e, d_pcm, format, n_frames, frames, "mtr_engine_process_device_pcm: null argument");
	if (crc) return crc;
	return process_chunked (e, { d_pcm, format, false, hip_stream }, n_frames, stride, frames);
}

// One LV2 block: interleave into page-locked memory, one H2D copy, the kernels, one D2H copy of the stream's state
// (and the bank's levels), ONE wait.  No allocation after the first block of a given size.
int mtr_engine_process_planar_host (mtr_engine* e, const float* const* ch, uint32_t n_frames)
{
	if (!e || !ch || !ch[0]) return fail (MTR_ERR_ARG, "mtr_engine_process_planar_host: null argument");
	if (e->cfg.n_streams != 1) return fail (MTR_ERR_ARG, "planar host input is the n_streams == 1 (LV2) path");
	if (n_frames == 0) return MTR_OK;
	const uint32_t C = e->cfg.n_channels;
	for (uint32_t c = 1; c < C; ++c) if (!ch[c]) return fail (MTR_ERR_ARG, "mtr_engine_process_planar_host: a channel pointer is NULL");
	HIPCHK (hipSetDevice (e->cfg.device));
	HIPCHK (e->own_stream.ensure ());
	const hipStream_t st = e->own_stream.v;
	if (e->last_stream != st) HIPCHK (hipStreamSynchronize (e->last_stream));   // resets queued before the first block
	const size_t total = (size_t) n_frames * C;
	if (e->pin_in.n < total || e->stage.n < total) {
		HIPCHK (hipStreamSynchronize (st));
		if (e->pin_in.reserve (total) || e->stage.reserve (total)) return fail (MTR_ERR_NOMEM, "staging buffers");
	}
	if (e->pin_state.reserve (1) || e->pin_bank.reserve (2 * MTR_NBANDS)) return fail (MTR_ERR_NOMEM, "hipHostMalloc snapshot");
	float* const il = e->pin_in.p;                 // free: the previous block ended with a wait
	if (C == 2) for (uint32_t i = 0; i < n_frames; ++i) { il[2 * i] = ch[0][i]; il[2 * i + 1] = ch[1][i]; }
	else if (C == 1) memcpy (il, ch[0], (size_t) n_frames * sizeof (float));
	else for (uint32_t i = 0; i < n_frames; ++i) for (uint32_t c = 0; c < C; ++c) il[(size_t) i * C + c] = ch[c][i];
	HIPCHK (hipMemcpyAsync (e->stage.p, il, total * sizeof (float), hipMemcpyHostToDevice, st));
	const int rc = process_call (e, { e->stage.p, n_frames, n_frames, st, 0, 1, nullptr, false, true });
	if (rc) return rc;
	{ const int jrc = join_tail (e, st); if (jrc) return jrc; }     // (a deferred gate — tail mode 2 only, at this size — writes the state copied next)
	HIPCHK (hipMemcpyAsync (e->pin_state.p, e->state.p, sizeof (mtr_stream_state), hipMemcpyDeviceToHost, st));
	if (e->cfg.meters & MTR_METER_SPECTR30) {
		HIPCHK (hipMemcpyAsync (e->pin_bank.p, e->bank.val.p, MTR_NBANDS * sizeof (float), hipMemcpyDeviceToHost, st));
		HIPCHK (hipMemcpyAsync (e->pin_bank.p + MTR_NBANDS, e->bank.max.p, MTR_NBANDS * sizeof (float), hipMemcpyDeviceToHost, st));
	}
	HIPCHK (hipStreamSynchronize (st));
	e->snap_valid = true;
	return MTR_OK;
}

int mtr_engine_prepare_host (mtr_engine* e, uint32_t max_block_frames)
{
	if (!e) return fail (MTR_ERR_ARG, "null engine");
	if (e->cfg.n_streams != 1) return fail (MTR_ERR_ARG, "mtr_engine_prepare_host is for the n_streams == 1 (LV2) path");
	if (max_block_frames == 0) return MTR_OK;
	// one silent block of the largest size: page-locked staging, device buffers, the engine's stream and every kernel's
	// code object exist afterwards (a first launch loads the module: milliseconds); then back to the state of a new engine
	std::vector<float> zeros (max_block_frames, 0.f);
	const float* ch[MTR_MAX_ENGINE_CHANNELS];
	for (const float*& p : ch) p = zeros.data ();
	int rc = mtr_engine_process_planar_host (e, ch, max_block_frames);
	if (rc) return rc;
	return mtr_engine_reset (e);
}

} // extern "C"
