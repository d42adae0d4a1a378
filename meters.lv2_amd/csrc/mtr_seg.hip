// mtr_seg.hip — K-weighting + true peak with LANE = TIME SEGMENT (gfx950), layout 7: the batch path.
//
// Replaces, for a whole batch, Ebu_r128_proc::detect_process (ebumeter/ebu_r128_proc.cc:302-337) and
// Resampler::process + TruePeakdsp::process_max (zita-resampler/resampler.cc:211-235, jmeters/truepeakdsp.cc:101-124),
// like k_kwtp16 (mtr_fused4.hip), whose arithmetic it shares: the K-weighting step is the reference's recurrence in f32,
// the interpolator runs on v_mfma_f32_16x16x32_f16 with samples and taps split into two f16 halves and three of the
// four partial products kept (mtr_mfma16_fir.h).
//
// What is different is the decomposition.  k_kwtp16 gives a wave ONE stream and its 64 lanes consecutive 38-frame runs
// of one 50 ms tile: the serial K-filter then needs an end-state pass, a DPP scan and a masked second pass (22 packed
// instructions per frame instead of the recurrence's 11), every tile has serial phases (scale reduction, split, pass 1,
// scan, pass 2, products), and its two waves per SIMD take turns (tools/f4_census.py: 1353 VALU + 342 MFMA + 361 SALU per
// tile).  Here a lane owns a whole TIME SEGMENT of a stream (the 64 lanes of a wave = 64 (stream, segment) units) and
// walks it 16 frames per step:
//   * the K-filter is the plain recurrence, 11 packed instructions per frame, state in registers; a segment that does
//     not start the call is warmed up over the 0.075 s in front of it (slowest pole 0.99502 per sample: 1.6e-8;
//     k_kwtp16 warms its own time segments the same way), segment 0 starts from the carried state;
//   * the 16 new frames of a lane are ONE column of the block-Toeplitz product: rows = the 16 outputs, window = the
//     lane's last 64 samples, which sit in a four-slot ring in LDS (f16 hi / lo words, 128 bytes per column and
//     array, 16-byte chunks XOR-swizzled by the column: conflict-free ds_read_b128 / ds_write_b128).  One step = 64 columns = 4 blocks x 2 channels x 18 MFMAs;
//   * the scale of a column is its lane's own: a power of two that puts the segment's running maximum into
//     [2^3, 2^15) — it only ever shrinks, and when it must (a sample 2^12 above what the scale was made for) the lane's
//     ring words are rescaled in place (exact: a power of two) and the peaks so far leave the scaled domain.  An Inf
//     or NaN sample poisons only the columns it reaches;
//   * no tile phases: every step is the same code, and the products of step j - 1 run UNDER the scalar and packed work
//     of step j in one instruction stream (one wave per SIMD, all the registers, 38 KB of LDS) — the MFMA shadows
//     carry the split, the maxima and a quarter of the recurrence (tools/issue_model.hip: two independent full-rate or
//     one half-rate VALU instruction per 16x16x32 MFMA cost 2 cycles; a packed-f32 one waits for the matrix pipe), the
//     rest of the recurrence is one packed block per step, software-pipelined over frames;
//   * loads: lane l reads its own 128 bytes per step (8 x global_load_dwordx4, one cache line), three steps ahead.
//
// The launch covers the whole 50 ms tiles of a call, n_main per lane; the rest of a fragment the call started in (`head`
// frames in front of the first tile) and what is left behind the last whole tile go to k_kwtp16 in the same stream order
// (mtr_engine.hip).  A tile need not be a whole number of steps (44.1 / 88.2 kHz): see ALIGNED below.  Σ y² per tile leaves through tile_power exactly as from k_kwtp16, so k_gate does
// not know which kernel ran.
#include <hip/hip_runtime.h>

#include <type_traits>
#include <utility>

#include "mtr_internal.h"
#include "mtr_mfma16_fir.h"
#include "mtr_wave.h"

// -DMTR_SEG_PROF: shader cycles per part of a step, summed over one wave's main loop (tools/seg_prof.py)
#ifdef MTR_SEG_PROF
__device__ unsigned long long g_seg_prof[10];
#define SPROF_NOW(v) unsigned long long v; asm volatile ("s_memtime %0\n s_waitcnt lgkmcnt(0)" : "=s"(v) :: "memory")
#define SPROF_ADD(i, d) sprof_[i] += (d)
#else
#define SPROF_NOW(v)
#define SPROF_ADD(i, d)
#endif

namespace {

constexpr int R     = MTR_SEG_STEP;          // frames per lane and step = one MFMA column
constexpr int COLB  = 128;                   // bytes per column and array: 4 ring slots x 32; the eight 16-byte chunks of a column sit at
                                             // chunk ^ (column & 7): conflict-free in ds_read_b128's 16-lane groups and ds_write_b128's 8-lane groups
constexpr int ARRB  = 64 * COLB;             // one array: HL | HR | LL | LR
constexpr int BLKB  = 16 * COLB;             // 16 columns = one MFMA block
constexpr int XCHG  = 4 * ARRB;              // exchange area: float [2 ch][4 blocks][4 kg][16 c]
constexpr int XEPS  = XCHG + 2048;           // ... and the screen's bounds: float [16 c][4 blocks][2 ch]
constexpr int XREF  = XEPS + 512;            // ... and its stream references, the same layout
constexpr int LDS_BYTES = XREF + 512;

typedef unsigned char lds_u8;          // (generic pointers into the dynamic LDS block: the compiler infers the address space)

__device__ __forceinline__ float max3abs (float m, float a, float b) { return fmaxf (fmaxf (m, fabsf (a)), fabsf (b)); }
// The maximum of two floats that are neither negative nor NaN — such floats order as their bit patterns do, and the maximum is
// the same bits (denormals are kept) — without the canonicalising v_max x, x that fmaxf puts in front of an operand it cannot
// prove quiet.  For pk0, rml, rmr and the maxima of |x| they take: each comes out of a maximum seeded with +0, which drops NaNs.
__device__ __forceinline__ float umaxf (float a, float b) { return __uint_as_float (max (__float_as_uint (a), __float_as_uint (b))); }
__device__ __forceinline__ v2f fma2 (v2f a, v2f b, v2f c) { return __builtin_elementwise_fma (a, b, c); }
__device__ __forceinline__ v2f scrub (v2f v) { return v2f{isfinite (v.x) ? v.x : 0.f, isfinite (v.y) ? v.y : 0.f}; }

// The scale of one channel of one lane.  A running maximum with exponent field e goes to [2^3, 2^4); the scale stands
// until a sample reaches 2^15 under it (cap = the bit pattern of that sample: non-negative floats order as uints, an
// Inf sets cap above every pattern).
struct Scale {
	float sc, un;          // scale, 2^-15 / scale
	uint32_t cap;
	__device__ __forceinline__ void set (float mx)
	{
		const int e = (int) (__float_as_uint (mx) >> 23);
		const int se = min (238, 257 - e);
		sc = __uint_as_float ((uint32_t) se << 23);
		un = __uint_as_float ((uint32_t) (239 - se) << 23);
		cap = (uint32_t) (269 - se) << 23;
	}
};

// The screen (SCREEN below): a chunk's first product F = sum Ghi Xhi, and the bound on what the other two can add to any of
// its outputs, |Y - F| <= eps = SCREEN_K_REL * M + SCREEN_K_ABS, in the accumulators' unit (x scale * 2^15).  M = the lane's running
// maximum of |x| since its segment's first history frame, in the column's current scale: it bounds every sample of the column's
// 64-sample window.  With h = x * scale, |h| <= M, for every word of the ring (fresh, or rescaled in place by 2^-12 and below):
//     |Xhi| <= (1 + 2^-11) M + 2^-24,     |Xlo| <= 2^-11 (1 + 2^-11) M + 2^-24 (1 + 2^-12)
// (round to nearest f16 with its subnormals: half an ulp, relative 2^-11 or absolute 2^-25, per rounding — the split's two and
// the rescale's one; the lo word is x - Xhi, exact in f32, rounded once by v_fma_mix).  The taps' halves (g * 2^15) have L1
// norms per row LH = sum |Ghi| <= 84157 and LL = sum |Glo| <= 11.41 (tests/test_seg_screen_bound.py recomputes both from
// mtr_setup's table), so the exact rest sum Ghi Xlo + Glo Xhi is at most
//     (LH 2^-11 + LL) (1 + 2^-11) M + (LH + LL) 2^-24 (1 + 2^-12)  =  52.53 M + 0.00503.
// The four MFMAs that add it round in f32: each by at most 2^-17 (|C| + sum |products|) — 33 additions that truncate, twice
// over — and |C| + sum |products| <= (LH + LL) ((1 + 2^-11) M + 2^-24) + 52.6 M, so 4 x 2^-17 x 84210 M = 2.57 M more:
// 55.10 M + 0.0051 in all, rounded up to 56 M + 2^-7 (the 1.6 % also covers the f32 rounding of eps itself).  Products of f16
// are exact in f32 and no partial sum of them is an f32 subnormal (the smallest is 2^-48), so nothing else rounds.
constexpr float SCREEN_K_REL = 56.0f;
constexpr float SCREEN_K_ABS = 0.0078125f;

// The core screen (CORE below, a.screen == 4): the screen's product is F' = sum over the row's CORE of Ghi Xhi — the taps of a row that
// lie inside one 32-sample stretch of the window (mtr_mfma16_fir.h: mtr_m16_build_core; the interpolator is a windowed sinc, its mass
// sits in the middle of the 48 taps) — one MFMA from a zero accumulator per row, and the bound is |Y - F'| <= eps' = CORE_K_REL * M +
// CORE_K_ABS, with Y = m16::block's computed value on the same ring words and M as above.  F' is no prefix of the dense
// accumulation any more, so the bound is built from the exact sums: with Ye = sum Ghi Xhi + sum Ghi Xlo + sum Glo Xhi and Fe = the
// core's exact sum,  |Y - F'| <= |Y - Ye| + |Ye - Fe| + |Fe - F'|.
//   * |Ye - Fe| is the exact rest, above: 52.53 M + 0.00503, plus the dropped taps' share of the first product: with LT = the largest
//     row sum of |Ghi| outside the row's stretch, 854.62 in tap units (0.02608 of a full-scale sample; tests/test_seg_core_bound.py
//     recomputes it from mtr_setup's table) and the bound on |Xhi| above,  LT ((1 + 2^-11) M + 2^-24) = 855.04 M + 0.000051.
//   * |Y - Ye|: all SIX dense MFMAs round, each by at most 2^-17 (|C| + sum |products|) as above, and |C| + sum |products| <=
//     (LH + LL) ((1 + 2^-11) M + 2^-24) + 52.6 M = 84262.1 M + 0.00502:  6 x 2^-17 x that = 3.858 M + 2.3e-7.
//   * |Fe - F'|: an output lies in ONE of a chunk's three core MFMAs, which starts from zero over at most LH ((1 + 2^-11) M + 2^-24):
//     2^-17 x that = 0.643 M + 4e-8.
// In all 912.06 M + 0.00508, rounded up to 920 M + 2^-7 (0.87 % and 2^-7 - 0.0051: the f32 rounding of eps' itself, one fmaf and
// the product M = rml * sc before it, is 2^-23 relative).  What was said of the screen and of its reference, re-read against F':
//   * the per-word bounds hold for every ring word, fresh or rescaled, so they hold for the words under the dropped taps: a rescale
//     inside a window changes nothing (M is in the column's current scale and bounds all 64 samples of the window).
//   * Products of f16 are exact in f32 and none of their partial sums is subnormal, for 32 products as for 64.
//   * NaN: a NaN word under a row's dropped taps leaves that row's F' finite where Y is NaN (every row of the dense product
//     multiplies every word of the window, by a zero tap if by no other).  The dense fold drops that Y, so a pass loses nothing; a
//     fail completes the chunk as the dense form computes it.  A NaN inside the stretch is dropped from the vote's maximum, as before.
//   * Inf: an Inf sample makes M, and with it eps', Inf for the rest of the lane's segment — fl (c + eps') < pk is false whatever
//     pk — so every chunk of a column that has seen one completes, as with eps; what F' holds does not matter.
//   * R': fl (F' + eps') <= (LH + 920) 2^27 stays far below FLT_MAX, and >= eps' >= 2^-7, so the two remarks on an R' that
//     overflows or is subnormal stand.  pm, pkf and R never receive F' — only completed chunks' dense values — so nothing else moves.
// The vote does not care which rows a lane holds: lane (c, kg) votes with rows 16 w + 4 kg .. + 3 (w = 0..2) of column c against
// pm of its own lane and R' of the column, both values the launch counts for the column's (stream, channel), and a chunk
// completes where any lane of any of its columns fails.  The core form screens the chunks form 3 does and completes more of them.
constexpr float CORE_K_REL = 920.0f;
constexpr float CORE_K_ABS = 0.0078125f;

// The screen's stream reference.  k_seg's result is the maximum per (stream, channel) of what its lanes count (tp_call, at the
// end): a chunk none of whose outputs can exceed a value already counted for the same (stream, channel) cannot change it, even
// where it would set a record of its own accumulator lane.  So the vote takes, besides the lane's own pm, R = the largest value
// the lanes of the column's stream in this wave have counted so far: each owner lane offers max (pk0, pkf) where its peak counts
// (live and peak_ok; otherwise +0, which every peak already bounds), the lanes of an aligned 16-lane row take the maximum of the
// offers of their own stream (four DPP steps, each taken only from a partner of the same stream: a subset of the stream's lanes,
// which is all a bound needs — streams that straddle rows or waves need nothing across them), every fourth step (a stale R is
// still counted), and the owner converts it into the column's unit each step, R * scale * 2^15, through LDS next to eps.  Then
//     fl (F + eps) < max (pm, R')   =>   |Y| <= F + eps < R' (or pm)   =>   the dense peak is the same bits.
//   * R holds only values of this launch that its final atomicMax counts for that (stream, channel) (pk0 and pkf only grow), never
//     a hold or a previous call's peak, and no !peak_ok lane (LEN: those segments go to k_kwtp16_len) feeds it.
//   * NaN: pk0 and pkf never hold one (fmaxf drops it, conservatively), and the vote's fmaxf would drop a NaN R too; the vote's maximum of |F|
//     drops NaNs as the dense fold does (a lane whose twelve values are all NaN votes with +0), and an Inf among them fails it.  The offers are non-negative floats, so their maximum is the unsigned one of their bit patterns.
//   * An Inf sample: R becomes Inf (where its phase 0 counts), every finite chunk passes and Inf ones fail; the result is Inf
//     either way.
//   * R' overflows to +Inf where R * scale * 2^15 >= 2^128: a finite fl (F + eps) <= FLT_MAX lies below the true R', so a pass is
//     still exact.  R' rounds only where it is subnormal, and then it cannot decide a vote: fl (F + eps) >= eps >= 2^-7.  A normal
//     R' is exact (a power of two times a float).
//   * The scale: R' is written in the step that runs and checks the chunks, after its rescale — in the scale of every chunk checked
//     there (a step votes on all eight of its chunks and completes the failing ones itself: none is pending at the next rescale).
// A wave in the bench's shape (8 segments per stream) holds 8 streams; their quiet segments stop completing against their own
// small records.  tests/test_gpu_seg_stream_reference.py holds the screened form to the dense one bit for bit.
//
// Completed interpolated peaks in the reference (a.screen == 2, 3 and 4 — LAZY and CORE below, the latter the default; 1 is the rule without them).  pkf receives
// interpolated values only in flush_pm, at a rescale and at the end of the launch, so under rule 1 R is in effect the stream's SAMPLE
// peak: what completed chunks have found lives in pm, per accumulator lane (one column, four rows of the step), and every chunk
// of the stream with a first product between the sample peak and the true peak found so far completes again, lane by lane, until
// each of the 64 accumulator lanes has met such a value itself.  Rule 2: a step that has completed chunks runs flush_pm's exchange
// without clearing pm (peek_pm), in front of its ring stores, so the owners' pkf — and with it R, at its next refresh — holds what the
// stream's completed chunks have found so far.  Why the launch's result is still the dense bits:
//   * The same final value.  pkf only ever receives fl (pm * un); pm only grows until a flush clears it, and x -> fl (x * un) is
//     monotone (un a power of two), so an early peek adds nothing that the next flush_pm — there is always one behind it, at a
//     rescale or at the end of the launch — would not deliver: max (pk0, pkf) at the end is the same float, subnormal results
//     included.  pm is left as it is because a cleared pm would be wrong for the lanes that offer nothing — the shadow lanes of a
//     partly filled last wave and the !peak_ok lanes: with pm = 0 and R = 0 they would fail every vote from then on.
//   * R still holds only values this launch counts for that (stream, channel).  pm of column 16 b + c holds outputs of that column
//     alone (completed chunks fold in the dense order, the launch's last step masks its rows as the dense form does), and they are
//     what the column's final atomicMax counts.  The offer stays gated by live && peak_ok: a !peak_ok lane's peeked pkf (its
//     chunk completes where a neighbouring column fails) is neither offered nor stored.  pkf, pm and R start every launch at zero.
//   * The scale.  pm is always in the column's current scale (a rescale flushes and clears it first, and the peek runs behind the
//     step's rescale, in the step that completed the chunks); the owner converts with its own current un.  Every lane writes all
//     eight of its exchange words in every peek, so no word of an older scale or of an earlier flush_pm is read.
//   * NaN, Inf: pm and pkf never hold a NaN (the folds' and the peek's fmaxf drop it); an Inf in pm makes pkf and R Inf, which the
//     argument above already covers.
//   * The conversion: R' = R * scale * 2^15 against pm of the same column — equal where nothing underflows (powers of two).  Where
//     pm * un is a subnormal, pkf is its rounding, a value the launch counts, and the pass is exact as for any R: |Y| < R' gives
//     fl (|Y| un) <= fl (R' un) = R by monotonicity.  Where R' itself underflows it is smaller than the true one or cannot decide
//     a vote (eps >= 2^-7, above): more completions, never fewer.
// tests/test_gpu_seg_ref_completed.py holds rules 2 and 1 to the dense form bit for bit on streams whose peaks are inter-sample values;
// tools/seg_screen_model.py is the host model the rule was chosen with (completions 4.35 / 7.84 / 3.90 % -> 0.43 / 0.51 / 1.30 % of
// the chunks on the bench's three signals, profiles/r28_kseg_ref_completed/).

struct KCoef { v2f a0, a1, a2, b1, b2, c3, c4, eps; };
struct KState { v2f z1, z2, z3, z4, sj; };

// ebu_r128_proc.cc:321-327 for both channels of a frame; the association of mtr_kw_steps.h's hand-scheduled pair
__device__ __forceinline__ void kstep (const KCoef& k, KState& s, v2f p)
{
	v2f t = p + k.eps;
	v2f u = k.a1 * s.z1;
	t = fma2 (-k.b2, s.z2, t);
	u = fma2 (k.a2, s.z2, u);
	const v2f x = fma2 (-k.b1, s.z1, t);
	u = fma2 (-k.c4, s.z4, u);
	s.z4 = s.z4 + s.z3;
	u = fma2 (-k.c3, s.z3, u);
	const v2f y = fma2 (k.a0, x, u);
	s.z3 = s.z3 + y;
	s.sj = fma2 (y, y, s.sj);
	s.z2 = s.z1; s.z1 = x;
}

// The recurrence of one step — 16 frames x 11 operations — as ONE sequence for the hand-placed schedule of the main loop,
// software-pipelined over frames: the x-chain of frame n + 1 (operations 0..4: it only needs x (n), x (n - 1)) runs between the
// y-chain of frame n (5..10), so that no operation reads the result of one of its two predecessors (a dependent packed
// operation issues after 8 cycles, an independent one after 5: tools/issue_model.hip).  Same operations, same operands,
// same association as kstep — only their order in the instruction stream differs.
//     0: t = p + eps         1: u = a1 z1          2: t -= b2 z2        3: u += a2 z2       4: x = t - b1 z1
//     5: u -= c4 z4          6: z4 += z3           7: u -= c3 z3        8: y = a0 x + u     9: z3 += y      10: sj += y y
constexpr int KOPS = 11 * R;
struct KSeq {
	int frame[KOPS], op[KOPS];
	constexpr KSeq () : frame{}, op{}
	{
		int n = 0;
		for (int o = 0; o < 5; ++o) { frame[n] = 0; op[n] = o; ++n; }
		constexpr int ord[11][2] = { {5, 0}, {0, 1}, {6, 0}, {7, 0}, {1, 1}, {2, 1}, {8, 0}, {3, 1}, {4, 1}, {9, 0}, {10, 0} };
		for (int f = 0; f < R; ++f)
			for (int i = 0; i < 11; ++i) {
				if (ord[i][1] && f + 1 == R) continue;
				frame[n] = f + ord[i][1]; op[n] = ord[i][0]; ++n;
			}
	}
};
constexpr KSeq kseq_tab{};
struct KWork { v2f t[R], u[R], y[R], x[R + 2]; };         // x[f + 2] = x of frame f; x[0], x[1] = z2, z1 carried into the step
template <int OP>
__device__ __forceinline__ void kopx (const KCoef& k, KState& s, KWork& w, const v2f (&p)[R], int f)
{
	if constexpr (OP == 0) w.t[f] = p[f] + k.eps;
	else if constexpr (OP == 1) w.u[f] = k.a1 * w.x[f + 1];
	else if constexpr (OP == 2) w.t[f] = fma2 (-k.b2, w.x[f], w.t[f]);
	else if constexpr (OP == 3) w.u[f] = fma2 (k.a2, w.x[f], w.u[f]);
	else if constexpr (OP == 4) w.x[f + 2] = fma2 (-k.b1, w.x[f + 1], w.t[f]);
	else if constexpr (OP == 5) w.u[f] = fma2 (-k.c4, s.z4, w.u[f]);
	else if constexpr (OP == 6) s.z4 = s.z4 + s.z3;
	else if constexpr (OP == 7) w.u[f] = fma2 (-k.c3, s.z3, w.u[f]);
	else if constexpr (OP == 8) w.y[f] = fma2 (k.a0, w.x[f + 2], w.u[f]);
	else if constexpr (OP == 9) s.z3 = s.z3 + w.y[f];
	else s.sj = fma2 (w.y[f], w.y[f], s.sj);
}

// The lo word of the f16 split (mtr_mfma16_fir.h: lo_pair) as two separate instructions, so that the two that share an MFMA's
// shadow are independent (the halves of one word are not: v_fma_mixhi keeps the word's low half).
__device__ __forceinline__ void lo_first (uint32_t& lw, uint32_t hw, float x0)
{
	asm ("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(lw) : "v"(hw), "v"(x0));
}
__device__ __forceinline__ void lo_second (uint32_t& lw, uint32_t hw, float x1)
{
	asm ("v_fma_mixhi_f16 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(lw) : "v"(hw), "v"(x1));
}

// The factor a rescale multiplies a lane's ring words with, and the multiplication itself (two f16 words of one 32-bit word):
// `rescale` below and the lazy form's replay of it (LAZY: lazy_lo) share them, so that a word built late is the ring word bit for bit.
typedef _Float16 seg_h2 __attribute__ ((ext_vector_type (2)));
__device__ __forceinline__ _Float16 rescale_ratio (float sc_new, float sc_old) { return (_Float16) (sc_new / sc_old); }   // 1 or 2^-12 and below (0 under 2^-24)
__device__ __forceinline__ uint32_t rescale_word (uint32_t w, seg_h2 r2)
{
	return __builtin_bit_cast (uint32_t, (seg_h2) (__builtin_bit_cast (seg_h2, w) * r2));
}

// ALIGNED: the tile (a 50 ms fragment) is a whole number of steps — 48, 96, 192, 32 kHz; otherwise (44.1, 88.2 kHz: 2205, 4410 frames)
// the step in which a tile ends is followed by a second run of its recurrence, frame by frame from the state the step started with,
// with the reference's end-of-fragment actions at the exact frame (every other step is the aligned kernel's code).
//
// SCREEN: each chunk runs the first of its three products (Ghi Xhi: MFMAs 0..5) and no more, unless one of its outputs may
// reach the running peak: a lane whose twelve first-product values all stay eps (above) under the peak of its completed
// values (pm) or under its stream's reference (what the launch has already counted for the stream: above) cannot raise the
// result, whatever the other two products add.  A step issues its eight chunks' first products back to back; each chunk's vote
// runs behind the next chunk's MFMAs (chunk 7's behind its own tail), on complete accumulators, and leaves a lane mask, and the
// step branches once, on the OR of the eight.  Every chunk one lane of which failed (an Inf fails; NaNs are dropped, as the dense fold drops them) then runs MFMAs 0..17
// from zero on all four of its operands, read again from the ring — m16::block's order, so bit for bit the dense values — and
// its maxima go into pm as in the dense form.  The step's ring stores (slot U: the oldest quarter of every window of its
// products) come only behind that, so all of a step's windows are intact when a chunk completes, and no step leaves a chunk
// pending: a rescale at the next step's head finds nothing to complete.  A vote reads pm and the bounds of its own step, which
// only its own chunk's completion can change.  The peak is the dense form's on every input; only the time depends on the data.
// The screened step issues no instruction its result does not need: the vote's maximum is six v_max3 (twelve values and a +0), pm
// is one value per block and channel, the maxima of values that are never NaN (pk0, rml, rmr) are unsigned ones, and whether a
// step lies in front of the call's last 24 frames is one scalar compare on the step's index (p0_steps) — 369 - 374 VALU
// instructions per step where there were 395 - 397 (profiles/r23_kseg_trim/).
//
// LEN: the call carries per-stream lengths (a.ends, call-relative: mtr_engine_process_*_lengths).  Every frame at or past a stream's
// end E is read as +0.0f — the global loads behind it are not issued — so the scale, the ring and the recurrence never see what the
// buffer holds there.  The peak of a lane counts only where all of its columns and phase-0 frames lie in front of E - 24: a segment
// that reaches further on a stream the call closes (E < n_frames) keeps its peak to itself, and the engine hands exactly those
// segments' peaks to k_kwtp16_len (a.from_tile: from the first such segment's first tile, masked at E).  A stream the call does not
// touch (E == 0) keeps its K-filter state.  The dense instantiation (LEN false) is the kernel's code as it always was.
//
// LAZY (a.screen == 3, and 4: CORE below; SCREEN without LEN): the screened form without the lo words in its hot path.  Only a chunk that completes
// and the launch's last, dense step read the lo halves of the split, 0.4 - 1.3 % of the chunks, so a step computes and stores
// the hi words alone — no v_fma_mix, no LL / LR store, sixteen registers less — and a completing block builds its lo operands
// on the spot, in the MFMA operand layout, from the stream's f32 samples (lazy_lo, below, with the reason it is exact).
//
// CORE (a.screen == 4, the default; a LAZY form): a chunk's screen is three MFMAs, not six — the taps' 32-sample core, one MFMA per
// 16 of the chunk's 48 rows, each from a zero accumulator and none waiting for another (the core screen, above: F' and eps').  Lane
// (c, kg) multiplies the window's 16-byte chunks kg + 1, kg + 2 and kg + 3: the middle one is fetch_hi's address RA[(U + 1) & 3],
// the two odd ones come from a second address array, RB.  Completions, the launch's last step, the ring, lazy_lo, peek_pm, rescale
// and the scale history are the lazy form's, untouched: only what is multiplied for the vote, and the bound it is held against, differ.
template <bool EBU, bool ALIGNED, bool SCREEN, bool LEN, bool LAZY = false, bool CORE = false>
__global__ __launch_bounds__ (64, 1) void k_seg (const mtr_seg_args a)
{
	static_assert (!LAZY || (SCREEN && !LEN), "the lazy form is a screened one, and calls with per-stream ends stay on form 2");
	static_assert (!CORE || LAZY, "the core form is a lazy one");
	constexpr float KREL = CORE ? CORE_K_REL : SCREEN_K_REL, KABS = CORE ? CORE_K_ABS : SCREEN_K_ABS;   // the vote's bound: eps or eps'
	extern __shared__ __attribute__ ((aligned (16))) unsigned char smem_[];
	lds_u8* const smem = smem_;
	const int lane = threadIdx.x;

	// ---- which (stream, segment) this lane owns --------------------------------------------------------------------------
	const uint32_t n_units = a.n_streams * a.n_segs;
	uint32_t unit = blockIdx.x * 64u + (uint32_t) lane;
	const bool live = unit < n_units;                               // lanes past the batch shadow the last unit, silently
	if (!live) unit = n_units - 1;
	const uint32_t s = unit / a.n_segs, q = unit - s * a.n_segs;
	const uint32_t fq = q * a.seg_base + min (q, a.seg_rem);          // first tile this lane answers for
	const uint32_t cq = a.seg_base + (q < a.seg_rem ? 1u : 0u);
	const uint32_t p0 = fq + cq - a.n_main;                           // first tile it processes (one early where its segment is short)
	const int64_t F0 = (int64_t) p0 * a.tile_frames;
	const v2f* const src = reinterpret_cast<const v2f*> (a.audio) + (size_t) s * a.stride + a.head;   // frame 0 = the launch's first tile
	mtr_stream_state* const st = a.state + s;
	const int n_steps = (int) (((uint64_t) a.n_main * a.tile_frames + R - 1) / R);   // (ALIGNED: n_main tiles of spt steps)
	const int spt = (int) (a.tile_frames / R);
	// Unaligned tiles: a lane's last tile ends last_rows frames into the launch's last step.  What follows is the next segment's
	// (read again there: harmless for a maximum, and the recurrence is rerun to the exact frame, below) — but behind a stream's
	// LAST segment it is the call's tail, another stream, or nobody's memory: those lanes never read it.  The stream pointer
	// (of every lane: the main loop stays uniform) stops one step early, the last step's frames are fetched one by one in front
	// of it — zeros behind the tile's end in a last segment — and the rows of that step's products behind the end do not count.
	const int last_rows = ALIGNED ? R : (int) ((uint64_t) a.n_main * a.tile_frames - (uint64_t) (n_steps - 1) * R);   // 1 .. 16, wave-uniform
	const bool cut = last_rows < R;
	const bool lastq = !ALIGNED && q == a.n_segs - 1;
	const int n_loads = n_steps - (cut ? 1 : 0);                      // steps the stream pointers walk
	// LEN: the stream's end relative to `src`; does this lane's peak count (see above)?
	const int64_t e_src = LEN ? (int64_t) a.ends[s] - (int64_t) a.head : 0;
	const bool closing = LEN && e_src < a.p0_end + 24;
	const bool peak_ok = !closing || (int64_t) (fq + cq) * a.tile_frames + 24 <= e_src;

	KCoef kc;
	kc.a0 = a.a0; kc.a1 = a.a1; kc.a2 = a.a2; kc.b1 = a.b1; kc.b2 = a.b2; kc.c3 = a.c3; kc.c4 = a.c4; kc.eps = 1e-15f;
	KState ks;
	ks.z1 = 0; ks.z2 = 0; ks.z3 = 0; ks.z4 = 0; ks.sj = 0;
	if (EBU && q == 0) {
		ks.z1 = v2f{st->kz[0], st->kz[1]}; ks.z2 = v2f{st->kz[2], st->kz[3]};
		ks.z3 = v2f{st->kz[4], st->kz[5]}; ks.z4 = v2f{st->kz[6], st->kz[7]};
	}

	// ---- the stream: four register buffers of 16 frames, loaded three steps ahead ------------------------------------------
	const bool warm = EBU && q > 0;
	typedef float f4v_ __attribute__ ((ext_vector_type (4)));
	typedef f4v_ float4_a8 __attribute__ ((aligned (8)));              // (a segment may start on any frame: 8-byte alignment is all there is)
	const float4_a8* lp = reinterpret_cast<const float4_a8*> (src + F0 - (warm ? (int64_t) a.warm_steps * R : 0));
	v2f xq[4][R];
	const float4_a8* const lp_base = reinterpret_cast<const float4_a8*> (src);
	auto load = [&]<int B> () __attribute__ ((always_inline)) {
		if constexpr (LEN) {
			// frames of this line in front of the stream's end: all of them but in the one line that holds the end
			const int64_t left = e_src - 2 * (int64_t) (lp - lp_base);
			if (__builtin_expect (left >= R, 1)) {
#pragma unroll
				for (int i = 0; i < R / 2; ++i) {
					const f4v_ v = lp[i];
					xq[B][2 * i] = v2f{v.x, v.y}; xq[B][2 * i + 1] = v2f{v.z, v.w};
				}
			} else {
				const int nl = (int) max (left, (int64_t) 0);
#pragma unroll
				for (int i = 0; i < R / 2; ++i) {
					f4v_ v = f4v_{0.f, 0.f, 0.f, 0.f};
					if (2 * i < nl) v = lp[i];
					if (2 * i + 1 >= nl) { v.z = 0.f; v.w = 0.f; }
					xq[B][2 * i] = v2f{v.x, v.y}; xq[B][2 * i + 1] = v2f{v.z, v.w};
				}
			}
		} else {
#pragma unroll
		for (int i = 0; i < R / 2; ++i) {
			const f4v_ v = lp[i];        // (plain loads: the eight 16-byte reads of a lane's line merge in the L1 — as nt loads they go to the L2 one by one: 17.4 ms)
			xq[B][2 * i] = v2f{v.x, v.y}; xq[B][2 * i + 1] = v2f{v.z, v.w};
		}
		}
	};
	load.template operator()<0> (); lp += R / 2;
	load.template operator()<1> (); lp += R / 2;
	load.template operator()<2> (); lp += R / 2;

	m16::AFrag A;
	A.load (a.mfma_a, lane);
	// the twelve tap fragments live in accumulation registers for the whole kernel: the matrix pipe reads them there, and the
	// 48 architectural registers they would take are what the step's working set needs (otherwise the register allocator
	// parks some fragments in AGPRs anyway and copies one back per chunk: 32 v_accvgpr_read per step; measured -1.5 %)
#pragma unroll
	for (int f = 0; f < MTR_M16_FRAGS; ++f) asm volatile ("" : "+a"(A.a[f]));
	// CORE: the three core fragments, which sit behind the twelve in the table, live there too
	m16::h8 AC[MTR_M16_CORE_FRAGS];
	if constexpr (CORE) {
#pragma unroll
		for (int w = 0; w < MTR_M16_CORE_FRAGS; ++w) {
			AC[w] = *reinterpret_cast<const m16::h8*> (a.mfma_a + (MTR_M16_FRAGS + w) * 512 + lane * 8);
			asm volatile ("" : "+a"(AC[w]));
		}
	}

	// ---- K-filter warm-up of the segments that do not start the call (warm_steps is a multiple of 4) -------------------------
	if (warm) {
		for (uint32_t w = 0; w < a.warm_steps; w += 4) {
			/* (the recurrence in the main loop's software-pipelined order — the x-chain of frame n + 1 between the y-chain of frame n: \
			 * the same operations on the same operands, 5 cycles apiece instead of the 8 a dependent packed pair takes) */ \
#define MTR_WARM(B)                                                              \
			{                                                                        \
				KWork kw_;                                                           \
				kw_.x[0] = ks.z2; kw_.x[1] = ks.z1;                                  \
				[&]<int... Is> (std::integer_sequence<int, Is...>) __attribute__ ((always_inline)) { \
					(kopx<kseq_tab.op[Is]> (kc, ks, kw_, xq[B], kseq_tab.frame[Is]), ...); \
				} (std::make_integer_sequence<int, KOPS>{});                         \
				ks.z2 = kw_.x[R]; ks.z1 = kw_.x[R + 1];                              \
				load.template operator()<(B + 3) & 3> (); lp += R / 2;                \
			}
			MTR_WARM (0) MTR_WARM (1) MTR_WARM (2) MTR_WARM (3)
#undef MTR_WARM
		}
		ks.z1 = scrub (ks.z1); ks.z2 = scrub (ks.z2); ks.z3 = scrub (ks.z3); ks.z4 = scrub (ks.z4);
		ks.sj = 0;
	}

	// ---- the ring: 48 frames in front of the segment (history of the previous call for segment 0) ---------------------------
	const int cc = lane & 15, kg = lane >> 4;
	int RA[4];                                                        // operand read address of window quarter v, this lane
#pragma unroll
	for (int v = 0; v < 4; ++v) RA[v] = cc * COLB + ((((kg & 1) + 2 * ((v + (kg >> 1)) & 3)) ^ (cc & 7)) * 16);
	// CORE: ... and of the window's 16-byte chunk 2 v + kg + 1, the odd neighbours of the core's middle chunk (RA[v + 1] is chunk
	// 2 v + kg + 2): the same swizzle, and a b128 lane group shares kg, so these reads are conflict-free as well
	int RB[4];
	if constexpr (CORE) {
#pragma unroll
		for (int v = 0; v < 4; ++v) RB[v] = cc * COLB + (((((kg + 1) & 1) + 2 * ((v + ((kg + 1) >> 1)) & 3)) ^ (cc & 7)) * 16);
	}
	const int WA = lane * COLB;                                       // this lane's column
	int WS[4];                                                        // ... and where the first half of ring slot s sits in it (the second: ^ 16)
#pragma unroll
	for (int sl = 0; sl < 4; ++sl) WS[sl] = WA + (((2 * sl) ^ (lane & 7)) * 16);

	Scale scl, scr;
	// LAZY: the scales' exponent fields, and those of the last four steps (byte k = the scale step j - 1 - k split its words in, as
	// seen from step j's completions; pushed at the end of every step: one v_lshl_or_b32 per channel)
	uint32_t sel_ = 0, ser_ = 0, shl_ = 0, shr_ = 0;
	v2f pk0 = v2f{0.f, 0.f};                                           // phase 0: max |x[n - 24]|, exact
	v2f pkf = v2f{0.f, 0.f};                                           // interpolated peaks that have left the scaled domain
	float pm[4][2][2];                                                // running |max| of the accumulators, scaled, per block and channel: two
	                                                                  // independent chains each (two dependent v_max3 in one MFMA's shadow cost 3 cycles).
	                                                                  // SCREEN folds only behind the step's branch, under no MFMA, and every reader
	                                                                  // (the vote, flush_pm) takes the maximum of the two: the fold leaves that
	                                                                  // maximum in [0] and +0 in [1] — the same bits, eight registers less
#pragma unroll
	for (int b = 0; b < 4; ++b) { pm[b][0][0] = 0.f; pm[b][0][1] = 0.f; pm[b][1][0] = 0.f; pm[b][1][1] = 0.f; }

	float rml = 0.f, rmr = 0.f;                                       // SCREEN: max |x| of the segment so far (history frames included), per channel
	uint32_t n_scr = 0, n_fin = 0;                                    // ... chunks screened / completed (wave-uniform)
	uint32_t refl = 0, refr = 0;                                      // ... the stream's reference (float bits, unscaled), per channel
	// ... the lanes it is taken from: the partners of the four DPP steps that meter the same stream, and whether this lane's peak counts
	const bool ref_own = live && peak_ok;
	const bool ref_q1 = SCREEN && (uint32_t) __builtin_amdgcn_mov_dpp ((int) s, 0xB1, 0xF, 0xF, false) == s;   // quad_perm [1,0,3,2]
	const bool ref_q2 = SCREEN && (uint32_t) __builtin_amdgcn_mov_dpp ((int) s, 0x4E, 0xF, 0xF, false) == s;   // quad_perm [2,3,0,1]
	const bool ref_hm = SCREEN && (uint32_t) __builtin_amdgcn_mov_dpp ((int) s, 0x141, 0xF, 0xF, false) == s;  // row_half_mirror
	const bool ref_rm = SCREEN && (uint32_t) __builtin_amdgcn_mov_dpp ((int) s, 0x140, 0xF, 0xF, false) == s;  // row_mirror
	auto ref_row = [&] (uint32_t v) __attribute__ ((always_inline)) {
		uint32_t t;
		t = max (v, (uint32_t) __builtin_amdgcn_update_dpp (0, (int) v, 0xB1, 0xF, 0xF, true));  v = ref_q1 ? t : v;
		t = max (v, (uint32_t) __builtin_amdgcn_update_dpp (0, (int) v, 0x4E, 0xF, 0xF, true));  v = ref_q2 ? t : v;
		t = max (v, (uint32_t) __builtin_amdgcn_update_dpp (0, (int) v, 0x141, 0xF, 0xF, true)); v = ref_hm ? t : v;
		t = max (v, (uint32_t) __builtin_amdgcn_update_dpp (0, (int) v, 0x140, 0xF, 0xF, true)); v = ref_rm ? t : v;
		return v;
	};

	auto split_store = [&] (const v2f (&x)[R], int slot) __attribute__ ((always_inline)) {
		const v2f sc = v2f{scl.sc, scr.sc};
		uint32_t hl[R / 2], hr[R / 2], ll[R / 2], lr[R / 2];
#pragma unroll
		for (int i = 0; i < R / 2; ++i) {
			const v2f u = x[2 * i] * sc, v = x[2 * i + 1] * sc;
			m16::split_pair (u.x, v.x, hl[i], ll[i]);
			m16::split_pair (u.y, v.y, hr[i], lr[i]);
		}
		lds_u8* const w0 = smem + WS[slot];
		lds_u8* const w1 = smem + (WS[slot] ^ 16);
		*reinterpret_cast<uint4*> (w0)            = uint4{hl[0], hl[1], hl[2], hl[3]};
		*reinterpret_cast<uint4*> (w1)            = uint4{hl[4], hl[5], hl[6], hl[7]};
		*reinterpret_cast<uint4*> (w0 + ARRB)     = uint4{hr[0], hr[1], hr[2], hr[3]};
		*reinterpret_cast<uint4*> (w1 + ARRB)     = uint4{hr[4], hr[5], hr[6], hr[7]};
		*reinterpret_cast<uint4*> (w0 + 2 * ARRB) = uint4{ll[0], ll[1], ll[2], ll[3]};
		*reinterpret_cast<uint4*> (w1 + 2 * ARRB) = uint4{ll[4], ll[5], ll[6], ll[7]};
		*reinterpret_cast<uint4*> (w0 + 3 * ARRB) = uint4{lr[0], lr[1], lr[2], lr[3]};
		*reinterpret_cast<uint4*> (w1 + 3 * ARRB) = uint4{lr[4], lr[5], lr[6], lr[7]};
	};

	// LAZY: the hi words alone (no lo word is built or stored outside lazy_lo)
	auto split_store_hi = [&] (const v2f (&x)[R], int slot) __attribute__ ((always_inline)) {
		const v2f sc = v2f{scl.sc, scr.sc};
		uint32_t hl[R / 2], hr[R / 2];
#pragma unroll
		for (int i = 0; i < R / 2; ++i) {
			const v2f u = x[2 * i] * sc, v = x[2 * i + 1] * sc;
			hl[i] = m16::hi_pair (u.x, v.x);
			hr[i] = m16::hi_pair (u.y, v.y);
		}
		lds_u8* const w0 = smem + WS[slot];
		lds_u8* const w1 = smem + (WS[slot] ^ 16);
		*reinterpret_cast<uint4*> (w0)        = uint4{hl[0], hl[1], hl[2], hl[3]};
		*reinterpret_cast<uint4*> (w1)        = uint4{hl[4], hl[5], hl[6], hl[7]};
		*reinterpret_cast<uint4*> (w0 + ARRB) = uint4{hr[0], hr[1], hr[2], hr[3]};
		*reinterpret_cast<uint4*> (w1 + ARRB) = uint4{hr[4], hr[5], hr[6], hr[7]};
	};

	{
		const v2f* const hst = reinterpret_cast<const v2f*> (a.hist) + (size_t) s * MTR_FIR_HALO;
		v2f px[3][R];
#pragma unroll
		for (int k = 0; k < 3; ++k)
#pragma unroll
			for (int n = 0; n < R; ++n) {
				const int64_t f = F0 - 48 + R * k + n;
				const int64_t fc = f + (int64_t) a.head;                     // the call's own frame; in front of it: the history
				px[k][n] = fc >= 0 ? ((!LEN || f < e_src) ? src[f] : v2f{0.f, 0.f}) : (fc >= -MTR_FIR_HALO ? hst[fc + MTR_FIR_HALO] : v2f{0.f, 0.f});
			}
		float ml = 0.f, mr = 0.f;
#pragma unroll
		for (int k = 0; k < 3; ++k)
#pragma unroll
			for (int n = 0; n < R; n += 2) { ml = max3abs (ml, px[k][n].x, px[k][n + 1].x); mr = max3abs (mr, px[k][n].y, px[k][n + 1].y); }
		scl.set (ml); scr.set (mr);
		rml = ml; rmr = mr;
		if constexpr (LAZY) {
			sel_ = __float_as_uint (scl.sc) >> 23; ser_ = __float_as_uint (scr.sc) >> 23;
			shl_ = sel_ * 0x01010101u; shr_ = ser_ * 0x01010101u;
			split_store_hi (px[0], 1); split_store_hi (px[1], 2); split_store_hi (px[2], 3);
		} else {
		split_store (px[0], 1); split_store (px[1], 2); split_store (px[2], 3);
		}
		if (F0 == 0) {
			// phase 0 of the launch's first outputs is frames -24 .. -1: the history of a launch that starts the call, else the
			// call's own frames in front of it (whose owner, the kernel of the call's head, stops 24 frames short of them)
#pragma unroll
			for (int n = 8; n < R; ++n) pk0 = v2f{fmaxf (pk0.x, fabsf (px[1][n].x)), fmaxf (pk0.y, fabsf (px[1][n].y))};
#pragma unroll
			for (int n = 0; n < R; ++n) pk0 = v2f{fmaxf (pk0.x, fabsf (px[2][n].x)), fmaxf (pk0.y, fabsf (px[2][n].y))};
		}
	}

	// ---- pieces of a step ---------------------------------------------------------------------------------------------------
	// the accumulators' running maxima leave the scaled domain: pm (accumulator layout: lane (c, kg), block b = column
	// 16 b + c) -> pkf of the lane that owns the column, through the exchange area
	auto flush_pm = [&] () __attribute__ ((always_inline)) {
		float* const X = reinterpret_cast<float*> (smem_ + XCHG);
#pragma unroll
		for (int b = 0; b < 4; ++b) {
			X[((0 * 4 + b) * 4 + kg) * 16 + cc] = fmaxf (pm[b][0][0], pm[b][0][1]);
			X[((1 * 4 + b) * 4 + kg) * 16 + cc] = fmaxf (pm[b][1][0], pm[b][1][1]);
			pm[b][0][0] = 0.f; pm[b][0][1] = 0.f; pm[b][1][0] = 0.f; pm[b][1][1] = 0.f;
		}
		__builtin_amdgcn_fence (__ATOMIC_RELEASE, "workgroup");
		__builtin_amdgcn_wave_barrier ();
		__builtin_amdgcn_fence (__ATOMIC_ACQUIRE, "workgroup");
		float fl = 0.f, fr = 0.f;
#pragma unroll
		for (int g = 0; g < 4; ++g) {
			fl = fmaxf (fl, X[((0 * 4 + kg) * 4 + g) * 16 + cc]);         // column `lane` = block lane >> 4 (= kg), c = lane & 15
			fr = fmaxf (fr, X[((1 * 4 + kg) * 4 + g) * 16 + cc]);
		}
		pkf = v2f{fmaxf (pkf.x, fl * scl.un), fmaxf (pkf.y, fr * scr.un)};
		__builtin_amdgcn_fence (__ATOMIC_RELEASE, "workgroup");
		__builtin_amdgcn_wave_barrier ();
	};
	// The peek of screen rule 2: flush_pm's exchange with pm left as it is, so that what the chunks completed so far have found
	// reaches the owner's pkf, and with it the stream's reference, while the launch is still running (the stream reference, above).
	// Every lane writes all eight of its words, so the owners read nothing an older exchange left there.
	auto peek_pm = [&] () __attribute__ ((always_inline)) {
		float* const X = reinterpret_cast<float*> (smem_ + XCHG);
#pragma unroll
		for (int b = 0; b < 4; ++b) {
			X[((0 * 4 + b) * 4 + kg) * 16 + cc] = fmaxf (pm[b][0][0], pm[b][0][1]);
			X[((1 * 4 + b) * 4 + kg) * 16 + cc] = fmaxf (pm[b][1][0], pm[b][1][1]);
		}
		__builtin_amdgcn_fence (__ATOMIC_RELEASE, "workgroup");
		__builtin_amdgcn_wave_barrier ();
		__builtin_amdgcn_fence (__ATOMIC_ACQUIRE, "workgroup");
		float fl = 0.f, fr = 0.f;
#pragma unroll
		for (int g = 0; g < 4; ++g) {
			fl = fmaxf (fl, X[((0 * 4 + kg) * 4 + g) * 16 + cc]);
			fr = fmaxf (fr, X[((1 * 4 + kg) * 4 + g) * 16 + cc]);
		}
		pkf = v2f{fmaxf (pkf.x, fl * scl.un), fmaxf (pkf.y, fr * scr.un)};
		__builtin_amdgcn_fence (__ATOMIC_RELEASE, "workgroup");
		__builtin_amdgcn_wave_barrier ();
	};

	// a sample has outgrown a lane's scale: peaks out of the scaled domain, new scales, the lane's ring words rescaled
	// in place by the (power-of-two) ratio — every word of the four slots; the slot about to be overwritten included
	auto rescale = [&] (float ml, float mr) __attribute__ ((always_inline)) {
		flush_pm ();
		const bool el = __float_as_uint (ml) >= scl.cap, er = __float_as_uint (mr) >= scr.cap;
		const float ol = scl.sc, orr = scr.sc;
		if (el) scl.set (ml);
		if (er) scr.set (mr);
		if (el || er) {
			typedef seg_h2 h2v;
			const _Float16 rl = rescale_ratio (scl.sc, ol), rr = rescale_ratio (scr.sc, orr);
			if constexpr (LAZY) { sel_ = __float_as_uint (scl.sc) >> 23; ser_ = __float_as_uint (scr.sc) >> 23; }
#pragma unroll 1
			for (int arr = 0; arr < (LAZY ? 2 : 4); ++arr) {                 // (LAZY: the ring holds hi words only)
				const _Float16 r = (arr & 1) ? rr : rl;
				const h2v r2 = h2v{r, r};
#pragma unroll 1
				for (int i = 0; i < 8; ++i) {
					uint4* const p = reinterpret_cast<uint4*> (smem + arr * ARRB + WA + 16 * i);
					uint4 v = *p;
					v.x = rescale_word (v.x, r2);
					v.y = rescale_word (v.y, r2);
					v.z = rescale_word (v.z, r2);
					v.w = rescale_word (v.w, r2);
					*p = v;
				}
			}
		}
		__builtin_amdgcn_fence (__ATOMIC_RELEASE, "workgroup");
		__builtin_amdgcn_wave_barrier ();
	};

	// Operands of (block, channel) bc for the products of the step whose window ends in ring slot (U + 3) & 3: window
	// quarter v sits in slot (U + v) & 3.
	m16::BFrag B0, B1;
	m16::f4 y0[3], y1[3];
#pragma unroll
	for (int p = 0; p < 3; ++p) { y0[p] = m16::f4{0.f, 0.f, 0.f, 0.f}; y1[p] = m16::f4{0.f, 0.f, 0.f, 0.f}; }
	auto fetch = [&]<int U> (m16::BFrag& B, int bc) __attribute__ ((always_inline)) {
		const int b = bc >> 1, ch = bc & 1;
		const lds_u8* const h = smem + ch * ARRB + b * BLKB;
		const lds_u8* const l = h + 2 * ARRB;
		B.h0 = *reinterpret_cast<const uint4*> (h + RA[U]);
		B.l0 = *reinterpret_cast<const uint4*> (l + RA[U]);
		B.h1 = *reinterpret_cast<const uint4*> (h + RA[(U + 2) & 3]);
		B.l1 = *reinterpret_cast<const uint4*> (l + RA[(U + 2) & 3]);
	};
	// SCREEN: the hi words alone, for MFMAs 0..5 (a chunk that completes reads all four again: fetch)
	auto fetch_hi = [&]<int U> (m16::BFrag& B, int bc) __attribute__ ((always_inline)) {
		const lds_u8* const h = smem + (bc & 1) * ARRB + (bc >> 1) * BLKB;
		B.h0 = *reinterpret_cast<const uint4*> (h + RA[U]);
		B.h1 = *reinterpret_cast<const uint4*> (h + RA[(U + 2) & 3]);
	};
	// CORE: the hi words under the three core fragments — window chunks kg + 1, kg + 2, kg + 3 — in B.h0, B.h1 and B.l0
	auto fetch_core = [&]<int U> (m16::BFrag& B, int bc) __attribute__ ((always_inline)) {
		const lds_u8* const h = smem + (bc & 1) * ARRB + (bc >> 1) * BLKB;
		B.h0 = *reinterpret_cast<const uint4*> (h + RB[U]);
		B.h1 = *reinterpret_cast<const uint4*> (h + RA[(U + 1) & 3]);
		B.l0 = *reinterpret_cast<const uint4*> (h + RB[(U + 1) & 3]);
	};
	// |max| of the accumulators of (block, channel) bc into pm
	auto fold = [&] (const m16::f4 (&y)[3], int bc) __attribute__ ((always_inline)) {
		float ma = pm[bc >> 1][bc & 1][0], mb = pm[bc >> 1][bc & 1][1];
#pragma unroll
		for (int p = 0; p < 3; ++p) { ma = max3abs (ma, y[p][0], y[p][1]); mb = max3abs (mb, y[p][2], y[p][3]); }
		if constexpr (SCREEN) { pm[bc >> 1][bc & 1][0] = fmaxf (ma, mb); pm[bc >> 1][bc & 1][1] = 0.f; }   // (one value: see pm)
		else { pm[bc >> 1][bc & 1][0] = ma; pm[bc >> 1][bc & 1][1] = mb; }
	};
	// ... of the launch's LAST step: lane (c, kg) holds rows (= frames of the step) 4 kg .. 4 kg + 3 of column 16 b + c; where that
	// column is the last segment of its stream, only the rows in front of its tile's end count
	auto fold_last = [&] (const m16::f4 (&y)[3], int bc) __attribute__ ((always_inline)) {
		if constexpr (ALIGNED) fold (y, bc);
		else {
			const uint32_t ucol = min (blockIdx.x * 64u + 16u * (uint32_t) (bc >> 1) + (uint32_t) cc, n_units - 1);
			const int rows = (ucol % a.n_segs == a.n_segs - 1) ? last_rows : R;
			float ma = pm[bc >> 1][bc & 1][0], mb = pm[bc >> 1][bc & 1][1];
#pragma unroll
			for (int p = 0; p < 3; ++p) {
				ma = max3abs (ma, 4 * kg + 0 < rows ? y[p][0] : 0.f, 4 * kg + 1 < rows ? y[p][1] : 0.f);
				mb = max3abs (mb, 4 * kg + 2 < rows ? y[p][2] : 0.f, 4 * kg + 3 < rows ? y[p][3] : 0.f);
			}
			if constexpr (SCREEN) { pm[bc >> 1][bc & 1][0] = fmaxf (ma, mb); pm[bc >> 1][bc & 1][1] = 0.f; }
			else { pm[bc >> 1][bc & 1][0] = ma; pm[bc >> 1][bc & 1][1] = mb; }
		}
	};
	// the products of the call's last step (nothing left to run under them); every chunk folds its predecessor's accumulators
	// (the first fold is still the step before's)
	auto products = [&]<int U> () __attribute__ ((always_inline)) {
		if constexpr (SCREEN) { n_scr += 8; n_fin += 8; }                // (dense; the step before left nothing pending)
		fetch.template operator()<U> (B0, 0);
#pragma unroll
		for (int bc = 0; bc < 8; bc += 2) {
			fetch.template operator()<U> (B1, bc + 1);
			m16::block (A, B0, y0);
			if (bc == 0) { if constexpr (!SCREEN) fold (y1, 7); } else fold_last (y1, bc - 1);
			if (bc + 2 < 8) fetch.template operator()<U> (B0, bc + 2);
			m16::block (A, B1, y1);
			fold_last (y0, bc);
		}
		fold_last (y1, 7);
	};

	// ---- LAZY: the lo operands of a completing block, built where they are needed -------------------------------------------
	// Lane (c, kg) of block b multiplies window samples [8 kg, 8 kg + 8) and [32 + 8 kg, 32 + 8 kg + 8) of column 16 b + c (the two
	// ds_read_b128 of `fetch`: B.l0, B.l1).  The window of the products that step jj completes is frames [F0 + 16 (jj - 4), F0 + 16 jj)
	// of the column's lane: two 64-byte pieces of its stream per lane, for both channels.  Why the words are the eager form's bits:
	//   1. A ring word is a pure function of its two samples and of the column's scales since.  The samples: the launch never
	//      writes the buffer or a.hist, and `sample` below is the rule the ring was filled by — the prologue's (the call's own frames,
	//      a.hist in front of them, +0 in front of that; frames below F0 are the previous segment's, read from the buffer) and, for the
	//      launch's last step where tiles are unaligned, last_frames' (+0 behind a last segment's tile end, never read).  The scale: a
	//      word of step m was split under the scale in force behind step m's head, S_m, by x * S_m -> v_cvt_pk_f16_f32 -> v_fma_mix —
	//      the instructions used here, on the same f32 operands, so Inf and NaN samples give the same halves — and every rescale
	//      since, at the heads of steps m + 1 .. jj, multiplied it in f16 by rescale_ratio (S_k, S_k-1) (1 where the channel kept
	//      its scale: the identity on every f16 that is no NaN, and NaNs stay NaNs; 0 for a ratio under 2^-24, which makes an Inf
	//      word a NaN — replayed like every other).  The owner keeps S_jj-4 .. S_jj-1 as bytes (shl_, shr_: pushed once per step) and
	//      S_jj is its current scale; the prologue's words (steps -3 .. -1) were split under the first scale, which is what the bytes
	//      start with.  A wave none of whose lanes changed a scale in those steps skips the replay (every factor is 1).
	//   2. The votes read hi products, pm, eps and R, none of which a lo word reaches except through a completed chunk's values —
	//      which are the eager ones by 1 — so the lazy form screens and completes the chunks form 2 does; pm, pkf and R evolve alike.
	//   3. The hi operands still come from the ring, whose stores stay behind the completions.
	// The column's parameters come from its owner lane 16 b + c by ds_bpermute.  NaN payloads may differ from the ring's where a
	// factor of 1 was skipped or applied; no result depends on them (the folds drop NaNs).
	// (the column's first frame as an offset into a.audio, not as a pointer: an integer made from a pointer would cost every load of
	// the kernel its address space — flat loads, which the main loop would wait for with its LDS reads)
	const int64_t coff = (int64_t) ((uint64_t) s * a.stride + a.head) + F0;
	auto lazy_lo = [&]<bool FINAL> (int b, int jj, uint32_t (&lo)[2][2][4]) __attribute__ ((always_inline)) {
		const int o = 16 * b + cc;
		const uint64_t cpw = (uint64_t) coff;
		const v2f* const xp = reinterpret_cast<const v2f*> (a.audio)
			+ (int64_t) (((uint64_t) (uint32_t) __shfl ((int) (cpw >> 32), o) << 32) | (uint32_t) __shfl ((int) (uint32_t) cpw, o))
			+ (int64_t) R * (jj - 4);                                       // the column's window
		// frames of the owner's window in front of the call (its history or +0): 0 but in the first steps of a lane that starts the call
		const int64_t fc0 = F0 + (int64_t) a.head + (int64_t) R * (jj - 4);
		const int front_own = (int) min (max (-fc0, (int64_t) 0), (int64_t) 64);
		const bool plain = __ballot (front_own != 0) == 0 && !(FINAL && cut);
		const bool flat = __ballot (shl_ != sel_ * 0x01010101u || shr_ != ser_ * 0x01010101u) == 0;
		const int qv = kg >> 1;
		v2f xs[2][8];
		if (__builtin_expect (plain, 1)) {
#pragma unroll
			for (int h = 0; h < 2; ++h) {
				const float4_a8* const pp = reinterpret_cast<const float4_a8*> (xp + 32 * h + 8 * kg);
#pragma unroll
				for (int i = 0; i < 4; ++i) {
					const f4v_ v = pp[i];
					xs[h][2 * i] = v2f{v.x, v.y}; xs[h][2 * i + 1] = v2f{v.z, v.w};
				}
			}
		} else {
			// sample (f), frame by frame: the prologue's rule and last_frames'
			const int front = __shfl (front_own, o);
			const v2f* const hs = reinterpret_cast<const v2f*> (a.hist) + (size_t) (uint32_t) __shfl ((int) s, o) * MTR_FIR_HALO;
			const bool clast = __shfl ((int) lastq, o) != 0;
#pragma unroll
			for (int h = 0; h < 2; ++h)
#pragma unroll
				for (int i = 0; i < 8; ++i) {
					const int w = 32 * h + 8 * kg + i;
					v2f v = v2f{0.f, 0.f};
					if (w >= front) { if (!(FINAL && clast && w - 48 >= last_rows)) v = xp[w]; }
					else if (w - front + MTR_FIR_HALO >= 0) v = hs[w - front + MTR_FIR_HALO];
					xs[h][i] = v;
				}
		}
		// the scales: e[i] = the exponent field of S_(jj - 4 + i)
		const uint32_t hl_ = (uint32_t) __shfl ((int) shl_, o), hr_ = (uint32_t) __shfl ((int) shr_, o);
		const uint32_t cl_ = (uint32_t) __shfl ((int) sel_, o), cr_ = (uint32_t) __shfl ((int) ser_, o);
		float sl[5], sr[5];
#pragma unroll
		for (int i = 0; i < 4; ++i) {
			sl[i] = __uint_as_float (((hl_ >> (8 * (3 - i))) & 255u) << 23);
			sr[i] = __uint_as_float (((hr_ >> (8 * (3 - i))) & 255u) << 23);
		}
		sl[4] = __uint_as_float (cl_ << 23); sr[4] = __uint_as_float (cr_ << 23);
		// piece h holds frames of step jj - 4 + 2 h + qv
#pragma unroll
		for (int h = 0; h < 2; ++h) {
			const v2f sc = v2f{qv ? sl[2 * h + 1] : sl[2 * h], qv ? sr[2 * h + 1] : sr[2 * h]};
#pragma unroll
			for (int i = 0; i < 4; ++i) {
				const v2f u = xs[h][2 * i] * sc, v = xs[h][2 * i + 1] * sc;
				lo[0][h][i] = m16::lo_pair (m16::hi_pair (u.x, v.x), u.x, v.x);
				lo[1][h][i] = m16::lo_pair (m16::hi_pair (u.y, v.y), u.y, v.y);
			}
		}
		if (__builtin_expect (!flat, 0)) {
			// the rescales at the heads of steps jj - 4 + i, i = 1 .. 4, in their order; a piece takes part in those behind its own step
			const seg_h2 one = seg_h2{(_Float16) 1.0f, (_Float16) 1.0f};
#pragma unroll
			for (int i = 1; i <= 4; ++i) {
				const _Float16 rl = rescale_ratio (sl[i], sl[i - 1]), rr = rescale_ratio (sr[i], sr[i - 1]);
#pragma unroll
				for (int h = 0; h < 2; ++h) {
					if (i <= 2 * h) continue;                            // (piece 1: steps jj - 2 and jj - 1)
					const bool in = i > 2 * h + qv;
					const seg_h2 r2l = in ? seg_h2{rl, rl} : one, r2r = in ? seg_h2{rr, rr} : one;
#pragma unroll
					for (int k = 0; k < 4; ++k) { lo[0][h][k] = rescale_word (lo[0][h][k], r2l); lo[1][h][k] = rescale_word (lo[1][h][k], r2r); }
				}
			}
		}
	};
	// ... and the completions of a step (fail8: bit bc = chunk bc completes) or, FINAL, of the launch's last, dense step: m16::block
	// on the ring's hi words and the lo words built here, folded into pm as `fold` / `fold_last` do.  One loop over the blocks, not
	// unrolled: every copy of the step carries one copy of this.
	auto complete = [&]<int U, bool FINAL> (uint32_t fail8, int jj) __attribute__ ((always_inline)) {
#pragma unroll 1
		for (int b = 0; b < 4; ++b) {
			const uint32_t f2 = (fail8 >> (2 * b)) & 3u;
			if (f2 == 0) continue;
			uint32_t lo[2][2][4];
			lazy_lo.template operator()<FINAL> (b, jj, lo);
			int rows = R;
			if constexpr (FINAL && !ALIGNED) {
				const uint32_t ucol = min (blockIdx.x * 64u + 16u * (uint32_t) b + (uint32_t) cc, n_units - 1);
				rows = (ucol % a.n_segs == a.n_segs - 1) ? last_rows : R;
			}
#pragma unroll
			for (int ch = 0; ch < 2; ++ch) {
				if (!((f2 >> ch) & 1u)) continue;
				const lds_u8* const h = smem + ch * ARRB + b * BLKB;
				B1.h0 = *reinterpret_cast<const uint4*> (h + RA[U]);
				B1.h1 = *reinterpret_cast<const uint4*> (h + RA[(U + 2) & 3]);
				B1.l0 = uint4{lo[ch][0][0], lo[ch][0][1], lo[ch][0][2], lo[ch][0][3]};
				B1.l1 = uint4{lo[ch][1][0], lo[ch][1][1], lo[ch][1][2], lo[ch][1][3]};
				m16::block (A, B1, y0);
				float ma = 0.f, mb = 0.f;
#pragma unroll
				for (int p = 0; p < 3; ++p) {
					ma = max3abs (ma, 4 * kg + 0 < rows ? y0[p][0] : 0.f, 4 * kg + 1 < rows ? y0[p][1] : 0.f);
					mb = max3abs (mb, 4 * kg + 2 < rows ? y0[p][2] : 0.f, 4 * kg + 3 < rows ? y0[p][3] : 0.f);
				}
				const float f = fmaxf (ma, mb);
				// (the same maximum as fold's, whose chains start from pm: pm[..][1] is +0 in every screened form)
#pragma unroll
				for (int bb = 0; bb < 4; ++bb) pm[bb][ch][0] = bb == b ? fmaxf (pm[bb][ch][0], f) : pm[bb][ch][0];
				++n_fin;
			}
		}
	};

	int tile_left = spt;
	uint32_t tile = p0;
	int j = 0;
	// Phase 0 counts a lane's whole step j where F0 + R (j + 1) <= p0_end.  No lane starts behind the launch's last segment,
	// F0 <= (tiles of a stream - n_main) tile_frames, so in front of step p0_steps that holds for every lane of every wave:
	// one scalar compare on j instead of a 64-bit compare per lane.
	const int64_t p0_room = a.p0_end - (int64_t) (a.n_segs * a.seg_base + min (a.n_segs, a.seg_rem) - a.n_main) * a.tile_frames;
	const int p0_steps = (int) min (max (p0_room, (int64_t) 0) / R, (int64_t) n_steps);

	// max |x| per channel of buffer B: always computed one step early, under the products of the step before
	float ml = 0.f, mr = 0.f;
	auto maxabs = [&]<int B> () __attribute__ ((always_inline)) {
		ml = 0.f; mr = 0.f;
#pragma unroll
		for (int n = 0; n < R; n += 2) { ml = max3abs (ml, xq[B][n].x, xq[B][n + 1].x); mr = max3abs (mr, xq[B][n].y, xq[B][n + 1].y); }
	};

	// one step: the scalar / packed work of step j on buffer U (ring slot U), and — PROD — the products of step j - 1,
	// interleaved by hand (the source order is the schedule: see the chunks below)
#ifdef MTR_SEG_PROF
	unsigned long long sprof_[10] = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 };
#endif
	// KW: the recurrence rides in this step's schedule (EBU; not in the step of an unaligned tile's end)
	auto step = [&]<int U, bool PROD, bool KW> () __attribute__ ((always_inline)) {
		v2f (&x)[R] = xq[U];
		SPROF_NOW (c0_);
		// phase 0 = |x[n - 24]| for the frames of this call: everything but its last 24 frames
		// (SCREEN: a scalar test on the step — in front of step p0_steps every lane's whole step counts, see p0_steps; behind it,
		// the launch's last two steps, each lane tests its own frames as the dense form does on every step)
		if (SCREEN && __builtin_expect (j < p0_steps, 1)) pk0 = v2f{umaxf (pk0.x, ml), umaxf (pk0.y, mr)};
		else if (F0 + (int64_t) R * (j + 1) <= a.p0_end) pk0 = v2f{fmaxf (pk0.x, ml), fmaxf (pk0.y, mr)};
		else {
			const int64_t lim = a.p0_end - F0 - (int64_t) R * j;
#pragma unroll
			for (int n = 0; n < R; ++n) if (n < lim) pk0 = v2f{fmaxf (pk0.x, fabsf (x[n].x)), fmaxf (pk0.y, fabsf (x[n].y))};
		}
		if (__builtin_expect (__ballot (__float_as_uint (ml) >= scl.cap || __float_as_uint (mr) >= scr.cap) != 0, 0)) {
			// (dense: the last chunk's accumulators of the step before are still waiting for their fold, which chunk 0 does: they
			// belong to the old scale, so they are folded here, in front of the flush, and cleared.  SCREEN: the step before has
			// voted on all of its chunks and completed the failing ones — nothing is pending)
			if constexpr (!SCREEN) {
				fold (y1, 7);
#pragma unroll
				for (int p = 0; p < 3; ++p) y1[p] = m16::f4{0.f, 0.f, 0.f, 0.f};
			}
			rescale (ml, mr);
			if constexpr (CORE) { if (PROD) fetch_core.template operator()<U> (B0, 0); }
			else if constexpr (SCREEN) { if (PROD) fetch_hi.template operator()<U> (B0, 0); }
			else if (PROD) fetch.template operator()<U> (B0, 0);          // (fetched before the ring was rescaled: again)
		}

		// the stream, three steps ahead (the pointer stops with the segment: the last loads re-read its last line)
#if !(defined (MTR_TIMING_ONLY_BUILD) && defined (MTR_SEG_DBG_NOADV))   /* (elimination runs of a timing-only library, wrong results: the same line over and over) */
		lp += (j + 3 < (ALIGNED ? n_steps : n_loads)) ? R / 2 : 0;
#endif
		load.template operator()<(U + 3) & 3> ();
		SPROF_NOW (h1_); SPROF_ADD (8, h1_ - c0_);
		// SCREEN: eps of the products of step j - 1 for every accumulator lane.  The owner of column 16 b + c (lane 16 b + c)
		// computes it in the column's current scale; lane (c, kg) needs the four columns c of blocks 0..3: through LDS.
		// The exchange relies on the hardware's DS ordering within a wave, not on the language's memory model: a wave's DS
		// instructions execute in issue order, and the block is this one wave, so the reads see the writes in front of them and
		// the next step's writes come behind these reads — as the ring stores and the operand fetch behind them have always
		// relied on.  All the compiler is told is not to move or forward across the two points (a fence there drained the LDS
		// queue twice a step, lgkmcnt (0), with no other wave to run under it); the bounds are first read by chunk 0's vote,
		// behind chunk 1's MFMAs.  flush_pm and rescale keep their fences: they run once per rescale and once at the end of a
		// launch, their values are consumed at once, so a drain there costs nothing that could be hidden.
		float eps[4][2], ref[4][2];
		if constexpr (SCREEN) {
			rml = umaxf (rml, ml); rmr = umaxf (rmr, mr);                // (step j's own samples too: a bound on more is still a bound)
			if constexpr (U == 0) {                                       // the stream reference, every fourth step
				refl = ref_row (ref_own ? max (__float_as_uint (pk0.x), __float_as_uint (pkf.x)) : 0u);
				refr = ref_row (ref_own ? max (__float_as_uint (pk0.y), __float_as_uint (pkf.y)) : 0u);
			}
			if (PROD) {
				float* const E = reinterpret_cast<float*> (smem_ + XEPS);
				// (LEN: a column whose peak does not count passes the screen whatever its values — eps = -inf — so that the zeros
				// behind a stream's end, which never pass it, do not complete every chunk of their waves)
				*reinterpret_cast<float2*> (E + (cc * 4 + kg) * 2) = (LEN && !peak_ok) ? float2{-INFINITY, -INFINITY} :
					float2{fmaf (KREL, rml * scl.sc, KABS), fmaf (KREL, rmr * scr.sc, KABS)};
				float* const Q = reinterpret_cast<float*> (smem_ + XREF);
				*reinterpret_cast<float2*> (Q + (cc * 4 + kg) * 2) =
					float2{__uint_as_float (refl) * (scl.sc * 32768.f), __uint_as_float (refr) * (scr.sc * 32768.f)};
				asm volatile ("" ::: "memory");
				const float4 e0 = *reinterpret_cast<const float4*> (E + cc * 8), e1 = *reinterpret_cast<const float4*> (E + cc * 8 + 4);
				eps[0][0] = e0.x; eps[0][1] = e0.y; eps[1][0] = e0.z; eps[1][1] = e0.w;
				eps[2][0] = e1.x; eps[2][1] = e1.y; eps[3][0] = e1.z; eps[3][1] = e1.w;
				const float4 r0 = *reinterpret_cast<const float4*> (Q + cc * 8), r1 = *reinterpret_cast<const float4*> (Q + cc * 8 + 4);
				ref[0][0] = r0.x; ref[0][1] = r0.y; ref[1][0] = r0.z; ref[1][1] = r0.w;
				ref[2][0] = r1.x; ref[2][1] = r1.y; ref[3][0] = r1.z; ref[3][1] = r1.w;
				SPROF_NOW (h2_);
				asm volatile ("" ::: "memory");
				SPROF_NOW (h3_); SPROF_ADD (9, h3_ - h2_);
			}
		}
		SPROF_NOW (c1_); SPROF_ADD (0, c1_ - c0_);

		// Eight chunks, one per (block, channel) of the products of step j - 1.  THE SOURCE ORDER IS THE SCHEDULE (this TU
		// is compiled without the machine schedulers, csrc/Makefile).  The issue model of one wave (tools/issue_model.hip,
		// profiles/r03_issue_model.txt), in shader cycles per MFMA:
		//     16x16x32 MFMA alone 17.2;  + 2 independent full-rate VALU (v_fma / v_mul / v_max3) 19.2;  + 3: 23.8;  + 2 DEPENDENT: 22.2
		//     + 1 half-rate VALU (v_fma_mix, v_cvt_pk, 8 cycles alone) 18.5;  + 2 of them 26.5;  mixlo + mixhi of ONE word 31.3
		//     + 1 v_pk_fma_f32: 34.3 (a packed-f32 instruction waits for the matrix pipe);  packed among themselves 5.1, 8.2 if
		//     the next one reads the last one's result;  + 1 ds_read_b128: + 6
		// So: behind every MFMA either two independent full-rate instructions (hipcc unpacks a packed one it finds there into its
		// two halves) or ONE half-rate instruction, and everything that does not fit — most of the recurrence — in ONE packed
		// block per step behind the last chunk (one wait for the matrix pipe per step instead of one per chunk):
		//   MFMA 0-1: the scale of two frames    2-3: f16 hi words (v_cvt_pk)    4-7: lo words (v_fma_mix, one each)
		//   8: the next step's maxima    9-11: |max| of the previous chunk's accumulators, two chains
		//   12-17: six operations of the recurrence's sequence
		const v2f sc2 = v2f{scl.sc, scr.sc};
		uint32_t hl[R / 2], hr[R / 2], ll[R / 2], lr[R / 2];
		float nl = 0.f, nr = 0.f;
		const v2f (&xn)[R] = xq[(U + 1) & 3];
		KWork kw;
		kw.x[0] = ks.z2; kw.x[1] = ks.z1;
		constexpr int KGAP = 6;                                     // operations of the recurrence behind the MFMAs of one chunk
		auto kseq = [&]<int I> () __attribute__ ((always_inline)) {
			if constexpr (KW && I < KOPS) kopx<kseq_tab.op[I]> (kc, ks, kw, x, kseq_tab.frame[I]);
		};
		// SCREEN: the vote on chunk K's first product y — the lanes that may reach the running peak, as a wave-uniform mask
		uint64_t msk[8];
		auto vote = [&]<int K> (const m16::f4 (&y)[3]) __attribute__ ((always_inline)) {
			// max (+0, |y| of the twelve values that are no NaN) as six v_max3: two chains of two, their merge with the eleventh value,
			// and the twelfth with the +0.  fmaxf returns the operand that is no NaN and a NaN only where both are; the last one's +0
			// is none, and a maximum of the same values does not depend on their order: c is, bit for bit, what two chains from +0
			// give.  A lane all of whose values are NaN votes with c = +0 (the dense fold drops them too), one with an Inf with +Inf.
			auto m3 = [] (float a, float b, float c) __attribute__ ((always_inline)) { return fmaxf (fmaxf (a, b), c); };
			float ca = m3 (fabsf (y[0][0]), fabsf (y[0][1]), fabsf (y[0][2])), cb = m3 (fabsf (y[0][3]), fabsf (y[1][0]), fabsf (y[1][1]));
			ca = m3 (ca, fabsf (y[1][2]), fabsf (y[1][3])); cb = m3 (cb, fabsf (y[2][0]), fabsf (y[2][1]));
			const float c = m3 (m3 (ca, cb, fabsf (y[2][2])), fabsf (y[2][3]), 0.f);
			const float pk = fmaxf (fmaxf (pm[K >> 1][K & 1][0], pm[K >> 1][K & 1][1]), ref[K >> 1][K & 1]);
			const bool below = c + eps[K >> 1][K & 1] < pk;                      // (false for a NaN in eps or in all of pk)
			msk[K] = __ballot (!below);
		};
		auto chunk =[&]<int BC> (m16::BFrag& Bc, m16::BFrag& Bn, m16::f4 (&yc)[3], m16::f4 (&yp)[3]) __attribute__ ((always_inline)) {
			constexpr int PB = (BC + 7) & 7;
			const v2f xa = x[2 * BC], xb = x[2 * BC + 1];
			if (PROD && BC < 7) fetch.template operator()<U> (Bn, BC + 1);
#if defined (MTR_TIMING_ONLY_BUILD) && defined (MTR_SEG_DBG_NOPROD)    /* (elimination runs of a timing-only library, wrong results: no products) */
#define MTR_M(I)
#else
#define MTR_M(I) if (PROD) m16::block_mfma<I> (A, Bc, yc)
#endif
			MTR_M (0);  const v2f um = xa * sc2;
			MTR_M (1);  const v2f vm = xb * sc2;
			MTR_M (2);  hl[BC] = m16::hi_pair (um.x, vm.x);
			MTR_M (3);  hr[BC] = m16::hi_pair (um.y, vm.y);
			MTR_M (4);  lo_first (ll[BC], hl[BC], um.x);
			MTR_M (5);  lo_first (lr[BC], hr[BC], um.y);
			MTR_M (6);  lo_second (ll[BC], hl[BC], vm.x);
			MTR_M (7);  lo_second (lr[BC], hr[BC], vm.y);
			MTR_M (8);  nl = max3abs (nl, xn[2 * BC].x, xn[2 * BC + 1].x); nr = max3abs (nr, xn[2 * BC].y, xn[2 * BC + 1].y);
			float ma = pm[PB >> 1][PB & 1][0], mb = pm[PB >> 1][PB & 1][1];
			MTR_M (9);  if (PROD) { ma = max3abs (ma, yp[0][0], yp[0][1]); mb = max3abs (mb, yp[0][2], yp[0][3]); }
			MTR_M (10); if (PROD) { ma = max3abs (ma, yp[1][0], yp[1][1]); mb = max3abs (mb, yp[1][2], yp[1][3]); }
			MTR_M (11); if (PROD) { ma = max3abs (ma, yp[2][0], yp[2][1]); mb = max3abs (mb, yp[2][2], yp[2][3]); }
			if (PROD) asm volatile ("" : "+v"(ma), "+v"(mb));   // consumed here: the maxima must not sink behind the accumulators' next writers
			pm[PB >> 1][PB & 1][0] = ma; pm[PB >> 1][PB & 1][1] = mb;
			// The ring stores of this step ride in the last two chunks — behind the last operand fetch that still reads the
			// slot they overwrite (chunk 6 fetches chunk 7's) — and the next step's first operands are fetched behind them:
			// neither the stores' VGPR transfer nor the fetch's latency is left for the step's head and tail.
#define MTR_ST(ARR, W_) \
			if constexpr (BC == 6) *reinterpret_cast<uint4*> (smem + WS[U] + (ARR) * ARRB) = uint4{W_[0], W_[1], W_[2], W_[3]}; \
			if constexpr (BC == 7) *reinterpret_cast<uint4*> (smem + (WS[U] ^ 16) + (ARR) * ARRB) = uint4{W_[4], W_[5], W_[6], W_[7]}
			MTR_M (12); kseq.template operator()<KGAP * BC + 0> ();
			MTR_ST (0, hl);
			MTR_M (13); kseq.template operator()<KGAP * BC + 1> ();
			MTR_ST (1, hr);
			MTR_M (14); kseq.template operator()<KGAP * BC + 2> ();
			MTR_ST (2, ll);
			MTR_M (15); kseq.template operator()<KGAP * BC + 3> ();
			MTR_ST (3, lr);
			MTR_M (16); kseq.template operator()<KGAP * BC + 4> ();
			if constexpr (BC == 7) fetch.template operator()<(U + 1) & 3> (Bn, 0);      // (Bn of the last chunk = B0 of the next step)
			MTR_M (17); kseq.template operator()<KGAP * BC + 5> ();
#undef MTR_ST
#undef MTR_M
		};
		// The screened chunk: MFMAs 0..5 only, so most of the split, the maxima and the recurrence issue bare (the issue model's
		// floor: the elimination run without products).  No verdict stands between two chunks' products: the next chunk's hi
		// operands are fetched first, whatever the vote, a whole chunk ahead of their use; behind the six MFMAs the scale, the hi
		// words and the lo words' first halves; then the lo words' second halves, the next step's maxima, the vote of the PREVIOUS
		// chunk (its accumulators are complete: this chunk's six MFMAs ran behind them) and six operations of the recurrence.  The
		// vote leaves its failing lanes as a mask; chunk 7 votes on itself behind its own tail, and the step branches once (the
		// SCREEN block behind chunk 7, below).
		auto chunk_s = [&]<int BC> (m16::BFrag& Bc, m16::BFrag& Bn, m16::f4 (&yc)[3], m16::f4 (&yp)[3]) __attribute__ ((always_inline)) {
			const v2f xa = x[2 * BC], xb = x[2 * BC + 1];
			if (PROD && BC < 7) fetch_hi.template operator()<U> (Bn, BC + 1);
#define MTR_M(I) if (PROD) m16::block_mfma<I> (A, Bc, yc)
			MTR_M (0);  v2f um = xa * sc2;
			MTR_M (1);  v2f vm = xb * sc2;
			MTR_M (2);  hl[BC] = m16::hi_pair (um.x, vm.x);
			MTR_M (3);  hr[BC] = m16::hi_pair (um.y, vm.y);
			MTR_M (4);  lo_first (ll[BC], hl[BC], um.x);
			MTR_M (5);  lo_first (lr[BC], hr[BC], um.y);
#undef MTR_M
			// (computed HERE, behind the six MFMAs: otherwise the compiler sinks them towards their uses)
			asm volatile ("" : "+v"(um), "+v"(vm), "+v"(hl[BC]), "+v"(hr[BC]), "+v"(ll[BC]), "+v"(lr[BC]));
			lo_second (ll[BC], hl[BC], vm.x);
			lo_second (lr[BC], hr[BC], vm.y);
			nl = max3abs (nl, xn[2 * BC].x, xn[2 * BC + 1].x); nr = max3abs (nr, xn[2 * BC].y, xn[2 * BC + 1].y);
			if constexpr (BC > 0) if (PROD) vote.template operator()<BC - 1> (yp);
			kseq.template operator()<KGAP * BC + 0> ();
			kseq.template operator()<KGAP * BC + 1> ();
			kseq.template operator()<KGAP * BC + 2> ();
			kseq.template operator()<KGAP * BC + 3> ();
			kseq.template operator()<KGAP * BC + 4> ();
			kseq.template operator()<KGAP * BC + 5> ();
			if constexpr (BC == 7) if (PROD) vote.template operator()<7> (yc);
		};
		// The lazy chunk: chunk_s without the lo words.  The shadows of MFMAs 4 and 5, which carried their first halves, take the
		// next step's maxima, and nothing of the split is left to issue bare.
		auto chunk_z = [&]<int BC> (m16::BFrag& Bc, m16::BFrag& Bn, m16::f4 (&yc)[3], m16::f4 (&yp)[3]) __attribute__ ((always_inline)) {
			const v2f xa = x[2 * BC], xb = x[2 * BC + 1];
			if (PROD && BC < 7) fetch_hi.template operator()<U> (Bn, BC + 1);
#define MTR_M(I) if (PROD) m16::block_mfma<I> (A, Bc, yc)
			MTR_M (0);  v2f um = xa * sc2;
			MTR_M (1);  v2f vm = xb * sc2;
			MTR_M (2);  hl[BC] = m16::hi_pair (um.x, vm.x);
			MTR_M (3);  hr[BC] = m16::hi_pair (um.y, vm.y);
			MTR_M (4);  nl = max3abs (nl, xn[2 * BC].x, xn[2 * BC + 1].x);
			MTR_M (5);  nr = max3abs (nr, xn[2 * BC].y, xn[2 * BC + 1].y);
#undef MTR_M
			// (computed HERE, behind the six MFMAs: otherwise the compiler sinks them towards their uses)
			asm volatile ("" : "+v"(hl[BC]), "+v"(hr[BC]), "+v"(nl), "+v"(nr));
			if constexpr (BC > 0) if (PROD) vote.template operator()<BC - 1> (yp);
			kseq.template operator()<KGAP * BC + 0> ();
			kseq.template operator()<KGAP * BC + 1> ();
			kseq.template operator()<KGAP * BC + 2> ();
			kseq.template operator()<KGAP * BC + 3> ();
			kseq.template operator()<KGAP * BC + 4> ();
			kseq.template operator()<KGAP * BC + 5> ();
			if constexpr (BC == 7) if (PROD) vote.template operator()<7> (yc);
		};
		// The core chunk: three MFMAs, each one row group's core product from zero — yc[w] = rows 16 w .. 16 w + 15, of which this lane
		// holds 4 kg .. 4 kg + 3 — on the operands fetched a chunk ahead (three ds_read_b128).  Their shadows take the scale of the
		// chunk's two frames (two full-rate instructions each) and one of its hi words (one half-rate instruction); the other hi
		// word, the next step's maxima, the previous chunk's vote on its twelve values and six operations of the recurrence issue bare.
		auto chunk_c = [&]<int BC> (m16::BFrag& Bc, m16::BFrag& Bn, m16::f4 (&yc)[3], m16::f4 (&yp)[3]) __attribute__ ((always_inline)) {
			const v2f xa = x[2 * BC], xb = x[2 * BC + 1];
			if (PROD && BC < 7) fetch_core.template operator()<U> (Bn, BC + 1);
			const m16::f4 z4 = m16::f4{0.f, 0.f, 0.f, 0.f};
			if (PROD) yc[0] = __builtin_amdgcn_mfma_f32_16x16x32_f16 (AC[0], __builtin_bit_cast (m16::h8, Bc.h0), z4, 0, 0, 0);
			v2f um = xa * sc2;
			if (PROD) yc[1] = __builtin_amdgcn_mfma_f32_16x16x32_f16 (AC[1], __builtin_bit_cast (m16::h8, Bc.h1), z4, 0, 0, 0);
			v2f vm = xb * sc2;
			if (PROD) yc[2] = __builtin_amdgcn_mfma_f32_16x16x32_f16 (AC[2], __builtin_bit_cast (m16::h8, Bc.l0), z4, 0, 0, 0);
			hl[BC] = m16::hi_pair (um.x, vm.x);
			// (computed HERE, behind the three MFMAs: otherwise the compiler sinks them towards their uses)
			asm volatile ("" : "+v"(um), "+v"(vm), "+v"(hl[BC]));
			hr[BC] = m16::hi_pair (um.y, vm.y);
			nl = max3abs (nl, xn[2 * BC].x, xn[2 * BC + 1].x); nr = max3abs (nr, xn[2 * BC].y, xn[2 * BC + 1].y);
			asm volatile ("" : "+v"(hr[BC]), "+v"(nl), "+v"(nr));
			if constexpr (BC > 0) if (PROD) vote.template operator()<BC - 1> (yp);
			kseq.template operator()<KGAP * BC + 0> ();
			kseq.template operator()<KGAP * BC + 1> ();
			kseq.template operator()<KGAP * BC + 2> ();
			kseq.template operator()<KGAP * BC + 3> ();
			kseq.template operator()<KGAP * BC + 4> ();
			kseq.template operator()<KGAP * BC + 5> ();
			if constexpr (BC == 7) if (PROD) vote.template operator()<7> (yc);
		};
		auto any_chunk = [&]<int BC> (m16::BFrag& Bc, m16::BFrag& Bn, m16::f4 (&yc)[3], m16::f4 (&yp)[3]) __attribute__ ((always_inline)) {
			if constexpr (CORE) chunk_c.template operator()<BC> (Bc, Bn, yc, yp);
			else if constexpr (LAZY) chunk_z.template operator()<BC> (Bc, Bn, yc, yp);
			else if constexpr (SCREEN) chunk_s.template operator()<BC> (Bc, Bn, yc, yp);
			else chunk.template operator()<BC> (Bc, Bn, yc, yp);
		};
		any_chunk.template operator()<0> (B0, B1, y0, y1);
		SPROF_NOW (c2_); SPROF_ADD (1, c2_ - c1_);
		any_chunk.template operator()<1> (B1, B0, y1, y0);
		any_chunk.template operator()<2> (B0, B1, y0, y1); any_chunk.template operator()<3> (B1, B0, y1, y0);
		any_chunk.template operator()<4> (B0, B1, y0, y1); any_chunk.template operator()<5> (B1, B0, y1, y0);
		any_chunk.template operator()<6> (B0, B1, y0, y1);
		SPROF_NOW (c3_); SPROF_ADD (2, c3_ - c2_);
		any_chunk.template operator()<7> (B1, B0, y1, y0);
		SPROF_NOW (c4_); SPROF_ADD (3, c4_ - c3_);
		if constexpr (SCREEN) {
			// One branch per step: the chunks some lane of which failed its vote run their three products from zero (m16::block:
			// MFMAs 0..17 in the dense order, so the dense values bit for bit) on operands read again from the ring — its slot U,
			// the oldest quarter of every window of this step's products, is overwritten only below — and fold into pm as there.
			if (PROD) {
				n_scr += 8;
				if (__builtin_expect ((msk[0] | msk[1] | msk[2] | msk[3] | msk[4] | msk[5] | msk[6] | msk[7]) != 0, 0)) {
#if !(defined (MTR_TIMING_ONLY_BUILD) && defined (MTR_SEG_DBG_NOLO))    /* (elimination run of a timing-only library, wrong results: the lazy hot path, completions on stale lo words) */
					if constexpr (LAZY) {
						uint32_t fail8 = 0;
#pragma unroll
						for (int k = 0; k < 8; ++k) fail8 |= msk[k] != 0 ? 1u << k : 0u;
						complete.template operator()<U, false> (fail8, j);
					} else
#endif
					[&]<int... Ks> (std::integer_sequence<int, Ks...>) __attribute__ ((always_inline)) {
						([&] () __attribute__ ((always_inline)) {
							if (msk[Ks] != 0) { fetch.template operator()<U> (B1, Ks); m16::block (A, B1, y0); fold (y0, Ks); ++n_fin; }
						} (), ...);
					} (std::make_integer_sequence<int, 8>{});
					// rule 2: what the chunks completed so far have found goes into the owners' pkf now, and from there into the
					// stream's reference at its next refresh (a launch argument, wave-uniform: no further instantiation)
					if (LAZY || a.screen == 2u) peek_pm ();                       // (the lazy form is rule 2's)
				}
			}
			// the step's ring stores (slot U), then the next step's first operands, which read them (Bn of chunk 7 = B0 of the next step)
			lds_u8* const w0 = smem + WS[U];
			lds_u8* const w1 = smem + (WS[U] ^ 16);
			*reinterpret_cast<uint4*> (w0)            = uint4{hl[0], hl[1], hl[2], hl[3]};
			*reinterpret_cast<uint4*> (w1)            = uint4{hl[4], hl[5], hl[6], hl[7]};
			*reinterpret_cast<uint4*> (w0 + ARRB)     = uint4{hr[0], hr[1], hr[2], hr[3]};
			*reinterpret_cast<uint4*> (w1 + ARRB)     = uint4{hr[4], hr[5], hr[6], hr[7]};
			if constexpr (LAZY) {
				shl_ = (shl_ << 8) | sel_; shr_ = (shr_ << 8) | ser_;        // the scale this step's words were split in
			} else {
			*reinterpret_cast<uint4*> (w0 + 2 * ARRB) = uint4{ll[0], ll[1], ll[2], ll[3]};
			*reinterpret_cast<uint4*> (w1 + 2 * ARRB) = uint4{ll[4], ll[5], ll[6], ll[7]};
			*reinterpret_cast<uint4*> (w0 + 3 * ARRB) = uint4{lr[0], lr[1], lr[2], lr[3]};
			*reinterpret_cast<uint4*> (w1 + 3 * ARRB) = uint4{lr[4], lr[5], lr[6], lr[7]};
			}
			if constexpr (CORE) fetch_core.template operator()<(U + 1) & 3> (B0, 0);
			else fetch_hi.template operator()<(U + 1) & 3> (B0, 0);
		}
		SPROF_NOW (c5_); SPROF_ADD (4, c5_ - c4_);
		// the rest of the recurrence's sequence: one packed block (SCREEN: the ring stores and the fetch above drain under it)
		if (KW) {
			[&]<int... Is> (std::integer_sequence<int, Is...>) __attribute__ ((always_inline)) {
				(kseq.template operator()<8 * KGAP + Is> (), ...);
			} (std::make_integer_sequence<int, KOPS - 8 * KGAP>{});
			ks.z2 = kw.x[R]; ks.z1 = kw.x[R + 1];
		}
		asm volatile ("" : "+v"(nl), "+v"(nr));
		ml = nl; mr = nr;
		++j;
		if (KW && ALIGNED && --tile_left == 0) {
			if (live && tile >= fq) a.tile_power[(size_t) s * a.n_tiles + a.tile0 + tile] = a.gain_l * ks.sj.x + a.gain_r * ks.sj.y;
			ks.sj = 0;
			ks.z1 = scrub (ks.z1); ks.z2 = scrub (ks.z2); ks.z3 = scrub (ks.z3); ks.z4 = scrub (ks.z4);   // ebu_r128_proc.cc:331-334
			tile_left = spt; ++tile;
		}
		SPROF_NOW (c6_); SPROF_ADD (5, c6_ - c5_); SPROF_ADD (6, c6_ - c0_); SPROF_ADD (7, 1);
	};

	// An unaligned tile ends inside a step (the same step and frame for all lanes: every lane starts on a tile boundary).  That
	// step runs like every other one — the very code of the aligned kernel, products, split and recurrence — and then its
	// recurrence is run AGAIN from the state the step started with, frame by frame: Σ y² closes at the exact frame, the states
	// are scrubbed there (ebu_r128_proc.cc:331-334), and the lane's last tile end is where its filter state is final — the frames
	// of the step behind it belong to the next segment (or to k_kwtp16's tail of the call).  One step in ~138 pays for sixteen
	// dependent recurrence steps (+ 0.3 % of the launch); the other 137 carry no trace of the boundary (round 3 compiled a second
	// form of the step without the recurrence and sixteen copies of the tile end into the loop: 450 registers, 1700 accumulator
	// copies, + 1.9 % cycles on EVERY step).
	int frames_left = (int) a.tile_frames;                            // of the open tile, at the start of the next step
	uint32_t tiles_done = 0;
	KState kfin = ks;
	auto kslow = [&]<int U> () __attribute__ ((always_inline)) {
		const v2f (&x)[R] = xq[U];
		const int k = frames_left;                                    // 1 .. 16: frames of this step that belong to the open tile (wave-uniform)
#pragma unroll
		for (int n = 0; n < R; ++n) if (n < k) kstep (kc, ks, x[n]);
		if (live && tile >= fq) a.tile_power[(size_t) s * a.n_tiles + a.tile0 + tile] = a.gain_l * ks.sj.x + a.gain_r * ks.sj.y;
		ks.sj = 0;
		ks.z1 = scrub (ks.z1); ks.z2 = scrub (ks.z2); ks.z3 = scrub (ks.z3); ks.z4 = scrub (ks.z4);
		++tile;
		if (++tiles_done == a.n_main) kfin = ks;
#pragma unroll
		for (int n = 0; n < R; ++n) if (n >= k) kstep (kc, ks, x[n]);
		frames_left = (int) a.tile_frames - (R - k);
	};
	// the launch's last step where tiles are unaligned: the lanes of a last segment fetch their last_rows frames one by one
	auto last_frames = [&]<int U> () __attribute__ ((always_inline)) {
		const v2f* f = src + F0 + (int64_t) (n_steps - 1) * R;
		int rows = lastq ? last_rows : R;                             // frames of the step that are this lane's to read
		asm volatile ("" : "+v"(f), "+v"(rows));                      // (computed HERE, once: not sixteen addresses and masks kept across the main loop)
		v2f t[R];
#pragma unroll
		for (int n = 0; n < R; ++n) t[n] = f[min (n, rows - 1)];
#pragma unroll
		for (int n = 0; n < R; ++n) xq[U][n] = (n < rows && (!LEN || F0 + (int64_t) (n_steps - 1) * R + n < e_src)) ? t[n] : v2f{0.f, 0.f};
		maxabs.template operator()<U> ();                             // (the maxima computed a step early saw a stale line)
	};
	auto do_step = [&]<int U, bool PROD> () __attribute__ ((always_inline)) {
		if constexpr (!ALIGNED) if (cut && j == n_steps - 1) last_frames.template operator()<U> ();
		if constexpr (!EBU || ALIGNED) step.template operator()<U, PROD, EBU> ();
		else {
			const bool boundary = frames_left <= R;                   // wave-uniform
			KState at_start = ks;
			step.template operator()<U, PROD, true> ();
			// (the step's recurrence is needed HERE, whichever way the branch below goes: without this the compiler sinks all 176
			// operations out of the MFMA shadows they were placed in, into the branch that uses them — one lump behind the step)
			asm volatile ("" : "+v"(ks.z1), "+v"(ks.z2), "+v"(ks.z3), "+v"(ks.z4), "+v"(ks.sj));
			if (boundary) { ks = at_start; kslow.template operator()<U> (); }
			else frames_left -= R;
		}
	};

	// (the first three loads above were steps 0..2; step 0 has no products in front of it)
	lp -= R / 2;                                                      // `step` advances before it loads
	maxabs.template operator()<0> ();
	do_step.template operator()<0, false> ();
	while (j + 4 <= n_steps) {
		do_step.template operator()<1, true> ();
		do_step.template operator()<2, true> ();
		do_step.template operator()<3, true> ();
		do_step.template operator()<0, true> ();
	}
	if (j < n_steps) do_step.template operator()<1, true> ();
	if (j < n_steps) do_step.template operator()<2, true> ();
	if (j < n_steps) do_step.template operator()<3, true> ();
	if constexpr (LAZY) {
		// the products of the last step: dense, so all four blocks build their lo words first (once per launch)
		n_scr += 8;
		switch (n_steps & 3) {
		case 0:  complete.template operator()<0, true> (0xffu, j); break;
		case 1:  complete.template operator()<1, true> (0xffu, j); break;
		case 2:  complete.template operator()<2, true> (0xffu, j); break;
		default: complete.template operator()<3, true> (0xffu, j); break;
		}
	} else
	switch (n_steps & 3) {                                           // the products of the last step
	case 0:  products.template operator()<0> (); break;
	case 1:  products.template operator()<1> (); break;
	case 2:  products.template operator()<2> (); break;
	default: products.template operator()<3> (); break;
	}
	flush_pm ();
#ifdef MTR_SEG_PROF
	if (blockIdx.x == gridDim.x / 2 && lane == 0) for (int i = 0; i < 10; ++i) g_seg_prof[i] = sprof_[i];
#endif

	if (SCREEN && lane == 0 && a.seg_stats) { atomicAdd (&a.seg_stats[0], n_scr); atomicAdd (&a.seg_stats[1], n_fin); }
	if (live) {
		if (peak_ok) {
			atomicMax (&st->tp_call[0], __float_as_uint (fmaxf (pk0.x, pkf.x)));
			atomicMax (&st->tp_call[1], __float_as_uint (fmaxf (pk0.y, pkf.y)));
		}
		if (EBU && q == a.n_segs - 1 && (!LEN || a.ends[s] != 0)) {
			const KState& kf = ALIGNED ? ks : kfin;                       // (unaligned: the state at the lane's last tile end)
			st->kz[0] = kf.z1.x; st->kz[1] = kf.z1.y; st->kz[2] = kf.z2.x; st->kz[3] = kf.z2.y;
			st->kz[4] = kf.z3.x; st->kz[5] = kf.z3.y; st->kz[6] = kf.z4.x; st->kz[7] = kf.z4.y;
		}
	}
}

}  // namespace

size_t mtr_seg_lds_bytes (void) { return LDS_BYTES; }

#ifdef MTR_SEG_PROF
extern "C" int mtr_debug_seg_prof (unsigned long long* out)
{
	return hipMemcpyFromSymbol (out, HIP_SYMBOL (g_seg_prof), 10 * sizeof (unsigned long long)) == hipSuccess ? 0 : -1;
}
#endif

int mtr_launch_seg (bool ebu, const mtr_seg_args& a, uint32_t n_waves, void* stream)
{
	hipStream_t st = (hipStream_t) stream;
	const bool aligned = a.tile_frames % R == 0;
	if ((a.screen == 3u || a.screen == 4u) && a.ends) {
		// calls with per-stream ends stay on form 2: the LEN instantiations sit at their SGPR limit
		mtr_seg_args a2 = a;
		a2.screen = 2u;
		return mtr_launch_seg (ebu, a2, n_waves, stream);
	}
	// the six forms <SCREEN, LEN, LAZY, CORE>, each for the four (EBU, ALIGNED): 24 instantiations (an unaligned one: the same code but for the
	// launch's last step; EBU false: no tiles without Σ y²)
	const auto launch = [&] (auto EBU, auto ALIGNED) {
		const auto form = [&] (auto kernel) { hipLaunchKernelGGL (kernel, dim3 (n_waves), dim3 (64), LDS_BYTES, st, a); };
		if (a.screen == 4u)          form (k_seg<EBU.value, ALIGNED.value, true, false, true, true>);
		else if (a.screen == 3u)     form (k_seg<EBU.value, ALIGNED.value, true, false, true>);
		else if (a.ends && a.screen) form (k_seg<EBU.value, ALIGNED.value, true, true>);
		else if (a.ends)             form (k_seg<EBU.value, ALIGNED.value, false, true>);
		else if (a.screen)           form (k_seg<EBU.value, ALIGNED.value, true, false>);
		else                         form (k_seg<EBU.value, ALIGNED.value, false, false>);
	};
	if (ebu) { if (aligned) launch (std::true_type {}, std::true_type {}); else launch (std::true_type {}, std::false_type {}); }
	else     { if (aligned) launch (std::false_type {}, std::true_type {}); else launch (std::false_type {}, std::false_type {}); }
	return hipGetLastError () == hipSuccess ? 0 : -1;
}
